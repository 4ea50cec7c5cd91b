// lists.h — the frame the list-producing calls stand on (outlets.hip, streams.hip, basins_ext.hip, subbasins_area.hip,
// window.hip: path, subgrid.hip; walks.h holds the rocprim-free part): the argument check of a call that returns a list, the
// handle's links and sequence on the device (pfd_with_graph, pfd_with_links),
// the stable compaction by a mark, the small list kernels, the hand-over of a list to the caller and the tail of a call
// that returns ragged lists (pfd_ragged_tail).
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>

#include "common.h"
#include "walks.h"

int pfd_gen_graph_dev(pfd_raster *h, const u32 **ds, const u32 **seq);  // general.hip: orders the graph

// what a call that returns a list of cells checks first: `data` the per-cell input, `list_out` with room for `cap` entries
static inline int pfd_check_list_args(pfd_raster *h, const char *what, const void *data, int idx_dtype, const void *list_out,
                                      i64 cap, const i64 *k_out) {
  PFDCHK(pfd_check_handle(h));
  PFDCHK(pfd_require_unblocked(h, what));
  if (!data || !k_out || cap < 0 || (cap > 0 && !list_out)) {
    pfd_set_error("%s: bad arguments (NULL pointer, cap=%lld)", what, (long long)cap);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("%s: unsupported index dtype code %d", what, idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  if (h->n > 4294967294ll && idx_dtype != PFD_I64) {
    pfd_set_error("%s of a raster of %lld cells needs the int64 index dtype (PFD_I64)", what, (long long)h->n);
    return PFD_EINVAL;
  }
  pfd_seg_clear(h);
  return PFD_OK;
}

// k values from HBM into the caller's list (a host list: counted as a download of the call)
static inline int give_list(pfd_raster *h, const void *dev, size_t bytes, void *out, int memspace) {
  if (!bytes) return PFD_OK;
  if (memspace == PFD_DEVICE) {
    HIPCHK(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PFD_OK;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  const double t0 = pfd_now_ms();
  HIPCHK(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  PfdTransfer &t = pfd_transfer();
  t.d2h_bytes += (double)bytes, t.d2h_ms += pfd_now_ms() - t0, t.host_results += 1;
  return PFD_OK;
}

// f(d): the handle's downstream links alone — nothing is ordered for it
template <class F>
static int pfd_with_links(pfd_raster *h, F f) {
  if (h->gen) {
    const u32 *ds = nullptr, *seq = nullptr;
    PFDCHK(pfd_gen_graph_dev(h, &ds, &seq));
    return f(DownGen{ds});
  }
  if (pfd_wide_cells(h)) return f(DownWide{h->ncode, h->ncol});
  return f(DownD8{h->ncode, h->geo});
}
// f(d, seq, m): the handle's downstream links and its own sequence (core.idxs_seq order; the installed order of a general
// graph) of m cells, in HBM for the time of the call — 32-bit cells, the 64-bit queue of order64.hip, a general graph
template <class F>
static int pfd_with_graph(pfd_raster *h, F f) {
  if (h->gen) {
    const u32 *ds = nullptr, *seq = nullptr;
    PFDCHK(pfd_gen_graph_dev(h, &ds, &seq));
    return f(DownGen{ds}, seq, (u64)h->n_seq);
  }
  if (pfd_wide_cells(h)) {
    DevBuf q;
    u64 nseq = 0;
    PFDCHK(pfd_wide_seq_dev(h, q, &nseq));
    return f(DownWide{h->ncode, h->ncol}, (const u64 *)q.p, nseq);
  }
  DevBuf oseq;
  PFDCHK(pfd_exact_seq_dev(h, oseq));
  return f(DownD8{h->ncode, h->geo}, (const u32 *)oseq.p, (u64)h->n_seq);
}

static inline int read_count(pfd_raster *h, const unsigned long long *dev, u64 *out) {
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, dev, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *out = (u64)v;
  return PFD_OK;
}

struct IsMarked {
  const u8 *mark;
  template <class I>
  __host__ __device__ bool operator()(const I &x) const { return mark[x] != 0; }
};
// compaction of the cells [0, n) / of the sequence by the mark; `out` has room for what is marked
template <class In, class Out>
static int select_marked(pfd_raster *h, In in, u64 m, const u8 *mark, Out *out, unsigned long long *count_dev) {
  DevBuf tmp;
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::select(p, b, in, out, count_dev, (size_t)m, IsMarked{mark}, h->stream);
  }));
  HIPCHK(hipStreamSynchronize(h->stream));  // (`tmp` is released on return)
  return PFD_OK;
}

// a compacted list as the caller sees it: 64-bit indices, `reversed` for the loops of the reference that walk seq[::-1];
// ids, if given: the numbers 1..k of the entries
template <class I>
__global__ void __launch_bounds__(256) k_number(const I *__restrict__ sel, u64 k, bool reversed, i64 *__restrict__ idx,
                                                u32 *__restrict__ ids) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  idx[i] = (i64)sel[reversed ? k - 1 - i : i];
  if (ids) ids[i] = (u32)(i + 1);
}
template <class T>
__global__ void __launch_bounds__(256) k_gather(const i64 *__restrict__ idx, u64 k, const T *__restrict__ v, T *__restrict__ out) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < k) out[i] = v[idx[i]];
}

template <class O>
__global__ void __launch_bounds__(256) k_export_i64(const i64 *__restrict__ idx, u64 k, O *__restrict__ out) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < k) out[i] = (O)idx[i];
}
// a list of 64-bit cell indices in the caller's index dtype
static inline int give_idxs(pfd_raster *h, const i64 *idx, u64 k, int idx_dtype, void *out, int memspace) {
  if (!k) return PFD_OK;
  if (idx_dtype == PFD_I64) return give_list(h, idx, (size_t)k * 8, out, memspace);
  return pfd_dispatch_idx(idx_dtype, "outlet indices", [&](auto itag) -> int {
    typedef typename decltype(itag)::type I;
    DevBuf tmp;
    PFDCHK(tmp.alloc((size_t)k * sizeof(I)));
    k_export_i64<I><<<cdiv_u32(k, 256), 256, 0, h->stream>>>(idx, k, tmp.as<I>());
    KCHK();
    return give_list(h, tmp.p, (size_t)k * sizeof(I), out, memspace);
  });
}

// ---- ragged lists: k lists of cells as (offsets[k + 1], indices[total]) ----------------------------------------------
// no list at all: the offsets are the single 0 (when the caller gave room for offsets)
static inline int give_empty(pfd_raster *h, i64 *offsets_out, int memspace) {
  if (offsets_out) {
    if (memspace == PFD_DEVICE) HIPCHK(hipMemsetAsync(offsets_out, 0, sizeof(i64), h->stream));
    else offsets_out[0] = 0;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}
struct RaggedOut {  // where the caller wants the lists, and how much room there is
  int idx_dtype;
  void *idxs;
  i64 cap_idxs;
  i64 *offsets;
  i64 cap_lists;
  int memspace;
};
struct RaggedSegs {  // the call's names: its three profiling segments, and what it calls its indices
  const char *count, *offsets, *fill, *indices;
};
// What a call that returns k ragged lists ends with.  count(len) launches the walk that writes the k lengths; checked()
// is the call's look at its error word before the lengths are used; fill(itag, off, dst) launches the same walk again,
// writing list i at dst + off[i] in the index type of itag.  *total = the length of all lists, also when they do not fit
// the caller's room; *given = the lists were handed over, and the caller's side arrays (one value per list) may follow.
template <class Count, class Checked, class Fill>
static int pfd_ragged_tail(pfd_raster *h, const RaggedSegs &sg, u64 k, const RaggedOut &o, Count count, Checked checked,
                           Fill fill, i64 *total, bool *given) {
  *total = 0, *given = false;
  if (!k) return give_empty(h, o.offsets, o.memspace);
  DevBuf off, tmp;
  PFDCHK(off.alloc((size_t)(k + 1) * sizeof(i64)));
  i64 *const offs = off.as<i64>();
  pfd_seg_begin(h, sg.count);
  HIPCHK(hipMemsetAsync(offs + k, 0, sizeof(i64), h->stream));
  PFDCHK(count(offs));
  pfd_seg_end(h, 1);
  PFDCHK(checked());
  pfd_seg_begin(h, sg.offsets);
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::exclusive_scan(p, b, offs, offs, (i64)0, (size_t)(k + 1), rocprim::plus<i64>(), h->stream);
  }));
  pfd_seg_end(h, 1);
  HIPCHK(hipMemcpyAsync(total, offs + k, sizeof(i64), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if ((i64)k > o.cap_lists || *total > o.cap_idxs) return PFD_OK;
  PFDCHK(pfd_dispatch_idx(o.idx_dtype, sg.indices, [&](auto itag) -> int {
    typedef typename decltype(itag)::type I;
    DevBuf stage;
    I *dst = (I *)o.idxs;
    if (o.memspace != PFD_DEVICE) {
      PFDCHK(stage.alloc((size_t)*total * sizeof(I)));
      dst = stage.as<I>();
    }
    pfd_seg_begin(h, sg.fill);
    PFDCHK(fill(itag, (const i64 *)offs, dst));
    pfd_seg_end(h, 1);
    if (o.memspace != PFD_DEVICE) PFDCHK(give_list(h, stage.p, (size_t)*total * sizeof(I), o.idxs, o.memspace));
    else HIPCHK(hipStreamSynchronize(h->stream));
    return PFD_OK;
  }));
  PFDCHK(give_list(h, off.p, (size_t)(k + 1) * sizeof(i64), o.offsets, o.memspace));
  *given = true;
  return PFD_OK;
}
