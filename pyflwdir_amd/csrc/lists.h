// lists.h — what the list-producing calls share (outlets.hip: outlet lists, streams.hip: segment lists): the downstream
// link under the three forms of a handle, the handle's own sequence on the device, the stable compaction by a mark, and
// the hand-over of a list to the caller.
#pragma once
#include <rocprim/device/device_select.hpp>

#include <algorithm>

#include "common.h"

int pfd_gen_graph_dev(pfd_raster *h, const u32 **ds, const u32 **seq);  // general.hip: orders the graph

// the downstream link under the three forms of a handle: valid(x), down(x) (own index for a pit)
struct DownD8 {
  const u8 *ncode;
  Geo g;
  __device__ __forceinline__ bool valid(u64 x) const { return ncode[x] != D8_MV; }
  __device__ __forceinline__ u64 down(u64 x) const { return d8_down(g, (u32)x, ncode[x]); }
};
struct DownWide {  // beyond 2^32 - 2 cells
  const u8 *ncode;
  i64 ncol;
  __device__ __forceinline__ bool valid(u64 x) const { return ncode[x] != D8_MV; }
  __device__ __forceinline__ u64 down(u64 x) const {
    const u32 code = ncode[x];
    if (!d8_is_dir(code)) return x;
    const int k = d8_slot(code);
    return (u64)((i64)x + (i64)d8_dr(k) * ncol + d8_dc(k));
  }
};
struct DownGen {  // general idxs_ds graph: 0xFFFFFFFF = nodata
  const u32 *ds;
  __device__ __forceinline__ bool valid(u64 x) const { return ds[x] != 0xFFFFFFFFu; }
  __device__ __forceinline__ u64 down(u64 x) const { return ds[x]; }
};

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

static inline u32 sweep_grid(u64 n) { return (u32)std::min<u64>((n + 255) / 256, 1u << 22); }

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
  size_t tb = 0;
  HIPCHK(rocprim::select(nullptr, tb, in, out, count_dev, (size_t)m, IsMarked{mark}, h->stream));
  DevBuf tmp;
  PFDCHK(tmp.alloc(std::max<size_t>(tb, 16)));
  HIPCHK(rocprim::select(tmp.p, tb, in, out, count_dev, (size_t)m, IsMarked{mark}, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (`tmp` is released on return)
  return PFD_OK;
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
