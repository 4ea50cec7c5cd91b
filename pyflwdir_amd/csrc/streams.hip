// streams.hip — stream segments: streams.streams (reference pyflwdir/streams.py:132-188; FlwdirRaster.streams
// pyflwdir.py:894-974) as a CSR triple (offsets, indices, pit flags) on the device.
//
// The reference walks seq[::-1] with a `done` array.  In closed form, with inm(x) = mask[x] (true without a mask),
// nup = core.upstream_count(idxs_ds, mask) and W(x) = "some walk stepped from x":
//   done(x)  = nup[x] <= 1 and OR over the upstream neighbours y of W(y)
//   W(x)     = inm(x) or done(x)
//   start(x) = inm(x) and not done(x)
// A segment starts at every start cell of the sequence, in reversed sequence order, follows the downstream links (through
// cells outside the mask as well) and ends with the first arrived-at cell with nup > 1, or at a pit.
//   nup      the existing upstream count (pfd_upstream_count: k_upstream_count / the general engine's), device memory;
//   W        a mask that is closed downstream (every masked non-pit cell drains into a masked cell; no mask at all) has
//            W = inm; any other mask runs ONE existing sweep: fillnodata(payload, nodata 0, "down", "max") == 2 with
//            payload = 2 inside the mask, 1 at nup > 1 (a walk stops there: W does not pass), else 0;
//   flags    one byte per cell: bit 0 W, bit 1 nup > 1 (a walk stops on arrival), bit 2 start.  "Any upstream neighbour
//            with W" is a scatter of 1 into any[down(y)] — all writers store the same byte;
//   list     the sequence compacted by the start bit (rocprim select), read backwards: cells on or above a cycle are not
//            in the sequence and never start a segment, and no walk from a sequence cell reaches them;
//   measure  one thread per segment walks from its start, one flag byte per step: length, ended-in-a-pit;
//   offsets  exclusive scan of the lengths;
//   fill     the same walk again, writing the cells at the segment's offset
//            (these three, the room check and the hand-over are pfd_ragged_tail of lists.h, given the two walks).
// The `[p, p]` entries after a segment that ends in a pit and the max_len pieces are O(segments) slicing of this triple
// and stay with the caller (pyflwdir_amd/raster.py).
#include <algorithm>

#include "common.h"
#include "lists.h"

namespace {

enum { F_W = 1, F_STOP = 2, F_START = 4 };

// *open = 1 if a masked cell drains into a cell outside the mask
template <class D>
__global__ void __launch_bounds__(256) k_mask_open(const D d, u32 n, const u8 *__restrict__ mask, u32 *__restrict__ open) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  bool o = false;
  if (x < n && d.valid(x) && mask[x]) o = !mask[d.down(x)];
  if (__ballot(o) && (threadIdx.x & 63u) == 0) *open = 1u;
}
// the payload of the sweep that carries W through the cells outside the mask
__global__ void __launch_bounds__(256) k_w_payload(u32 n, const u8 *__restrict__ mask, const int8_t *__restrict__ nup,
                                                   i32 *__restrict__ pay) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x < n) pay[x] = mask[x] ? 2 : (nup[x] > 1 ? 1 : 0);
}
// W(x): from the sweep, else the mask, else every cell
__device__ __forceinline__ bool w_of(u32 x, const u8 *mask, const i32 *wfill) {
  return wfill ? wfill[x] == 2 : (mask ? mask[x] != 0 : true);
}
template <class D>
__global__ void __launch_bounds__(256) k_any_up(const D d, u32 n, const u8 *__restrict__ mask, const i32 *__restrict__ wfill,
                                                u8 *__restrict__ any) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n || !d.valid(x) || !w_of(x, mask, wfill)) return;
  const u32 y = (u32)d.down(x);
  if (y != x) any[y] = 1;
}
// the flag byte; *count += start cells (one atomic per wave that holds any)
template <class D>
__global__ void __launch_bounds__(256) k_flags(const D d, u32 n, const u8 *__restrict__ mask, const i32 *__restrict__ wfill,
                                               const int8_t *__restrict__ nup, const u8 *__restrict__ any, u8 *__restrict__ flag,
                                               unsigned long long *__restrict__ count) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  u32 f = 0;
  if (x < n && d.valid(x)) {
    const bool inm = mask ? mask[x] != 0 : true;
    const int up = nup[x];
    if (w_of(x, mask, wfill)) f |= F_W;
    if (up > 1) f |= F_STOP;
    if (inm && !(up <= 1 && any[x])) f |= F_START;
  }
  if (x < n) flag[x] = (u8)f;
  const u64 b = __ballot((f & F_START) != 0);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}
struct IsStart {
  const u8 *flag;
  __host__ __device__ bool operator()(const u32 &x) const { return (flag[x] & F_START) != 0; }
};
// segment j starts at sel[k - 1 - j] (reversed sequence order).  FILL = false: its length and pit flag; FILL = true:
// its cells at off[j]
template <bool FILL, class D, class O>
__global__ void __launch_bounds__(256) k_walk(const D d, const u32 *__restrict__ sel, u64 k, const u8 *__restrict__ flag,
                                              i64 *__restrict__ len, u8 *__restrict__ pit, const i64 *__restrict__ off,
                                              O *__restrict__ out) {
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  if (j >= k) return;
  u32 x = sel[k - 1 - j];
  i64 l = 1;
  bool p = false;
  O *o = FILL ? out + off[j] : nullptr;
  if (FILL) o[0] = (O)x;
  for (;;) {
    const u32 y = (u32)d.down(x);
    if (y == x) {
      p = true;
      break;
    }
    if (FILL) o[l] = (O)y;
    ++l;
    if (flag[y] & F_STOP) break;
    x = y;
  }
  if (!FILL) len[j] = l, pit[j] = p ? 1 : 0;
}

template <class D>
static int streams_run(pfd_raster *h, const D &d, const u32 *seq, u64 m, const u8 *mask, const int8_t *nup, int idx_dtype,
                       void *idxs_out, i64 cap_idxs, i64 *offsets_out, u8 *pit_out, i64 cap_segs, i64 *n_out, int memspace) {
  const u32 n = h->geo.n, grid = cdiv_u32(n, 256);
  DevBuf cnt, wfill;
  PFDCHK(cnt.alloc(4 * sizeof(unsigned long long)));
  unsigned long long *c = cnt.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(unsigned long long), h->stream));
  if (mask) {
    pfd_seg_begin(h, "streams_closed_check");
    k_mask_open<D><<<grid, 256, 0, h->stream>>>(d, n, mask, (u32 *)(c + 1));
    KCHK();
    pfd_seg_end(h, 1);
    u32 open = 0;
    HIPCHK(hipMemcpyAsync(&open, c + 1, sizeof(open), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (open) {  // W reaches beyond the mask: one down-fill of the payload (the segments of the fill follow ours)
      DevBuf pay;
      PFDCHK(pay.alloc((size_t)n * sizeof(i32)));
      PFDCHK(wfill.alloc((size_t)n * sizeof(i32)));
      pfd_seg_begin(h, "streams_w_payload");
      k_w_payload<<<grid, 256, 0, h->stream>>>(n, mask, nup, pay.as<i32>());
      KCHK();
      pfd_seg_end(h, 1);
      PFDCHK(pfd_fillnodata_impl(h, PFD_I32, pay.p, 0, 0.0, 1, PFD_DOWN, PFD_FILL_MAX, wfill.p, PFD_DEVICE, false));
    }
  }
  const i32 *wf = wfill.as<i32>();
  DevBuf any, flag;
  PFDCHK(any.alloc((size_t)n));
  PFDCHK(flag.alloc((size_t)n));
  pfd_seg_begin(h, "streams_flags");
  HIPCHK(hipMemsetAsync(any.p, 0, (size_t)n, h->stream));
  k_any_up<D><<<grid, 256, 0, h->stream>>>(d, n, mask, wf, any.as<u8>());
  k_flags<D><<<grid, 256, 0, h->stream>>>(d, n, mask, wf, nup, any.as<u8>(), flag.as<u8>(), c);
  KCHK();
  pfd_seg_end(h, 3);
  unsigned long long starts = 0, kk = 0;
  HIPCHK(hipMemcpyAsync(&starts, c, sizeof(starts), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  n_out[0] = n_out[1] = 0;
  if (!starts || !m) return give_empty(h, offsets_out, memspace);
  // (cells off the sequence may carry the start bit: `starts` is room enough, the selection counts the segments)
  DevBuf sel, tmp;
  PFDCHK(sel.alloc((size_t)starts * sizeof(u32)));
  pfd_seg_begin(h, "streams_list");
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::select(p, b, seq, sel.as<u32>(), c + 2, (size_t)m, IsStart{flag.as<u8>()}, h->stream);
  }));
  pfd_seg_end(h, 1);
  HIPCHK(hipMemcpyAsync(&kk, c + 2, sizeof(kk), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const u64 k = (u64)kk;
  DevBuf pit;
  PFDCHK(pit.alloc(std::max<size_t>((size_t)k, 1)));
  const u32 wgrid = cdiv_u32(k, 256);
  const RaggedSegs segs = {"streams_walk_measure", "streams_offsets", "streams_walk_fill", "streams indices"};
  const RaggedOut ro = {idx_dtype, idxs_out, cap_idxs, offsets_out, cap_segs, memspace};
  i64 total = 0;
  bool given = false;
  PFDCHK(pfd_ragged_tail(
      h, segs, k, ro,
      [&](i64 *len) -> int {
        k_walk<false, D, i32><<<wgrid, 256, 0, h->stream>>>(d, sel.as<u32>(), k, flag.as<u8>(), len, pit.as<u8>(), nullptr, nullptr);
        KCHK();
        return PFD_OK;
      },
      [] { return PFD_OK; },  // (no error word: a walk from a cell of the sequence ends at a pit)
      [&](auto itag, const i64 *off, auto *dst) -> int {
        typedef typename decltype(itag)::type I;
        k_walk<true, D, I><<<wgrid, 256, 0, h->stream>>>(d, sel.as<u32>(), k, flag.as<u8>(), nullptr, nullptr, off, dst);
        KCHK();
        return PFD_OK;
      },
      &total, &given));
  n_out[0] = (i64)k, n_out[1] = total;
  if (given) PFDCHK(give_list(h, pit.p, (size_t)k, pit_out, memspace));
  return PFD_OK;
}

}  // namespace

extern "C" int pfd_streams(pfd_raster *h, const uint8_t *mask, int idx_dtype, void *idxs_out, int64_t cap_idxs,
                           int64_t *offsets_out, uint8_t *pit_out, int64_t cap_segs, int64_t n_out[2], int memspace) {
  PFDCHK(pfd_check_handle(h));
  PFDCHK(pfd_require_unblocked(h, "streams"));
  if (!n_out || cap_idxs < 0 || cap_segs < 0 || (cap_idxs > 0 && !idxs_out) || (cap_segs > 0 && (!offsets_out || !pit_out))) {
    pfd_set_error("streams: bad arguments (NULL pointer, cap_idxs=%lld, cap_segs=%lld)", (long long)cap_idxs,
                  (long long)cap_segs);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("streams: unsupported index dtype code %d", idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  if (!h->gen && pfd_wide_cells(h)) {
    pfd_set_error("streams: stream segments are limited to rasters of at most 4294967294 (2^32 - 2) cells; this one has "
                  "%lld (or runs with 64-bit cell indices)", (long long)h->n);
    return PFD_EUNSUPPORTED;
  }
  pfd_seg_clear(h);
  InArg mk;
  PFDCHK(mk.bind(mask, (size_t)h->n, memspace, h->stream));
  DevBuf nup;
  PFDCHK(nup.alloc((size_t)h->n));
  pfd_seg_begin(h, "streams_nup");
  PFDCHK(pfd_upstream_count(h, (const u8 *)mk.dev, nup.as<int8_t>(), PFD_DEVICE));
  pfd_seg_end(h, 1);
  // (a raster with 64-bit cells was refused above: the sequence is one of 32-bit cells)
  return pfd_with_graph(h, [&](auto d, auto seq, u64 m) -> int {
    if constexpr (std::is_same<decltype(seq), const u32 *>::value)
      return streams_run(h, d, seq, m, (const u8 *)mk.dev, nup.as<int8_t>(), idx_dtype, idxs_out, cap_idxs, offsets_out, pit_out,
                         cap_segs, n_out, memspace);
    else
      return PFD_EUNSUPPORTED;
  });
}
