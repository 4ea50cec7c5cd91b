// walks.h — what the calls that walk along the links share (subgrid.hip: segment_*, window.hip: moving_*, path,
// subbasins_area.hip, upscale.hip), free of rocprim: the downstream link under the three forms of a handle, the opening
// checks of a D8-only whole-raster call, the device error word, the import of a caller's index list into 32-bit lanes and
// the two link functors of a walk.  lists.h adds what the list-producing calls need on top of it.
#pragma once
#include <algorithm>

#include "common.h"

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

static inline u32 sweep_grid(u64 n) { return (u32)std::min<u64>((n + 255) / 256, 1u << 22); }

// what a D8-only whole-raster call opens with: a usable handle, no general graph, no row block, 32-bit cell indices; the
// profiling segments of the previous call are dropped
static inline int pfd_begin_whole(pfd_raster *h, const char *what) {
  PFDCHK(pfd_check_handle(h));
  PFDCHK(pfd_reject_general(h, what));
  PFDCHK(pfd_require_whole(h, what));
  pfd_seg_clear(h);
  return PFD_OK;
}

// ---- the links of a walk -------------------------------------------------------------------------------------------
#define PFD_NOCELL 0xFFFFFFFFu  // "no cell" in a 32-bit lane: a missing list entry, no main upstream cell (a headwater)
template <class D>
struct NextDown {
  D d;
  __device__ __forceinline__ u32 operator()(u32 x) const { return (u32)d.down(x); }  // own index at a pit / nodata cell
};
struct NextUp {
  const u32 *us;
  __device__ __forceinline__ u32 operator()(u32 x) const { return us[x]; }  // PFD_NOCELL at a headwater
};

// ---- the device error word -----------------------------------------------------------------------------------------
// One u32 that the kernels of a call OR their findings into.  The three bits below mean the same in every call; a call's
// own findings start at WE_OWN and keep their messages in the call's file.
enum {
  WE_CAP = 1,      // a walk did not end within n steps
  WE_INPUT = 2,    // a list entry outside its range
  WE_INVERSE = 4,  // a main upstream cell that does not drain into its cell
  WE_OWN = 8
};
// how a family of calls words the shared findings: "<what>: <lists> lies outside the raster", "<what>: <walk>"
struct WalkErrText {
  const char *lists, *walk;
};
struct WalkErr {
  DevBuf buf;
  u32 *dev() { return buf.as<u32>(); }
  int init(pfd_raster *h) {
    PFDCHK(buf.alloc(sizeof(u32)));
    HIPCHK(hipMemsetAsync(buf.p, 0, sizeof(u32), h->stream));
    return PFD_OK;
  }
  // waits for the stream; PFD_EINVAL + message for a shared bit, else *own = the caller's own bits (0: nothing found)
  int check(pfd_raster *h, const char *what, const WalkErrText &t, u32 *own = nullptr) {
    u32 e = 0;
    HIPCHK(hipMemcpyAsync(&e, buf.p, sizeof(e), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (own) *own = 0;
    if (e & WE_INPUT) {
      pfd_set_error("%s: %s lies outside the raster", what, t.lists);
      return PFD_EINVAL;
    }
    if (e & WE_INVERSE) {
      pfd_set_error("%s: idxs_us_main holds a cell that does not drain into the cell it is listed for", what);
      return PFD_EINVAL;
    }
    if (e & WE_CAP) {
      pfd_set_error("%s: %s", what, t.walk);
      return PFD_EINVAL;
    }
    if (own) *own = e & ~(u32)(WE_OWN - 1);
    return PFD_OK;
  }
};

// ---- the import of a caller's index list ---------------------------------------------------------------------------
// Which entries a list may hold, next to "missing" (the dtype's -1) and "inside [0, limit)".  The rules differ because the
// walks rely on the list to different degrees, and each call keeps the rule it was written with:
//   IMPORT_OUTLETS  subgrid's outlet lists (segment_*): ANY negative value is a missing outlet, as in the reference, whose
//                   loops skip `idx0 < 0`;
//   IMPORT_ANY      no further check.  segment_* and path(direction="up") only FOLLOW idxs_us_main, like the reference's
//                   loops: a wrong entry gives the reference's wrong answer, and the step cap ends a cycle.  upscale_error
//                   takes lists of coarse cells, for which there is no link to check;
//   IMPORT_DRAINS   down(entry) == cell.  moving_average / moving_median walk up the list and come back DOWN the D8
//                   links (win_visit): only an inverse of the links brings them back to the centre.  A pit listed as its
//                   own main upstream cell passes (down(pit) == pit); the walk up then runs into its bound of n steps;
//   IMPORT_STRICT   down(entry) == cell, entry != cell and entry is no nodata cell.  subbasins_area compares the entry
//                   with the decoded upstream neighbours of the cell, which are other, valid cells by construction.
enum { IMPORT_OUTLETS, IMPORT_ANY, IMPORT_DRAINS, IMPORT_STRICT };
// out[j] = in[j] as a 32-bit lane (PFD_NOCELL: missing).  An outlet list (IMPORT_OUTLETS) also raises flag[cell] of every
// listed cell; the other rules take no flag.  (The kernel runs at the latency of its one load and one store per lane: a
// count in 32 bits and no argument fetched between the two keep a lane as short as it was in each call's own kernel.)
template <class I, int CHECK>
__global__ void __launch_bounds__(256) k_import_cells(const I *__restrict__ in, u32 count, u64 limit, const DownD8 d,
                                                      u32 *__restrict__ out, u8 *__restrict__ flag, u32 *__restrict__ err) {
  const u32 j = blockIdx.x * 256u + threadIdx.x;
  if (j >= count) return;
  const I v = in[j];
  u32 o = PFD_NOCELL;
  if (!(v == (I)-1 || (CHECK == IMPORT_OUTLETS && (i64)v < 0))) {
    if ((i64)v < 0 || (u64)v >= limit) {
      atomicOr(err, (u32)WE_INPUT);
    } else {
      o = (u32)v;
      if (CHECK == IMPORT_DRAINS && (u32)d.down(o) != j) atomicOr(err, (u32)WE_INVERSE);
      if (CHECK == IMPORT_STRICT && (o == j || !d.valid(o) || (u32)d.down(o) != j)) atomicOr(err, (u32)WE_INVERSE);
      if (CHECK == IMPORT_OUTLETS) flag[o] = 1;
    }
  }
  out[j] = o;
}
// count entries (fewer than 2^32) of the caller's index dtype; `flag`: the outlet flags of IMPORT_OUTLETS, else nullptr
template <int CHECK>
static int pfd_import_cells(pfd_raster *h, const char *what, int idx_dtype, const void *in, u64 count, u64 limit, u32 *out,
                            u8 *flag, u32 *err) {
  if ((CHECK == IMPORT_OUTLETS) != (flag != nullptr) || count >= 0xFFFFFFFFull) {
    pfd_set_error("%s: internal: list import with %llu entries, flags %s", what, (unsigned long long)count, flag ? "given" : "missing");
    return PFD_EINVAL;
  }
  return pfd_dispatch_idx(idx_dtype, what, [&](auto itag) -> int {
    typedef typename decltype(itag)::type I;
    k_import_cells<I, CHECK><<<cdiv_u32(count, 256), 256, 0, h->stream>>>((const I *)in, (u32)count, limit,
                                                                         DownD8{h->ncode, h->geo}, out, flag, err);
    KCHK();
    return PFD_OK;
  });
}
