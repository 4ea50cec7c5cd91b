// fill.h — the per-cell rules of FlwdirRaster.fillnodata (reference pyflwdir/flwdir.py:360-392), shared by the D8
// engines (sweeps.hip: FillDown / FillUp) and the general idxs_ds engine (general.hip).
//
//   core.fillnodata_upstream   (core.py:120-146)  direction "up":   a nodata cell takes the value of its downstream cell
//                                                 when that is not nodata — the first valid value on its path
//   core.fillnodata_downstream (core.py:149-188)  direction "down": a nodata cell folds the values of its upstream cells
//                                                 that are not nodata, in the serial loop's order (descending linear
//                                                 index): the first one is taken, the others merged with max / min / +=
// All comparisons are by value in the payload dtype, like numpy's.  has_nodata == 0 (NaN nodata, or one no element of
// the dtype can equal): nothing is nodata and the result is the payload.
#pragma once
#include "common.h"

#include "../../include/pfd.h"

__device__ __forceinline__ i32 fill_add(i32 a, i32 b) { return (i32)((u32)a + (u32)b); }
__device__ __forceinline__ i64 fill_add(i64 a, i64 b) { return (i64)((u64)a + (u64)b); }
__device__ __forceinline__ u32 fill_add(u32 a, u32 b) { return a + b; }
__device__ __forceinline__ u64 fill_add(u64 a, u64 b) { return a + b; }
__device__ __forceinline__ float fill_add(float a, float b) { return a + b; }
__device__ __forceinline__ double fill_add(double a, double b) { return a + b; }
// int8 / int16 / uint8 / uint16 payloads travel in int32 lanes: a sum wraps in the narrow dtype (sh = 32 - bits; uns:
// zero- instead of sign-extended), so that its "equals nodata" test sees the narrow value like the reference's
__device__ __forceinline__ i32 fill_wrap(i32 v, u32 sh, u32 uns) {
  const u32 u = (u32)v << sh;
  return uns ? (i32)(u >> sh) : ((i32)u >> sh);
}
template <class T>
__device__ __forceinline__ T fill_wrap(T v, u32, u32) { return v; }

template <class T>
struct FillRule {
  T nodata;
  int has_nodata;
  int how;  // PFD_FILL_MAX / PFD_FILL_MIN / PFD_FILL_SUM (direction "down" only)
  u32 nsh, nuns;
  __device__ __forceinline__ bool isnd(T v) const { return has_nodata && v == nodata; }
  // Python's max(v, s) keeps v unless s > v (v: the upstream cell, s: the running value); min the same with <
  __device__ __forceinline__ T merge(T v, T s) const {
    if (how == PFD_FILL_MAX) return s > v ? s : v;
    if (how == PFD_FILL_MIN) return s < v ? s : v;
    return fill_wrap(fill_add(s, v), nsh, nuns);
  }
  // one upstream value v into the running value s of a nodata cell (core.py:177-187); a running SUM that comes out
  // equal to nodata is replaced by the next value, like in the serial loop
  __device__ __forceinline__ T step(T s, T v) const { return isnd(v) ? s : (isnd(s) ? v : merge(v, s)); }
  // direction "up" (core.py:142-145): own value, given the final value pv of the downstream cell
  __device__ __forceinline__ T up(T own, T pv) const { return (isnd(own) && !isnd(pv)) ? pv : own; }
};

// payload code -> the lane type of the kernels and its rule.  Direction "up" only compares for equality: unsigned
// payloads run as their signed view there; "down" compares (max / min) in the payload's own order.
template <class FD, class FU>
static int fill_dispatch(int dtype, bool down, int64_t nodata_i, double nodata_f, int has_nodata, int how,
                         const char *what, FD fdown, FU fup) {
  auto narrow = [&](u32 sh, u32 uns) {
    const FillRule<i32> r{(i32)nodata_i, has_nodata, how, sh, uns};
    return down ? fdown(r) : fup(r);
  };
  switch (dtype) {
    case PFD_I32: return narrow(0u, 0u);
    case PFD_I8: return narrow(24u, 0u);
    case PFD_U8: return narrow(24u, 1u);
    case PFD_I16: return narrow(16u, 0u);
    case PFD_U16: return narrow(16u, 1u);
    case PFD_U32:
      return down ? fdown(FillRule<u32>{(u32)nodata_i, has_nodata, how, 0u, 0u})
                  : fup(FillRule<i32>{(i32)nodata_i, has_nodata, how, 0u, 0u});
    case PFD_I64: {
      const FillRule<i64> r{(i64)nodata_i, has_nodata, how, 0u, 0u};
      return down ? fdown(r) : fup(r);
    }
    case PFD_U64:
      return down ? fdown(FillRule<u64>{(u64)nodata_i, has_nodata, how, 0u, 0u})
                  : fup(FillRule<i64>{(i64)nodata_i, has_nodata, how, 0u, 0u});
    case PFD_F32: {
      const FillRule<float> r{(float)nodata_f, has_nodata, how, 0u, 0u};
      return down ? fdown(r) : fup(r);
    }
    case PFD_F64: {
      const FillRule<double> r{nodata_f, has_nodata, how, 0u, 0u};
      return down ? fdown(r) : fup(r);
    }
    default:
      pfd_set_error("%s: unsupported payload dtype code %d", what, dtype);
      return PFD_EUNSUPPORTED;
  }
}
