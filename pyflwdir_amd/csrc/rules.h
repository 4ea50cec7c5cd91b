// rules.h — the per-cell arithmetic of the sweeps, stated once for the three engines that run it: the level engine and
// the exact-order engine of a D8 raster (sweeps.hip, exact_sweep.h) and the general idxs_ds engine (general.hip); the
// verify kernels (checks.hip) compute their expected values through the same rules.  The bit-identity with the
// reference's serial loops rests on these few lines: operand order, the type an addition or difference is taken in,
// and which operands are tested against nodata.  Graph-agnostic: operands come in as values (fill.h holds the rules
// of fillnodata in the same shape).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// payload arithmetic: integers wrap like numba's fixed-width ints, floats are plain IEEE adds
// ---------------------------------------------------------------------------------------------
template <class T> struct Num;
// neutral(): x with add(x, y) == y bit for bit, for every y (-0.0 for floats: +0.0 would turn a -0.0 into +0.0)
template <> struct Num<i32> {
  static __device__ __forceinline__ i32 neutral() { return 0; }
  static __device__ __forceinline__ i32 add(i32 a, i32 b) { return (i32)((u32)a + (u32)b); }
};
template <> struct Num<i64> {
  static __device__ __forceinline__ i64 neutral() { return 0; }
  static __device__ __forceinline__ i64 add(i64 a, i64 b) { return (i64)((u64)a + (u64)b); }
};
template <> struct Num<float> {
  static __device__ __forceinline__ float neutral() { return -0.0f; }
  static __device__ __forceinline__ float add(float a, float b) { return a + b; }
};
template <> struct Num<double> {
  static __device__ __forceinline__ double neutral() { return -0.0; }
  static __device__ __forceinline__ double add(double a, double b) { return a + b; }
};

// streams.accuflux / accuflux_ds (pyflwdir/streams.py:15-70): add unless either operand is nodata.  The speculative
// folds of the exact-order engine use the plain Num<T>::add wherever special() is false.
template <class T>
struct AccuRule {
  T nodata;
  int has_nodata;
  // the accumulator after the operand a; acc is the running value of the serial loop's downstream cell
  // (branch-free: runs on the serial critical path)
  __device__ __forceinline__ T join(T acc, T a) const {
    const T sum = Num<T>::add(acc, a);
    const bool ok = !has_nodata || (acc != nodata && a != nodata);
    return ok ? sum : acc;
  }
  // the same value, written as a branch: the form the level kernels and the down-sweeps were tuned with (the select form
  // costs k_sweep_up<int64> and k_xtrunk_dscan<float> a wave of occupancy)
  __device__ __forceinline__ T join_br(T acc, T a) const {
    if (!has_nodata || (acc != nodata && a != nodata)) acc = Num<T>::add(acc, a);
    return acc;
  }
  __device__ __forceinline__ bool special(T t, T e) const { return has_nodata && ((t == nodata) | (e == nodata)); }
};

// streams.strahler_order (pyflwdir/streams.py:252-268), order-independent closed form: among the upstream cells inside
// the mask let m be the largest order and cnt the number of cells that hold it
struct StrahlerRule {
  static __device__ __forceinline__ void join(u32 v, u32 &m, u32 &cnt) {
    if (v > m) {
      m = v;
      cnt = 1;
    } else if (v == m) {
      ++cnt;
    }
  }
  // own: the order of a headwater (1 inside the mask, 0 outside)
  static __device__ __forceinline__ u32 finish(u32 m, u32 cnt, u32 own) { return cnt == 0 ? own : (cnt >= 2 ? m + 1 : m); }
};

// dem.height_above_nearest_drain (pyflwdir/dem.py:299-330): the difference is taken in the elevation dtype
// (dem.py:328), widened, and added to the downstream cell's height; a drain cell is 0
template <class E>
struct HandRule {
  static __device__ __forceinline__ E dz(E ex, E ep) { return ex - ep; }
  static __device__ __forceinline__ double root(bool is_drain, E dz) { return is_drain ? 0.0 : 0.0 + (double)dz; }
  static __device__ __forceinline__ double fold(bool is_drain, E dz, double pv) { return is_drain ? 0.0 : pv + (double)dz; }
  static __device__ __forceinline__ double fold_fast(E dz, double pv) { return pv + (double)dz; }  // no drain cell
};

// streams.stream_order (pyflwdir/streams.py:191-225): uint8 arithmetic like the reference; flag = 1 on a tributary at
// a confluence; 0 outside the mask, 1 at a pit
struct ClassicRule {
  static __device__ __forceinline__ u32 root(bool outside) { return outside ? 0u : 1u; }
  static __device__ __forceinline__ u32 fold(bool outside, u32 flag, u32 pv) { return outside ? 0u : ((pv + flag) & 0xFFu); }
};

// streams.stream_distance (pyflwdir/streams.py:272-315): int32 cell counts or float32 lengths; reset: a pit or a cell
// inside the mask, where the distance restarts; real: lengths (float32 arithmetic, step = the cell's step length), else cells
template <class T>
struct DistRule {
  static __device__ __forceinline__ T fold(bool reset, bool real, T step, T pv) {
    if (reset) return (T)0;
    if (real) return (T)((float)pv + (float)step);
    return (T)((u32)pv + 1u);
  }
};

// basins.basins (pyflwdir/basins.py:12-18, core.fillnodata_upstream with nodata 0): the own seed wins, else the
// downstream cell's label; an unseeded pit keeps 0
template <class L>
struct LabelRule {
  static __device__ __forceinline__ L root(L own) { return own; }
  static __device__ __forceinline__ L fold(L own, L pv) { return own != 0 ? own : pv; }
};
