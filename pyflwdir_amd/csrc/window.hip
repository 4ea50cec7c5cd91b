// window.hip — the calls that look along the flow path around a cell (LOCAL / GLOBAL ARITHMETICS of the reference):
//   pfd_downstream      Flwdir.downstream      (reference pyflwdir/flwdir.py:394-410)
//   pfd_moving_average  Flwdir.moving_average  (flwdir.py:435-470, arithmetics.py:67-103, core._window core.py:369-397)
//   pfd_moving_median   Flwdir.moving_median   (flwdir.py:472-504, arithmetics.py:106-143)
//   pfd_path            FlwdirRaster.path      (pyflwdir.py:443-500, core.path / core._trace core.py:308-437)
// Every output depends on a bounded walk: one lane per cell (per start cell for the paths), no order-dependent state.
//
// The window of a cell, `_window(idx0, n)`: at most n cells down the downstream links — ending at a pit, and BEFORE a cell
// whose stream order is greater than the centre's when an order is given — and at most n cells up the main upstream cells,
// ending at a headwater.  The reference fills an array of 2n + 1 positions, farthest upstream cell first, and drops the empty
// ones: that position order is the order of the float sums.  Because idxs_ds[idxs_us_main[x]] == x (checked when the caller's
// list is imported), a lane needs no storage for it: it walks up u <= n steps, then makes ONE walk down, u steps back to the
// centre and up to n steps beyond, which meets the cells in summation order (win_visit).
//
// The import of the caller's list, its error word, the links of a walk and the tail of pfd_path (count walk, scan, fill walk,
// hand-over) are the shared ones of walks.h / lists.h; the windows import under IMPORT_DRAINS, the paths under IMPORT_ANY.
//
// The median keeps the window's values: a lane insertion-sorts their order-preserving integer keys, in LDS when the window
// fits (2n + 1 <= WMAX), else in a strided global workspace that serves the raster in chunks of a fixed byte budget.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "lists.h"

namespace {

// what the window calls say about the shared findings of the error word
const WalkErrText WIN_TEXT = {"an index of idxs_us_main",
                              "a walk did not end within n_cells steps (the raster or idxs_us_main holds a cycle)"};

// LDS budget of the small-window median ("Windows along the flow path"): slot * 256 + tid of 4-byte (float32)
// or 8-byte (float64) keys; 31 * 256 * 4 = 31744 B and 15 * 256 * 8 = 30720 B per workgroup, i.e. about 124 B per lane,
// so that 5 workgroups of 256 lanes (20 of the 32 wave slots of a CU) share the 160 KiB of a gfx950 CU.
template <class T>
struct WinCfg;
template <>
struct WinCfg<float> {
  typedef u32 Key;
  static constexpr u32 WMAX = 31;
};
template <>
struct WinCfg<double> {
  typedef u64 Key;
  static constexpr u32 WMAX = 15;
};
constexpr u32 WIN_BLOCK = 256;
constexpr size_t WIN_WS_BYTES = (size_t)256 << 20;  // byte budget of the large-window workspace

// order-preserving keys of the float types (total order: -0.0 < 0.0; no NaN is ever stored)
__device__ __forceinline__ u32 key_of(float v) {
  const u32 b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ u64 key_of(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}
__device__ __forceinline__ float val_of(u32 k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ double val_of(u64 k) {
  return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull)));
}

// the stream order of a cell as an integer, whatever integer dtype the caller holds it in (kind 0: no order given)
struct StrOrd {
  const void *p;
  int kind;
  __device__ __forceinline__ i64 at(u32 x) const {
    switch (kind) {
      case PFD_U8: return ((const u8 *)p)[x];
      case PFD_I32: return ((const i32 *)p)[x];
      case PFD_U32: return ((const u32 *)p)[x];
      default: return ((const i64 *)p)[x];
    }
  }
};

// ---- downstream: out[x] = data[idxs_ds[x]] for a valid cell (a pit: itself), data[x] for a nodata cell -------------------
template <class E>
__global__ void __launch_bounds__(256) k_downstream(const DownD8 d, u32 n, const E *__restrict__ data, E *__restrict__ out) {
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  out[x] = data[(u32)d.down(x)];  // (the code of a pit and of a nodata cell is no direction: its own index)
}

// ---- the window, in summation order --------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void win_visit(const DownD8 &d, const u32 *__restrict__ us, const StrOrd &so, u32 x0, u64 n,
                                          F &&visit) {
  u32 x = x0;
  u64 u = 0;
  while (u < n) {  // up the main stem
    const u32 y = us[x];
    if (y == PFD_NOCELL) break;
    x = y, ++u;
  }
  for (u64 i = 0; i < u; ++i) {  // back down to the centre
    visit(x);
    x = (u32)d.down(x);
  }
  visit(x);  // (== x0)
  const i64 s0 = so.kind ? so.at(x0) : 0;
  for (u64 i = 0; i < n; ++i) {  // down, below the centre only under the stream-order rule
    const u32 y = (u32)d.down(x);
    if (y == x) break;  // pit (a nodata centre as well)
    if (so.kind && so.at(y) > s0) break;
    x = y;
    visit(x);
  }
}

// moving_average: arithmetics._average over the window.  v += w0 * v0 in P = promote(W, T) with the product rounded
// before the add, w += w0 in W, v / w in P, stored as T; nodata where w == 0.  No weights: float64 ones.
template <class T, class W>
__global__ void __launch_bounds__(256) k_win_average(const DownD8 d, const u32 *__restrict__ us, const StrOrd so, u32 ncell,
                                                     u64 n, const T *__restrict__ data, const W *__restrict__ weights,
                                                     T nodata, bool nan, T *__restrict__ out) {
  typedef typename Wider<T, W>::type P;
  const u64 x = (u64)blockIdx.x * 256u + threadIdx.x;
  if (x >= ncell) return;
  T r = nodata;
  if (!(data[x] == nodata)) {
    P v = P(0);
    W w = W(0);
    win_visit(d, us, so, (u32)x, n, [&](u32 y) {
      const T v0 = data[y];
      if (nan ? v0 != v0 : v0 == nodata) return;
      const W w0 = weights ? weights[y] : W(1);
      v = v + (P)w0 * (P)v0;
      w = w + w0;
    });
    if (w != W(0)) r = (T)(v / (P)w);
  }
  out[x] = r;
}

// moving_median: np.nanmedian of the window's values that are neither nodata nor NaN.  A lane keeps the keys of its window
// sorted at buf[slot * stride]: `buf` is its column of the workgroup's LDS (stride 256: a wave's 64 lanes hit 64 different
// banks) or of the chunk's global workspace (stride = lanes of the chunk: a wave's accesses are one contiguous run).
template <class K>
__device__ __forceinline__ void win_insert(K *buf, u32 stride, u32 cnt, K key) {
  u32 j = cnt;
  while (j > 0) {
    const K p = buf[(size_t)(j - 1) * stride];
    if (p <= key) break;
    buf[(size_t)j * stride] = p;
    --j;
  }
  buf[(size_t)j * stride] = key;
}
template <class T, bool LDS>
__global__ void __launch_bounds__(256) k_win_median(const DownD8 d, const u32 *__restrict__ us, const StrOrd so, u32 x_begin,
                                                    u32 count, u64 n, const T *__restrict__ data, T nodata,
                                                    typename WinCfg<T>::Key *__restrict__ ws, u32 ws_stride,
                                                    T *__restrict__ out) {
  typedef typename WinCfg<T>::Key K;
  __shared__ K sh[LDS ? WinCfg<T>::WMAX * WIN_BLOCK : 1];
  const u64 lane = (u64)blockIdx.x * WIN_BLOCK + threadIdx.x;
  if (lane >= count) return;  // (no barrier below: a lane only touches its own column)
  const u32 x = x_begin + (u32)lane;
  K *buf = LDS ? sh + threadIdx.x : ws + lane;
  const u32 stride = LDS ? WIN_BLOCK : ws_stride;
  T r = nodata;
  if (!(data[x] == nodata)) {
    u32 cnt = 0;
    win_visit(d, us, so, x, n, [&](u32 y) {
      const T v = data[y];
      if (v != v || v == nodata) return;
      win_insert<K>(buf, stride, cnt, key_of(v));
      ++cnt;
    });
    if (cnt == 0) r = (T)NAN;
    else if (cnt & 1u) r = val_of(buf[(size_t)(cnt / 2) * stride]);
    else r = (val_of(buf[(size_t)(cnt / 2 - 1) * stride]) + val_of(buf[(size_t)(cnt / 2) * stride])) / T(2);
  }
  out[x] = r;
}

// what the two window calls start with
struct WinCtx {
  DevBuf us;
  WalkErr err;
  InArg uin, sin;
  StrOrd so{nullptr, 0};
};
// the caller's main upstream cells in 32-bit lanes under the call's import rule (walks.h), checked before anything is indexed
// with them
template <int CHECK>
static int win_import_us(pfd_raster *h, const char *what, int idx_dtype, const void *us_dev, DevBuf &us, WalkErr &err) {
  const u64 n = (u64)h->n;
  pfd_seg_begin(h, "window_import");
  PFDCHK(us.alloc((size_t)n * sizeof(u32)));
  PFDCHK(pfd_import_cells<CHECK>(h, what, idx_dtype, us_dev, n, n, us.as<u32>(), nullptr, err.dev()));
  pfd_seg_end(h, 1);
  return err.check(h, what, WIN_TEXT);
}
static int win_setup(pfd_raster *h, const char *what, int64_t n, int idx_dtype, const void *idxs_us_main, int strord_dtype,
                     const void *strord, const void *data, const void *out, int memspace, WinCtx &c) {
  PFDCHK(pfd_begin_whole(h, what));
  if (n < 0 || n > ((int64_t)1 << 61) || !idxs_us_main || !data || !out) {
    pfd_set_error("%s: bad arguments (NULL pointer, or n = %lld)", what, (long long)n);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("%s: unsupported index dtype code %d", what, idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  size_t ssz = 0;
  if (strord) {
    ssz = strord_dtype == PFD_U8 ? 1 : (strord_dtype == PFD_I32 || strord_dtype == PFD_U32 ? 4 : (strord_dtype == PFD_I64 ? 8 : 0));
    if (!ssz) {
      pfd_set_error("%s: the stream order is uint8, int32, uint32 or int64, not dtype code %d", what, strord_dtype);
      return PFD_EUNSUPPORTED;
    }
  }
  PFDCHK(c.err.init(h));
  PFDCHK(c.uin.bind(idxs_us_main, (size_t)h->n * pfd_idx_bytes(idx_dtype), memspace, h->stream));
  PFDCHK(c.sin.bind(strord, (size_t)h->n * ssz, memspace, h->stream));
  c.so = StrOrd{c.sin.dev, strord ? strord_dtype : 0};
  return win_import_us<IMPORT_DRAINS>(h, what, idx_dtype, c.uin.dev, c.us, c.err);
}

static size_t win_ws_budget() {
  const char *e = pfd_knob("PFD_WINDOW_WS_BYTES");  // (tests: a workspace chunk smaller than the raster)
  return e ? (size_t)std::max<long long>(1, atoll(e)) : WIN_WS_BYTES;
}

template <class T>
static int win_median_run(pfd_raster *h, WinCtx &c, int64_t n, const T *data, T nodata, T *out) {
  typedef typename WinCfg<T>::Key K;
  const u32 ncell = (u32)h->n;
  const DownD8 d{h->ncode, h->geo};
  const u64 W = 2 * (u64)n + 1;
  if (W <= WinCfg<T>::WMAX) {
    pfd_seg_begin(h, "moving_median_lds");
    k_win_median<T, true><<<cdiv_u32((u64)ncell, WIN_BLOCK), WIN_BLOCK, 0, h->stream>>>(d, c.us.as<u32>(), c.so, 0u, ncell, (u64)n,
                                                                                       data, nodata, (K *)nullptr, 0u, out);
    KCHK();
    pfd_seg_end(h, 1);
    return PFD_OK;
  }
  // the chunk of cells one workspace serves: sized by the byte budget, never by n_cells * (2n + 1)
  const u64 per_lane = W * sizeof(K);
  u64 lanes = std::max<u64>(WIN_BLOCK, (u64)win_ws_budget() / per_lane / WIN_BLOCK * WIN_BLOCK);
  lanes = std::min<u64>(lanes, std::min<u64>((u64)cdiv_u32((u64)ncell, WIN_BLOCK) * WIN_BLOCK, 0xFFFFFF00ull));
  if (per_lane > (u64)1 << 40) {  // (256 lanes of it are beyond any device)
    pfd_set_error("moving_median: no workspace for windows of %llu cells", (unsigned long long)W);
    return PFD_ENOMEM;
  }
  DevBuf ws;
  PFDCHK(ws.alloc((size_t)(lanes * per_lane)));
  pfd_seg_begin(h, "moving_median_workspace");
  i64 launches = 0;
  for (u64 x0 = 0; x0 < ncell; x0 += lanes, ++launches) {
    const u32 count = (u32)std::min<u64>(lanes, (u64)ncell - x0);
    k_win_median<T, false><<<cdiv_u32((u64)count, WIN_BLOCK), WIN_BLOCK, 0, h->stream>>>(d, c.us.as<u32>(), c.so, (u32)x0, count,
                                                                                        (u64)n, data, nodata, ws.as<K>(),
                                                                                        (u32)lanes, out);
  }
  KCHK();
  pfd_seg_end(h, launches);
  HIPCHK(hipStreamSynchronize(h->stream));  // (the workspace is released on return)
  return PFD_OK;
}

// ---- path: core._trace per start cell, as a count walk, a scan and a fill walk -----------------------------------------
// FILL = false: the length and the distance of path i; FILL = true: its cells at off[i]
template <bool FILL, class N, class O>
__global__ void __launch_bounds__(256) k_path(const N next, const Geo g, const i64 *__restrict__ start, u32 k,
                                              const u8 *__restrict__ mask, const double *__restrict__ steps, double max_length,
                                              int has_max, u32 cap, i64 *__restrict__ len, double *__restrict__ dist,
                                              const i64 *__restrict__ off, O *__restrict__ out, u32 *__restrict__ err) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  u32 x = (u32)start[i];
  O *o = FILL ? out + off[i] : nullptr;
  i64 l = 1;
  double dsum = 0.0;
  if (FILL) o[0] = (O)x;
  for (u32 nstep = 0;; ++nstep) {
    if (mask && mask[x]) break;  // (the first masked cell is part of the path)
    const u32 y = next(x);
    if (y == PFD_NOCELL || y == x) break;
    double step = 1.0;
    if (steps) {
      const u32 r0 = geo_row(g, x), r1 = geo_row(g, y);
      const u32 c0 = x - r0 * g.ncol, c1 = y - r1 * g.ncol;
      const int kind = r0 == r1 ? 1 : (c0 == c1 ? 0 : 2);  // vertical, horizontal, diagonal
      step = steps[(size_t)(r0 + r1) * 3 + kind];
    }
    if (has_max && dsum + step > max_length) break;
    if (nstep >= cap) {  // (n_cells steps: a cycle)
      atomicOr(err, (u32)WE_CAP);
      break;
    }
    dsum += step;
    x = y;
    if (FILL) o[l] = (O)x;
    ++l;
  }
  if (!FILL) len[i] = l, dist[i] = dsum;
}

}  // namespace

extern "C" int pfd_debug_window_wmax(int dtype, int *wmax) {
  if (!wmax || !is_float_code(dtype)) {
    pfd_set_error("pfd_debug_window_wmax: float32 or float64 (code %d), and room for the answer", dtype);
    return PFD_EINVAL;
  }
  *wmax = dtype == PFD_F32 ? (int)WinCfg<float>::WMAX : (int)WinCfg<double>::WMAX;
  return PFD_OK;
}

extern "C" int pfd_downstream(pfd_raster *h, int elem_bytes, const void *data, void *out, int memspace) {
  PFDCHK(pfd_begin_whole(h, "downstream"));
  if (!data || !out || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)) {
    pfd_set_error("pfd_downstream: bad arguments (NULL pointer, or elements of %d bytes: 1, 2, 4 or 8)", elem_bytes);
    return data && out ? PFD_EUNSUPPORTED : PFD_EINVAL;
  }
  const u32 n = (u32)h->n, grid = cdiv_u32((u64)n, 256);
  InArg da;
  PFDCHK(da.bind(data, (size_t)h->n * elem_bytes, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)h->n * elem_bytes, memspace));
  const DownD8 d{h->ncode, h->geo};
  pfd_seg_begin(h, "downstream");
  switch (elem_bytes) {
    case 1: k_downstream<u8><<<grid, 256, 0, h->stream>>>(d, n, (const u8 *)da.dev, (u8 *)o.dev); break;
    case 2: k_downstream<uint16_t><<<grid, 256, 0, h->stream>>>(d, n, (const uint16_t *)da.dev, (uint16_t *)o.dev); break;
    case 4: k_downstream<u32><<<grid, 256, 0, h->stream>>>(d, n, (const u32 *)da.dev, (u32 *)o.dev); break;
    default: k_downstream<u64><<<grid, 256, 0, h->stream>>>(d, n, (const u64 *)da.dev, (u64 *)o.dev); break;
  }
  KCHK();
  pfd_seg_end(h, 1);
  return o.finish(h->stream);
}

extern "C" int pfd_moving_average(pfd_raster *h, int64_t n, int idx_dtype, const void *idxs_us_main, int strord_dtype,
                                  const void *strord, int dtype, const void *data, int weight_dtype, const void *weights,
                                  double nodata, void *out, int memspace) {
  const char *what = "moving_average";
  if (!is_float_code(dtype) || (weights && !is_float_code(weight_dtype))) {
    pfd_set_error("moving_average: data and weights are float32 or float64 (codes %d, %d)", dtype, weight_dtype);
    return PFD_EUNSUPPORTED;
  }
  WinCtx c;
  PFDCHK(win_setup(h, what, n, idx_dtype, idxs_us_main, strord_dtype, strord, data, out, memspace, c));
  const size_t esz = dtype == PFD_F64 ? 8 : 4, wsz = weight_dtype == PFD_F64 ? 8 : 4;
  InArg da, we;
  PFDCHK(da.bind(data, (size_t)h->n * esz, memspace, h->stream));
  PFDCHK(we.bind(weights, (size_t)h->n * wsz, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)h->n * esz, memspace));
  const bool nan = nodata != nodata;
  const u32 ncell = (u32)h->n, grid = cdiv_u32((u64)ncell, 256);
  const DownD8 d{h->ncode, h->geo};
  auto launch = [&](auto tt, auto wt) {
    typedef typename decltype(tt)::type T;
    typedef typename decltype(wt)::type W;
    k_win_average<T, W><<<grid, 256, 0, h->stream>>>(d, c.us.as<u32>(), c.so, ncell, (u64)n, (const T *)da.dev, (const W *)we.dev,
                                                    (T)nodata, nan, (T *)o.dev);
  };
  pfd_seg_begin(h, "moving_average");
  const bool w32 = weights && weight_dtype == PFD_F32;  // (no weights: float64 ones)
  if (dtype == PFD_F32 && w32) launch(PfdTag<float>{}, PfdTag<float>{});
  else if (dtype == PFD_F32) launch(PfdTag<float>{}, PfdTag<double>{});
  else if (w32) launch(PfdTag<double>{}, PfdTag<float>{});
  else launch(PfdTag<double>{}, PfdTag<double>{});
  KCHK();
  pfd_seg_end(h, 1);
  return o.finish(h->stream);
}

extern "C" int pfd_moving_median(pfd_raster *h, int64_t n, int idx_dtype, const void *idxs_us_main, int strord_dtype,
                                 const void *strord, int dtype, const void *data, double nodata, void *out, int memspace) {
  const char *what = "moving_median";
  if (!is_float_code(dtype)) {
    pfd_set_error("moving_median: data is float32 or float64, not dtype code %d", dtype);
    return PFD_EUNSUPPORTED;
  }
  WinCtx c;
  PFDCHK(win_setup(h, what, n, idx_dtype, idxs_us_main, strord_dtype, strord, data, out, memspace, c));
  const size_t esz = dtype == PFD_F64 ? 8 : 4;
  InArg da;
  PFDCHK(da.bind(data, (size_t)h->n * esz, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)h->n * esz, memspace));
  if (dtype == PFD_F32) PFDCHK(win_median_run<float>(h, c, n, (const float *)da.dev, (float)nodata, (float *)o.dev));
  else PFDCHK(win_median_run<double>(h, c, n, (const double *)da.dev, nodata, (double *)o.dev));
  return o.finish(h->stream);
}

extern "C" int pfd_path(pfd_raster *h, const int64_t *idxs, int64_t k, int direction, int idx_dtype, const void *idxs_us_main,
                        const uint8_t *mask, const double *step_lengths, int has_max_length, double max_length,
                        void *idxs_out, int64_t cap_idxs, int64_t *offsets_out, double *dist_out, int64_t *n_out,
                        int memspace) {
  const char *what = "path";
  PFDCHK(pfd_begin_whole(h, what));
  if (k < 0 || k >= 0xFFFFFFFFll || (k && !idxs) || !n_out || cap_idxs < 0 || (cap_idxs > 0 && (!idxs_out || !offsets_out || !dist_out)) ||
      (direction != PFD_UP && direction != PFD_DOWN) || (direction == PFD_UP && !idxs_us_main)) {
    pfd_set_error("path: bad arguments (NULL pointer, %lld start cells, cap_idxs=%lld, direction code %d)", (long long)k,
                  (long long)cap_idxs, direction);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("path: unsupported index dtype code %d", idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  for (i64 i = 0; i < k; ++i)
    if (idxs[i] < 0 || idxs[i] >= h->n) {
      pfd_set_error("path: start index %lld outside the raster", (long long)idxs[i]);
      return PFD_EINVAL;
    }
  *n_out = 0;
  if (!k) return give_empty(h, offsets_out, memspace);
  const u32 ku = (u32)k, grid = cdiv_u32((u64)k, 256), cap = (u32)h->n;
  WalkErr err;
  DevBuf us, dist;
  InArg di, dm, du, ds;
  PFDCHK(err.init(h));
  PFDCHK(di.bind(idxs, (size_t)k * sizeof(i64), PFD_HOST, h->stream));
  PFDCHK(dm.bind(mask, (size_t)h->n, memspace, h->stream));
  PFDCHK(ds.bind(step_lengths, (size_t)(2 * h->nrow - 1) * 3 * sizeof(double), PFD_HOST, h->stream));
  if (direction == PFD_UP) {
    PFDCHK(du.bind(idxs_us_main, (size_t)h->n * pfd_idx_bytes(idx_dtype), memspace, h->stream));
    PFDCHK(win_import_us<IMPORT_ANY>(h, what, idx_dtype, du.dev, us, err));
  }
  PFDCHK(dist.alloc((size_t)k * sizeof(double)));
  const DownD8 d{h->ncode, h->geo};
  // the count walk (FILL = false: lengths into `lens`, distances into `dist`) and the fill walk (cells at dst + off[i])
  auto walk = [&](auto fill, auto itag, i64 *lens, const i64 *off, void *dst) -> int {
    typedef typename decltype(itag)::type I;
    constexpr bool FILL = decltype(fill)::value;
    auto launch = [&](auto next) {
      k_path<FILL, decltype(next), I><<<grid, 256, 0, h->stream>>>(next, h->geo, (const i64 *)di.dev, ku, (const u8 *)dm.dev,
                                                                 (const double *)ds.dev, max_length, has_max_length, cap, lens,
                                                                 dist.as<double>(), off, (I *)dst, err.dev());
    };
    if (direction == PFD_DOWN) launch(NextDown<DownD8>{d});
    else launch(NextUp{us.as<u32>()});
    KCHK();
    return PFD_OK;
  };
  const RaggedSegs segs = {"path_count", "path_offsets", "path_fill", what};
  const RaggedOut ro = {idx_dtype, idxs_out, cap_idxs, offsets_out, INT64_MAX, memspace};
  bool given = false;
  PFDCHK(pfd_ragged_tail(
      h, segs, (u64)k, ro, [&](i64 *lens) { return walk(std::false_type{}, PfdTag<i64>{}, lens, nullptr, nullptr); },
      [&] { return err.check(h, what, WIN_TEXT); },
      [&](auto itag, const i64 *off, auto *dst) { return walk(std::true_type{}, itag, nullptr, off, dst); }, n_out, &given));
  if (given) PFDCHK(give_list(h, dist.p, (size_t)k * sizeof(double), dist_out, memspace));
  return PFD_OK;
}
