// upscale.hip — the data-parallel upscaling methods of the reference (pyflwdir/upscale.py): DMM (dmm_exitcell :66-111,
// dmm_nextidx :114-169), EAM (eam_repcell :243-287, eam_nextidx :290-335), EAM+ = ihu(niter=0) (ihu_outlets :381-434,
// ihu_nextidx :437-496), upscale_error (:1312-1363) and subgrid.outlets (pyflwdir/subgrid.py:13-48).
//
// Every step of these methods is one of two shapes:
//   arg-max   per coarse cell the fine cell with the largest `uparea` among the cells that are valid and (a pit or inside a
//             selector: the coarse cell's edge for DMM, the effective area for EAM).  The reference scans the fine raster in
//             ascending index with a strict `>` against an initial 0, i.e. the result is the maximum of the key
//             (uparea, -index) over the candidates with uparea > 0 — a total order, so the reduction order is free.  This
//             pass reads the whole fine raster once (1 code byte per cell, the area of the candidates) and is the
//             bandwidth-bound part.  cellsize <= 256: a workgroup takes one coarse row and a strip of whole coarse cells,
//             one thread per fine column (coalesced rows), then a segmented tree over the columns of each cell in LDS.
//             cellsize > 256: a workgroup per coarse cell.
//   walk      one thread per coarse cell follows the fine downstream links from a start cell to a stop condition.  The
//             walks are bounded by the network, not by cellsize; every walk is capped at n_fine steps and reports an error
//             instead of spinning on a cycle (the reference's `while True` never returns there).
// The error word of the walks and the import of upscale_error's lists are the shared ones of walks.h.
// The effective area ri**0.5 + ci**0.5 <= R**0.5 depends on (ri, ci, cellsize) only: the host evaluates it in float64 and
// uploads a byte mask — no square root is taken on the device.  The offset window of dmm_nextidx (R = cellsize / 2, `// R`
// in float) is restated in doubled integers, exact for odd cellsize as well.
#include <algorithm>

#include "common.h"
#include "walks.h"

namespace {

enum { SEL_EDGE = 0, SEL_EFFAREA = 1 };
enum { UE_NODS = WE_OWN };  // the calls' own bit of the error word (walks.h)
const WalkErrText UP_TEXT = {"an index",
                             "a walk along the fine flow directions did not end within n cells (the raster holds a cycle)"};

// the fine raster, the coarse grid over it and the effective-area mask
struct Up {
  const u8 *ncode;
  Geo g;
  u32 cs, nrow1, ncol1, n1;
  const u8 *ea;  // [min(cs, nrow)][min(cs, ncol)] bytes, may be null where no kernel reads it
  u32 mcol;
  __device__ __forceinline__ void rc(u32 i, u32 *r, u32 *c) const {
    *r = geo_row(g, i);
    *c = i - *r * g.ncol;
  }
  __device__ __forceinline__ u32 coarse(u32 i) const {
    u32 r, c;
    rc(i, &r, &c);
    return (r / cs) * ncol1 + c / cs;
  }
  __device__ __forceinline__ u32 down(u32 i) const { return d8_down(g, i, ncode[i]); }
  __device__ __forceinline__ bool effarea(u32 i) const {
    u32 r, c;
    rc(i, &r, &c);
    return ea[(r % cs) * mcol + c % cs] != 0;
  }
};

// max of (uparea, -index): a NaN never wins, nothing wins against the initial (0, none) without uparea > 0
template <class T>
__device__ __forceinline__ void take(T &bu, u32 &bi, T u, u32 i) {
  if (i == PFD_NOCELL) return;
  if (u > bu || (u == bu && bi != PFD_NOCELL && i < bi)) bu = u, bi = i;
}
template <int SEL>
__device__ __forceinline__ bool selected(const Up &f, u32 ri, u32 ci) {
  if (SEL == SEL_EDGE) return ri == 0 || ci == 0 || ri + 1 == f.cs || ci + 1 == f.cs;
  return f.ea[ri * f.mcol + ci] != 0;
}

// cellsize <= 256: workgroup = (coarse row, strip of W = (256 / cs) * cs fine columns), thread = fine column
template <int SEL, class T>
__global__ void __launch_bounds__(256) k_rep_strip(const Up f, const T *__restrict__ upa, u32 strips, u32 W,
                                                   u32 *__restrict__ rep) {
  __shared__ T su[256];
  __shared__ u32 si[256];
  const u32 R = blockIdx.x / strips, s = blockIdx.x - R * strips, t = threadIdx.x;
  const u64 col = (u64)s * W + t;
  const bool active = t < W && col < f.g.ncol;
  const u32 ci = t % f.cs;  // (W is a multiple of cs)
  T bu = T(0);
  u32 bi = PFD_NOCELL;
  if (active) {
    const u64 r0 = (u64)R * f.cs, r1 = r0 + f.cs < f.g.nrow ? r0 + f.cs : f.g.nrow;
    for (u64 r = r0; r < r1; ++r) {
      const u32 i = (u32)(r * f.g.ncol + col);
      const u32 code = f.ncode[i];
      if (code == D8_MV) continue;
      if (code == 0 || selected<SEL>(f, (u32)(r - r0), ci)) take(bu, bi, upa[i], i);
    }
  }
  su[t] = bu, si[t] = bi;
  __syncthreads();
  for (u32 st = 1; st < f.cs; st <<= 1) {
    // (a slot read in this step belongs to a thread with ci % (2 * st) == st, which does not write in it)
    if (ci % (2 * st) == 0 && ci + st < f.cs && t + st < 256u) {
      take(bu, bi, su[t + st], si[t + st]);
      su[t] = bu, si[t] = bi;
    }
    __syncthreads();
  }
  if (active && ci == 0) rep[(u64)R * f.ncol1 + (u32)(col / f.cs)] = bi;
}
// cellsize > 256: workgroup = coarse cell
template <int SEL, class T>
__global__ void __launch_bounds__(256) k_rep_cell(const Up f, const T *__restrict__ upa, u32 *__restrict__ rep) {
  __shared__ T su[256];
  __shared__ u32 si[256];
  const u32 R = blockIdx.x / f.ncol1, C = blockIdx.x - R * f.ncol1, t = threadIdx.x;
  const u64 r0 = (u64)R * f.cs, r1 = r0 + f.cs < f.g.nrow ? r0 + f.cs : f.g.nrow;
  const u64 c0 = (u64)C * f.cs, c1 = c0 + f.cs < f.g.ncol ? c0 + f.cs : f.g.ncol;
  T bu = T(0);
  u32 bi = PFD_NOCELL;
  for (u64 r = r0; r < r1; ++r)
    for (u64 c = c0 + t; c < c1; c += 256u) {
      const u32 i = (u32)(r * f.g.ncol + c);
      const u32 code = f.ncode[i];
      if (code == D8_MV) continue;
      if (code == 0 || selected<SEL>(f, (u32)(r - r0), (u32)(c - c0))) take(bu, bi, upa[i], i);
    }
  su[t] = bu, si[t] = bi;
  __syncthreads();
  for (u32 st = 128; st > 0; st >>= 1) {
    if (t < st) {
      take(bu, bi, su[t + st], si[t + st]);
      su[t] = bu, si[t] = bi;
    }
    __syncthreads();
  }
  if (t == 0) rep[blockIdx.x] = bi;
}

// ihu_outlets: from the representative cell down to the last cell inside the coarse cell (or a pit)
__global__ void __launch_bounds__(256) k_outlet_walk(const Up f, const u32 *__restrict__ rep, u32 *__restrict__ out,
                                                     u32 *__restrict__ err) {
  const u32 idx0 = blockIdx.x * 256u + threadIdx.x;
  if (idx0 >= f.n1) return;
  u32 sub = rep[idx0];
  if (sub != PFD_NOCELL) {
    u32 steps = 0;
    for (;;) {
      const u32 sub1 = f.down(sub);
      if (sub1 == sub || f.coarse(sub1) != idx0) break;
      sub = sub1;
      if (++steps >= f.g.n) {
        atomicOr(err, (u32)WE_CAP);
        sub = PFD_NOCELL;
        break;
      }
    }
  }
  out[idx0] = sub;
}
// dmm_nextidx: the exit cell is followed until it leaves the coarse cell shifted by half a cell towards it.  With
// d = 1 where the cell lies in the lower / right half (2 * ri >= cs), the window is |subr - ((r0 + d) * cs - 0.5)| <= cs / 2.
__global__ void __launch_bounds__(256) k_next_dmm(const Up f, const u32 *__restrict__ rep, u32 *__restrict__ ds,
                                                  u32 *__restrict__ err) {
  const u32 idx0 = blockIdx.x * 256u + threadIdx.x;
  if (idx0 >= f.n1) return;
  u32 sub = rep[idx0], idx = idx0;
  if (sub == PFD_NOCELL) {
    ds[idx0] = PFD_NOCELL;
    return;
  }
  u32 r, c;
  f.rc(sub, &r, &c);
  const i64 cs = f.cs;
  const i64 dr = 2 * (i64)(r % f.cs) >= cs, dc = 2 * (i64)(c % f.cs) >= cs;
  const i64 wr = 2 * ((i64)(idx0 / f.ncol1) + dr) * cs - 1, wc = 2 * ((i64)(idx0 % f.ncol1) + dc) * cs - 1;  // doubled centres
  u32 steps = 0;
  for (;;) {
    const u32 sub1 = f.down(sub);
    if (sub1 == sub) break;
    const u32 idx1 = f.coarse(sub1);
    if (idx1 != idx0) {
      f.rc(sub, &r, &c);
      const i64 a = 2 * (i64)r - wr, b = 2 * (i64)c - wc;
      if ((a < 0 ? -a : a) > cs || (b < 0 ? -b : b) > cs) break;
    }
    sub = sub1, idx = idx1;
    if (++steps >= f.g.n) {
      atomicOr(err, (u32)WE_CAP);
      idx = PFD_NOCELL;
      break;
    }
  }
  ds[idx0] = idx;
}
// eam_nextidx: to the first effective area of another coarse cell, or to the pit
__global__ void __launch_bounds__(256) k_next_eam(const Up f, const u32 *__restrict__ rep, u32 *__restrict__ ds,
                                                  u32 *__restrict__ err) {
  const u32 idx0 = blockIdx.x * 256u + threadIdx.x;
  if (idx0 >= f.n1) return;
  u32 sub = rep[idx0], idx1 = PFD_NOCELL;
  if (sub != PFD_NOCELL) {
    u32 steps = 0;
    for (;;) {
      const u32 sub1 = f.down(sub);
      idx1 = f.coarse(sub1);
      if (sub1 == sub || (idx1 != idx0 && f.effarea(sub1))) break;
      sub = sub1;
      if (++steps >= f.g.n) {
        atomicOr(err, (u32)WE_CAP);
        idx1 = PFD_NOCELL;
        break;
      }
    }
  }
  ds[idx0] = idx1;
}
// ihu_nextidx: to the next outlet cell (or pit); taken when it lies within the 8 neighbours, else the first effective area
// met on the way.  Neither: the reference indexes with its missing value (UE_NODS).
__global__ void __launch_bounds__(256) k_next_ihu(const Up f, const u32 *__restrict__ out, u32 *__restrict__ ds,
                                                  u32 *__restrict__ err) {
  const u32 idx0 = blockIdx.x * 256u + threadIdx.x;
  if (idx0 >= f.n1) return;
  u32 sub = out[idx0], res = PFD_NOCELL;
  if (sub != PFD_NOCELL) {
    u32 sub_ds = PFD_NOCELL, steps = 0;
    bool capped = false;
    for (;;) {
      const u32 sub1 = f.down(sub);
      const u32 idx1 = f.coarse(sub1);
      if (out[idx1] == sub1 || sub1 == sub) {
        const i64 dr = (i64)(idx1 / f.ncol1) - (i64)(idx0 / f.ncol1), dc = (i64)(idx1 % f.ncol1) - (i64)(idx0 % f.ncol1);
        if (dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1) sub_ds = sub1;
        break;
      }
      if (sub_ds == PFD_NOCELL && f.effarea(sub1)) sub_ds = sub1;
      sub = sub1;
      if (++steps >= f.g.n) {
        capped = true;
        break;
      }
    }
    if (capped) atomicOr(err, (u32)WE_CAP);
    else if (sub_ds == PFD_NOCELL) atomicOr(err, (u32)UE_NODS);
    else res = f.coarse(sub_ds);
  }
  ds[idx0] = res;
}

template <class I>
__global__ void __launch_bounds__(256) k_export_idx(const u32 *__restrict__ in, u32 k, I *__restrict__ out) {
  const u32 j = blockIdx.x * 256u + threadIdx.x;
  if (j < k) out[j] = in[j] == PFD_NOCELL ? (I)-1 : (I)in[j];
}
__global__ void __launch_bounds__(256) k_flag_outlets(const u32 *__restrict__ out, u32 k, u8 *__restrict__ flag) {
  const u32 j = blockIdx.x * 256u + threadIdx.x;
  if (j < k && out[j] != PFD_NOCELL) flag[out[j]] = 1;
}
__global__ void __launch_bounds__(256) k_error_walk(const u8 *__restrict__ ncode, const Geo g, const u32 *__restrict__ out,
                                                    const u32 *__restrict__ ds1, u32 k, const u8 *__restrict__ flag,
                                                    u8 *__restrict__ res, u32 *__restrict__ err) {
  const u32 idx0 = blockIdx.x * 256u + threadIdx.x;
  if (idx0 >= k) return;
  u32 sub = out[idx0];
  const u32 idx_ds = ds1[idx0];
  u8 v = 255;
  if (sub != PFD_NOCELL && idx_ds != PFD_NOCELL) {
    u32 steps = 0;
    for (;;) {
      const u32 sub1 = d8_down(g, sub, ncode[sub]);
      if (flag[sub1] || sub1 == sub) {
        v = sub1 == out[idx_ds] ? 1 : 0;
        break;
      }
      sub = sub1;
      if (++steps >= g.n) {
        atomicOr(err, (u32)WE_CAP);
        break;
      }
    }
  }
  res[idx0] = v;
}

// the shared findings of the error word, then the calls' own
static int up_check_err(pfd_raster *h, WalkErr &err, const char *what) {
  u32 own = 0;
  PFDCHK(err.check(h, what, UP_TEXT, &own));
  if (own & UE_NODS) {
    pfd_set_error("%s: a coarse cell found neither an outlet within its 8 neighbours nor an effective area downstream "
                  "(the reference indexes with its missing value there)", what);
    return PFD_EINVAL;
  }
  return PFD_OK;
}

static int check_fine(pfd_raster *h, const char *what, i64 cellsize) {
  PFDCHK(pfd_begin_whole(h, what));
  if (cellsize < 1 || cellsize > 0x7FFFFFFFll) {
    pfd_set_error("%s: cellsize %lld is not a positive 32-bit integer", what, (long long)cellsize);
    return PFD_EINVAL;
  }
  return PFD_OK;
}

static Up make_up(pfd_raster *h, i64 cellsize, const u8 *ea_dev) {
  Up f;
  f.ncode = h->ncode, f.g = h->geo, f.cs = (u32)cellsize;
  f.nrow1 = (u32)((h->nrow + cellsize - 1) / cellsize), f.ncol1 = (u32)((h->ncol + cellsize - 1) / cellsize);
  f.n1 = f.nrow1 * f.ncol1;
  f.ea = ea_dev, f.mcol = (u32)std::min<i64>(cellsize, h->ncol);
  return f;
}

template <int SEL, class T>
static int rep_cells(pfd_raster *h, const Up &f, const T *upa, u32 *rep) {
  pfd_seg_begin(h, SEL == SEL_EDGE ? "upscale_exitcell" : "upscale_repcell");
  if (f.cs <= 256u) {
    const u32 W = (256u / f.cs) * f.cs, strips = cdiv_u32((u64)f.g.ncol, W);
    k_rep_strip<SEL, T><<<strips * f.nrow1, 256, 0, h->stream>>>(f, upa, strips, W, rep);
  } else {
    k_rep_cell<SEL, T><<<f.n1, 256, 0, h->stream>>>(f, upa, rep);
  }
  KCHK();
  pfd_seg_end(h, 1);
  return PFD_OK;
}

enum { M_DMM = PFD_UPSCALE_DMM, M_EAM = PFD_UPSCALE_EAM, M_EAM_PLUS = PFD_UPSCALE_EAM_PLUS };

// rep/exit cells -> (outlets) -> (next index); ds == nullptr: the outlets only
template <class T>
static int upscale_run(pfd_raster *h, int method, const Up &f, const T *upa, u32 *out, u32 *ds, u32 *err) {
  const u32 grid = cdiv_u32(f.n1, 256);
  if (method == M_DMM) {
    PFDCHK((rep_cells<SEL_EDGE, T>(h, f, upa, out)));
    if (!ds) return PFD_OK;
    pfd_seg_begin(h, "upscale_nextidx");
    k_next_dmm<<<grid, 256, 0, h->stream>>>(f, out, ds, err);
  } else if (method == M_EAM) {
    PFDCHK((rep_cells<SEL_EFFAREA, T>(h, f, upa, out)));
    if (!ds) return PFD_OK;
    pfd_seg_begin(h, "upscale_nextidx");
    k_next_eam<<<grid, 256, 0, h->stream>>>(f, out, ds, err);
  } else {
    DevBuf rep;
    PFDCHK(rep.alloc((size_t)f.n1 * sizeof(u32)));
    PFDCHK((rep_cells<SEL_EFFAREA, T>(h, f, upa, rep.as<u32>())));
    pfd_seg_begin(h, "upscale_outlets");
    k_outlet_walk<<<grid, 256, 0, h->stream>>>(f, rep.as<u32>(), out, err);
    KCHK();
    pfd_seg_end(h, 1);
    HIPCHK(hipStreamSynchronize(h->stream));  // (`rep` is released on return)
    if (!ds) return PFD_OK;
    pfd_seg_begin(h, "upscale_nextidx");
    k_next_ihu<<<grid, 256, 0, h->stream>>>(f, out, ds, err);
  }
  KCHK();
  pfd_seg_end(h, 1);
  return PFD_OK;
}

static int upscale_impl(pfd_raster *h, const char *what, int method, i64 cellsize, int uparea_dtype, const void *uparea,
                        const u8 *effarea_host, int idx_dtype, void *idxs_ds_out, void *idxs_out_out, int memspace) {
  PFDCHK(check_fine(h, what, cellsize));
  if (method != M_DMM && method != M_EAM && method != M_EAM_PLUS) {
    pfd_set_error("%s: unknown method code %d", what, method);
    return PFD_EINVAL;
  }
  if (!uparea || !idxs_out_out || (method != M_DMM && !effarea_host)) {
    pfd_set_error("%s: NULL argument", what);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("%s: unsupported index dtype code %d", what, idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  InArg ea;
  if (method != M_DMM)
    PFDCHK(ea.bind(effarea_host, (size_t)std::min<i64>(cellsize, h->nrow) * (size_t)std::min<i64>(cellsize, h->ncol), PFD_HOST,
                   h->stream));
  const Up f = make_up(h, cellsize, (const u8 *)ea.dev);
  const size_t isz = pfd_idx_bytes(idx_dtype);
  DevBuf out, ds;
  WalkErr err;
  PFDCHK(out.alloc((size_t)f.n1 * sizeof(u32)));
  if (idxs_ds_out) PFDCHK(ds.alloc((size_t)f.n1 * sizeof(u32)));
  PFDCHK(err.init(h));
  InArg upa;
  const size_t esz = uparea_dtype == PFD_I32 || uparea_dtype == PFD_F32 ? 4 : 8;
  PFDCHK(upa.bind(uparea, (size_t)h->n * esz, memspace, h->stream));
  switch (uparea_dtype) {
    case PFD_I32: PFDCHK(upscale_run<i32>(h, method, f, (const i32 *)upa.dev, out.as<u32>(), ds.as<u32>(), err.dev())); break;
    case PFD_F32: PFDCHK(upscale_run<float>(h, method, f, (const float *)upa.dev, out.as<u32>(), ds.as<u32>(), err.dev())); break;
    case PFD_F64: PFDCHK(upscale_run<double>(h, method, f, (const double *)upa.dev, out.as<u32>(), ds.as<u32>(), err.dev())); break;
    default:
      pfd_set_error("%s: uparea dtype code %d is not supported (int32, float32, float64)", what, uparea_dtype);
      return PFD_EUNSUPPORTED;
  }
  PFDCHK(up_check_err(h, err, what));
  return pfd_dispatch_idx(idx_dtype, what, [&](auto itag) -> int {
    typedef typename decltype(itag)::type I;
    OutArg o1, o2;
    PFDCHK(o1.bind(idxs_out_out, (size_t)f.n1 * isz, memspace));
    k_export_idx<I><<<cdiv_u32(f.n1, 256), 256, 0, h->stream>>>(out.as<u32>(), f.n1, (I *)o1.dev);
    KCHK();
    if (idxs_ds_out) {
      PFDCHK(o2.bind(idxs_ds_out, (size_t)f.n1 * isz, memspace));
      k_export_idx<I><<<cdiv_u32(f.n1, 256), 256, 0, h->stream>>>(ds.as<u32>(), f.n1, (I *)o2.dev);
      KCHK();
      PFDCHK(o2.finish(h->stream));
    }
    return o1.finish(h->stream);
  });
}

}  // namespace

extern "C" int pfd_upscale(pfd_raster *h, int method, int64_t cellsize, int uparea_dtype, const void *uparea,
                           const uint8_t *effarea_host, int idx_dtype, void *idxs_ds_out, void *idxs_out_out, int memspace) {
  if (!idxs_ds_out) {
    pfd_set_error("upscale: NULL idxs_ds_out");
    return PFD_EINVAL;
  }
  return upscale_impl(h, "upscale", method, cellsize, uparea_dtype, uparea, effarea_host, idx_dtype, idxs_ds_out, idxs_out_out,
                      memspace);
}

extern "C" int pfd_upscale_outlets(pfd_raster *h, int method, int64_t cellsize, int uparea_dtype, const void *uparea,
                                   const uint8_t *effarea_host, int idx_dtype, void *idxs_out_out, int memspace) {
  return upscale_impl(h, "ucat_outlets", method, cellsize, uparea_dtype, uparea, effarea_host, idx_dtype, nullptr, idxs_out_out,
                      memspace);
}

extern "C" int pfd_upscale_error(pfd_raster *h, int idx_dtype, const void *idxs_out, const void *idxs_ds_coarse, int64_t k,
                                 uint8_t *out, int memspace) {
  PFDCHK(check_fine(h, "upscale_error", 1));
  if (!idxs_out || !idxs_ds_coarse || !out || k < 1 || k > h->n) {
    pfd_set_error("upscale_error: bad arguments (NULL pointer, or %lld coarse cells for %lld fine cells)", (long long)k,
                  (long long)h->n);
    return PFD_EINVAL;
  }
  const size_t isz = pfd_idx_bytes(idx_dtype);
  if (!isz) {
    pfd_set_error("upscale_error: unsupported index dtype code %d", idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  InArg a, b;
  PFDCHK(a.bind(idxs_out, (size_t)k * isz, memspace, h->stream));
  PFDCHK(b.bind(idxs_ds_coarse, (size_t)k * isz, memspace, h->stream));
  DevBuf so, sd, flag;
  WalkErr err;
  PFDCHK(so.alloc((size_t)k * sizeof(u32)));
  PFDCHK(sd.alloc((size_t)k * sizeof(u32)));
  PFDCHK(flag.alloc((size_t)h->n));
  PFDCHK(err.init(h));
  HIPCHK(hipMemsetAsync(flag.p, 0, (size_t)h->n, h->stream));
  const u32 grid = cdiv_u32((u64)k, 256);
  // (fine cells, then coarse cells: IMPORT_ANY, there is no link to hold them against)
  PFDCHK(pfd_import_cells<IMPORT_ANY>(h, "upscale_error", idx_dtype, a.dev, (u64)k, (u64)h->n, so.as<u32>(), nullptr, err.dev()));
  PFDCHK(pfd_import_cells<IMPORT_ANY>(h, "upscale_error", idx_dtype, b.dev, (u64)k, (u64)k, sd.as<u32>(), nullptr, err.dev()));
  PFDCHK(up_check_err(h, err, "upscale_error"));  // (before anything is indexed with the lists)
  OutArg o;
  PFDCHK(o.bind(out, (size_t)k, memspace));
  pfd_seg_begin(h, "upscale_error");
  k_flag_outlets<<<grid, 256, 0, h->stream>>>(so.as<u32>(), (u32)k, flag.as<u8>());
  KCHK();
  k_error_walk<<<grid, 256, 0, h->stream>>>(h->ncode, h->geo, so.as<u32>(), sd.as<u32>(), (u32)k, flag.as<u8>(), (u8 *)o.dev,
                                            err.dev());
  KCHK();
  pfd_seg_end(h, 2);
  PFDCHK(up_check_err(h, err, "upscale_error"));
  return o.finish(h->stream);
}
