// subgrid.hip — unit catchments: subgrid.ucat_area (reference pyflwdir/subgrid.py:51-93;
// FlwdirRaster.ucat_area pyflwdir/pyflwdir.py:1159-1191) = a label flood from the unit-catchment outlets (the
// basins query of paths.hip) + a per-label sum of the cell areas.
//
// The reference accumulates `ucatch_are[label] += area[cell]` while it walks the cells in idxs_seq order, so a
// float sum depends on that order.  Integer areas (unit="cell") are a histogram (atomics, exact in any order);
// float areas are summed in the reference's order: cells of the exact idxs_seq order (order.hip) are stably
// sorted by label, then ONE LANE per label adds its cells from first to last — bit-identical.
// The segment walks further down stand on walks.h (opening checks, error word, list import, links); every rocprim call
// takes its scratch through pfd_rocprim (lists.h).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "lists.h"

int pfd_export_u32(pfd_raster *h, const u32 *src, i64 m, int idx_dtype, void *out, int memspace);  // api.hip

__global__ void k_mark_cells(const i64 *__restrict__ idx, u32 k, u8 *__restrict__ flag) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < k) flag[idx[t]] = 1;
}
__global__ void __launch_bounds__(256) k_ucat_count(const u32 *__restrict__ lab, const u8 *__restrict__ is_out, u64 n,
                                                    u32 *__restrict__ cnt) {
  // (grid-stride in whole workgroups: n may exceed the 2^32 threads one launch dimension runs)
  for (u64 x0 = (u64)blockIdx.x * blockDim.x; x0 < n; x0 += (u64)gridDim.x * blockDim.x) {
  const u64 x = x0 + threadIdx.x;
  u32 u = 0;
  if (x < n) {
    u = lab[x];
    if (is_out[x]) u = 0;
  }
  // neighbouring cells mostly carry the same label: the first lane of a run of equal labels adds the run's
  // length (a large catchment would otherwise queue up one same-address atomic per cell in L2)
  const u32 lane = threadIdx.x & 63u;
  const u32 prev = (u32)__shfl_up((int)u, 1);
  const bool head = lane == 0 || prev != u;
  const u64 heads = __ballot(head);
  if (head && u) {
    const u64 later = lane == 63u ? 0ull : (heads >> (lane + 1u));
    const u32 len = later ? (u32)__ffsll((long long)later) : 64u - lane;
    atomicAdd(&cnt[u - 1], len);
  }
  }
}
__global__ void __launch_bounds__(256) k_ucat_keys(const u32 *__restrict__ oseq, u32 nseq, const u32 *__restrict__ lab,
                                                   const u8 *__restrict__ is_out, u32 *__restrict__ keys) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nseq) return;
  const u32 x = oseq[j];
  const u32 u = lab[x];
  keys[j] = (u && !is_out[x]) ? u : 0u;
}
__global__ void __launch_bounds__(256) k_seg_bounds(const u32 *__restrict__ keys, u32 m, u32 *__restrict__ first,
                                                    u32 *__restrict__ last) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const u32 k = keys[j];
  if (k == 0) return;
  if (j == 0 || keys[j - 1] != k) first[k - 1] = j;
  if (j + 1 == m || keys[j + 1] != k) last[k - 1] = j + 1;
}
// one lane per label: its cells in idxs_seq order, added one after the other like the serial loop
template <class T>
__global__ void __launch_bounds__(64) k_ucat_sum(const u32 *__restrict__ cells, const u32 *__restrict__ first,
                                                 const u32 *__restrict__ last, u32 k, const T *__restrict__ rows, Geo g,
                                                 T *__restrict__ are) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= k) return;
  T acc = are[u];
  for (u32 j = first[u]; j < last[u]; ++j) acc = acc + rows[geo_row(g, cells[j])];
  are[u] = acc;
}

// the cells of the exact idxs_seq order that take a label from downstream, stably sorted by label: label u + 1 owns
// cells[first[u] .. last[u]) (first = bounds, last = bounds + k; both 0 for a label without cells)
static int ucat_sorted_cells(pfd_raster *h, const u32 *lab, const u8 *is_out, u32 k, DevBuf &cells, DevBuf &bounds, u32 *m_out,
                             const char *seg_name = nullptr) {
  DevBuf oseq, keys, keys2, tmp;
  PFDCHK(pfd_exact_seq_dev(h, oseq));
  const u32 m = (u32)h->n_seq;
  *m_out = m;
  if (!m) return PFD_OK;
  if (seg_name) pfd_seg_begin(h, seg_name);
  PFDCHK(keys.alloc((size_t)m * sizeof(u32)));
  PFDCHK(keys2.alloc((size_t)m * sizeof(u32)));
  PFDCHK(cells.alloc((size_t)m * sizeof(u32)));
  PFDCHK(bounds.alloc(2 * (size_t)k * sizeof(u32)));
  HIPCHK(hipMemsetAsync(bounds.p, 0, 2 * (size_t)k * sizeof(u32), h->stream));  // first = last = 0: empty segment
  k_ucat_keys<<<cdiv_u32(m, 256), 256, 0, h->stream>>>(oseq.as<u32>(), m, lab, is_out, keys.as<u32>());
  int bits = 1;
  while ((1ull << bits) <= (u64)k) ++bits;
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::radix_sort_pairs(p, b, keys.as<u32>(), keys2.as<u32>(), oseq.as<u32>(), cells.as<u32>(), (size_t)m, 0u,
                                     (unsigned)bits, h->stream);
  }));
  k_seg_bounds<<<cdiv_u32(m, 256), 256, 0, h->stream>>>(keys2.as<u32>(), m, bounds.as<u32>(), bounds.as<u32>() + k);
  KCHK();
  if (seg_name) pfd_seg_end(h, 4);
  HIPCHK(hipStreamSynchronize(h->stream));  // (the sort's buffers are released on return)
  return PFD_OK;
}

template <class T>
static int ucat_float(pfd_raster *h, const u32 *lab, const u8 *is_out, u32 k, const T *rows_dev, T *are_dev) {
  DevBuf cells, bounds;
  u32 m = 0;
  PFDCHK(ucat_sorted_cells(h, lab, is_out, k, cells, bounds, &m));
  if (!m) return PFD_OK;
  k_ucat_sum<T><<<cdiv_u32(k, 64), 64, 0, h->stream>>>(cells.as<u32>(), bounds.as<u32>(), bounds.as<u32>() + k, k, rows_dev,
                                                     h->geo, are_dev);
  KCHK();
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// beyond 2^32 - 2 cells: the same sum over the 64-bit sequence (order64.hip), in pieces of the sequence — per piece the
// (label, area) pairs of its cells are stably sorted by label, then ONE WAVE per label adds the label's values of the
// piece to the label's running sum, one after the other: lane 0's chain of adds is the reference's loop, the other
// lanes only fetch (64 consecutive values per load, the next 64 in flight while the chain runs)
// ---------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) k_ucat_pairs64(const u64 *__restrict__ q, u64 m, const u32 *__restrict__ lab,
                                                      const u8 *__restrict__ is_out, const T *__restrict__ rows, u64 ncol,
                                                      u32 *__restrict__ keys, T *__restrict__ vals) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const u64 x = q[j];
  const u32 u = lab[x];
  keys[j] = (u && !is_out[x]) ? u : 0u;
  vals[j] = rows[x / ncol];
}
template <class T>
__global__ void __launch_bounds__(64) k_ucat_sum_wave(const T *__restrict__ vals, const u32 *__restrict__ first,
                                                      const u32 *__restrict__ last, u32 k, T *__restrict__ are) {
  const u32 u = blockIdx.x, lane = threadIdx.x;
  const u32 b = first[u], e = last[u];
  if (b >= e) return;
  T acc = are[u];
  T v = b + lane < e ? vals[b + lane] : (T)0;
  for (u32 j = b; j < e; j += 64u) {
    const T cur = v;
    const u32 nx = j + 64u + lane;
    v = nx < e ? vals[nx] : (T)0;  // (in flight while the chain below runs)
    const u32 cnt = min(64u, e - j);
    if (cnt == 64u) {
#pragma unroll
      for (int i = 0; i < 64; ++i) acc = acc + __shfl(cur, i);
    } else {
      for (u32 i = 0; i < cnt; ++i) acc = acc + __shfl(cur, (int)i);
    }
  }
  if (lane == 0) are[u] = acc;
}

template <class T>
static int ucat_float_wide(pfd_raster *h, const u32 *lab, const u8 *is_out, u32 k, const T *rows_dev, T *are_dev) {
  DevBuf q;
  u64 nseq = 0;
  PFDCHK(pfd_wide_seq_dev(h, q, &nseq));
  if (!nseq) return PFD_OK;
  u64 piece = 1ull << 28;
  if (const char *e = pfd_knob("PFD_UCAT_PIECE")) piece = std::max<u64>(64, (u64)atoll(e));  // (tests: several pieces of a small raster)
  piece = std::min(piece, nseq);
  DevBuf keys, keys2, vals, vals2, bounds, tmp;
  PFDCHK(keys.alloc((size_t)piece * sizeof(u32)));
  PFDCHK(keys2.alloc((size_t)piece * sizeof(u32)));
  PFDCHK(vals.alloc((size_t)piece * sizeof(T)));
  PFDCHK(vals2.alloc((size_t)piece * sizeof(T)));
  PFDCHK(bounds.alloc(2 * (size_t)k * sizeof(u32)));
  int bits = 1;
  while ((1ull << bits) <= (u64)k) ++bits;
  // one scratch, sized for the largest piece, serves the sort of every piece
  auto sort_piece = [&](u64 m) {
    return [&, m](void *p, size_t &b) {
      return rocprim::radix_sort_pairs(p, b, keys.as<u32>(), keys2.as<u32>(), vals.as<T>(), vals2.as<T>(), (size_t)m, 0u,
                                       (unsigned)bits, h->stream);
    };
  };
  size_t tb = 0;
  PFDCHK(pfd_rocprim_scratch(tmp, sort_piece(piece), &tb));
  pfd_seg_begin(h, "ucat_sums");
  i64 launches = 0;
  for (u64 p0 = 0; p0 < nseq; p0 += piece) {
    const u64 m = std::min(piece, nseq - p0);
    k_ucat_pairs64<T><<<cdiv_u32(m, 256), 256, 0, h->stream>>>(q.as<u64>() + p0, m, lab, is_out, rows_dev, (u64)h->ncol, keys.as<u32>(),
                                                              vals.as<T>());
    size_t tb2 = tb;
    HIPCHK(sort_piece(m)(tmp.p, tb2));
    HIPCHK(hipMemsetAsync(bounds.p, 0, 2 * (size_t)k * sizeof(u32), h->stream));  // first = last = 0: empty segment
    k_seg_bounds<<<cdiv_u32(m, 256), 256, 0, h->stream>>>(keys2.as<u32>(), (u32)m, bounds.as<u32>(), bounds.as<u32>() + k);
    k_ucat_sum_wave<T><<<k, 64, 0, h->stream>>>(vals2.as<T>(), bounds.as<u32>(), bounds.as<u32>() + k, k, are_dev);
    launches += 5;
  }
  KCHK();
  pfd_seg_end(h, launches);
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

// The label fill of ucat_area / ucat_volume.  Outlets: a missing value (< 0) is skipped; of a repeated cell the LAST entry
// owns the label (`ucatch_map[idx0] = i + 1` in a loop over i).  lab: n labels (u32), is_out: n bytes, 1 on outlet cells.
static int ucat_labels(pfd_raster *h, const char *what, const int64_t *idxs_out, int64_t k, DevBuf &lab, DevBuf &is_out) {
  const u64 n = (u64)h->n;
  std::vector<i64> uidx;
  std::vector<u32> uid;
  {
    std::unordered_map<i64, size_t> pos;
    for (i64 i = 0; i < k; ++i) {
      const i64 c = idxs_out[i];
      if (c < 0) continue;
      if (c >= (i64)n) {
        pfd_set_error("%s: outlet index %lld outside the raster", what, (long long)c);
        return PFD_EINVAL;
      }
      auto it = pos.find(c);
      if (it == pos.end()) {
        pos[c] = uidx.size();
        uidx.push_back(c);
        uid.push_back((u32)(i + 1));
      } else {
        uid[it->second] = (u32)(i + 1);
      }
    }
  }
  const u32 ku = (u32)uidx.size();
  InArg di, dl;
  PFDCHK(di.bind(ku ? uidx.data() : nullptr, (size_t)ku * sizeof(i64), PFD_HOST, h->stream));
  PFDCHK(dl.bind(ku ? uid.data() : nullptr, (size_t)ku * sizeof(u32), PFD_HOST, h->stream));
  PFDCHK(lab.alloc((size_t)n * sizeof(u32) + 64));
  PFDCHK(is_out.alloc((size_t)n));
  PFDCHK(pfd_basins_dev(h, (const i64 *)di.dev, dl.dev, ku, 4, lab.p));
  HIPCHK(hipMemsetAsync(is_out.p, 0, (size_t)n, h->stream));
  if (ku) k_mark_cells<<<cdiv_u32(ku, 256), 256, 0, h->stream>>>((const i64 *)di.dev, ku, is_out.as<u8>());
  KCHK();
  HIPCHK(hipStreamSynchronize(h->stream));  // (the staged lists are released on return)
  return PFD_OK;
}

extern "C" int pfd_ucat_area(pfd_raster *h, const int64_t *idxs_out, int64_t k, int map_dtype, void *map_out, int memspace,
                             int area_dtype, const void *area_rows, void *area_out) {
  PFDCHK(pfd_check_handle(h));
  PFDCHK(pfd_reject_general(h, "ucat_area"));
  PFDCHK(pfd_require_unblocked(h, "ucat_area"));
  const bool wide = pfd_wide_cells(h);  // (64-bit cell indices: the label query runs at any size, the float sums walk order64.hip's sequence)
  if (!idxs_out || k < 0 || k >= 0xFFFFFFFFll || !map_out || !area_out ||
      (area_dtype != PFD_I32 && area_dtype != PFD_F32 && area_dtype != PFD_F64) || (area_dtype != PFD_I32 && !area_rows)) {
    pfd_set_error("pfd_ucat_area: bad arguments");
    return PFD_EINVAL;
  }
  pfd_seg_clear(h);
  const u64 n = (u64)h->n;
  DevBuf lab, is_out;
  PFDCHK(ucat_labels(h, "pfd_ucat_area", idxs_out, k, lab, is_out));
  const size_t esz = area_dtype == PFD_F64 ? 8 : 4;
  std::vector<unsigned char> are((size_t)std::max<i64>(k, 1) * esz);
  auto area_of = [&](i64 cell, unsigned char *dst) {
    const i64 r = cell / h->ncol;
    if (area_dtype == PFD_I32) {
      const i32 one = 1;
      memcpy(dst, &one, 4);
    } else {
      memcpy(dst, (const unsigned char *)area_rows + (size_t)r * esz, esz);
    }
  };
  for (i64 i = 0; i < k; ++i) {
    unsigned char *dst = are.data() + (size_t)i * esz;
    if (idxs_out[i] < 0) {
      if (area_dtype == PFD_I32) {
        const i32 v = -9999;
        memcpy(dst, &v, 4);
      } else if (area_dtype == PFD_F32) {
        const float v = -9999.f;
        memcpy(dst, &v, 4);
      } else {
        const double v = -9999.;
        memcpy(dst, &v, 8);
      }
    } else {
      area_of(idxs_out[i], dst);
    }
  }
  if (k) {
    DevBuf are_dev;
    PFDCHK(are_dev.alloc((size_t)k * esz));
    HIPCHK(hipMemcpyAsync(are_dev.p, are.data(), (size_t)k * esz, hipMemcpyHostToDevice, h->stream));
    if (area_dtype == PFD_I32) {
      // (int32 adds commute: the counts are added to the start values, wrapping like the reference's int32)
      k_ucat_count<<<(u32)std::min<u64>(cdiv_u32(n, 256), 1u << 22), 256, 0, h->stream>>>(lab.as<u32>(), is_out.as<u8>(), n, are_dev.as<u32>());
      KCHK();
    } else {
      InArg rows;
      PFDCHK(rows.bind(area_rows, (size_t)h->nrow * esz, PFD_HOST, h->stream));
      if (wide && area_dtype == PFD_F32)
        PFDCHK(ucat_float_wide<float>(h, lab.as<u32>(), is_out.as<u8>(), (u32)k, (const float *)rows.dev, are_dev.as<float>()));
      else if (wide)
        PFDCHK(ucat_float_wide<double>(h, lab.as<u32>(), is_out.as<u8>(), (u32)k, (const double *)rows.dev, are_dev.as<double>()));
      else if (area_dtype == PFD_F32)
        PFDCHK(ucat_float<float>(h, lab.as<u32>(), is_out.as<u8>(), (u32)k, (const float *)rows.dev, are_dev.as<float>()));
      else
        PFDCHK(ucat_float<double>(h, lab.as<u32>(), is_out.as<u8>(), (u32)k, (const double *)rows.dev, are_dev.as<double>()));
    }
    HIPCHK(hipMemcpyAsync(area_out, are_dev.p, (size_t)k * esz, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return pfd_export_u32(h, lab.as<u32>(), (i64)n, map_dtype, map_out, memspace);
}

// ---------------------------------------------------------------------------------------------------------------
// subgrid.ucat_volume (reference pyflwdir/subgrid.py:96-142; FlwdirRaster.ucat_volume pyflwdir.py:1193-1225): the label
// fill and the sorted cell list of ucat_area, then ONE LANE per label adds `area * max(0, depth - hand)` of its cells from
// first to last, for up to 8 depths held in registers (more depths: one launch per chunk of 8).  The reference's types,
// with D / H / A the dtypes of depths / hand / area: dh in promote(D, H), the product in P = promote(A, D, H), the running
// column `col = D(P(col) + product)` — rounded to D after every add (the build uses -ffp-contract=off: no fused add).
// ---------------------------------------------------------------------------------------------------------------
namespace {

// np.maximum(0, x): 0 where 0 >= x, else x (a NaN stays)
template <class T>
__device__ __forceinline__ T vol_dh(T depth, T hand) {
  const T x = depth - hand;
  return (T(0) >= x) ? T(0) : x;
}
template <class D, class H, class A>
__global__ void __launch_bounds__(256) k_vol_init(const i64 *__restrict__ idx, u32 k, u32 nd, const H *__restrict__ hand,
                                                  const A *__restrict__ rows, Geo g, const D *__restrict__ depths,
                                                  D *__restrict__ vol) {
  typedef typename Wider<D, H>::type DH;
  typedef typename Wider<DH, A>::type P;
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  if (j >= (u64)nd * k) return;
  const u32 d = (u32)(j / k), i = (u32)(j - (u64)d * k);
  const i64 c = idx[i];
  D v = (D)-9999;
  if (c >= 0) v = (D)((P)rows[geo_row(g, (u32)c)] * (P)vol_dh<DH>((DH)depths[d], (DH)hand[c]));
  vol[j] = v;
}
template <class D, class H, class A>
__global__ void __launch_bounds__(64) k_vol_sum(const u32 *__restrict__ cells, const u32 *__restrict__ first,
                                                const u32 *__restrict__ last, u32 k, const H *__restrict__ hand,
                                                const A *__restrict__ rows, Geo g, const D *__restrict__ depths, u32 d0, u32 nd,
                                                D *__restrict__ vol) {
  typedef typename Wider<D, H>::type DH;
  typedef typename Wider<DH, A>::type P;
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= k) return;
  const u32 b = first[u], e = last[u];
  if (b >= e) return;
  D acc[8];
  DH dep[8];
#pragma unroll
  for (u32 j = 0; j < 8; ++j) {
    acc[j] = j < nd ? vol[(u64)(d0 + j) * k + u] : D(0);
    dep[j] = j < nd ? (DH)depths[d0 + j] : DH(0);
  }
  for (u32 c = b; c < e; ++c) {
    const u32 cell = cells[c];
    const DH hv = (DH)hand[cell];
    const P a = (P)rows[geo_row(g, cell)];
#pragma unroll
    for (u32 j = 0; j < 8; ++j) acc[j] = (D)((P)acc[j] + a * (P)vol_dh<DH>(dep[j], hv));
  }
#pragma unroll
  for (u32 j = 0; j < 8; ++j)
    if (j < nd) vol[(u64)(d0 + j) * k + u] = acc[j];
}

template <class D, class H, class A>
static int vol_run(pfd_raster *h, const i64 *idx_dev, u32 k, u32 nd, const u32 *lab, const u8 *is_out, const H *hand,
                   const A *rows, const D *depths, D *vol) {
  pfd_seg_begin(h, "ucat_volume_init");
  k_vol_init<D, H, A><<<cdiv_u32((u64)nd * k, 256), 256, 0, h->stream>>>(idx_dev, k, nd, hand, rows, h->geo, depths, vol);
  KCHK();
  pfd_seg_end(h, 1);
  DevBuf cells, bounds;
  u32 m = 0;
  PFDCHK(ucat_sorted_cells(h, lab, is_out, k, cells, bounds, &m, "ucat_volume_sort"));
  if (!m) return PFD_OK;
  pfd_seg_begin(h, "ucat_volume_sums");
  i64 launches = 0;
  for (u32 d0 = 0; d0 < nd; d0 += 8, ++launches)
    k_vol_sum<D, H, A><<<cdiv_u32(k, 64), 64, 0, h->stream>>>(cells.as<u32>(), bounds.as<u32>(), bounds.as<u32>() + k, k, hand,
                                                             rows, h->geo, depths, d0, std::min<u32>(8u, nd - d0), vol);
  KCHK();
  pfd_seg_end(h, launches);
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

}  // namespace

extern "C" int pfd_ucat_volume(pfd_raster *h, const int64_t *idxs_out, int64_t k, int map_dtype, void *map_out, int hand_dtype,
                               const void *hand, int area_dtype, const void *area_rows, int depth_dtype, const void *depths,
                               int64_t ndepths, void *vol_out, int memspace) {
  PFDCHK(pfd_begin_whole(h, "ucat_volume"));
  if (!idxs_out || k < 0 || ndepths < 0 || !map_out || !hand || !area_rows || (ndepths && (!depths || !vol_out)) ||
      (u64)k * (u64)std::max<i64>(ndepths, 1) >= 0xFFFFFFFFull) {
    pfd_set_error("pfd_ucat_volume: bad arguments (NULL pointer, or %lld outlets x %lld depths)", (long long)k,
                  (long long)ndepths);
    return PFD_EINVAL;
  }
  if (!is_float_code(hand_dtype) || !is_float_code(area_dtype) || !is_float_code(depth_dtype)) {
    pfd_set_error("pfd_ucat_volume: hand, area and depths are float32 or float64 (codes %d, %d, %d)", hand_dtype, area_dtype,
                  depth_dtype);
    return PFD_EUNSUPPORTED;
  }
  DevBuf lab, is_out;
  PFDCHK(ucat_labels(h, "pfd_ucat_volume", idxs_out, k, lab, is_out));
  if (k && ndepths) {
    const size_t hsz = hand_dtype == PFD_F64 ? 8 : 4, asz = area_dtype == PFD_F64 ? 8 : 4, dsz = depth_dtype == PFD_F64 ? 8 : 4;
    InArg hd, rows, dep, idx;
    PFDCHK(hd.bind(hand, (size_t)h->n * hsz, memspace, h->stream));
    PFDCHK(rows.bind(area_rows, (size_t)h->nrow * asz, PFD_HOST, h->stream));
    PFDCHK(dep.bind(depths, (size_t)ndepths * dsz, PFD_HOST, h->stream));
    PFDCHK(idx.bind(idxs_out, (size_t)k * sizeof(i64), PFD_HOST, h->stream));
    OutArg vo;
    PFDCHK(vo.bind(vol_out, (size_t)k * (size_t)ndepths * dsz, memspace));
    const u32 *l = lab.as<u32>();
    const u8 *o = is_out.as<u8>();
    const i64 *ix = (const i64 *)idx.dev;
    const u32 ku = (u32)k, nd = (u32)ndepths;
#define PFD_VOL(D, H, A) PFDCHK((vol_run<D, H, A>(h, ix, ku, nd, l, o, (const H *)hd.dev, (const A *)rows.dev, (const D *)dep.dev, (D *)vo.dev)))
    const int sel = (depth_dtype == PFD_F64 ? 4 : 0) | (hand_dtype == PFD_F64 ? 2 : 0) | (area_dtype == PFD_F64 ? 1 : 0);
    switch (sel) {
      case 0: PFD_VOL(float, float, float); break;
      case 1: PFD_VOL(float, float, double); break;
      case 2: PFD_VOL(float, double, float); break;
      case 3: PFD_VOL(float, double, double); break;
      case 4: PFD_VOL(double, float, float); break;
      case 5: PFD_VOL(double, float, double); break;
      case 6: PFD_VOL(double, double, float); break;
      default: PFD_VOL(double, double, double); break;
    }
#undef PFD_VOL
    PFDCHK(vo.finish(h->stream));
  }
  return pfd_export_u32(h, lab.as<u32>(), (i64)h->n, map_dtype, map_out, memspace);
}

// ---------------------------------------------------------------------------------------------------------------
// The segment walks of the SUBGRID section: subgrid.segment_length / segment_average / segment_median / segment_slope /
// fixed_length_slope (reference pyflwdir/subgrid.py:145-337, :414-559).  One lane per outlet follows `next` — the decoded
// downstream link (accessor D) or the caller's main upstream cells — from its outlet cell.  Outlet flags are scattered into
// a byte raster first.  Three stop rules:
//   ONTO    segment_length steps ONTO the next outlet and includes it; it stops before a masked-out cell, at a pit and
//           at a missing next cell;
//   BEFORE  segment_average / _median / _slope stop BEFORE the next outlet (and before a masked-out cell, at a pit, at a
//           missing next cell; the slope ignores the mask like the interpreted reference, whose `mask[i] is False` never
//           holds);
//   FIXED   fixed_length_slope walks down while distnc > x0 (ends at a pit), then up the main stem while distnc < x1 (ends
//           at a missing upstream cell).
// Every walk ends after n steps with WE_CAP set (walks.h): no kernel can spin on a cycle.  The outlet list is imported under
// IMPORT_OUTLETS, idxs_us_main under IMPORT_ANY.  The walks are latency-bound gathers,
// one dependent load per step; neighbouring lanes follow unrelated paths, so a wave runs as long as its longest segment.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// what the segment calls say about the shared findings of the error word
const WalkErrText SG_TEXT = {"an index of idxs_out or idxs_us_main",
                             "a walk did not end within n cells (the raster or idxs_us_main holds a cycle)"};

// the cells of one segment, in walk order, handed to `visit`; false: the step cap was hit
template <bool ONTO, class N, class F>
__device__ __forceinline__ bool sg_walk(const N &next, u32 idx0, const u8 *__restrict__ flag, const u8 *__restrict__ mask,
                                        u32 cap, F &&visit) {
  u32 idx = idx0, steps = 0;
  visit(idx0);
  for (;;) {
    const u32 idx1 = next(idx);
    if (idx1 == PFD_NOCELL || idx1 == idx || (mask && !mask[idx1])) break;
    if (!ONTO && flag[idx1]) break;
    idx = idx1;
    visit(idx);
    if (ONTO && flag[idx1]) break;
    if (++steps >= cap) return false;
  }
  return true;
}

template <class T>
__device__ __forceinline__ T sg_abs(T v) { return v < T(0) ? -v : v; }
__device__ __forceinline__ float sg_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double sg_abs(double v) { return fabs(v); }

// segment_length: |distnc[last] - distnc[outlet]| in the dtype of distnc (int32 cells, float32 metres)
template <class N, class T>
__global__ void __launch_bounds__(256) k_sg_length(const N next, const u32 *__restrict__ out_idx, u32 k,
                                                   const u8 *__restrict__ flag, const u8 *__restrict__ mask, u32 cap,
                                                   const T *__restrict__ distnc, T *__restrict__ res, u32 *__restrict__ err) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  const u32 idx0 = out_idx[i];
  T v = (T)-9999;
  if (idx0 != PFD_NOCELL) {
    u32 lastc = idx0;
    if (!sg_walk<true>(next, idx0, flag, mask, cap, [&](u32 x) { lastc = x; })) atomicOr(err, (u32)WE_CAP);
    v = sg_abs((T)(distnc[lastc] - distnc[idx0]));
  }
  res[i] = v;
}

// the reference's nodata test of _average (arithmetics.py:17-29) and of the median's np.where + nanmedian
template <class T>
__device__ __forceinline__ bool sg_skip_avg(T v, T nodata, bool nan) { return nan ? v != v : v == nodata; }

// segment_average: v += w0 * v0 in P = promote(W, T), w += w0 in W, v / w in P, stored as T
template <class N, class T, class W>
__global__ void __launch_bounds__(256) k_sg_average(const N next, const u32 *__restrict__ out_idx, u32 k,
                                                    const u8 *__restrict__ flag, const u8 *__restrict__ mask, u32 cap,
                                                    const T *__restrict__ data, const W *__restrict__ weights, T nodata,
                                                    bool nan, T *__restrict__ res, u32 *__restrict__ err) {
  typedef typename Wider<T, W>::type P;
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  const u32 idx0 = out_idx[i];
  T r = nodata;
  if (idx0 != PFD_NOCELL) {
    P v = P(0);
    W w = W(0);
    const bool ok = sg_walk<false>(next, idx0, flag, mask, cap, [&](u32 x) {
      const T v0 = data[x];
      if (sg_skip_avg(v0, nodata, nan)) return;
      const W w0 = weights ? weights[x] : W(1);
      v = v + (P)w0 * (P)v0;
      w = w + w0;
    });
    if (!ok) atomicOr(err, (u32)WE_CAP);
    if (w != W(0)) r = (T)(v / (P)w);
  }
  res[i] = r;
}

// segment_slope (mean): |dz / dx| between the first and the last cell of the segment, in the dtype of elevtn
template <class N, class E>
__global__ void __launch_bounds__(256) k_sg_slope(const N next, const u32 *__restrict__ out_idx, u32 k,
                                                  const u8 *__restrict__ flag, u32 cap, const E *__restrict__ elevtn,
                                                  const float *__restrict__ distnc, E *__restrict__ res, u32 *__restrict__ err) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  const u32 idx0 = out_idx[i];
  E r = (E)-9999;
  if (idx0 != PFD_NOCELL) {
    u32 lastc = idx0;
    if (!sg_walk<false>(next, idx0, flag, nullptr, cap, [&](u32 x) { lastc = x; })) atomicOr(err, (u32)WE_CAP);
    r = E(0);
    if (lastc != idx0) {
      const E dz = elevtn[idx0] - elevtn[lastc];
      const float dx = distnc[idx0] - distnc[lastc];
      r = sg_abs((E)(dz / (E)dx));
    }
  }
  res[i] = r;
}

// fixed_length_slope (mean): down to distnc <= x0 or a pit, up the main stem to distnc >= x1 or a headwater; float32
template <class D, class E>
__global__ void __launch_bounds__(256) k_sg_fixed_slope(const D d, const u32 *__restrict__ us, const u32 *__restrict__ out_idx,
                                                        u32 k, u32 cap, const E *__restrict__ elevtn,
                                                        const float *__restrict__ distnc, float half, float *__restrict__ res,
                                                        u32 *__restrict__ err) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  u32 idx = out_idx[i];
  float r = -9999.f;
  if (idx != PFD_NOCELL) {
    const float x0 = distnc[idx] - half, x1 = distnc[idx] + half;
    u32 steps = 0;
    bool ok = true;
    while (distnc[idx] > x0) {
      const u32 ds = (u32)d.down(idx);
      if (ds == idx) break;
      idx = ds;
      if (++steps >= cap) {
        ok = false;
        break;
      }
    }
    const u32 first = idx;
    steps = 0;
    while (ok && distnc[idx] < x1) {
      const u32 up = us[idx];
      if (up == PFD_NOCELL) break;
      idx = up;
      if (++steps >= cap) ok = false;
    }
    if (!ok) atomicOr(err, (u32)WE_CAP);
    r = 0.f;
    if (idx != first) r = (float)sg_abs((E)((elevtn[first] - elevtn[idx]) / (E)(distnc[first] - distnc[idx])));
  }
  res[i] = r;
}

// segment_median: count / write the values of a segment that are neither nodata nor NaN
template <bool FILL, class N, class T>
__global__ void __launch_bounds__(256) k_sg_collect(const N next, const u32 *__restrict__ out_idx, u32 k,
                                                    const u8 *__restrict__ flag, const u8 *__restrict__ mask, u32 cap,
                                                    const T *__restrict__ data, T nodata, u32 *__restrict__ cnt,
                                                    const u32 *__restrict__ off, T *__restrict__ vals,
                                                    unsigned long long *__restrict__ total, u32 *__restrict__ err) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  const u32 idx0 = out_idx[i];
  u32 c = 0;
  if (idx0 != PFD_NOCELL) {
    const u32 o = FILL ? off[i] : 0u;
    const bool ok = sg_walk<false>(next, idx0, flag, mask, cap, [&](u32 x) {
      const T v = data[x];
      if (v == nodata || v != v) return;
      if (FILL) vals[o + c] = v;
      ++c;
    });
    if (!ok) atomicOr(err, (u32)WE_CAP);
  }
  if (!FILL) {
    cnt[i] = c;
    if (c) atomicAdd(total, (unsigned long long)c);
  }
}
template <class T>
__global__ void __launch_bounds__(256) k_sg_median(const u32 *__restrict__ out_idx, u32 k, const u32 *__restrict__ cnt,
                                                   const u32 *__restrict__ off, const T *__restrict__ sorted, T nodata,
                                                   T *__restrict__ res) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  T r = nodata;
  if (out_idx[i] != PFD_NOCELL) {
    const u32 c = cnt[i], o = off[i];
    if (c == 0) r = (T)NAN;
    else if (c & 1u) r = sorted[o + c / 2];
    else r = (sorted[o + c / 2 - 1] + sorted[o + c / 2]) / T(2);
  }
  res[i] = r;
}

// what every segment call starts with: the outlet list in 32-bit lanes, the outlet flags, the main upstream cells
struct SegCtx {
  DevBuf out_idx, flag, us;
  WalkErr err;
  InArg mask, oin, uin;
  u32 k = 0, cap = 0;
};
static int sg_setup(pfd_raster *h, const char *what, const int64_t *idxs_out, int64_t k, bool need_us, int idx_dtype,
                    const void *idxs_us_main, const uint8_t *mask, const void *out, int memspace, SegCtx &c) {
  PFDCHK(pfd_begin_whole(h, what));
  if (k < 0 || k >= 0xFFFFFFFFll || (k && (!idxs_out || !out)) || (need_us && !idxs_us_main)) {
    pfd_set_error("%s: bad arguments (NULL pointer, or %lld outlets)", what, (long long)k);
    return PFD_EINVAL;
  }
  if (need_us && !pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("%s: unsupported index dtype code %d", what, idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  c.k = (u32)k, c.cap = (u32)h->n;
  if (!k) return PFD_OK;
  const u32 n = (u32)h->n;
  PFDCHK(c.err.init(h));
  PFDCHK(c.out_idx.alloc((size_t)k * sizeof(u32)));
  PFDCHK(c.flag.alloc((size_t)n));
  HIPCHK(hipMemsetAsync(c.flag.p, 0, (size_t)n, h->stream));
  PFDCHK(c.oin.bind(idxs_out, (size_t)k * sizeof(i64), PFD_HOST, h->stream));
  PFDCHK(c.mask.bind(mask, (size_t)n, memspace, h->stream));
  if (need_us) PFDCHK(c.uin.bind(idxs_us_main, (size_t)n * pfd_idx_bytes(idx_dtype), memspace, h->stream));
  pfd_seg_begin(h, "segment_import");
  // (the rules of the two lists: walks.h.  The outlets raise their flags as they are imported)
  PFDCHK(pfd_import_cells<IMPORT_OUTLETS>(h, what, PFD_I64, c.oin.dev, (u64)k, (u64)n, c.out_idx.as<u32>(), c.flag.as<u8>(), c.err.dev()));
  if (need_us) {
    PFDCHK(c.us.alloc((size_t)n * sizeof(u32)));
    PFDCHK(pfd_import_cells<IMPORT_ANY>(h, what, idx_dtype, c.uin.dev, (u64)n, (u64)n, c.us.as<u32>(), nullptr, c.err.dev()));
  }
  pfd_seg_end(h, need_us ? 2 : 1);
  return c.err.check(h, what, SG_TEXT);  // (before anything is indexed with the lists)
}
// f(next) with the walk's link: the decoded D8 codes downstream, the imported main upstream cells upstream
template <class F>
static int sg_dispatch_dir(pfd_raster *h, const char *what, int direction, SegCtx &c, F f) {
  if (direction == PFD_DOWN) return f(NextDown<DownD8>{DownD8{h->ncode, h->geo}});
  if (direction == PFD_UP) return f(NextUp{c.us.as<u32>()});
  pfd_set_error("%s: unknown direction code %d", what, direction);
  return PFD_EINVAL;
}
static bool sg_dir_ok(const char *what, int direction, bool both) {
  if (direction == PFD_UP || direction == PFD_DOWN || (both && direction == PFD_BOTH)) return true;
  pfd_set_error("%s: unknown direction code %d", what, direction);
  return false;
}

template <class T>
static int sg_median_run(pfd_raster *h, int direction, SegCtx &c, const T *data, T nodata, T *res) {
  const char *what = "segment_median";
  const u32 k = c.k, grid = cdiv_u32((u64)k, 256);
  DevBuf cnt, off, vals, sorted, total, tmp;
  PFDCHK(cnt.alloc((size_t)k * sizeof(u32)));
  PFDCHK(off.alloc(((size_t)k + 1) * sizeof(u32)));
  PFDCHK(total.alloc(sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), h->stream));
  pfd_seg_begin(h, "segment_median_measure");
  PFDCHK(sg_dispatch_dir(h, what, direction, c, [&](auto next) -> int {
    k_sg_collect<false><<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), k, c.flag.as<u8>(), (const u8 *)c.mask.dev, c.cap,
                                                     data, nodata, cnt.as<u32>(), (const u32 *)nullptr, (T *)nullptr,
                                                     (unsigned long long *)total.p, c.err.dev());
    KCHK();
    return PFD_OK;
  }));
  pfd_seg_end(h, 1);
  PFDCHK(c.err.check(h, what, SG_TEXT));
  unsigned long long m = 0;
  HIPCHK(hipMemcpyAsync(&m, total.p, sizeof(m), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (m >= 0xFFFFFFFFull) {
    pfd_set_error("segment_median: the segments hold %llu values, beyond 32-bit offsets", m);
    return PFD_EUNSUPPORTED;
  }
  pfd_seg_begin(h, "segment_median_sort");
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::exclusive_scan(p, b, cnt.as<u32>(), off.as<u32>(), 0u, (size_t)k, rocprim::plus<u32>(), h->stream);
  }));
  const u32 mm = (u32)m;
  HIPCHK(hipMemcpyAsync(off.as<u32>() + k, &mm, sizeof(u32), hipMemcpyHostToDevice, h->stream));
  i64 launches = 1;
  if (m) {
    PFDCHK(vals.alloc((size_t)m * sizeof(T)));
    PFDCHK(sorted.alloc((size_t)m * sizeof(T)));
    PFDCHK(sg_dispatch_dir(h, what, direction, c, [&](auto next) -> int {
      k_sg_collect<true><<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), k, c.flag.as<u8>(), (const u8 *)c.mask.dev, c.cap,
                                                      data, nodata, (u32 *)nullptr, off.as<u32>(), vals.as<T>(),
                                                      (unsigned long long *)nullptr, c.err.dev());
      KCHK();
      return PFD_OK;
    }));
    // per segment, on rocprim's order-preserving radix keys of the float type (no NaN among the values)
    DevBuf stmp;
    PFDCHK(pfd_rocprim(stmp, [&](void *p, size_t &b) {
      return rocprim::segmented_radix_sort_keys(p, b, vals.as<T>(), sorted.as<T>(), (unsigned int)m, (unsigned int)k, off.as<u32>(),
                                                off.as<u32>() + 1, 0u, (unsigned int)(8 * sizeof(T)), h->stream);
    }));
    HIPCHK(hipStreamSynchronize(h->stream));  // (stmp is released here)
    launches += 3;
  }
  k_sg_median<T><<<grid, 256, 0, h->stream>>>(c.out_idx.as<u32>(), k, cnt.as<u32>(), off.as<u32>(), sorted.as<T>(), nodata, res);
  KCHK();
  pfd_seg_end(h, launches + 1);
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

}  // namespace

extern "C" int pfd_segment_length(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                                  const void *idxs_us_main, const uint8_t *mask, int dist_dtype, const void *distnc, void *out,
                                  int memspace) {
  const char *what = "segment_length";
  if (!sg_dir_ok(what, direction, false)) return PFD_EINVAL;
  if (dist_dtype != PFD_I32 && dist_dtype != PFD_F32) {
    pfd_set_error("segment_length: distnc is int32 (cells) or float32 (metres), not dtype code %d", dist_dtype);
    return PFD_EUNSUPPORTED;
  }
  SegCtx c;
  PFDCHK(sg_setup(h, what, idxs_out, k, direction == PFD_UP, idx_dtype, idxs_us_main, mask, out, memspace, c));
  if (!k) return PFD_OK;
  if (!distnc) {
    pfd_set_error("segment_length: NULL distnc");
    return PFD_EINVAL;
  }
  InArg dn;
  PFDCHK(dn.bind(distnc, (size_t)h->n * 4, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)k * 4, memspace));
  pfd_seg_begin(h, "segment_length");
  PFDCHK(sg_dispatch_dir(h, what, direction, c, [&](auto next) -> int {
    const u32 grid = cdiv_u32((u64)k, 256);
    if (dist_dtype == PFD_I32)
      k_sg_length<<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), c.k, c.flag.as<u8>(), (const u8 *)c.mask.dev, c.cap,
                                               (const i32 *)dn.dev, (i32 *)o.dev, c.err.dev());
    else
      k_sg_length<<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), c.k, c.flag.as<u8>(), (const u8 *)c.mask.dev, c.cap,
                                               (const float *)dn.dev, (float *)o.dev, c.err.dev());
    KCHK();
    return PFD_OK;
  }));
  pfd_seg_end(h, 1);
  PFDCHK(c.err.check(h, what, SG_TEXT));
  return o.finish(h->stream);
}

extern "C" int pfd_segment_slope(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                                 const void *idxs_us_main, int elev_dtype, const void *elevtn, const float *distnc, double length,
                                 void *out, int memspace) {
  const char *what = "segment_slope";
  if (!sg_dir_ok(what, direction, true)) return PFD_EINVAL;
  if (!is_float_code(elev_dtype)) {
    pfd_set_error("segment_slope: elevtn is float32 or float64, not dtype code %d", elev_dtype);
    return PFD_EUNSUPPORTED;
  }
  SegCtx c;
  PFDCHK(sg_setup(h, what, idxs_out, k, direction != PFD_DOWN, idx_dtype, idxs_us_main, nullptr, out, memspace, c));
  if (!k) return PFD_OK;
  if (!distnc || !elevtn) {
    pfd_set_error("segment_slope: NULL elevtn or distnc");
    return PFD_EINVAL;
  }
  const size_t esz = elev_dtype == PFD_F64 ? 8 : 4;
  InArg dn, el;
  PFDCHK(dn.bind(distnc, (size_t)h->n * 4, memspace, h->stream));
  PFDCHK(el.bind(elevtn, (size_t)h->n * esz, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)k * (direction == PFD_BOTH ? 4 : esz), memspace));
  const u32 grid = cdiv_u32((u64)k, 256);
  pfd_seg_begin(h, direction == PFD_BOTH ? "fixed_length_slope" : "segment_slope");
  if (direction == PFD_BOTH) {
    const float half = (float)(length / 2.0);  // (`distnc[idx0] - length / 2`: the Python float joins the float32 operand)
    const DownD8 d{h->ncode, h->geo};
    if (elev_dtype == PFD_F32)
      k_sg_fixed_slope<<<grid, 256, 0, h->stream>>>(d, c.us.as<u32>(), c.out_idx.as<u32>(), c.k, c.cap, (const float *)el.dev,
                                                    (const float *)dn.dev, half, (float *)o.dev, c.err.dev());
    else
      k_sg_fixed_slope<<<grid, 256, 0, h->stream>>>(d, c.us.as<u32>(), c.out_idx.as<u32>(), c.k, c.cap, (const double *)el.dev,
                                                    (const float *)dn.dev, half, (float *)o.dev, c.err.dev());
    KCHK();
  } else {
    PFDCHK(sg_dispatch_dir(h, what, direction, c, [&](auto next) -> int {
      if (elev_dtype == PFD_F32)
        k_sg_slope<<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), c.k, c.flag.as<u8>(), c.cap, (const float *)el.dev,
                                                (const float *)dn.dev, (float *)o.dev, c.err.dev());
      else
        k_sg_slope<<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), c.k, c.flag.as<u8>(), c.cap, (const double *)el.dev,
                                                (const float *)dn.dev, (double *)o.dev, c.err.dev());
      KCHK();
      return PFD_OK;
    }));
  }
  pfd_seg_end(h, 1);
  PFDCHK(c.err.check(h, what, SG_TEXT));
  return o.finish(h->stream);
}

extern "C" int pfd_segment_average(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                                   const void *idxs_us_main, const uint8_t *mask, int dtype, const void *data, int weight_dtype,
                                   const void *weights, double nodata, void *out, int memspace) {
  const char *what = "segment_average";
  if (!sg_dir_ok(what, direction, false)) return PFD_EINVAL;
  if (!is_float_code(dtype) || !is_float_code(weight_dtype)) {
    pfd_set_error("segment_average: data and weights are float32 or float64 (codes %d, %d)", dtype, weight_dtype);
    return PFD_EUNSUPPORTED;
  }
  SegCtx c;
  PFDCHK(sg_setup(h, what, idxs_out, k, direction == PFD_UP, idx_dtype, idxs_us_main, mask, out, memspace, c));
  if (!k) return PFD_OK;
  if (!data) {
    pfd_set_error("segment_average: NULL data");
    return PFD_EINVAL;
  }
  const size_t esz = dtype == PFD_F64 ? 8 : 4, wsz = weight_dtype == PFD_F64 ? 8 : 4;
  InArg da, we;
  PFDCHK(da.bind(data, (size_t)h->n * esz, memspace, h->stream));
  PFDCHK(we.bind(weights, (size_t)h->n * wsz, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)k * esz, memspace));
  const bool nan = nodata != nodata;
  pfd_seg_begin(h, "segment_average");
  PFDCHK(sg_dispatch_dir(h, what, direction, c, [&](auto next) -> int {
    const u32 grid = cdiv_u32((u64)k, 256);
    auto launch = [&](auto tt, auto wt) {
      typedef typename decltype(tt)::type T;
      typedef typename decltype(wt)::type W;
      k_sg_average<<<grid, 256, 0, h->stream>>>(next, c.out_idx.as<u32>(), c.k, c.flag.as<u8>(), (const u8 *)c.mask.dev, c.cap,
                                                (const T *)da.dev, (const W *)we.dev, (T)nodata, nan, (T *)o.dev,
                                                c.err.dev());
    };
    if (dtype == PFD_F32 && weight_dtype == PFD_F32) launch(PfdTag<float>{}, PfdTag<float>{});
    else if (dtype == PFD_F32) launch(PfdTag<float>{}, PfdTag<double>{});
    else if (weight_dtype == PFD_F32) launch(PfdTag<double>{}, PfdTag<float>{});
    else launch(PfdTag<double>{}, PfdTag<double>{});
    KCHK();
    return PFD_OK;
  }));
  pfd_seg_end(h, 1);
  PFDCHK(c.err.check(h, what, SG_TEXT));
  return o.finish(h->stream);
}

extern "C" int pfd_segment_median(pfd_raster *h, const int64_t *idxs_out, int64_t k, int direction, int idx_dtype,
                                  const void *idxs_us_main, const uint8_t *mask, int dtype, const void *data, double nodata,
                                  void *out, int memspace) {
  const char *what = "segment_median";
  if (!sg_dir_ok(what, direction, false)) return PFD_EINVAL;
  if (!is_float_code(dtype)) {
    pfd_set_error("segment_median: data is float32 or float64, not dtype code %d", dtype);
    return PFD_EUNSUPPORTED;
  }
  SegCtx c;
  PFDCHK(sg_setup(h, what, idxs_out, k, direction == PFD_UP, idx_dtype, idxs_us_main, mask, out, memspace, c));
  if (!k) return PFD_OK;
  if (!data) {
    pfd_set_error("segment_median: NULL data");
    return PFD_EINVAL;
  }
  const size_t esz = dtype == PFD_F64 ? 8 : 4;
  InArg da;
  PFDCHK(da.bind(data, (size_t)h->n * esz, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)k * esz, memspace));
  if (dtype == PFD_F32) PFDCHK(sg_median_run<float>(h, direction, c, (const float *)da.dev, (float)nodata, (float *)o.dev));
  else PFDCHK(sg_median_run<double>(h, direction, c, (const double *)da.dev, nodata, (double *)o.dev));
  return o.finish(h->stream);
}
