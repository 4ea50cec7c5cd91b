// basins_ext.hip — the rest of the reference's BASINS section: basins.interbasin_mask (reference pyflwdir/basins.py:25-64),
// core.inflow_idxs (core.py:485-497), regions.region_bounds (regions.py:57-125) and basins.subbasins_pfafstetter
// (basins.py:106-191).  The serial loops are restated in closed form ("The rest of BASINS"); the argument check
// of the list calls, the handle's links and sequence, the compaction and the list kernels are those of lists.h:
//   interbasin_mask   the second loop never reads the first loop's mask off a pit, so the result is: inside the region,
//                     the pit's basin holds a stream cell, and no edge "outside -> inside" on the path down to the pit.
//                     Two label fills (pfd_basins_dev): basin numbers (which pits have a stream cell), then the pits and
//                     the entry cells as seeds with 1-byte ids 1 = open / 2 = closed, the own seed winning.
//   inflow_idxs       `mask[idx_ds] = mask[idx0]` over seq[::-1] is a last-writer-wins over the children of a cell: the
//                     child that comes FIRST in the sequence.  First-child edges form disjoint chains that partition the
//                     sequence; one thread per headwater carries the flag down its chain and marks; the marks are listed
//                     by the stable compaction of the sequence, reversed.
//   basin_bounds      per label min / max row and column: labels of the run starts sorted + made unique (rocprim), then
//                     atomicMin / atomicMax of the run ends into the label's slot.
//   pfafstetter       classic stream order under uparea >= upa_min, capped at depth + 1; tributary list in sequence order;
//                     the reference's FIFO of labels is a breadth-first walk over depth and the labels of one depth touch
//                     disjoint cells: per depth one grouping step (4 largest tributaries per label by 4 rounds of
//                     atomicMax of the key / atomicMin of the list position = a stable sort on the negated key), the
//                     host turns the <= 4 entries per label into paint jobs in the reference's order (incl. its
//                     `idx1 not in idxs` test), one thread per label runs its jobs along idxs_us_main.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <numeric>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "common.h"
#include "lists.h"

namespace {

typedef unsigned long long ull;

__device__ __forceinline__ void amin(u32 *p, u32 v) { atomicMin(p, v); }
__device__ __forceinline__ void amin(u64 *p, u64 v) { atomicMin((ull *)p, (ull)v); }
__device__ __forceinline__ void amax(u64 *p, u64 v) { atomicMax((ull *)p, (ull)v); }

// ---- interbasin_mask ------------------------------------------------------------------------------------------------
// SEEDS = false: the pits; SEEDS = true: the pits and the entry cells (outside the region, draining into it)
template <bool SEEDS, class D>
__global__ void __launch_bounds__(256) k_mark_pits(const D d, u64 n, const u8 *__restrict__ region, u8 *__restrict__ mark,
                                                   ull *__restrict__ count) {
  for (u64 x0 = (u64)blockIdx.x * 256u; x0 < n; x0 += (u64)gridDim.x * 256u) {
    const u64 x = x0 + threadIdx.x;
    bool m = false;
    if (x < n && d.valid(x)) {
      const u64 y = d.down(x);
      m = y == x || (SEEDS && !region[x] && region[y]);
    }
    if (x < n) mark[x] = m ? 1 : 0;
    const u64 b = __ballot(m);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (ull)__popcll(b));
  }
}
__global__ void __launch_bounds__(256) k_iota_u32(u32 *__restrict__ ids, u64 k) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < k) ids[i] = (u32)(i + 1);
}
// has[b] = 1: basin number b holds a stream cell (cells off the sequence have basin number 0)
__global__ void __launch_bounds__(256) k_basin_has_stream(u64 n, const u8 *__restrict__ stream, const u32 *__restrict__ basin,
                                                          u8 *__restrict__ has) {
  for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < n; x += (u64)gridDim.x * 256u)
    if (stream[x] && basin[x]) has[basin[x]] = 1;
}
template <class D>
__global__ void __launch_bounds__(256) k_seed_ids(const D d, const i64 *__restrict__ seeds, u64 k, const u32 *__restrict__ basin,
                                                  const u8 *__restrict__ has, u8 *__restrict__ ids) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= k) return;
  const u64 x = (u64)seeds[i];
  const bool open = d.down(x) == x && (has == nullptr || has[basin[x]]);
  ids[i] = open ? 1 : 2;
}
__global__ void __launch_bounds__(256) k_interbasin_out(u64 n, const u8 *__restrict__ region, const u8 *__restrict__ stream,
                                                        const u8 *__restrict__ lab, u8 *__restrict__ out) {
  for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < n; x += (u64)gridDim.x * 256u) {
    const u8 l = lab[x];
    const bool m = l ? l == 1 : (stream == nullptr || stream[x]);
    out[x] = (m && region[x]) ? 1 : 0;
  }
}

template <class D>
static int interbasin_run(pfd_raster *h, const D &d, const u8 *region, const u8 *stream, u8 *out) {
  const u64 n = (u64)h->n;
  DevBuf mark, cnt, basin, has, seeds, ids, lab;
  PFDCHK(mark.alloc((size_t)n));
  PFDCHK(cnt.alloc(4 * sizeof(ull)));
  ull *c = cnt.as<ull>();
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(ull), h->stream));
  if (stream) {  // which pits have a stream cell in their basin: number the basins, scatter the stream flags
    pfd_seg_begin(h, "interbasin_pits");
    k_mark_pits<false, D><<<sweep_grid(n), 256, 0, h->stream>>>(d, n, region, mark.as<u8>(), c);
    KCHK();
    pfd_seg_end(h, 1);
    u64 np = 0;
    PFDCHK(read_count(h, c, &np));
    if (np >= 0xFFFFFFFFull) {
      pfd_set_error("interbasin_mask: %llu pits are more than the label fill takes", (ull)np);
      return PFD_EUNSUPPORTED;
    }
    PFDCHK(basin.alloc((size_t)n * sizeof(u32) + 64));
    PFDCHK(has.alloc((size_t)np + 1));
    HIPCHK(hipMemsetAsync(has.p, 0, (size_t)np + 1, h->stream));
    if (np) {
      PFDCHK(seeds.alloc((size_t)np * sizeof(i64)));
      PFDCHK(ids.alloc((size_t)np * sizeof(u32)));
      PFDCHK(select_marked(h, rocprim::counting_iterator<i64>(0), n, mark.as<u8>(), seeds.as<i64>(), c + 1));
      k_iota_u32<<<cdiv_u32(np, 256), 256, 0, h->stream>>>(ids.as<u32>(), np);
      KCHK();
    }
    PFDCHK(pfd_basins_dev(h, seeds.as<i64>(), ids.p, (u32)np, 4, basin.p));
    k_basin_has_stream<<<sweep_grid(n), 256, 0, h->stream>>>(n, stream, basin.as<u32>(), has.as<u8>());
    KCHK();
  }
  pfd_seg_begin(h, "interbasin_seeds");
  k_mark_pits<true, D><<<sweep_grid(n), 256, 0, h->stream>>>(d, n, region, mark.as<u8>(), c + 2);
  KCHK();
  pfd_seg_end(h, 1);
  u64 ns = 0;
  PFDCHK(read_count(h, c + 2, &ns));
  if (ns >= 0xFFFFFFFFull) {
    pfd_set_error("interbasin_mask: %llu seed cells are more than the label fill takes", (ull)ns);
    return PFD_EUNSUPPORTED;
  }
  PFDCHK(lab.alloc((size_t)n + 64));
  if (ns) {
    PFDCHK(seeds.alloc((size_t)ns * sizeof(i64)));
    PFDCHK(ids.alloc((size_t)ns));
    PFDCHK(select_marked(h, rocprim::counting_iterator<i64>(0), n, mark.as<u8>(), seeds.as<i64>(), c + 3));
    k_seed_ids<D><<<cdiv_u32(ns, 256), 256, 0, h->stream>>>(d, seeds.as<i64>(), ns, basin.as<u32>(),
                                                             stream ? has.as<u8>() : nullptr, ids.as<u8>());
    KCHK();
  }
  PFDCHK(pfd_basins_dev(h, seeds.as<i64>(), ids.p, (u32)ns, 1, lab.p));
  pfd_seg_begin(h, "interbasin_out");
  k_interbasin_out<<<sweep_grid(n), 256, 0, h->stream>>>(n, region, stream, lab.as<u8>(), out);
  KCHK();
  pfd_seg_end(h, 1);
  HIPCHK(hipStreamSynchronize(h->stream));  // (the temporaries are released on return)
  return PFD_OK;
}

// ---- inflow_idxs ----------------------------------------------------------------------------------------------------
// fc[p] = the smallest sequence position among the children of p (all-ones: none)
template <class D, class I>
__global__ void __launch_bounds__(256) k_first_child_pos(const D d, const I *__restrict__ seq, u64 m, I *__restrict__ fc) {
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < m; i += (u64)gridDim.x * 256u) {
    const u64 c = seq[i], p = d.down(c);
    if (p != c) amin(&fc[p], (I)i);
  }
}
template <class I>
__global__ void __launch_bounds__(256) k_pos_to_cell(const I *__restrict__ seq, u64 n, I *__restrict__ fc) {
  for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < n; x += (u64)gridDim.x * 256u) {
    const I p = fc[x];
    if (p != (I)~(I)0) fc[x] = seq[p];
  }
}
// one thread per headwater of the sequence: down its first-child chain, mask[c] = mask[f] && !(region[c] && !region[f])
template <class D, class I>
__global__ void __launch_bounds__(256) k_inflow_walk(const D d, const I *__restrict__ seq, u64 m, const I *__restrict__ fc,
                                                     const u8 *__restrict__ region, u8 *__restrict__ mark,
                                                     ull *__restrict__ count) {
  for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < m; i += (u64)gridDim.x * 256u) {
    u64 c = seq[i];
    if (fc[c] != (I)~(I)0) continue;  // has an upstream cell: another walk comes through, or stops, here
    bool flag = true, rc = region[c] != 0;
    u32 found = 0;
    for (;;) {
      const u64 p = d.down(c);
      if (p == c) break;  // a pit is never listed
      const bool rp = region[p] != 0, in = rp && !rc;
      if (flag && in) mark[c] = 1, ++found;
      if ((u64)fc[p] != c) break;  // p takes its flag from another child
      flag = flag && !in;
      c = p, rc = rp;
    }
    if (found) atomicAdd(count, (ull)found);
  }
}
template <class D, class I>
static int inflow_run(pfd_raster *h, const D &d, const I *seq, u64 m, const u8 *region, DevBuf &idx, u64 *k_out) {
  const u64 n = (u64)h->n;
  *k_out = 0;
  if (!m) return PFD_OK;
  DevBuf fc, mark, cnt, sel;
  PFDCHK(fc.alloc((size_t)n * sizeof(I)));
  PFDCHK(mark.alloc((size_t)n));
  PFDCHK(cnt.alloc(2 * sizeof(ull)));
  ull *c = cnt.as<ull>();
  HIPCHK(hipMemsetAsync(c, 0, 2 * sizeof(ull), h->stream));
  HIPCHK(hipMemsetAsync(fc.p, 0xFF, (size_t)n * sizeof(I), h->stream));
  HIPCHK(hipMemsetAsync(mark.p, 0, (size_t)n, h->stream));
  pfd_seg_begin(h, "inflow_first_child");
  k_first_child_pos<D, I><<<sweep_grid(m), 256, 0, h->stream>>>(d, seq, m, fc.as<I>());
  KCHK();
  k_pos_to_cell<I><<<sweep_grid(n), 256, 0, h->stream>>>(seq, n, fc.as<I>());
  KCHK();
  pfd_seg_end(h, 2);
  pfd_seg_begin(h, "inflow_walk");
  k_inflow_walk<D, I><<<sweep_grid(m), 256, 0, h->stream>>>(d, seq, m, fc.as<I>(), region, mark.as<u8>(), c);
  KCHK();
  pfd_seg_end(h, 1);
  u64 marked = 0;
  PFDCHK(read_count(h, c, &marked));
  if (!marked) return PFD_OK;
  PFDCHK(sel.alloc((size_t)marked * sizeof(I)));
  PFDCHK(idx.alloc((size_t)marked * sizeof(i64)));
  pfd_seg_begin(h, "inflow_list");
  PFDCHK(select_marked(h, seq, m, mark.as<u8>(), sel.as<I>(), c + 1));
  k_number<I><<<cdiv_u32(marked, 256), 256, 0, h->stream>>>(sel.as<I>(), marked, true, idx.as<i64>(), nullptr);
  KCHK();
  pfd_seg_end(h, 2);
  HIPCHK(hipStreamSynchronize(h->stream));
  *k_out = marked;
  return PFD_OK;
}

// ---- basin_bounds ---------------------------------------------------------------------------------------------------
// a run = cells of one label > 0 that follow each other within a row
template <class T>
__global__ void __launch_bounds__(256) k_run_starts(const T *__restrict__ v, u64 n, u64 ncol, u8 *__restrict__ mark,
                                                    ull *__restrict__ count) {
  for (u64 x0 = (u64)blockIdx.x * 256u; x0 < n; x0 += (u64)gridDim.x * 256u) {
    const u64 x = x0 + threadIdx.x;
    bool m = false;
    if (x < n) {
      const T a = v[x];
      m = a > T(0) && (x % ncol == 0 || v[x - 1] != a);
      mark[x] = m ? 1 : 0;
    }
    const u64 b = __ballot(m);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (ull)__popcll(b));
  }
}
// bounds = [rmin[k], rmax[k], cmin[k], cmax[k]]; only the two ends of a run touch them
template <class T>
__global__ void __launch_bounds__(256) k_bounds(const T *__restrict__ v, u64 n, u64 ncol, const T *__restrict__ lbs, u64 k,
                                                u64 *__restrict__ bounds) {
  for (u64 x = (u64)blockIdx.x * 256u + threadIdx.x; x < n; x += (u64)gridDim.x * 256u) {
    const T a = v[x];
    if (!(a > T(0))) continue;
    const u64 row = x / ncol, col = x - row * ncol;
    const bool first = col == 0 || v[x - 1] != a, last = col == ncol - 1 || v[x + 1] != a;
    if (!first && !last) continue;
    u64 lo = 0, hi = k;  // lower bound of a in lbs (sorted, unique, holds a)
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (lbs[mid] < a) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= k) continue;
    if (first) amin(&bounds[lo], row), amax(&bounds[k + lo], row), amin(&bounds[2 * k + lo], col);
    if (last) amax(&bounds[3 * k + lo], col);
  }
}

template <class T>
static int bounds_t(pfd_raster *h, const void *labels, void *lbs_out, i64 *bounds_out, i64 cap, i64 *k_out, int memspace) {
  const u64 n = (u64)h->n, ncol = (u64)h->ncol;
  InArg v;
  PFDCHK(v.bind(labels, (size_t)n * sizeof(T), memspace, h->stream));
  DevBuf mark, cnt, starts, lb, lb2, uq, tmp, bounds;
  PFDCHK(mark.alloc((size_t)n));
  PFDCHK(cnt.alloc(3 * sizeof(ull)));
  ull *c = cnt.as<ull>();
  HIPCHK(hipMemsetAsync(c, 0, 3 * sizeof(ull), h->stream));
  pfd_seg_begin(h, "bounds_runs");
  k_run_starts<T><<<sweep_grid(n), 256, 0, h->stream>>>((const T *)v.dev, n, ncol, mark.as<u8>(), c);
  KCHK();
  pfd_seg_end(h, 1);
  u64 ns = 0;
  PFDCHK(read_count(h, c, &ns));
  *k_out = 0;
  if (!ns) return PFD_OK;
  PFDCHK(starts.alloc((size_t)ns * sizeof(i64)));
  PFDCHK(lb.alloc((size_t)ns * sizeof(T)));
  PFDCHK(lb2.alloc((size_t)ns * sizeof(T)));
  PFDCHK(uq.alloc((size_t)ns * sizeof(T)));
  pfd_seg_begin(h, "bounds_labels");
  PFDCHK(select_marked(h, rocprim::counting_iterator<i64>(0), n, mark.as<u8>(), starts.as<i64>(), c + 1));
  k_gather<T><<<cdiv_u32(ns, 256), 256, 0, h->stream>>>(starts.as<i64>(), ns, (const T *)v.dev, lb.as<T>());
  KCHK();
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::radix_sort_keys(p, b, lb.as<T>(), lb2.as<T>(), (size_t)ns, 0u, (unsigned)(8 * sizeof(T)), h->stream);
  }));
  HIPCHK(hipStreamSynchronize(h->stream));
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::unique(p, b, lb2.as<T>(), uq.as<T>(), c + 2, (size_t)ns, rocprim::equal_to<T>(), h->stream);
  }));
  pfd_seg_end(h, 4);
  u64 k = 0;
  PFDCHK(read_count(h, c + 2, &k));
  *k_out = (i64)k;
  if ((i64)k > cap) return PFD_OK;
  PFDCHK(bounds.alloc((size_t)k * 4 * sizeof(u64)));
  HIPCHK(hipMemsetAsync(bounds.p, 0, (size_t)k * 4 * sizeof(u64), h->stream));
  HIPCHK(hipMemsetAsync(bounds.p, 0xFF, (size_t)k * sizeof(u64), h->stream));                       // rmin
  HIPCHK(hipMemsetAsync(bounds.as<u64>() + 2 * k, 0xFF, (size_t)k * sizeof(u64), h->stream));  // cmin
  pfd_seg_begin(h, "bounds_reduce");
  k_bounds<T><<<sweep_grid(n), 256, 0, h->stream>>>((const T *)v.dev, n, ncol, uq.as<T>(), k, bounds.as<u64>());
  KCHK();
  pfd_seg_end(h, 1);
  PFDCHK(give_list(h, uq.p, (size_t)k * sizeof(T), lbs_out, memspace));
  return give_list(h, bounds.p, (size_t)k * 4 * sizeof(u64), bounds_out, memspace);
}

// ---- subbasins_pfafstetter ------------------------------------------------------------------------------------------
// order-preserving 64-bit key of an upstream area: a larger area has a larger key, -0.0 == 0.0, NaN is the smallest
// (np.argsort puts the NaNs of the negated areas last)
template <class T>
__device__ __forceinline__ u64 okey(T a) {
  if (std::is_floating_point<T>::value) {
    double x = (double)a;
    if (x != x) return 0;
    if (x == 0.0) x = 0.0;
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  }
  return (u64)(i64)a ^ 0x8000000000000000ull;
}
template <class T>
__global__ void __launch_bounds__(256) k_upa_mask(const T *__restrict__ upa, u32 n, double upa_min, u8 *__restrict__ mask) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n) return;
  // (numpy compares a float array with a Python float in the array's dtype, an integer array in float64)
  mask[x] = (std::is_floating_point<T>::value ? upa[x] >= (T)upa_min : (double)upa[x] >= upa_min) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_cap_order(u8 *__restrict__ strord, u32 n, u32 max_order) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x < n && strord[x] > max_order) strord[x] = 0;
}
template <class D>
__global__ void __launch_bounds__(256) k_mark_trib(const D d, u32 n, const u8 *__restrict__ strord, u8 *__restrict__ mark,
                                                   ull *__restrict__ count) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  bool m = false;
  if (x < n && d.valid(x)) {
    const u8 s = strord[x];
    m = s > 0 && s > strord[d.down(x)];
  }
  if (x < n) mark[x] = m ? 1 : 0;
  const u64 b = __ballot(m);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (ull)__popcll(b));
}
// a given idxs_us_main must lead strictly upstream, or a paint walk would not end
template <class D>
__global__ void __launch_bounds__(256) k_check_usm(const D d, u32 n, const i64 *__restrict__ usm, ull *__restrict__ bad) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x >= n || !d.valid(x)) return;
  const i64 u = usm[x];
  if (u == -1) return;
  if (u < 0 || u >= (i64)n || u == (i64)x || !d.valid((u64)u) || d.down((u64)u) != x) atomicAdd(bad, 1ull);
}
__global__ void __launch_bounds__(256) k_nonzero(const i32 *__restrict__ v, u32 n, u8 *__restrict__ mark, ull *__restrict__ count) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  const bool m = x < n && v[x] != 0;
  if (x < n) mark[x] = m ? 1 : 0;
  const u64 b = __ballot(m);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (ull)__popcll(b));
}
__global__ void __launch_bounds__(256) k_mod(i32 *__restrict__ v, u32 n, i32 m) {
  const u32 x = blockIdx.x * 256u + threadIdx.x;
  if (x < n) v[x] = v[x] % m;
}
__global__ void __launch_bounds__(256) k_paint_pits(const i64 *__restrict__ pits, const i32 *__restrict__ labels, u32 k,
                                                    const i64 *__restrict__ usm, const u8 *__restrict__ strord,
                                                    i32 *__restrict__ branch) {
  const u32 t = blockIdx.x * 256u + threadIdx.x;
  if (t >= k) return;
  i64 x = pits[t];
  const i32 l = labels[t];
  branch[x] = l;
  for (;;) {
    x = usm[x];
    if (x < 0 || strord[x] == 0) break;
    branch[x] = l;
  }
}
struct PaintJob {
  i64 start;
  i32 label, old;  // old == 0: a sub-basin (up the main stem while strord > 0); else an inter-basin (while the label is `old`)
};
// one thread per label of the depth: its jobs in the reference's order (the labels of one depth touch disjoint cells)
__global__ void __launch_bounds__(64) k_paint_jobs(const PaintJob *__restrict__ jobs, const u32 *__restrict__ off, u32 nl,
                                                   const i64 *__restrict__ usm, const u8 *__restrict__ strord,
                                                   i32 *__restrict__ branch) {
  const u32 t = blockIdx.x * 64u + threadIdx.x;
  if (t >= nl) return;
  for (u32 e = off[t]; e < off[t + 1]; ++e) {
    const PaintJob j = jobs[e];
    i64 x = j.start;
    branch[x] = j.label;
    for (;;) {
      x = usm[x];
      if (x < 0) break;
      if (j.old == 0 ? strord[x] == 0 : branch[x] != j.old) break;
      branch[x] = j.label;
    }
  }
}
// slot[j] = the place in the depth's label list of the label that tributary j is a candidate of (all-ones: none)
template <class D, class I>
__global__ void __launch_bounds__(256) k_candidates(const D d, const I *__restrict__ trib, u64 nt, const i32 *__restrict__ branch,
                                                    const i32 *__restrict__ labs, const u32 *__restrict__ labs_slot, u32 nl,
                                                    u32 *__restrict__ slot) {
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  if (j >= nt) return;
  const u64 x = trib[j];
  u32 s = 0xFFFFFFFFu;
  if (branch[x] == 0) {
    const i32 l = branch[d.down(x)];
    u32 lo = 0, hi = nl;
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (labs[mid] < l) lo = mid + 1;
      else hi = mid;
    }
    if (l != 0 && lo < nl && labs[lo] == l) s = labs_slot[lo];
  }
  slot[j] = s;
}
// round r of "the 4 largest, ties in list order": ARG = false: kmax[s] = the largest key among the candidates of s not
// taken yet; ARG = true: sel[4 s + r] = the smallest list position among those that hold it
template <bool ARG, class T, class I>
__global__ void __launch_bounds__(256) k_round(const I *__restrict__ trib, u64 nt, const u32 *__restrict__ slot,
                                               const T *__restrict__ upa, int r, u64 *__restrict__ kmax, u64 *__restrict__ sel) {
  const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
  if (j >= nt) return;
  const u32 s = slot[j];
  if (s == 0xFFFFFFFFu) return;
  for (int q = 0; q < r; ++q)
    if (sel[4 * (u64)s + q] == j) return;
  const u64 key = okey<T>(upa[trib[j]]);
  if (!ARG) amax(&kmax[s], key);
  else if (key == kmax[s]) amin(&sel[4 * (u64)s + r], j);
}
template <class D, class T, class I>
__global__ void __launch_bounds__(256) k_gather_sel(const D d, const I *__restrict__ trib, const u64 *__restrict__ sel, u64 ne,
                                                    const T *__restrict__ upa, const i64 *__restrict__ usm, i64 *__restrict__ idx,
                                                    u64 *__restrict__ key2, i64 *__restrict__ idx1) {
  const u64 e = (u64)blockIdx.x * 256u + threadIdx.x;
  if (e >= ne) return;
  const u64 j = sel[e];
  if (j == ~0ull) {
    idx[e] = -1, key2[e] = 0, idx1[e] = -1;
    return;
  }
  const u64 x = trib[j], y = d.down(x);
  idx[e] = (i64)x, key2[e] = okey<T>(upa[y]), idx1[e] = usm[y];
}

template <class V>
static int upload(pfd_raster *h, DevBuf &b, const std::vector<V> &v) {
  PFDCHK(b.alloc(std::max<size_t>(v.size() * sizeof(V), 16)));
  if (!v.empty()) HIPCHK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}
template <class V>
static int download(pfd_raster *h, const void *dev, std::vector<V> &v, size_t k) {
  v.resize(k);
  if (k) HIPCHK(hipMemcpyAsync(v.data(), dev, k * sizeof(V), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

// everything after the stream order: tributaries, the depths, the final fill.  `out` = the int32 map; `idxs` = the
// outlets in the reference's append order
template <class T, class D, class I>
static int pfaf_run(pfd_raster *h, const D &d, const I *seq, u64 m, const T *upa, const i64 *usm, const u8 *strord,
                    const std::vector<i64> &pits, int depth, i32 *out, std::vector<i64> &idxs) {
  const u32 n = h->geo.n;
  i64 p10 = 1;
  for (int q = 0; q < depth; ++q) p10 *= 10;
  i64 pfaf0 = 1;
  for (i64 q = 10; q < p10; q *= 10) pfaf0 += q;
  if (pfaf0 + ((i64)pits.size() + 1) * p10 > 0x7FFFFFFFll) {
    pfd_set_error("subbasins_pfafstetter: the labels of %lld pits at depth %d do not fit the int32 map", (long long)pits.size(),
                  depth);
    return PFD_EUNSUPPORTED;
  }
  DevBuf mark, cnt, trib, branch;
  PFDCHK(mark.alloc((size_t)n));
  PFDCHK(cnt.alloc(4 * sizeof(ull)));
  ull *c = cnt.as<ull>();
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(ull), h->stream));
  // tributaries in sequence order (basins._tributaries)
  pfd_seg_begin(h, "pfaf_tributaries");
  k_mark_trib<D><<<cdiv_u32(n, 256), 256, 0, h->stream>>>(d, n, strord, mark.as<u8>(), c);
  KCHK();
  pfd_seg_end(h, 1);
  u64 nt = 0;
  PFDCHK(read_count(h, c, &nt));
  if (nt && m) {
    PFDCHK(trib.alloc((size_t)nt * sizeof(I)));
    PFDCHK(select_marked(h, seq, m, mark.as<u8>(), trib.as<I>(), c + 1));
    PFDCHK(read_count(h, c + 1, &nt));
  } else {
    nt = 0;
  }
  // the pits' labels up their main stems
  PFDCHK(branch.alloc((size_t)n * sizeof(i32)));
  HIPCHK(hipMemsetAsync(branch.p, 0, (size_t)n * sizeof(i32), h->stream));
  std::vector<i32> labs(pits.size());
  std::unordered_set<i64> seen;
  idxs.clear();
  for (size_t i = 0; i < pits.size(); ++i) {
    labs[i] = (i32)(pfaf0 + ((i64)i + 1) * p10);
    idxs.push_back(pits[i]);
    seen.insert(pits[i]);
  }
  {
    DevBuf dp, dl;
    PFDCHK(upload(h, dp, pits));
    PFDCHK(upload(h, dl, labs));
    pfd_seg_begin(h, "pfaf_paint_pits");
    if (!pits.empty()) {
      k_paint_pits<<<cdiv_u32(pits.size(), 256), 256, 0, h->stream>>>(dp.as<i64>(), dl.as<i32>(), (u32)pits.size(), usm, strord,
                                                                      branch.as<i32>());
      KCHK();
    }
    pfd_seg_end(h, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  DevBuf slot;
  PFDCHK(slot.alloc(std::max<size_t>((size_t)nt * sizeof(u32), 16)));
  for (int d0 = 1; d0 <= depth && !labs.empty() && nt; ++d0) {
    const u32 nl = (u32)labs.size();
    i64 step = 1;  // 10 ** (depth - d0)
    for (int q = d0; q < depth; ++q) step *= 10;
    // the depth's labels sorted, with their place in the FIFO
    std::vector<u32> order(nl);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return labs[a] < labs[b]; });
    std::vector<i32> sorted(nl);
    for (u32 q = 0; q < nl; ++q) sorted[q] = labs[order[q]];
    DevBuf dlab, dslot, kmax, sel, gidx, gkey, gidx1;
    PFDCHK(upload(h, dlab, sorted));
    PFDCHK(upload(h, dslot, order));
    PFDCHK(kmax.alloc((size_t)nl * sizeof(u64)));
    PFDCHK(sel.alloc((size_t)nl * 4 * sizeof(u64)));
    PFDCHK(gidx.alloc((size_t)nl * 4 * sizeof(i64)));
    PFDCHK(gkey.alloc((size_t)nl * 4 * sizeof(u64)));
    PFDCHK(gidx1.alloc((size_t)nl * 4 * sizeof(i64)));
    HIPCHK(hipMemsetAsync(sel.p, 0xFF, (size_t)nl * 4 * sizeof(u64), h->stream));
    pfd_seg_begin(h, "pfaf_group");
    const u32 gt = cdiv_u32(nt, 256);
    k_candidates<D, I><<<gt, 256, 0, h->stream>>>(d, trib.as<I>(), nt, branch.as<i32>(), dlab.as<i32>(), dslot.as<u32>(), nl,
                                                  slot.as<u32>());
    KCHK();
    for (int r = 0; r < 4; ++r) {
      HIPCHK(hipMemsetAsync(kmax.p, 0, (size_t)nl * sizeof(u64), h->stream));
      k_round<false, T, I><<<gt, 256, 0, h->stream>>>(trib.as<I>(), nt, slot.as<u32>(), upa, r, kmax.as<u64>(), sel.as<u64>());
      KCHK();
      k_round<true, T, I><<<gt, 256, 0, h->stream>>>(trib.as<I>(), nt, slot.as<u32>(), upa, r, kmax.as<u64>(), sel.as<u64>());
      KCHK();
    }
    k_gather_sel<D, T, I><<<cdiv_u32((u64)nl * 4, 256), 256, 0, h->stream>>>(d, trib.as<I>(), sel.as<u64>(), (u64)nl * 4, upa, usm,
                                                                             gidx.as<i64>(), gkey.as<u64>(), gidx1.as<i64>());
    KCHK();
    pfd_seg_end(h, 14);
    std::vector<i64> hidx, hidx1;
    std::vector<u64> hkey;
    PFDCHK(download(h, gidx.p, hidx, (size_t)nl * 4));
    PFDCHK(download(h, gkey.p, hkey, (size_t)nl * 4));
    PFDCHK(download(h, gidx1.p, hidx1, (size_t)nl * 4));
    // the reference's loop body per label, in FIFO order: the outlet list, the next depth's labels, the paint jobs
    std::vector<i32> next;
    std::vector<PaintJob> jobs;
    std::vector<u32> off(nl + 1, 0);
    for (u32 s = 0; s < nl; ++s) {
      int e[4], ne = 0;
      for (int r = 0; r < 4; ++r)
        if (hidx[4 * (size_t)s + r] >= 0) e[ne++] = r;
      // down- to upstream: descending area of the downstream cell, ties in the order of the first sort
      std::stable_sort(e, e + ne, [&](int a, int b) { return hkey[4 * (size_t)s + a] > hkey[4 * (size_t)s + b]; });
      const i64 lab0 = labs[s];
      i64 int_ds = lab0;
      for (int i = 0; i < ne; ++i) {
        const i64 idx = hidx[4 * (size_t)s + e[i]], idx1 = hidx1[4 * (size_t)s + e[i]];
        if (idx1 < 0) {
          pfd_set_error("subbasins_pfafstetter: idxs_us_main has no main upstream cell where cell %lld joins", (long long)idx);
          return PFD_EINVAL;
        }
        idxs.push_back(idx);
        seen.insert(idx);
        const i64 sub = lab0 + ((i64)i * 2 + 1) * step;
        jobs.push_back(PaintJob{idx, (i32)sub, 0});
        if (d0 < depth) next.push_back((i32)sub);
        if (!seen.count(idx1)) {
          idxs.push_back(idx1);
          seen.insert(idx1);
          const i64 pint = lab0 + ((i64)i + 1) * 2 * step;
          jobs.push_back(PaintJob{idx1, (i32)pint, (i32)int_ds});
          int_ds = pint;
          if (d0 < depth) next.push_back((i32)pint);
        }
      }
      off[s + 1] = (u32)jobs.size();
    }
    if (!jobs.empty()) {
      DevBuf dj, doff;
      PFDCHK(upload(h, dj, jobs));
      PFDCHK(upload(h, doff, off));
      pfd_seg_begin(h, "pfaf_paint");
      k_paint_jobs<<<cdiv_u32(nl, 64), 64, 0, h->stream>>>(dj.as<PaintJob>(), doff.as<u32>(), nl, usm, strord, branch.as<i32>());
      KCHK();
      pfd_seg_end(h, 1);
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    labs.swap(next);
  }
  // core.fillnodata_upstream(pfaf_branch, 0) % 10 ** depth: the painted cells are the seeds of one label fill
  HIPCHK(hipMemsetAsync(c + 2, 0, 2 * sizeof(ull), h->stream));
  k_nonzero<<<cdiv_u32(n, 256), 256, 0, h->stream>>>(branch.as<i32>(), n, mark.as<u8>(), c + 2);
  KCHK();
  u64 ks = 0;
  PFDCHK(read_count(h, c + 2, &ks));
  DevBuf sidx, sids;
  if (ks) {
    PFDCHK(sidx.alloc((size_t)ks * sizeof(i64)));
    PFDCHK(sids.alloc((size_t)ks * sizeof(i32)));
    PFDCHK(select_marked(h, rocprim::counting_iterator<i64>(0), (u64)n, mark.as<u8>(), sidx.as<i64>(), c + 3));
    k_gather<i32><<<cdiv_u32(ks, 256), 256, 0, h->stream>>>(sidx.as<i64>(), ks, branch.as<i32>(), sids.as<i32>());
    KCHK();
  }
  PFDCHK(pfd_basins_dev(h, sidx.as<i64>(), sids.p, (u32)ks, 4, out));
  k_mod<<<cdiv_u32(n, 256), 256, 0, h->stream>>>(out, n, (i32)p10);
  KCHK();
  HIPCHK(hipStreamSynchronize(h->stream));
  return PFD_OK;
}

template <class T>
static int pfaf_t(pfd_raster *h, const void *uparea, double upa_min, int depth, const i64 *idxs_us_main, const i64 *pits_host,
                  i64 npits, int idx_dtype, void *idxs_out, i64 cap, i64 *k_out, i32 *map_out, int memspace) {
  const u32 n = h->geo.n;
  InArg a, u;
  PFDCHK(a.bind(uparea, (size_t)n * sizeof(T), memspace, h->stream));
  PFDCHK(u.bind(idxs_us_main, (size_t)n * sizeof(i64), memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(map_out, (size_t)n * sizeof(i32), memspace));
  DevBuf cells, usm, mask, strord;
  const T *upa = (const T *)a.dev;
  const i64 *us = (const i64 *)u.dev;
  if (!upa || !us) {  // the upstream cell count: the default area, and what the main upstream cell is chosen by
    PFDCHK(cells.alloc((size_t)n * sizeof(i32)));
    PFDCHK(pfd_upstream_area_cell(h, cells.as<i32>(), PFD_DEVICE));
  }
  if (!us) {
    PFDCHK(usm.alloc((size_t)n * sizeof(i64)));
    PFDCHK(pfd_main_upstream(h, PFD_I32, cells.p, 0.0, PFD_I64, usm.p, PFD_DEVICE));
    us = usm.as<i64>();
  }
  if (!upa) upa = (const T *)cells.p;  // (T is int32 then)
  PFDCHK(mask.alloc((size_t)n));
  PFDCHK(strord.alloc((size_t)n + 64));
  k_upa_mask<T><<<cdiv_u32(n, 256), 256, 0, h->stream>>>(upa, n, upa_min, mask.as<u8>());
  KCHK();
  PFDCHK(pfd_stream_order_classic(h, PFD_I64, us, mask.as<u8>(), strord.as<u8>(), PFD_DEVICE));
  k_cap_order<<<cdiv_u32(n, 256), 256, 0, h->stream>>>(strord.as<u8>(), n, (u32)depth + 1u);
  KCHK();
  std::vector<i64> pits(pits_host, pits_host + npits), idxs;
  const bool given = u.dev != nullptr;
  PFDCHK(pfd_with_graph(h, [&](auto d, auto seq, u64 m) -> int {
    typedef decltype(d) D;
    typedef typename std::remove_cv<typename std::remove_pointer<decltype(seq)>::type>::type I;
    if (given) {
      DevBuf bad;
      PFDCHK(bad.alloc(sizeof(ull)));
      HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(ull), h->stream));
      k_check_usm<D><<<cdiv_u32(n, 256), 256, 0, h->stream>>>(d, n, us, bad.as<ull>());
      KCHK();
      u64 nbad = 0;
      PFDCHK(read_count(h, bad.as<ull>(), &nbad));
      if (nbad) {
        pfd_set_error("subbasins_pfafstetter: idxs_us_main holds %llu entries that are no upstream cell of their cell", (ull)nbad);
        return PFD_EINVAL;
      }
    }
    return pfaf_run<T, D, I>(h, d, seq, m, upa, us, strord.as<u8>(), pits, depth, (i32 *)o.dev, idxs);
  }));
  *k_out = (i64)idxs.size();
  if ((i64)idxs.size() <= cap && !idxs.empty()) {
    if (memspace == PFD_DEVICE) {
      DevBuf di;
      PFDCHK(upload(h, di, idxs));
      PFDCHK(give_idxs(h, di.as<i64>(), idxs.size(), idx_dtype, idxs_out, memspace));
    } else {  // (the list was built on the host)
      PFDCHK(pfd_dispatch_idx(idx_dtype, "subbasins_pfafstetter", [&](auto itag) -> int {
        typedef typename decltype(itag)::type O;
        for (size_t i = 0; i < idxs.size(); ++i) ((O *)idxs_out)[i] = (O)idxs[i];
        return PFD_OK;
      }));
    }
  }
  return o.finish(h->stream);
}

}  // namespace

extern "C" int pfd_interbasin_mask(pfd_raster *h, const uint8_t *region, const uint8_t *stream, uint8_t *out, int memspace) {
  PFDCHK(pfd_check_handle(h));
  PFDCHK(pfd_require_unblocked(h, "interbasin_mask"));
  if (!region || !out) {
    pfd_set_error("interbasin_mask: NULL region or out");
    return PFD_EINVAL;
  }
  pfd_seg_clear(h);
  InArg r, s;
  PFDCHK(r.bind(region, (size_t)h->n, memspace, h->stream));
  PFDCHK(s.bind(stream, (size_t)h->n, memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(out, (size_t)h->n, memspace));
  // (order-independent: the links alone, no sequence)
  PFDCHK(pfd_with_links(h, [&](auto d) { return interbasin_run(h, d, (const u8 *)r.dev, (const u8 *)s.dev, (u8 *)o.dev); }));
  return o.finish(h->stream);
}

extern "C" int pfd_inflow_idxs(pfd_raster *h, const uint8_t *region, int idx_dtype, void *idxs_out, int64_t cap,
                               int64_t *k_out, int memspace) {
  PFDCHK(pfd_check_list_args(h, "inflow_idxs", region, idx_dtype, idxs_out, cap, k_out));
  InArg r;
  PFDCHK(r.bind(region, (size_t)h->n, memspace, h->stream));
  DevBuf idx;
  u64 k = 0;
  PFDCHK(pfd_with_graph(h, [&](auto d, auto seq, u64 m) -> int {
    typedef typename std::remove_cv<typename std::remove_pointer<decltype(seq)>::type>::type I;
    return inflow_run<decltype(d), I>(h, d, seq, m, (const u8 *)r.dev, idx, &k);
  }));
  *k_out = (i64)k;
  if ((i64)k <= cap) PFDCHK(give_idxs(h, idx.as<i64>(), k, idx_dtype, idxs_out, memspace));
  return PFD_OK;
}

extern "C" int pfd_basin_bounds(pfd_raster *h, int dtype, const void *labels, void *lbs_out, int64_t *bounds_out, int64_t cap,
                                int64_t *k_out, int memspace) {
  PFDCHK(pfd_check_handle(h));
  if (!labels || !k_out || cap < 0 || (cap > 0 && (!lbs_out || !bounds_out))) {
    pfd_set_error("basin_bounds: bad arguments (NULL pointer, cap=%lld)", (long long)cap);
    return PFD_EINVAL;
  }
  pfd_seg_clear(h);
  switch (dtype) {
    case PFD_I32: return bounds_t<i32>(h, labels, lbs_out, bounds_out, cap, k_out, memspace);
    case PFD_U32: return bounds_t<u32>(h, labels, lbs_out, bounds_out, cap, k_out, memspace);
    case PFD_I64: return bounds_t<i64>(h, labels, lbs_out, bounds_out, cap, k_out, memspace);
    case PFD_U64: return bounds_t<u64>(h, labels, lbs_out, bounds_out, cap, k_out, memspace);
    default:
      pfd_set_error("basin_bounds: label dtype code %d is not supported (int32, uint32, int64, uint64)", dtype);
      return PFD_EUNSUPPORTED;
  }
}

extern "C" int pfd_subbasins_pfafstetter(pfd_raster *h, int dtype, const void *uparea, double upa_min, int depth,
                                         const int64_t *idxs_us_main, const int64_t *idxs_pit, int64_t npits, int idx_dtype,
                                         void *idxs_out, int64_t cap, int64_t *k_out, int32_t *map_out, int memspace) {
  PFDCHK(pfd_check_list_args(h, "subbasins_pfafstetter", map_out, idx_dtype, idxs_out, cap, k_out));
  if (pfd_wide_cells(h)) {
    pfd_set_error("subbasins_pfafstetter: pfd_main_upstream and pfd_stream_order_classic have no one-handle form beyond "
                  "2^32 - 2 cells (%lld cells)", (long long)h->n);
    return PFD_EUNSUPPORTED;
  }
  if (!h->gen) PFDCHK(pfd_require_whole(h, "subbasins_pfafstetter"));
  if (depth < 1 || depth > 8 || npits < 0 || (npits > 0 && !idxs_pit)) {
    pfd_set_error("subbasins_pfafstetter: bad arguments (depth=%d must be 1 .. 8, npits=%lld)", depth, (long long)npits);
    return PFD_EINVAL;
  }
  for (i64 i = 0; i < npits; ++i)
    if (idxs_pit[i] < 0 || idxs_pit[i] >= h->n) {
      pfd_set_error("subbasins_pfafstetter: pit index %lld outside the raster", (long long)idxs_pit[i]);
      return PFD_EINVAL;
    }
  if (!uparea) return pfaf_t<i32>(h, nullptr, upa_min, depth, idxs_us_main, idxs_pit, npits, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
  return pfd_dispatch_payload(dtype, "subbasins_pfafstetter", [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    return pfaf_t<T>(h, uparea, upa_min, depth, idxs_us_main, idxs_pit, npits, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
  });
}
