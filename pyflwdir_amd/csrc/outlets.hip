// outlets.hip — outlets derived from the network itself: basins.subbasins_streamorder (reference pyflwdir/basins.py:67-103),
// core.outflow_idxs (core.py:501-514) and regions.region_outlets (regions.py:129-163).
//
// The three serial loops of the reference are one primitive:
//   mark    one thread per cell decides from the cell's value and its downstream cell's value whether it is an outlet;
//   list    the marked cells in the order of core.idxs_seq — a stable compaction OF THE SEQUENCE (rocprim select with the
//           mark as predicate), so a cell that is not in the sequence (on or above a cycle) is never listed, as in the
//           reference, whose loops run over `seq`; two of the loops walk the sequence backwards: the list is reversed;
//   fill    (sub-basins) the list positions + 1 are the labels of the label query behind pfd_basins (pfd_basins_dev):
//           core.fillnodata_upstream over nested outlets is "the first outlet on the downstream path".
// outflow_idxs has one more step: its `mask`, inherited from the downstream cell and cleared at every listed cell, says
// "no listed cell further down the path" — and since the lowest candidate of a path is always listed, that is "no
// CANDIDATE further down": one label fill of the candidate flags, then every candidate looks at its downstream cell.
// The sequence comes from the engine the handle already has (pfd_with_graph, lists.h) and never leaves the device; the
// argument check, the compaction and the list kernels are those of lists.h.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "lists.h"

namespace {

enum { R_STO = 0, R_REGION = 1, R_LABEL = 2 };

template <class T>
__device__ __forceinline__ bool at_least(T a, i64 m) {
  if (std::is_unsigned<T>::value) return m <= 0 || (u64)a >= (u64)m;
  return (i64)a >= m;
}

// mark[x] = the cell-local rule; *count += marked cells (one atomic per wave that holds any)
template <int RULE, class T, class D>
__global__ void __launch_bounds__(256) k_mark(const D d, u64 n, const T *__restrict__ v, i64 min_sto, u8 *__restrict__ mark,
                                              unsigned long long *__restrict__ count) {
  // (grid-stride in whole workgroups: n may exceed the 2^32 threads one launch dimension runs)
  for (u64 x0 = (u64)blockIdx.x * 256u; x0 < n; x0 += (u64)gridDim.x * 256u) {
    const u64 x = x0 + threadIdx.x;
    bool m = false;
    if (x < n && d.valid(x)) {
      const u64 y = d.down(x);
      const T a = v[x];
      if (RULE == R_STO) m = at_least<T>(a, min_sto) && (y == x || v[y] != a);
      else if (RULE == R_REGION) m = a != T(0) && (y == x || v[y] == T(0));
      else m = a > T(0) && (y == x || v[y] != a);
    }
    if (x < n) mark[x] = m ? 1 : 0;
    const u64 b = __ballot(m);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
  }
}
// outflow_idxs: a candidate with a candidate at or below its downstream cell (lab != 0 there) is dropped
template <class D>
__global__ void __launch_bounds__(256) k_drop_shadowed(const D d, u64 n, const u8 *__restrict__ lab, u8 *__restrict__ mark,
                                                       unsigned long long *__restrict__ count) {
  for (u64 x0 = (u64)blockIdx.x * 256u; x0 < n; x0 += (u64)gridDim.x * 256u) {
    const u64 x = x0 + threadIdx.x;
    bool m = false;
    if (x < n && mark[x]) {
      const u64 y = d.down(x);
      m = y == x || lab[y] == 0;
      if (!m) mark[x] = 0;
    }
    const u64 b = __ballot(m);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
  }
}
struct Outlets {  // the numbered list on the device
  DevBuf idx, ids;  // k x i64 cells in the reference's list order, k x u32 numbers 1..k
  u64 k = 0;
};

template <int RULE, class T, class D, class I>
static int outlets_run(pfd_raster *h, const D &d, const I *seq, u64 m, const T *v, i64 min_sto, bool reversed, Outlets &R) {
  const u64 n = (u64)h->n;
  DevBuf mark, cnt;
  PFDCHK(mark.alloc((size_t)n));
  PFDCHK(cnt.alloc(4 * sizeof(unsigned long long)));
  unsigned long long *c = cnt.as<unsigned long long>();
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(unsigned long long), h->stream));
  pfd_seg_begin(h, "outlets_mark");
  k_mark<RULE, T, D><<<sweep_grid(n), 256, 0, h->stream>>>(d, n, v, min_sto, mark.as<u8>(), c);
  KCHK();
  pfd_seg_end(h, 1);
  u64 marked = 0;
  PFDCHK(read_count(h, c, &marked));
  if (RULE == R_REGION && marked) {
    if (marked >= 0xFFFFFFFFull) {
      pfd_set_error("outflow_idxs: %llu candidate cells are more than the label fill takes", (unsigned long long)marked);
      return PFD_EUNSUPPORTED;
    }
    DevBuf cand, ones, lab;
    PFDCHK(cand.alloc((size_t)marked * sizeof(i64)));
    PFDCHK(ones.alloc((size_t)marked));
    PFDCHK(lab.alloc((size_t)n + 64));
    PFDCHK(select_marked(h, rocprim::counting_iterator<i64>(0), n, mark.as<u8>(), cand.as<i64>(), c + 1));
    HIPCHK(hipMemsetAsync(ones.p, 1, (size_t)marked, h->stream));
    PFDCHK(pfd_basins_dev(h, cand.as<i64>(), ones.p, (u32)marked, 1, lab.p));
    pfd_seg_begin(h, "outlets_drop_shadowed");
    k_drop_shadowed<D><<<sweep_grid(n), 256, 0, h->stream>>>(d, n, lab.as<u8>(), mark.as<u8>(), c + 2);
    KCHK();
    pfd_seg_end(h, 1);
    PFDCHK(read_count(h, c + 2, &marked));
  }
  R.k = 0;
  if (!marked || !m) return PFD_OK;
  DevBuf sel;
  PFDCHK(sel.alloc((size_t)marked * sizeof(I)));
  pfd_seg_begin(h, "outlets_list");
  PFDCHK(select_marked(h, seq, m, mark.as<u8>(), sel.as<I>(), c + 3));
  PFDCHK(read_count(h, c + 3, &R.k));
  if (R.k) {
    PFDCHK(R.idx.alloc((size_t)R.k * sizeof(i64)));
    PFDCHK(R.ids.alloc((size_t)R.k * sizeof(u32)));
    k_number<I><<<cdiv_u32(R.k, 256), 256, 0, h->stream>>>(sel.as<I>(), R.k, reversed, R.idx.as<i64>(), R.ids.as<u32>());
    KCHK();
  }
  pfd_seg_end(h, 3);
  HIPCHK(hipStreamSynchronize(h->stream));  // (`sel` and `mark` are released on return)
  return PFD_OK;
}

template <class T>
static int streamorder_t(pfd_raster *h, const void *strord, i64 min_sto, int idx_dtype, void *idxs_out, i64 cap, i64 *k_out,
                         i32 *map_out, int memspace) {
  InArg v;
  PFDCHK(v.bind(strord, (size_t)h->n * sizeof(T), memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(map_out, (size_t)h->n * sizeof(i32), memspace));
  Outlets R;
  PFDCHK(pfd_with_graph(h, [&](auto d, auto seq, u64 m) { return outlets_run<R_STO, T>(h, d, seq, m, (const T *)v.dev, min_sto, true, R); }));
  if (R.k > 0x7FFFFFFFull) {
    pfd_set_error("subbasins_streamorder: %llu outlets do not fit the int32 map", (unsigned long long)R.k);
    return PFD_EUNSUPPORTED;
  }
  PFDCHK(pfd_basins_dev(h, R.idx.as<i64>(), R.ids.p, (u32)R.k, 4, o.dev));
  *k_out = (i64)R.k;
  if ((i64)R.k <= cap) PFDCHK(give_idxs(h, R.idx.as<i64>(), R.k, idx_dtype, idxs_out, memspace));
  return o.finish(h->stream);
}

template <class T>
static int basin_outlets_t(pfd_raster *h, const void *regions, int idx_dtype, void *idxs_out, void *lbs_out, i64 cap,
                           i64 *k_out, int memspace) {
  InArg v;
  PFDCHK(v.bind(regions, (size_t)h->n * sizeof(T), memspace, h->stream));
  Outlets R;
  PFDCHK(pfd_with_graph(h, [&](auto d, auto seq, u64 m) { return outlets_run<R_LABEL, T>(h, d, seq, m, (const T *)v.dev, 0, true, R); }));
  *k_out = (i64)R.k;
  if (!R.k || (i64)R.k > cap) return PFD_OK;
  // by label, stable: the outlets of one label stay in reversed sequence order
  const u64 k = R.k;
  DevBuf lb, lb2, idx2, tmp;
  PFDCHK(lb.alloc((size_t)k * sizeof(T)));
  PFDCHK(lb2.alloc((size_t)k * sizeof(T)));
  PFDCHK(idx2.alloc((size_t)k * sizeof(i64)));
  pfd_seg_begin(h, "outlets_sort");
  k_gather<T><<<cdiv_u32(k, 256), 256, 0, h->stream>>>(R.idx.as<i64>(), k, (const T *)v.dev, lb.as<T>());
  KCHK();
  PFDCHK(pfd_rocprim(tmp, [&](void *p, size_t &b) {
    return rocprim::radix_sort_pairs(p, b, lb.as<T>(), lb2.as<T>(), R.idx.as<i64>(), idx2.as<i64>(), (size_t)k, 0u,
                                     (unsigned)(8 * sizeof(T)), h->stream);
  }));
  pfd_seg_end(h, 2);
  PFDCHK(give_list(h, lb2.p, (size_t)k * sizeof(T), lbs_out, memspace));
  return give_idxs(h, idx2.as<i64>(), k, idx_dtype, idxs_out, memspace);
}

}  // namespace

extern "C" int pfd_subbasins_streamorder(pfd_raster *h, int dtype, const void *strord, int64_t min_sto, int idx_dtype,
                                         void *idxs_out, int64_t cap, int64_t *k_out, int32_t *map_out, int memspace) {
  PFDCHK(pfd_check_list_args(h, "subbasins_streamorder", strord, idx_dtype, idxs_out, cap, k_out));
  if (!map_out) {
    pfd_set_error("subbasins_streamorder: NULL map_out");
    return PFD_EINVAL;
  }
  switch (dtype) {
    case PFD_U8: return streamorder_t<u8>(h, strord, min_sto, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
    case PFD_I32: return streamorder_t<i32>(h, strord, min_sto, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
    case PFD_U32: return streamorder_t<u32>(h, strord, min_sto, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
    case PFD_I64: return streamorder_t<i64>(h, strord, min_sto, idx_dtype, idxs_out, cap, k_out, map_out, memspace);
    default:
      pfd_set_error("subbasins_streamorder: stream order dtype code %d is not supported (uint8, int32, uint32, int64)", dtype);
      return PFD_EUNSUPPORTED;
  }
}

extern "C" int pfd_outflow_idxs(pfd_raster *h, const uint8_t *region, int idx_dtype, void *idxs_out, int64_t cap,
                                int64_t *k_out, int memspace) {
  PFDCHK(pfd_check_list_args(h, "outflow_idxs", region, idx_dtype, idxs_out, cap, k_out));
  InArg v;
  PFDCHK(v.bind(region, (size_t)h->n, memspace, h->stream));
  Outlets R;
  PFDCHK(pfd_with_graph(h, [&](auto d, auto seq, u64 m) { return outlets_run<R_REGION, u8>(h, d, seq, m, (const u8 *)v.dev, 0, false, R); }));
  *k_out = (i64)R.k;
  if ((i64)R.k <= cap) PFDCHK(give_idxs(h, R.idx.as<i64>(), R.k, idx_dtype, idxs_out, memspace));
  return PFD_OK;
}

extern "C" int pfd_basin_outlets(pfd_raster *h, int dtype, const void *regions, int idx_dtype, void *idxs_out, void *lbs_out,
                                 int64_t cap, int64_t *k_out, int memspace) {
  PFDCHK(pfd_check_list_args(h, "basin_outlets", regions, idx_dtype, idxs_out, cap, k_out));
  if (cap > 0 && !lbs_out) {
    pfd_set_error("basin_outlets: NULL lbs_out");
    return PFD_EINVAL;
  }
  switch (dtype) {
    case PFD_I32: return basin_outlets_t<i32>(h, regions, idx_dtype, idxs_out, lbs_out, cap, k_out, memspace);
    case PFD_U32: return basin_outlets_t<u32>(h, regions, idx_dtype, idxs_out, lbs_out, cap, k_out, memspace);
    case PFD_I64: return basin_outlets_t<i64>(h, regions, idx_dtype, idxs_out, lbs_out, cap, k_out, memspace);
    case PFD_U64: return basin_outlets_t<u64>(h, regions, idx_dtype, idxs_out, lbs_out, cap, k_out, memspace);
    default:
      pfd_set_error("basin_outlets: label dtype code %d is not supported (int32, uint32, int64, uint64)", dtype);
      return PFD_EUNSUPPORTED;
  }
}
