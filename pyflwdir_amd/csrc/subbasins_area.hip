// subbasins_area.hip — basins.subbasins_area (reference pyflwdir/basins.py:194-233): sub-basins of a minimum area.
// The reference is one loop over the sequence with a running `upa_out`.  The sequence is ordered by rank and lists the
// upstream cells of one cell next to each other, so the loop falls apart into GROUPS, one per parent cell p (DESIGN.md,
// "subbasins_area"): while the children of p are visited the loop reads upa_out[p] only, and writes upa_out[p] and
// upa_out[child of p] only.  A group is a serial loop over at most 8 children in ascending linear index; what it hands
// to the groups of its children is one number per child; no order between groups matters.
//   import     idxs_us_main into 32-bit lanes under the strict rule of walks.h: another, valid cell that drains into its cell
//   scan       the pits (outlets, and the jobs of round 0); whether {area > area_min} is closed downstream: then a child
//              outside it can neither be nor lead to an outlet and is not followed (PRUNED mode; else FULL mode); the
//              number of cells a round can queue, which sizes the job lists
//   rounds     a job = (cell p, upa_out[p]).  One lane per job runs p's group, marks outlets in a byte raster, queues the
//              children off the main stem for the next round (one atomic per wave and step) and goes on with the main
//              upstream cell itself.  With the default main upstream cells (largest upstream cell count) a queued child
//              holds at most half of its parent's cells: at most log2(n_seq) + 1 rounds.
//   list, map  the stable compaction of the exact sequence by the marks; the label fill of pfd_basins with ids 1 .. k
// The walks are latency-bound gathers with one lane per job, like the other walks of this library; the error word, the
// import kernel and the list kernels are the shared ones of walks.h / lists.h.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "lists.h"

namespace {

typedef unsigned long long ull;

enum { SA_NOMAIN = WE_OWN, SA_LIST = WE_OWN << 1 };  // the call's own bits of the error word (walks.h)
const WalkErrText SA_TEXT = {"an index of idxs_us_main", "a walk did not end within n_cells steps"};

// x > area_min, in the areas' own type (F64 = false: `thr` is area_min rounded to it) or in float64
template <class T, bool F64>
struct Above {
  T thr;
  double thr64;
  __device__ __forceinline__ bool operator()(T x) const { return F64 ? (double)x > thr64 : x > thr; }
};
// a - b rounded once in the areas' type (integers wrap, as numpy's do)
template <class T>
__device__ __forceinline__ T sa_sub(T a, T b) {
  if constexpr (std::is_integral<T>::value) {
    typedef typename std::make_unsigned<T>::type U;
    return (T)((U)a - (U)b);
  } else {
    return a - b;
  }
}

// mark = the pits; count[0] = valid non-pit cells above area_min that drain to a cell not above it, count[1] / [2] = the
// cells off the main stem (the only ones a round queues) above area_min / in all
template <class T, bool F64>
__global__ void __launch_bounds__(256) k_sa_scan(const DownD8 d, u64 n, const T *__restrict__ A, const u32 *__restrict__ usm,
                                                 const Above<T, F64> ab, u8 *__restrict__ mark, ull *__restrict__ count) {
  for (u64 x0 = (u64)blockIdx.x * 256u; x0 < n; x0 += (u64)gridDim.x * 256u) {
    const u64 x = x0 + threadIdx.x;
    bool pit = false, open = false, light = false, in = false;
    if (x < n && d.valid(x)) {
      const u64 y = d.down(x);
      pit = y == x;
      in = ab(A[x]);
      if (!pit) {
        open = in && !ab(A[y]);
        light = (u64)usm[y] != x;
      }
    }
    if (x < n) mark[x] = pit ? 1 : 0;
    const u64 b0 = __ballot(open), b1 = __ballot(light && in), b2 = __ballot(light);
    if ((threadIdx.x & 63u) == 0) {
      if (b0) atomicAdd(count, (ull)__popcll(b0));
      if (b1) atomicAdd(count + 1, (ull)__popcll(b1));
      if (b2) atomicAdd(count + 2, (ull)__popcll(b2));
    }
  }
}

// One lane per job.  ctr[0] = jobs queued for the next round, ctr[1] = lane steps (groups run), ctr[2] = outlets marked.
// `vals` == nullptr: the jobs are pits and start from their own area.  Every lane of a wave stays in the loop until the
// last one is done, so the shuffles of the append run in uniform control flow.
template <class T, bool F64>
__global__ void __launch_bounds__(256) k_sa_walk(const DownD8 d, const T *__restrict__ A, const u32 *__restrict__ usm,
                                                 const Above<T, F64> ab, int full, const u32 *__restrict__ jobs,
                                                 const T *__restrict__ vals, u32 njobs, u32 *__restrict__ next,
                                                 T *__restrict__ next_vals, u32 cap, u8 *__restrict__ mark,
                                                 ull *__restrict__ ctr, u32 *__restrict__ err) {
  constexpr int ASC[8] = {5, 6, 7, 4, 0, 3, 2, 1};  // NW, N, NE, W, E, SW, S, SE: ascending linear index
  const u32 t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  bool live = t < njobs;
  u32 p = 0, steps = 0, found = 0;
  T up = T(0);
  if (live) {
    p = jobs[t];
    up = vals ? vals[t] : A[p];
  }
  while (__any(live)) {
    u32 kid[8], qm = 0;
    T vq[8];
    if (live) {
      ++steps;
      const u32 m = usm[p];
      const T ap = A[p];
      const u32 r = geo_row(d.g, p), c = p - r * d.g.ncol;
      u32 has = 0;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (d8_child(d.ncode, d.g, p, r, c, ASC[s], &kid[s])) has |= 1u << s;
      T a[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) a[s] = (has >> s) & 1u ? A[kid[s]] : T(0);
      // the group: um = upa_out[m] as the siblings and m itself leave it
      T um = T(0), am = T(0);
      bool um_set = false, saw_m = false;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (!((has >> s) & 1u)) continue;
        const u32 x = kid[s];
        const T u = a[s];
        const bool cond = ab(sa_sub(up, u)) && ab(u);
        if (x == m) {
          saw_m = true, am = u;
          if (cond) {
            if (!ab(sa_sub(ap, u))) mark[x] = 1, ++found, um = u;  // an inter-basin outlet
            else if (!um_set) um = u;                              // (else keeps what a tributary wrote)
          } else {
            um = up;
          }
          um_set = true;
        } else {
          T v = up;
          if (cond) {  // a tributary above the threshold: an outlet, and its area leaves the main stem
            mark[x] = 1, ++found;
            v = u;
            up = sa_sub(up, u);
            um = up, um_set = true;
            if (m == PFD_NOCELL) atomicOr(err, (u32)SA_NOMAIN);
          }
          if (full || ab(u)) qm |= 1u << s, vq[s] = v;
        }
      }
      if (saw_m && (full || ab(am))) p = m, up = um;
      else live = false;
      if (live && steps > d.g.n) {
        atomicOr(err, (u32)WE_CAP);
        live = false;
      }
    }
    // append the queued children: one atomic per wave
    const u32 nq = (u32)__popc(qm);
    u32 incl = nq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 y = (u32)__shfl_up((int)incl, o);
      if (lane >= (u32)o) incl += y;
    }
    const u32 total = (u32)__shfl((int)incl, 63);
    if (total) {
      u32 base = 0;
      if (lane == 63u) base = (u32)atomicAdd(ctr, (ull)total);
      base = (u32)__shfl((int)base, 63);
      u32 pos = base + incl - nq;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        if (!((qm >> s) & 1u)) continue;
        if (pos < cap) next[pos] = kid[s], next_vals[pos] = vq[s];
        else atomicOr(err, (u32)SA_LIST);
        ++pos;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    steps += (u32)__shfl_down((int)steps, o);
    found += (u32)__shfl_down((int)found, o);
  }
  if (lane == 0 && steps) atomicAdd(ctr + 1, (ull)steps);
  if (lane == 0 && found) atomicAdd(ctr + 2, (ull)found);
}

// the shared findings of the error word, then the call's own.  (WE_CAP cannot be set beside SA_NOMAIN: a walk follows
// decoded upstream neighbours only, which never lead back to a cell.)
static int sa_check_err(pfd_raster *h, WalkErr &err) {
  u32 own = 0;
  PFDCHK(err.check(h, "subbasins_area", SA_TEXT, &own));
  if (own & SA_NOMAIN) {
    pfd_set_error("subbasins_area: idxs_us_main has no main upstream cell where a tributary above area_min joins");
    return PFD_EINVAL;
  }
  if (own & SA_LIST) {
    pfd_set_error("subbasins_area: a round queued more jobs than there are cells to follow");
    return PFD_EINVAL;
  }
  return PFD_OK;
}

// the marks of the outlets and their number; stats = mode, rounds, jobs, lane steps
template <class T, bool F64>
static int sa_rounds(pfd_raster *h, const T *A, const u32 *usm, double area_min, int flags, u8 *mark, WalkErr &err, u64 *marked,
                     i64 stats[4]) {
  const DownD8 d{h->ncode, h->geo};
  const u64 n = (u64)h->n;
  const Above<T, F64> ab{(T)area_min, area_min};
  DevBuf cnt;
  PFDCHK(cnt.alloc(4 * sizeof(ull)));
  ull *c = cnt.as<ull>();
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(ull), h->stream));
  pfd_seg_begin(h, "subarea_closure");
  k_sa_scan<T, F64><<<sweep_grid(n), 256, 0, h->stream>>>(d, n, A, usm, ab, mark, c);
  KCHK();
  pfd_seg_end(h, 1);
  ull hc[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(hc, c, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemsetAsync(c, 0, 4 * sizeof(ull), h->stream));  // (from here on: c[0] the next round's jobs, c[1] lane steps, c[2] outlets)
  const int full =((flags & PFD_SUBAREA_FULL) || hc[0]) ? 1 : 0;
  const u64 cap = std::max<u64>(full ? hc[2] : hc[1], 1);
  DevBuf jobs[2], vals[2];
  for (int q = 0; q < 2; ++q) {
    PFDCHK(jobs[q].alloc((size_t)cap * sizeof(u32)));
    PFDCHK(vals[q].alloc((size_t)cap * sizeof(T)));
  }
  PFDCHK(pfd_ensure_pits(h));
  const u32 *cur = h->pits;
  const T *cur_vals = nullptr;
  u64 nj = (u64)h->n_pits;
  i64 rounds = 0, total = 0, launches = 0;
  pfd_seg_begin(h, "subarea_rounds");
  while (nj) {
    if (rounds > h->n_seq) {
      pfd_set_error("subbasins_area: the job list did not run empty within n_seq rounds");
      return PFD_EINVAL;
    }
    const int q = (int)(rounds & 1);
    HIPCHK(hipMemsetAsync(c, 0, sizeof(ull), h->stream));
    k_sa_walk<T, F64><<<cdiv_u32(nj, 256), 256, 0, h->stream>>>(d, A, usm, ab, full, cur, cur_vals, (u32)nj, jobs[q].as<u32>(),
                                                                 vals[q].as<T>(), (u32)cap, mark, c, err.dev());
    KCHK();
    ++launches, ++rounds, total += (i64)nj;
    u64 nn = 0;
    PFDCHK(read_count(h, c, &nn));  // (one count per round)
    if (nn > cap) break;            // (SA_LIST is set: reported below)
    cur = jobs[q].as<u32>(), cur_vals = vals[q].as<T>(), nj = nn;
  }
  pfd_seg_end(h, launches);
  PFDCHK(sa_check_err(h, err));
  u64 lane_steps = 0, found = 0;
  PFDCHK(read_count(h, c + 1, &lane_steps));
  PFDCHK(read_count(h, c + 2, &found));
  *marked = (u64)h->n_pits + found;
  stats[0] = full, stats[1] = rounds, stats[2] = total, stats[3] = (i64)lane_steps;
  return PFD_OK;
}

template <class T>
static int sa_t(pfd_raster *h, const void *uparea, double area_min, int compare, const i64 *idxs_us_main, int idx_dtype,
                void *idxs_out, i64 cap, i64 *k_out, u32 *map_out, i64 *stats_out, int flags, int memspace) {
  const u32 n = h->geo.n;
  if (std::is_integral<T>::value && compare == PFD_COMPARE_OWN &&
      !(area_min == std::trunc(area_min) && std::fabs(area_min) <= 9007199254740992.0 && (T)area_min == area_min)) {
    pfd_set_error("subbasins_area: area_min = %g is no value of the integer areas' dtype (compare in float64)", area_min);
    return PFD_EINVAL;
  }
  InArg a, u;
  PFDCHK(a.bind(uparea, (size_t)n * sizeof(T), memspace, h->stream));
  PFDCHK(u.bind(idxs_us_main, (size_t)n * sizeof(i64), memspace, h->stream));
  OutArg o;
  PFDCHK(o.bind(map_out, (size_t)n * sizeof(u32), memspace));
  DevBuf cells, usm, mark, oseq, cnt, sel, idx, ids;
  WalkErr err;
  const T *upa = (const T *)a.dev;
  PFDCHK(usm.alloc((size_t)n * sizeof(u32)));
  if (!upa || !u.dev) {  // the upstream cell count: the default area, and what the main upstream cell is chosen by
    PFDCHK(cells.alloc((size_t)n * sizeof(i32)));
    PFDCHK(pfd_upstream_area_cell(h, cells.as<i32>(), PFD_DEVICE));
  }
  if (!u.dev) PFDCHK(pfd_main_upstream(h, PFD_I32, cells.p, 0.0, PFD_U32, usm.p, PFD_DEVICE));  // (none: all-ones = PFD_NOCELL)
  if (!upa) upa = (const T *)cells.p;  // (T is int32 then)
  pfd_seg_clear(h);
  PFDCHK(err.init(h));
  if (u.dev) {
    pfd_seg_begin(h, "subarea_import");
    PFDCHK(pfd_import_cells<IMPORT_STRICT>(h, "subbasins_area", PFD_I64, u.dev, (u64)n, (u64)n, usm.as<u32>(), nullptr, err.dev()));
    pfd_seg_end(h, 1);
    PFDCHK(sa_check_err(h, err));  // (before anything is indexed with the list)
  }
  PFDCHK(pfd_exact_seq_dev(h, oseq));  // (orders the cells: n_seq bounds the rounds)
  const u64 m = (u64)h->n_seq;
  PFDCHK(mark.alloc((size_t)n));
  i64 stats[4] = {0, 0, 0, 0};
  u64 marked = 0;
  if (compare == PFD_COMPARE_F64) PFDCHK((sa_rounds<T, true>(h, upa, usm.as<u32>(), area_min, flags, mark.as<u8>(), err, &marked, stats)));
  else PFDCHK((sa_rounds<T, false>(h, upa, usm.as<u32>(), area_min, flags, mark.as<u8>(), err, &marked, stats)));
  if (stats_out)
    for (int q = 0; q < 4; ++q) stats_out[q] = stats[q];
  // the list: the sequence compacted by the marks
  PFDCHK(cnt.alloc(sizeof(ull)));
  HIPCHK(hipMemsetAsync(cnt.p, 0, sizeof(ull), h->stream));
  u64 k = 0;
  pfd_seg_begin(h, "subarea_list");
  if (m && marked) {
    PFDCHK(sel.alloc((size_t)marked * sizeof(u32)));
    PFDCHK(select_marked(h, (const u32 *)oseq.p, m, mark.as<u8>(), sel.as<u32>(), cnt.as<ull>()));
    PFDCHK(read_count(h, cnt.as<ull>(), &k));
    if (k != marked) {  // (every outlet is marked by the one group of its parent; the pits lie in the sequence)
      pfd_set_error("subbasins_area: %llu marks, %llu outlets listed", (ull)marked, (ull)k);
      return PFD_EHIP;
    }
  }
  PFDCHK(idx.alloc(std::max<size_t>((size_t)k * sizeof(i64), 16)));
  PFDCHK(ids.alloc(std::max<size_t>((size_t)k * sizeof(u32), 16)));
  if (k) {
    k_number<u32><<<cdiv_u32(k, 256), 256, 0, h->stream>>>(sel.as<u32>(), k, false, idx.as<i64>(), ids.as<u32>());
    KCHK();
  }
  pfd_seg_end(h, 3);
  *k_out = (i64)k;
  if ((i64)k <= cap) PFDCHK(give_idxs(h, idx.as<i64>(), k, idx_dtype, idxs_out, memspace));
  // the map: core.fillnodata_upstream of the labels 1 .. k = one label fill
  PFDCHK(pfd_basins_dev(h, idx.as<i64>(), ids.p, (u32)k, 4, o.dev));
  return o.finish(h->stream);
}

}  // namespace

extern "C" int pfd_subbasins_area(pfd_raster *h, int dtype, const void *uparea, double area_min, int compare,
                                  const int64_t *idxs_us_main, int idx_dtype, void *idxs_out, int64_t cap, int64_t *k_out,
                                  uint32_t *map_out, int64_t *stats_out, int flags, int memspace) {
  const char *what = "subbasins_area";
  PFDCHK(pfd_check_handle(h));
  if (h->gen) {
    pfd_set_error("subbasins_area is not available on a general idxs_ds graph: its only sequence is an unstable sort by rank, "
                  "which leaves the order of the upstream cells of one cell, on which the result depends, unspecified");
    return PFD_EUNSUPPORTED;
  }
  PFDCHK(pfd_require_whole(h, what));
  if (!map_out || !k_out || cap < 0 || (cap > 0 && !idxs_out) || (compare != PFD_COMPARE_OWN && compare != PFD_COMPARE_F64) ||
      (flags & ~PFD_SUBAREA_FULL)) {
    pfd_set_error("%s: bad arguments (NULL pointer, cap=%lld, compare=%d, flags=%d, area_min=%g)", what, (long long)cap, compare,
                  flags, area_min);
    return PFD_EINVAL;
  }
  if (!pfd_idx_bytes(idx_dtype)) {
    pfd_set_error("%s: unsupported index dtype code %d", what, idx_dtype);
    return PFD_EUNSUPPORTED;
  }
  if (!uparea)
    return sa_t<i32>(h, nullptr, area_min, compare, idxs_us_main, idx_dtype, idxs_out, cap, k_out, map_out, stats_out, flags, memspace);
  return pfd_dispatch_payload(dtype, what, [&](auto tag) -> int {
    typedef typename decltype(tag)::type T;
    return sa_t<T>(h, uparea, area_min, compare, idxs_us_main, idx_dtype, idxs_out, cap, k_out, map_out, stats_out, flags, memspace);
  });
}
