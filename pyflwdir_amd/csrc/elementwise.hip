// elementwise.hip — the small per-cell expressions between two sweeps, on arrays that stay in HBM: comparisons with a
// scalar, logic on byte masks, select, the exact widenings, and the reductions no execution order can change
// (include/pfd.h "elementwise").  pyflwdir_amd/device_array.py is the front end.
//
// All of it is bound by memory.  A lane moves 16 bytes of the WIDEST operand per step (a 16-byte load or store; the
// narrower operands of the same elements travel as 2 / 4 / 8-byte accesses), the loops are grid-stride over 64-bit
// indices with a grid sized from the CU count, and the last n mod vector elements take a scalar loop of the same kernel.
// Pointers that are not 16-byte aligned (nothing an allocator returns: a C caller's offset into a block) take the scalar
// loop for everything; tests/test_gpu_device_array.py runs that path through _hip.ew_* with offset addresses.
//
// Ordering: the kernels run on the null stream and every entry point waits for it before it returns — the rule of
// pfd.h ("memory spaces"): a result is complete in HBM when the call that produced it returns.
#include <string.h>

#include "common.h"

namespace {

template <class T, int N>
struct alignas(sizeof(T) * N) Pack {
  T v[N];
};

constexpr int EW_BLOCK = 256;

int ew_cu_count(int device) {
  static int cached[64] = {0};
  if (device >= 0 && device < 64 && cached[device]) return cached[device];
  int cu = 0;
  if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0) {
    (void)hipGetLastError();
    cu = 256;
  }
  if (device >= 0 && device < 64) cached[device] = cu;
  return cu;
}
// workgroups of a streaming kernel over `units` lane steps: 8 per CU at the most, never more than the work
u32 ew_grid(int device, u64 units) {
  const u64 want = (units + EW_BLOCK - 1) / EW_BLOCK;
  return (u32)std::max<u64>(1, std::min<u64>(want, (u64)ew_cu_count(device) * 8));
}
bool ew_aligned(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- compare ---------------------------------------------------------------------------------------------------------
// `rel`: which of the four outcomes of comparing x with the scalar give 1 — bit 0 x < s, bit 1 x == s, bit 2 x > s,
// bit 3 unordered (a NaN on either side).  <: 1, <=: 3, >: 4, >=: 6, ==: 2, !=: 13.
template <class C>
__device__ __forceinline__ u8 ew_rel(C x, C s, u32 rel) {
  const u32 lt = x < s, eq = x == s, gt = x > s;
  const u32 o = lt | (eq << 1) | (gt << 2);
  return (u8)(((o ? o : 8u) & rel) != 0);
}
template <class T, class C>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_compare(const T *__restrict__ a, C s, u32 rel, u8 *__restrict__ out, u64 n,
                                                         u64 nvec) {
  constexpr int N = 16 / sizeof(T);
  const u64 stride = (u64)gridDim.x * EW_BLOCK, t0 = (u64)blockIdx.x * EW_BLOCK + threadIdx.x;
  for (u64 i = t0; i < nvec; i += stride) {
    const Pack<T, N> x = ((const Pack<T, N> *)a)[i];
    Pack<u8, N> r;
#pragma unroll
    for (int k = 0; k < N; ++k) r.v[k] = ew_rel<C>((C)x.v[k], s, rel);
    ((Pack<u8, N> *)out)[i] = r;
  }
  for (u64 i = nvec * N + t0; i < n; i += stride) out[i] = ew_rel<C>((C)a[i], s, rel);
}

// ---- logic on byte masks (0 / 1) ---------------------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ u32 ew_logic32(u32 x, u32 y) {
  return OP == 0 ? (x & y) : OP == 1 ? (x | y) : OP == 2 ? (x ^ y) : (x ^ 0x01010101u);
}
template <int OP>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_logic(const u8 *__restrict__ a, const u8 *__restrict__ b, u8 *__restrict__ out,
                                                       u64 n, u64 nvec) {
  const u64 stride = (u64)gridDim.x * EW_BLOCK, t0 = (u64)blockIdx.x * EW_BLOCK + threadIdx.x;
  for (u64 i = t0; i < nvec; i += stride) {
    const Pack<u32, 4> x = ((const Pack<u32, 4> *)a)[i];
    Pack<u32, 4> y = x;
    if (OP != 3) y = ((const Pack<u32, 4> *)b)[i];
    Pack<u32, 4> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = ew_logic32<OP>(x.v[k], y.v[k]);
    ((Pack<u32, 4> *)out)[i] = r;
  }
  for (u64 i = nvec * 16 + t0; i < n; i += stride) out[i] = (u8)ew_logic32<OP>(a[i], OP != 3 ? b[i] : 0u);
}

// ---- select: out = mask != 0 ? a : b (b an array, or the scalar `bs` when b is null); elements move as bit patterns -----
template <class U>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_where(const u8 *__restrict__ mask, const U *__restrict__ a,
                                                       const U *__restrict__ b, U bs, U *__restrict__ out, u64 n, u64 nvec) {
  constexpr int N = 16 / sizeof(U);
  const u64 stride = (u64)gridDim.x * EW_BLOCK, t0 = (u64)blockIdx.x * EW_BLOCK + threadIdx.x;
  for (u64 i = t0; i < nvec; i += stride) {
    const Pack<u8, N> m = ((const Pack<u8, N> *)mask)[i];
    const Pack<U, N> x = ((const Pack<U, N> *)a)[i];
    Pack<U, N> y = x;
    if (b) y = ((const Pack<U, N> *)b)[i];
    Pack<U, N> r;
#pragma unroll
    for (int k = 0; k < N; ++k) r.v[k] = m.v[k] ? x.v[k] : (b ? y.v[k] : bs);
    ((Pack<U, N> *)out)[i] = r;
  }
  for (u64 i = nvec * N + t0; i < n; i += stride) out[i] = mask[i] ? a[i] : (b ? b[i] : bs);
}

// ---- the exact widenings ---------------------------------------------------------------------------------------------
template <class S, class D>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_convert(const S *__restrict__ a, D *__restrict__ out, u64 n, u64 nvec) {
  constexpr int N = 16 / sizeof(D);
  const u64 stride = (u64)gridDim.x * EW_BLOCK, t0 = (u64)blockIdx.x * EW_BLOCK + threadIdx.x;
  for (u64 i = t0; i < nvec; i += stride) {
    const Pack<S, N> x = ((const Pack<S, N> *)a)[i];
    Pack<D, N> r;
#pragma unroll
    for (int k = 0; k < N; ++k) r.v[k] = (D)x.v[k];
    ((Pack<D, N> *)out)[i] = r;
  }
  for (u64 i = nvec * N + t0; i < n; i += stride) out[i] = (D)a[i];
}

// ---- reductions ------------------------------------------------------------------------------------------------------
// One 64-bit accumulator and one flag per lane: the count of non-zero elements (PFD_EW_COUNT), or the smallest / largest
// KEY — the value itself for the integer types, for the float types the bit pattern made monotone (negative patterns
// flipped), so that min and max are integer folds with one answer whatever the order, -0.0 below 0.0 included.  A NaN
// never enters the fold: it sets the flag, and the caller returns NaN.  Fold within the wave, one partial per workgroup,
// a second launch of one workgroup over the partials; no atomics.
__device__ __forceinline__ i64 ew_key(u8 v) { return (i64)v; }
__device__ __forceinline__ i64 ew_key(int8_t v) { return (i64)v; }
__device__ __forceinline__ i64 ew_key(i32 v) { return (i64)v; }
__device__ __forceinline__ i64 ew_key(u32 v) { return (i64)v; }
__device__ __forceinline__ i64 ew_key(i64 v) { return v; }
__device__ __forceinline__ i64 ew_key(float v) {
  const i32 b = __float_as_int(v);
  return (i64)(b ^ ((b >> 31) & 0x7FFFFFFF));
}
__device__ __forceinline__ i64 ew_key(double v) {
  const i64 b = __double_as_longlong(v);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}
template <class T>
__device__ __forceinline__ bool ew_isnan(T v) { return v != v; }

template <int OP>
__device__ __forceinline__ i64 ew_fold(i64 x, i64 y) {
  return OP == PFD_EW_COUNT ? x + y : OP == PFD_EW_MIN ? (y < x ? y : x) : (y > x ? y : x);
}
template <int OP>
__device__ __forceinline__ i64 ew_identity() {
  return OP == PFD_EW_COUNT ? 0 : OP == PFD_EW_MIN ? INT64_MAX : INT64_MIN;
}
template <int OP, class T>
__device__ __forceinline__ void ew_take(T v, i64 &acc, u32 &flag) {
  if (OP == PFD_EW_COUNT) {
    acc += (v != (T)0) ? 1 : 0;  // (a NaN is not zero: counted, like numpy)
  } else if (ew_isnan(v)) {
    flag = 1;
  } else {
    acc = ew_fold<OP>(acc, ew_key(v));
  }
}
// fold of the workgroup's lanes; the result is valid in thread 0
template <int OP>
__device__ __forceinline__ void ew_block_fold(i64 &acc, u32 &flag) {
  for (int o = 32; o > 0; o >>= 1) {
    acc = ew_fold<OP>(acc, __shfl_down(acc, o));
    flag |= __shfl_down(flag, o);
  }
  __shared__ i64 s_acc[EW_BLOCK / 64];
  __shared__ u32 s_flag[EW_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc, s_flag[threadIdx.x >> 6] = flag;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < EW_BLOCK / 64; ++w) acc = ew_fold<OP>(acc, s_acc[w]), flag |= s_flag[w];
  }
}
template <int OP, class T>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_reduce(const T *__restrict__ a, u64 n, u64 nvec, i64 *__restrict__ part_acc,
                                                        u32 *__restrict__ part_flag) {
  constexpr int N = 16 / sizeof(T);
  const u64 stride = (u64)gridDim.x * EW_BLOCK, t0 = (u64)blockIdx.x * EW_BLOCK + threadIdx.x;
  i64 acc = ew_identity<OP>();
  u32 flag = 0;
  for (u64 i = t0; i < nvec; i += stride) {
    const Pack<T, N> x = ((const Pack<T, N> *)a)[i];
#pragma unroll
    for (int k = 0; k < N; ++k) ew_take<OP, T>(x.v[k], acc, flag);
  }
  for (u64 i = nvec * N + t0; i < n; i += stride) ew_take<OP, T>(a[i], acc, flag);
  ew_block_fold<OP>(acc, flag);
  if (threadIdx.x == 0) part_acc[blockIdx.x] = acc, part_flag[blockIdx.x] = flag;
}
template <int OP>
__global__ void __launch_bounds__(EW_BLOCK) k_ew_reduce_final(const i64 *__restrict__ part_acc, const u32 *__restrict__ part_flag,
                                                              u32 nparts, i64 *__restrict__ res) {
  i64 acc = ew_identity<OP>();
  u32 flag = 0;
  for (u32 i = threadIdx.x; i < nparts; i += EW_BLOCK) acc = ew_fold<OP>(acc, part_acc[i]), flag |= part_flag[i];
  ew_block_fold<OP>(acc, flag);
  if (threadIdx.x == 0) res[0] = acc, res[1] = (i64)flag;
}

// ---- host side -------------------------------------------------------------------------------------------------------
int ew_enter(const char *what, int device, int64_t n) {
  if (device < 0 || n < 0) {
    pfd_set_error("%s: bad arguments (device %d, n %lld)", what, device, (long long)n);
    return PFD_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  return PFD_OK;
}
// the rule of pfd.h: the result is complete when the call returns
int ew_leave() {
  KCHK();
  HIPCHK(hipStreamSynchronize(nullptr));
  return PFD_OK;
}

template <class T, class C>
void ew_launch_compare(int device, const void *a, C s, u32 rel, u8 *out, u64 n) {
  constexpr int N = 16 / sizeof(T);
  const u64 nvec = (ew_aligned(a) && ew_aligned(out)) ? n / N : 0;
  k_ew_compare<T, C><<<ew_grid(device, std::max<u64>(nvec, n - nvec * N)), EW_BLOCK>>>((const T *)a, s, rel, out, n, nvec);
}
template <class T>
void ew_compare_typed(int device, const void *a, bool in_f64, T s_own, double s_f64, u32 rel, u8 *out, u64 n) {
  if (in_f64) ew_launch_compare<T, double>(device, a, s_f64, rel, out, n);
  else ew_launch_compare<T, T>(device, a, s_own, rel, out, n);
}
template <class U>
void ew_launch_where(int device, const u8 *mask, const void *a, const void *b, U bs, void *out, u64 n) {
  constexpr int N = 16 / sizeof(U);
  const u64 nvec = (ew_aligned(mask) && ew_aligned(a) && ew_aligned(b) && ew_aligned(out)) ? n / N : 0;
  k_ew_where<U><<<ew_grid(device, std::max<u64>(nvec, n - nvec * N)), EW_BLOCK>>>(mask, (const U *)a, (const U *)b, bs, (U *)out, n,
                                                                                  nvec);
}
template <class S, class D>
void ew_launch_convert(int device, const void *a, void *out, u64 n) {
  constexpr int N = 16 / sizeof(D);
  const u64 nvec = (ew_aligned(a) && ew_aligned(out)) ? n / N : 0;
  k_ew_convert<S, D><<<ew_grid(device, std::max<u64>(nvec, n - nvec * N)), EW_BLOCK>>>((const S *)a, (D *)out, n, nvec);
}
template <int OP, class T>
void ew_launch_reduce(u32 grid, const void *a, u64 n, i64 *part_acc, u32 *part_flag) {
  constexpr int N = 16 / sizeof(T);
  const u64 nvec = ew_aligned(a) ? n / N : 0;
  k_ew_reduce<OP, T><<<grid, EW_BLOCK>>>((const T *)a, n, nvec, part_acc, part_flag);
}
template <int OP>
int ew_reduce_op(int dtype, u32 grid, const void *a, u64 n, i64 *part_acc, u32 *part_flag, i64 *res) {
  switch (dtype) {
    case PFD_U8: ew_launch_reduce<OP, u8>(grid, a, n, part_acc, part_flag); break;
    case PFD_I8: ew_launch_reduce<OP, int8_t>(grid, a, n, part_acc, part_flag); break;
    case PFD_I32: ew_launch_reduce<OP, i32>(grid, a, n, part_acc, part_flag); break;
    case PFD_U32: ew_launch_reduce<OP, u32>(grid, a, n, part_acc, part_flag); break;
    case PFD_I64: ew_launch_reduce<OP, i64>(grid, a, n, part_acc, part_flag); break;
    case PFD_F32: ew_launch_reduce<OP, float>(grid, a, n, part_acc, part_flag); break;
    case PFD_F64: ew_launch_reduce<OP, double>(grid, a, n, part_acc, part_flag); break;
    default: return PFD_EUNSUPPORTED;
  }
  KCHK();
  k_ew_reduce_final<OP><<<1, EW_BLOCK>>>(part_acc, part_flag, grid, res);
  return PFD_OK;
}
size_t ew_elem_bytes(int dtype) {
  switch (dtype) {
    case PFD_U8: case PFD_I8: return 1;
    case PFD_I32: case PFD_U32: case PFD_F32: return 4;
    case PFD_I64: case PFD_F64: return 8;
    default: return 0;
  }
}
int ew_bad_dtype(const char *what, int dtype) {
  pfd_set_error("%s: dtype code %d is not an elementwise dtype (PFD_U8, PFD_I8, PFD_I32, PFD_U32, PFD_I64, PFD_F32, PFD_F64)",
                what, dtype);
  return PFD_EUNSUPPORTED;
}

}  // namespace

extern "C" int pfd_ew_compare(int device, int rel, int dtype, const void *a, int compare_dtype, int64_t scalar_i,
                              double scalar_f, uint8_t *out, int64_t n) {
  PFDCHK(ew_enter("pfd_ew_compare", device, n));
  if (!ew_elem_bytes(dtype)) return ew_bad_dtype("pfd_ew_compare", dtype);
  if (rel < 0 || rel > 15 || (compare_dtype != dtype && compare_dtype != PFD_F64) || (n && (!a || !out))) {
    pfd_set_error("pfd_ew_compare: bad arguments (relation %d, dtype code %d compared as %d)", rel, dtype, compare_dtype);
    return PFD_EINVAL;
  }
  if (!n) return PFD_OK;
  const bool in_f64 = compare_dtype == PFD_F64;
  const u32 r = (u32)rel;
  const u64 m = (u64)n;
  switch (dtype) {
    case PFD_U8: ew_compare_typed<u8>(device, a, in_f64, (u8)scalar_i, scalar_f, r, out, m); break;
    case PFD_I8: ew_compare_typed<int8_t>(device, a, in_f64, (int8_t)scalar_i, scalar_f, r, out, m); break;
    case PFD_I32: ew_compare_typed<i32>(device, a, in_f64, (i32)scalar_i, scalar_f, r, out, m); break;
    case PFD_U32: ew_compare_typed<u32>(device, a, in_f64, (u32)scalar_i, scalar_f, r, out, m); break;
    case PFD_I64: ew_compare_typed<i64>(device, a, in_f64, (i64)scalar_i, scalar_f, r, out, m); break;
    case PFD_F32: ew_compare_typed<float>(device, a, in_f64, (float)scalar_f, scalar_f, r, out, m); break;
    default: ew_launch_compare<double, double>(device, a, scalar_f, r, out, m); break;
  }
  return ew_leave();
}

extern "C" int pfd_ew_logic(int device, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, int64_t n) {
  PFDCHK(ew_enter("pfd_ew_logic", device, n));
  if (op < PFD_EW_AND || op > PFD_EW_NOT || (n && (!a || !out || (op != PFD_EW_NOT && !b)))) {
    pfd_set_error("pfd_ew_logic: bad arguments (op %d)", op);
    return PFD_EINVAL;
  }
  if (!n) return PFD_OK;
  const u64 m = (u64)n;
  const u64 nvec = (ew_aligned(a) && ew_aligned(b) && ew_aligned(out)) ? m / 16 : 0;
  const u32 grid = ew_grid(device, std::max<u64>(nvec, m - nvec * 16));
  if (op == PFD_EW_AND) k_ew_logic<0><<<grid, EW_BLOCK>>>(a, b, out, m, nvec);
  else if (op == PFD_EW_OR) k_ew_logic<1><<<grid, EW_BLOCK>>>(a, b, out, m, nvec);
  else if (op == PFD_EW_XOR) k_ew_logic<2><<<grid, EW_BLOCK>>>(a, b, out, m, nvec);
  else k_ew_logic<3><<<grid, EW_BLOCK>>>(a, nullptr, out, m, nvec);
  return ew_leave();
}

extern "C" int pfd_ew_where(int device, int dtype, const uint8_t *mask, const void *a, const void *b, int64_t scalar_i,
                            double scalar_f, void *out, int64_t n) {
  PFDCHK(ew_enter("pfd_ew_where", device, n));
  const size_t eb = ew_elem_bytes(dtype);
  if (!eb) return ew_bad_dtype("pfd_ew_where", dtype);
  if (n && (!mask || !a || !out)) {
    pfd_set_error("pfd_ew_where: NULL argument");
    return PFD_EINVAL;
  }
  if (!n) return PFD_OK;
  const u64 m = (u64)n;
  if (eb == 1) {
    ew_launch_where<u8>(device, mask, a, b, (u8)scalar_i, out, m);
  } else if (eb == 4) {
    u32 bits = (u32)scalar_i;
    if (dtype == PFD_F32) {
      const float f = (float)scalar_f;
      memcpy(&bits, &f, 4);
    }
    ew_launch_where<u32>(device, mask, a, b, bits, out, m);
  } else {
    u64 bits = (u64)scalar_i;
    if (dtype == PFD_F64) memcpy(&bits, &scalar_f, 8);
    ew_launch_where<u64>(device, mask, a, b, bits, out, m);
  }
  return ew_leave();
}

extern "C" int pfd_ew_convert(int device, int src_dtype, const void *a, int dst_dtype, void *out, int64_t n) {
  PFDCHK(ew_enter("pfd_ew_convert", device, n));
  if (n && (!a || !out)) {
    pfd_set_error("pfd_ew_convert: NULL argument");
    return PFD_EINVAL;
  }
  const u64 m = (u64)n;
  const int s = src_dtype, d = dst_dtype;
  const bool known = (d == PFD_I32 && (s == PFD_U8 || s == PFD_I8)) || ((d == PFD_I64 || d == PFD_F64) && (s == PFD_I32 || s == PFD_U32)) ||
                     (d == PFD_F64 && s == PFD_F32);
  if (!known) {
    pfd_set_error("pfd_ew_convert: dtype code %d -> %d is not one of the exact widenings (one byte -> int32; int32 / uint32 -> "
                  "int64 / float64; float32 -> float64)", s, d);
    return PFD_EUNSUPPORTED;
  }
  if (!n) return PFD_OK;
  if (d == PFD_I32 && s == PFD_U8) ew_launch_convert<u8, i32>(device, a, out, m);
  else if (d == PFD_I32) ew_launch_convert<int8_t, i32>(device, a, out, m);
  else if (d == PFD_I64 && s == PFD_I32) ew_launch_convert<i32, i64>(device, a, out, m);
  else if (d == PFD_I64) ew_launch_convert<u32, i64>(device, a, out, m);
  else if (s == PFD_I32) ew_launch_convert<i32, double>(device, a, out, m);
  else if (s == PFD_U32) ew_launch_convert<u32, double>(device, a, out, m);
  else ew_launch_convert<float, double>(device, a, out, m);
  return ew_leave();
}

extern "C" int pfd_ew_reduce(int device, int op, int dtype, const void *a, int64_t n, int64_t *res_i, double *res_f,
                             int *has_nan) {
  PFDCHK(ew_enter("pfd_ew_reduce", device, n));
  if (!ew_elem_bytes(dtype)) return ew_bad_dtype("pfd_ew_reduce", dtype);
  if (op < PFD_EW_COUNT || op > PFD_EW_MAX || !res_i || !res_f || !has_nan || (n && !a) || (n == 0 && op != PFD_EW_COUNT)) {
    pfd_set_error("pfd_ew_reduce: bad arguments (op %d, n %lld: the smallest / largest of no elements)", op, (long long)n);
    return PFD_EINVAL;
  }
  *res_i = 0, *res_f = 0.0, *has_nan = 0;
  if (!n) return PFD_OK;
  const u64 m = (u64)n;
  const u32 grid = ew_grid(device, m / (16 / ew_elem_bytes(dtype)) + 1);
  DevBuf part;  // [grid] int64 accumulators, 2 int64 of result, [grid] flags
  PFDCHK(part.alloc((size_t)grid * 12 + 16));
  i64 *part_acc = part.as<i64>(), *res = part_acc + grid;
  u32 *part_flag = (u32 *)(res + 2);
  int rc = PFD_OK;
  if (op == PFD_EW_COUNT) rc = ew_reduce_op<PFD_EW_COUNT>(dtype, grid, a, m, part_acc, part_flag, res);
  else if (op == PFD_EW_MIN) rc = ew_reduce_op<PFD_EW_MIN>(dtype, grid, a, m, part_acc, part_flag, res);
  else rc = ew_reduce_op<PFD_EW_MAX>(dtype, grid, a, m, part_acc, part_flag, res);
  PFDCHK(rc);
  KCHK();
  i64 host[2] = {0, 0};
  HIPCHK(hipMemcpy(host, res, sizeof(host), hipMemcpyDeviceToHost));  // (waits for the null stream)
  *has_nan = host[1] != 0;
  if (op != PFD_EW_COUNT && (dtype == PFD_F32 || dtype == PFD_F64)) {
    // back from the monotone key to the value (the flip is its own inverse)
    if (dtype == PFD_F32) {
      i32 b = (i32)host[0];
      b ^= (b >> 31) & 0x7FFFFFFF;
      float f;
      memcpy(&f, &b, 4);
      *res_f = (double)f;
    } else {
      i64 b = host[0];
      b ^= (b >> 63) & 0x7FFFFFFFFFFFFFFFll;
      memcpy(res_f, &b, 8);
    }
  } else {
    *res_i = host[0], *res_f = (double)host[0];
  }
  return PFD_OK;
}
