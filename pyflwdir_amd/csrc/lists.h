// lists.h — what the list-producing calls share (outlets.hip: outlet lists, streams.hip: segment lists): the downstream
// link under the three forms of a handle, and the hand-over of a list to the caller.
#pragma once
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

// k values from HBM into the caller's list (a host list: counted as a download of the call)
static inline int give_list(pfd_raster *h, const void *dev, size_t bytes, void *out, int memspace) {
  if (!bytes) return PFD_OK;
  if (memspace == PFD_DEVICE) {
    HIPCHK(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PFD_OK;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  const double t0 = pfd_now_ms();
  HIPCHK(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  PfdTransfer &t = pfd_transfer();
  t.d2h_bytes += (double)bytes, t.d2h_ms += pfd_now_ms() - t0, t.host_results += 1;
  return PFD_OK;
}

