// The frame of a codeblock's decode that the three LDPC decoder kernels share (ldpc_decode_row.hip, ldpc_decode_pk.hip, ldpc_decode_pkw.hip):
// what happens around the layer loop -- the plain load, the output of an all-zero input and the number of layers. Reference:
// ldpc_decoder_impl.cpp:60-146. The geometry (base-graph dimensions, layer bound, soft-bit bytes) is miphy_internal.h's, the same functions
// the launch planner calls. The per-lane layer word and the checksum test stay with the kernels: the packed and the wave kernel are tuned
// against the register allocator, and shared forms of those two pieces cost them registers and spills (profiles/r03_ab_decoder_frame.txt).
#pragma once
#include "ldpc_pk_device.h"

namespace {

// The position behind the last non-zero byte of input bytes [16 q, 16 q + 16), or `last` where all sixteen are zero.
__device__ __forceinline__ int last_nonzero_behind(uint4 v, int q, int last)
{
  int hi = -1;
  hi     = v.x ? 3 - (__clz((int)v.x) >> 3) : hi;
  hi     = v.y ? 7 - (__clz((int)v.y) >> 3) : hi;
  hi     = v.z ? 11 - (__clz((int)v.z) >> 3) : hi;
  hi     = v.w ? 15 - (__clz((int)v.w) >> 3) : hi;
  return (hi >= 0) ? 16 * q + hi + 1 : last;
}

// The plain load of a workgroup's codeblock (every thread calls: it holds a barrier): soft bits cleared in front of the input (the two
// punctured nodes) and behind it, the input copied to soft[2 Z ...] -- 16 bytes per lane and step where the buffers allow it (the common
// case: Z a multiple of 8, 16-byte aligned codeblock buffers). Returns this lane's candidate for the position behind the last non-zero input.
__device__ __forceinline__ int cb_plain_load(int8_t* soft, const int8_t* llr, int in_len, int Z, int soft_bytes, int tid, int nt)
{
  for (int k = tid; k < 2 * Z; k += nt)
    soft[k] = 0;
  for (int k = 2 * Z + in_len + tid; k < soft_bytes; k += nt)
    soft[k] = 0;
  __syncthreads();
  int last = 0;
  if ((((uintptr_t)llr | (uintptr_t)(2 * Z)) & 15) == 0) {
    const uint4* src = reinterpret_cast<const uint4*>(llr);
    uint4*       dst = reinterpret_cast<uint4*>(soft + 2 * Z);
    const int    nq  = in_len >> 4;
    for (int q = tid; q < nq; q += nt) {
      const uint4 v = src[q];
      dst[q]        = v;
      last          = last_nonzero_behind(v, q, last);
    }
    for (int k = (nq << 4) + tid; k < in_len; k += nt) {
      const int8_t v  = llr[k];
      soft[2 * Z + k] = v;
      last            = (v != 0) ? k + 1 : last;
    }
  } else {
    for (int k = tid; k < in_len; k += nt) {
      const int8_t v  = llr[k];
      soft[2 * Z + k] = v;
      last            = (v != 0) ? k + 1 : last;
    }
  }
  return last;
}

// The output of an all-zero input when no checksum is asked for: K ones (ldpc_decoder_impl.cpp:88-94), bytes first, first + stride, ...
__device__ __forceinline__ void store_all_ones(uint8_t* out, int K, int first, int stride)
{
  for (int b = first; b < (K + 7) / 8; b += stride) {
    const int rem = K - 8 * b;
    out[b]        = (rem >= 8) ? 0xff : (uint8_t)(0xff << (8 - rem));
  }
}

// Layers of a decode whose last non-zero input sits in front of position `last` > 0 (ldpc_decoder_impl.cpp:101-114).
__device__ __forceinline__ int cb_nof_layers(int last, int Z, int bgi)
{
  int cb_len = max(last + 2 * Z, (miphy_bg_K(bgi) + 4) * Z);
  cb_len     = ((cb_len + Z - 1) / Z) * Z;
  return cb_len / Z - miphy_bg_K(bgi);
}

} // namespace
