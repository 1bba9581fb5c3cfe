// The wavefront sum and the complex products of the PUCCH, SRS and PRACH kernels (pucch_device.h includes it; prach.hip takes it alone).
#pragma once
#include <hip/hip_runtime.h>

// Sum over the 64 lanes by the xor tree 32, 16, ... 1; every lane gets it.
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) // a * conj(b)
{
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ float2 cconj(float2 a)
{
  return make_float2(a.x, -a.y);
}
