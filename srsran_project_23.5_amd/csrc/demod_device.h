// Soft-demapper quantisation shared by the PUSCH demodulator (pusch_demod.hip) and the PUCCH format-2 demodulator (pucch.hip), so
// both LLR paths round the same way.
#pragma once
#include <hip/hip_runtime.h>

// Quantisation of avx2_helpers.h:103-157: scale, clip to +-120, round to nearest even, NaN -> 0.
static __device__ __forceinline__ int demod_quantize(float v, float scale)
{
#pragma clang fp contract(off)
  float s = v * scale;
  s       = (s > 120.0f) ? 120.0f : s;
  s       = (s < -120.0f) ? -120.0f : s;
  const float r = rintf(s);
  return (r <= 120.0f && r >= -120.0f) ? (int)r : 0; // NaN -> 0
}
// Same for a value that is known not to be NaN (the caller checks the inputs once per resource element).
static __device__ __forceinline__ int demod_quantize_fast(float v, float scale)
{
#pragma clang fp contract(off)
  return (int)rintf(__builtin_amdgcn_fmed3f(v * scale, -120.0f, 120.0f));
}
