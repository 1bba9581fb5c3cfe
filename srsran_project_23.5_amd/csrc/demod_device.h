// Soft-demapper quantisation shared by the PUSCH demodulator (pusch_demod.hip) and the PUCCH format-2 demodulator (pucch.hip), so
// both LLR paths round the same way.
#pragma once
#include <hip/hip_runtime.h>
#include "tables/nr_demod_tables.h" // (a translation unit that reads the interval tables on the device defines NR_DEMOD_TABLE_ATTR first)

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

// The exact soft demapper of one equalised symbol (demodulation_mapper_*.cpp restated): shared by the PUSCH demodulator, which also has a packed
// variant for the common case (pusch_demod.hip), and the PUCCH format 3 / 4 processor (pucch_f34.hip). tab: the LDS interval tables of QAM64 / QAM256
// (not read below them).
// The reference converts the interval position with cvtps2dq / cvttss2si, which turn NaN and everything outside int32 -- a huge POSITIVE component
// too -- into INT_MIN, and the clamp then takes that to interval 0. The conversion of this target saturates (v_cvt_i32_f32: INT_MAX); adding the
// offset in unsigned arithmetic wraps that to a negative index, interval 0 again. (With a signed addition the compiler assumes no overflow and
// clamps first: a huge positive component then lands in the last interval, where half of the tables have the opposite slope.
// tests/test_demod_edges_gpu.py holds the toolchain to this.)
static __device__ __forceinline__ int demod_interval_idx(float x, float rcp_width, int count)
{
#pragma clang fp contract(off)
  const int idx = (int)((unsigned)(int)floorf(x * rcp_width) + (unsigned)(count / 2));
  return idx < 0 ? 0 : (idx > count - 1 ? count - 1 : idx);
}
static __device__ __forceinline__ float demod_interval_at(float x, float rcp_noise, float2 si)
{
#pragma clang fp contract(off)
  float t = si.x * x;
  t       = t + si.y;
  return t * rcp_noise;
}

// One equalised symbol -> MOD LLRs in l[]. FAST: no NaN can appear (finite symbol, finite reciprocal noise), which allows the
// one-instruction clamp; otherwise the exact NaN-preserving sequence of the reference is used.
template <int MOD, bool FAST>
static __device__ __forceinline__ void demod_symbol(float re, float im, float nvar, unsigned sym_idx, const float2* tab, int* l)
{
#pragma clang fp contract(off)
#define Q(v, sc) (FAST ? demod_quantize_fast((v), (sc)) : demod_quantize((v), (sc)))
  if (MOD == 1) {
    l[0] = 0;
    if (nvar > 0.f) {
      const float a = (sym_idx & 1u) ? im : re, b = (sym_idx & 1u) ? -re : im;
      const float v = NR_DEMOD_QPSK_GAIN * (a + b) / nvar;
      float       c = v;
      if (fabsf(v) > 24.f)
        c = copysignf(24.f, v);
      l[0] = (int)roundf(c / 24.f * 120.f);
    }
    return;
  }
  const float rcp  = (nvar > 0.f) ? 1.0f / nvar : 0.0f;
  const float x[2] = {re, im};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    if (MOD == 2) {
      l[d] = Q((NR_DEMOD_QPSK_GAIN * x[d]) * rcp, 120.0f / 24.f);
    } else if (MOD == 4) {
      const float first  = NR_DEMOD_QAM16_GAIN * x[d];
      const float second = 2.0f * first - copysignf(0.8f, x[d]);
      const float l01    = (fabsf(x[d]) > NR_DEMOD_QAM16_THRESHOLD) ? second : first;
      const float l23    = 0.8f - fabsf(first);
      l[d]               = Q(l01 * rcp, 6.0f);
      l[2 + d]           = Q(l23 * rcp, 6.0f);
    } else if (MOD == 6) {
      const int i0 = demod_interval_idx(x[d], NR_DEMOD_QAM64_B0_RCP_WIDTH, 8); // bits 0-3 share the grid of 8 intervals
      const int i2 = demod_interval_idx(x[d], NR_DEMOD_QAM64_B2_RCP_WIDTH, 4);
      l[d]         = Q(demod_interval_at(x[d], rcp, tab[i0]), 6.0f);
      l[2 + d]     = Q(demod_interval_at(x[d], rcp, tab[16 + i0]), 6.0f);
      l[4 + d]     = Q(demod_interval_at(x[d], rcp, tab[32 + i2]), 6.0f);
    } else {
      const int i0 = demod_interval_idx(x[d], NR_DEMOD_QAM256_B0_RCP_WIDTH, 16); // bits 0-5 share the grid of 16 intervals
      const int i3 = demod_interval_idx(x[d], NR_DEMOD_QAM256_B3_RCP_WIDTH, 8);
      l[d]         = Q(demod_interval_at(x[d], rcp, tab[i0]), 6.0f);
      l[2 + d]     = Q(demod_interval_at(x[d], rcp, tab[16 + i0]), 6.0f);
      l[4 + d]     = Q(demod_interval_at(x[d], rcp, tab[32 + i0]), 6.0f);
      l[6 + d]     = Q(demod_interval_at(x[d], rcp, tab[48 + i3]), 6.0f);
    }
  }
#undef Q
}
