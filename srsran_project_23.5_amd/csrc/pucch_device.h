// Device functions shared by the PUCCH kernels (pucch.hip: formats 1 and 2; pucch_f34.hip: formats 3 and 4): Gold-sequence words, the
// wavefront sum, the time alignment of one hop and the final per-port quantities of port_channel_estimator_average_impl::compute.
#pragma once
#include "gold_device.h"
#include "miphy_internal.h"

namespace {

constexpr int   PUCCH_DFT     = 4096;
constexpr int   PUCCH_HALF_CP = ((144 / 2) * PUCCH_DFT) / 2048; // 144
constexpr float PUCCH_TWOPI   = 6.28318530717958647692f;

// c(offset .. offset + 31) of the Gold sequence of c_init, bit i = c(offset + i).
__device__ __forceinline__ uint32_t gold_word(const gold_tables& gt, uint32_t c_init, uint32_t offset)
{
  const uint32_t s1 = gold_state(gt, false, c_init, offset), s2 = gold_state(gt, true, c_init, offset);
  return (s1 ^ s2) | (((x1_step28(s1) ^ x2_step28(s2)) & 1u) << 31);
}

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

// Time alignment of one hop in IDFT taps (estimate_time_alignment, port_channel_estimator_average_impl.cpp:307-347): the first maximum
// of |x| over taps [0, HALF_CP) against the first maximum over [DFT - HALF_CP, DFT); the pilots lse[i] sit at subcarrier pos(i). By one
// wavefront: lane = the lane index within it.
template <typename POS>
__device__ float hop_time_alignment(const float2* lse, int npil, POS pos, int lane)
{
  uint64_t kd = 0, ka = 0; // (|x|^2 bits, ~tap): the maximum is the first maximum
  for (int t = lane; t < 2 * PUCCH_HALF_CP; t += 64) {
    const int tap = t < PUCCH_HALF_CP ? t : PUCCH_DFT - 2 * PUCCH_HALF_CP + t;
    float     re = 0.f, im = 0.f;
    for (int i = 0; i < npil; ++i) {
      float      s, c;
      const int  ph = (pos(i) * tap) & (PUCCH_DFT - 1);
      __sincosf(PUCCH_TWOPI * (float)ph / (float)PUCCH_DFT, &s, &c);
      re += lse[i].x * c - lse[i].y * s;
      im += lse[i].x * s + lse[i].y * c;
    }
    const uint64_t key = ((uint64_t)__float_as_uint(re * re + im * im) << 32) | (uint32_t)(0xffffffffu - (uint32_t)t);
    if (t < PUCCH_HALF_CP)
      kd = max(kd, key);
    else
      ka = max(ka, key);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    kd = max(kd, (uint64_t)__shfl_xor((long long)kd, off));
    ka = max(ka, (uint64_t)__shfl_xor((long long)ka, off));
  }
  const float    md = __uint_as_float((uint32_t)(kd >> 32)), ma = __uint_as_float((uint32_t)(ka >> 32));
  const uint32_t td = 0xffffffffu - (uint32_t)kd, ta = 0xffffffffu - (uint32_t)ka - PUCCH_HALF_CP;
  if (md >= ma)
    return (float)td;
  return -(float)(PUCCH_HALF_CP - ta);
}

struct port_csi {
  float epre, rsrp, noise, snr, ta;
};

// Final per-port quantities of port_channel_estimator_average_impl::compute (lines 97-138).
__device__ __forceinline__ port_csi finish_port(float epre, float rsrp, float noise, float ta, int nof_pilots_all, int window, int ndmrs_all,
                                                bool hop, int numerology)
{
  port_csi r;
  r.rsrp = rsrp / (float)nof_pilots_all;
  r.epre = epre / (float)nof_pilots_all;
  if (hop)
    ta /= 2.0f;
  r.ta  = ta / ((float)PUCCH_DFT * (float)(15 << numerology) * 1000.0f);
  noise = noise / (float)(window * ndmrs_all - 1);
  if (ndmrs_all < 3 || hop)
    noise = 0.001f * r.epre;
  r.noise = noise;
  r.snr   = noise != 0.f ? r.rsrp / noise : 1000.f;
  return r;
}

__device__ __forceinline__ float to_db(float v)
{
  return 10.0f * log10f(v);
}

} // namespace
