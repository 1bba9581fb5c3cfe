// Device functions shared by the PUCCH kernels and the SRS estimator. Included by pucch.hip (formats 1 and 2) and pucch_f34.hip (formats 3 and 4):
// Gold-sequence words, the cyclic shift of a symbol, the time alignment of one hop, the final per-port quantities of
// port_channel_estimator_average_impl::compute, their sum over the ports and the record written from it; by pucch_f0.hip (format 0) and srs.hip:
// to_db and, through wave_device.h, the wavefront sum and the complex products.
#pragma once
#include "gold_device.h"
#include "miphy_internal.h"
#include "wave_device.h"

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

// Cyclic-shift index of symbol l_abs of the slot (TS 38.211 6.3.2.2.2): alpha = (m0 + n_cs(n_s, l)) mod 12 in twelfths of a turn, n_cs = the eight
// Gold bits c(8 (14 n_s + l) .. + 7) of c_init = n_id. Formats 1, 3 and 4; format 0 takes both of its symbols' n_cs in one wavefront jump.
__device__ __forceinline__ int pucch_alpha(const gold_tables& gt, uint32_t n_id, uint32_t slot, uint32_t l_abs, uint32_t m0)
{
  return (int)((m0 + (gold_word(gt, n_id, 8u * (14u * slot + l_abs)) & 0xffu)) % 12u);
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

// The CSI of a coherent PDU: the per-port quantities added in port order (channel_estimation.h:211-233 averages them linearly) and the noise variance
// of the first port, which the equaliser takes.
struct pucch_csi_sum {
  float epre = 0.f, rsrp = 0.f, snr = 0.f, ta = 0.f, noise0 = 0.f;

  __device__ __forceinline__ void add(const port_csi& c, bool is_first_port)
  {
    epre += c.epre, rsrp += c.rsrp, snr += c.snr, ta += c.ta;
    noise0 = is_first_port ? c.noise : noise0;
  }
};
// The record of a PDU on nports ports, by one lane.
__device__ __forceinline__ void pucch_write_result(miphy_pucch_result& r, const pucch_csi_sum& sum, int nports, uint8_t status, float detection_metric)
{
  const float np = (float)nports;
  r.status = status, r.detection_metric = detection_metric, r.time_alignment_s = sum.ta / np;
  r.epre_db = to_db(sum.epre / np), r.rsrp_db = to_db(sum.rsrp / np), r.sinr_db = to_db(sum.snr / np);
}

} // namespace
