// Device code shared by the polar decoding kernels (polar.hip, uci_polar.hip): the reference's LLR algebra, the rate dematcher as a
// gather, and the pruned SSC schedule run by the lanes of one codeword on its LDS slice.
#pragma once
#include "polar_code.h"

// LLR algebra of log_likelihood_ratio.cpp:38-85 / .h:208-216.
__device__ __forceinline__ int llr_add(int a, int b)
{ // a + b (special cases inspect the right operand first, like `rhs += *this`)
  if (b == -a)
    return 0;
  if (b > 120 || b < -120)
    return b;
  if (a > 120 || a < -120)
    return a;
  return min(max(a + b, -120), 120);
}
__device__ __forceinline__ int llr_promotion_sum(int a, int b)
{
  if (a == -b)
    return 0;
  if (a > 120 || a < -120)
    return a;
  if (b > 120 || b < -120)
    return b;
  const int t = a + b;
  return (t > 120) ? 127 : ((t < -120) ? -127 : t);
}
__device__ __forceinline__ int llr_soft_xor(int x, int y)
{
  const int m = min(abs(x), abs(y));
  return (x * y < 0) ? -m : m;
}

// Rate dematching (polar_rate_dematcher_impl.cpp:29-118) of one codeword position as a gather: `first` is the position's rx_first
// entry, repetitions are accumulated in order.
__device__ __forceinline__ int polar_dematch_value(int first, int N, int E, const int8_t* __restrict__ f, const uint16_t* __restrict__ rx_fidx)
{
  if (first == -1)
    return 0;
  if (first == -2)
    return 127;
  int v = f[rx_fidx[first]];
  for (int k = first + N; k < E; k += N)
    v = llr_promotion_sum(v, f[rx_fidx[k]]);
  return v;
}

// The pruned SSC schedule (polar_decoder_impl.cpp:179-350) run by the W lanes of one codeword: L holds the stage-s LLRs at offset 2^s
// (the channel LLRs at N), est the partial sums, u the decisions; est and u start at zero. Every codeword of a workgroup runs the same
// schedule, so the barriers are uniform; the last one leaves u complete for every lane.
template <int W>
__device__ __forceinline__ void polar_ssc_run(int8_t* L, uint8_t* est, uint8_t* u, const uint32_t* __restrict__ sched, uint32_t sched_len, int lane)
{
  for (uint32_t k = 0; k < sched_len; ++k) {
    const uint32_t op   = sched[k];
    const int      type = op & 15, s = (op >> 4) & 15, pos = (int)(op >> 8);
    const int      size = 1 << s, half = size >> 1;
    int8_t*        ls   = L + size;
    int8_t*        lc   = L + half;
    if (type == POLAR_SSC_F) {
      for (int i = lane; i < half; i += W)
        lc[i] = (int8_t)llr_soft_xor(ls[i], ls[i + half]);
    } else if (type == POLAR_SSC_G) {
      for (int i = lane; i < half; i += W) {
        const int x = ls[i], y = ls[i + half];
        lc[i]       = (int8_t)(est[pos + i] ? llr_add(y, -x) : llr_add(y, x));
      }
    } else if (type == POLAR_SSC_R1) {
      for (int i = lane; i < size; i += W) {
        const uint8_t b = ls[i] <= 0;
        est[pos + i]    = b;
        u[pos + i]      = b;
      }
      __syncthreads();
      for (int h = 1; h < size; h <<= 1) { // re-encode the subtree (polar_decoder_impl.cpp:243-248)
        for (int t = lane; t < half; t += W) {
          const int b = ((t / h) * 2 * h) + (t % h);
          u[pos + b] ^= u[pos + b + h];
        }
        __syncthreads();
      }
    } else { // POLAR_SSC_COMB
      for (int i = lane; i < half; i += W)
        est[pos + i] ^= est[pos + half + i];
    }
    __syncthreads();
  }
}
