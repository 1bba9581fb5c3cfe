// Transform de-precoding of one DFT-s-OFDM symbol (TS 38.211 6.3.1.4, receive side) in LDS, shared by the stand-alone de-precoder
// (transform_precoding.hip, miphy_transform_deprecode_batch) and the fused demodulator (pusch_demod.hip, miphy_pusch_demodulate_tp_batch): the same
// equalised elements give the same bits through either kernel.
//   y[n] = (1 / sqrt(M)) sum_k x[k] e^(+j 2 pi k n / M),   M = 12 N_PRB,  N_PRB = 2^a 3^b 5^c <= 270 (53 sizes, 12 ... 3240)
//   v    = (sum over the normal elements of v[k]) / (number of normal elements);  +inf when no element is normal.
// An element is normal when its noise variance is positive and finite; any other element (the equaliser marks one it could not invert with symbol 0
// and variance +inf) enters the IDFT as 0 and is left out of the mean.
//
// Geometry: a workgroup of TP_THREADS = 256 lanes per symbol, the Stockham passes of fft_device.h on one padded LDS buffer (M = 3240: 29 KB, five
// workgroups = 20 wavefronts per CU by LDS); radix 8, 4, 2, 3 and 5 passes in that order, the non-power-of-two strides last. 256 lanes cover the
// N / 16 butterflies-per-lane bound of fft_pass up to M = 4096.
// Order of the additions of v, whatever the launch: lane t adds the elements t, t + 256, t + 512, ... in ascending order (tp_put), the 64 lanes of a
// wavefront add by the xor tree 32, 16, ... 1, the four wavefronts in sequence.
#pragma once
#include "fft_device.h"

constexpr int TP_THREADS  = 256;
constexpr int TP_MAX_PRB  = 270;
constexpr int TP_MAX_M    = 12 * TP_MAX_PRB;
constexpr int TP_PER_LANE = (TP_MAX_M + TP_THREADS - 1) / TP_THREADS; // 13

// Whether nprb PRBs are a transform-precoding allocation: 2^a 3^b 5^c, at most 270.
__host__ __device__ __forceinline__ bool tp_nprb_ok(unsigned nprb)
{
  if (nprb < 1 || nprb > (unsigned)TP_MAX_PRB)
    return false;
  while (nprb % 2 == 0)
    nprb /= 2;
  while (nprb % 3 == 0)
    nprb /= 3;
  while (nprb % 5 == 0)
    nprb /= 5;
  return nprb == 1;
}
__host__ __device__ __forceinline__ bool tp_size_ok(unsigned M)
{
  return M % 12 == 0 && tp_nprb_ok(M / 12);
}

// The allocation of a five-word PRB mask on a grid of grid_nof_prb PRBs: its first PRB and PRB count; false when it is empty or not contiguous.
__host__ __device__ __forceinline__ bool tp_contiguous(const uint64_t* rb_mask, unsigned grid_nof_prb, unsigned& first, unsigned& count)
{
  first = count = 0;
  if (grid_nof_prb < 1 || grid_nof_prb > 275)
    return false;
  count = miphy_count_prb(rb_mask, grid_nof_prb);
  if (count == 0)
    return false;
  uint64_t m[5];
  bool     found = false;
#pragma unroll
  for (int w = 0; w < 5; ++w) { // the words with the bits behind the grid masked off; the first set bit
    const int left = (int)grid_nof_prb - 64 * w;
    m[w]           = left <= 0 ? 0ull : (rb_mask[w] & (left >= 64 ? ~0ull : ((1ull << left) - 1ull)));
    if (!found && m[w]) {
      first = 64u * w + (unsigned)__builtin_ctzll(m[w]);
      found = true;
    }
  }
  bool ok = true;
#pragma unroll
  for (int w = 0; w < 5; ++w) { // every word holds its part of [first, first + count) and nothing else
    const int      lo = (int)first > 64 * w ? (int)first : 64 * w, hi = (int)(first + count) < 64 * w + 64 ? (int)(first + count) : 64 * w + 64;
    const uint64_t e  = lo < hi ? ((hi - lo == 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << (lo - 64 * w)) : 0ull;
    ok                = ok && m[w] == e;
  }
  return ok;
}

// A lane's part of the variance mean.
struct tp_var_acc {
  float sum = 0.f;
  int   cnt = 0;
};

// Element k (k = tid + TP_THREADS c, a lane takes its c in ascending order) of the symbol into the LDS buffer.
__device__ __forceinline__ void tp_put(cplx* x, int k, float2 sym, float var, tp_var_acc& acc)
{
  const bool normal = var > 0.f && var < INFINITY;
  x[fpad(k)]        = normal ? cplx{sym.x, sym.y} : cplx{0.f, 0.f};
  if (normal) {
    acc.sum = acc.cnt ? acc.sum + var : var;
    ++acc.cnt;
  }
}

// Every lane of the TP_THREADS-lane workgroup calls it once its elements are in x (tp_put). tw: exp(-2 pi i j / M), j < M. red: 8 floats of LDS.
// Returns v; x then holds sqrt(M) y[n] at fpad(n), visible to every lane: tp_symbol(x, n, scale) with scale = tp_scale(M) is y[n].
__device__ __forceinline__ float tp_deprecode_symbol(cplx* x, int M, const cplx* __restrict__ tw, const tp_var_acc& acc, float* red, int tid)
{
  float s = acc.sum;
  int   c = acc.cnt;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    c += __shfl_xor(c, off);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6]                    = s;
    red[4 + (tid >> 6)]              = __int_as_float(c);
  }
  __syncthreads(); // the elements and the partial sums are in LDS
  const float sum = ((red[0] + red[1]) + red[2]) + red[3];
  const int   cnt = __float_as_int(red[4]) + __float_as_int(red[5]) + __float_as_int(red[6]) + __float_as_int(red[7]);
  fft_lds<true, true>(x, M, tw, tid, TP_THREADS);
  return cnt ? sum / (float)cnt : INFINITY;
}
__device__ __forceinline__ float tp_scale(int M)
{
  return 1.0f / sqrtf((float)M);
}
__device__ __forceinline__ float2 tp_symbol(const cplx* x, int n, float scale)
{
  const cplx v = x[fpad(n)];
  return make_float2(v.x * scale, v.y * scale);
}
