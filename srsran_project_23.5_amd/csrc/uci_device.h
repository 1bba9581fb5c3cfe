// UCI short-block detector of one field by one wavefront, shared by the UCI decoder (uci.hip) and the PUCCH format-2 pipeline
// (pucch.hip). See uci.hip for the behaviour contract and the arithmetic.
#pragma once
#include "miphy_internal.h"

// The reference's preconditions (validate_spans, short_block_detector_impl.cpp:58-83) plus the modulation orders it knows.
__host__ __device__ static inline bool miphy_uci_job_ok(uint32_t K, uint32_t Qm, uint32_t E)
{
  if (K < 1 || K > 11 || !(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8) || E > (1u << 31))
    return false;
  return K > 2 ? E > K : E >= (K == 1 ? Qm : 3 * Qm);
}

// TS 38.212 Table 5.3.3.3-1, row i = output bit i; the leftmost binary digit is M_{i,0}, the rightmost M_{i,10}.
constexpr uint16_t TS_BASIS_ROWS[32] = {
    0b11000000001, 0b11100000011, 0b10010010111, 0b10110000101, 0b11110001001, 0b11001011101, 0b10101010111, 0b10011001101,
    0b11011001011, 0b10111010011, 0b10100111011, 0b11100110101, 0b10010101111, 0b11010101011, 0b10001101001, 0b11001111011,
    0b11101110010, 0b10011100100, 0b11011111000, 0b10000110000, 0b10100010001, 0b11010000011, 0b10001001101, 0b11101000111,
    0b11111011110, 0b11000111001, 0b10110100110, 0b11110101110, 0b10101110100, 0b10111111100, 0b11111111111, 0b10000000000};

// Basis sequence n as a 32-bit mask (bit i = M_{i,n}).
__host__ __device__ static constexpr uint32_t basis_column(int n)
{
  uint32_t m = 0;
  for (int i = 0; i < 32; ++i)
    m |= static_cast<uint32_t>((TS_BASIS_ROWS[i] >> (10 - n)) & 1u) << i;
  return m;
}

// Detection thresholds of the GLRT per message length K = 1..11 (short_block_detector_impl.cpp:196-199).
static __device__ __forceinline__ double uci_threshold(uint32_t K)
{
  switch (K) {
    case 3: return 12;
    case 4: return 14;
    case 5: return 16;
    case 6: return 18;
    case 7: return 20;
    case 8: return 22;
    case 9: return 24;
    case 10: return 26;
    case 11: return 29;
    default: return 0;
  }
}

// log_likelihood_ratio::operator+= (lib/phy/upper/log_likelihood_ratio.cpp:38-70).
static __device__ __forceinline__ int llr_add(int a, int b)
{
  if (a == -b)
    return 0;
  if (a == 127 || a == -127)
    return a;
  if (b == 127 || b == -127)
    return b;
  return min(max(a + b, -120), 120);
}

// One field of K = 1..11 bits (miphy_uci_job_ok holds) by the whole wavefront: E soft bits at llr (global or LDS), K payload bytes to
// out, the verdict to *status. lane: the lane index within the wavefront; every lane of the wavefront must call it.
static __device__ __forceinline__ void uci_short_block_field(uint32_t K, uint32_t Qm, uint32_t E, const int8_t* llr, uint8_t* out, uint8_t* status,
                                                      uint32_t lane)
{
  const uint32_t L = K == 1 ? Qm : (K == 2 ? 3 * Qm : 32);

  // Rate dematch: one accumulator per lane, its positions in input order.
  int acc = 0;
  if (lane < L) {
    const int8_t* p = llr;
#pragma unroll 8
    for (uint32_t i = lane; i < E; i += L)
      acc = llr_add(acc, p[i]);
  }

  if (K == 1) { // bit = tmp[0] > 0 ? 0 : 1, metric 1 > threshold 0: always valid
    if (lane == 0) {
      out[0]    = acc > 0 ? 0 : 1;
      *status = MIPHY_UCI_STATUS_VALID;
    }
    return;
  }

  if (K == 2) { // short_block_detector_impl.cpp:85-122: combine the repeated symbols, correlate with the four codewords
    int x0, x1, x2;
    if (Qm == 1) {
      x0 = __builtin_amdgcn_readlane(acc, 0), x1 = __builtin_amdgcn_readlane(acc, 1), x2 = __builtin_amdgcn_readlane(acc, 2);
    } else {
      const uint32_t s = Qm - 2; // in_size / 3 - 2
      x0 = __builtin_amdgcn_readlane(acc, 0) + __builtin_amdgcn_readlane(acc, s + 3);
      x1 = __builtin_amdgcn_readlane(acc, 1) + __builtin_amdgcn_readlane(acc, 2 * s + 4);
      x2 = __builtin_amdgcn_readlane(acc, s + 2) + __builtin_amdgcn_readlane(acc, 2 * s + 5);
    }
    if (lane == 0) {
      const int corr[4] = {x0 + x1 + x2, -x0 + x1 - x2, x0 - x1 - x2, -x0 - x1 + x2};
      int       best = 0, idx = 0; // the reference starts at DBL_MIN: an integer correlation wins only from 1 on
      for (int c = 0; c < 4; ++c)
        if (corr[c] > best)
          best = corr[c], idx = c;
      const double m2     = static_cast<double>(best) * best;
      const double norm   = static_cast<double>(x0 * x0 + x1 * x1 + x2 * x2);
      const double metric = 2.0 * m2 / (3.0 * norm - m2);
      out[0] = idx & 1, out[1] = (idx >> 1) & 1;
      *status = metric > 0.0 ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
    }
    return;
  }

  // 3..11 bits: the 32 dematched values, wave-uniform.
  int x[32];
  int sum = 0, norm = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    x[i] = __builtin_amdgcn_readlane(acc, i);
    sum += x[i], norm += x[i] * x[i];
  }
  uint32_t lo = 0; // codeword of message bits 1..6 = the lane index
#pragma unroll
  for (int b = 0; b < 6; ++b)
    lo ^= ((lane >> b) & 1u) ? basis_column(b + 1) : 0u;
  const uint32_t ncw = 1u << (K - 1);
  uint32_t       key = 0; // |corr| << 11 | (1023 - idx) << 1 | (corr < 0): the maximum is the reference's first maximum
  for (uint32_t r = 0; r < 16 && 64 * r < ncw; ++r) {
    const uint32_t idx = lane + 64 * r;
    uint32_t       m   = lo; // message bits 7..10 = r
#pragma unroll
    for (int b = 0; b < 4; ++b)
      m ^= ((r >> b) & 1u) ? basis_column(b + 7) : 0u;
    int ones = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      ones += ((m >> i) & 1u) ? x[i] : 0;
    const int      corr = sum - 2 * ones;
    const uint32_t k    = (static_cast<uint32_t>(abs(corr)) << 11) | ((1023u - idx) << 1) | (corr < 0 ? 1u : 0u);
    if (idx < ncw)
      key = max(key, k);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    key = max(key, static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), off)));
  const uint32_t best = key >> 11, idx = 1023u - ((key >> 1) & 1023u), v = 2 * idx + (key & 1u);
  if (lane < K)
    out[lane] = (v >> lane) & 1u; // payload bit k = bit k of 2 idx + bit0
  if (lane == 0) {
    const double m2     = static_cast<double>(best) * best;
    const double metric = 31.0 * m2 / (32.0 * static_cast<double>(norm) - m2);
    *status             = metric > uci_threshold(K) ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
  }
}
