// Low-PAPR base sequences r_(u,v)(n) of TS 38.211 5.2.2 and the group / sequence hopping that selects (u, v), for every channel built on them: PUCCH
// formats 0, 3 and 4 (pucch_f0.hip, pucch_f34.hip), SRS (srs.hip) and the DM-RS of transform-precoded PUSCH (transform_precoding.hip). Host and device.
//   length 12: TS 38.211 Table 5.2.2.2-2, the row of shift 0 of tables/nr_low_papr_tables.h;
//   length 30: r(n) = exp(-j pi (u + 1)(n + 1)(n + 2) / 31);
//   length 36 and above: r(n) = x_q(n mod N_ZC), x_q(m) = exp(-j pi q m (m + 1) / N_ZC), N_ZC the largest prime below the length.
// Lengths 6, 18 and 24 need Tables 5.2.2.2-1, -3 and -4, which the library does not hold.
#pragma once
#include "gold_device.h"
#include "tables/nr_low_papr_tables.h"
#include <cmath>

// Up to 1620 elements: 6 per PRB of the widest transform-precoded allocation (270 PRBs).
__host__ __device__ inline bool low_papr_length_ok(unsigned len)
{
  return len == 12 || len == 30 || (len >= 36 && len % 6 == 0 && len <= 1620);
}
// N_ZC: the largest prime below len (36 <= len <= 1632); 0 below 36, where the sequences are not Zadoff-Chu.
__host__ __device__ inline unsigned low_papr_prime_below(unsigned len)
{
  for (unsigned c = len < 36 ? 0 : len - 1; c > 2; --c) {
    bool prime = true;
    for (unsigned d = 2; d * d <= c; ++d)
      if (c % d == 0) {
        prime = false;
        break;
      }
    if (prime)
      return c;
  }
  return 0;
}
// Root q of the Zadoff-Chu sequence of (u, v) with length N_ZC: floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = N_ZC (u+1) / 31; unused where nzc = 0.
__host__ __device__ inline unsigned low_papr_zc_root(unsigned u, unsigned v, unsigned nzc)
{
  const unsigned t = 2 * nzc * (u + 1);
  const int      q = (int)((t + 31) / 62) + (v ? (((t / 31) & 1u) ? -1 : 1) : 0);
  return (unsigned)q;
}
// Phase of element n as a fraction f of pi, r(n) = exp(-j pi f), reduced to [0, 2) in integers: len = 30 or len >= 36.
__host__ __device__ inline void low_papr_phase(unsigned u, unsigned q, unsigned nzc, unsigned len, unsigned n, unsigned& num, unsigned& den)
{
  if (len == 30) {
    num = ((u + 1) * (n + 1) * (n + 2)) % 62u, den = 31u;
    return;
  }
  const uint64_t m = n % nzc;
  num = (unsigned)(((uint64_t)q * m * (m + 1)) % (2ull * nzc)), den = nzc;
}

// r_(u,0)(n) of length 12.
__host__ __device__ __forceinline__ float2 low_papr12(unsigned u, unsigned n)
{
  return make_float2(NR_LOW_PAPR12[u][0][n][0], NR_LOW_PAPR12[u][0][n][1]);
}
// r_(u,v)(n) of length len = 12, 30 or >= 36 in single precision; q = low_papr_zc_root(u, v, nzc), nzc = low_papr_prime_below(len).
__device__ __forceinline__ float2 low_papr_element(unsigned u, unsigned q, unsigned nzc, unsigned len, unsigned n)
{
  if (len == 12)
    return low_papr12(u, n);
  unsigned num, den;
  low_papr_phase(u, q, nzc, len, n, num, den);
  float sn, cs;
  sincospif((float)num / (float)den, &sn, &cs);
  return make_float2(cs, -sn);
}
// The same element from double-precision angles, on the host.
inline float2 low_papr_element_host(unsigned u, unsigned q, unsigned nzc, unsigned len, unsigned n)
{
  if (len == 12)
    return low_papr12(u, n);
  unsigned num, den;
  low_papr_phase(u, q, nzc, len, n, num, den);
  const double a = M_PI * (double)num / (double)den;
  return make_float2((float)std::cos(a), (float)-std::sin(a));
}

// Group and sequence hopping of symbol l_abs of the slot (TS 38.211 6.4.1.1.1.2, 6.4.1.4.2), by one lane. hopping 1: f_gh = the eight Gold bits from
// 8 (14 n_s + l) of c_init_group (the DM-RS: floor(n_id / 30); SRS: n_id), modulo 30. hopping 2: v = c(14 n_s + l) of c_init = n_id where len >= 72.
// u = (f_gh + n_id) mod 30.
__device__ __forceinline__ void low_papr_hop(const gold_tables& gt, unsigned hopping, uint32_t c_init_group, uint32_t n_id, uint32_t slot, uint32_t l_abs,
                                             unsigned len, uint32_t& u, uint32_t& v)
{
  uint32_t f_gh = v = 0;
  if (hopping == 1) {
    const uint32_t off = 8u * (14u * slot + l_abs);
    f_gh               = ((gold_state(gt, false, 0, off) ^ gold_state(gt, true, c_init_group, off)) & 0xffu) % 30u;
  } else if (hopping == 2 && len >= 72) {
    const uint32_t off = 14u * slot + l_abs;
    v                  = (gold_state(gt, false, 0, off) ^ gold_state(gt, true, n_id, off)) & 1u;
  }
  u = (f_gh + n_id) % 30u;
}
