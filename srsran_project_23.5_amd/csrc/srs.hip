// SRS channel estimator (TS 38.211 6.4.1.4), for a batch of jobs that share one device grid: per-PRG channel matrices H[g][rx][tx], the wideband matrix, the
// noise variance, EPRE, RSRP per transmit port, SINR and one time alignment per job. Beyond the 23.5 reference, which has no SRS code; the contract is the
// standard, restated in numpy in tests/srs_tx.py (transmitter) and tests/srs_ref.py (float64 receiver).
//
// The signal, normal cyclic prefix. n_cs_max = 8 (K = 2) or 12 (K = 4). Transmit port i: n_cs,i = (n_cs + n_cs_max i / N_ap) mod n_cs_max; its comb offset is
// (kbar + K / 2) mod K when N_ap = 4, i is 1 or 3 and n_cs >= n_cs_max / 2, else kbar. M = 12 nof_prb / K. Element n of symbol l sits on subcarrier
// 12 start_prb + offset_i + K n and carries r_(u,v)(n) e^(j 2 pi n_cs,i n / n_cs_max). (u, v) by the group and sequence hopping of low_papr_device.h
// (low_papr_hop with c_init = n_id for the group; l is the symbol index in the slot); r is the base sequence of that header: the table at length 12, from
// 36 on Zadoff-Chu with the phases of low_papr_phase (reduced in 64-bit integers; N_ZC up to 1627).
//
// The arithmetic. P = the ports that share a comb (N_ap, or 2 on each of two combs when four ports split), Q = 12 prg_size / K elements per PRG, a
// multiple of P (a rule), G = nof_prb / prg_size. Per comb c in use, n_ref = the cyclic shift of its lowest port, d_i = (n_cs,i - n_ref) mod n_cs_max:
//  1. z_(r,l,c)[n] = y_r[l, 12 start_prb + c + K n] conj(r_(u_l,v_l)(n)) e^(-j 2 pi n_ref n / n_cs_max).
//  2. Delay, one per job: C = sum_(r,l,c) sum_(n < M - P) z[n + P] conj(z[n]); phi = atan2(Im C, Re C); theta = phi / (K P) rad per subcarrier;
//     time_alignment_s = -theta / (2 pi 15 kHz 2^numerology), 0 when C = 0. The products are single precision, their sum and phi double. The ports of
//     a comb sit at relative shifts of whole multiples of 2 pi / P, so at lag P they add coherently; the range is |tau| < 1 / (2 delta_f K P).
//  3. Per PRG g (elements g Q .. (g + 1) Q - 1, centre n_c = g Q + (Q - 1) / 2), receive port r and port i of the comb:
//     H[g][r][i] = (1 / (L Q)) sum_l sum_n z[n] e^(-j theta K (n - n_c)) e^(-j 2 pi d_i n / n_cs_max): the channel at the PRG's centre element as the grid
//     shows it. hhat = H e^(-j theta K n_c) is the delay-compensated estimate (the mean of w[n] = z[n] e^(-j theta K n)); H_wb[r][i] = mean_g hhat.
//     The compensation is referred to the PRG centre so that its angles stay small in single precision; the one large angle per PRG, theta K n_c, is
//     reduced in double.
//  4. Residual, computed directly (a difference of energies cancels in single precision at high SNR):
//     e[n] = z[n] e^(-j theta K (n - n_c)) - sum_(i on the comb) H[g][r][i] e^(+j 2 pi d_i n / n_cs_max), the same magnitude as w[n] - sum hhat e^(...).
//     noise_var = sum |e|^2 / (R |combs| (L M - G P)); the denominator is positive: Q is 3, 6, 12 or 24 and a multiple of P = 1, 2 or 4, so Q > P.
//  5. EPRE = mean |y|^2 over the SRS elements; rsrp_i = mean over (r, g) of |hhat|^2; sinr = mean_i rsrp_i / noise_var.
// The estimator takes the comb to carry the job's ports and nothing else. UEs that share a comb at cyclic shifts n_cs_max / P apart are the ports of one
// job with that P: each is then separated from the others over whole periods.
//
// Geometry: one workgroup of 256 lanes per job. conj(r_(u_l,v_l)) goes to LDS once (one copy without hopping, one per symbol with it: at most 52 KB); u, v
// and the Zadoff-Chu root are computed once per symbol. The grid (up to 209 KB per job) is not staged; it is read twice, the second time from L2.
// Phase A: lane t takes the lag products n = t, t + 256, ... of every (r, l, c) row in ascending row order; the 64 lanes of a wavefront add by the xor
// tree 32, 16, ... 1, the four wavefronts in sequence. Phase B: wavefront w takes the pairs (g, r) = w, w + 4, ... (pair = g R + r); a comb's L Q <= 96
// elements of the pair sit in two registers per lane (element e and e + 64, added in that order, then the xor tree), so H and then the residual come
// from the same loads; the wavefront's sums over its pairs are kept in LDS in pair order, and lane 0 adds the four wavefronts in sequence. Every sum has
// an order that depends on the job alone: a job's output is bit-identical whatever else is in the call. No atomics.
#include "low_papr_device.h"
#include "miphy_ext.h"
#include "pucch_device.h"
#include <algorithm>
#include <cmath>

struct srs_derived {
  uint32_t M, Q, P, G, ncombs, ncs_max;
  uint8_t  cs[4], off[4];
};

// What follows from a job's fields (any job: nothing here divides by a field).
__host__ __device__ static inline void miphy_srs_derive(const miphy_srs_job& j, srs_derived& d)
{
  const uint32_t K = j.comb_size == 4 ? 4u : 2u, nap = j.nof_tx_ports == 4 ? 4u : (j.nof_tx_ports == 2 ? 2u : 1u);
  d.ncs_max          = K == 4 ? 12u : 8u;
  const bool split   = nap == 4 && j.cyclic_shift >= d.ncs_max / 2;
  d.M                = 12u * j.nof_prb / K;
  const uint32_t prg = j.prg_size == 4 ? 4u : (j.prg_size == 2 ? 2u : 1u);
  d.Q = 12u * prg / K, d.G = j.nof_prb / prg;
  d.ncombs = split ? 2u : 1u, d.P = split ? 2u : nap;
  for (uint32_t i = 0; i < 4; ++i) {
    d.cs[i]  = i < nap ? (uint8_t)((j.cyclic_shift + d.ncs_max * i / nap) % d.ncs_max) : 0;
    d.off[i] = i < nap ? (uint8_t)((split && (i & 1u)) ? (j.comb_offset + K / 2) % K : j.comb_offset) : 0;
  }
}

// The rules of one job, for the host and for the kernels (device jobs the host could not check): 0, or the number of the first rule it breaks
// (SRS_RULE_TEXT). Rule SRS_RULE_UNSUPP is MIPHY_EUNSUPP, the others MIPHY_EINVAL.
constexpr int SRS_RULE_UNSUPP = 12;
__host__ __device__ static inline int miphy_srs_rule(const miphy_srs_job& j)
{
  if (j.numerology > 4 || j.slot >= (10u << j.numerology))
    return 1;
  if (j.nof_rx_ports < 1 || j.nof_rx_ports > 4)
    return 2;
  if (j.nof_tx_ports != 1 && j.nof_tx_ports != 2 && j.nof_tx_ports != 4)
    return 3;
  if ((j.nof_symbols != 1 && j.nof_symbols != 2 && j.nof_symbols != 4) || j.start_symbol > 13 || j.start_symbol + j.nof_symbols > 14)
    return 4;
  if ((j.comb_size != 2 && j.comb_size != 4) || j.comb_offset >= j.comb_size)
    return 5;
  if (j.cyclic_shift >= (j.comb_size == 4 ? 12 : 8))
    return 6;
  if (j.n_id > 1023)
    return 7;
  if (j.hopping > 2)
    return 8;
  if (j.prg_size != 1 && j.prg_size != 2 && j.prg_size != 4)
    return 9;
  if (j.nof_prb < 4 || j.nof_prb > 272 || j.nof_prb % 4 != 0)
    return 10;
  if (j.grid_nprb < 1 || j.grid_nprb > 275 || (uint32_t)j.start_prb + j.nof_prb > j.grid_nprb)
    return 11;
  srs_derived d;
  miphy_srs_derive(j, d);
  if (d.M == 24)
    return SRS_RULE_UNSUPP;
  if (d.Q % d.P != 0)
    return 13;
  return 0;
}

namespace {

const char* const SRS_RULE_TEXT[14] = {"",
                                       "the slot lies outside the frame of the numerology (0..4)",
                                       "invalid number of receive ports (1..4)",
                                       "invalid number of transmit ports (1, 2 or 4)",
                                       "invalid symbol range (1, 2 or 4 symbols within the slot)",
                                       "comb_size is 2 or 4 and comb_offset below it",
                                       "cyclic_shift is below 8 (comb 2) or 12 (comb 4)",
                                       "n_id is 0..1023",
                                       "hopping is 0 (neither), 1 (group) or 2 (sequence)",
                                       "prg_size is 1, 2 or 4 PRBs",
                                       "nof_prb is a multiple of 4 in 4..272",
                                       "the allocation leaves the grid window (1..275 PRBs)",
                                       "a sequence of 24 elements needs TS 38.211 Table 5.2.2.2-4, which the library does not hold",
                                       "the comb elements of a PRG (12 prg_size / comb_size) are not a multiple of the ports that share the comb"};

constexpr int SRS_THREADS = 256;
constexpr int SRS_MAX_M   = 1632;

// e^(-j 2 pi m / 24): the cyclic shifts of both combs (n_cs_max = 8: m = 3 a; 12: m = 2 a).
__constant__ float SRS_TW[24][2] = {{1.0f, -0.0f},
                                    {0.965925826289068287f, -0.258819045102520762f},
                                    {0.866025403784438647f, -0.5f},
                                    {0.707106781186547524f, -0.707106781186547524f},
                                    {0.5f, -0.866025403784438647f},
                                    {0.258819045102520762f, -0.965925826289068287f},
                                    {0.0f, -1.0f},
                                    {-0.258819045102520762f, -0.965925826289068287f},
                                    {-0.5f, -0.866025403784438647f},
                                    {-0.707106781186547524f, -0.707106781186547524f},
                                    {-0.866025403784438647f, -0.5f},
                                    {-0.965925826289068287f, -0.258819045102520762f},
                                    {-1.0f, 0.0f},
                                    {-0.965925826289068287f, 0.258819045102520762f},
                                    {-0.866025403784438647f, 0.5f},
                                    {-0.707106781186547524f, 0.707106781186547524f},
                                    {-0.5f, 0.866025403784438647f},
                                    {-0.258819045102520762f, 0.965925826289068287f},
                                    {0.0f, 1.0f},
                                    {0.258819045102520762f, 0.965925826289068287f},
                                    {0.5f, 0.866025403784438647f},
                                    {0.707106781186547524f, 0.707106781186547524f},
                                    {0.866025403784438647f, 0.5f},
                                    {0.965925826289068287f, 0.258819045102520762f}};

// x mod n_cs_max with the two moduli as constants: a division by a register costs some thirty instructions, and the PRG loop takes it per element.
__device__ __forceinline__ uint32_t srs_mod(uint32_t x, uint32_t ncs_max)
{
  return ncs_max == 8 ? (x & 7u) : x % 12u;
}
// e^(-j 2 pi a n / n_cs_max), the product a n reduced in integers; unit = 24 / n_cs_max.
__device__ __forceinline__ float2 srs_shift(uint32_t a, uint32_t n, uint32_t ncs_max, uint32_t unit)
{
  const uint32_t m = srs_mod(a * n, ncs_max) * unit;
  return make_float2(SRS_TW[m][0], SRS_TW[m][1]);
}

// Sequence group, sequence number and Zadoff-Chu root of symbol l_abs of the slot (one lane).
__device__ __forceinline__ void srs_uvq(const gold_tables& gt, const miphy_srs_job& j, uint32_t M, uint32_t nzc, uint32_t l_abs, uint32_t& u, uint32_t& q)
{
  uint32_t v;
  low_papr_hop(gt, j.hopping, j.n_id, j.n_id, j.slot, l_abs, M, u, v);
  q = low_papr_zc_root(u, v, nzc);
}

// r_(u,v)(n) e^(j 2 pi a n / n_cs_max) with one angle: the base sequence's phase -pi num / den and the shift's 2 pi a n / n_cs_max over the common
// denominator, reduced in integers (below 2 den n_cs_max <= 39048). M = 12: the table times the shift.
__device__ __forceinline__ float2 srs_element(uint32_t M, uint32_t u, uint32_t q, uint32_t nzc, uint32_t n, uint32_t a, uint32_t ncs_max)
{
  if (M == 12)
    return cmulc(low_papr12(u, n), srs_shift(a, n, ncs_max, 24u / ncs_max));
  unsigned num, den;
  low_papr_phase(u, q, nzc, M, n, num, den);
  const uint32_t full = 2u * den * ncs_max;
  const uint32_t t    = (2u * den * srs_mod(a * n, ncs_max) + full - num * ncs_max) % full; // the angle is pi t / (den n_cs_max)
  float          sn, cs;
  sincospif((float)t / (float)(den * ncs_max), &sn, &cs);
  return make_float2(cs, sn);
}

// One workgroup per (job, symbol of the job): the transmitted sequences [symbol][tx port][M] from pilots_offset.
__global__ void __launch_bounds__(SRS_THREADS) srs_pilots_kernel(const miphy_srs_job* __restrict__ jobs, const gold_tables* __restrict__ gt, float2* __restrict__ pilots)
{
  __shared__ uint32_t     uq[3];
  const miphy_srs_job j = load_words(jobs + blockIdx.x);
  const uint32_t      l = blockIdx.y;
  if (miphy_srs_rule(j) != 0 || l >= j.nof_symbols) // uniform
    return;
  srs_derived d;
  miphy_srs_derive(j, d);
  if (threadIdx.x == 0) {
    uq[2] = low_papr_prime_below(d.M);
    srs_uvq(*gt, j, d.M, uq[2], j.start_symbol + l, uq[0], uq[1]);
  }
  __syncthreads();
  const uint32_t u = uq[0], q = uq[1], nzc = uq[2];
  float2*        out = pilots + j.pilots_offset + (size_t)l * j.nof_tx_ports * d.M;
  for (uint32_t e = threadIdx.x; e < j.nof_tx_ports * d.M; e += SRS_THREADS) {
    const uint32_t i = e / d.M, n = e - i * d.M;
    out[e]           = srs_element(d.M, u, q, nzc, n, d.cs[i], d.ncs_max);
  }
}

// What the four wavefronts add up over their pairs, per wavefront, in LDS.
struct srs_sums {
  float hwb[4][4][2]; // [r][i]: sum_g hhat
  float rsrp[4];      // [i]: sum_(r,g) |hhat|^2
  float noise, epre;
};

__global__ void __launch_bounds__(SRS_THREADS) srs_estimate_kernel(const miphy_srs_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                                   const float2* __restrict__ grid, float2* __restrict__ h_out,
                                                                   miphy_srs_result* __restrict__ results)
{
#pragma clang fp contract(off)
  extern __shared__ float2 seq[]; // conj(r_(u_l,v_l)(n)) at [copy][n]; one copy without hopping
  __shared__ uint32_t      uq[4][2];
  __shared__ uint32_t      s_nzc;
  __shared__ double        red[8];
  __shared__ srs_sums      sums[4];
  const int           tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const miphy_srs_job j = load_words(jobs + blockIdx.x);
  if (miphy_srs_rule(j) != 0) // a device job the host could not check: nothing is written
    return;
  srs_derived d;
  miphy_srs_derive(j, d);
  const uint32_t M = d.M, Q = d.Q, P = d.P, G = d.G, K = j.comb_size, R = j.nof_rx_ports, L = j.nof_symbols, nap = j.nof_tx_ports;
  const uint32_t unit = 24u / d.ncs_max, ncopies = j.hopping ? L : 1u;
  const int      nsc  = 12 * (int)j.grid_nprb;
  const float2*  g0   = grid + j.grid_offset + 12u * j.start_prb;

  // ---- the sequences
  if (tid == 0)
    s_nzc = low_papr_prime_below(M);
  for (uint32_t i = tid; i < 4 * (sizeof(srs_sums) / sizeof(float)); i += SRS_THREADS)
    reinterpret_cast<float*>(sums)[i] = 0.f;
  __syncthreads();
  if ((uint32_t)tid < ncopies)
    srs_uvq(*gt, j, M, s_nzc, j.start_symbol + tid, uq[tid][0], uq[tid][1]);
  __syncthreads();
  for (uint32_t e = tid; e < ncopies * M; e += SRS_THREADS) {
    const uint32_t c = e / M, n = e - c * M;
    seq[e]           = cconj(srs_element(M, uq[c][0], uq[c][1], s_nzc, n, 0, d.ncs_max));
  }
  __syncthreads();

  // comb c of the job: its offset and the cyclic shift of its lowest port (ports 0 and 1 are the lowest of the two combs of a split)
  const uint32_t off0 = d.off[0], off1 = d.off[1], ref0 = d.cs[0], ref1 = d.cs[1];
  auto z_of = [&](uint32_t r, uint32_t l, uint32_t c, uint32_t n, float& energy) {
    const float2 y = g0[((size_t)r * 14 + j.start_symbol + l) * nsc + (c ? off1 : off0) + K * n];
    energy         = y.x * y.x + y.y * y.y;
    return cmul(cmul(y, seq[(j.hopping ? l : 0u) * M + n]), srs_shift(c ? ref1 : ref0, n, d.ncs_max, unit));
  };

  // ---- phase A: the delay
  // The products are single precision; they are added, and phi is taken, in double: hhat turns by n_c d(phi) / P, and at n_c = 1632 one unit in the
  // last place of a single-precision phi (2.4e-7 rad) would already be 4e-4 rad there.
  double Cx = 0.0, Cy = 0.0;
  for (uint32_t row = 0; row < R * L * d.ncombs; ++row) {
    const uint32_t c = row % d.ncombs, l = (row / d.ncombs) % L, r = row / (d.ncombs * L);
    for (uint32_t n = tid; n + P < M; n += SRS_THREADS) {
      float        en;
      const float2 t = cmulc(z_of(r, l, c, n + P, en), z_of(r, l, c, n, en));
      Cx += (double)t.x, Cy += (double)t.y;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    Cx += __shfl_xor(Cx, off), Cy += __shfl_xor(Cy, off);
  if (lane == 0)
    red[2 * wave] = Cx, red[2 * wave + 1] = Cy;
  __syncthreads();
  Cx = ((red[0] + red[2]) + red[4]) + red[6], Cy = ((red[1] + red[3]) + red[5]) + red[7];
  const double phi    = (Cx == 0.0 && Cy == 0.0) ? 0.0 : atan2(Cy, Cx);
  const double turnsd = phi / (6.283185307179586476925 * (double)P); // theta K in turns per comb element
  const float  turns  = (float)turnsd;

  // ---- phase B: the PRGs
  const float    inv_lq = 1.0f / (float)(L * Q);
  const uint32_t LQ     = L * Q;
  for (uint32_t pair = wave; pair < G * R; pair += 4) {
    const uint32_t g = pair / R, r = pair - g * R;
    const float    n_c = (float)(g * Q) + 0.5f * (float)(Q - 1);
    float          sn, cs;
    {
      double x = turnsd * (double)n_c;
      x -= rint(x);
      sincospif((float)(-2.0 * x), &sn, &cs);
    }
    const float2 back = make_float2(cs, sn); // e^(-j theta K n_c)
    float        noise = 0.f, epre = 0.f;
    for (uint32_t c = 0; c < d.ncombs; ++c) {
      // element e = l Q + nq of the pair and comb: lane and lane + 64
      float2   w[2];
      uint32_t nn[2];
      float    en2 = 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint32_t e = lane + 64u * k;
        w[k] = make_float2(0.f, 0.f), nn[k] = 0;
        if (e < LQ) {
          const uint32_t l = (e >= Q) + (e >= 2 * Q) + (e >= 3 * Q), n = g * Q + (e - l * Q); // l = e / Q, L <= 4
          float          en;
          const float2   z = z_of(r, l, c, n, en);
          float          s1, c1;
          sincospif(-2.0f * (turns * ((float)n - n_c)), &s1, &c1);
          w[k] = cmul(z, make_float2(c1, s1)), nn[k] = n;
          en2 = k ? en2 + en : en;
        }
      }
      epre += wave_sum(en2);
      // the ports of this comb: i = c, c + ncombs, ... (one comb: 0 .. N_ap - 1; a split: 0, 2 and 1, 3)
      float2 fit[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
      for (uint32_t pi = 0; pi < P; ++pi) {
        const uint32_t i = c + pi * d.ncombs, di = pi * (d.ncs_max / P); // n_cs,i - n_ref: the ports of a comb are n_cs_max / P apart
        float2         acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (lane + 64u * k < LQ) {
            const float2 t = cmul(w[k], srs_shift(di, nn[k], d.ncs_max, unit));
            acc.x += t.x, acc.y += t.y;
          }
        acc.x = wave_sum(acc.x) * inv_lq, acc.y = wave_sum(acc.y) * inv_lq;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float2 t = cmulc(acc, srs_shift(di, nn[k], d.ncs_max, unit));
          fit[k].x += t.x, fit[k].y += t.y;
        }
        if (lane == 0) {
          const float2 hh = cmul(acc, back);
          h_out[j.h_offset + ((size_t)g * R + r) * nap + i] = acc;
          sums[wave].hwb[r][i][0] += hh.x, sums[wave].hwb[r][i][1] += hh.y;
          sums[wave].rsrp[i] += acc.x * acc.x + acc.y * acc.y;
        }
      }
      float e2 = 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (lane + 64u * k < LQ) {
          const float ex = w[k].x - fit[k].x, ey = w[k].y - fit[k].y;
          e2 += ex * ex + ey * ey;
        }
      noise += wave_sum(e2);
    }
    if (lane == 0)
      sums[wave].noise += noise, sums[wave].epre += epre;
  }
  __syncthreads();

  // ---- the record
  if (tid == 0) {
    miphy_srs_result& res = results[blockIdx.x];
    auto              sum4 = [&](auto f) { return ((f(sums[0]) + f(sums[1])) + f(sums[2])) + f(sums[3]); };
    float             mean_rsrp = 0.f;
    for (uint32_t r = 0; r < 4; ++r)
      for (uint32_t i = 0; i < 4; ++i) {
        const bool used   = r < R && i < nap;
        res.h_wb[r][i][0] = used ? sum4([&](const srs_sums& s) { return s.hwb[r][i][0]; }) / (float)G : 0.f;
        res.h_wb[r][i][1] = used ? sum4([&](const srs_sums& s) { return s.hwb[r][i][1]; }) / (float)G : 0.f;
      }
    for (uint32_t i = 0; i < 4; ++i) {
      const float p  = i < nap ? sum4([&](const srs_sums& s) { return s.rsrp[i]; }) / (float)(R * G) : 0.f;
      res.rsrp_db[i] = i < nap ? to_db(p) : 0.f;
      mean_rsrp += p;
    }
    mean_rsrp /= (float)nap;
    const float noise_var = sum4([](const srs_sums& s) { return s.noise; }) / (float)(R * d.ncombs * (L * M - G * P));
    res.noise_var         = noise_var;
    res.epre_db           = to_db(sum4([](const srs_sums& s) { return s.epre; }) / (float)(R * d.ncombs * L * M));
    res.sinr_db           = to_db(mean_rsrp / noise_var);
    res.time_alignment_s  = (float)(-(phi / (double)(K * P)) / (6.283185307179586476925 * 15000.0 * (double)(1u << j.numerology)));
  }
}

// The rules of one job on the host: the code of the first rule it breaks, with its text in miphy_last_error().
int srs_check(const char* who, uint32_t i, const miphy_srs_job& j)
{
  const int rule = miphy_srs_rule(j);
  if (rule == SRS_RULE_UNSUPP) {
    miphy_set_error("%s: job %u: %s", who, i, SRS_RULE_TEXT[rule]);
    return MIPHY_EUNSUPP;
  }
  MIPHY_REQUIRE(rule == 0, "%s: job %u: %s", who, i, SRS_RULE_TEXT[rule]);
  return MIPHY_OK;
}

} // namespace

extern "C" int miphy_srs_info(const miphy_srs_job* job, miphy_srs_info_t* out)
{
  MIPHY_REQUIRE(job && out, "miphy_srs_info: null argument");
  if (const int rc = srs_check("miphy_srs_info", 0, *job))
    return rc;
  srs_derived d;
  miphy_srs_derive(*job, d);
  out->M = d.M, out->Q = d.Q, out->P = d.P, out->G = d.G, out->nof_combs = d.ncombs;
  for (int i = 0; i < 4; ++i)
    out->cyclic_shifts[i] = d.cs[i], out->comb_offsets[i] = d.off[i];
  out->nof_h       = d.G * job->nof_rx_ports * job->nof_tx_ports;
  out->max_delay_s = (float)(1.0 / (2.0 * 15000.0 * (double)(1u << job->numerology) * (double)job->comb_size * (double)d.P));
  return MIPHY_OK;
}

extern "C" int miphy_srs_pilots_batch(miphy_ctx* ctx, const miphy_srs_job* jobs, int jobs_on_device, uint32_t n, float* pilots, void* stream)
{
  static const char* const who = "miphy_srs_pilots_batch";
  MIPHY_REQUIRE(ctx && jobs && pilots, "%s: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 jobs per call", who);
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i)
      if (const int rc = srs_check(who, i, jobs[i]))
        return rc;
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_srs_job) * (size_t)n, s, &d_jobs)))
    return rc;
  hipLaunchKernelGGL(srs_pilots_kernel, dim3(n, 4), dim3(SRS_THREADS), 0, s, (const miphy_srs_job*)d_jobs, gt, (float2*)pilots);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_srs_estimate_batch(miphy_ctx* ctx, const miphy_srs_job* jobs, int jobs_on_device, uint32_t n, const float* grid, float* h_out,
                                        miphy_srs_result* results, void* stream)
{
  static const char* const who = "miphy_srs_estimate_batch";
  MIPHY_REQUIRE(ctx && jobs && grid && h_out && results, "%s: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 jobs per call", who);
  // Host jobs: every one is checked before anything is enqueued, and the LDS is sized for the longest sequences; device jobs: for the longest possible.
  size_t lds = 4 * (size_t)SRS_MAX_M * sizeof(float2);
  if (!jobs_on_device) {
    lds = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (const int rc = srs_check(who, i, jobs[i]))
        return rc;
      srs_derived d;
      miphy_srs_derive(jobs[i], d);
      lds = std::max(lds, (size_t)(jobs[i].hopping ? jobs[i].nof_symbols : 1) * d.M * sizeof(float2));
    }
  }
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_srs_job) * (size_t)n, s, &d_jobs)))
    return rc;
  hipLaunchKernelGGL(srs_estimate_kernel, dim3(n), dim3(SRS_THREADS), lds, s, (const miphy_srs_job*)d_jobs, gt, (const float2*)grid, (float2*)h_out, results);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
