// PUCCH processor, format 0 (TS 38.211 6.3.2.3, TS 38.213 9.2.3), for a batch of PDUs that share one device grid. Beyond the 23.5 reference, whose
// format0_configuration cannot express a PDU; the contract is the standard, restated in numpy in tests/pucch_f0_tx.py (transmitter) and
// tests/pucch_f0_ref.py (float64 receiver, thresholds included). Format 0 has no DM-RS: the detector is a non-coherent decision between cyclic shifts
// against a noise level.
//
// The arithmetic. Per PDU, D = nof_ports nof_symbols pairs (port p, symbol l); symbol l is on starting_prb, except the second symbol of a two-symbol
// PDU with intra_slot_hopping, which is on second_hop_prb.
//  1. Per pair: y(n), n < 12, the REs of the PRB; w(n) = y(n) conj(r_u(n)), u = n_id mod 30, v = 0 (no group or sequence hopping, as formats 1, 3
//     and 4), r_u of TS 38.211 Table 5.2.2.2-2 (the row of shift 0 of tables/nr_low_papr_tables.h).
//  2. c_(p,l)[k] = (1 / 12) sum_n w(n) e^(-j 2 pi k n / 12) for all twelve k, n ascending.
//  3. Unhopped shift energies E[k'] = sum_(p,l) |c_(p,l)[(k' + n_cs(n_s, l_abs)) mod 12]|^2, n_cs of TS 38.211 6.3.2.2.2: the eight Gold bits of
//     c_init = n_id from 8 (14 n_s + l_abs), l_abs the symbol index in the slot -- what tests/pucch_tx.py::alpha_index and the format-1 kernel compute.
//     Summation order: ports outer, symbols inner (pair d = p nof_symbols + l ascending).
//  4. Hypotheses k' = (initial_cyclic_shift + m_cs) mod 12 with m_cs of TS 38.213 9.2.3 in this order: one HARQ-ACK bit: 0 -> 0, 1 -> 6; two bits
//     (b0, b1): (0,0) -> 0, (0,1) -> 3, (1,1) -> 6, (1,0) -> 9; SR alone: 0; SR with HARQ-ACK: the HARQ-only hypotheses (negative SR) followed by the
//     positive-SR ones, one bit: 0 -> 3, 1 -> 9, two bits: (0,0) -> 1, (0,1) -> 4, (1,1) -> 7, (1,0) -> 10. H = 1, 2, 4, 4 or 8.
//  5. S = the largest E[k'] over the hypotheses; on a tie the first in that order.
//  6. Noise: the occupied set is used_shifts_mask together with the PDU's own hypotheses, the free set its complement, F its size. noise_var > 0:
//     sigma^2 = noise_var. Otherwise (F >= 1 is a rule) sigma^2 = 12 sum_(k' free) E[k'] / (F D).
//  7. metric = 12 S / (D sigma^2): the energy of the best hypothesis over the noise energy of one shift.
//  8. Threshold: a total false-alarm probability of 1 % per PDU, union bound over the hypotheses (q = 0.01 / H); every degree of freedom is an integer,
//     so both forms are closed and solved by bisection in double on the host. Estimated noise: S / (S + N) is Beta(D, F D) on noise alone, x solves
//     sum_(j<D) C(n, j) x^j (1 - x)^(n - j) = q with n = D + F D - 1, the threshold is F x / (1 - x). Known noise: t solves
//     e^(-t) sum_(j<D) t^j / j! = q, the threshold is t / D. A job's own threshold > 0 replaces it.
//  9. Verdict: VALID when metric >= threshold, else INVALID. The payload always receives the best hypothesis, nof_harq_ack bytes then nof_sr bytes; SR
//     alone: 1 when VALID, else 0. detection_metric = metric / threshold; epre = sum_k' E[k'] / D, rsrp = S / D, sinr = (S / D) / sigma^2, each as
//     10 log10; time alignment 0: a delay and a cyclic shift cannot be told apart without DM-RS.
// The detector assumes a channel that is flat over the PRB; a timing offset leaks energy into the neighbouring shifts. That is the known limit of the
// format, not something this kernel resolves.
//
// Geometry: one wavefront per PDU, four PDUs per 256-lane workgroup, a slot's PDUs in one launch. Lane 12 q + k, q < 5, holds RE k of pair
// 5 pass + q and then shift k of it (D > 5: two passes); w(n) is exchanged inside the wavefront, the twiddles are twelve constants, the energies are
// unhopped and added over the pairs through wavefront shuffles. Both symbols' n_cs are sixteen consecutive Gold bits: one jump, the x1 register on lanes
// 0-31 and x2 on lanes 32-63 (gold_state_wave). No LDS, no barrier, no scratch.
#include "low_papr_device.h"
#include "miphy_ext.h"
#include "pucch_device.h"
#include <cmath>
#include <vector>

// The hypotheses of a job in table order: H of them, m_cs of hypothesis i in nibble i of the result.
__host__ __device__ static inline uint32_t miphy_pucch_f0_mcs(const miphy_pucch_f0_job& j, uint32_t& H)
{
  if (j.nof_harq_ack == 0) {
    H = 1;
    return 0x0u;
  }
  if (j.nof_harq_ack == 1) {
    H = j.nof_sr ? 4 : 2;
    return 0x9360u;
  }
  H = j.nof_sr ? 8 : 4;
  return 0xa7419630u;
}
// The PDU's own hypotheses as a mask of unhopped shifts.
__host__ __device__ static inline uint32_t miphy_pucch_f0_own_mask(const miphy_pucch_f0_job& j)
{
  uint32_t       H, own = 0;
  const uint32_t mcs = miphy_pucch_f0_mcs(j, H);
  for (uint32_t i = 0; i < H; ++i)
    own |= 1u << ((j.initial_cyclic_shift + ((mcs >> (4 * i)) & 0xfu)) % 12u);
  return own;
}
// The rules of one job, for the host and for the kernel (device jobs the host could not check): 0, or the number of the first rule it breaks
// (F0_RULE_TEXT).
__host__ __device__ static inline int miphy_pucch_f0_rule(const miphy_pucch_f0_job& j)
{
  if (j.format != 0)
    return 1;
  if (j.numerology > 4 || j.slot >= (10u << j.numerology))
    return 2;
  if (j.nof_ports < 1 || j.nof_ports > 4)
    return 3;
  if (j.nof_symbols < 1 || j.nof_symbols > 2 || j.start_symbol > 13 || j.start_symbol + j.nof_symbols > 14)
    return 4;
  if (j.intra_slot_hopping > 1 || (j.intra_slot_hopping && j.nof_symbols != 2))
    return 5;
  if (j.grid_nprb < 1 || j.grid_nprb > 275 || (uint32_t)j.bwp_start_rb + j.bwp_size_rb > j.grid_nprb)
    return 6;
  if (j.starting_prb >= j.bwp_size_rb || (j.intra_slot_hopping && j.second_hop_prb >= j.bwp_size_rb))
    return 7;
  if (j.initial_cyclic_shift > 11)
    return 8;
  if (j.nof_harq_ack > 2 || j.nof_sr > 1)
    return 9;
  if (j.nof_harq_ack == 0 && j.nof_sr == 0)
    return 10;
  if (j.used_shifts_mask > 0xfffu)
    return 11;
  if (j.n_id > 1023)
    return 12;
  if (!(j.threshold >= 0.f && j.threshold <= 3.402823466e+38f) || !(j.noise_var >= 0.f && j.noise_var <= 3.402823466e+38f))
    return 13;
  if (!(j.noise_var > 0.f) && ((j.used_shifts_mask | miphy_pucch_f0_own_mask(j)) & 0xfffu) == 0xfffu)
    return 14;
  return 0;
}

namespace {

const char* const F0_RULE_TEXT[15] = {"",
                                      "the format is not 0",
                                      "the slot lies outside the frame of the numerology (0..4)",
                                      "invalid number of receive ports (1..4)",
                                      "invalid symbol range (1..2 symbols within the slot)",
                                      "intra_slot_hopping is 0 or 1, and 1 only with two symbols",
                                      "the BWP leaves the grid (1..275 PRBs)",
                                      "the allocation leaves the BWP",
                                      "initial_cyclic_shift is 0..11",
                                      "nof_harq_ack is 0..2 and nof_sr 0..1",
                                      "no UCI bits (nof_harq_ack and nof_sr are both 0)",
                                      "used_shifts_mask has bits above the twelve shifts",
                                      "n_id is 0..1023",
                                      "threshold and noise_var are finite and not negative",
                                      "no free cyclic shift to estimate the noise from"};

constexpr int F0_PDUS_PER_WG = 4;

// e^(-j 2 pi m / 12)
__constant__ float F0_TW[12][2] = {{1.0f, 0.0f},
                                   {0.866025403784438647f, -0.5f},
                                   {0.5f, -0.866025403784438647f},
                                   {0.0f, -1.0f},
                                   {-0.5f, -0.866025403784438647f},
                                   {-0.866025403784438647f, -0.5f},
                                   {-1.0f, 0.0f},
                                   {-0.866025403784438647f, 0.5f},
                                   {-0.5f, 0.866025403784438647f},
                                   {0.0f, 1.0f},
                                   {0.5f, 0.866025403784438647f},
                                   {0.866025403784438647f, 0.5f}};

__global__ void __launch_bounds__(64 * F0_PDUS_PER_WG) pucch_f0_kernel(const miphy_pucch_f0_job* __restrict__ jobs, uint32_t n, const gold_tables* __restrict__ gt,
                                                                       const float2* __restrict__ grid, uint8_t* __restrict__ payload,
                                                                       miphy_pucch_result* __restrict__ results, float* __restrict__ energy_out)
{
#pragma clang fp contract(off)
  const int      lane = threadIdx.x & 63;
  const uint32_t pdu  = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * F0_PDUS_PER_WG + (threadIdx.x >> 6)));
  if (pdu >= n)
    return;
  const miphy_pucch_f0_job j = load_words(jobs + pdu);
  // Device jobs the host could not check, or without a threshold (the default is host arithmetic): nothing is written.
  if (miphy_pucch_f0_rule(j) != 0 || !(j.threshold > 0.f))
    return;
  const int     nsym = j.nof_symbols, D = j.nof_ports * nsym, s = j.start_symbol;
  const int     nsc  = 12 * (int)j.grid_nprb;
  const float2* g    = grid + j.grid_offset;
  const int     prb0 = j.bwp_start_rb + j.starting_prb, prb1 = j.bwp_start_rb + (j.intra_slot_hopping ? j.second_hop_prb : j.starting_prb);

  // n_cs of the first symbol in bits 0..7 and of the second in bits 8..15: c(8 (14 n_s + l) ...) of c_init = n_id, the rule of pucch_alpha
  // (pucch_device.h) for both symbols in one wavefront jump.
  uint32_t ncs;
  {
    const uint32_t st = gold_state_wave(*gt, lane >= 32, j.n_id, 8u * (14u * j.slot + (uint32_t)s), lane & 31);
    ncs               = (uint32_t)__shfl((int)st, 0) ^ (uint32_t)__shfl((int)st, 32);
  }

  const int    q = lane / 12, k = lane - 12 * q; // lanes 60..63 (q = 5) hold nothing
  const int    base = q < 5 ? 12 * q : 0;
  const int    u = j.n_id % 30;
  const float2 r = low_papr12(u, k);
  float        E = 0.f; // lane k' < 12: E[k']
  for (int d0 = 0; d0 < D; d0 += 5) {
    const int    d = d0 + q, p = d / nsym, l = d - p * nsym;
    const bool   mine = q < 5 && d < D;
    const float2 y = mine ? g[((size_t)p * 14 + s + l) * nsc + 12 * (l ? prb1 : prb0) + k] : make_float2(0.f, 0.f);
    const float2 w = cmulc(y, r);
    float2       c = make_float2(0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const float2 wi = make_float2(__shfl(w.x, base + i), __shfl(w.y, base + i));
      const int    m  = (k * i) % 12;
      const float2 t  = cmul(wi, make_float2(F0_TW[m][0], F0_TW[m][1]));
      c.x += t.x, c.y += t.y;
    }
    c.x /= 12.0f, c.y /= 12.0f;
    const float e = c.x * c.x + c.y * c.y;
    // this lane takes the unhopped shift k of its pair, then lanes 0..11 add the pairs in order
    const float eu = __shfl(e, base + (int)((k + ((ncs >> (8 * l)) & 0xffu)) % 12u));
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const float v = __shfl(eu, 12 * qq + (lane < 12 ? lane : 0));
      if (d0 + qq < D) // uniform
        E += v;
    }
  }

  // The decision, on lanes 0..11 through wavefront reductions.
  uint32_t       H;
  const uint32_t mcs = miphy_pucch_f0_mcs(j, H);
  uint32_t       own = 0;
  uint64_t       key = 0; // (E bits, ~hypothesis index): the maximum is the first of the largest
  for (uint32_t i = 0; i < H; ++i) {
    const uint32_t sh = (j.initial_cyclic_shift + ((mcs >> (4 * i)) & 0xfu)) % 12u;
    own |= 1u << sh;
    if ((uint32_t)lane == sh)
      key = ((uint64_t)__float_as_uint(E) << 32) | (uint32_t)(0xffffffffu - i);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    key = max(key, (uint64_t)__shfl_xor((long long)key, off));
  const float    S         = __uint_as_float((uint32_t)(key >> 32));
  const uint32_t best      = 0xffffffffu - (uint32_t)key;
  const uint32_t free_mask = ~(own | j.used_shifts_mask) & 0xfffu;
  const int      F         = __popc(free_mask);
  const float    sum_all   = wave_sum(lane < 12 ? E : 0.f);
  const float    sum_free  = wave_sum(lane < 12 && ((free_mask >> lane) & 1u) ? E : 0.f);
  const float    fD        = (float)D;
  const float    sigma2    = j.noise_var > 0.f ? j.noise_var : (12.0f * sum_free) / ((float)F * fD);
  const float    metric    = (12.0f * S) / (fD * sigma2);
  const bool     valid     = metric >= j.threshold;

  if (energy_out && lane < 12)
    energy_out[j.energy_offset + lane] = E;
  if (lane == 0) {
    uint8_t*       pay = payload + j.payload_offset;
    const uint32_t A = j.nof_harq_ack, hb = best & (A == 2 ? 3u : 1u);
    if (A == 1)
      pay[0] = (uint8_t)hb;
    if (A == 2)
      pay[0] = (uint8_t)(hb >> 1), pay[1] = (uint8_t)(hb == 1 || hb == 2);
    if (j.nof_sr)
      pay[A] = (uint8_t)(A ? (best >> A) & 1u : (valid ? 1u : 0u));
    miphy_pucch_result& res = results[pdu];
    res.status             = valid ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
    res.detection_metric   = metric / j.threshold;
    res.epre_db            = to_db(sum_all / fD);
    res.rsrp_db            = to_db(S / fD);
    res.sinr_db            = to_db((S / fD) / sigma2);
    res.time_alignment_s   = 0.f;
  }
}

// The default thresholds (step 8) for every D = 1..8, F = 0..11 and H = 1, 2, 4, 8, solved once.
struct f0_thresholds {
  double t[2][8][12][4]; // [known noise][D - 1][F][log2 H]
  static double bisect(double lo, double hi, double q, double (*tail)(int, int, double), int D, int n)
  {
    for (int i = 0; i < 100; ++i) { // the tail falls from 1 to 0
      const double mid = 0.5 * (lo + hi);
      if (tail(D, n, mid) > q)
        lo = mid;
      else
        hi = mid;
    }
    return 0.5 * (lo + hi);
  }
  static double tail_beta(int D, int n, double x) // sum_(j<D) C(n, j) x^j (1 - x)^(n - j)
  {
    double term = std::pow(1.0 - x, n), sum = 0.0;
    for (int j = 0; j < D; ++j) {
      sum += term;
      term *= (double)(n - j) / (double)(j + 1) * (x / (1.0 - x));
    }
    return sum;
  }
  static double tail_gamma(int D, int, double t) // e^(-t) sum_(j<D) t^j / j!
  {
    double term = std::exp(-t), sum = 0.0;
    for (int j = 0; j < D; ++j) {
      sum += term;
      term *= t / (double)(j + 1);
    }
    return sum;
  }
  f0_thresholds()
  {
    for (int D = 1; D <= 8; ++D)
      for (int F = 0; F < 12; ++F)
        for (int h = 0; h < 4; ++h) {
          const double q = 0.01 / (double)(1 << h);
          double       x = 0.0;
          if (F >= 1)
            x = bisect(0.0, 1.0, q, tail_beta, D, D + F * D - 1);
          t[0][D - 1][F][h] = F >= 1 ? (double)F * x / (1.0 - x) : 0.0;
          t[1][D - 1][F][h] = bisect(0.0, 200.0, q, tail_gamma, D, 0) / (double)D;
        }
  }
};

struct f0_derived {
  uint32_t H, mcs, D, free_mask, F;
  float    threshold;
};

// The rules of one job on the host: MIPHY_EINVAL with the first rule it breaks in miphy_last_error(); what follows from an accepted job.
int f0_check(const char* who, uint32_t i, const miphy_pucch_f0_job& j, f0_derived& d)
{
  const int rule = miphy_pucch_f0_rule(j);
  MIPHY_REQUIRE(rule == 0, "%s: job %u: %s", who, i, F0_RULE_TEXT[rule]);
  static const f0_thresholds T;
  d.mcs       = miphy_pucch_f0_mcs(j, d.H);
  d.D         = (uint32_t)j.nof_ports * j.nof_symbols;
  d.free_mask = ~(miphy_pucch_f0_own_mask(j) | j.used_shifts_mask) & 0xfffu;
  d.F         = (uint32_t)__builtin_popcount(d.free_mask);
  const int h = d.H == 1 ? 0 : (d.H == 2 ? 1 : (d.H == 4 ? 2 : 3));
  d.threshold = j.threshold > 0.f ? j.threshold : (float)T.t[j.noise_var > 0.f][d.D - 1][d.F][h];
  return MIPHY_OK;
}

} // namespace

extern "C" int miphy_pucch_f0_info(const miphy_pucch_f0_job* job, miphy_pucch_f0_info_t* out)
{
  MIPHY_REQUIRE(job && out, "miphy_pucch_f0_info: null argument");
  f0_derived d;
  if (const int rc = f0_check("miphy_pucch_f0_info", 0, *job, d))
    return rc;
  out->nof_hypotheses = d.H;
  for (uint32_t i = 0; i < 8; ++i)
    out->shifts[i] = i < d.H ? (uint8_t)((job->initial_cyclic_shift + ((d.mcs >> (4 * i)) & 0xfu)) % 12u) : 0;
  out->D = d.D, out->free_mask = d.free_mask, out->F = d.F, out->threshold = d.threshold;
  return MIPHY_OK;
}

extern "C" int miphy_pucch_process_f0_batch(miphy_ctx* ctx, const miphy_pucch_f0_job* jobs, int jobs_on_device, uint32_t n, const float* grid, uint8_t* payload,
                                            miphy_pucch_result* results, float* energy_out, void* stream)
{
  static const char* const who = "miphy_pucch_process_f0_batch";
  MIPHY_REQUIRE(ctx && jobs && grid && payload && results, "%s: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 PDUs per call", who);
  // Host jobs: every one is checked before anything is enqueued, and the staged copy carries the thresholds.
  std::vector<miphy_pucch_f0_job> own;
  if (!jobs_on_device) {
    own.assign(jobs, jobs + n);
    for (uint32_t i = 0; i < n; ++i) {
      f0_derived d;
      if (const int rc = f0_check(who, i, own[i], d))
        return rc;
      own[i].threshold = d.threshold;
    }
    jobs = own.data();
  }
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pucch_f0_job) * (size_t)n, s, &d_jobs)))
    return rc;
  hipLaunchKernelGGL(pucch_f0_kernel, dim3((n + F0_PDUS_PER_WG - 1) / F0_PDUS_PER_WG), dim3(64 * F0_PDUS_PER_WG), 0, s, (const miphy_pucch_f0_job*)d_jobs, n, gt,
                     (const float2*)grid, payload, results, energy_out);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
