// PRACH detector and generator: srsran::prach_detector_simple_impl::detect (prach_detector_simple_impl.cpp:35-169) and
// srsran::prach_generator_impl::generate (prach_generator_impl.cpp:105-301) for a batch of occasions.
// One workgroup of 256 threads per (occasion, preamble index) runs the reference's per-preamble loop body:
//  - RSSI: the average power of the occasion's symbol, recomputed by every workgroup of the occasion in one fixed order (lane partial
//    sums over n = tid, tid + 256, ..., a butterfly over the wavefront, the four wavefronts in order), so that a record does not
//    depend on where its occasion sits in the batch. The 64 workgroups of an occasion read the same 6.7 KB, which L2 serves.
//  - preamble: y_u,v(n) = sqrt(L) exp(j pi k(n) / (2 L)) with the integer phase index
//    k(n) = 2 u f n (f n + 1) + 4 C_v n + off_u (mod 4 L), f = u^-1 mod L, off_u the phase of sum_m x_u(m) (tables/nr_prach_tables.h),
//    reduced in 32-bit integers before any floating-point step; the angle is rounded like the entries of the reference's
//    single-precision table (float pi * float k / float 2L). No table of 4 L exponentials: a thread evaluates at most four samples.
//  - correlation symbol * conj(preamble) into the padded LDS buffer of fft_device.h, lower half of the sequence in the last bins, upper
//    half in the first, guard bins zeroed; unnormalised inverse transform in LDS (fft_lds<true>);
//  - peak of |c|^2 as a (power, index) pair, the lowest index winning a tie; metric = peak / (rssi preamble_power L L) with the preamble
//    power summed like the RSSI; threshold 0.07; delay sign and window. One lane writes the record.
// What the detector derives before it looks at the signal (L, N_CS, cyclic prefix in samples, delay_n_maximum) is derived here from
// TS 38.211 Tables 6.3.3.1-1, -2, -5, -6 and -7 by one function (prach_info.h) that the host uses to validate and the kernel to run, so
// that jobs may live on the device. No per-call scratch; the launch only needs the twiddle tables the context keeps.
#include "fft_device.h"
#include "miphy_ext.h"
#include "prach_info.h"
#include "wave_device.h"
#define NR_PRACH_TABLE_ATTR __device__
#include "tables/nr_prach_tables.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int      PRACH_THREADS  = 256; // fft_lds needs N <= 16 threads: 3072 <= 4096; 1536 <= 8 threads runs the wide passes
constexpr uint32_t PRACH_MAX_IDFT = 3072;
constexpr float    PRACH_THRESHOLD = 0.07f;
constexpr float    PRACH_PI        = 3.14159265358979323846f;

struct prach_derived {
  uint32_t L, n_cs, delay_n_maximum, n_cs_limited;
};

__host__ __device__ inline bool prach_job_derive(const miphy_prach_job& j, prach_derived& d)
{
  uint32_t scs_hz = 0, cp_kappa = 0;
  if (!prach_preamble_info(j.format, j.ra_scs, j.zero_correlation_zone, j.restricted_set, d.L, scs_hz, cp_kappa, d.n_cs))
    return false;
  if (j.nof_preamble_indices > MIPHY_PRACH_MAX_PREAMBLES || j.start_preamble_index + j.nof_preamble_indices > MIPHY_PRACH_MAX_PREAMBLES)
    return false;
  if (j.idft_size != 1536 && j.idft_size != PRACH_MAX_IDFT)
    return false;
  // phy_time_unit::to_samples of the cyclic prefix at ra_scs * idft_size (it asserts a whole number of samples).
  const uint64_t num = (uint64_t)cp_kappa * scs_hz * j.idft_size, den = 15000ull * 2048ull;
  if (num % den)
    return false;
  d.delay_n_maximum = (uint32_t)(num / den);
  d.n_cs_limited    = 0;
  if (d.n_cs != 0) {
    const uint32_t by_ncs = (d.n_cs * j.idft_size) / d.L;
    if (d.delay_n_maximum > by_ncs)
      d.delay_n_maximum = by_ncs, d.n_cs_limited = 1;
  }
  return true;
}

// Physical root, its inverse and phase offset, and the cyclic shift of a preamble index (prach_generator_impl::generate).
struct prach_root {
  uint32_t a, f, off, cv; // a = u f mod 2L
};
__device__ __forceinline__ prach_root prach_root_of(uint32_t L, uint32_t n_cs, uint32_t root_sequence_index, uint32_t preamble_index)
{
  uint32_t logical = root_sequence_index + preamble_index, cv = 0;
  if (n_cs != 0) {
    const uint32_t per_root = L / n_cs;
    logical                 = root_sequence_index + preamble_index / per_root;
    cv                      = (preamble_index % per_root) * n_cs;
  }
  uint32_t u, f, off;
  if (L == 839) {
    u = NR_PRACH_ROOT_LONG[logical % 838u], f = NR_PRACH_INV_LONG[u], off = NR_PRACH_OFF_LONG[u];
  } else {
    u = NR_PRACH_ROOT_SHORT[logical % 138u], f = NR_PRACH_INV_SHORT[u], off = NR_PRACH_OFF_SHORT[u];
  }
  return {(u * f) % (2 * L), f, off, cv};
}

// x mod 2L with the two moduli as compile-time constants (a multiply and a shift instead of a division).
__device__ __forceinline__ uint32_t mod2L(uint32_t x, bool is_long)
{
  return is_long ? x % 1678u : x % 278u;
}

// y_u,v(n). Every intermediate stays below 2^32: the factors are below 2L <= 1678 or below 4 * 839 * 839.
__device__ __forceinline__ float2 prach_sample(const prach_root& r, uint32_t L, uint32_t n)
{
  const bool     is_long = L == 839;
  const uint32_t t       = mod2L(n * mod2L(r.f * n + 1u, is_long), is_long);
  const uint32_t x       = mod2L(r.a * t, is_long); // u f n (f n + 1) mod 2L
  uint32_t       k       = 2u * x + mod2L(2u * r.cv * n, is_long) * 2u + r.off;
  k                      = is_long ? k % 3356u : k % 556u;
  float s, c;
  sincosf((PRACH_PI * (float)k) / (float)(2 * L), &s, &c);
  const float amp = sqrtf((float)L);
  return make_float2(amp * c, amp * s);
}

__global__ void __launch_bounds__(PRACH_THREADS)
    prach_detect_kernel(const miphy_prach_job* __restrict__ jobs, uint32_t n, const float2* __restrict__ symbols, const cplx* __restrict__ tw1536,
                        const cplx* __restrict__ tw3072, uint32_t lds_idft, miphy_prach_result* __restrict__ results,
                        miphy_prach_preamble_result* __restrict__ preambles)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cplx*     x      = reinterpret_cast<cplx*>(smem);
  float*    red    = reinterpret_cast<float*>(smem + ((fft_lds_bytes(lds_idft) + 15) & ~(size_t)15)); // [0..3] rssi, [4..7] preamble power,
  uint32_t* red_i  = reinterpret_cast<uint32_t*>(red + 12);                                          // [8..11] peak power, red_i[0..3] index
  const int tid    = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t occ = blockIdx.x >> 6, slot = blockIdx.x & 63u;
  if (occ >= n)
    return;
  const miphy_prach_job j = jobs[occ];
  prach_derived         d;
  // Everything below is uniform over the workgroup: the early returns come before or between barriers for all threads alike.
  if (!prach_job_derive(j, d) || j.idft_size > lds_idft)
    return;
  if (slot >= j.nof_preamble_indices && slot != 0)
    return; // slot 0 stays to write the occasion's result, also for an empty range
  const bool     run   = slot < j.nof_preamble_indices;
  const uint32_t L     = d.L, N = j.idft_size, lower = L / 2, upper = L - lower;
  const float2*  sym   = symbols + j.symbol_offset;
  const prach_root r   = prach_root_of(L, d.n_cs, j.root_sequence_index, j.start_preamble_index + slot);

  if (run)
    for (uint32_t i = upper + tid; i < N - lower; i += PRACH_THREADS)
      x[fpad(i)] = cplx{0.f, 0.f};
  float p_sig = 0.f, p_pre = 0.f;
  for (uint32_t i = tid; i < L; i += PRACH_THREADS) {
    const float2 s = sym[i];
    p_sig += s.x * s.x + s.y * s.y;
    if (run) {
      const float2 y = prach_sample(r, L, i);
      p_pre += y.x * y.x + y.y * y.y;
      const uint32_t bin = i < lower ? N - lower + i : i - lower;
      x[fpad(bin)]       = cplx{s.x * y.x + s.y * y.y, s.y * y.x - s.x * y.y}; // s conj(y)
    }
  }
  p_sig = wave_sum(p_sig), p_pre = wave_sum(p_pre);
  if (lane == 0)
    red[wave] = p_sig, red[4 + wave] = p_pre;
  __syncthreads();
  const float rssi = (((red[0] + red[1]) + red[2]) + red[3]) / (float)L;
  const float ppow = (((red[4] + red[5]) + red[6]) + red[7]) / (float)L;
  if (slot == 0 && tid == 0) {
    miphy_prach_result& o = results[occ];
    o.rssi = rssi, o.delay_n_maximum = d.delay_n_maximum, o.n_cs = d.n_cs, o.n_cs_limited = d.n_cs_limited;
  }
  if (!run)
    return;
  miphy_prach_preamble_result& rec = preambles[(size_t)j.preamble_offset + slot];
  if (!isnormal(rssi)) { // "Early stop if the RSSI is zero": no preamble is tested
    if (tid == 0)
      rec.peak_index = 0, rec.delay_n = 0, rec.peak_power = 0.f, rec.metric = 0.f, rec.detected = 0;
    return;
  }

  fft_lds<true>(x, (int)N, N == 1536 ? tw1536 : tw3072, tid, PRACH_THREADS);

  float    best = -1.f;
  uint32_t bidx = 0;
  for (uint32_t i = tid; i < N; i += PRACH_THREADS) { // ascending: the first of equal powers stays
    const cplx  v = x[fpad(i)];
    const float p = v.x * v.x + v.y * v.y;
    if (p > best)
      best = p, bidx = i;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float    op = __shfl_xor(best, off);
    const uint32_t oi = __shfl_xor(bidx, off);
    if (op > best || (op == best && oi < bidx))
      best = op, bidx = oi;
  }
  if (lane == 0)
    red[8 + wave] = best, red_i[wave] = bidx;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PRACH_THREADS / 64; ++w)
      if (red[8 + w] > best || (red[8 + w] == best && red_i[w] < bidx))
        best = red[8 + w], bidx = red_i[w];
    const float metric = best / (((rssi * ppow) * (float)L) * (float)L);
    int32_t     delay  = (int32_t)bidx;
    uint32_t    mag    = bidx;
    if (bidx > N / 2)
      mag = N - bidx, delay = -(int32_t)mag;
    rec.peak_index = bidx, rec.delay_n = delay, rec.peak_power = best, rec.metric = metric;
    rec.detected   = (!(metric < PRACH_THRESHOLD) && mag < d.delay_n_maximum) ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(PRACH_THREADS)
    prach_generate_kernel(const miphy_prach_gen_job* __restrict__ jobs, uint32_t n, float2* __restrict__ out)
{
  if (blockIdx.x >= n)
    return;
  const miphy_prach_gen_job j = jobs[blockIdx.x];
  uint32_t                  L = 0, scs_hz = 0, cp_kappa = 0, n_cs = 0;
  if (!prach_preamble_info(j.format, 0, j.zero_correlation_zone, j.restricted_set, L, scs_hz, cp_kappa, n_cs) ||
      j.preamble_index >= MIPHY_PRACH_MAX_PREAMBLES)
    return;
  const prach_root r = prach_root_of(L, n_cs, j.root_sequence_index, j.preamble_index);
  for (uint32_t i = threadIdx.x; i < L; i += PRACH_THREADS)
    out[(size_t)j.out_offset + i] = prach_sample(r, L, i);
}

} // namespace

extern "C" int miphy_prach_detect_batch(miphy_ctx* ctx, const miphy_prach_job* jobs, int jobs_on_device, uint32_t n, const float* symbols,
                                        miphy_prach_result* results, miphy_prach_preamble_result* preambles, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && symbols && results && preambles, "miphy_prach_detect_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "prach_detect: at most 2^24 occasions per call");
  uint32_t lds_idft = PRACH_MAX_IDFT; // device jobs: room for the largest size
  if (!jobs_on_device) {
    lds_idft = 1536;
    for (uint32_t i = 0; i < n; ++i) {
      prach_derived d;
      MIPHY_REQUIRE(prach_job_derive(jobs[i], d),
                    "prach_detect: job %u: invalid occasion (format %u, ra_scs %u, zone %u, restricted set %u, preambles %u + %u, IDFT %u)", i,
                    jobs[i].format, jobs[i].ra_scs, jobs[i].zero_correlation_zone, jobs[i].restricted_set, jobs[i].start_preamble_index,
                    jobs[i].nof_preamble_indices, jobs[i].idft_size);
      lds_idft = std::max(lds_idft, jobs[i].idft_size);
    }
  }
  const float *tw1536 = nullptr, *tw3072 = nullptr;
  int          rc;
  if ((rc = miphy_get_twiddles(ctx, 1536, &tw1536)) || (rc = miphy_get_twiddles(ctx, PRACH_MAX_IDFT, &tw3072)))
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  rc                 = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_prach_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  const size_t lds = ((fft_lds_bytes(lds_idft) + 15) & ~(size_t)15) + 64;
  hipLaunchKernelGGL(prach_detect_kernel, dim3(n * MIPHY_PRACH_MAX_PREAMBLES), dim3(PRACH_THREADS), lds, s, (const miphy_prach_job*)d_jobs, n,
                     (const float2*)symbols, (const cplx*)tw1536, (const cplx*)tw3072, lds_idft, results, preambles);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_prach_generate_batch(miphy_ctx* ctx, const miphy_prach_gen_job* jobs, int jobs_on_device, uint32_t n, float* out, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && out, "miphy_prach_generate_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "prach_generate: at most 2^24 sequences per call");
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t L, scs_hz, cp_kappa, n_cs;
      MIPHY_REQUIRE(prach_preamble_info(jobs[i].format, 0, jobs[i].zero_correlation_zone, jobs[i].restricted_set, L, scs_hz, cp_kappa, n_cs) &&
                        jobs[i].preamble_index < MIPHY_PRACH_MAX_PREAMBLES,
                    "prach_generate: job %u: invalid sequence (format %u, zone %u, restricted set %u, preamble %u)", i, jobs[i].format,
                    jobs[i].zero_correlation_zone, jobs[i].restricted_set, jobs[i].preamble_index);
    }
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  int         rc     = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_prach_gen_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  hipLaunchKernelGGL(prach_generate_kernel, dim3(n), dim3(PRACH_THREADS), 0, s, (const miphy_prach_gen_job*)d_jobs, n, (float2*)out);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
