// PUSCH with transform precoding (DFT-s-OFDM, TS 38.211 6.3.1.4), the blocks of its own: the de-precoder (miphy_transform_deprecode_batch) and the
// low-PAPR DM-RS (TS 38.211 5.2.2, 6.4.1.1.1.2: miphy_low_papr_sequence, miphy_dmrs_pusch_tp_pilots_batch). Beyond the 23.5 reference, which has no
// transform precoding; the contract is TS 38.211 itself, restated in numpy in tests/pusch_tp_ref.py. The fused demodulator is in pusch_demod.hip, the
// estimator entry point in chest.hip, the processor in pusch_proc.hip; the per-symbol function they share with this file is tp_device.h, the sequences
// and their hopping low_papr_device.h.
#include "tp_device.h"
#include "low_papr_device.h"
#include "miphy_ext.h"
#include <cmath>
#include <vector>

// ------------------------------------------------------------------------------------------------ twiddle tables of the 53 sizes
int miphy_tp_twiddles(miphy_ctx* ctx, const float* const** out)
{
  if (!ctx->ext->d_tp_twiddles) {
    std::vector<const float*> h(TP_MAX_PRB + 1, nullptr);
    for (unsigned nprb = 1; nprb <= (unsigned)TP_MAX_PRB; ++nprb)
      if (tp_nprb_ok(nprb))
        if (int rc = miphy_get_twiddles(ctx, 12 * nprb, &h[nprb]))
          return rc;
    const float** d = nullptr;
    if (int rc = miphy_keep_device_copy(ctx, h.data(), h.size(), &d))
      return rc;
    ctx->ext->d_tp_twiddles = d;
  }
  *out = ctx->ext->d_tp_twiddles;
  return MIPHY_OK;
}

namespace {

// ------------------------------------------------------------------------------------------------ de-precoder
// One workgroup per (row, job).
__global__ void __launch_bounds__(TP_THREADS) tp_deprecode_kernel(const miphy_transform_deprecode_job* __restrict__ jobs, const float* const* __restrict__ tws,
                                                                  const float2* __restrict__ eq_symbols, const float* __restrict__ eq_noise_vars,
                                                                  float2* __restrict__ out_symbols, float* __restrict__ out_noise_var)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float red[8];
  cplx*                               x = reinterpret_cast<cplx*>(smem);
  const miphy_transform_deprecode_job j = load_words(jobs + blockIdx.y);
  if (!tp_size_ok(j.M) || j.nof_symbols > 14 || blockIdx.x >= j.nof_symbols) // uniform
    return;
  const int     M = (int)j.M, tid = threadIdx.x, row = blockIdx.x;
  const float2* xs = eq_symbols + j.eq_symbols_offset + (size_t)row * M;
  const float*  vs = eq_noise_vars + j.eq_noise_vars_offset + (size_t)row * M;
  tp_var_acc    acc;
  for (int k = tid; k < M; k += TP_THREADS)
    tp_put(x, k, xs[k], vs[k], acc);
  const float v     = tp_deprecode_symbol(x, M, reinterpret_cast<const cplx*>(tws[M / 12]), acc, red, tid);
  const float scale = tp_scale(M);
  float2*     ys    = out_symbols + j.out_symbols_offset + (size_t)row * M;
  for (int n = tid; n < M; n += TP_THREADS)
    ys[n] = tp_symbol(x, n, scale);
  if (tid == 0)
    out_noise_var[j.out_noise_var_offset + row] = v;
}

} // namespace

extern "C" int miphy_transform_deprecode_batch(miphy_ctx* ctx, const miphy_transform_deprecode_job* jobs, int jobs_on_device, uint32_t n, const float* eq_symbols,
                                               const float* eq_noise_vars, float* out_symbols, float* out_noise_var, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && eq_symbols && eq_noise_vars && out_symbols && out_noise_var, "miphy_transform_deprecode_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "transform_deprecode: at most 65535 jobs per call");
  uint32_t max_M = TP_MAX_M, max_rows = 14; // device-resident jobs: the largest
  if (!jobs_on_device) {
    max_M = 12, max_rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (!tp_size_ok(jobs[i].M)) {
        miphy_set_error("transform_deprecode: job %u: size %u not supported (12 N, N = 2^a*3^b*5^c <= 270)", i, jobs[i].M);
        return MIPHY_EUNSUPP;
      }
      MIPHY_REQUIRE(jobs[i].nof_symbols <= 14, "transform_deprecode: job %u: %u symbols (at most 14)", i, jobs[i].nof_symbols);
      max_M    = std::max(max_M, jobs[i].M);
      max_rows = std::max(max_rows, jobs[i].nof_symbols);
    }
    if (max_rows == 0)
      return MIPHY_OK;
  }
  hipStream_t         s   = (hipStream_t)stream;
  const float* const* tws = nullptr;
  int                 rc  = miphy_tp_twiddles(ctx, &tws);
  if (rc)
    return rc;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_transform_deprecode_job) * (size_t)n, s, &d_jobs)))
    return rc;
  hipLaunchKernelGGL(tp_deprecode_kernel, dim3(max_rows, n), dim3(TP_THREADS), fft_lds_bytes(max_M), s, (const miphy_transform_deprecode_job*)d_jobs, tws,
                     (const float2*)eq_symbols, eq_noise_vars, (float2*)out_symbols, out_noise_var);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ------------------------------------------------------------------------------------------------ low-PAPR sequences
namespace {

// The rules of a transform-precoded DM-RS job (j = the record, b = its base): R(condition, message, arguments), evaluated in this order. nprb, first:
// the allocation (tp_contiguous ran). The host refuses with the message, the kernel skips.
#define TP_CHEST_RULES(R)                                                                                                                       \
  R(b.numerology <= 4, "invalid numerology")                                                                                                    \
  R(b.slot_in_frame < (10u << b.numerology), "slot %u outside the frame", b.slot_in_frame)                                                      \
  R(b.nof_tx_layers == 1, "transform precoding is on one layer")                                                                                \
  R(b.nof_rx_ports >= 1 && b.nof_rx_ports <= 4, "invalid number of rx ports %u", (unsigned)b.nof_rx_ports)                                      \
  R(b.grid_nof_prb >= 1 && b.grid_nof_prb <= 275, "invalid grid width")                                                                         \
  R(b.nof_symbols > 0 && b.first_symbol + b.nof_symbols <= 14, "invalid symbol range")                                                          \
  R(b.scaling > 0, "the DM-RS to data scaling factor should be a positive number")                                                              \
  R(tp_nof_dmrs(b) >= 1 && tp_nof_dmrs(b) <= 4, "%u DM-RS symbols (1..4 supported)", tp_nof_dmrs(b))                                            \
  R(b.hop_symbol == 0 && b.re_odd_mask == 0, "no intra-slot hopping, DM-RS port 0")                                                             \
  R(b.n_scid == 0 && b.scrambling_id < 1008, "n_ID^RS is 0..1007 and n_scid 0")                                                                 \
  R(j.hopping <= 2, "invalid hopping mode %u", (unsigned)j.hopping)                                                                             \
  R(contiguous, "the allocation is not contiguous")                                                                                             \
  R(tp_nprb_ok(nprb), "%u PRBs are not 2^a*3^b*5^c <= 270", nprb)

__host__ __device__ inline unsigned tp_nof_dmrs(const miphy_pusch_chest_job& b)
{
  unsigned nds = 0;
  for (unsigned l = b.first_symbol; l < (unsigned)b.first_symbol + b.nof_symbols && l < 14; ++l)
    nds += (b.symbols_mask >> l) & 1u;
  return nds;
}
__host__ __device__ inline bool tp_chest_job_ok(const miphy_pusch_chest_tp_job& j, unsigned& nprb)
{
  const miphy_pusch_chest_job& b = j.base;
  unsigned                     first;
  const bool                   contiguous = tp_contiguous(b.rb_mask, b.grid_nof_prb, first, nprb);
#define TP_RULE_HOLDS(cond, ...) &&(cond)
  return true TP_CHEST_RULES(TP_RULE_HOLDS) && nprb != 1 && nprb != 3 && nprb != 4;
#undef TP_RULE_HOLDS
}

constexpr int TP_MAX_DMRS = 4;

// One workgroup per (job, DM-RS symbol of the job). base_out (the estimator entry point): a copy of the base records for chest_kernel, the pilots of job i
// at i * stride + [DM-RS symbol][6 nprb] and that offset in the copy; a job that breaks a rule gets no receive port there, so the estimator's workgroups
// leave at once. Without base_out the pilots go to the job's pilots_offset.
__global__ void __launch_bounds__(TP_THREADS) tp_pilots_kernel(const miphy_pusch_chest_tp_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                               float2* __restrict__ pilots, miphy_pusch_chest_job* __restrict__ base_out,
                                                               uint32_t stride)
{
  __shared__ uint32_t                     uv[2];
  const miphy_pusch_chest_tp_job&          jm  = jobs[blockIdx.x];
  const int                                tid = threadIdx.x, d = blockIdx.y;
  unsigned                                 nprb = 0;
  const bool                               ok   = tp_chest_job_ok(jm, nprb); // uniform
  if (base_out && d == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&jm.base);
    uint32_t*       dst = reinterpret_cast<uint32_t*>(base_out + blockIdx.x);
    for (int i = tid; i < (int)(sizeof(miphy_pusch_chest_job) / 4); i += TP_THREADS)
      dst[i] = src[i];
    __syncthreads();
    if (tid == 0) {
      base_out[blockIdx.x].pilots_offset = (uint64_t)blockIdx.x * stride;
      if (!ok)
        base_out[blockIdx.x].nof_rx_ports = 0;
    }
  }
  if (!ok)
    return;
  const miphy_pusch_chest_job& b = jm.base;
  // the d-th DM-RS symbol of the allocation
  int l = -1, seen = 0;
  for (int s = b.first_symbol; s < b.first_symbol + b.nof_symbols; ++s)
    if ((b.symbols_mask >> s) & 1) {
      if (seen == d)
        l = s;
      ++seen;
    }
  if (l < 0) // uniform
    return;
  const unsigned len = 6 * nprb, n_id = b.scrambling_id;
  if (tid == 0)
    low_papr_hop(*gt, jm.hopping, n_id / 30u, n_id, b.slot_in_frame, (uint32_t)l, len, uv[0], uv[1]);
  __syncthreads();
  const unsigned u = uv[0], v = uv[1];
  float2*        out = pilots + (base_out ? (size_t)blockIdx.x * stride : (size_t)b.pilots_offset) + (size_t)d * len;
  const unsigned nzc = low_papr_prime_below(len), q = low_papr_zc_root(u, v, nzc);
  for (unsigned n = tid; n < len; n += TP_THREADS)
    out[n] = low_papr_element(u, q, nzc, len, n);
}

} // namespace

extern "C" int miphy_low_papr_sequence(uint32_t u, uint32_t v, uint32_t length, float* out)
{
  MIPHY_REQUIRE(out, "miphy_low_papr_sequence: null argument");
  if (length == 6 || length == 18 || length == 24) {
    miphy_set_error("miphy_low_papr_sequence: length %u needs TS 38.211 Tables 5.2.2.2-1, -3, -4, which the library does not hold", length);
    return MIPHY_EUNSUPP;
  }
  MIPHY_REQUIRE(low_papr_length_ok(length), "miphy_low_papr_sequence: invalid length %u", length);
  MIPHY_REQUIRE(u < 30 && v < 2, "miphy_low_papr_sequence: invalid sequence (u = %u, v = %u)", u, v);
  const unsigned nzc = low_papr_prime_below(length), q = low_papr_zc_root(u, v, nzc);
  for (unsigned n = 0; n < length; ++n) {
    const float2 r = low_papr_element_host(u, q, nzc, length, n);
    out[2 * n] = r.x, out[2 * n + 1] = r.y;
  }
  return MIPHY_OK;
}

// The host's rules on a batch of jobs: the first rule a job breaks, by message. max_nprb: the widest allocation.
int miphy_tp_chest_validate(const char* who, const miphy_pusch_chest_tp_job* jobs, uint32_t n, unsigned& max_nprb, unsigned& max_ports)
{
  max_nprb = 2, max_ports = 1;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pusch_chest_tp_job& j = jobs[i];
    const miphy_pusch_chest_job&    b = j.base;
    unsigned                        first, nprb;
    const bool                      contiguous = tp_contiguous(b.rb_mask, b.grid_nof_prb, first, nprb);
#define TP_RULE_REQUIRE(cond, msg, ...) MIPHY_REQUIRE(cond, "%s: job %u: " msg, who, i, ##__VA_ARGS__);
    TP_CHEST_RULES(TP_RULE_REQUIRE)
#undef TP_RULE_REQUIRE
    if (nprb == 1 || nprb == 3 || nprb == 4) {
      miphy_set_error("%s: job %u: the DM-RS of %u PRBs needs TS 38.211 Tables 5.2.2.2-1, -3, -4, which the library does not hold", who, i, nprb);
      return MIPHY_EUNSUPP;
    }
    max_nprb  = std::max(max_nprb, nprb);
    max_ports = std::max(max_ports, (unsigned)b.nof_rx_ports);
  }
  return MIPHY_OK;
}

int miphy_tp_pilots_launch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* d_jobs, uint32_t n, float* pilots, miphy_pusch_chest_job* base_out, uint32_t stride,
                           hipStream_t s)
{
  const gold_tables* gt = nullptr;
  if (const int rc = miphy_get_gold_tables(ctx, &gt))
    return rc;
  hipLaunchKernelGGL(tp_pilots_kernel, dim3(n, TP_MAX_DMRS), dim3(TP_THREADS), 0, s, d_jobs, gt, (float2*)pilots, base_out, stride);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_dmrs_pusch_tp_pilots_batch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* jobs, int jobs_on_device, uint32_t n, float* pilots, void* stream)
{
  const char* who = "miphy_dmrs_pusch_tp_pilots_batch";
  MIPHY_REQUIRE(ctx && jobs && pilots, "%s: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "%s: at most 65535 jobs per call", who);
  unsigned max_nprb, max_ports;
  int      rc;
  if (!jobs_on_device && (rc = miphy_tp_chest_validate(who, jobs, n, max_nprb, max_ports)))
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_tp_job) * (size_t)n, s, &d_jobs)))
    return rc;
  return miphy_tp_pilots_launch(ctx, (const miphy_pusch_chest_tp_job*)d_jobs, n, pilots, nullptr, 0, s);
}
