// UCI short-block detector: srsran::short_block_detector::detect (lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:58-199),
// the whole UCI decoder of the reference for the 1..11-bit fields it accepts (uci_decoder_impl.cpp:41-50). Restated from TS 38.212
// 5.3.3 (the (32, K) block code and its 1- / 2-bit repetition forms) and 5.4.3 (rate matching e_k = d_{k mod N}), with the
// reference's saturating LLR arithmetic and its GLRT verdict.
//
// One wavefront per field, four fields per workgroup:
//  - rate dematch: lane j < L folds positions j, j + L, j + 2L, ... of the field strictly in input order with the saturating LLR sum
//    (not associative: no tree reduction);
//  - 3..11 bits: the 32 dematched values become wave-uniform (readlane); lane l scores the codewords of the even messages
//    idx = l + 64 r (r = 0..15, idx < 2^(K-1)); a correlation is sum(x) - 2 * (sum of x over the codeword's one bits), the codeword
//    mask comes from the linearity of the code (XOR of basis columns, no table); (|corr|, -idx, sign) is packed into one key and the
//    wave's maximum picks the largest |corr| with the lowest index on a tie, as the reference's first-maximum scan does;
//  - 1 and 2 bits: lane 0 finishes from the dematched values.
// Arithmetic of the verdict: every quantity before the final division is an integer below 2^53 (|corr| <= 32 * 127, the squared norm
// <= 32 * 127^2, their products < 2^30), so each step in FP64 is exact whether or not the compiler contracts it into an FMA and the
// metric is the one correctly rounded quotient of the reference; 0 / 0 (all-zero input) is NaN, which fails the strict > threshold
// comparison, as in the reference.
#include "miphy_internal.h"

// The reference's preconditions (validate_spans, short_block_detector_impl.cpp:58-83) plus the modulation orders it knows.
__host__ __device__ static inline bool miphy_uci_job_ok(uint32_t K, uint32_t Qm, uint32_t E)
{
  if (K < 1 || K > 11 || !(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8) || E > (1u << 31))
    return false;
  return K > 2 ? E > K : E >= (K == 1 ? Qm : 3 * Qm);
}

namespace {

constexpr int UCI_WAVES = 4; // fields per workgroup

// TS 38.212 Table 5.3.3.3-1, row i = output bit i; the leftmost binary digit is M_{i,0}, the rightmost M_{i,10}.
constexpr uint16_t TS_BASIS_ROWS[32] = {
    0b11000000001, 0b11100000011, 0b10010010111, 0b10110000101, 0b11110001001, 0b11001011101, 0b10101010111, 0b10011001101,
    0b11011001011, 0b10111010011, 0b10100111011, 0b11100110101, 0b10010101111, 0b11010101011, 0b10001101001, 0b11001111011,
    0b11101110010, 0b10011100100, 0b11011111000, 0b10000110000, 0b10100010001, 0b11010000011, 0b10001001101, 0b11101000111,
    0b11111011110, 0b11000111001, 0b10110100110, 0b11110101110, 0b10101110100, 0b10111111100, 0b11111111111, 0b10000000000};

// Basis sequence n as a 32-bit mask (bit i = M_{i,n}).
__host__ __device__ constexpr uint32_t basis_column(int n)
{
  uint32_t m = 0;
  for (int i = 0; i < 32; ++i)
    m |= static_cast<uint32_t>((TS_BASIS_ROWS[i] >> (10 - n)) & 1u) << i;
  return m;
}

// Detection thresholds of the GLRT per message length K = 1..11 (short_block_detector_impl.cpp:196-199).
__device__ __forceinline__ double uci_threshold(uint32_t K)
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
__device__ __forceinline__ int llr_add(int a, int b)
{
  if (a == -b)
    return 0;
  if (a == 127 || a == -127)
    return a;
  if (b == 127 || b == -127)
    return b;
  return min(max(a + b, -120), 120);
}

__global__ void __launch_bounds__(64 * UCI_WAVES)
uci_short_block_kernel(const miphy_uci_field_job* __restrict__ jobs, uint32_t n, const int8_t* __restrict__ llr, uint8_t* __restrict__ payload,
                       uint8_t* __restrict__ status)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f    = blockIdx.x * UCI_WAVES + (threadIdx.x >> 6);
  if (f >= n)
    return;
  const miphy_uci_field_job j = jobs[f];
  const uint32_t            K = j.nof_bits, Qm = j.mod, E = j.nof_llr;
  if (!miphy_uci_job_ok(K, Qm, E)) // device jobs the host could not check: the field is left untouched
    return;
  const uint32_t L = K == 1 ? Qm : (K == 2 ? 3 * Qm : 32);

  // Rate dematch: one accumulator per lane, its positions in input order.
  int acc = 0;
  if (lane < L) {
    const int8_t* __restrict__ p = llr + j.llr_offset;
#pragma unroll 8
    for (uint32_t i = lane; i < E; i += L)
      acc = llr_add(acc, p[i]);
  }
  uint8_t* out = payload + j.payload_offset;

  if (K == 1) { // bit = tmp[0] > 0 ? 0 : 1, metric 1 > threshold 0: always valid
    if (lane == 0) {
      out[0]    = acc > 0 ? 0 : 1;
      status[f] = MIPHY_UCI_STATUS_VALID;
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
      status[f] = metric > 0.0 ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
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
    status[f]           = metric > uci_threshold(K) ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
  }
}

} // namespace

extern "C" int miphy_uci_decode_batch(miphy_ctx* ctx, const miphy_uci_field_job* jobs, int jobs_on_device, uint32_t n, const int8_t* llr, uint8_t* payload,
                                      uint8_t* status, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && llr && payload && status, "miphy_uci_decode_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 28), "uci_decode: at most 2^28 fields per call");
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i)
      MIPHY_REQUIRE(miphy_uci_job_ok(jobs[i].nof_bits, jobs[i].mod, jobs[i].nof_llr),
                    "uci_decode: job %u: invalid field (%u bits, %u bits per symbol, %u soft bits)", i, jobs[i].nof_bits, jobs[i].mod, jobs[i].nof_llr);
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  int         rc     = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_uci_field_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  hipLaunchKernelGGL(uci_short_block_kernel, dim3((n + UCI_WAVES - 1) / UCI_WAVES), dim3(64 * UCI_WAVES), 0, s, (const miphy_uci_field_job*)d_jobs, n, llr,
                     payload, status);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_pusch_uci_field_jobs(const miphy_pusch_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, miphy_uci_field_job* jobs,
                                          uint32_t* job_field, uint32_t* nof_jobs)
{
  MIPHY_REQUIRE(pdus && uci && jobs && nof_jobs, "miphy_pusch_uci_field_jobs: null argument");
  uint32_t cnt = 0;
  uint64_t pos = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pusch_uci& u = uci[i];
    const uint32_t         O[3] = {u.nof_harq_ack_bits, u.nof_csi_part1_bits, u.nof_csi_part2_bits};
    const uint32_t         G[3] = {u.nof_enc_harq_ack_bits, u.nof_enc_csi_part1_bits, u.nof_enc_csi_part2_bits};
    const uint64_t         off[3] = {u.harq_ack_offset, u.csi_part1_offset, u.csi_part2_offset};
    for (uint32_t k = 0; k < 3; ++k) {
      if (O[k] == 0)
        continue;
      MIPHY_REQUIRE(O[k] <= 11, "pusch_uci_field_jobs: PDU %u field %u: %u bits (the short-block detector takes 1 to 11)", i, k, O[k]);
      MIPHY_REQUIRE(miphy_uci_job_ok(O[k], pdus[i].mod, G[k]), "pusch_uci_field_jobs: PDU %u field %u: invalid field (%u bits, %u bits per symbol, %u soft bits)",
                    i, k, O[k], pdus[i].mod, G[k]);
      miphy_uci_field_job& j = jobs[cnt];
      j                      = {};
      j.nof_bits = static_cast<uint8_t>(O[k]), j.mod = pdus[i].mod, j.nof_llr = G[k], j.llr_offset = off[k], j.payload_offset = pos;
      if (job_field)
        job_field[cnt] = 3 * i + k;
      pos += O[k];
      ++cnt;
    }
  }
  *nof_jobs = cnt;
  return MIPHY_OK;
}
