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
#include "uci_device.h"
#include "uci_polar_info.h"

namespace {

constexpr int UCI_WAVES = 4; // fields per workgroup

__global__ void __launch_bounds__(64 * UCI_WAVES)
uci_short_block_kernel(const miphy_uci_field_job* __restrict__ jobs, uint32_t n, const int8_t* __restrict__ llr, uint8_t* __restrict__ payload,
                       uint8_t* __restrict__ status)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f    = blockIdx.x * UCI_WAVES + (threadIdx.x >> 6);
  if (f >= n)
    return;
  const miphy_uci_field_job j = jobs[f];
  if (!miphy_uci_job_ok(j.nof_bits, j.mod, j.nof_llr)) // device jobs the host could not check: the field is left untouched
    return;
  uci_short_block_field(j.nof_bits, j.mod, j.nof_llr, llr + j.llr_offset, payload + j.payload_offset, status + f, lane);
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

// The field jobs of PUSCH PDUs whose fields may be polar coded: 1..11 bits as above, 12..1706 bits framed by uci_polar_info.h for
// miphy_uci_polar_decode_batch (uci_polar.hip); one payload area in (PDU, field) order.
extern "C" int miphy_pusch_uci_jobs(const miphy_pusch_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, miphy_uci_field_job* short_jobs, uint32_t* short_field,
                                    uint32_t* nof_short, miphy_uci_polar_job* polar_jobs, uint32_t* polar_field, uint32_t* nof_polar)
{
  MIPHY_REQUIRE(pdus && uci && short_jobs && nof_short && polar_jobs && nof_polar, "miphy_pusch_uci_jobs: null argument");
  uint32_t ns = 0, np = 0;
  uint64_t pos = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pusch_uci& u = uci[i];
    const uint32_t         O[3] = {u.nof_harq_ack_bits, u.nof_csi_part1_bits, u.nof_csi_part2_bits};
    const uint32_t         G[3] = {u.nof_enc_harq_ack_bits, u.nof_enc_csi_part1_bits, u.nof_enc_csi_part2_bits};
    const uint64_t         off[3] = {u.harq_ack_offset, u.csi_part1_offset, u.csi_part2_offset};
    for (uint32_t k = 0; k < 3; ++k) {
      if (O[k] == 0)
        continue;
      if (O[k] <= 11) {
        MIPHY_REQUIRE(miphy_uci_job_ok(O[k], pdus[i].mod, G[k]), "pusch_uci_jobs: PDU %u field %u: invalid field (%u bits, %u bits per symbol, %u soft bits)", i,
                      k, O[k], pdus[i].mod, G[k]);
        miphy_uci_field_job& j = short_jobs[ns];
        j                      = {};
        j.nof_bits = static_cast<uint8_t>(O[k]), j.mod = pdus[i].mod, j.nof_llr = G[k], j.llr_offset = off[k], j.payload_offset = pos;
        if (short_field)
          short_field[ns] = 3 * i + k;
        ++ns;
      } else {
        uci_polar_framing f;
        int               rc = uci_polar_frame_or_error("pusch_uci_jobs", 3 * i + k, O[k], G[k], f);
        if (rc)
          return rc;
        miphy_uci_polar_job& j = polar_jobs[np];
        j                      = {};
        j.nof_bits = static_cast<uint16_t>(O[k]), j.nof_llr = G[k], j.llr_offset = off[k], j.payload_offset = pos;
        if (polar_field)
          polar_field[np] = 3 * i + k;
        ++np;
      }
      pos += O[k];
    }
  }
  *nof_short = ns, *nof_polar = np;
  return MIPHY_OK;
}
