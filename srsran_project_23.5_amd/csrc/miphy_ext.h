// Host-side caches hanging off a context: FFT twiddle tables, OFDM symbol plans, polar tables.
#pragma once
#include "miphy_internal.h"
#include <cstddef>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

struct ofdm_plan_dev {
  int   N, rg, window_offset, nsymb_sf;
  int   cp_len[56];   // per symbol of the subframe
  int   sym_off[56];  // offset of the symbol start (CP included) inside its slot
  float coef_re[56];  // phase compensation * scale
  float coef_im[56];
};

// Device-resident description of one polar code (polar_code_impl::set) plus the pruned SSC schedule.
struct polar_plan {
  uint32_t K, E, n, N, nPC;
  // device tables
  uint16_t* d_info_pos;  // K + nPC positions of the K-set, ascending
  uint8_t*  d_is_pc;     // K + nPC flags: 1 = parity-check position
  uint16_t* d_tx_src;    // E entries: rate-matched bit o = encoded bit tx_src[o]
  int32_t*  d_rx_first;  // N entries: first rate-matched index feeding codeword position q (-1: punctured -> 0, -2: shortened -> +inf)
  uint16_t* d_rx_fidx;   // E entries: index in the received sequence of bit-selection index k (identity unless ibil)
  uint32_t* d_sched;     // SSC schedule: op | stage << 4 | pos << 8
  uint8_t*  d_pi_il;     // K entries: CRC interleaver (pdcch)
  uint32_t  sched_len;
};

// One constructed code of the polar-coded UCI decoder (uci_polar.hip) on the HOST: header and tables as one relocatable block that is
// copied into every call that uses the code. A bounded cache, least recently used entry evicted; nothing of it lives on the device.
struct uci_polar_host_code {
  uint32_t                                     key  = 0; // K_r << 16 | E_r
  uint64_t                                     used = 0;
  std::shared_ptr<const std::vector<uint8_t>>  blob;
};
enum { UCI_POLAR_HOST_CACHE_ENTRIES = 128 };

// Soft-bit address tables of the LDPC decoder (miphy_ldpc_address_tables) of one (base graph, layers): device pointers by Z / 16.
struct ldpc_adr_tables {
  const void* h_ptr[MIPHY_MAX_Z / 16 + 1] = {}; // host copy of the device array d_ptr
  void**      d_ptr                       = nullptr;
};

struct miphy_ctx_ext {
  std::map<std::pair<int, int>, ldpc_adr_tables> ldpc_adr; // (base graph - 1, layers) -> tables; freed with to_free
  std::vector<uci_polar_host_code> uci_polar_codes;
  uint64_t                         uci_polar_clock = 0;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, polar_plan> polar_plans;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint8_t*>   polar_kset; // per-position K-set flags (SCL)
  std::map<uint32_t, float*>                                    twiddles; // N -> device exp(-2 pi i j / N), j < N
  std::map<std::pair<uint32_t, uint32_t>, float*>               ramps;    // (N, offset) -> device window ramp
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, float, double, int>, ofdm_plan_dev*> plans;
  std::vector<void*>                                            to_free;
  void*                                                         d_gold = nullptr; // Gold-sequence jump table (chest.hip)
  void*                                                         d_pi_il_max = nullptr; // polar interleaver pattern (polar.hip)
  const float**                                                 d_tp_twiddles = nullptr; // transform precoding: twiddle table of 12 N_PRB points at [N_PRB]
};

// A device copy of `bytes` of host memory that lives as long as the context (freed by miphy_destroy): what the context's caches hold.
// When the allocation or the copy fails nothing is kept and *out is left as it was.
int miphy_keep_device_copy(miphy_ctx* ctx, const void* src, size_t bytes, void** out);
template <class T>
int miphy_keep_device_copy(miphy_ctx* ctx, const T* src, size_t count, T** out)
{
  void*     d  = nullptr;
  const int rc = miphy_keep_device_copy(ctx, static_cast<const void*>(src), count * sizeof(T), &d);
  if (!rc)
    *out = static_cast<T*>(d);
  return rc;
}

// Returns the device twiddle table for size N (creates and caches it).
int miphy_get_twiddles(miphy_ctx* ctx, uint32_t N, const float** out);

// Transform precoding (transform_precoding.hip). The device array of the twiddle tables of the 53 de-precoding sizes, table of 12 N_PRB points at
// [N_PRB] (null where N_PRB is none of them), created on first use.
int miphy_tp_twiddles(miphy_ctx* ctx, const float* const** out);
// The host rules of a batch of transform-precoded DM-RS jobs (MIPHY_EINVAL / MIPHY_EUNSUPP and a message that begins with `who`), its widest allocation
// and largest port count; and the pilots kernel on staged jobs: with base_out, a copy of the base records for chest_kernel with the pilots of job i at
// i * stride (cf_t) of `pilots`, a job that breaks a rule without receive ports; without, the pilots at the jobs' pilots_offset.
int miphy_tp_chest_validate(const char* who, const miphy_pusch_chest_tp_job* jobs, uint32_t n, unsigned& max_nprb, unsigned& max_ports);
int miphy_tp_pilots_launch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* d_jobs, uint32_t n, float* pilots, miphy_pusch_chest_job* base_out, uint32_t stride,
                           hipStream_t s);

// miphy_uci_polar_decode_list_batch (uci_polar.hip) for a caller inside the library whose status bytes sit in records of its own: the
// verdict of field i goes to status[status_index[i]] (status_index null: status[i]). `who` names the caller in the error messages.
int miphy_uci_polar_decode_fields(const char* who, miphy_ctx* ctx, const miphy_uci_polar_job* jobs, uint32_t n, uint32_t list_size, const int8_t* llr,
                                  uint8_t* payload, uint8_t* status, const uint32_t* status_index, hipStream_t s);
// The long-PDU path of the coherent PUCCH entry points (JOB = miphy_pucch_job in pucch.hip, miphy_pucch_f34_job in pucch_f34.hip), behind the
// caller's own rule loop: `longs` names the polar-coded PDUs (above 11 bits) in job order with the (K, E) the rules derived. Builds their fields for
// miphy_uci_polar_decode_fields with the byte offset of each status in the miphy_pucch_result array; with llr_out null, routes their soft bits through
// MIPHY_WS_PUCCH_LLR, llr_stride bytes each, in a private copy of the jobs; stages the jobs. llr_long: the long PDUs' soft bits, null without any.
struct miphy_pucch_long_pdu {
  uint32_t job, K, E;
};
struct miphy_pucch_long_staged {
  const void*                      d_jobs   = nullptr;
  int8_t*                          llr_long = nullptr;
  std::vector<miphy_uci_polar_job> fields;
  std::vector<uint32_t>            status_at;
};
template <class JOB>
int miphy_pucch_stage_long(miphy_ctx* ctx, const JOB* jobs, uint32_t n, const std::vector<miphy_pucch_long_pdu>& longs, size_t llr_stride, int8_t* llr_out,
                           hipStream_t s, miphy_pucch_long_staged& out)
{
  for (const miphy_pucch_long_pdu& l : longs) {
    miphy_uci_polar_job pj = {};
    pj.nof_bits = (uint16_t)l.K, pj.nof_llr = l.E, pj.llr_offset = jobs[l.job].llr_offset, pj.payload_offset = jobs[l.job].payload_offset;
    out.fields.push_back(pj);
    out.status_at.push_back(l.job * (uint32_t)sizeof(miphy_pucch_result) + (uint32_t)offsetof(miphy_pucch_result, status));
  }
  out.llr_long = longs.empty() ? nullptr : llr_out;
  std::vector<JOB> own;
  if (!longs.empty() && !llr_out) {
    void* w = nullptr;
    if (const int rc = miphy_get_workspace(ctx, MIPHY_WS_PUCCH_LLR, llr_stride * longs.size(), &w))
      return rc;
    out.llr_long = (int8_t*)w;
    own.assign(jobs, jobs + n);
    for (size_t k = 0; k < longs.size(); ++k)
      out.fields[k].llr_offset = own[longs[k].job].llr_offset = (uint64_t)llr_stride * k;
    jobs = own.data();
  }
  return miphy_stage_descs(ctx, jobs, 0, sizeof(JOB) * (size_t)n, s, &out.d_jobs);
}

// Prepared PDSCH encode (sch.hip): segmentation and descriptor upload once; used by the PDSCH processor plan (pdsch_proc.hip).
struct miphy_pdsch_encode_prepared;
int  miphy_pdsch_encode_prepare(miphy_ctx* ctx, const miphy_pdsch_tb_desc* tbs, uint32_t n, miphy_pdsch_encode_prepared** out);
int  miphy_pdsch_encode_prepared_run(miphy_pdsch_encode_prepared* p, const uint8_t* tb_in, uint8_t* codeword_out, hipStream_t s);
void miphy_pdsch_encode_prepared_destroy(miphy_pdsch_encode_prepared* p);

// Launch halves of miphy_pdsch_modulate_batch and miphy_dmrs_pdsch_map_batch (pdsch_mod.hip), for callers that hold device jobs, the
// Gold tables (miphy_get_gold_tables) and the modulator's scratch of miphy_pdsch_modulate_scratch_bytes(n) bytes already.
struct gold_tables;
size_t miphy_pdsch_modulate_scratch_bytes(uint32_t n);
int    miphy_pdsch_modulate_launch(const miphy_pdsch_mod_job* d_jobs, uint32_t n, const gold_tables* gt, const uint8_t* codewords, float* grid, void* seq,
                                   hipStream_t s);
int    miphy_dmrs_pdsch_map_launch(const miphy_dmrs_pdsch_job* d_jobs, uint32_t n, const gold_tables* gt, float* grid, hipStream_t s);
// The one list of rules for a modulator job on the host (pdsch_mod.hip), for the modulator entry points and for the PDSCH processors, which
// refuse a batch before they enqueue anything: MIPHY_EINVAL and the message "<who>: <what> <i>: ..." on the first rule the job breaks. ports: the grid
// port of each of the nof_layers layers, null for the one-layer entry points (the port is job.port, and the messages name no layer). nof_re: the
// data REs per layer where the caller has counted them already, 0: counted here.
int    miphy_pdsch_mod_job_check(const char* who, const char* what, uint32_t i, const miphy_pdsch_mod_job& job, unsigned nof_layers, const uint8_t* ports,
                                 uint32_t nof_re);
// The list rules of a mapped job on the host (pdsch_mod.hip: PDSCH_MOD_LIST_RULES and PDSCH_MOD_LIST_ENTRY_RULES, which the kernels hold device-resident
// jobs to): MIPHY_EINVAL and the message "<who>: <what> <i>: ..." on the first rule the list of `job` breaks; a job without a list (nof_prb = 0) passes.
int    miphy_pdsch_mod_list_check(const char* who, const char* what, uint32_t i, const miphy_pdsch_mod_mapped_job& job, const uint16_t* prb_lists,
                                  uint32_t nof_list_entries);
// The rules of a codewords job on the host (pdsch_mod.hip: PDSCH_MOD_CODEWORDS_RULES, the field rules, the list rules and PDSCH_MOD_CODEWORDS_SIZE_RULES, in
// that order, which the kernels hold device-resident jobs to); nof_re = data REs per layer when the caller knows them, 0 = count here.
int    miphy_pdsch_mod_codewords_check(const char* who, const char* what, uint32_t i, const miphy_pdsch_mod_codewords_job& job, const uint16_t* prb_lists,
                                       uint32_t nof_list_entries, uint32_t nof_re);
// The rules of a precoding on the host (pdsch_mod.hip: PDSCH_PRECODING_RULES, likewise): nof_layers = the layers of the job, rb_mask = its five mask
// words, nof_weights = cf_t entries of the call's weights. MIPHY_EINVAL and the message "<who>: <what> <i>: precoding: ..." on the first rule broken.
int    miphy_precoding_check(const char* who, const char* what, uint32_t i, const miphy_precoding& p, unsigned nof_layers, const uint64_t* rb_mask,
                             uint32_t nof_weights);
// The rules of a precoded DM-RS job on the host: those of its DM-RS part, then miphy_precoding_check.
int    miphy_dmrs_pdsch_precoded_job_check(const char* who, const char* what, uint32_t i, const miphy_dmrs_pdsch_precoded_job& job, uint32_t nof_weights);
// The staging, the scratch and the two launches behind miphy_pdsch_modulate_layers_batch, _mapped_batch and _precoded_batch (pdsch_mod.hip), for JOB =
// miphy_pdsch_mod_layers_job, miphy_pdsch_mod_mapped_job, miphy_pdsch_mod_precoded_job or miphy_pdsch_mod_codewords_job (_codewords_batch): jobs that
// passed the checks above, or that sit on the device with their lists and weights, where the kernels validate them. Host jobs go to the staging ring in one upload together with the host lists (mapped and
// precoded jobs) and the host weights (precoded jobs); the arrays a kind of job does not have are not looked at. max_layers = the largest nof_layers of
// the batch (codewords jobs: the largest layer count of one codeword), 4 for device-resident jobs.
template <class JOB>
int miphy_pdsch_modulate_layered_enqueue(miphy_ctx* ctx, const JOB* jobs, int jobs_on_device, uint32_t n, uint32_t max_layers, const uint16_t* prb_lists,
                                         uint32_t nof_list_entries, const float* weights, uint32_t nof_weights, const uint8_t* codewords, float* grid, hipStream_t s);

// One codeblock of the transport-block level PDSCH encoder (pdsch_cb_encode.hip): assembly from the transport block, LDPC encoding and rate
// matching in one kernel.
struct miphy_pdsch_cb_desc {
  uint64_t tb_offset;       // packed transport-block bytes
  uint64_t cw_offset;       // byte offset of this codeblock's E rate-matched bits (one per byte) in the codeword array
  uint32_t tb_bit_offset;   // first transport-block bit of the codeblock
  uint32_t take_bits;       // transport-block bits copied
  uint32_t tb_index;        // index into the TB CRC array
  uint32_t E, Nref, out_len; // rate-matched length, limited buffer (0 = none), part of the circular buffer the rate matcher reads
  uint16_t nof_tb_crc_bits, zero_pad; // > 0 on the last codeblock: append the TB CRC and the zero padding
  uint16_t Z, nof_filler_bits;
  uint8_t  nof_cb_crc_bits, bg, rv, mod;
  uint32_t K;
};
// A codeblock the bit-packed kernel takes (pdsch_cb_encode.hip): lifting size a multiple of 32, byte-aligned pieces, selected bits within its LDS buffer.
__host__ __device__ inline bool miphy_pdsch_cb_packed_ok(const miphy_pdsch_cb_desc& d)
{
  return d.Z % 32 == 0 && d.tb_bit_offset % 8 == 0 && d.take_bits % 8 == 0 && d.zero_pad % 8 == 0 && d.nof_tb_crc_bits % 8 == 0 &&
         (d.nof_cb_crc_bits == 0 || d.nof_cb_crc_bits == 24) && d.E <= (1u << 16);
}
size_t miphy_pdsch_cb_encode_lds(uint32_t K, uint32_t Z, uint32_t out_len);
size_t miphy_pdsch_cb_encode_pk_lds(const miphy_pdsch_cb_desc& d);
int    miphy_pdsch_cb_encode_launch(miphy_ctx* ctx, const miphy_pdsch_cb_desc* d_descs, uint32_t ncb, size_t max_lds, const uint8_t* tb_in, const uint32_t* tb_crc,
                                    uint8_t* cw_out, hipStream_t s, uint32_t npacked = 0, size_t max_lds_pk = 0);
