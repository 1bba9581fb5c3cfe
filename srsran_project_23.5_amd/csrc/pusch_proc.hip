// PUSCH processor: channel estimation, demodulation and transport-block decoding of a batch of PUSCH PDUs in one
// call, everything between the resource grid and the transport block stays on the device.
// Behaviour contract: lib/phy/upper/channel_processors/pusch_processor_impl.cpp:108-330 for PDUs without UCI (the reference
// itself restricts the rest: DM-RS type 1, two CDM groups without data, one layer: pusch_processor_impl.cpp:96-104,331-345).
// This is host-side composition of miphy_dmrs_pusch_estimate_batch, miphy_pusch_demodulate_batch and miphy_pusch_decode_batch
// with the parameters the reference derives (DM-RS scaling from the SCH-to-DM-RS power ratio, codeword length from the allocation);
// with multiplexed UCI, miphy_ulsch_demultiplex_batch between the last two. One codeword on 1..4 layers goes through the layered stages, a
// transform-precoded PUSCH (DFT-s-OFDM) through miphy_dmrs_pusch_estimate_tp_batch and miphy_pusch_demodulate_tp_batch, a layered PDU with MMSE-IRC
// through the layered estimator, miphy_pusch_noise_covariance_batch and miphy_pusch_demodulate_layers_mmse_batch_ex. A layered PDU of a UE with a carrier
// frequency offset goes through miphy_dmrs_pusch_estimate_cfo_batch, whose estimate differs from symbol to symbol and is kept per symbol; one whose
// channel changes within the slot through miphy_dmrs_pusch_estimate_tv_batch in its place.
#include "miphy_ext.h"
#include <cmath>
#include <vector>

namespace {
// EVM of every PDU from the per-symbol sums of the demodulator: sqrt(sum / data REs) (evm_calculator_generic_impl.cpp:45-46).
__global__ void evm_finish_kernel(const float* __restrict__ sums, const uint32_t* __restrict__ nof_re, float* __restrict__ evm, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  float acc = 0.f;
  for (int l = 0; l < 14; ++l)
    acc += sums[(size_t)i * 14 + l];
  evm[i] = nof_re[i] ? sqrtf(acc / (float)nof_re[i]) : 0.f;
}
__global__ void zero_results_kernel(miphy_pusch_result* __restrict__ r, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    r[i] = miphy_pusch_result{};
}

// What the _ex processors enqueue for a batch, built once from the PDUs: the one-layer entry point (lpdus == NULL: every PDU on one layer, 20 scalars
// per PDU, the one-layer rules) and the layered one (the layer count of each PDU, 80 scalars, the layered rules) differ in nothing else. The waveform:
// with tpdus (transform precoding: one layer, 20 scalars) the estimator jobs carry the hopping mode (tcj) and the PDUs are held to the rules of the two
// transform-precoded stages. With mpdus (MMSE-IRC: layered PDUs, their rules and scalars) there is a covariance job per PDU (nj) and the demodulator
// jobs carry where its matrices are (mj).
struct pusch_batch {
  std::vector<miphy_pusch_chest_job>        cj;
  std::vector<miphy_pusch_chest_tp_job>     tcj;      // transform precoding: cj with the hopping mode
  std::vector<miphy_pusch_demod_layers_job> dj;
  std::vector<miphy_pusch_tb_desc>          tb;
  std::vector<miphy_ulsch_demux_job>        xj;       // PDUs with multiplexed UCI
  std::vector<uint16_t>                     ph;       // their repetition placeholders, back to back
  std::vector<uint32_t>                     nof_sym;  // data REs x layers per PDU (EVM)
  std::vector<uint32_t>                     tb_index; // PDU of every transport-block descriptor
  std::vector<miphy_pusch_ncov_job>         nj;       // MMSE-IRC: cj with the PRG size, the loading and where the matrices go
  std::vector<miphy_pusch_demod_mmse_job>   mj;       // MMSE-IRC: dj with the PRG size and where the matrices are
  size_t                                    ce_elems = 0, llr_bytes = 0, sch_bytes = 0, cov_elems = 0;
};

int pusch_batch_build(const miphy_pusch_pdu* pdus, const miphy_pusch_layers_pdu* lpdus_in, const miphy_pusch_tp_pdu* tpdus, const miphy_pusch_mmse_pdu* mpdus,
                      const miphy_pusch_uci* uci, uint32_t n, bool have_uci_out, bool ce_per_symbol, pusch_batch& b)
{
  b.cj.resize(n), b.dj.resize(n), b.nof_sym.resize(n);
  std::vector<miphy_pusch_layers_pdu> layered_of_mmse; // the layered PDU inside every MMSE PDU, in one array like lpdus_in
  if (mpdus) {
    layered_of_mmse.resize(n);
    for (uint32_t i = 0; i < n; ++i)
      layered_of_mmse[i] = mpdus[i].base;
  }
  const miphy_pusch_layers_pdu* lpdus = mpdus ? layered_of_mmse.data() : lpdus_in;
  const bool strict = lpdus || tpdus; // the entry points beyond the reference check what their stages would only find once the estimator is enqueued
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pusch_pdu& p = lpdus ? lpdus[i].base : (tpdus ? tpdus[i].base : pdus[i]);
    const unsigned         L = lpdus ? lpdus[i].nof_tx_layers : 1;
    if (mpdus)
      MIPHY_REQUIRE(mpdus[i].loading >= 0.f && mpdus[i].loading <= 3.402823466e+38f, "pusch_process: PDU %u: the diagonal loading should be finite and not negative", i);
    const miphy_pusch_uci* u = uci ? &uci[i] : nullptr;
    const bool has_uci = u && (u->nof_harq_ack_bits || u->nof_csi_part1_bits || u->nof_csi_part2_bits);
    const bool has_tb  = !u || u->has_codeword;
    MIPHY_REQUIRE(p.nof_rx_ports >= 1 && p.nof_rx_ports <= 4, "pusch_process: PDU %u: invalid number of receive ports", i);
    if (lpdus) {
      MIPHY_REQUIRE(L >= 1 && L <= 4, "pusch_process: PDU %u: invalid number of layers %u", i, L);
      MIPHY_REQUIRE(L <= p.nof_rx_ports, "pusch_process: PDU %u: %u layers on %u receive ports", i, L, (unsigned)p.nof_rx_ports);
    }
    if (strict)
      MIPHY_REQUIRE(p.numerology <= 4, "pusch_process: PDU %u: invalid numerology", i);
    MIPHY_REQUIRE(p.nof_symbols >= 1 && p.start_symbol + p.nof_symbols <= 14, "pusch_process: PDU %u: invalid time allocation", i);
    if (!strict)
      MIPHY_REQUIRE(p.dmrs_symbols_mask != 0, "pusch_process: PDU %u: no DM-RS symbol", i);
    MIPHY_REQUIRE(p.grid_nof_prb >= 1 && p.grid_nof_prb <= 275, "pusch_process: PDU %u: invalid grid width", i);
    if (strict) {
      unsigned nds = 0;
      for (unsigned l = p.start_symbol; l < (unsigned)p.start_symbol + p.nof_symbols; ++l)
        nds += (p.dmrs_symbols_mask >> l) & 1;
      MIPHY_REQUIRE(nds >= 1 && nds <= 4, "pusch_process: PDU %u: %u DM-RS symbols in the allocation (1..4 supported)", i, nds);
      MIPHY_REQUIRE(p.mod == 1 || p.mod == 2 || p.mod == 4 || p.mod == 6 || p.mod == 8, "pusch_process: PDU %u: invalid modulation", i);
      if (tpdus)
        MIPHY_REQUIRE(p.n_id < 1024 && p.rnti < 65536, "pusch_process: PDU %u: invalid scrambling identifier or RNTI", i);
      if (has_tb) { // (the decoder's rules on the transport block, which it would only find behind the stages in front of it)
        MIPHY_REQUIRE((p.bg == 1 || p.bg == 2) && p.rv <= 3 && p.nof_ldpc_iterations > 0, "pusch_process: PDU %u: invalid base graph, redundancy version or iterations", i);
        miphy_sch_segmentation sg = {};
        MIPHY_REQUIRE(miphy_sch_segmentation_info(p.tb_bytes, p.bg, &sg) == MIPHY_OK, "pusch_process: PDU %u: transport block of %u bytes cannot be segmented", i, p.tb_bytes);
        MIPHY_REQUIRE((sg.cb_info_bits % 8) == 0 || sg.nof_cbs == 1,
                      "pusch_process: PDU %u: %u bytes is not a TS 38.214 transport block size (codeblock payloads are not byte aligned)", i, p.tb_bytes);
      }
    }
    const uint32_t nsc = p.grid_nof_prb * 12u, nsym_ce = (uint32_t)p.start_symbol + p.nof_symbols;
    miphy_pusch_chest_job& c = b.cj[i];
    c                        = {};
    c.numerology = p.numerology, c.slot_in_frame = p.slot_in_frame, c.scrambling_id = p.dmrs_scrambling_id;
    // pusch_processor_impl.cpp:150: amplitude of the DM-RS relative to the data, two CDM groups without data -> +3 dB
    c.scaling = powf(10.0f, 3.0f / 20.0f);
    c.n_scid = p.n_scid, c.nof_tx_layers = (uint8_t)L, c.nof_rx_ports = p.nof_rx_ports, c.first_symbol = p.start_symbol, c.nof_symbols = p.nof_symbols;
    c.symbols_mask = p.dmrs_symbols_mask, c.grid_nof_prb = p.grid_nof_prb;
    // the estimate only feeds the demodulator below: one row per port instead of a copy per symbol -- unless the symbols differ (ce_per_symbol: the
    // estimator that compensates a carrier frequency offset)
    c.ce_compact = ce_per_symbol ? 0 : 1;
    miphy_pusch_demod_layers_job& lj = b.dj[i];
    lj                               = {};
    lj.nof_tx_layers                 = (uint8_t)L;
    miphy_pusch_demod_job& d         = lj.base;
    d.rnti = p.rnti, d.n_id = p.n_id, d.mod = p.mod, d.nof_rx_ports = p.nof_rx_ports, d.start_symbol = p.start_symbol, d.nof_symbols = p.nof_symbols;
    d.dmrs_type = 1, d.nof_cdm_groups_without_data = 2, d.ce_nof_symbols = (uint8_t)nsym_ce, d.ce_compact = c.ce_compact;
    d.dmrs_symbols_mask = p.dmrs_symbols_mask, d.grid_nof_prb = p.grid_nof_prb;
    for (int k = 0; k < 4; ++k)
      c.rx_ports[k] = p.rx_ports[k], d.rx_ports[k] = p.rx_ports[k];
    for (int k = 0; k < 5; ++k)
      c.rb_mask[k] = p.rb_mask[k], d.rb_mask[k] = p.rb_mask[k];
    c.grid_offset = d.grid_offset = p.grid_offset;
    c.ce_offset = d.ce_offset = b.ce_elems;
    // per PDU [4 ports][5] floats of layer 0, or [4 ports][4 layers][5]
    c.scalars_offset = d.scalars_offset = (uint64_t)i * (lpdus ? 80 : 20);
    d.llr_offset                       = b.llr_bytes;
    d.nof_llr                          = lpdus ? miphy_pusch_demod_layers_nof_llr(&lj) : miphy_pusch_demod_nof_llr(&d);
    MIPHY_REQUIRE(d.nof_llr > 0, "pusch_process: PDU %u: empty allocation", i);
    d.evm_offset = (uint64_t)i * 14;
    b.nof_sym[i] = d.nof_llr / p.mod;
    uint64_t sch_llr_offset = b.llr_bytes; // where the decoder reads the UL-SCH soft bits: the codeword itself unless UCI is multiplexed
    uint32_t nof_sch_llr    = d.nof_llr;
    if (has_uci) {
      MIPHY_REQUIRE(have_uci_out, "pusch_process: PDU %u carries UCI but uci_llr_out is NULL", i);
      miphy_ulsch_demux_job x    = {};
      const uint32_t        nprb = miphy_count_prb(p.rb_mask, p.grid_nof_prb);
      x.mod = p.mod, x.nof_layers = (uint8_t)L, x.start_symbol = p.start_symbol, x.nof_symbols = p.nof_symbols, x.dmrs_type = 1, x.nof_cdm_groups_without_data = 2;
      x.dmrs_symbols_mask = p.dmrs_symbols_mask, x.nof_prb = (uint16_t)nprb, x.nof_harq_ack_rvd = u->nof_harq_ack_rvd;
      x.nof_enc_harq_ack_bits = u->nof_enc_harq_ack_bits, x.nof_enc_csi_part1_bits = u->nof_enc_csi_part1_bits;
      x.nof_enc_csi_part2_bits = u->nof_enc_csi_part2_bits;
      x.nof_harq_ack_bits = u->nof_harq_ack_bits, x.nof_csi_part1_bits = u->nof_csi_part1_bits, x.nof_csi_part2_bits = u->nof_csi_part2_bits;
      uint32_t nin = 0;
      int      rc  = miphy_ulsch_demux_sizes(&x, &nin, &nof_sch_llr);
      if (rc)
        return rc;
      MIPHY_REQUIRE(nin == d.nof_llr, "pusch_process: PDU %u: the UL-SCH multiplexing covers %u soft bits, the allocation holds %u", i, nin, d.nof_llr);
      x.in_offset = b.llr_bytes, x.sch_offset = b.sch_bytes, x.harq_ack_offset = u->harq_ack_offset, x.csi_part1_offset = u->csi_part1_offset;
      x.csi_part2_offset = u->csi_part2_offset;
      b.xj.push_back(x);
      // repetition placeholders of the descrambler
      uint32_t nph = 0;
      if ((rc = miphy_ulsch_placeholders(&x, nullptr, 0, &nph)))
        return rc;
      d.placeholders_offset = (uint32_t)b.ph.size(), d.nof_placeholders = nph;
      b.ph.resize(b.ph.size() + nph);
      if (nph && (rc = miphy_ulsch_placeholders(&x, b.ph.data() + d.placeholders_offset, nph, &nph)))
        return rc;
      sch_llr_offset = b.sch_bytes; // relative to the SCH region, rebased below
      b.sch_bytes += (nof_sch_llr + 15u) & ~15u;
    }
    // include/miphy.h: has_codeword = 0 means the PDU carries no transport block -- whatever its UCI fields say. A PDU with neither is
    // not a PUSCH transmission.
    MIPHY_REQUIRE(has_tb || has_uci, "pusch_process: PDU %u: neither a codeword nor UCI", i);
    if (has_tb) {
      miphy_pusch_tb_desc t = {};
      t.bg = p.bg, t.rv = p.rv, t.mod = p.mod, t.nof_layers = (uint8_t)L, t.new_data = p.new_data, t.use_early_stop = p.use_early_stop;
      t.nof_ldpc_iterations = p.nof_ldpc_iterations, t.Nref = p.Nref, t.nof_ch_symbols = nof_sch_llr / p.mod, t.tb_bytes = p.tb_bytes;
      t.harq_cb_index = p.harq_cb_index, t.tb_offset = p.tb_offset;
      t.llr_offset = has_uci ? (uint64_t)1 << 63 | sch_llr_offset : sch_llr_offset; // bit 63: offset inside the SCH region (resolved below)
      b.tb.push_back(t);
      b.tb_index.push_back(i);
    }
    b.ce_elems += (size_t)L * p.nof_rx_ports * nsc * (ce_per_symbol ? nsym_ce : 1u);
    b.llr_bytes += (d.nof_llr + 15u) & ~15u;
  }
  for (auto& t : b.tb) // SCH region behind the codeword LLRs
    if (t.llr_offset >> 63)
      t.llr_offset = (t.llr_offset & ~((uint64_t)1 << 63)) + b.llr_bytes;
  for (auto& x : b.xj)
    x.sch_offset += b.llr_bytes;
  if (mpdus) { // the covariance and demodulator jobs: the estimator's and the layered demodulator's with the PRG size; matrices back to back
    b.nj.resize(n), b.mj.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      b.nj[i]            = {};
      b.nj[i].base       = b.cj[i];
      b.nj[i].cov_offset = b.cov_elems;
      b.nj[i].loading    = mpdus[i].loading;
      b.nj[i].prg_size   = mpdus[i].prg_size;
      b.mj[i]            = {};
      b.mj[i].base       = b.dj[i];
      b.mj[i].cov_offset = b.cov_elems;
      b.mj[i].prg_size   = mpdus[i].prg_size;
      const uint32_t nprg = miphy_pusch_noise_covariance_nof_prg(&b.nj[i]);
      MIPHY_REQUIRE(nprg > 0, "pusch_process: PDU %u: the noise covariance estimator refuses its job", i);
      b.cov_elems += (size_t)nprg * b.cj[i].nof_rx_ports * b.cj[i].nof_rx_ports;
    }
  }
  if (tpdus) { // the rules of the transform-precoded stages on the allocation and the DM-RS (contiguous, 2^a 3^b 5^c PRBs, n_ID^RS, hopping mode)
    b.tcj.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      b.tcj[i]         = {};
      b.tcj[i].base    = b.cj[i];
      b.tcj[i].hopping = tpdus[i].hopping;
    }
    unsigned max_nprb, max_ports;
    return miphy_tp_chest_validate("pusch_process_tp", b.tcj.data(), n, max_nprb, max_ports);
  }
  return MIPHY_OK;
}

// Estimator, demodulator with placeholders and EVM, EVM finish (divisor: data REs x layers), demultiplexer and decoder on one stream. Every rule is
// checked before anything is enqueued (pusch_batch_build); the stages check their own rules again on the jobs built there.
int pusch_process_ex(miphy_ctx* ctx, const miphy_pusch_pdu* pdus, const miphy_pusch_layers_pdu* lpdus, const miphy_pusch_tp_pdu* tpdus,
                     const miphy_pusch_mmse_pdu* mpdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs,
                     uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, float* cfo_out,
                     uint32_t time_mode, float* var_out, hipStream_t s)
{
  pusch_batch b;
  int         rc = pusch_batch_build(pdus, lpdus, tpdus, mpdus, uci, n, uci_llr_out != nullptr, cfo_out != nullptr, b);
  if (rc)
    return rc;
  // [placeholders | data REs || channel estimates cf_t | codeword LLRs, UL-SCH LLRs of the PDUs with UCI | EVM sums] in a workspace of the
  // context, the two arrays in front uploaded as one; the estimator scalars go straight to the caller's array.
  device_image img;
  const auto   s_ph  = img.put(b.ph);
  const auto   s_nre = img.put(b.nof_sym.data(), evm_out ? n : 0); // (read by the EVM kernel only)
  const auto   s_ce  = img.reserve<float>(b.ce_elems * 2, 256);
  const auto   s_llr = img.reserve<int8_t>(b.llr_bytes + b.sch_bytes, 256);
  const auto   s_evm = img.reserve<float>(evm_out ? (size_t)n * 14 : 0);
  const auto   s_cov = mpdus ? img.reserve<float>(b.cov_elems * 2, 256) : image_slot<float>{}; // (MMSE-IRC only: the covariance matrices of every PDU)
  void*        work  = nullptr;
  if ((rc = miphy_image_to_workspace(ctx, MIPHY_WS_PUSCH_PROC, img, s, &work)))
    return rc;
  float*          d_ce  = s_ce.at(work);
  int8_t*         d_llr = s_llr.at(work);
  float*          d_evm = evm_out ? s_evm.at(work) : nullptr;
  const uint16_t* d_ph  = b.ph.empty() ? nullptr : s_ph.at(work);
  uint32_t*       d_nre = s_nre.at(work);
  if (mpdus) {
    float* d_cov = s_cov.at(work);
    if ((rc = miphy_dmrs_pusch_estimate_layers_batch(ctx, b.cj.data(), 0, n, grid, d_ce, scalars_out, s)))
      return rc;
    if ((rc = miphy_pusch_noise_covariance_batch(ctx, b.nj.data(), 0, n, grid, d_cov, s)))
      return rc;
    if ((rc = miphy_pusch_demodulate_layers_mmse_batch_ex(ctx, b.mj.data(), 0, n, grid, d_ce, scalars_out, d_cov, d_llr, d_ph, d_evm, s)))
      return rc;
  } else if (lpdus && var_out) { // (layered PDUs only) the per-symbol estimate that follows the channel through the slot; the variation of PDU i at 16 i
    std::vector<miphy_pusch_chest_tv_job> vj(n);
    for (uint32_t i = 0; i < n; ++i)
      vj[i] = {}, vj[i].base.base = b.cj[i], vj[i].base.cfo_offset = 2ull * i, vj[i].var_offset = 16ull * i, vj[i].time_mode = (uint8_t)time_mode;
    if ((rc = miphy_dmrs_pusch_estimate_tv_batch(ctx, vj.data(), 0, n, grid, d_ce, scalars_out, cfo_out, var_out, s)))
      return rc;
    if ((rc = miphy_pusch_demodulate_layers_batch_ex(ctx, b.dj.data(), 0, n, grid, d_ce, scalars_out, d_llr, d_ph, d_evm, s)))
      return rc;
  } else if (lpdus && cfo_out) { // (layered PDUs only) the per-symbol estimate of the offset-compensating estimator, {cfo_hz, rho} of PDU i at 2 i
    std::vector<miphy_pusch_chest_cfo_job> fj(n);
    for (uint32_t i = 0; i < n; ++i)
      fj[i].base = b.cj[i], fj[i].cfo_offset = 2ull * i;
    if ((rc = miphy_dmrs_pusch_estimate_cfo_batch(ctx, fj.data(), 0, n, grid, d_ce, scalars_out, cfo_out, s)))
      return rc;
    if ((rc = miphy_pusch_demodulate_layers_batch_ex(ctx, b.dj.data(), 0, n, grid, d_ce, scalars_out, d_llr, d_ph, d_evm, s)))
      return rc;
  } else if (lpdus) {
    if ((rc = miphy_dmrs_pusch_estimate_layers_batch(ctx, b.cj.data(), 0, n, grid, d_ce, scalars_out, s)))
      return rc;
    if ((rc = miphy_pusch_demodulate_layers_batch_ex(ctx, b.dj.data(), 0, n, grid, d_ce, scalars_out, d_llr, d_ph, d_evm, s)))
      return rc;
  } else {
    std::vector<miphy_pusch_demod_job> dj(n);
    for (uint32_t i = 0; i < n; ++i)
      dj[i] = b.dj[i].base;
    if (tpdus) {
      if ((rc = miphy_dmrs_pusch_estimate_tp_batch(ctx, b.tcj.data(), 0, n, grid, d_ce, scalars_out, s)))
        return rc;
      if ((rc = miphy_pusch_demodulate_tp_batch_ex(ctx, dj.data(), 0, n, grid, d_ce, scalars_out, d_llr, d_ph, d_evm, s)))
        return rc;
    } else {
      if ((rc = miphy_dmrs_pusch_estimate_batch(ctx, b.cj.data(), 0, n, grid, d_ce, scalars_out, s)))
        return rc;
      if ((rc = miphy_pusch_demodulate_batch_ex(ctx, dj.data(), 0, n, grid, d_ce, scalars_out, d_llr, d_ph, d_evm, s)))
        return rc;
    }
  }
  if (evm_out) {
    hipLaunchKernelGGL(evm_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_evm, d_nre, evm_out, n);
    MIPHY_HIP_CHECK(hipGetLastError());
  }
  if (!b.xj.empty() &&
      (rc = miphy_ulsch_demultiplex_batch(ctx, b.xj.data(), (uint32_t)b.xj.size(), d_llr, d_llr, uci_llr_out, uci_llr_out, uci_llr_out, s)))
    return rc;
  if (b.tb.size() == n) // the common case: every PDU has a transport block, results in PDU order
    return miphy_pusch_decode_batch(ctx, b.tb.data(), n, d_llr, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, s);
  // Some PDUs carry UCI only: decode the others into a compact result array, then put the records in PDU order.
  hipLaunchKernelGGL(zero_results_kernel, dim3((n + 255) / 256), dim3(256), 0, s, results, n);
  MIPHY_HIP_CHECK(hipGetLastError());
  if (b.tb.empty())
    return MIPHY_OK;
  void* rws = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_OUTPUT, b.tb.size() * sizeof(miphy_pusch_result), &rws)))
    return rc;
  if ((rc = miphy_pusch_decode_batch(ctx, b.tb.data(), (uint32_t)b.tb.size(), d_llr, harq_softbits, harq_msgs, harq_crc_ok, tb_out, (miphy_pusch_result*)rws, s)))
    return rc;
  for (size_t k = 0; k < b.tb.size(); ++k)
    MIPHY_HIP_CHECK(hipMemcpyAsync(results + b.tb_index[k], (miphy_pusch_result*)rws + k, sizeof(miphy_pusch_result), hipMemcpyDeviceToDevice, s));
  return MIPHY_OK;
}
} // namespace

extern "C" int miphy_pusch_process_batch(miphy_ctx* ctx, const miphy_pusch_pdu* pdus, uint32_t n, const float* grid, int8_t* harq_softbits,
                                         uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results, float* scalars_out,
                                         void* stream)
{
  return miphy_pusch_process_batch_ex(ctx, pdus, nullptr, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, nullptr, nullptr,
                                      stream);
}

// One codeword on 1..4 layers, with multiplexed UCI and the EVM (include/miphy.h).
extern "C" int miphy_pusch_process_layers_batch_ex(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                                   int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                                   miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out,
                "miphy_pusch_process_layers_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, nullptr, pdus, nullptr, nullptr, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out, evm_out, nullptr,
                          0, nullptr, (hipStream_t)stream);
}

extern "C" int miphy_pusch_process_layers_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus, uint32_t n, const float* grid, int8_t* harq_softbits,
                                                uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results,
                                                float* scalars_out, void* stream)
{
  return miphy_pusch_process_layers_batch_ex(ctx, pdus, nullptr, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, nullptr,
                                             nullptr, stream);
}

extern "C" int miphy_pusch_process_batch_ex(miphy_ctx* ctx, const miphy_pusch_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                            int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results,
                                            float* scalars_out, int8_t* uci_llr_out, float* evm_out, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out,
                "miphy_pusch_process_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, pdus, nullptr, nullptr, nullptr, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out, evm_out, nullptr,
                          0, nullptr, (hipStream_t)stream);
}

// A transform-precoded PUSCH (DFT-s-OFDM), with multiplexed UCI and the EVM (include/miphy.h).
extern "C" int miphy_pusch_process_tp_batch_ex(miphy_ctx* ctx, const miphy_pusch_tp_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                               int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results,
                                               float* scalars_out, int8_t* uci_llr_out, float* evm_out, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out,
                "miphy_pusch_process_tp_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, nullptr, nullptr, pdus, nullptr, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out, evm_out, nullptr,
                          0, nullptr, (hipStream_t)stream);
}

extern "C" int miphy_pusch_process_tp_batch(miphy_ctx* ctx, const miphy_pusch_tp_pdu* pdus, uint32_t n, const float* grid, int8_t* harq_softbits,
                                            uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out, miphy_pusch_result* results, float* scalars_out,
                                            void* stream)
{
  return miphy_pusch_process_tp_batch_ex(ctx, pdus, nullptr, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, nullptr, nullptr,
                                         stream);
}

// The layered processor with the estimator that estimates and compensates a carrier frequency offset in front (include/miphy.h).
extern "C" int miphy_pusch_process_layers_cfo_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                                    int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                                    miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, float* cfo_out,
                                                    void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out && cfo_out,
                "miphy_pusch_process_layers_cfo_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, nullptr, pdus, nullptr, nullptr, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out, evm_out,
                          cfo_out, 0, nullptr, (hipStream_t)stream);
}

// The layered processor with the estimator that follows a channel through the slot in front (include/miphy.h).
extern "C" int miphy_pusch_process_layers_tv_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                                   int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                                   miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, float* cfo_out,
                                                   uint32_t time_mode, float* var_out, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out && cfo_out && var_out,
                "miphy_pusch_process_layers_tv_batch: null argument");
  MIPHY_REQUIRE(time_mode == MIPHY_TIME_INTERPOLATE || time_mode == MIPHY_TIME_LINE,
                "miphy_pusch_process_layers_tv_batch: time_mode must be MIPHY_TIME_INTERPOLATE or MIPHY_TIME_LINE");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, nullptr, pdus, nullptr, nullptr, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out, evm_out,
                          cfo_out, time_mode, var_out, (hipStream_t)stream);
}

// One codeword on 1..4 layers through MMSE-IRC: the layered processor with the covariance estimator between its estimator and an MMSE demodulator.
extern "C" int miphy_pusch_process_layers_mmse_batch(miphy_ctx* ctx, const miphy_pusch_mmse_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, const float* grid,
                                                     int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                                     miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid && harq_softbits && harq_msgs && harq_crc_ok && tb_out && results && scalars_out,
                "miphy_pusch_process_layers_mmse_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  return pusch_process_ex(ctx, nullptr, nullptr, nullptr, pdus, uci, n, grid, harq_softbits, harq_msgs, harq_crc_ok, tb_out, results, scalars_out, uci_llr_out,
                          evm_out, nullptr, 0, nullptr, (hipStream_t)stream);
}
