// PDSCH processor: transport blocks to resource-grid REs in one call, the codewords stay on the device.
// Behaviour contract: lib/phy/upper/channel_processors/pdsch_processor_impl.cpp:110-305 (process = encode + modulate + put_dmrs,
// with the restrictions of assert_pdu :143-196). Host-side composition of miphy_pdsch_encode_batch, miphy_pdsch_modulate_batch and
// miphy_dmrs_pdsch_map_batch with the parameters the reference derives from the PDU.
#include "gold_device.h"
#include "miphy_ext.h"
#include <cmath>
#include <type_traits>
#include <vector>

namespace {
// pdsch_processor_impl::modulate (:256-276): the modulator configuration of a PDU.
void mod_job_of(const miphy_pdsch_pdu& p, miphy_pdsch_mod_job& m)
{
  m      = {};
  m.rnti = p.rnti, m.n_id = p.n_id, m.mod = p.mod, m.port = p.port, m.start_symbol = p.start_symbol, m.nof_symbols = p.nof_symbols;
  m.scaling   = powf(10.0f, -p.ratio_pdsch_data_to_sss_dB / 20.0f); // convert_dB_to_amplitude(-ratio)
  m.dmrs_type = 1, m.nof_cdm_groups_without_data = p.nof_cdm_groups_without_data, m.nof_reserved = p.nof_reserved;
  m.dmrs_symbols_mask = p.dmrs_symbols_mask, m.grid_nof_prb = p.grid_nof_prb, m.bwp_start_rb = p.bwp_start_rb, m.bwp_size_rb = p.bwp_size_rb;
  for (int k = 0; k < 5; ++k)
    m.rb_mask[k] = p.rb_mask[k];
  for (int k = 0; k < 4; ++k)
    m.reserved[k] = p.reserved[k];
  m.grid_offset = p.grid_offset;
}
} // namespace

extern "C" uint32_t miphy_pdsch_pdu_nof_re(const miphy_pdsch_pdu* pdu)
{
  if (!pdu || pdu->nof_reserved > 4)
    return 0;
  miphy_pdsch_mod_job m;
  mod_job_of(*pdu, m);
  return miphy_pdsch_mod_nof_re(&m);
}

namespace {
// What pdsch_processor_impl::process derives from PDU i of a batch (assert_pdu :143-196, modulate :256-276, put_dmrs :278-305) for one codeword on L
// layers: the encoder's transport-block record, the modulator job and the DM-RS job; cw_bytes = bytes of the codeword area so far (one bit per
// byte), advanced by the PDU's codeword. ports: the grid port of each layer, null for the one-layer forms (L = 1 on p.port). Every rule of the
// three steps that the PDU can break is checked here, so that a processor refuses a batch before it enqueues or allocates anything.
int derive_pdsch_jobs(const char* who, uint32_t i, const miphy_pdsch_pdu& p, unsigned L, const uint8_t* ports, miphy_pdsch_tb_desc& t, miphy_pdsch_mod_job& m,
                      miphy_dmrs_pdsch_job& d, size_t& cw_bytes)
{
  MIPHY_REQUIRE(p.dmrs_symbols_mask != 0 && p.dmrs_symbols_mask < (1u << 14), "pdsch_process: PDU %u: invalid DM-RS symbol mask", i);
  MIPHY_REQUIRE(p.nof_symbols >= 1 && p.start_symbol + p.nof_symbols <= 14, "pdsch_process: PDU %u: the time allocation exceeds the slot", i);
  const unsigned first_dmrs = __builtin_ctz(p.dmrs_symbols_mask), last_dmrs = 31 - __builtin_clz((unsigned)p.dmrs_symbols_mask);
  MIPHY_REQUIRE(first_dmrs >= p.start_symbol && last_dmrs < (unsigned)p.start_symbol + p.nof_symbols,
                "pdsch_process: PDU %u: DM-RS symbols outside the time allocation", i);
  MIPHY_REQUIRE(p.nof_cdm_groups_without_data >= 1 && p.nof_cdm_groups_without_data <= 2, "pdsch_process: PDU %u: invalid number of CDM groups without data", i);
  MIPHY_REQUIRE(p.tbs_lbrm_bytes > 0 && p.tbs_lbrm_bytes <= 66 * 384 / 8, "pdsch_process: PDU %u: invalid LBRM size (%u bytes)", i, p.tbs_lbrm_bytes);
  MIPHY_REQUIRE(p.nof_reserved <= 4, "pdsch_process: PDU %u: at most 4 reserved RE patterns", i);
  MIPHY_REQUIRE(p.bg == 1 || p.bg == 2, "pdsch_process: PDU %u: invalid base graph", i);
  mod_job_of(p, m);
  const uint32_t nre = miphy_pdsch_mod_nof_re(&m); // per layer
  MIPHY_REQUIRE(nre > 0, "pdsch_process: PDU %u: invalid or empty allocation", i);
  m.nof_bits  = nre * L * p.mod;
  m.cw_offset = cw_bytes;
  if (int rc = miphy_pdsch_mod_job_check(who, "PDU", i, m, L, ports, nre))
    return rc;
  MIPHY_REQUIRE(!p.ref_point_prb0 || p.bwp_start_rb < p.grid_nof_prb, "%s: PDU %u: reference point outside the grid", who, i);
  t    = {};
  t.bg = p.bg, t.rv = p.rv, t.mod = p.mod, t.nof_layers = (uint8_t)L, t.Nref = p.tbs_lbrm_bytes * 8, t.nof_ch_symbols = nre * L, t.tb_bytes = p.tb_bytes;
  t.tb_offset = p.tb_offset, t.codeword_offset = cw_bytes;
  d = {};
  d.slot_in_frame = p.slot_in_frame, d.reference_point_k_rb = p.ref_point_prb0 ? p.bwp_start_rb : 0, d.scrambling_id = p.dmrs_scrambling_id;
  d.amplitude = powf(10.0f, -p.ratio_pdsch_dmrs_to_sss_dB / 20.0f);
  d.dmrs_type = 1, d.n_scid = p.n_scid, d.nof_ports = (uint8_t)L, d.symbols_mask = p.dmrs_symbols_mask, d.grid_nof_prb = p.grid_nof_prb;
  for (unsigned ly = 0; ly < L; ++ly)
    d.ports[ly] = ports ? ports[ly] : p.port;
  for (int k = 0; k < 5; ++k)
    d.rb_mask[k] = p.rb_mask[k];
  d.grid_offset = p.grid_offset;
  cw_bytes += ((size_t)m.nof_bits + 15u) & ~(size_t)15u;
  return MIPHY_OK;
}

// The one-layer forms: every PDU of the batch on one layer, on its own port.
int derive_one_layer_jobs(const miphy_pdsch_pdu* pdus, uint32_t n, std::vector<miphy_pdsch_tb_desc>& tb, std::vector<miphy_pdsch_mod_job>& mj,
                          std::vector<miphy_dmrs_pdsch_job>& dj, size_t& cw_bytes)
{
  tb.resize(n), mj.resize(n), dj.resize(n);
  cw_bytes = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (int rc = derive_pdsch_jobs("pdsch_process", i, pdus[i], 1, nullptr, tb[i], mj[i], dj[i], cw_bytes))
      return rc;
  return MIPHY_OK;
}

// The tail of every processor: the codewords (one bit per byte) in a workspace of the context, the encoder, then the form's modulator on the codewords
// and its DM-RS mapper.
template <class MOD, class DMRS>
int pdsch_process_tail(miphy_ctx* ctx, const std::vector<miphy_pdsch_tb_desc>& tb, size_t cw_bytes, const uint8_t* tb_in, hipStream_t s, MOD&& modulate, DMRS&& map_dmrs)
{
  void* work = nullptr;
  int   rc   = miphy_get_workspace(ctx, MIPHY_WS_OUTPUT, cw_bytes + 64, &work);
  if (rc)
    return rc;
  uint8_t* d_cw = static_cast<uint8_t*>(work);
  if ((rc = miphy_pdsch_encode_batch(ctx, tb.data(), (uint32_t)tb.size(), tb_in, d_cw, s)) || (rc = modulate(d_cw)))
    return rc;
  return map_dmrs();
}
} // namespace

extern "C" int miphy_pdsch_process_batch(miphy_ctx* ctx, const miphy_pdsch_pdu* pdus, uint32_t n, const uint8_t* tb_in, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && tb_in && grid, "miphy_pdsch_process_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  hipStream_t                       s = (hipStream_t)stream;
  std::vector<miphy_pdsch_tb_desc>  tb;
  std::vector<miphy_pdsch_mod_job>  mj;
  std::vector<miphy_dmrs_pdsch_job> dj;
  size_t                            cw_bytes = 0;
  int                               rc = derive_one_layer_jobs(pdus, n, tb, mj, dj, cw_bytes);
  if (rc)
    return rc;
  return pdsch_process_tail(
      ctx, tb, cw_bytes, tb_in, s, [&](const uint8_t* cw) { return miphy_pdsch_modulate_batch(ctx, mj.data(), 0, n, cw, grid, s); },
      [&] { return miphy_dmrs_pdsch_map_batch(ctx, dj.data(), 0, n, grid, s); });
}

// ---- one codeword on 1..4 layers, in three forms (and, further down, one or two on 1..8 layers through the same composition): layers on named grid ports, the same with the PRBs in the mapping order of a list (interleaved
// VRB-to-PRB mapping), the same behind a precoding. One composition: the encoder's nof_layers = L and nof_ch_symbols = REs x L, the layered modulator
// of the form, the DM-RS on L ports.
extern "C" uint32_t miphy_pdsch_layers_pdu_nof_re(const miphy_pdsch_layers_pdu* pdu)
{
  if (!pdu || pdu->nof_layers < 1 || pdu->nof_layers > 4)
    return 0;
  return miphy_pdsch_pdu_nof_re(&pdu->base);
}

namespace {
// The arrays of a layered call next to its PDUs: null / 0 where the form has none.
struct pdsch_pdu_arrays {
  const uint16_t* prb_lists;
  uint32_t        nof_list_entries;
  const float*    weights;
  uint32_t        nof_weights;
};

// derive_pdsch_jobs for PDU i of a layered batch, with the layered modulator job and the encoder's limits: what every layered processor asks of a PDU.
// max_layers: the largest nof_layers so far.
int derive_layers_jobs(const char* who, uint32_t i, const miphy_pdsch_layers_pdu& p, const pdsch_pdu_arrays&, miphy_pdsch_tb_desc& t, miphy_pdsch_mod_layers_job& lj,
                       miphy_dmrs_pdsch_job& d, size_t& cw_bytes, uint32_t& max_layers)
{
  const uint32_t L = p.nof_layers;
  lj               = {};
  if (int rc = derive_pdsch_jobs(who, i, p.base, L, p.ports, t, lj.base, d, cw_bytes))
    return rc;
  lj.nof_layers = (uint8_t)L;
  for (uint32_t ly = 0; ly < 4; ++ly)
    lj.ports[ly] = p.ports[ly];
  max_layers = L > max_layers ? L : max_layers;
  // what the encoder accepts (sch.hip, ldpc_segmenter_impl.cpp:104-141): at most 52 codeblocks, none of them empty
  const uint32_t nre = t.nof_ch_symbols / L; // REs per layer
  const uint64_t tbs = (uint64_t)p.base.tb_bytes * 8, B = tbs + (tbs <= 3824 ? 16 : 24), Kcb = p.base.bg == 1 ? 8448 : 3840;
  const uint64_t ncb = B <= Kcb ? 1 : (B + Kcb - 24 - 1) / (Kcb - 24);
  MIPHY_REQUIRE(p.base.tb_bytes > 0 && ncb <= 52, "%s: PDU %u: transport block of %u bytes outside what the encoder accepts (1 .. %u bytes on base graph %u)", who, i,
                p.base.tb_bytes, p.base.bg == 1 ? 54753u : 24801u, (unsigned)p.base.bg);
  MIPHY_REQUIRE(p.base.rv <= 3, "%s: PDU %u: invalid redundancy version", who, i);
  MIPHY_REQUIRE(nre >= ncb, "%s: PDU %u: %u REs per layer cannot carry %u codeblocks", who, i, nre, (unsigned)ncb);
  return MIPHY_OK;
}

// The same for a mapped PDU: the records of its layers, then its list under the list rules. The DM-RS job takes rb_mask, as derive_pdsch_jobs fills it:
// the DM-RS does not depend on the mapping order.
int derive_layers_jobs(const char* who, uint32_t i, const miphy_pdsch_mapped_pdu& p, const pdsch_pdu_arrays& a, miphy_pdsch_tb_desc& t, miphy_pdsch_mod_mapped_job& mj,
                       miphy_dmrs_pdsch_job& d, size_t& cw_bytes, uint32_t& max_layers)
{
  if (int rc = derive_layers_jobs(who, i, p.layers, a, t, mj.layers, d, cw_bytes, max_layers))
    return rc;
  mj.prb_list_offset = p.prb_list_offset, mj.nof_prb = p.nof_prb;
  return miphy_pdsch_mod_list_check(who, "PDU", i, mj, a.prb_lists, a.nof_list_entries);
}

// The same for a precoded PDU: the records of the mapped PDU, then the same matrices for the data and its DM-RS under the precoding rules. The layers'
// ports are not used (antenna port a is grid port precoding.ports[a]): the PDU's rules are checked with the layers on ports 0 .. L - 1.
int derive_layers_jobs(const char* who, uint32_t i, const miphy_pdsch_precoded_pdu& p, const pdsch_pdu_arrays& a, miphy_pdsch_tb_desc& t,
                       miphy_pdsch_mod_precoded_job& mj, miphy_dmrs_pdsch_precoded_job& dj, size_t& cw_bytes, uint32_t& max_layers)
{
  miphy_pdsch_mapped_pdu mp = p.mapped;
  for (uint8_t ly = 0; ly < 4; ++ly)
    mp.layers.ports[ly] = ly;
  if (int rc = derive_layers_jobs(who, i, mp, a, t, mj.mapped, dj.base, cw_bytes, max_layers))
    return rc;
  mj.precoding = dj.precoding = p.precoding;
  return miphy_dmrs_pdsch_precoded_job_check(who, "PDU", i, dj, a.nof_weights);
}

// The same for a PDU of one or two transport blocks on 1..8 layers. Up to four layers it is the mapped PDU it contains, on nof_layers and ports of its own:
// the same records, the same refusals. From five, transport block q goes through the records of a layered PDU on its own L_q layers and its slice of the
// ports -- so every rule of a transport block, the encoder's limits among them, holds for each -- and leaves the encoder's record of block 1 in `second`;
// the modulator job carries both codewords and the DM-RS job all L ports. DM-RS ports 1004 .. 1007 of type 1 exist only on a double-symbol DM-RS with two
// CDM groups, hence the two rules of their own.
int derive_layers_jobs(const char* who, uint32_t i, const miphy_pdsch_codewords_pdu& p, const pdsch_pdu_arrays& a, miphy_pdsch_tb_desc& t,
                       miphy_pdsch_mod_codewords_job& cj, miphy_dmrs_pdsch_job& d, size_t& cw_bytes, uint32_t& max_layers, std::vector<miphy_pdsch_tb_desc>& second)
{
  const uint32_t L = p.nof_layers;
  cj               = {};
  cj.nof_layers    = (uint8_t)L;
  for (uint32_t ly = 0; ly < 8; ++ly)
    cj.ports[ly] = p.ports[ly];
  if (L <= 4) {
    miphy_pdsch_mapped_pdu mp = p.mapped;
    mp.layers.nof_layers      = (uint8_t)L;
    for (uint32_t ly = 0; ly < 4; ++ly)
      mp.layers.ports[ly] = p.ports[ly];
    return derive_layers_jobs(who, i, mp, a, t, cj.mapped, d, cw_bytes, max_layers);
  }
  MIPHY_REQUIRE(L <= 8, "%s: PDU %u: invalid number of layers %u (1..4: one transport block, 5..8: two)", who, i, L);
  const miphy_pdsch_pdu& b = p.mapped.layers.base;
  MIPHY_REQUIRE(b.nof_cdm_groups_without_data == 2, "%s: PDU %u: %u layers need 2 CDM groups without data", who, i, L);
  const uint32_t m = b.dmrs_symbols_mask, first = m & ~(m << 1), last = m & ~(m >> 1); // the first and the last symbol of every run
  MIPHY_REQUIRE((first << 1) == last, "%s: PDU %u: %u layers need a double-symbol DM-RS (every DM-RS symbol in a run of exactly two)", who, i, L);
  const uint32_t         L0 = L / 2, L1 = L - L0;
  miphy_pdsch_layers_pdu lp = p.mapped.layers;
  lp.nof_layers             = (uint8_t)L0;
  for (uint32_t ly = 0; ly < 4; ++ly)
    lp.ports[ly] = p.ports[ly];
  if (int rc = derive_layers_jobs(who, i, lp, a, t, cj.mapped.layers, d, cw_bytes, max_layers))
    return rc;
  lp.nof_layers = (uint8_t)L1;
  for (uint32_t ly = 0; ly < 4; ++ly)
    lp.ports[ly] = p.ports[ly + L0 < 8 ? ly + L0 : 7];
  lp.base.bg = p.bg1, lp.base.rv = p.rv1, lp.base.mod = p.mod1, lp.base.tb_bytes = p.tb_bytes1, lp.base.tb_offset = p.tb_offset1;
  miphy_pdsch_tb_desc        t1;
  miphy_pdsch_mod_layers_job lj1;
  miphy_dmrs_pdsch_job       d1;
  if (int rc = derive_layers_jobs(who, i, lp, a, t1, lj1, d1, cw_bytes, max_layers))
    return rc;
  second.push_back(t1);
  cj.mapped.prb_list_offset = p.mapped.prb_list_offset, cj.mapped.nof_prb = p.mapped.nof_prb;
  cj.mod1 = p.mod1, cj.nof_bits1 = lj1.base.nof_bits, cj.cw1_offset = lj1.base.cw_offset;
  d.nof_ports = (uint8_t)L;
  for (uint32_t ly = 0; ly < L; ++ly)
    d.ports[ly] = p.ports[ly];
  return miphy_pdsch_mod_codewords_check(who, "PDU", i, cj, a.prb_lists, a.nof_list_entries, t.nof_ch_symbols / L0);
}

// A layered processor behind its null-argument test: the records of every PDU (MJ: the modulator job of the form, DJ: its DM-RS job), refused before
// anything is enqueued or allocated, then the tail. map_dmrs(jobs, stream): the DM-RS mapper of the form. The encoder runs over all transport blocks of the
// batch: one per PDU and, behind them, the second blocks of the PDUs that have two.
template <class MJ, class DJ, class PDU, class DMRS>
int pdsch_process_layered(const char* who, miphy_ctx* ctx, const PDU* pdus, uint32_t n, const pdsch_pdu_arrays& a, const uint8_t* tb_in, float* grid, void* stream,
                          DMRS&& map_dmrs)
{
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "%s: at most 65535 PDUs per call", who);
  hipStream_t                      s = (hipStream_t)stream;
  std::vector<miphy_pdsch_tb_desc> tb(n);
  std::vector<MJ>                  mj(n);
  std::vector<DJ>                  dj(n);
  size_t                           cw_bytes   = 0;
  uint32_t                         max_layers = 1;
  std::vector<miphy_pdsch_tb_desc> second;
  for (uint32_t i = 0; i < n; ++i) {
    int rc;
    if constexpr (std::is_same<PDU, miphy_pdsch_codewords_pdu>::value)
      rc = derive_layers_jobs(who, i, pdus[i], a, tb[i], mj[i], dj[i], cw_bytes, max_layers, second);
    else
      rc = derive_layers_jobs(who, i, pdus[i], a, tb[i], mj[i], dj[i], cw_bytes, max_layers);
    if (rc)
      return rc;
  }
  tb.insert(tb.end(), second.begin(), second.end());
  return pdsch_process_tail(
      ctx, tb, cw_bytes, tb_in, s,
      [&](const uint8_t* cw) { // (the jobs passed the modulator's host rules in derive_layers_jobs)
        return miphy_pdsch_modulate_layered_enqueue(ctx, mj.data(), 0, n, max_layers, a.prb_lists, a.nof_list_entries, a.weights, a.nof_weights, cw, grid, s);
      },
      [&] { return map_dmrs(dj.data(), s); });
}
} // namespace

extern "C" int miphy_pdsch_process_layers_batch(miphy_ctx* ctx, const miphy_pdsch_layers_pdu* pdus, uint32_t n, const uint8_t* tb_in, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && tb_in && grid, "miphy_pdsch_process_layers_batch: null argument");
  return pdsch_process_layered<miphy_pdsch_mod_layers_job, miphy_dmrs_pdsch_job>(
      "pdsch_process_layers", ctx, pdus, n, {nullptr, 0, nullptr, 0}, tb_in, grid, stream,
      [&](const miphy_dmrs_pdsch_job* dj, hipStream_t s) { return miphy_dmrs_pdsch_map_batch(ctx, dj, 0, n, grid, s); });
}

extern "C" int miphy_pdsch_process_mapped_batch(miphy_ctx* ctx, const miphy_pdsch_mapped_pdu* pdus, uint32_t n, const uint16_t* prb_lists,
                                                uint32_t nof_list_entries, const uint8_t* tb_in, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && tb_in && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_process_mapped_batch: null argument");
  return pdsch_process_layered<miphy_pdsch_mod_mapped_job, miphy_dmrs_pdsch_job>(
      "pdsch_process_mapped", ctx, pdus, n, {prb_lists, nof_list_entries, nullptr, 0}, tb_in, grid, stream,
      [&](const miphy_dmrs_pdsch_job* dj, hipStream_t s) { return miphy_dmrs_pdsch_map_batch(ctx, dj, 0, n, grid, s); });
}

extern "C" int miphy_pdsch_process_precoded_batch(miphy_ctx* ctx, const miphy_pdsch_precoded_pdu* pdus, uint32_t n, const uint16_t* prb_lists,
                                                  uint32_t nof_list_entries, const float* weights, uint32_t nof_weights, const uint8_t* tb_in, float* grid,
                                                  void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && weights && tb_in && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_process_precoded_batch: null argument");
  return pdsch_process_layered<miphy_pdsch_mod_precoded_job, miphy_dmrs_pdsch_precoded_job>(
      "pdsch_process_precoded", ctx, pdus, n, {prb_lists, nof_list_entries, weights, nof_weights}, tb_in, grid, stream,
      [&](const miphy_dmrs_pdsch_precoded_job* dj, hipStream_t s) { return miphy_dmrs_pdsch_map_precoded_batch(ctx, dj, 0, n, weights, nof_weights, grid, s); });
}

// ---- one or two transport blocks on 1..8 layers
extern "C" uint32_t miphy_pdsch_codewords_pdu_nof_re(const miphy_pdsch_codewords_pdu* pdu)
{
  if (!pdu || pdu->nof_layers < 1 || pdu->nof_layers > 8)
    return 0;
  return miphy_pdsch_pdu_nof_re(&pdu->mapped.layers.base);
}

extern "C" int miphy_pdsch_process_codewords_batch(miphy_ctx* ctx, const miphy_pdsch_codewords_pdu* pdus, uint32_t n, const uint16_t* prb_lists,
                                                   uint32_t nof_list_entries, const uint8_t* tb_in, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && tb_in && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_process_codewords_batch: null argument");
  return pdsch_process_layered<miphy_pdsch_mod_codewords_job, miphy_dmrs_pdsch_job>(
      "pdsch_process_codewords", ctx, pdus, n, {prb_lists, nof_list_entries, nullptr, 0}, tb_in, grid, stream,
      [&](const miphy_dmrs_pdsch_job* dj, hipStream_t s) { return miphy_dmrs_pdsch_map_batch(ctx, dj, 0, n, grid, s); });
}

// ---- prepared form: PDU validation, segmentation, every descriptor upload and the scratch happen once; a run is the seven launches of the
// chain, nothing staged or allocated, no host synchronisation -- for allocations that repeat slot after slot (and for batches whose descriptors exceed the staging ring,
// where the per-call form has to wait for its upload).
struct miphy_pdsch_process_plan {
  miphy_ctx*                      ctx = nullptr;
  uint32_t                        n   = 0;
  miphy_pdsch_encode_prepared*    enc = nullptr;
  const gold_tables*              gt  = nullptr;
  miphy_device_block              buf; // [modulator jobs | DM-RS jobs | codewords | the modulator's sequences and prefixes]
  image_slot<miphy_pdsch_mod_job>  mj;
  image_slot<miphy_dmrs_pdsch_job> dj;
  image_slot<uint8_t>              cw, seq;
  ~miphy_pdsch_process_plan() { miphy_pdsch_encode_prepared_destroy(enc); }
};

extern "C" int miphy_pdsch_process_plan_create(miphy_ctx* ctx, const miphy_pdsch_pdu* pdus, uint32_t n, miphy_pdsch_process_plan** out)
{
  MIPHY_REQUIRE(ctx && pdus && out && n > 0, "miphy_pdsch_process_plan_create: null argument or empty batch");
  MIPHY_REQUIRE(n <= 65535, "pdsch_process: at most 65535 PDUs per plan");
  std::vector<miphy_pdsch_tb_desc>  tb;
  std::vector<miphy_pdsch_mod_job>  mj;
  std::vector<miphy_dmrs_pdsch_job> dj;
  size_t                            cw_bytes = 0;
  int                               rc = derive_one_layer_jobs(pdus, n, tb, mj, dj, cw_bytes);
  if (rc)
    return rc;
  std::unique_ptr<miphy_pdsch_process_plan> p(new miphy_pdsch_process_plan());
  p->ctx = ctx, p->n = n;
  if ((rc = miphy_get_gold_tables(ctx, &p->gt)) || (rc = miphy_pdsch_encode_prepare(ctx, tb.data(), n, &p->enc)))
    return rc;
  device_image img;
  p->mj  = img.put(mj);
  p->dj  = img.put(dj);
  p->cw  = img.reserve<uint8_t>(cw_bytes + 64);
  p->seq = img.reserve<uint8_t>(miphy_pdsch_modulate_scratch_bytes(n), 256);
  if ((rc = miphy_image_to_block("miphy_pdsch_process_plan_create", img, p->buf)))
    return rc;
  *out = p.release();
  return MIPHY_OK;
}

extern "C" int miphy_pdsch_process_plan_run(miphy_pdsch_process_plan* p, const uint8_t* tb_in, float* grid, void* stream)
{
  MIPHY_REQUIRE(p && tb_in && grid, "miphy_pdsch_process_plan_run: null argument");
  hipStream_t s = (hipStream_t)stream;
  int         rc;
  void*       buf = p->buf.get();
  uint8_t*    cw  = p->cw.at(buf);
  if ((rc = miphy_pdsch_encode_prepared_run(p->enc, tb_in, cw, s)))
    return rc;
  if ((rc = miphy_pdsch_modulate_launch(p->mj.at(buf), p->n, p->gt, cw, grid, p->seq.at(buf), s)))
    return rc;
  return miphy_dmrs_pdsch_map_launch(p->dj.at(buf), p->n, p->gt, grid, s);
}

extern "C" void miphy_pdsch_process_plan_destroy(miphy_pdsch_process_plan* p)
{
  delete p;
}
