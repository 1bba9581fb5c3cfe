// Fixture driver for tests/golden/pucch_processor.npz: runs the reference's PUCCH processor, obtained through its public factory
// (create_pucch_processor_factory_sw), on resource grids read from stdin and writes its results to stdout. The format-2 soft bits, which
// the processor keeps to itself, come from the reference's own format-2 DM-RS estimator and PUCCH demodulator driven exactly as
// pucch_processor_impl::process drives them. Built and run by tools/gen_pucch_golden.py against the reference library that build()
// compiles into oracle/_ref/. The reference's DFT factory translation unit needs FFTW, so the driver hands out the generic DFT itself.
//
// stdin:  uint32 n, then n records {int32 hdr[21], float grid[nports][14][grid_nprb * 12][2]}
//         hdr: format, numerology, slot, nports, start_symbol, nof_symbols, bwp_start, bwp_size, starting_prb, hopping,
//              second_hop_prb, nof_prb, n_id, n_id_0, rnti, initial_cyclic_shift, time_domain_occ, nof_harq_ack, nof_sr,
//              nof_csi_part1, grid_nprb
// stdout: float low_papr[30][12][12][2] (u, alpha index, n; v = 0), then n records
//         {uint8 status, uint8 nbits, uint8 payload[nbits], float metric, epre_dB, rsrp_dB, sinr_dB, time_alignment_s,
//          uint32 nllr, int8 llr[nllr]}
#include "srsran/phy/generic_functions/generic_functions_factories.h"
#include "srsran/phy/support/support_factories.h"
#include "srsran/phy/upper/channel_modulation/channel_modulation_factories.h"
#include "srsran/phy/upper/channel_coding/channel_coding_factories.h"
#include "srsran/phy/upper/channel_processors/channel_processor_factories.h"
#include "srsran/phy/upper/equalization/equalization_factories.h"
#include "srsran/phy/upper/sequence_generators/sequence_generator_factories.h"
#include "srsran/phy/upper/signal_processors/signal_processor_factories.h"
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace srsran;

namespace {

class generic_dft_factory : public dft_processor_factory
{
public:
  std::unique_ptr<dft_processor> create(const dft_processor::configuration& config) override
  {
    auto p = std::make_unique<dft_processor_generic_impl>(config);
    if (!p->is_valid()) {
      return nullptr;
    }
    return p;
  }
};

void read_exact(void* p, size_t n)
{
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "gen_pucch_golden: short read\n");
    std::exit(1);
  }
}

template <typename T>
void put(const T& v)
{
  fwrite(&v, sizeof(T), 1, stdout);
}

} // namespace

int main()
{
  channel_estimate::channel_estimate_dimensions dims;
  dims.nof_prb       = 275;
  dims.nof_symbols   = 14;
  dims.nof_rx_ports  = 4;
  dims.nof_tx_layers = 1;

  auto prg_f   = create_pseudo_random_generator_sw_factory();
  auto lpg_f   = create_low_papr_sequence_generator_sw_factory();
  auto lpc_f   = create_low_papr_sequence_collection_sw_factory(lpg_f);
  auto eq_f    = create_channel_equalizer_factory_zf();
  auto port_f  = create_port_channel_estimator_factory_sw(std::make_shared<generic_dft_factory>());
  auto dmrs_f  = create_dmrs_pucch_estimator_factory_sw(prg_f, lpc_f, port_f);
  auto det_f   = create_pucch_detector_factory_sw(lpc_f, prg_f, eq_f);
  auto demod_f = create_pucch_demodulator_factory_sw(eq_f, create_channel_modulation_sw_factory(), prg_f);
  uci_decoder_factory_sw_configuration dec_cfg;
  dec_cfg.decoder_factory = create_short_block_detector_factory_sw();
  auto proc_f             = create_pucch_processor_factory_sw(dmrs_f, det_f, demod_f, create_uci_decoder_factory_sw(dec_cfg), dims);
  auto processor          = proc_f->create();
  auto est_f2             = dmrs_f->create_format2();
  auto demod              = demod_f->create();

  // The detector's table: 12 cyclic shifts alpha = 2 pi k / 12 of the length-12 base sequences.
  std::array<float, NRE> alphas = {};
  for (unsigned k = 0; k != NRE; ++k) {
    alphas[k] = TWOPI * static_cast<float>(k) / static_cast<float>(NRE);
  }
  auto lpc = lpc_f->create(1, 0, alphas);
  for (unsigned u = 0; u != 30; ++u) {
    for (unsigned a = 0; a != NRE; ++a) {
      span<const cf_t> r = lpc->get(u, 0, a);
      fwrite(r.data(), sizeof(cf_t), NRE, stdout);
    }
  }

  uint32_t n = 0;
  read_exact(&n, sizeof(n));
  std::vector<cf_t> buf;
  for (uint32_t i = 0; i != n; ++i) {
    int32_t h[21];
    read_exact(h, sizeof(h));
    const unsigned fmt = h[0], nports = h[3], grid_nprb = h[20];
    buf.resize(size_t(nports) * 14 * grid_nprb * NRE);
    read_exact(buf.data(), buf.size() * sizeof(cf_t));
    auto grid = create_resource_grid(nports, 14, grid_nprb * NRE);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid->put(p, l, 0, span<const cf_t>(buf.data() + (size_t(p) * 14 + l) * grid_nprb * NRE, grid_nprb * NRE));
      }
    }
    static_vector<uint8_t, MAX_PORTS> ports;
    for (unsigned p = 0; p != nports; ++p) {
      ports.push_back(p);
    }
    const slot_point slot(h[1], h[2]);

    pucch_processor_result res;
    std::vector<log_likelihood_ratio> llr;
    if (fmt == 1) {
      pucch_processor::format1_configuration c;
      c.slot         = slot;
      c.bwp_size_rb  = h[7];
      c.bwp_start_rb = h[6];
      c.cp           = cyclic_prefix::NORMAL;
      c.starting_prb = h[8];
      if (h[9]) {
        c.second_hop_prb.emplace(h[10]);
      }
      c.n_id                 = h[12];
      c.nof_harq_ack         = h[17];
      c.ports                = ports;
      c.initial_cyclic_shift = h[15];
      c.nof_symbols          = h[5];
      c.start_symbol_index   = h[4];
      c.time_domain_occ      = h[16];
      // A detector of its own per PDU: the reference's detector averages over its whole work buffer (get_data() of its tensors is
      // their capacity, pucch_detector_impl.cpp:397-402), so a shared one carries the equalised symbols of earlier, longer PDUs into
      // the metric of a shorter one. A fresh detector holds zeros there, which leave the metric as the PDU's own.
      res = proc_f->create()->process(*grid, c);
    } else {
      pucch_processor::format2_configuration c;
      c.slot               = slot;
      c.cp                 = cyclic_prefix::NORMAL;
      c.ports              = ports;
      c.bwp_size_rb        = h[7];
      c.bwp_start_rb       = h[6];
      c.starting_prb       = h[8];
      c.nof_prb            = h[11];
      c.start_symbol_index = h[4];
      c.nof_symbols        = h[5];
      c.rnti               = h[14];
      c.n_id               = h[12];
      c.n_id_0             = h[13];
      c.nof_harq_ack       = h[17];
      c.nof_sr             = h[18];
      c.nof_csi_part1      = h[19];
      c.nof_csi_part2      = 0;
      res                  = processor->process(*grid, c);

      // The soft bits, as pucch_processor_impl::process(format2) computes them.
      dmrs_pucch_processor::config_t ec = {};
      ec.format             = pucch_format::FORMAT_2;
      ec.slot               = slot;
      ec.cp                 = cyclic_prefix::NORMAL;
      ec.start_symbol_index = c.start_symbol_index;
      ec.nof_symbols        = c.nof_symbols;
      ec.starting_prb       = c.bwp_start_rb + c.starting_prb;
      ec.nof_prb            = c.nof_prb;
      ec.n_id               = c.n_id;
      ec.n_id_0             = c.n_id_0;
      ec.ports.assign(ports.begin(), ports.end());
      channel_estimate::channel_estimate_dimensions d = dims;
      d.nof_prb                                       = c.bwp_start_rb + c.bwp_size_rb;
      d.nof_rx_ports                                  = nports;
      channel_estimate ce(d);
      est_f2->estimate(ce, *grid, ec);
      llr.resize(8 * c.nof_prb * c.nof_symbols * 2);
      pucch_demodulator::format2_configuration dc = {};
      dc.rx_ports                                 = ports;
      dc.first_prb                                = c.bwp_start_rb + c.starting_prb;
      dc.nof_prb                                  = c.nof_prb;
      dc.start_symbol_index                       = c.start_symbol_index;
      dc.nof_symbols                              = c.nof_symbols;
      dc.rnti                                     = c.rnti;
      dc.n_id                                     = c.n_id;
      demod->demodulate(llr, *grid, ce, dc);
    }

    span<const uint8_t> payload = res.message.get_full_payload();
    put<uint8_t>(static_cast<uint8_t>(res.message.get_status()));
    put<uint8_t>(static_cast<uint8_t>(payload.size()));
    fwrite(payload.data(), 1, payload.size(), stdout);
    put<float>(res.detection_metric.has_value() ? res.detection_metric.value() : 0.0F);
    put<float>(res.csi.epre_dB);
    put<float>(res.csi.rsrp_dB);
    put<float>(res.csi.sinr_dB);
    put<float>(res.csi.time_alignment.to_seconds<float>());
    put<uint32_t>(static_cast<uint32_t>(llr.size()));
    for (log_likelihood_ratio l : llr) {
      put<int8_t>(l.to_value_type());
    }
  }
  return 0;
}
