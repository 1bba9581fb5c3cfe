// Fixture driver for tests/golden/prach_demod.npz: runs the reference's OFDM PRACH demodulator, obtained through its public factory
// (create_ofdm_prach_demodulator_factory_sw over the generic DFT), on windows of baseband samples read from stdin and writes the
// complete content of the PRACH buffer it filled to stdout. The buffer is a prach_buffer_impl one row larger than the configuration
// needs in every dimension and pre-filled with a sentinel: the driver fails if a sentinel is left in the region the configuration
// covers or if a row outside it changed. Built and run by tools/gen_prach_demod_golden.py against the reference library that build()
// compiles into oracle/_ref/. The reference's DFT factory translation unit needs FFTW, so the driver hands out the generic DFT itself;
// the demodulator wants a DFT for every RA subcarrier spacing, also those whose size the generic DFT lacks (64 points at 7.68 MHz /
// 120 kHz), and gets a placeholder for them that no case runs.
//
// stdin:  uint32 n, then n records {uint32 sampling_rate_hz, format, pusch_scs, nof_td_occasions, nof_fd_occasions, start_symbol,
//                                   rb_offset, nof_prb_ul_grid, nof_samples, float samples[nof_samples][2]}
// stdout: n records {uint32 nof_td_occasions, nof_fd_occasions, nof_symbols, L, float buffer[td][fd][symbol][L][2]}
// --time: mean time of demodulate() per window, one thread, for format 0 (1 and 4 frequency-domain occasions) and B4 at 30.72 MHz.
#include "srsran/phy/lower/modulation/modulation_factories.h"
#include "srsran/ran/prach/prach_preamble_information.h"
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/prach_buffer_impl.h"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace srsran;

namespace {

const cf_t SENTINEL(12345.f, -54321.f);

class placeholder_dft : public dft_processor
{
  configuration     cfg;
  std::vector<cf_t> data;

public:
  explicit placeholder_dft(const configuration& c) : cfg(c), data(c.size) {}
  direction        get_direction() const override { return cfg.dir; }
  unsigned         get_size() const override { return cfg.size; }
  span<cf_t>       get_input() override { return data; }
  span<const cf_t> run() override
  {
    fprintf(stderr, "gen_prach_demod_golden: a case ran the placeholder DFT of size %u\n", cfg.size);
    std::exit(1);
  }
};

class generic_dft_factory : public dft_processor_factory
{
public:
  std::unique_ptr<dft_processor> create(const dft_processor::configuration& config) override
  {
    auto p = std::make_unique<dft_processor_generic_impl>(config);
    if (!p->is_valid()) {
      return std::make_unique<placeholder_dft>(config);
    }
    return p;
  }
};

void read_exact(void* p, size_t n)
{
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "gen_prach_demod_golden: short read\n");
    std::exit(1);
  }
}

prach_preamble_information info_of(prach_format_type format, subcarrier_spacing pusch_scs)
{
  return is_long_preamble(format) ? get_prach_preamble_long_info(format)
                                  : get_prach_preamble_short_info(format, to_ra_subcarrier_spacing(pusch_scs), false);
}

int time_mode()
{
  const sampling_rate             srate = sampling_rate::from_MHz(30.72);
  auto                            demod = create_ofdm_prach_demodulator_factory_sw(std::make_shared<generic_dft_factory>(), srate)->create();
  std::mt19937                    rng(1);
  std::normal_distribution<float> gauss(0.f, 1.f);
  for (int pass = 0; pass != 3; ++pass) {
    ofdm_prach_demodulator::configuration c = {};
    c.format           = pass == 2 ? prach_format_type::B4 : prach_format_type::zero;
    c.nof_td_occasions = 1;
    c.nof_fd_occasions = pass == 1 ? 4 : 1;
    c.start_symbol     = 0;
    c.rb_offset        = 0;
    c.nof_prb_ul_grid  = pass == 2 ? 51 : 106;
    c.pusch_scs        = pass == 2 ? subcarrier_spacing::kHz30 : subcarrier_spacing::kHz15;
    const prach_preamble_information info = info_of(c.format, c.pusch_scs);
    const unsigned nsym = info.symbol_length.to_samples(ra_scs_to_Hz(info.scs));
    prach_buffer_impl buf(1, 1, c.nof_fd_occasions, nsym, info.sequence_length);
    const unsigned    window = get_prach_window_duration(c.format, c.pusch_scs, c.start_symbol, c.nof_td_occasions).to_samples(srate.to_Hz());
    std::vector<cf_t> x(window);
    for (cf_t& v : x) {
      v = cf_t(gauss(rng), gauss(rng));
    }
    for (int i = 0; i != 5; ++i) {
      demod->demodulate(buf, x, c);
    }
    const int reps = 50;
    auto      t0   = std::chrono::steady_clock::now();
    for (int i = 0; i != reps; ++i) {
      demod->demodulate(buf, x, c);
    }
    auto t1 = std::chrono::steady_clock::now();
    printf("reference ofdm_prach_demodulator_impl, 30.72 MHz, format %s, %u frequency-domain occasion(s), one thread: %.1f us per window (%g)\n",
           pass == 2 ? "B4 at 30 kHz" : "0", c.nof_fd_occasions, std::chrono::duration<double, std::micro>(t1 - t0).count() / reps,
           (double)buf.get_symbol(0, 0, 0, 0)[0].real());
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc > 1 && !strcmp(argv[1], "--time")) {
    return time_mode();
  }
  uint32_t n = 0;
  read_exact(&n, sizeof(n));
  auto dft_f = std::make_shared<generic_dft_factory>();
  for (uint32_t i = 0; i != n; ++i) {
    uint32_t h[9];
    read_exact(h, sizeof(h));
    std::vector<cf_t> x(h[8]);
    read_exact(x.data(), x.size() * sizeof(cf_t));

    const sampling_rate                   srate = sampling_rate::from_Hz(h[0]);
    ofdm_prach_demodulator::configuration c     = {};
    c.format                                    = static_cast<prach_format_type>(h[1]);
    c.pusch_scs                                 = static_cast<subcarrier_spacing>(h[2]);
    c.nof_td_occasions                          = h[3];
    c.nof_fd_occasions                          = h[4];
    c.start_symbol                              = h[5];
    c.rb_offset                                 = h[6];
    c.nof_prb_ul_grid                           = h[7];
    const prach_preamble_information info = info_of(c.format, c.pusch_scs);
    const unsigned                   L = info.sequence_length, nsym = info.symbol_length.to_samples(ra_scs_to_Hz(info.scs));
    const unsigned                   ntd = c.nof_td_occasions, nfd = c.nof_fd_occasions;

    prach_buffer_impl buf(1, ntd + 1, nfd + 1, nsym + 1, L);
    for (unsigned td = 0; td != ntd + 1; ++td) {
      for (unsigned fd = 0; fd != nfd + 1; ++fd) {
        for (unsigned s = 0; s != nsym + 1; ++s) {
          for (cf_t& v : buf.get_symbol(0, td, fd, s)) {
            v = SENTINEL;
          }
        }
      }
    }
    // A fresh demodulator per case, so that no case sees what an earlier one left in a DFT input.
    create_ofdm_prach_demodulator_factory_sw(dft_f, srate)->create()->demodulate(buf, x, c);

    const uint32_t dims[4] = {ntd, nfd, nsym, L};
    fwrite(dims, sizeof(dims), 1, stdout);
    for (unsigned td = 0; td != ntd + 1; ++td) {
      for (unsigned fd = 0; fd != nfd + 1; ++fd) {
        for (unsigned s = 0; s != nsym + 1; ++s) {
          const bool       inside = td < ntd && fd < nfd && s < nsym;
          span<const cf_t> row    = buf.get_symbol(0, td, fd, s);
          for (const cf_t& v : row) {
            if ((v == SENTINEL) == inside) {
              fprintf(stderr, "gen_prach_demod_golden: case %u: row (%u, %u, %u) %s\n", i, td, fd, s,
                      inside ? "keeps a sentinel" : "was written outside the configuration");
              return 1;
            }
          }
          if (inside) {
            fwrite(row.data(), sizeof(cf_t), row.size(), stdout);
          }
        }
      }
    }
  }
  return 0;
}
