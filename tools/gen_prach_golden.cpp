// Fixture driver for tests/golden/prach_detector.npz: runs the reference's PRACH detector, obtained through its public factory
// (create_prach_detector_factory_simple over create_prach_generator_factory_sw and the generic IDFT of size 1536, the wiring of
// upper_phy_factories.cpp), on frequency-domain symbols read from stdin and writes its results to stdout. detect() returns only the
// preambles that survive the threshold and the delay window, so every case is also replayed step by step with the reference's own
// generator, srsvec functions and IDFT, which gives the peak of every requested preamble; the survivors of the replay must be those
// of detect(). Built and run by tools/gen_prach_golden.py against the reference library that build() compiles into oracle/_ref/.
// The reference's DFT factory translation unit needs FFTW, so the driver hands out the generic DFT itself.
//
// stdin:  uint32 mode
//   mode 0 (generate): uint32 n, then n records {uint32 format, root_sequence_index, zero_correlation_zone, preamble_index}
//     stdout: n records {uint32 L, float y[L][2]}
//   mode 1 (detect):   uint32 n, then n records {uint32 format, ra_scs, root_sequence_index, zero_correlation_zone,
//                      start_preamble_index, nof_preamble_indices, L, float symbol[L][2]}
//     stdout: n records {float rssi_dB, float rssi, int64 time_resolution_Tc, int64 time_advance_max_Tc, uint32 ndet,
//                        ndet x {uint32 preamble_index, int64 time_advance_Tc, float power_dB},
//                        nof_preamble_indices x {uint32 peak_index, float peak_power, float metric}}
// --time: prints the mean time of detect() per occasion (64 preambles, one thread) for format 0 and format B4.
#include "srsran/phy/generic_functions/generic_functions_factories.h"
#include "srsran/phy/upper/channel_processors/channel_processor_factories.h"
#include "srsran/ran/prach/prach_cyclic_shifts.h"
#include "srsran/ran/prach/prach_preamble_information.h"
#include "srsran/srsvec/compare.h"
#include "srsran/srsvec/dot_prod.h"
#include "srsran/srsvec/prod.h"
#include "srsran/srsvec/zero.h"
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace srsran;

namespace {

constexpr unsigned IDFT_SIZE = 1536;
constexpr double   TC_PER_S  = 480e3 * 4096;

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

// One port, one occasion, one symbol: all the detector reads.
class one_symbol_buffer : public prach_buffer
{
  std::vector<cf_t> data;

public:
  explicit one_symbol_buffer(unsigned L) : data(L) {}
  unsigned         get_max_nof_ports() const override { return 1; }
  unsigned         get_max_nof_td_occasions() const override { return 1; }
  unsigned         get_max_nof_fd_occasions() const override { return 1; }
  unsigned         get_max_nof_symbols() const override { return 1; }
  unsigned         get_sequence_length() const override { return data.size(); }
  span<cf_t>       get_symbol(unsigned, unsigned, unsigned, unsigned) override { return data; }
  span<const cf_t> get_symbol(unsigned, unsigned, unsigned, unsigned) const override { return data; }
};

void read_exact(void* p, size_t n)
{
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "gen_prach_golden: short read\n");
    std::exit(1);
  }
}

template <typename T>
void put(const T& v)
{
  fwrite(&v, sizeof(T), 1, stdout);
}

int64_t to_tc(phy_time_unit t)
{
  return std::llround(t.to_seconds<double>() * TC_PER_S);
}

int time_mode()
{
  auto det_f = create_prach_detector_factory_simple(std::make_shared<generic_dft_factory>(), create_prach_generator_factory_sw(), IDFT_SIZE);
  std::mt19937                    rng(1);
  std::normal_distribution<float> gauss(0.f, 1.f);
  for (int pass = 0; pass != 2; ++pass) {
    prach_detector::configuration c = {};
    c.format                        = pass ? prach_format_type::B4 : prach_format_type::zero;
    c.ra_scs                        = pass ? prach_subcarrier_spacing::kHz30 : prach_subcarrier_spacing::kHz1_25;
    c.root_sequence_index           = 1;
    c.restricted_set                = restricted_set_config::UNRESTRICTED;
    c.zero_correlation_zone         = pass ? 11 : 1;
    c.start_preamble_index          = 0;
    c.nof_preamble_indices          = 64;
    one_symbol_buffer buf(pass ? 139 : 839);
    for (cf_t& v : buf.get_symbol(0, 0, 0, 0)) {
      v = cf_t(gauss(rng), gauss(rng));
    }
    auto     det  = det_f->create();
    unsigned sink = 0;
    for (int i = 0; i != 20; ++i) {
      sink += det->detect(buf, c).preambles.size();
    }
    const int reps = 400;
    auto      t0   = std::chrono::steady_clock::now();
    for (int i = 0; i != reps; ++i) {
      sink += det->detect(buf, c).preambles.size();
    }
    auto t1 = std::chrono::steady_clock::now();
    printf("reference prach_detector_simple_impl, format %s, 64 preambles, IDFT %u, one thread: %.1f us per occasion (%u)\n", pass ? "B4" : "0",
           IDFT_SIZE, std::chrono::duration<double, std::micro>(t1 - t0).count() / reps, sink);
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc > 1 && !strcmp(argv[1], "--time")) {
    return time_mode();
  }
  uint32_t mode = 0, n = 0;
  read_exact(&mode, sizeof(mode));
  read_exact(&n, sizeof(n));
  auto gen_f = create_prach_generator_factory_sw();

  if (mode == 0) {
    auto gen = gen_f->create();
    for (uint32_t i = 0; i != n; ++i) {
      uint32_t h[4];
      read_exact(h, sizeof(h));
      prach_generator::configuration c;
      c.format                = static_cast<prach_format_type>(h[0]);
      c.root_sequence_index   = h[1];
      c.zero_correlation_zone = h[2];
      c.preamble_index        = h[3];
      c.restricted_set        = restricted_set_config::UNRESTRICTED;
      span<const cf_t> y      = gen->generate(c);
      put<uint32_t>(y.size());
      fwrite(y.data(), sizeof(cf_t), y.size(), stdout);
    }
    return 0;
  }

  auto                        dft_f = std::make_shared<generic_dft_factory>();
  auto                        det_f = create_prach_detector_factory_simple(dft_f, gen_f, IDFT_SIZE);
  dft_processor::configuration idft_cfg = {};
  idft_cfg.size                         = IDFT_SIZE;
  idft_cfg.dir                          = dft_processor::direction::INVERSE;
  auto idft                             = dft_f->create(idft_cfg);
  auto gen                              = gen_f->create();

  for (uint32_t i = 0; i != n; ++i) {
    uint32_t h[7];
    read_exact(h, sizeof(h));
    const unsigned    L = h[6];
    one_symbol_buffer buf(L);
    read_exact(buf.get_symbol(0, 0, 0, 0).data(), L * sizeof(cf_t));

    prach_detector::configuration c;
    c.format                = static_cast<prach_format_type>(h[0]);
    c.ra_scs                = static_cast<prach_subcarrier_spacing>(h[1]);
    c.root_sequence_index   = h[2];
    c.zero_correlation_zone = h[3];
    c.start_preamble_index  = h[4];
    c.nof_preamble_indices  = h[5];
    c.restricted_set        = restricted_set_config::UNRESTRICTED;

    // A fresh detector per case, so that no case sees what an earlier one left in the IDFT input.
    const prach_detection_result res = det_f->create()->detect(buf, c);

    // Replay of prach_detector_simple_impl::detect with the same blocks, keeping every preamble.
    prach_preamble_information info = is_long_preamble(c.format) ? get_prach_preamble_long_info(c.format)
                                                                 : get_prach_preamble_short_info(c.format, c.ra_scs, false);
    const unsigned lower = L / 2, upper = L - lower;
    const unsigned fs    = ra_scs_to_Hz(info.scs) * IDFT_SIZE;
    const unsigned n_cs  = prach_cyclic_shifts_get(info.scs, c.restricted_set, c.zero_correlation_zone);
    unsigned       delay_n_maximum = info.cp_length.to_samples(fs);
    if (n_cs != 0) {
      delay_n_maximum = std::min(delay_n_maximum, (n_cs * IDFT_SIZE) / L);
    }
    span<cf_t> in = idft->get_input();
    srsvec::zero(in.subspan(upper, IDFT_SIZE - L));
    span<const cf_t> sig  = buf.get_symbol(0, 0, 0, 0);
    const float      rssi = srsvec::average_power(sig);

    struct peak {
      uint32_t index;
      float    power, metric;
    };
    std::vector<peak>     peaks(c.nof_preamble_indices, peak{0, 0.f, 0.f});
    std::vector<unsigned> replay_detected;
    if (std::isnormal(rssi)) {
      for (unsigned k = 0; k != c.nof_preamble_indices; ++k) {
        prach_generator::configuration g;
        g.format                = c.format;
        g.root_sequence_index   = c.root_sequence_index;
        g.preamble_index        = c.start_preamble_index + k;
        g.restricted_set        = c.restricted_set;
        g.zero_correlation_zone = c.zero_correlation_zone;
        span<const cf_t> y      = gen->generate(g);
        const float      ppow   = srsvec::average_power(y);
        srsvec::prod_conj(sig.first(lower), y.first(lower), in.last(lower));
        srsvec::prod_conj(sig.last(upper), y.last(upper), in.first(upper));
        span<const cf_t>           corr = idft->run();
        std::pair<unsigned, float> m    = srsvec::max_abs_element(corr);
        const float                norm = m.second / (rssi * ppow * y.size() * y.size());
        peaks[k]                        = peak{m.first, m.second, norm};
        unsigned delay_n                = m.first;
        if (delay_n > IDFT_SIZE / 2) {
          delay_n = IDFT_SIZE - delay_n;
        }
        if (!(norm < 0.07F) && delay_n < delay_n_maximum) {
          replay_detected.push_back(g.preamble_index);
        }
      }
    }
    bool same = replay_detected.size() == res.preambles.size();
    for (size_t k = 0; same && k != replay_detected.size(); ++k) {
      same = replay_detected[k] == res.preambles[k].preamble_index;
    }
    if (!same) {
      fprintf(stderr, "gen_prach_golden: case %u: the replay detects %zu preambles, detect() %zu\n", i, replay_detected.size(),
              (size_t)res.preambles.size());
      return 1;
    }

    put<float>(res.rssi_dB);
    put<float>(rssi);
    put<int64_t>(to_tc(res.time_resolution));
    put<int64_t>(to_tc(res.time_advance_max));
    put<uint32_t>(res.preambles.size());
    for (const auto& p : res.preambles) {
      put<uint32_t>(p.preamble_index);
      put<int64_t>(to_tc(p.time_advance));
      put<float>(p.power_dB);
    }
    for (const peak& p : peaks) {
      put<uint32_t>(p.index);
      put<float>(p.power);
      put<float>(p.metric);
    }
  }
  return 0;
}
