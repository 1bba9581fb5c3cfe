// What the PRACH blocks derive from a configuration before they look at a sample, restated from TS 38.211 Tables 6.3.3.1-1, -2, -5, -6,
// -7 and 6.3.3.2-1 once for the detector / generator (prach.hip) and the OFDM PRACH demodulator (prach_demod.hip):
//  - prach_preamble_info: L, RA subcarrier spacing, N_CP and N_CS of a (format, ra_scs, zone, set), host and device;
//  - prach_demod_geometry: the time and frequency geometry of srsran::ofdm_prach_demodulator_impl::demodulate
//    (lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:31-199, lib/ran/prach/prach_preamble_information.cpp,
//    lib/ran/prach/prach_frequency_mapping.cpp), a plain host function: jobs of the demodulator live on the host.
#pragma once
#include "miphy_internal.h"
#include <algorithm>

// L, RA subcarrier spacing in Hz, N_CP in units of kappa and N_CS of a (format, ra_scs, zone, set); false where the reference asserts
// (get_prach_preamble_short_info on a long RA spacing, "Unrestricted sets are not implemented", "Reserved cyclic shift").
__host__ __device__ inline bool prach_preamble_info(uint32_t format, uint32_t ra_scs, uint32_t zone, uint32_t restricted_set, uint32_t& L,
                                                    uint32_t& scs_hz, uint32_t& cp_kappa, uint32_t& n_cs)
{
  // TS 38.211 Tables 6.3.3.1-5, -6, -7 (unrestricted set) and 6.3.3.1-1, -2 (N_CP^RA / kappa; the A/B pairs take the A value, every
  // occasion but the last one of a slot).
  static constexpr uint16_t NCS_1_25[16]  = {0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419};
  static constexpr uint16_t NCS_5[16]     = {0, 13, 26, 33, 38, 41, 49, 55, 64, 76, 93, 119, 139, 209, 279, 419};
  static constexpr uint16_t NCS_SHORT[16] = {0, 2, 4, 6, 8, 10, 12, 13, 15, 17, 19, 23, 27, 34, 46, 69};
  static constexpr uint16_t CP_LONG[4]    = {3168, 21024, 4688, 3168};
  static constexpr uint16_t CP_SHORT[10]  = {288, 576, 864, 216, 936, 1240, 2048, 288, 576, 864};
  if (format >= MIPHY_PRACH_NOF_FORMATS || restricted_set != 0 || zone > 15)
    return false;
  if (format <= MIPHY_PRACH_FORMAT_3) {
    L        = 839;
    scs_hz   = (format == MIPHY_PRACH_FORMAT_3) ? 5000 : 1250;
    cp_kappa = CP_LONG[format];
    n_cs     = (format == MIPHY_PRACH_FORMAT_3) ? NCS_5[zone] : NCS_1_25[zone];
    return true;
  }
  if (ra_scs > 3)
    return false;
  L        = 139;
  scs_hz   = 15000u << ra_scs;
  cp_kappa = (uint32_t)CP_SHORT[format - MIPHY_PRACH_FORMAT_A1] >> ra_scs;
  n_cs     = NCS_SHORT[zone];
  return true;
}

// DFT sizes the device transforms: 2^a 3^b in 8 .. 4096 in one LDS pass, or one of the four-step sizes (ofdm.hip).
bool miphy_dft_size_served(uint32_t N);

// Times are whole numbers of kappa = 64 T_c (1 / (15 kHz * 2048)): every duration below is one. 0.5 ms = 15360 kappa, 1 ms = 30720.
// Returns MIPHY_OK, MIPHY_EINVAL where the reference asserts (the message names the rule) or MIPHY_EUNSUPP for a DFT size the reference
// would take and the device does not transform.
inline int prach_demod_geometry(uint32_t srate_hz, const miphy_prach_demod_job& j, miphy_prach_demod_info_t& o)
{
  static constexpr uint64_t KAPPA_PER_S  = 15000ull * 2048ull;
  static constexpr uint32_t HALF_MS      = 15360, SIXTEEN = 16;
  static constexpr uint32_t SYM_LONG[4]  = {24576, 2 * 24576, 4 * 24576, 4 * 6144};                 // symbol_length of formats 0..3
  static constexpr uint8_t  SYM_SHORT[10] = {2, 4, 6, 2, 12, 1, 4, 2, 4, 6};                          // x 2048 kappa >> mu: A1 A2 A3 B1 B4 C0 C2 pairs
  static constexpr uint8_t  DURATION[10]  = {2, 4, 6, 2, 12, 2, 6, 2, 4, 6};                          // get_preamble_duration, PUSCH symbols
  static constexpr uint16_t CP_LAST[3]    = {216, 360, 504};                                          // B1, B2, B3: last occasion of an A/B pair
  // prach_frequency_mapping_get: {nof_rb_ra, k_bar} by [RA spacing 1.25, 5, 15, 30, 60, 120 kHz][PUSCH spacing 15 .. 120 kHz], 0 = reserved
  static constexpr uint8_t MAP[6][4][2] = {{{6, 7}, {3, 1}, {2, 133}, {0, 0}},   {{24, 12}, {12, 10}, {6, 7}, {0, 0}}, {{12, 2}, {6, 2}, {3, 2}, {0, 0}},
                                           {{24, 2}, {12, 2}, {6, 2}, {0, 0}},   {{0, 0}, {0, 0}, {12, 2}, {6, 2}},    {{0, 0}, {0, 0}, {24, 2}, {12, 2}}};
  o = miphy_prach_demod_info_t{};
  MIPHY_REQUIRE(j.format < MIPHY_PRACH_NOF_FORMATS, "prach_demod: format %u is not a PRACH format", j.format);
  MIPHY_REQUIRE(j.pusch_scs <= 3, "prach_demod: PUSCH subcarrier spacing %u (0..3 = 15..120 kHz)", j.pusch_scs);
  const bool     is_long = j.format <= MIPHY_PRACH_FORMAT_3;
  const uint32_t mu      = j.pusch_scs;
  if (is_long)
    MIPHY_REQUIRE(j.nof_td_occasions == 1, "prach_demod: long preambles only support one occasion (%u)", j.nof_td_occasions);
  MIPHY_REQUIRE(j.nof_td_occasions > 0 && j.nof_fd_occasions > 0, "prach_demod: the number of occasions must be greater than 0 (%u x %u)",
                j.nof_td_occasions, j.nof_fd_occasions);
  MIPHY_REQUIRE(j.nof_td_occasions <= MIPHY_PRACH_MAX_TD_OCCASIONS && j.nof_fd_occasions <= MIPHY_PRACH_MAX_FD_OCCASIONS &&
                    j.nof_fd_occasions <= j.max_nof_fd_occasions,
                "prach_demod: %u x %u occasions exceed the maxima (%u x %u) or the buffer's frequency-domain occasions (%u)", j.nof_td_occasions,
                j.nof_fd_occasions, MIPHY_PRACH_MAX_TD_OCCASIONS, MIPHY_PRACH_MAX_FD_OCCASIONS, j.max_nof_fd_occasions);
  // the strides are this interface's own: bounded so that every row offset below stays far inside 64 bits and a row stride inside 32
  MIPHY_REQUIRE(j.max_nof_fd_occasions <= MIPHY_PRACH_MAX_STRIDE && j.max_nof_symbols <= MIPHY_PRACH_MAX_STRIDE,
                "prach_demod: buffer strides %u x %u exceed %u", j.max_nof_fd_occasions, j.max_nof_symbols, MIPHY_PRACH_MAX_STRIDE);
  uint32_t L = 0, scs_hz = 0, cp_kappa = 0, n_cs = 0;
  prach_preamble_info(j.format, mu, 0, 0, L, scs_hz, cp_kappa, n_cs); // short formats: to_ra_subcarrier_spacing(pusch_scs)
  const uint32_t ra_index = is_long ? (j.format == MIPHY_PRACH_FORMAT_3 ? 1u : 0u) : 2u + mu;
  const uint32_t sym_kappa = is_long ? SYM_LONG[j.format] : ((uint32_t)SYM_SHORT[j.format - MIPHY_PRACH_FORMAT_A1] * 2048u) >> mu;
  o.L = L, o.ra_scs_hz = scs_hz;
  o.nof_rb_ra = MAP[ra_index][mu][0], o.k_bar = MAP[ra_index][mu][1];
  MIPHY_REQUIRE(o.nof_rb_ra != 0, "prach_demod: the PRACH (%u Hz) and PUSCH (%u kHz) subcarrier spacing combination is reserved", scs_hz, 15u << mu);
  MIPHY_REQUIRE(srate_hz != 0 && srate_hz % scs_hz == 0, "prach_demod: the sampling rate %u Hz is not a multiple of the RA subcarrier spacing %u Hz",
                srate_hz, scs_hz);
  o.dft_size = srate_hz / scs_hz;
  // phy_time_unit::to_samples: asserts a whole number of samples
  // (caller fields are multiplied in 64 bits, times by the sampling rate in 128: nothing wraps before it is compared)
  auto whole = [&](uint64_t kappa) { return ((unsigned __int128)kappa * srate_hz) % KAPPA_PER_S == 0; };
  auto samples = [&](uint64_t kappa) { return (uint64_t)(((unsigned __int128)kappa * srate_hz) / KAPPA_PER_S); };
  MIPHY_REQUIRE(((uint64_t)sym_kappa * scs_hz) % KAPPA_PER_S == 0, "prach_demod: the symbol length is not a whole number of symbols");
  o.nof_symbols = (uint32_t)(((uint64_t)sym_kappa * scs_hz) / KAPPA_PER_S);
  MIPHY_REQUIRE(o.nof_symbols <= j.max_nof_symbols, "prach_demod: %u symbols exceed the buffer's %u", o.nof_symbols, j.max_nof_symbols);
  o.K                  = (15000u << mu) / scs_hz;
  const uint64_t grid  = (uint64_t)j.nof_prb_ul_grid * o.K * 12u;
  MIPHY_REQUIRE(o.dft_size > grid, "prach_demod: DFT size %u for PRACH SCS %u is not sufficient for K=%u, N_RB=%u", o.dft_size, scs_hz, o.K,
                j.nof_prb_ul_grid);
  for (uint32_t fd = 0; fd < j.nof_fd_occasions; ++fd) {
    const uint64_t k_start = (uint64_t)o.K * 12u * ((uint64_t)j.rb_offset + o.nof_rb_ra * fd) + o.k_bar;
    MIPHY_REQUIRE(k_start + L < grid, "prach_demod: start subcarrier %llu plus sequence length %u exceeds PRACH grid size %llu",
                  (unsigned long long)k_start, L, (unsigned long long)grid);
    o.k_start[fd] = (uint32_t)k_start; // below grid, which is below dft_size
  }
  const uint32_t sym_pusch = (144u + 2048u) >> mu; // occasions start on PUSCH symbols, also for long formats
  const uint32_t duration  = is_long ? 0u : DURATION[j.format - MIPHY_PRACH_FORMAT_A1];
  auto start_of = [&](uint64_t t) { // + 16 kappa past the start of the subframe, + 16 kappa past 0.5 ms (both strict)
    if (t > 0)
      t += SIXTEEN;
    if (t > HALF_MS)
      t += SIXTEEN;
    return t;
  };
  for (uint32_t td = 0; td < j.nof_td_occasions; ++td) {
    uint32_t cp = cp_kappa;
    if (td + 1 == j.nof_td_occasions && j.format >= MIPHY_PRACH_FORMAT_A1_B1)
      cp = (uint32_t)CP_LAST[j.format - MIPHY_PRACH_FORMAT_A1_B1] >> mu;
    const uint64_t t_start = start_of((uint64_t)sym_pusch * ((uint64_t)j.start_symbol + duration * td));
    const uint64_t t_end   = t_start + cp + sym_kappa;
    if (!is_long) { // the occasion overlaps with time zero / with 0.5 ms (both ends included)
      if (t_start == 0)
        cp += SIXTEEN;
      if (t_start <= HALF_MS && t_end >= HALF_MS)
        cp += SIXTEEN;
    }
    MIPHY_REQUIRE(whole(t_start) && whole(cp) && whole((uint64_t)cp + sym_kappa),
                  "prach_demod: occasion %u: its start (%llu kappa) or cyclic prefix (%u kappa) is not a whole number of samples at %u Hz", td,
                  (unsigned long long)t_start, cp, srate_hz);
    MIPHY_REQUIRE(samples(t_start) + samples((uint64_t)cp + sym_kappa) <= j.nof_samples,
                  "prach_demod: occasion %u reads samples %llu .. %llu of a window of %u", td, (unsigned long long)samples(t_start),
                  (unsigned long long)(samples(t_start) + samples((uint64_t)cp + sym_kappa)), j.nof_samples);
    o.td_sample_offset[td] = (uint32_t)samples(t_start); // inside the window
    o.td_cp_samples[td]    = (uint32_t)samples(cp);
  }
  // get_prach_window_duration: counted in 15 kHz symbols for long formats, rounded up to a whole subframe
  const uint64_t w_start = start_of((uint64_t)(is_long ? 144u + 2048u : sym_pusch) * j.start_symbol);
  uint64_t       w_end;
  if (is_long) {
    w_end = (w_start + cp_kappa + sym_kappa + 30719u) / 30720u * 30720u;
  } else {
    w_end = w_start + (uint64_t)sym_pusch * duration * j.nof_td_occasions;
    if (w_start == 0)
      w_end += SIXTEEN;
    if (w_start <= HALF_MS && w_end > HALF_MS) // strict at the end, unlike the occasion's own test
      w_end += SIXTEEN;
    MIPHY_REQUIRE(whole(w_end), "prach_demod: the window (%llu kappa) is not a whole number of samples at %u Hz", (unsigned long long)w_end, srate_hz);
    MIPHY_REQUIRE(j.nof_samples >= samples(w_end), "prach_demod: the number of input samples (%u) must be equal to or greater than the PRACH window (%llu)",
                  j.nof_samples, (unsigned long long)samples(w_end));
  }
  o.window_samples = (uint32_t)std::min<uint64_t>(samples(w_end), UINT32_MAX);
  if (!miphy_dft_size_served(o.dft_size)) {
    miphy_set_error("prach_demod: DFT size %u not supported (2^a*3^b <= 4096, or one of 4608 ... 49152)", o.dft_size);
    return MIPHY_EUNSUPP;
  }
  return MIPHY_OK;
}
