// Host-side construction of a polar code (polar_code_impl::set), of its pruned SSC schedule and of the index tables the device
// kernels read. Shared by polar.hip (tables cached per code on the device) and uci_polar.hip (tables that travel with a call).
#pragma once
#include "miphy_internal.h"
#include "tables/nr_polar_tables.h"
#include <algorithm>
#include <vector>

enum { POLAR_SSC_F = 1, POLAR_SSC_G = 2, POLAR_SSC_R1 = 3, POLAR_SSC_COMB = 4 };

struct polar_host_code {
  uint32_t              K, E, n, N, nPC, nWmPC;
  std::vector<uint8_t>  k_set;
  std::vector<uint16_t> pc_set;
  std::vector<uint16_t> blk;
};

// log2 of the mother code size (polar_code_impl.cpp:365-404, TS 38.212 5.3.1)
inline uint32_t polar_code_n(uint32_t K, uint32_t E, uint32_t nMax)
{
  uint32_t e = 1;
  while (e <= 13 && (1u << e) < E)
    ++e;
  const uint32_t n1 = ((8 * E <= 9 * (1u << (e - 1))) && (16 * K < 9 * E)) ? e - 1 : e;
  uint32_t       k  = 0;
  while (k <= 10 && (1u << k) < K)
    ++k;
  return std::max(std::min(std::min(n1, k + 3), nMax), 5u);
}

// polar_code_impl.cpp:325-490
inline int polar_build_code(const miphy_polar_code* c, polar_host_code& h)
{
  const uint32_t K = c->K, E = c->E, nMax = c->nMax;
  MIPHY_REQUIRE(E <= 8192, "polar: E = %u exceeds EMAX", E);
  if (nMax == 9) {
    MIPHY_REQUIRE(!(K < 36 || K > 164), "polar: codeblock length (K=%u) not supported for downlink transmission, choose 165 > K > 35", K);
  } else if (nMax == 10) {
    MIPHY_REQUIRE(!(K < 18 || (K > 25 && K < 31) || K > 1023), "polar: codeblock length (K=%u) not supported for uplink transmission", K);
  } else {
    MIPHY_REQUIRE(false, "polar: nMax not supported, choose 9 for downlink and 10 for uplink transmissions");
  }
  uint32_t nPC = 0, nWmPC = 0;
  if (K <= 25) {
    nPC = 3;
    if (E > K + 189)
      nWmPC = 1;
  }
  MIPHY_REQUIRE(K + nPC < E, "polar: rate-matched codeword length (E=%u) not supported, choose E > K + nPC", E);
  const uint32_t n = polar_code_n(K, E, nMax);
  const uint32_t N = 1u << n;
  MIPHY_REQUIRE(K < N, "polar: codeblock length (K=%u) not supported, choose K < N", K);
  h.K = K, h.E = E, h.n = n, h.N = N, h.nPC = nPC, h.nWmPC = nWmPC;
  std::vector<uint16_t> mother;
  for (uint32_t i = 0; i < 1024; ++i)
    if (NR_POLAR_Q1024[i] < N)
      mother.push_back(NR_POLAR_Q1024[i]);
  h.blk.resize(N);
  for (uint32_t j = 0; j < N; ++j)
    h.blk[j] = (uint16_t)(NR_POLAR_SUBBLOCK_P[32 * j / N] * (N / 32) + j % (N / 32));
  std::vector<uint16_t> cand(mother);
  if (N > E) {
    std::vector<uint8_t> drop(N, 0);
    uint32_t             T = 0;
    if (16 * K <= 7 * E) { // puncturing
      const uint32_t N_th = 3 * N / 4;
      T                   = (E >= N_th) ? N_th - (E >> 1) - 1 : 9 * N / 16 - (E >> 2);
      for (uint32_t i = 0; i < N - E; ++i)
        drop[h.blk[i]] = 1;
    } else { // shortening
      for (uint32_t i = E; i < N; ++i)
        drop[h.blk[i]] = 1;
    }
    cand.clear();
    for (uint16_t q : mother)
      if (!(q <= T) && !drop[q]) // setdiff_stable: also drops every index <= T (T = 0 when shortening)
        cand.push_back(q);
  }
  MIPHY_REQUIRE(cand.size() >= K + nPC, "polar: not enough reliable positions");
  const uint16_t* Kset = cand.data() + (cand.size() - K - nPC);
  h.pc_set.clear();
  for (uint32_t i = 0; i < ((nPC > nWmPC) ? nPC - nWmPC : 0); ++i)
    h.pc_set.push_back(Kset[i]);
  if (nWmPC == 1)
    h.pc_set.push_back((K <= 21) ? 252 : 248);
  std::sort(h.pc_set.begin(), h.pc_set.end());
  h.k_set.assign(N, 0);
  for (uint32_t i = 0; i < K + nPC; ++i)
    h.k_set[Kset[i]] = 1;
  return MIPHY_OK;
}

// What the list decoders read per position (polar_scl_run): the N information-set flags, followed by, per position, the exponent r of
// the largest aligned all-frozen block [i, i + 2^r) that starts there (orc_polar_scl_decode's rate-0 rule; 0 at an information bit).
inline void polar_build_list_flags(const polar_host_code& h, std::vector<uint8_t>& tab)
{
  tab.assign(h.k_set.begin(), h.k_set.end());
  const uint32_t Np = (uint32_t)h.k_set.size();
  uint32_t       np = 0;
  while ((1u << np) < Np)
    ++np;
  tab.resize(2 * Np, 0);
  for (uint32_t i = 0; i < Np; ++i) {
    uint32_t r = 0;
    if (!h.k_set[i]) {
      while (r < np && (i & ((2u << r) - 1u)) == 0) {
        bool frozen = true;
        for (uint32_t j = 0; j < (2u << r) && frozen; ++j)
          frozen = !h.k_set[i + j];
        if (!frozen)
          break;
        ++r;
      }
    }
    tab[Np + i] = (uint8_t)r;
  }
}

inline void polar_emit(std::vector<uint32_t>& s, uint32_t op, uint32_t stage, uint32_t pos)
{
  s.push_back(op | (stage << 4) | (pos << 8));
}

// Flattens polar_decoder_impl.cpp:209-333 (rate_0_node / rate_1_node / rate_r_node) into a list of vector operations.
inline void polar_build_schedule(const std::vector<uint8_t>& k_set, uint32_t s, uint32_t pos, std::vector<uint32_t>& out)
{
  const uint32_t size = 1u << s;
  bool           any = false, all = true;
  for (uint32_t i = 0; i < size; ++i) {
    any |= k_set[pos + i] != 0;
    all &= k_set[pos + i] != 0;
  }
  if (!any)
    return;
  if (all) {
    polar_emit(out, POLAR_SSC_R1, s, pos);
    return;
  }
  polar_emit(out, POLAR_SSC_F, s, pos);
  polar_build_schedule(k_set, s - 1, pos, out);
  polar_emit(out, POLAR_SSC_G, s, pos);
  polar_build_schedule(k_set, s - 1, pos + size / 2, out);
  polar_emit(out, POLAR_SSC_COMB, s, pos);
}

// The tables of one code as the kernels index them (see polar_plan in miphy_ext.h for the meaning of each).
struct polar_host_tables {
  std::vector<uint16_t> info_pos;
  std::vector<uint8_t>  is_pc;
  std::vector<uint16_t> tx_src, rx_fidx;
  std::vector<int32_t>  rx_first;
  std::vector<uint32_t> sched;
  std::vector<uint8_t>  pi_il;
};

inline void polar_build_tables(const polar_host_code& h, bool ibil, polar_host_tables& t)
{
  const uint32_t N = h.N, E = h.E, K = h.K;
  t = polar_host_tables();
  for (uint32_t q = 0; q < N; ++q)
    if (h.k_set[q]) {
      t.info_pos.push_back((uint16_t)q);
      t.is_pc.push_back(std::find(h.pc_set.begin(), h.pc_set.end(), (uint16_t)q) != h.pc_set.end());
    }
  // Channel interleaver (polar_rate_matcher_impl.cpp:62-88): f[io] = e[ii].
  std::vector<uint16_t> perm(E);
  if (ibil) {
    uint32_t S = 1, T = 1;
    while (S < E) {
      ++T;
      S += T;
    }
    uint32_t io = 0;
    for (uint32_t r = 0; r < T; ++r) {
      uint32_t ii = r;
      for (uint32_t cc = 0; cc < T - r; ++cc) {
        if (ii < E) {
          perm[io++] = (uint16_t)ii;
          ii += T - cc;
        } else
          break;
      }
    }
  } else {
    for (uint32_t i = 0; i < E; ++i)
      perm[i] = (uint16_t)i;
  }
  // Bit selection (polar_rate_matcher_impl.cpp:43-60): e[k] = y[sel(k)], y[j] = d[blk[j]].
  const bool punct = (E < N) && (16 * K <= 7 * E);
  auto       sel   = [&](uint32_t k) { return (E >= N) ? k % N : (punct ? k + (N - E) : k); };
  t.tx_src.resize(E), t.rx_fidx.resize(E);
  for (uint32_t o = 0; o < E; ++o) {
    t.tx_src[o]        = h.blk[sel(perm[o])];
    t.rx_fidx[perm[o]] = (uint16_t)o;
  }
  // Inverse (polar_rate_dematcher_impl.cpp:43-68): for codeword position q = blk[j], y[j] comes from e[j'] (+ repetitions).
  t.rx_first.resize(N);
  for (uint32_t j = 0; j < N; ++j) {
    int32_t first;
    if (E >= N)
      first = (int32_t)j;
    else if (punct)
      first = (j < N - E) ? -1 : (int32_t)(j - (N - E));
    else
      first = (j < E) ? (int32_t)j : -2;
    t.rx_first[h.blk[j]] = first;
  }
  polar_build_schedule(h.k_set, h.n, 0, t.sched);
  for (uint32_t m = 0; m < NR_POLAR_K_MAX_IL; ++m)
    if (K <= NR_POLAR_K_MAX_IL && NR_POLAR_PI_IL_MAX[m] >= NR_POLAR_K_MAX_IL - K)
      t.pi_il.push_back((uint8_t)(NR_POLAR_PI_IL_MAX[m] - (NR_POLAR_K_MAX_IL - K)));
}
