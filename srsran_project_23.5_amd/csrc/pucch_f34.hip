// PUCCH processor, formats 3 and 4 (DFT-s-OFDM; TS 38.211 6.3.2.6, 6.4.1.3.3), for a batch of PDUs that share one device grid. Beyond the 23.5 reference,
// whose demodulator asserts on both formats; the contract is the standard, restated in numpy in tests/pucch_f34_tx.py and tests/pucch_f34_ref.py.
// One workgroup per PDU goes from the grid to soft bits, channel state and, for 3..11 bits, the payload.
//
// The signal. DM-RS symbols by length (offsets from start_symbol, Table 6.4.1.3.3.2-1): 4: {1}, with hopping {0, 2}; 5: {0, 3}; 6, 7: {1, 4}; 8: {1, 5};
// 9: {1, 6}; 10, 11: {2, 7}; 12: {2, 8}; 13: {2, 9}; 14: {3, 10}; with additional DM-RS 10: {1, 3, 6, 8}; 11: {1, 3, 6, 9}; 12: {1, 4, 7, 10};
// 13: {1, 4, 7, 11}; 14: {1, 5, 8, 12}. With hopping the first floor(N / 2) symbols are on starting_prb, the others on second_hop_prb. DM-RS symbol l
// (absolute) carries r(n) = e^(j alpha_l n) rbar_(u,0)(n), n < M = 12 nof_prb, rbar the base sequence of low_papr_device.h, u = n_id_hopping mod 30,
// alpha_l = 2 pi / 12 ((m0 + n_cs(n_s, l)) mod 12) as for format 1 (pucch_alpha of pucch_device.h, c_init = n_id_hopping); m0 = 0 (format 3),
// {0, 6}[occ_index] (format 4, two sequences), {0, 6, 3, 9}[occ_index] (four). Data: E = Qm M (data symbols) bits for format 3, Qm (12 / N_SF) (data
// symbols) for format 4, scrambled with c_init = rnti 2^15 + n_id_scrambling, QPSK or pi/2-BPSK (rotation by the parity of the symbol index); format 4
// spreads the 12 / N_SF symbols of an OFDM symbol to y(k) = w_n(k) d(k mod (12 / N_SF)), w_n(k) = g_n^floor(k N_SF / 12) with g = (1, -1) for two sequences and (1, -j, -1, +j) for four;
// every data symbol is transform precoded, z = DFT_M(y) / sqrt(M).
//
// The receiver, per receive port and hop (the arithmetic of port_channel_estimator_average_impl::compute with all 12 REs of a PRB as DM-RS: window 12,
// no interpolation -- what pucch.hip does for format 1 on one PRB, on nof_prb PRBs):
//  1. s(k) = sum over the hop's DM-RS symbols of x_l(k) conj(r_l(k)), symbols ascending; EPRE += sum |x_l(k)|^2.
//  2. Format 4 only, before anything uses s: s(k) <- (s(b) + ... + s(b + N_SF - 1)) / N_SF over the aligned block b = k - k mod N_SF. The cyclic
//     shifts of the other N_SF - 1 PDUs of the PRB differ by multiples of 12 / N_SF, so their DM-RS cancel exactly in such a block (on a channel that
//     is flat over it) -- the idea of the pair despreading of miphy_dmrs_pusch_estimate_layers_batch.
//  3. RSRP += sum |s(k)|^2 / n_dmrs(hop); h(k) = s(k) / n_dmrs(hop); noise += (12 / M) sum_l sum_k |x_l(k) - a(k) r_l(k)|^2 with a = the mean of h over
//     the PRB of k; time alignment += the peak of |IDFT_4096(h)| inside +-144 taps (hop_time_alignment of pucch_device.h).
//  4. finish_port: EPRE and RSRP over M n_dmrs pilots, noise / (12 n_dmrs - 1), forced to EPRE / 1000 with fewer than 3 DM-RS symbols or with
//     hopping, time alignment averaged over the hops; the CSI is averaged linearly over the ports. Decision: the noise estimate does not remove the
//     DM-RS of co-scheduled format-4 PDUs, as format 1 does not today.
//  5. Every data symbol: zero forcing 1 x N with the noise variance of the first port (zf_prepare / zf_apply of equalize_device.h on one layer: the
//     arithmetic of miphy_channel_equalize_batch), the M elements into LDS (tp_put) and through tp_deprecode_symbol, which gives y(n) and the
//     symbol's noise variance v -- the functions of miphy_transform_deprecode_batch.
//  6. Format 4: d(j) = (((t_0 + t_1) + t_2) + t_3) / N_SF, t_q = conj(w_n(j + q 12 / N_SF)) y(j + q 12 / N_SF) (the products by +-1, +-j exact), v / N_SF.
//  7. The exact soft demapper of demod_device.h (what miphy_pusch_demodulate_tp_batch computes), descrambled, into LDS; from there to llr_out, and for
//     3..11 bits through the short-block detector of uci_device.h by the first wavefront. 12 bits and more: the soft bits leave the kernel and the
//     polar decoder of uci_polar.hip takes them behind it on the same stream and stores its verdict over the status byte (as
//     miphy_pucch_process_batch_ex chains it).
// est_out receives h as the data path read it, [port][hop][M], and the noise variance per port.
//
// Geometry: 256 lanes per PDU. A PDU has at most 192 subcarriers, so 192 lanes would hold one each; the de-precoding functions of tp_device.h are
// written for TP_THREADS = 256 lanes (tp_deprecode_symbol adds four wavefront partials in a fixed order, which is what makes a symbol's noise variance
// the same bits through the stand-alone de-precoder and through here), and giving them a lane-count parameter would have to leave every existing caller's
// code as it is. Launching 256 lanes leaves them untouched; the fourth wavefront only takes part in barriers, reductions and the time alignment, where the
// four wavefronts share the up to eight (port, hop) searches. LDS: 4 x 2 x 192 estimates (12 KB), 4608 soft bits, the padded 192-point buffer and the
// scrambling words: 19.8 KB, so eight workgroups = 32 wavefronts fit a CU by LDS and the wavefront slots, not LDS, bound the occupancy. A slot's batch is at
// most a workgroup per CU, so what a call costs is the latency of one PDU's chain (DESIGN.md section 5 has the measurement and what was tried on it).
#include "demod_device.h"
#include "equalize_device.h"
#include "low_papr_device.h"
#include "miphy_ext.h"
#include "pucch_device.h"
#include "tp_device.h"
#include "uci_device.h"
#include "uci_polar_info.h"
#include <vector>

namespace {

constexpr int F34_MAX_M   = 192;
constexpr int F34_MAX_LLR = 2 * F34_MAX_M * 12; // 14 symbols, two of them DM-RS

// DM-RS symbols of an allocation of nsym symbols as a mask of offsets from its first symbol.
__host__ __device__ inline uint32_t f34_dmrs_offsets(unsigned nsym, bool hop, bool additional)
{
  if (additional && nsym >= 10) {
    const unsigned third = nsym >= 12 ? 7 + (nsym == 14) : 6, last = nsym == 10 ? 8 : (nsym == 11 ? 9 : nsym - 2);
    return (1u << 1) | (1u << (nsym == 14 ? 5 : (nsym >= 12 ? 4 : 3))) | (1u << third) | (1u << last);
  }
  switch (nsym) {
    case 4:
      return hop ? 0x5u : 0x2u;
    case 5:
      return (1u << 0) | (1u << 3);
    case 6:
    case 7:
      return (1u << 1) | (1u << 4);
    case 8:
      return (1u << 1) | (1u << 5);
    case 9:
      return (1u << 1) | (1u << 6);
    case 10:
    case 11:
      return (1u << 2) | (1u << 7);
    case 12:
      return (1u << 2) | (1u << 8);
    case 13:
      return (1u << 2) | (1u << 9);
    default:
      return (1u << 3) | (1u << 10);
  }
}

// What follows from the fields of a job that passed the rules below.
struct f34_layout {
  uint32_t dmrs; // offsets from start_symbol
  int      split; // first offset of the second hop; nof_symbols without hopping
  int      ndm[2], ndata[2];
  int      M, Qm, per_symbol, E; // per_symbol: modulation symbols of one data OFDM symbol
};
__host__ __device__ inline f34_layout f34_layout_of(const miphy_pucch_f34_job& j)
{
  f34_layout l;
  const int  nsym = j.nof_symbols;
  l.dmrs  = f34_dmrs_offsets(nsym, j.intra_slot_hopping != 0, j.additional_dmrs != 0);
  l.split = j.intra_slot_hopping ? nsym / 2 : nsym;
  l.ndm[0] = l.ndm[1] = l.ndata[0] = l.ndata[1] = 0;
  for (int i = 0; i < nsym; ++i) {
    const int h = i >= l.split;
    if ((l.dmrs >> i) & 1u)
      ++l.ndm[h];
    else
      ++l.ndata[h];
  }
  l.M          = 12 * j.nof_prb;
  l.Qm         = j.pi2_bpsk ? 1 : 2;
  l.per_symbol = j.format == 4 ? 12 / j.occ_length : l.M;
  l.E          = l.Qm * l.per_symbol * (l.ndata[0] + l.ndata[1]);
  return l;
}

// The rules of one job on the host: MIPHY_EINVAL or MIPHY_EUNSUPP with the first rule it breaks in miphy_last_error().
int f34_check(const char* who, uint32_t i, const miphy_pucch_f34_job& j, f34_layout& lay)
{
#define F34_REQUIRE(cond, msg, ...) MIPHY_REQUIRE(cond, "%s: job %u: " msg, who, i, ##__VA_ARGS__)
  F34_REQUIRE(j.format == 3 || j.format == 4, "format %u is not 3 or 4", (unsigned)j.format);
  F34_REQUIRE(j.numerology <= 4 && j.slot < (10u << j.numerology), "slot %u outside the frame of numerology %u", (unsigned)j.slot, (unsigned)j.numerology);
  F34_REQUIRE(j.nof_ports >= 1 && j.nof_ports <= 4, "invalid number of receive ports %u", (unsigned)j.nof_ports);
  F34_REQUIRE(j.nof_symbols >= 4 && j.nof_symbols <= 14 && j.start_symbol + j.nof_symbols <= 14, "invalid symbol range (%u symbols from %u; 4..14 within the slot)",
              (unsigned)j.nof_symbols, (unsigned)j.start_symbol);
  F34_REQUIRE(j.grid_nprb >= 1 && j.grid_nprb <= 275 && (uint32_t)j.bwp_start_rb + j.bwp_size_rb <= j.grid_nprb, "the BWP (%u PRBs from %u) leaves the grid of %u PRBs",
              (unsigned)j.bwp_size_rb, (unsigned)j.bwp_start_rb, j.grid_nprb);
  F34_REQUIRE(j.pi2_bpsk <= 1 && j.additional_dmrs <= 1 && j.intra_slot_hopping <= 1, "pi2_bpsk, additional_dmrs and intra_slot_hopping are 0 or 1");
  F34_REQUIRE(j.n_id_hopping <= 1023 && j.n_id_scrambling <= 1023, "n_id_hopping and n_id_scrambling are 0..1023");
  if (j.format == 3) {
    if (j.nof_prb == 2) {
      miphy_set_error("%s: job %u: format 3 on 2 PRBs needs the length-24 sequences of TS 38.211 Table 5.2.2.2-4, which the library does not hold", who, i);
      return MIPHY_EUNSUPP;
    }
    F34_REQUIRE(j.nof_prb <= 16 && tp_nprb_ok(j.nof_prb), "format 3 on %u PRBs (1, 3, 4, 5, 6, 8, 9, 10, 12, 15 or 16)", (unsigned)j.nof_prb);
  } else {
    F34_REQUIRE(j.nof_prb == 1, "format 4 on %u PRBs (it takes one)", (unsigned)j.nof_prb);
    F34_REQUIRE(j.occ_length == 2 || j.occ_length == 4, "format 4 with occ_length %u (2 or 4)", (unsigned)j.occ_length);
    F34_REQUIRE(j.occ_index < j.occ_length, "occ_index %u is not below occ_length %u", (unsigned)j.occ_index, (unsigned)j.occ_length);
  }
  F34_REQUIRE((uint32_t)j.starting_prb + j.nof_prb <= j.bwp_size_rb && (!j.intra_slot_hopping || (uint32_t)j.second_hop_prb + j.nof_prb <= j.bwp_size_rb),
              "the allocation leaves the BWP of %u PRBs", (unsigned)j.bwp_size_rb);
  F34_REQUIRE(j.nof_csi_part2 == 0, "CSI part 2 (%u bits) is not decoded on PUCCH", (unsigned)j.nof_csi_part2);
  const uint32_t K = (uint32_t)j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
  F34_REQUIRE(K >= 3, "%u UCI bits (formats 3 and 4 carry 3 and more)", K);
  lay = f34_layout_of(j);
  if (K <= 11) {
    F34_REQUIRE(miphy_uci_job_ok(K, (uint32_t)lay.Qm, (uint32_t)lay.E), "%u bits in %u soft bits: the short block code needs more soft bits than bits", K, (unsigned)lay.E);
    return MIPHY_OK;
  }
#undef F34_REQUIRE
  uci_polar_framing f;
  return uci_polar_frame_or_error(who, i, K, (uint32_t)lay.E, f);
}

// y j^e, exact
__device__ __forceinline__ float2 mul_j_pow(float2 y, int e)
{
  switch (e & 3) {
    case 1:
      return make_float2(-y.y, y.x);
    case 2:
      return make_float2(-y.x, -y.y);
    case 3:
      return make_float2(y.y, -y.x);
    default:
      return y;
  }
}

struct f34_lds {
  float2   ce[4][2][F34_MAX_M];                       // h per port and hop
  cplx     x[fft_lds_bytes(F34_MAX_M) / sizeof(cplx)]; // the de-precoder's buffer
  uint32_t scr[F34_MAX_LLR / 32];
  int8_t   llr[F34_MAX_LLR];
  float    part[8][4][3]; // per (port, hop) and wavefront: EPRE, RSRP and noise sums
  float    ta[8];
  float    red[8];
  int      alpha[4];
  uint8_t  status;
};

__global__ void __launch_bounds__(TP_THREADS) pucch_f34_kernel(const miphy_pucch_f34_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                               const float* const* __restrict__ tws, const float2* __restrict__ grid,
                                                               uint8_t* __restrict__ payload, miphy_pucch_result* __restrict__ results,
                                                               int8_t* __restrict__ llr_out, int8_t* __restrict__ llr_long, float* __restrict__ est_out)
{
#pragma clang fp contract(off)
  __shared__ f34_lds        L;
  const int                 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const miphy_pucch_f34_job j   = jobs[blockIdx.x];
  const f34_layout          lay = f34_layout_of(j);
  const int                 M = lay.M, nports = j.nof_ports, s = j.start_symbol, nsym = j.nof_symbols;
  const bool                hop = j.intra_slot_hopping != 0, f4 = j.format == 4;
  const int                 nh = hop ? 2 : 1, occ = f4 ? j.occ_length : 1;
  const int                 ndm_all = lay.ndm[0] + lay.ndm[1];
  const int                 nsc = 12 * (int)j.grid_nprb;
  const int                 prb[2] = {j.bwp_start_rb + j.starting_prb, j.bwp_start_rb + (hop ? j.second_hop_prb : j.starting_prb)};
  const float2*             g = grid + j.grid_offset;
  const uint32_t            K = (uint32_t)j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
  const int                 k = tid; // this lane's subcarrier of the allocation
  const bool                mine = k < M;

  // The DM-RS symbols (absolute), ascending: those of the first hop come first.
  int dm_l[4] = {0, 0, 0, 0};
  {
    int d = 0;
    for (int i = 0; i < nsym; ++i)
      if ((lay.dmrs >> i) & 1u)
        dm_l[d++] = s + i;
  }
  // Scrambling words; cyclic shift of every DM-RS symbol.
  if (tid < (lay.E + 31) / 32)
    L.scr[tid] = gold_word(*gt, (uint32_t)j.rnti * 32768u + j.n_id_scrambling, 32u * (uint32_t)tid);
  if (tid >= F34_MAX_M && tid < F34_MAX_M + ndm_all) {
    const int      d  = tid - F34_MAX_M;
    const uint32_t m0 = !f4 ? 0u : (occ == 2 ? 6u * j.occ_index : (uint32_t)((0x9360u >> (4 * j.occ_index)) & 0xfu)); // {0, 6, 3, 9}
    L.alpha[d]        = pucch_alpha(*gt, j.n_id_hopping, j.slot, (uint32_t)dm_l[d], m0);
  }
  __syncthreads();

  // r_l(k) of this lane for every DM-RS symbol.
  const int u = j.n_id_hopping % 30;
  float2    pil[4];
  {
    // rbar from the table's row of shift 0 (M = 12) or in closed form, then the shift as an exact twelfth of a turn: the table's rows of the other shifts
    // hold the reference's format-1 values, whose single-precision angles of up to 63 rad are off by up to 4e-6.
    const unsigned nzc  = low_papr_prime_below((unsigned)M);
    float2         rbar = make_float2(0.f, 0.f);
    if (mine)
      rbar = low_papr_element((unsigned)u, low_papr_zc_root((unsigned)u, 0, nzc), nzc, (unsigned)M, (unsigned)k);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      pil[d] = make_float2(0.f, 0.f);
      if (d < ndm_all && mine) {
        float sn, cs;
        sincospif((float)((L.alpha[d] * k) % 12) / 6.0f, &sn, &cs);
        pil[d] = cmul(rbar, make_float2(cs, sn));
      }
    }
  }

  // ---- estimation
  for (int p = 0; p < nports; ++p) {
    for (int h = 0; h < nh; ++h) {
      const int     d0 = h ? lay.ndm[0] : 0, nd = lay.ndm[h];
      const float2* col = g + (size_t)p * 14 * nsc + 12 * prb[h] + (mine ? k : 0);
      float2        y[4];
      float2        sum = make_float2(0.f, 0.f);
      float         e   = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        y[d] = make_float2(0.f, 0.f);
        if (d >= d0 && d < d0 + nd && mine) {
          y[d]            = col[(size_t)dm_l[d] * nsc];
          const float2 pr = cmulc(y[d], pil[d]);
          sum.x += pr.x, sum.y += pr.y;
          e += y[d].x * y[d].x + y[d].y * y[d].y;
        }
      }
      float2* ce = L.ce[p][h];
      if (f4) { // uniform
        if (mine)
          ce[k] = sum;
        __syncthreads();
        if (mine) {
          const int b  = k - k % occ;
          float2    a = ce[b];
          for (int q = 1; q < occ; ++q)
            a.x += ce[b + q].x, a.y += ce[b + q].y;
          const float sc = 1.0f / (float)occ;
          sum            = make_float2(a.x * sc, a.y * sc);
        }
        __syncthreads();
      }
      const float  rs  = sum.x * sum.x + sum.y * sum.y;
      const float  sc  = 1.0f / (float)nd;
      const float2 lse = make_float2(sum.x * sc, sum.y * sc);
      if (mine)
        ce[k] = lse;
      __syncthreads();
      float ne = 0.f;
      if (mine) {
        const int b   = k - k % 12;
        float2    avg = ce[b];
        for (int q = 1; q < 12; ++q)
          avg.x += ce[b + q].x, avg.y += ce[b + q].y;
        avg.x /= 12.0f, avg.y /= 12.0f;
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (d >= d0 && d < d0 + nd) {
            const float2 pv = cmul(avg, pil[d]);
            const float  dx = y[d].x - pv.x, dy = y[d].y - pv.y;
            ne += dx * dx + dy * dy;
          }
      }
      const float se = wave_sum(e), sr = wave_sum(rs), sn = wave_sum(ne);
      if (lane == 0) {
        float* q = L.part[2 * p + h][wave];
        q[0] = se, q[1] = sr, q[2] = sn;
      }
    }
  }
  __syncthreads();
  // Time alignment: the (port, hop) searches, one wavefront each.
  for (int c = wave; c < nports * nh; c += 4) {
    const float ta = hop_time_alignment(L.ce[c / nh][c % nh], M, [](int i) { return i; }, lane);
    if (lane == 0)
      L.ta[c] = ta;
  }
  __syncthreads();
  pucch_csi_sum csi;
  float         noise_mine = 0.f;
  for (int p = 0; p < nports; ++p) {
    float epre = 0.f, rsrp = 0.f, noise = 0.f, ta = 0.f;
    for (int h = 0; h < nh; ++h) {
      const float(*q)[3] = L.part[2 * p + h];
      epre += ((q[0][0] + q[1][0]) + q[2][0]) + q[3][0];
      rsrp += (((q[0][1] + q[1][1]) + q[2][1]) + q[3][1]) / (float)lay.ndm[h];
      noise += ((((q[0][2] + q[1][2]) + q[2][2]) + q[3][2]) / (float)M) * 12.0f;
      ta += L.ta[p * nh + h];
    }
    const port_csi c = finish_port(epre, rsrp, noise, ta, M * ndm_all, 12, ndm_all, hop, j.numerology);
    csi.add(c, p == 0);
    if (p == tid)
      noise_mine = c.noise;
  }
  if (est_out) {
    float* eo = est_out + j.est_offset;
    if (mine)
      for (int c = 0; c < nports * nh; ++c) {
        const float2 v = L.ce[c / nh][c % nh][k];
        eo[2 * (c * M + k)] = v.x, eo[2 * (c * M + k) + 1] = v.y;
      }
    if (tid < nports)
      eo[2 * nports * nh * M + tid] = noise_mine;
  }

  // ---- data symbols
  const cplx* tw    = reinterpret_cast<const cplx*>(tws[j.nof_prb]); // the context's table, as for miphy_transform_deprecode_batch
  const float scale = tp_scale(M);
  const int   per   = lay.per_symbol;
  int         r     = 0; // data symbols in front of this one
  for (int i = 0; i < nsym; ++i) {
    if ((lay.dmrs >> i) & 1u)
      continue;
    const int  h = i >= lay.split;
    tp_var_acc acc;
    if (mine) {
      float2 hh[1][4], y[4], xo[1];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        hh[0][p] = p < nports ? L.ce[p][h][k] : make_float2(0.f, 0.f);
        y[p]     = p < nports ? g[((size_t)p * 14 + s + i) * nsc + 12 * prb[h] + k] : make_float2(0.f, 0.f);
      }
      zf_prepared<1> q;
      zf_prepare<1>(hh, nports, csi.noise0, 1.0f, q);
      zf_apply<1>(hh, nports, y, q, xo);
      tp_put(L.x, k, xo[0], q.nvar[0], acc);
    }
    float v = tp_deprecode_symbol(L.x, M, tw, acc, L.red, tid);
    if (tid < per) {
      float2 d;
      if (f4) {
        const int step = occ == 2 ? 2 * j.occ_index : j.occ_index; // conj(w_n) of run q is j^(step q)
        d              = tp_symbol(L.x, tid, scale);
        for (int q = 1; q < occ; ++q) {
          const float2 t = mul_j_pow(tp_symbol(L.x, tid + q * per, scale), step * q);
          d              = make_float2(d.x + t.x, d.y + t.y);
        }
        const float sc = 1.0f / (float)occ;
        d              = make_float2(d.x * sc, d.y * sc);
        v              = v * sc;
      } else {
        d = tp_symbol(L.x, tid, scale);
      }
      const unsigned idx = (unsigned)(r * per + tid);
      int            l[8];
      if (lay.Qm == 2) {
        demod_symbol<2, false>(d.x, d.y, v, idx, nullptr, l);
        const uint32_t c = L.scr[(2 * idx) >> 5] >> ((2 * idx) & 31u);
        L.llr[2 * idx]     = (int8_t)((c & 1u) ? -l[0] : l[0]);
        L.llr[2 * idx + 1] = (int8_t)((c & 2u) ? -l[1] : l[1]);
      } else {
        demod_symbol<1, false>(d.x, d.y, v, idx, nullptr, l);
        const uint32_t c = L.scr[idx >> 5] >> (idx & 31u);
        L.llr[idx]       = (int8_t)((c & 1u) ? -l[0] : l[0]);
      }
    }
    ++r;
    __syncthreads(); // the buffer is free for the next symbol, the soft bits are in LDS
  }

  int8_t* dst = K > 11 ? llr_long : llr_out;
  if (dst)
    for (int i = tid; i < lay.E; i += TP_THREADS)
      dst[j.llr_offset + i] = L.llr[i];
  uint8_t status = 0; // above 11 bits: 0 until the polar decoder behind this kernel stores the CRC verdict over it
  if (K <= 11 && wave == 0) {
    uci_short_block_field(K, (uint32_t)lay.Qm, (uint32_t)lay.E, L.llr, payload + j.payload_offset, &L.status, (uint32_t)lane); // the verdict by lane 0, read by lane 0
    status = L.status;
  }
  if (tid == 0)
    pucch_write_result(results[blockIdx.x], csi, nports, status, 0.f);
}

} // namespace

extern "C" int miphy_pucch_f34_info(const miphy_pucch_f34_job* job, miphy_pucch_f34_info_t* out)
{
  MIPHY_REQUIRE(job && out, "miphy_pucch_f34_info: null argument");
  f34_layout lay;
  if (const int rc = f34_check("miphy_pucch_f34_info", 0, *job, lay))
    return rc;
  out->dmrs_symbols_mask = lay.dmrs << job->start_symbol;
  for (int h = 0; h < 2; ++h)
    out->nof_dmrs_symbols[h] = (uint32_t)lay.ndm[h], out->nof_data_symbols[h] = (uint32_t)lay.ndata[h];
  out->M = (uint32_t)lay.M, out->E = (uint32_t)lay.E;
  out->polar = (uint32_t)job->nof_harq_ack + job->nof_sr + job->nof_csi_part1 > 11;
  return MIPHY_OK;
}

extern "C" int miphy_pucch_process_f34_batch(miphy_ctx* ctx, const miphy_pucch_f34_job* jobs, uint32_t n, uint32_t list_size, const float* grid, uint8_t* payload,
                                             miphy_pucch_result* results, int8_t* llr_out, float* est_out, void* stream)
{
  static const char* const who = "miphy_pucch_process_f34_batch";
  MIPHY_REQUIRE(ctx && jobs && grid && payload && results, "%s: null argument", who);
  MIPHY_REQUIRE(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "%s: list size %u not in {1,2,4,8}", who, list_size);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 PDUs per call", who);
  // Every job is checked before anything is enqueued; the PDUs above 11 bits become the polar decoder's fields, in job order.
  std::vector<miphy_pucch_long_pdu> longs;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pucch_f34_job& j = jobs[i];
    f34_layout                 lay;
    if (const int rc = f34_check(who, i, j, lay))
      return rc;
    const uint32_t K = (uint32_t)j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
    if (K > 11)
      longs.push_back({i, K, (uint32_t)lay.E});
  }
  hipStream_t             s   = (hipStream_t)stream;
  const gold_tables*      gt  = nullptr;
  const float* const*     tws = nullptr;
  miphy_pucch_long_staged st;
  int                     rc;
  if ((rc = miphy_get_gold_tables(ctx, &gt)) || (rc = miphy_tp_twiddles(ctx, &tws)) || (rc = miphy_pucch_stage_long(ctx, jobs, n, longs, F34_MAX_LLR, llr_out, s, st)))
    return rc;
  hipLaunchKernelGGL(pucch_f34_kernel, dim3(n), dim3(TP_THREADS), 0, s, (const miphy_pucch_f34_job*)st.d_jobs, gt, tws, (const float2*)grid, payload, results, llr_out,
                     st.llr_long, est_out);
  MIPHY_HIP_CHECK(hipGetLastError());
  if (st.fields.empty())
    return MIPHY_OK;
  // Behind the kernel on the same stream: the decoder's verdict lands on the status byte after the kernel wrote the record.
  return miphy_uci_polar_decode_fields(who, ctx, st.fields.data(), (uint32_t)st.fields.size(), list_size, st.llr_long, payload, (uint8_t*)results,
                                       st.status_at.data(), s);
}
