// PUCCH processor, formats 1 and 2: srsran::pucch_processor_impl::process (pucch_processor_impl.cpp:28-189) for a batch of PDUs that
// share one device grid. One wavefront per PDU runs the whole chain of the reference for it:
//  - pilots: format 1 -- the length-12 low-PAPR sequence of group u = n_id mod 30 (TS 38.211 Table 5.2.2.2-2, tables/nr_low_papr_tables.h)
//    at the cyclic shift of each symbol (pucch_helper.h:get_alpha_index, n_cs from the Gold sequence of c_init = n_id) times the OCC
//    w_i(m) of the symbol's hop (pucch_orthogonal_sequence.h); format 2 -- QPSK of the Gold sequence of
//    c_init = ((14 n_slot + l + 1)(2 n_id_0 + 1) 2^17 + 2 n_id_0) mod 2^31 advanced by 8 starting_prb, subcarriers {1, 4, 7, 10};
//  - per receive port and hop, port_channel_estimator_average_impl.cpp:97-347: LS over the DM-RS symbols, EPRE, RSRP, noise against the
//    average over one PRB, time alignment, linear interpolation (format 2: offset 1, stride 3, the reference's running sum); the CSI is
//    averaged linearly over the ports (channel_estimation.h:211-233);
//  - format 1: pucch_detector_impl::detect on the first port (ZF 1x1, w* per hop with the hop's own length, conj(r_uv) with the
//    data-symbol cyclic shifts, average, detect_bits, threshold 2.33, the SR-only rule);
//  - format 2: pucch_demodulator_impl::demodulate (ZF 1xN with the noise variance of the first port, QPSK soft demapping with the
//    quantisation of the PUSCH demodulator, descrambling with c_init = rnti 2^15 + n_id) into LDS, then the short-block detector of
//    uci_device.h by the same wavefront;
//  - format 2 above 11 bits (miphy_pucch_process_batch_ex only): the same chain up to the soft bits, which leave the kernel; the
//    polar decoder of uci_polar.hip takes them as one UCI field per PDU behind the kernel on the same stream and stores its CRC
//    verdict over the status byte of the PDU's record. The kernel holds no second copy of the polar recursion.
// Time alignment: the reference takes the peak of |IDFT_4096| of the LS estimates inside +-HALF_CP taps. With at most 12 (format 1) or
// 64 (format 2) pilots per hop, the 288 taps of the window are evaluated directly (a few per lane) instead of the whole transform;
// the magnitude does not depend on where the pilots sit in the grid, so the pilots are placed from subcarrier 0 of the hop.
// Floating point: the reference's operation order where it matters for the LLRs (equaliser and demapper as in pusch_demod.hip, exact
// division); the reference's AVX2 equaliser uses an approximate reciprocal, so its equalised values differ from these by up to
// about 4e-4 relative per element: the format-1 metric by up to about 2e-3 relative on noisy channels, the format-2 soft bits by one
// quantisation step at most.
#include "demod_device.h"
#include "gold_device.h"
#include "miphy_ext.h"
#include "pucch_device.h"
#include "tables/nr_demod_tables.h"
#include "tables/nr_low_papr_tables.h"
#include "uci_device.h"
#include "uci_polar_info.h"
#include <cmath>
#include <vector>

// The reference's assertions for one PDU (pucch_processor_impl.cpp:191-285, pucch_detector_impl.cpp:155-186; the detector's w*
// table asserts i < N for the data-symbol count N of every hop). Format 2's code rate (at most 11 bits over 16 nof_prb nof_symbols
// >= 16 soft bits) never exceeds 0.8. long_ok: format 2 above 11 bits passes too (whether the polar framing takes its bits in its
// soft bits is the host's check, uci_polar_frame).
__host__ __device__ static inline bool miphy_pucch_job_ok(const miphy_pucch_job& j, bool long_ok = false)
{
  if (j.nof_ports < 1 || j.nof_ports > 4 || j.numerology > 4 || j.slot >= (10u << j.numerology) || j.start_symbol + j.nof_symbols > 14)
    return false;
  if (j.bwp_start_rb + j.bwp_size_rb > j.grid_nprb || j.grid_nprb > 275)
    return false;
  if (j.format == 1) {
    if (j.nof_symbols < 4 || j.start_symbol > 10 || j.time_domain_occ > 6 || j.nof_harq_ack > 2 || j.initial_cyclic_shift > 11 || j.n_id > 1023)
      return false;
    if (j.starting_prb >= j.bwp_size_rb || (j.intra_slot_hopping && j.second_hop_prb >= j.bwp_size_rb))
      return false;
    const unsigned nd = j.nof_symbols / 2, pre = j.intra_slot_hopping ? j.nof_symbols / 4 : nd;
    if (j.time_domain_occ >= pre || (j.intra_slot_hopping && j.time_domain_occ >= nd - pre))
      return false;
    return true;
  }
  if (j.format == 2) {
    const unsigned K = j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
    return j.nof_symbols >= 1 && j.nof_symbols <= 2 && j.nof_prb >= 1 && j.nof_prb <= 16 && j.starting_prb + j.nof_prb <= j.bwp_size_rb &&
           !j.intra_slot_hopping && j.nof_csi_part2 == 0 && K >= 3 && (K <= 11 || long_ok);
  }
  return false;
}

namespace {

// TS 38.211 Table 6.3.2.4.1-2: phi of w_i(m) = exp(j 2 pi phi / N), [N - 1][i][m].
__constant__ uint8_t OCC_PHI[7][7][7] = {
    {{0}},
    {{0, 0}, {0, 1}},
    {{0, 0, 0}, {0, 1, 2}, {0, 2, 1}},
    {{0, 0, 0, 0}, {0, 2, 0, 2}, {0, 0, 2, 2}, {0, 2, 2, 0}},
    {{0, 0, 0, 0, 0}, {0, 1, 2, 3, 4}, {0, 2, 4, 1, 3}, {0, 3, 1, 4, 2}, {0, 4, 3, 2, 1}},
    {{0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5}, {0, 2, 4, 0, 2, 4}, {0, 3, 0, 3, 0, 3}, {0, 4, 2, 0, 4, 2}, {0, 5, 4, 3, 2, 1}},
    {{0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6}, {0, 2, 4, 6, 1, 3, 5}, {0, 3, 6, 2, 5, 1, 4}, {0, 4, 1, 5, 2, 6, 3}, {0, 5, 3, 1, 6, 4, 2},
     {0, 6, 5, 4, 3, 2, 1}}};

// w_i(m) of a sequence of length n (pucch_orthogonal_sequence.h; indices beyond the table give 1 there).
__device__ __forceinline__ float2 occ_value(int n, int i, int m, bool conj_)
{
  const int ph = i < n ? OCC_PHI[n - 1][i][m] : 0;
  float     s, c;
  sincosf(PUCCH_TWOPI * (float)ph / (float)n, &s, &c);
  return make_float2(c, conj_ ? -s : s);
}

struct f1_lds {
  float2 pil[7][12];    // DM-RS pilots per DM-RS symbol
  float2 ce[2][12];     // first port: channel estimate per hop
  float2 lse[12];
  int    alpha[14];     // cyclic-shift index per symbol of the allocation
};

struct f2_lds {
  float2   pil[2][64];
  float2   lse[64];
  float2   ce[4][192];  // per port, 12 nof_prb subcarriers
  uint32_t dmrs_bits[2][4];
  uint32_t scr[16];
  int8_t   llr[512];
  uint8_t  status;
};

// Format 1 of one PDU by its wavefront: the estimate of every port into csi, the detector on the first port.
__device__ __forceinline__ void f1_receive(f1_lds& L, const miphy_pucch_job& j, const gold_tables& gt, const float2* g, int nsc, int lane, uint8_t* __restrict__ payload,
                                           pucch_csi_sum& csi, uint8_t& status, float& det_metric)
{
#pragma clang fp contract(off)
  const int  s = j.start_symbol, nsym = j.nof_symbols, nports = j.nof_ports;
  const bool hop = j.intra_slot_hopping != 0;
  const int  prb0 = j.bwp_start_rb + j.starting_prb, prb1 = j.bwp_start_rb + (hop ? j.second_hop_prb : j.starting_prb);
  const int  u      = j.n_id % 30;
  // Cyclic shift of every symbol of the allocation.
  if (lane < nsym)
    L.alpha[lane] = pucch_alpha(gt, j.n_id, j.slot, (uint32_t)(s + lane), j.initial_cyclic_shift);
  __syncthreads();
  // DM-RS on the even symbols of the allocation; the hop starts at s + nsym / 2.
  const int half   = nsym / 2;
  const int ndm    = (nsym + 1) / 2;
  const int ndm0   = hop ? (half + 1) / 2 : ndm; // even offsets below nsym / 2
  for (int i = lane; i < ndm * 12; i += 64) {
    const int    k = i / 12, e = i - 12 * (i / 12);
    const int    h = k >= ndm0, m = h ? k - ndm0 : k, np = h ? ndm - ndm0 : ndm0;
    const float2 w = occ_value(np, j.time_domain_occ, m, false);
    const float* r = NR_LOW_PAPR12[u][L.alpha[2 * k]][e];
    L.pil[k][e]    = cmul(make_float2(r[0], r[1]), w);
  }
  __syncthreads();
  for (int p = 0; p < nports; ++p) {
    float epre = 0.f, rsrp = 0.f, noise = 0.f, ta = 0.f;
    for (int h = 0; h < (hop ? 2 : 1); ++h) {
      const int k0 = h ? ndm0 : 0, nd = h ? ndm - ndm0 : ndm0;
      float2    lse = make_float2(0.f, 0.f);
      float     e   = 0.f;
      const float2* row = g + (size_t)p * 14 * nsc + 12 * (h ? prb1 : prb0) + (lane < 12 ? lane : 0);
      float2        y[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (k >= nd)
          break;
        y[k] = lane < 12 ? row[(size_t)(s + 2 * (k0 + k)) * nsc] : make_float2(0.f, 0.f);
        const float2 pr = lane < 12 ? cmulc(y[k], L.pil[k0 + k][lane]) : make_float2(0.f, 0.f);
        lse.x += pr.x, lse.y += pr.y;
        e += y[k].x * y[k].x + y[k].y * y[k].y;
      }
      epre += wave_sum(e);
      rsrp += wave_sum(lse.x * lse.x + lse.y * lse.y) / (float)nd;
      const float sc = 1.0f / (float)nd;
      lse.x *= sc, lse.y *= sc;
      if (lane < 12)
        L.lse[lane] = lse;
      // Noise against the average over the PRB (window of 12 pilots).
      const float2 avg = make_float2(wave_sum(lse.x) / 12.0f, wave_sum(lse.y) / 12.0f);
      float        ne  = 0.f;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (k < nd && lane < 12) {
          const float2 pv = cmul(avg, L.pil[k0 + k][lane]);
          const float  dx = y[k].x - pv.x, dy = y[k].y - pv.y;
          ne += dx * dx + dy * dy;
        }
      }
      noise += wave_sum(ne);
      __syncthreads();
      ta += hop_time_alignment(L.lse, 12, [](int i) { return i; }, lane);
      if (p == 0 && lane < 12)
        L.ce[h][lane] = lse;
      __syncthreads();
    }
    const port_csi c = finish_port(epre, rsrp, noise, ta, 12 * ndm, 12, ndm, hop, j.numerology);
    csi.add(c, p == 0);
  }

  // Detector on the first port: data on the odd symbols, nsym / 4 of them before the hop when hopping.
  const int   nd = nsym / 2, pre = hop ? nsym / 4 : nd;
  float2      acc = make_float2(0.f, 0.f);
  float       nv_sum = 0.f;
  const bool  nv_ok = isnormal(csi.noise0) && csi.noise0 > 0.f;
  for (int i = lane; i < 12 * nd; i += 64) {
    const int    d = i / 12, e = i - 12 * (i / 12);
    const int    h = d >= pre, m = h ? d - pre : d, np = h ? nd - pre : pre;
    const int    l = s + 1 + 2 * d;
    const float2 y  = g[(size_t)l * nsc + 12 * (h ? prb1 : prb0) + e];
    const float2 hc = L.ce[h][e];
    const float  d_pinv = hc.x * hc.x + hc.y * hc.y;
    float2       z  = make_float2(0.f, 0.f);
    float        nv = INFINITY;
    if (isnormal(d_pinv) && nv_ok) {
      const float rcp = 1.0f / d_pinv;
      const float2 t  = cmulc(y, hc);
      z               = make_float2(t.x * rcp, t.y * rcp);
      nv              = rcp * csi.noise0;
    }
    const float2 w = occ_value(np, j.time_domain_occ, m, true);
    const float* r = NR_LOW_PAPR12[u][L.alpha[1 + 2 * d]][e];
    const float2 v = cmulc(cmul(z, w), make_float2(r[0], r[1]));
    acc.x += v.x, acc.y += v.y;
    nv_sum += nv;
  }
  const float nrep = (float)(12 * nd);
  const float dre = wave_sum(acc.x) / nrep, dim = wave_sum(acc.y) / nrep;
  const float eq_nv = (wave_sum(nv_sum) / nrep) / nrep;
  // detect_bits (pucch_detector_impl.cpp:189-207)
  const int nbits = j.nof_harq_ack ? j.nof_harq_ack : 1;
  float     m1 = dre + dim;
  unsigned  bits = m1 > 0 ? 0u : 3u;
  m1             = fabsf(m1);
  float     m2 = dre - dim;
  unsigned  bits2 = m2 > 0 ? 2u : 1u;
  m2              = fabsf(m2);
  float     metric;
  unsigned  b;
  if (nbits > 1 && m2 > m1)
    b = bits2, metric = m2 / sqrtf(eq_nv);
  else
    b = bits, metric = m1 / sqrtf(eq_nv);
  if (lane == 0) {
    const bool ok = metric > 2.33f;
    det_metric = metric / 2.33f;
    status     = !ok ? MIPHY_UCI_STATUS_INVALID : (j.nof_harq_ack > 0 || (b & 1u) == 0 ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_UNKNOWN);
    for (int k = 0; k < j.nof_harq_ack; ++k)
      payload[j.payload_offset + k] = (b >> k) & 1u;
  }
}

// Format 2 of one PDU by its wavefront: the estimate of every port into csi, the demodulator, and up to 11 bits the short-block detector.
__device__ __forceinline__ void f2_receive(f2_lds& L, const miphy_pucch_job& j, const gold_tables& gt, const float2* g, int nsc, int lane, uint8_t* __restrict__ payload,
                                           int8_t* __restrict__ llr_out, int8_t* __restrict__ llr_long, pucch_csi_sum& csi, uint8_t& status)
{
#pragma clang fp contract(off)
  const int s = j.start_symbol, nsym = j.nof_symbols, nports = j.nof_ports;
  const int nprb = j.nof_prb, prb0 = j.bwp_start_rb + j.starting_prb, npil = 4 * nprb;
  // DM-RS sequences: 8 nof_prb bits of each symbol's c_init from bit 8 prb0; scrambling sequence: 16 nof_prb nof_symbols bits.
  if (lane < 4 * nsym) {
    const uint32_t l = s + lane / 4, q = lane & 3;
    const uint32_t ci = (uint32_t)(((uint64_t)(14u * j.slot + l + 1u) * (2u * j.n_id_0 + 1u) * 131072u + 2u * j.n_id_0) % 2147483648u);
    L.dmrs_bits[lane / 4][q] = gold_word(gt, ci, 8u * prb0 + 32u * q);
  } else if (lane >= 16 && lane < 16 + (nprb * nsym + 1) / 2) {
    L.scr[lane - 16] = gold_word(gt, (uint32_t)j.rnti * 32768u + j.n_id, 32u * (lane - 16));
  }
  __syncthreads();
  for (int i = lane; i < nsym * npil; i += 64) {
    const int      k = i / npil, m = i - npil * k;
    const uint32_t w = L.dmrs_bits[k][(2 * m) >> 5];
    const float    a = (float)M_SQRT1_2;
    L.pil[k][m]      = make_float2(((w >> ((2 * m) & 31)) & 1u) ? -a : a, ((w >> ((2 * m + 1) & 31)) & 1u) ? -a : a);
  }
  __syncthreads();
  const int pil_sc = 12 * (lane >> 2) + 1 + 3 * (lane & 3); // this lane's pilot subcarrier within the allocation
  for (int p = 0; p < nports; ++p) {
    const float2* row = g + (size_t)p * 14 * nsc + 12 * prb0;
    float2        y[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
    float2        lse  = make_float2(0.f, 0.f);
    float         e    = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < nsym && lane < npil) {
        y[k]            = row[(size_t)(s + k) * nsc + pil_sc];
        const float2 pr = cmulc(y[k], L.pil[k][lane]);
        lse.x += pr.x, lse.y += pr.y;
        e += y[k].x * y[k].x + y[k].y * y[k].y;
      }
    }
    const float epre = wave_sum(e);
    const float rsrp = wave_sum(lse.x * lse.x + lse.y * lse.y) / (float)nsym;
    const float sc   = 1.0f / (float)nsym;
    lse.x *= sc, lse.y *= sc;
    if (lane < npil)
      L.lse[lane] = lse;
    __syncthreads();
    const float ta = hop_time_alignment(L.lse, npil, [](int i) { return 12 * (i >> 2) + 1 + 3 * (i & 3); }, lane);
    // interpolator_linear_impl::interpolate, offset 1, stride 3: the running sum of the reference, one lane.
    if (lane == 0) {
      float2* out = L.ce[p];
      const int nout = 12 * nprb;
      if (npil == 1) {
        for (int i = 0; i < nout; ++i)
          out[i] = L.lse[0];
      } else {
        int i_out = 1, i_in = 0;
        out[0] = out[1] = L.lse[0];
        for (int next = i_out + 3; next < nout; next += 3) {
          const float2 jump = make_float2((L.lse[i_in + 1].x - L.lse[i_in].x) / 3.0f, (L.lse[i_in + 1].y - L.lse[i_in].y) / 3.0f);
          float2       val  = out[i_out];
          for (int t = 1; t <= 3; ++t) {
            val.x += jump.x, val.y += jump.y;
            out[i_out + t] = val;
          }
          i_out = next;
          ++i_in;
        }
        for (int i = i_out + 1; i < nout; ++i)
          out[i] = L.lse[i_in];
      }
    }
    __syncthreads();
    // Format 2 has at most two DM-RS symbols, and with fewer than three the reference replaces the noise estimate by EPRE / 1000
    // (port_channel_estimator_average_impl.cpp:133-137): finish_port does that, so the residual noise is not measured here.
    const port_csi c = finish_port(epre, rsrp, 0.f, ta, npil * nsym, 4, nsym, false, j.numerology);
    csi.add(c, p == 0);
  }
  // Demodulator: data REs symbol by symbol, PRB by PRB, subcarriers {0, 2, 3, 5, 6, 8, 9, 11}.
  const int  nre   = 8 * nprb * nsym;
  const bool nv_ok = isnormal(csi.noise0) && csi.noise0 > 0.f;
  for (int re = lane; re < nre; re += 64) {
    const int k = re / (8 * nprb), r = re - 8 * nprb * k, q = r >> 3, jj = r & 7;
    const int sc = 12 * q + jj + (jj + 1) / 2; // 0, 2, 3, 5, 6, 8, 9, 11
    float     ch_mod_sq = 0.f, acc_re = 0.f, acc_im = 0.f;
    for (int p = 0; p < nports; ++p) {
      const float2 y = g[((size_t)p * 14 + s + k) * nsc + 12 * prb0 + sc];
      const float2 h = L.ce[p][sc];
      const float  t = h.x * h.x, u = h.y * h.y;
      ch_mod_sq      = ch_mod_sq + (t + u);
      const float aa = y.x * h.x, b = y.y * h.y, cc = y.y * h.x, d = y.x * h.y;
      acc_re = acc_re + (aa + b);
      acc_im = acc_im + (cc - d);
    }
    float z_re = 0.f, z_im = 0.f, nv = INFINITY;
    if (isnormal(ch_mod_sq) && nv_ok) {
      const float rcpd = 1.0f / ch_mod_sq;
      z_re = acc_re * rcpd, z_im = acc_im * rcpd;
      nv   = rcpd * csi.noise0;
    }
    const float rcp = (nv > 0.f) ? 1.0f / nv : 0.0f;
    const uint32_t cw = L.scr[re >> 4];
    const int l0 = demod_quantize((NR_DEMOD_QPSK_GAIN * z_re) * rcp, 120.0f / 24.f);
    const int l1 = demod_quantize((NR_DEMOD_QPSK_GAIN * z_im) * rcp, 120.0f / 24.f);
    L.llr[2 * re]     = (int8_t)(((cw >> ((2 * re) & 31)) & 1u) ? -l0 : l0);
    L.llr[2 * re + 1] = (int8_t)(((cw >> ((2 * re + 1) & 31)) & 1u) ? -l1 : l1);
  }
  __syncthreads();
  const uint32_t K   = j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
  int8_t*        dst = K > 11 ? llr_long : llr_out;
  if (dst)
    for (int i = lane; i < 2 * nre; i += 64)
      dst[j.llr_offset + i] = L.llr[i];
  if (K <= 11) {
    uci_short_block_field(K, 2, 2 * nre, L.llr, payload + j.payload_offset, &L.status, lane); // the verdict by lane 0, read by lane 0
    status = L.status;
  } // above 11 bits: status 0 until the polar decoder behind this kernel stores the CRC verdict over it
}

__global__ void __launch_bounds__(64) pucch_kernel(const miphy_pucch_job* __restrict__ jobs, uint32_t n, const gold_tables* __restrict__ gt,
                                                   const float2* __restrict__ grid, uint8_t* __restrict__ payload,
                                                   miphy_pucch_result* __restrict__ results, int8_t* __restrict__ llr_out,
                                                   int8_t* __restrict__ llr_long)
{
#pragma clang fp contract(off)
  __shared__ union {
    f1_lds f1;
    f2_lds f2;
  } sm;
  const int      lane = threadIdx.x;
  const uint32_t pdu  = blockIdx.x;
  if (pdu >= n)
    return;
  const miphy_pucch_job j = jobs[pdu];
  // Device jobs the host could not check: nothing is written. Format 2 above 11 bits passes only where the caller gave its soft bits
  // a place (llr_long, miphy_pucch_process_batch_ex).
  if (!miphy_pucch_job_ok(j, llr_long != nullptr))
    return;
  const int     nsc = 12 * (int)j.grid_nprb;
  const float2* g   = grid + j.grid_offset;
  pucch_csi_sum csi;
  uint8_t       status     = 0;
  float         det_metric = 0.f;
  if (j.format == 1)
    f1_receive(sm.f1, j, *gt, g, nsc, lane, payload, csi, status, det_metric);
  else
    f2_receive(sm.f2, j, *gt, g, nsc, lane, payload, llr_out, llr_long, csi, status);
  if (lane == 0)
    pucch_write_result(results[pdu], csi, j.nof_ports, status, det_metric);
}

} // namespace

extern "C" int miphy_pucch_process_batch(miphy_ctx* ctx, const miphy_pucch_job* jobs, int jobs_on_device, uint32_t n, const float* grid, uint8_t* payload,
                                         miphy_pucch_result* results, int8_t* llr_out, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && grid && payload && results, "miphy_pucch_process_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "pucch_process: at most 2^24 PDUs per call");
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i)
      MIPHY_REQUIRE(miphy_pucch_job_ok(jobs[i]), "pucch_process: job %u: invalid PDU (format %u, %u symbols from %u, %u ports)", i, jobs[i].format,
                    jobs[i].nof_symbols, jobs[i].start_symbol, jobs[i].nof_ports);
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  rc                 = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pucch_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  hipLaunchKernelGGL(pucch_kernel, dim3(n), dim3(64), 0, s, (const miphy_pucch_job*)d_jobs, n, gt, (const float2*)grid, payload, results, llr_out,
                     (int8_t*)nullptr);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_pucch_process_batch_ex(miphy_ctx* ctx, const miphy_pucch_job* jobs, uint32_t n, uint32_t list_size, const float* grid, uint8_t* payload,
                                            miphy_pucch_result* results, int8_t* llr_out, void* stream)
{
  static const char* const who = "miphy_pucch_process_batch_ex";
  MIPHY_REQUIRE(ctx && jobs && grid && payload && results, "%s: null argument", who);
  MIPHY_REQUIRE(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "%s: list size %u not in {1,2,4,8}", who, list_size);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 PDUs per call", who);
  // Every job is checked before anything is enqueued; the long PDUs go to the polar decoder, in job order.
  std::vector<miphy_pucch_long_pdu> longs;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pucch_job& j = jobs[i];
    MIPHY_REQUIRE(j.format != 2 || j.nof_csi_part2 == 0, "%s: job %u: CSI part 2 (%u bits) is not decoded on PUCCH", who, i, j.nof_csi_part2);
    MIPHY_REQUIRE(miphy_pucch_job_ok(j, true), "%s: job %u: invalid PDU (format %u, %u symbols from %u, %u ports)", who, i, j.format, j.nof_symbols,
                  j.start_symbol, j.nof_ports);
    const uint32_t K = j.nof_harq_ack + j.nof_sr + j.nof_csi_part1;
    if (j.format != 2 || K <= 11)
      continue;
    const uint32_t    E = 16u * j.nof_prb * j.nof_symbols;
    uci_polar_framing f;
    if (const int rc = uci_polar_frame_or_error(who, i, K, E, f))
      return rc;
    longs.push_back({i, K, E});
  }
  hipStream_t             s  = (hipStream_t)stream;
  const gold_tables*      gt = nullptr;
  miphy_pucch_long_staged st;
  int                     rc;
  if ((rc = miphy_get_gold_tables(ctx, &gt)) || (rc = miphy_pucch_stage_long(ctx, jobs, n, longs, 512, llr_out, s, st))) // E <= 512
    return rc;
  hipLaunchKernelGGL(pucch_kernel, dim3(n), dim3(64), 0, s, (const miphy_pucch_job*)st.d_jobs, n, gt, (const float2*)grid, payload, results, llr_out, st.llr_long);
  MIPHY_HIP_CHECK(hipGetLastError());
  if (st.fields.empty())
    return MIPHY_OK;
  // Behind the kernel on the same stream: the decoder's verdict lands on the status byte after the kernel wrote the record.
  return miphy_uci_polar_decode_fields(who, ctx, st.fields.data(), (uint32_t)st.fields.size(), list_size, st.llr_long, payload, (uint8_t*)results,
                                       st.status_at.data(), s);
}
