// PDSCH modulator and PDSCH DM-RS mapping, the transmit-side counterpart of pusch_demod.hip; PDCCH, SS/PBCH block and NZP-CSI-RS mapping.
//
// Behaviour contract:
//   lib/phy/upper/channel_processors/pdsch_modulator_impl.cpp:30-282 (scrambling c_init = rnti * 2^15 + q * 2^14 + n_id, modulation,
//   optional scaling, mapping to the allocated PRBs in ascending order skipping the DM-RS pattern of the bandwidth part and the
//   reserved RE patterns), lib/phy/upper/channel_modulation/modulation_mapper_impl.cpp:31-146 (constellation = integer level *
//   sqrtf(1 / average power)), lib/phy/upper/signal_processors/dmrs_pdsch_processor_impl.cpp:30-169 + dmrs_helper.h:44-96.
// The 23.5 reference maps one layer of one codeword to ascending PRBs and cannot do more: its layer mapper indexes out of bounds for more than one
// layer (pdsch_modulator_impl.cpp:80-103), its non-contiguous mapping path writes a single PRB (map_to_prb_other), and it joins its precoder
// (channel_precoder_generic.cpp:27-48, precoding_configuration.h) to no modulator. Beyond it the contract is the oracle's orc_pdsch_modulate: the layer
// mapping of TS 38.211 7.3.1.3 and a prb_list walked as given. Every resource element is written once, with the exact single-precision value of the
// reference (level * scale [* scaling]); a precoded one with precode_sum of those values.
//
// Two paths. The one-layer path, miphy_pdsch_modulate_batch (and the prepared plan of pdsch_proc.hip): pdsch_seq_kernel, one workgroup per
// transmission with x1 from the table, and pdsch_mod_kernel. The layered path, one codeword on 1..4 layers, with three front doors that differ in what a
// job carries and in nothing else:
//   miphy_pdsch_modulate_layers_batch    miphy_pdsch_mod_layers_job: layer ly on grid port ports[ly], PRBs of rb_mask ascending
//   miphy_pdsch_modulate_mapped_batch    ... and a PRB list in mapping order: the interleaved VRB-to-PRB mapping of TS 38.211 7.3.1.6
//                                        (miphy_vrb_to_prb_list) or any other order
//   miphy_pdsch_modulate_precoded_batch  ... and a miphy_precoding: the L symbols of an element through the weight matrix of its PRG onto antenna ports
// and a fourth for one or two codewords on 1..8 layers (TS 38.211 Table 7.3.1.3-1), which shares the same bodies:
//   miphy_pdsch_modulate_codewords_batch miphy_pdsch_mod_codewords_job: a mapped job plus codeword 1 and eight ports. pdsch_seq_codewords_kernel generates
//                                        both sequences of a job (the codeword is one more grid dimension), pdsch_mod_codewords_kernel maps codeword 0 and
//                                        behind it codeword 1 in one workgroup: one symbol setup, one prefix and one launch pair for both
// Behind the doors: one host loop (pdsch_modulate_layered: job, list, precoding, in that order), one enqueue (miphy_pdsch_modulate_layered_enqueue: staging,
// the scratch of pdsch_layers_scratch_of, two launches), one sequence body (pdsch_seq_layers_body: chunks of the L-fold sequence with both registers
// jumped; chunk 0 holds a device-resident job, its list and its precoding to the rules and says so in info[15]) and one mapping body
// (pdsch_mod_layers_body, parametrised on the sink: pdsch_no_precoding or pdsch_precoder). The __global__ kernels of a door (pdsch_seq_layers_kernel /
// _mapped_ / _precoded_, pdsch_mod_layers_kernel / _mapped_ / _precoded_) only pick the parts of its job.
// Both paths share the helpers: a sequence kernel leaves, through pdsch_count_symbols, the data elements of the transmission before every OFDM
// symbol; a mapping workgroup (transmission, OFDM symbol) fills a pdsch_symbol_lds through pdsch_symbol_setup and maps its elements through
// pdsch_layers_fast (16QAM / 256QAM on aligned codewords) or pdsch_map_elements (everything else). Which REs carry data is stated once, in
// pdsch_keep_rule_of and pdsch_keep_mask, for every kernel and the host's count. What a job, a list and a precoding must satisfy is stated once each
// (PDSCH_MOD_FIELD_RULES, PDSCH_MOD_LIST_RULES / PDSCH_MOD_LIST_ENTRY_RULES, PDSCH_PRECODING_RULES, PDSCH_MOD_CODEWORDS_RULES / PDSCH_MOD_CODEWORDS_SIZE_RULES),
// for the kernels' predicate and the host's messages.
// DM-RS: dmrs_pdsch_kernel and, behind a precoding, dmrs_pdsch_precoded_kernel generate an OFDM symbol through the same helpers (dmrs_pdsch_symbol_setup,
// dmrs_pdsch_re_of, dmrs_pdsch_weight) and differ in their store loop; channel_precode_kernel is the precoder as a block of its own, and precode_sum
// holds the arithmetic for all three precoding kernels.
#include "gold_device.h"
#include "mod_device.h"
#include "miphy_ext.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <type_traits>

namespace {

__host__ __device__ __forceinline__ unsigned dmrs_prb_mask(int type, unsigned cdm)
{
  unsigned m = 0;
  for (unsigned k = 0; k < 12; ++k)
    m |= ((type == 1) ? ((k % 2) < cdm) : ((k % 6) < 2 * cdm)) ? (1u << k) : 0u;
  return m;
}

// What decides which REs of a PRB carry data, read from the job once: on the device into uniform registers, before the first barrier, so that no
// load of a job field waits behind one.
struct pdsch_keep_rule {
  unsigned dmask;                      // the DM-RS pattern within a PRB (dmrs_prb_mask) ...
  unsigned dmrs_syms, bwp0, bwp1;      // ... which applies in these OFDM symbols to the PRBs [bwp0, bwp1)
  unsigned nres, res_re[4], res_sy[4]; // the reserved patterns (at most four): RE mask and OFDM symbols of each
};

__host__ __device__ __forceinline__ pdsch_keep_rule pdsch_keep_rule_of(const miphy_pdsch_mod_job& j)
{
  pdsch_keep_rule k = {};
  k.dmask     = dmrs_prb_mask(j.dmrs_type, j.nof_cdm_groups_without_data);
  k.dmrs_syms = j.dmrs_symbols_mask, k.bwp0 = j.bwp_start_rb, k.bwp1 = k.bwp0 + j.bwp_size_rb;
  k.nres      = j.nof_reserved < 4 ? j.nof_reserved : 4;
#pragma unroll
  for (unsigned r = 0; r < 4; ++r)
    if (r < k.nres) {
      k.res_re[r] = j.reserved[r].re_mask;
      k.res_sy[r] = j.reserved[r].symbols;
    }
  return k;
}

// The REs of PRB rb in OFDM symbol s that carry data, as a 12-bit mask: all but the DM-RS pattern where the symbol carries DM-RS and the PRB lies
// in the bandwidth part, and but the RE masks of the reserved patterns that name the symbol and the PRB. Word w of the PRB mask of pattern r is
// res_prb[r * res_stride + w]: a copy in LDS on the device, the job itself on the host.
__host__ __device__ __forceinline__ unsigned pdsch_keep_mask(const pdsch_keep_rule& k, unsigned s, unsigned rb, const uint64_t* res_prb, unsigned res_stride)
{
  unsigned ex = (((k.dmrs_syms >> s) & 1u) && rb >= k.bwp0 && rb < k.bwp1) ? k.dmask : 0u;
#pragma unroll
  for (unsigned r = 0; r < 4; ++r)
    if (r < k.nres && ((k.res_sy[r] >> s) & 1u) && ((res_prb[r * res_stride + (rb >> 6)] >> (rb & 63)) & 1ull))
      ex |= k.res_re[r];
  return ~ex & 0xfffu;
}

// The PRB masks of a job -- the allocation and the (at most four) reserved patterns -- into LDS; the caller synchronises.
__device__ __forceinline__ void pdsch_load_masks(const miphy_pdsch_mod_job& j, uint64_t* rbm, uint64_t (*resm)[5], int tid)
{
  const int nres = min((int)j.nof_reserved, 4);
  if (tid < 5)
    rbm[tid] = j.rb_mask[tid];
  if (tid >= 32 && tid < 32 + 5 * nres)
    resm[(tid - 32) / 5][(tid - 32) % 5] = j.reserved[(tid - 32) / 5].prb_mask[(tid - 32) % 5];
}

// Allocated-PRB list (compact, ascending) from a 275-bit mask held in LDS; returns the number of allocated PRBs through *count.
__device__ __forceinline__ void build_prb_list(const uint64_t* rbm, int nprb_grid, int first_rb, uint16_t* prb_of, int* count, int tid, int nt)
{
  for (int r = tid; r < nprb_grid; r += nt) {
    const int      wd = r >> 6, bt = r & 63;
    const uint64_t m  = rbm[wd];
    if (r >= first_rb && ((m >> bt) & 1ull)) {
      int idx = __popcll(m & ((1ull << bt) - 1ull));
      for (int w = 0; w < wd; ++w)
        idx += __popcll(rbm[w]);
      prb_of[idx] = (uint16_t)r;
    }
  }
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < 5; ++w)
      c += __popcll(w * 64 < nprb_grid ? (rbm[w] & ((nprb_grid - w * 64 >= 64) ? ~0ull : ((1ull << (nprb_grid - w * 64)) - 1ull))) : 0ull);
    *count = c;
  }
}

// Prologue of the two sequence kernels: the data REs (per layer) of the job in every OFDM symbol of the slot, left in cnt[0..13] behind a barrier.
// The caller turns them into the prefixes the mapping kernel reads: each (transmission, symbol) workgroup of the modulator used to recount all
// earlier symbols itself.
__device__ __forceinline__ void pdsch_count_symbols(const miphy_pdsch_mod_job& j, uint64_t* rbm, uint64_t (*resm)[5], int* cnt, int tid, int nt)
{
  const pdsch_keep_rule keep      = pdsch_keep_rule_of(j);
  const int             nprb_grid = j.grid_nof_prb, s0 = j.start_symbol, s1 = s0 + j.nof_symbols;
  pdsch_load_masks(j, rbm, resm, tid);
  if (tid >= 64 && tid < 78)
    cnt[tid - 64] = 0;
  __syncthreads();
  for (int q = tid; q < 14 * nprb_grid; q += nt) {
    const int s = q / nprb_grid, rb = q - s * nprb_grid;
    if (s < s0 || s >= s1 || !((rbm[rb >> 6] >> (rb & 63)) & 1ull))
      continue;
    atomicAdd(&cnt[s], __popc(pdsch_keep_mask(keep, s, rb, &resm[0][0], 5)));
  }
  __syncthreads();
}

// What a mapping workgroup knows of its OFDM symbol (pdsch_symbol_setup).
struct pdsch_symbol_lds {
  uint16_t prb_of[276];  // the allocated PRBs, ascending
  uint16_t keep_of[276]; // per allocated PRB: 12-bit mask of the REs that carry data in this symbol
  uint16_t off_of[276];  // per allocated PRB: index of its first data RE within the symbol
  uint64_t rbm[5], resm[4][5];
  int      nprb, n_re;   // allocated PRBs, data REs of the symbol
};

// Fills S for OFDM symbol sy of the job, every thread of the workgroup (at least one wavefront) calling; returns the data REs of the symbol.
// list: the nof_list (1 .. 275) allocated PRBs in mapping order, a list that passed pdsch_list_ok (the mapped kernels) -- one coalesced read of
// at most 550 bytes into prb_of[], which keep_of[] and off_of[] then follow; null (a literal from the other kernels, so that the branch
// folds): the PRBs of rb_mask, ascending.
__device__ __forceinline__ int pdsch_symbol_setup(const miphy_pdsch_mod_job& j, int sy, pdsch_symbol_lds& S, int tid, int nt, const uint16_t* list = nullptr,
                                                  int nof_list = 0)
{
  const pdsch_keep_rule keep      = pdsch_keep_rule_of(j);
  const int             nprb_grid = j.grid_nof_prb;
  pdsch_load_masks(j, S.rbm, S.resm, tid);
  if (list) {
    for (int i = tid; i < nof_list; i += nt)
      S.prb_of[i] = list[i];
    if (tid == 0)
      S.nprb = nof_list;
  }
  __syncthreads();
  if (!list)
    build_prb_list(S.rbm, nprb_grid, 0, S.prb_of, &S.nprb, tid, nt);
  __syncthreads();
  const int nprb = S.nprb;
  for (int i = tid; i < nprb; i += nt)
    S.keep_of[i] = (uint16_t)pdsch_keep_mask(keep, sy, S.prb_of[i], &S.resm[0][0], 5);
  __syncthreads();
  // exclusive scan of the per-PRB counts of this symbol (<= 275 entries: one wavefront, 5 entries per lane)
  if (tid < 64) {
    int c[5], sum = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const int i = tid * 5 + q;
      c[q]        = (i < nprb) ? __popc((unsigned)S.keep_of[i]) : 0;
      sum += c[q];
    }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o);
      inc += (tid >= o) ? v : 0;
    }
    int run = inc - sum;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const int i = tid * 5 + q;
      if (i < nprb)
        S.off_of[i] = (uint16_t)run;
      run += c[q];
    }
    if (tid == 63)
      S.n_re = inc;
  }
  __syncthreads();
  return S.n_re;
}

// y = w[0] x[0] + ... + w[n - 1] x[n - 1] (complex, n = 1 .. 4) in the order of channel_precoder_generic.cpp:41-45: the product of the first layer, then
// the others accumulated. A fixed sequence of one multiplication and fused multiply-adds per part, nothing left to the compiler's contraction: the three
// precoding kernels call it, and the same inputs give the same bits in each. A weight 1 + 0j alone returns x[0] bit for bit.
__device__ __forceinline__ float2 precode_sum(const float2* __restrict__ w, const float2 (&x)[4], const int n)
{
  const float2 w0 = w[0];
  float        re = w0.x * x[0].x, im = w0.x * x[0].y;
  re = fmaf(-w0.y, x[0].y, re), im = fmaf(w0.y, x[0].x, im);
#pragma unroll
  for (int ly = 1; ly < 4; ++ly) {
    if (ly >= n)
      break;
    const float2 wl = w[ly];
    re = fmaf(wl.x, x[ly].x, re), im = fmaf(wl.x, x[ly].y, im);
    re = fmaf(-wl.y, x[ly].y, re), im = fmaf(wl.y, x[ly].x, im);
  }
  return make_float2(re, im);
}

// Where the L symbols of a data element go: the sink of a mapping kernel. A sink type says what it stages in LDS ahead of the barriers of
// pdsch_symbol_setup (stage) and how it is built, behind them, from the job (the constructor: lj = the layers job, pc = its precoding and weights = the
// call's weights where the entry point has them, slot = element 0 of the job's grid, nsc = subcarriers of a grid row, staged = what stage returned).
// Without precoding (the modulators of 1..4 layers): layer ly to g[ly], the symbol's row of grid port ports[ly], in the mapping functions themselves.
struct pdsch_no_precoding {
  static constexpr bool on = false;
  float2*               g[4];
  __device__ __forceinline__ static const uint8_t* stage(const miphy_precoding*, int) { return nullptr; }
  __device__ __forceinline__ pdsch_no_precoding(const miphy_pdsch_mod_layers_job& lj, const miphy_precoding*, const float2*, const uint8_t*, float2* slot, int sy,
                                                int nsc)
  {
    const int L = lj.nof_layers;
#pragma unroll
    for (int ly = 0; ly < 4; ++ly)
      g[ly] = slot + ((size_t)lj.ports[ly < L ? ly : 0] * 14 + sy) * nsc;
  }
  __device__ __forceinline__ explicit pdsch_no_precoding(float2* row) : g{row, nullptr, nullptr, nullptr} {} // (one layer: pdsch_mod_kernel)
  // (one codeword of a codewords job: its L layers on its slice of the job's ports, layer ly on the port in byte ly of `ports`)
  __device__ __forceinline__ pdsch_no_precoding(uint32_t ports, int L, float2* slot, int sy, int nsc)
  {
#pragma unroll
    for (int ly = 0; ly < 4; ++ly)
      g[ly] = slot + ((size_t)((ports >> (ly < L ? 8 * ly : 0)) & 0xffu) * 14 + sy) * nsc;
  }
};
// With precoding (pdsch_mod_precoded_kernel): antenna port a = 0 .. P - 1 receives the sum of its row of the matrix of the element's PRG, on the symbol's
// row of grid port ports[a]. The matrix (at most 64 cf_t) is read with plain loads: the twelve REs of a PRB, and with prg_size > 1 their neighbours, read
// the same addresses, which L1 and L2 serve ("precoding").
struct pdsch_precoder {
  static constexpr bool on = true;
  const float2*  W;       // W[0][0][0] of the job
  float2*        sym;     // the OFDM symbol's row of grid port 0
  size_t         pstride; // elements from one grid port to the next
  const uint8_t* ports;   // grid port of each antenna port (a copy in LDS)
  int            P, L;
  unsigned       prg_size;
  __device__ __forceinline__ static const uint8_t* stage(const miphy_precoding* pc, int tid)
  {
    __shared__ uint8_t aports[16];
    if (tid < 16)
      aports[tid] = pc->ports[tid]; // (read behind the barriers of pdsch_symbol_setup)
    return aports;
  }
  __device__ __forceinline__ pdsch_precoder(const miphy_pdsch_mod_layers_job& lj, const miphy_precoding* pc, const float2* weights, const uint8_t* staged, float2* slot,
                                            int sy, int nsc)
      : W(weights + pc->weights_offset), sym(slot + (size_t)sy * nsc), pstride((size_t)14 * nsc), ports(staged), P(pc->nof_ports), L(lj.nof_layers),
        prg_size(pc->prg_size)
  {
  }
  __device__ __forceinline__ void store(const float2 (&x)[4], const int n, const int col) const
  {
    const float2* w = W + (size_t)(((unsigned)col / 12u) / prg_size) * (unsigned)(P * L);
    for (int a = 0; a < P; ++a)
      sym[ports[a] * pstride + col] = precode_sum(w + a * L, x, n);
  }
};

// Bit 0 of each of the mod bytes at cp (one bit per byte, b0 first) gathered into bit t = t-th bit: one wide load where the run of bytes is
// aligned, then bit 0 of every byte through a multiplication ((x & 0x01010101) * 0x01020408 puts bytes 0..3 into bits 24..27).
__device__ __forceinline__ uint32_t gather_bits(const uint8_t* cp, int mod)
{
  uint32_t raw = 0;
  if (mod == 8 && (((uintptr_t)cp) & 7u) == 0) {
    const uint2 v = *reinterpret_cast<const uint2*>(cp);
    raw           = (((v.x & 0x01010101u) * 0x01020408u) >> 24) | ((((v.y & 0x01010101u) * 0x01020408u) >> 24) << 4);
  } else if (mod == 4 && (((uintptr_t)cp) & 3u) == 0) {
    raw = ((*reinterpret_cast<const uint32_t*>(cp) & 0x01010101u) * 0x01020408u) >> 24;
  } else if (mod == 2 && (((uintptr_t)cp) & 1u) == 0) {
    const uint32_t v = *reinterpret_cast<const uint16_t*>(cp);
    raw              = (v & 1u) | ((v >> 7) & 2u);
  } else if (mod == 6 && (((uintptr_t)cp) & 1u) == 0) {
    const uint16_t* c2 = reinterpret_cast<const uint16_t*>(cp);
    const uint32_t  v0 = c2[0], v1 = c2[1], v2 = c2[2];
    raw = (v0 & 1u) | ((v0 >> 7) & 2u) | ((v1 & 1u) << 2) | ((v1 >> 5) & 8u) | ((v2 & 1u) << 4) | ((v2 >> 3) & 32u);
  } else {
    for (int t = 0; t < mod; ++t)
      raw |= (uint32_t)(cp[t] & 1u) << t;
  }
  return raw;
}

// The elements of one OFDM symbol, one at a time, on L layers (a literal 1 from the one-layer kernel, so that the layer loop folds). TS 38.211
// 7.3.1.3: x^(ly)(i) = d(L i + ly), so the resource element of rank i_re in the transmission (prefix = its rank at the start of the symbol) owns
// the codeword symbols L i_re .. L i_re + L - 1: L mod consecutive bytes of the codeword and L mod <= 32 consecutive bits of the scrambling
// sequence, one 64-bit window of two sequence words. Bit offsets stay in 32 bits: the longest codeword is 4 layers x 275 PRB x 12 x 14
// symbols x 8 bits = 1 478 400 bits. The element's symbols go to the sink `out`. This function and pdsch_layers_fast take their
// arguments by reference, as a lambda captures them: taken by value, both mapping kernels come out two to four registers above the 80 that six
// waves per SIMD allow (tools/kernel_resources.sh).
template <class PRE>
__device__ __forceinline__ void pdsch_map_elements(const pdsch_symbol_lds& S, const int& L, const int& mod, const int& prefix, const uint32_t* const& seq,
                                                   const uint8_t* const& cw, const PRE& out, const bool& scale, const float& scaling, const int& tid, const int& nt)
{
  const int      nprb = S.nprb;
  const uint32_t mask = (1u << mod) - 1u;
  for (int idx = tid; idx < nprb * 12; idx += nt) {
    const int      i = idx / 12, k = idx - i * 12;
    const unsigned keep = S.keep_of[i];
    if (!((keep >> k) & 1u))
      continue;
    const int      j  = S.off_of[i] + __popc(keep & ((1u << k) - 1u));   // RE index within the symbol
    const uint32_t d0 = ((uint32_t)prefix + (uint32_t)j) * (uint32_t)L;  // first codeword symbol of the element
    const uint32_t bi = d0 * (uint32_t)mod;                              // its first bit: position in the transmission's scrambling sequence
    const uint64_t two = (uint64_t)seq[bi >> 5] | ((uint64_t)seq[(bi >> 5) + 1] << 32);
    const uint32_t cb  = (uint32_t)(two >> (bi & 31)); // scrambling bits of the element's L symbols, bit t = t-th bit
    const uint8_t* cp  = cw + (size_t)bi;
    const int      col = S.prb_of[i] * 12 + k;
    float2         xs[4]; // (the precoded kernel alone: the element's layers, then all antenna ports)
#pragma unroll
    for (int ly = 0; ly < 4; ++ly) {
      if (ly >= L)
        break;
      const uint32_t nat = (gather_bits(cp + ly * mod, mod) ^ (cb >> (ly * mod))) & mask; // scrambled bits, bit t = t-th bit of the symbol (b0 first)
      float2         x   = map_symbol(mod, nat, d0 + (uint32_t)ly); // pi/2-BPSK turns with the parity of the codeword symbol
      if (scale) {
        x.x = x.x * scaling;
        x.y = x.y * scaling;
      }
      if constexpr (PRE::on)
        xs[ly] = x;
      else
        out.g[ly][col] = x;
    }
    if constexpr (PRE::on)
      out.store(xs, L, col);
  }
}

// The common shapes (16QAM / 256QAM, the element's run of bytes aligned to words) in two sweeps: the loads of a group of the thread's elements -- the
// LL x MOD bytes of each as one wide load and the two words of its scrambling window -- are issued before the first of them is mapped, unconditionally
// (an element that carries no data reads element 0 of the symbol and is not stored). The one-element-at-a-time loop above pays one memory round trip
// per element: thirteen per thread on 273 PRBs. The group shrinks as the element grows, so that the loaded words stay in registers.
template <int LL, int MOD, class PRE>
__device__ __forceinline__ void pdsch_layers_fast(const pdsch_symbol_lds& S, const int& prefix, const uint32_t* const& seq, const uint8_t* const& cw,
                                                  const PRE& out, const bool& scale, const float& scaling, const int& tid)
{
  constexpr int NW = LL * MOD / 4; // codeword words of one element
  constexpr int IT = (275 * 12 + 255) / 256, G = NW >= 6 ? 4 : (NW >= 3 ? 7 : IT);
  struct alignas(4) words {
    uint32_t v[NW];
  };
  const int nprb = S.nprb;
  for (int it0 = 0; it0 < IT && it0 * 256 < nprb * 12; it0 += G) {
    words    cv[G];
    uint32_t q0[G], q1[G], sh[G];
    int      dst[G]; // grid column of the element, -1: none
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int      idx  = tid + (it0 + u) * 256;
      const bool     in   = idx < nprb * 12;
      const int      i    = in ? idx / 12 : 0, k = in ? idx - i * 12 : 0;
      const unsigned keep = S.keep_of[i];
      const bool     has  = in && ((keep >> k) & 1u);
      const int      j    = has ? S.off_of[i] + __popc(keep & ((1u << k) - 1u)) : 0;
      const uint32_t d0   = ((uint32_t)prefix + (uint32_t)j) * (uint32_t)LL; // first codeword symbol of the element
      const uint32_t bi   = d0 * (uint32_t)MOD;
      q0[u] = seq[bi >> 5], q1[u] = seq[(bi >> 5) + 1];
      sh[u]  = bi & 31u;
      cv[u]  = *reinterpret_cast<const words*>(cw + (size_t)d0 * MOD);
      dst[u] = has ? (int)S.prb_of[i] * 12 + k : -1;
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const uint32_t cb  = (uint32_t)((((uint64_t)q1[u] << 32) | q0[u]) >> sh[u]);
      uint32_t       raw = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w)
        raw |= (((cv[u].v[w] & 0x01010101u) * 0x01020408u) >> 24) << (4 * w);
      const uint32_t bits = raw ^ cb; // scrambled bits of the element, layer after layer
      float2         xs[4];           // (the precoded kernel alone)
#pragma unroll
      for (int ly = 0; ly < LL; ++ly) {
        float2 x = map_symbol(MOD, (bits >> (ly * MOD)) & ((1u << MOD) - 1u), 0u);
        if (scale) {
          x.x = x.x * scaling;
          x.y = x.y * scaling;
        }
        if constexpr (PRE::on)
          xs[ly] = x;
        else if (dst[u] >= 0)
          out.g[ly][dst[u]] = x;
      }
      if constexpr (PRE::on)
        if (dst[u] >= 0)
          out.store(xs, LL, dst[u]);
    }
  }
}

// Scrambling sequence c(0 .. nof_bits - 1) of every transmission, one workgroup each (c_init = rnti * 2^15 + n_id, TS 38.211 7.3.1.1): x1 from
// the table, x2 from its linear basis and the doubling word recurrence (gold_device.h) -- as the PUSCH demodulator does. The OFDM symbols
// of a transmission use consecutive pieces of it; before, every (transmission, symbol) workgroup jumped both LFSRs to its first bit and ran
// the recurrences on one wavefront while three waited (0.40 ms per 1024 slots of 273 PRB: the longest kernel of the transmit chain).
// prefix_out[job][14]: the data elements of the transmission before every OFDM symbol.
constexpr int PDSCH_SEQ_STRIDE = GOLD_X1_WORDS;
__global__ void __launch_bounds__(512) pdsch_seq_kernel(const miphy_pdsch_mod_job* __restrict__ jobs, const gold_tables* __restrict__ gt, uint32_t* __restrict__ seq,
                                                        int* __restrict__ prefix_out)
{
  __shared__ uint32_t w[PDSCH_SEQ_STRIDE];
  __shared__ uint64_t rbm[5], resm[4][5];
  __shared__ int      cnt[14];
  const miphy_pdsch_mod_job* __restrict__ jp = jobs + blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  pdsch_count_symbols(*jp, rbm, resm, cnt, tid, nt);
  if (tid == 0) {
    int run = 0;
    for (int s = 0; s < 14; ++s) {
      prefix_out[blockIdx.x * 14 + s] = run;
      run += cnt[s];
    }
  }
  int       nwords = (int)((jp->nof_bits + 31u) >> 5) + 2; // + the 64-bit window of the last resource element
  nwords           = nwords > PDSCH_SEQ_STRIDE ? PDSCH_SEQ_STRIDE : nwords;
  gold_x2_sequence(*gt, (jp->rnti << 15) + jp->n_id, nwords, w, tid, nt);
  uint32_t* o = seq + (size_t)blockIdx.x * PDSCH_SEQ_STRIDE;
  for (int i = tid; i < nwords; i += nt)
    o[i] = w[i] ^ gt->x1_seq[i];
}

__global__ void __launch_bounds__(256) pdsch_mod_kernel(const miphy_pdsch_mod_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                        const uint8_t* __restrict__ cw_base, float2* __restrict__ grid, const uint32_t* __restrict__ seq_base,
                                                        const int* __restrict__ prefix_base)
{
  __shared__ pdsch_symbol_lds S;
  const miphy_pdsch_mod_job* __restrict__ jp = jobs + blockIdx.x;
  const int sy  = blockIdx.y;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int start_symbol = jp->start_symbol, nof_symbols = jp->nof_symbols;
  if (sy < start_symbol || sy >= start_symbol + nof_symbols)
    return;
  const int prefix = prefix_base[blockIdx.x * 14 + sy]; // elements of the transmission in earlier symbols (pdsch_seq_kernel)
  if (pdsch_symbol_setup(*jp, sy, S, tid, nt) == 0)
    return;
  const int       mod = jp->mod;
  const uint32_t* seq = seq_base + (size_t)blockIdx.x * PDSCH_SEQ_STRIDE;
  const float     scaling = jp->scaling;
  const bool      scale   = isnormal(scaling);
  const uint8_t*  cw      = cw_base + jp->cw_offset;
  const pdsch_no_precoding g(grid + jp->grid_offset + ((size_t)jp->port * 14 + sy) * (jp->grid_nof_prb * 12));
  if (mod == 8 && (((uintptr_t)(cw + (size_t)prefix * 8)) & 3u) == 0) {
    pdsch_layers_fast<1, 8>(S, prefix, seq, cw, g, scale, scaling, tid);
    return;
  }
  if (mod == 4 && (((uintptr_t)(cw + (size_t)prefix * 4)) & 3u) == 0) {
    pdsch_layers_fast<1, 4>(S, prefix, seq, cw, g, scale, scaling, tid);
    return;
  }
  pdsch_map_elements(S, 1, mod, prefix, seq, cw, g, scale, scaling, tid, nt);
}

// What the two PDSCH DM-RS kernels share of a workgroup's (job, OFDM symbol): the LDS, the sequence and every value of an RE up to its store.
struct dmrs_pdsch_lds {
  uint32_t w1[128], w2[128]; // the symbol's sequence c(n) in w1 (w2: the second register while it is generated)
  uint16_t prb_of[276];      // the allocated PRBs at and above the reference point, ascending
  uint64_t rbm[5];
  int      nprb;
};
struct dmrs_pdsch_symbol {
  int   nprb, npr, ref, l_prime; // allocated PRBs, DM-RS REs per PRB and port, reference point, 1 = second symbol of a double-symbol DM-RS
  bool  type2;
  float amp;
};
struct dmrs_pdsch_re {
  int   rb, k;    // PRB and, within it, subcarrier of CDM group 0
  float re0, im0; // the sequence value r(n) of the RE
};

// rb_mask of the job into D.rbm, cut at the reference point: PRBs below it are never generated (dmrs_helper.h:53). full: where the uncut words go as
// well, null (a literal) where nobody asks. The caller synchronises.
__device__ __forceinline__ void dmrs_pdsch_load_mask(const miphy_dmrs_pdsch_job& j, dmrs_pdsch_lds& D, uint64_t* full, int tid)
{
  const int ref = j.reference_point_k_rb;
  if (tid < 5) {
    uint64_t m = j.rb_mask[tid];
    if (full)
      full[tid] = m;
    for (int b = 0; b < 64; ++b)
      if (tid * 64 + b < ref)
        m &= ~(1ull << b);
    D.rbm[tid] = m;
  }
}

// Behind dmrs_pdsch_load_mask and a barrier: the PRB list and the Gold sequence of OFDM symbol sy (dmrs_pdsch_processor_impl.cpp:30-169) into D, and
// what the symbol's REs have in common.
__device__ __forceinline__ dmrs_pdsch_symbol dmrs_pdsch_symbol_setup(const miphy_dmrs_pdsch_job& j, int sy, const gold_tables& gt, dmrs_pdsch_lds& D, int tid, int nt)
{
  dmrs_pdsch_symbol y;
  const unsigned    syms      = j.symbols_mask;
  const int         nprb_grid = j.grid_nof_prb;
  y.ref = j.reference_point_k_rb, y.type2 = j.dmrs_type == 2, y.npr = y.type2 ? 4 : 6;
  build_prb_list(D.rbm, nprb_grid, 0, D.prb_of, &D.nprb, tid, nt);
  const uint64_t t      = ((uint64_t)(14u * j.slot_in_frame + (uint32_t)sy + 1u) * (2ull * j.scrambling_id + 1ull)) % (1ull << 31);
  const uint32_t c_init = (uint32_t)((t * (1ull << 17) + (2ull * j.scrambling_id + (j.n_scid ? 1u : 0u))) % (1ull << 31));
  const int      nbits  = 2 * y.npr * (nprb_grid - y.ref);
  __syncthreads();
  gold_long_block(gt, c_init, 0, ((nbits + 31) >> 5) + 1, D.w1, D.w2, D.w1, tid, nt);
  y.nprb    = D.nprb;
  y.amp     = (float)(0.70710678118654752440 * (double)j.amplitude);
  y.l_prime = (sy != 0 && ((syms >> (sy - 1)) & 1u)) ? 1 : 0;
  return y;
}

// RE idx = 0 .. nprb x npr - 1 of the symbol: idx is also its index in the generated sequence, which counts allocated PRBs only.
__device__ __forceinline__ dmrs_pdsch_re dmrs_pdsch_re_of(const dmrs_pdsch_lds& D, const dmrs_pdsch_symbol& y, int idx)
{
  dmrs_pdsch_re r;
  const int     i = idx / y.npr, q = idx - i * y.npr;
  r.rb            = D.prb_of[i];
  const int gI    = (r.rb - y.ref) * y.npr + q;            // position in the sequence, counted from the reference point
  r.k             = !y.type2 ? 2 * q : (q < 2 ? q : 4 + q); // type 1: 0,2,..,10 ; type 2: 0,1,6,7
  r.re0           = ((D.w1[(2 * gI) >> 5] >> ((2 * gI) & 31)) & 1u) ? -y.amp : y.amp;
  r.im0           = ((D.w1[(2 * gI + 1) >> 5] >> ((2 * gI + 1) & 31)) & 1u) ? -y.amp : y.amp;
  return r;
}

// w_f(k') w_t(l') of DM-RS port p on RE idx (TS 38.211 Tables 7.4.1.1.2-1 and -2).
__device__ __forceinline__ float dmrs_pdsch_weight(int p, int idx, const dmrs_pdsch_symbol& y)
{
  const float wf1 = (p & 1) ? -1.f : 1.f;
  const float wt  = (y.l_prime && p >= (y.type2 ? 6 : 4)) ? -1.f : 1.f;
  return wt * ((idx & 1) ? wf1 : 1.f);
}

__global__ void __launch_bounds__(256) dmrs_pdsch_kernel(const miphy_dmrs_pdsch_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                         float2* __restrict__ grid)
{
  __shared__ dmrs_pdsch_lds D;
  const miphy_dmrs_pdsch_job* __restrict__ jp = jobs + blockIdx.x;
  const int sy = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (!((jp->symbols_mask >> sy) & 1u))
    return;
  dmrs_pdsch_load_mask(*jp, D, nullptr, tid);
  __syncthreads();
  const dmrs_pdsch_symbol y = dmrs_pdsch_symbol_setup(*jp, sy, *gt, D, tid, nt);
  const int nprb_grid = jp->grid_nof_prb, nports = jp->nof_ports;
  for (int idx = tid; idx < y.nprb * y.npr; idx += nt) {
    const dmrs_pdsch_re r = dmrs_pdsch_re_of(D, y, idx);
    for (int p = 0; p < nports; ++p) {
      const int   delta = !y.type2 ? (p >> 1) & 1 : 2 * ((p >> 1) % 3);
      const float w     = dmrs_pdsch_weight(p, idx, y);
      grid[jp->grid_offset + ((size_t)jp->ports[p] * 14 + sy) * (nprb_grid * 12) + r.rb * 12 + r.k + delta] = make_float2(r.re0 * w, r.im0 * w);
    }
  }
}

// PDCCH: QPSK mapping of the encoded, scrambled bits and the DM-RS of one (PDU, symbol of the CORESET) per workgroup
// (pdcch_modulator_impl.cpp:30-91, dmrs_pdcch_processor_impl.cpp:30-101).
__global__ void __launch_bounds__(256) pdcch_map_kernel(const miphy_pdcch_pdu* __restrict__ pdus, const gold_tables* __restrict__ gt,
                                                        const uint8_t* __restrict__ enc_base, float2* __restrict__ grid)
{
  __shared__ uint32_t w1[128], w2[128];
  __shared__ uint16_t prb_of[276];
  __shared__ uint64_t rbm[5];
  __shared__ int      nprb_s;
  const miphy_pdcch_pdu* __restrict__ pp = pdus + blockIdx.x;
  const int s = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (s >= pp->duration)
    return;
  const int sy = pp->start_symbol + s, nprb_grid = pp->grid_nof_prb, ref = pp->reference_point_k_rb;
  if (tid < 5)
    rbm[tid] = pp->rb_mask[tid];
  __syncthreads();
  build_prb_list(rbm, nprb_grid, 0, prb_of, &nprb_s, tid, nt);
  __syncthreads();
  const int nprb = nprb_s, R = 9 * nprb, prefix = s * R;
  float2*   g    = grid + pp->grid_offset + ((size_t)pp->port * 14 + sy) * (nprb_grid * 12);
  // data: scrambling slice of this symbol, c_init = (n_rnti << 16) + n_id (mod 2^31)
  gold_long_block(*gt, ((pp->n_rnti << 16) + pp->n_id_pdcch_data) & 0x7fffffffu, 2u * (uint32_t)prefix, ((2 * R + 31) >> 5) + 1, w1, w2, w1, tid, nt);
  const float    scaling = powf(10.0f, pp->data_power_offset_dB / 20.0f); // convert_dB_to_amplitude
  const bool     scale   = isnormal(scaling);
  const uint8_t* enc     = enc_base + pp->work_offset;
  for (int idx = tid; idx < R; idx += nt) {
    const int      i = idx / 9, q = idx - i * 9;
    const int      k = q + (q + 2) / 3;                       // REs 0,2,3,4,6,7,8,10,11: the DM-RS sit on 1, 5, 9
    const int      d = prefix + idx;                          // QPSK symbol index within the PDU
    const uint32_t c0 = (w1[(2 * idx) >> 5] >> ((2 * idx) & 31)) & 1u, c1 = (w1[(2 * idx + 1) >> 5] >> ((2 * idx + 1) & 31)) & 1u;
    const uint32_t nat = ((uint32_t)(enc[2 * d] & 1u) ^ c0) | (((uint32_t)(enc[2 * d + 1] & 1u) ^ c1) << 1);
    float2 x = map_symbol(2, nat, (unsigned)d);
    if (scale) {
      x.x = x.x * scaling;
      x.y = x.y * scaling;
    }
    g[prb_of[i] * 12 + k] = x;
  }
  __syncthreads();
  // DM-RS of this symbol (normal cyclic prefix: 14 symbols per slot)
  const uint64_t t      = ((uint64_t)(14u * pp->slot_in_frame + (uint32_t)sy + 1u) * (2ull * pp->n_id_pdcch_dmrs + 1ull)) % (1ull << 31);
  const uint32_t c_init = (uint32_t)((t * (1ull << 17) + 2ull * pp->n_id_pdcch_dmrs) % (1ull << 31));
  const int      nbits  = 2 * 3 * (nprb_grid - ref);
  gold_long_block(*gt, c_init, 0, ((nbits + 31) >> 5) + 1, w1, w2, w1, tid, nt);
  const float amp = (float)(0.70710678118654752440 * (double)powf(10.0f, pp->dmrs_power_offset_dB / 20.0f));
  for (int idx = tid; idx < 3 * nprb; idx += nt) {
    const int i = idx / 3, q = idx - 3 * i, rb = prb_of[i];
    if (rb < ref)
      continue; // never generated (dmrs_helper.h:58)
    const int   gI = (rb - ref) * 3 + q;
    const float re = ((w1[(2 * gI) >> 5] >> ((2 * gI) & 31)) & 1u) ? -amp : amp;
    const float im = ((w1[(2 * gI + 1) >> 5] >> ((2 * gI + 1) & 31)) & 1u) ? -amp : amp;
    g[rb * 12 + 1 + 4 * q] = make_float2(re, im);
  }
}

// SS/PBCH block: PBCH symbols, PBCH DM-RS, PSS and SSS of one block per workgroup (pbch_modulator_impl.cpp:28-113,
// dmrs_pbch_processor_impl.cpp:28-100, pss_processor_impl.cpp:28-91, sss_processor_impl.cpp:28-119).
__global__ void __launch_bounds__(256) ssb_map_kernel(const miphy_ssb_pdu* __restrict__ pdus, const gold_tables* __restrict__ gt,
                                                      const uint8_t* __restrict__ enc_base, float2* __restrict__ grid)
{
#pragma clang fp contract(off)
  __shared__ uint32_t w1[64], w2[64];
  __shared__ uint8_t  xp[134], x0[134], x1[134]; // m-sequences of PSS / SSS
  const miphy_ssb_pdu* __restrict__ pp = pdus + blockIdx.x;
  const int      tid = threadIdx.x, nt = blockDim.x;
  const unsigned N_id = pp->msg.N_id, ssb_idx = pp->msg.ssb_idx, v = N_id % 4;
  const unsigned l0 = pp->ssb_first_symbol, k0 = pp->ssb_first_subcarrier, nsc = pp->grid_nof_prb * 12u;
  if (tid < 3) {
    uint8_t* x = tid == 0 ? xp : (tid == 1 ? x0 : x1);
    for (int i = 0; i < 7; ++i)
      x[i] = 0;
    if (tid == 0)
      x[6] = 1, x[5] = 1, x[4] = 1, x[3] = 0, x[2] = 1, x[1] = 1, x[0] = 0; // pss_processor_impl.cpp:32-38
    else
      x[0] = 1;                                                             // sss_processor_impl.cpp:30-37, 51-58
    for (int i = 0; i < 127; ++i)
      x[i + 7] = (uint8_t)((x[i + (tid == 2 ? 1 : 4)] + x[i]) & 1u);
  }
  // PBCH: scrambling sequence of the cell, advanced by (ssb_idx & 7) * 864 (pbch_modulator_impl.cpp:28-38)
  gold_long_block(*gt, N_id, (ssb_idx & 7u) * 864u, 28, w1, w2, w1, tid, nt);
  const uint8_t* enc = enc_base + (size_t)blockIdx.x * 864u;
  // position of the idx-th PBCH symbol / DM-RS: symbol 1 (240 subcarriers), symbol 2 lower (48) and upper (48) part, symbol 3 (240)
  auto place = [&](int idx, int per4, unsigned& l, unsigned& k) { // per4 = 3 data REs or 1 DM-RS per group of four subcarriers
    const int n1 = 60 * per4, n2 = 12 * per4;
    int       g, r, base, ls;
    if (idx < n1)
      ls = 1, base = 0, g = idx / per4, r = idx - g * per4;
    else if (idx < n1 + n2)
      ls = 2, base = 0, g = (idx - n1) / per4, r = (idx - n1) - g * per4;
    else if (idx < n1 + 2 * n2)
      ls = 2, base = 192, g = (idx - n1 - n2) / per4, r = (idx - n1 - n2) - g * per4;
    else
      ls = 3, base = 0, g = (idx - n1 - 2 * n2) / per4, r = (idx - n1 - 2 * n2) - g * per4;
    const int pos = per4 == 1 ? (int)v : r + (r >= (int)v ? 1 : 0); // DM-RS on k % 4 == v, data on the other three
    l = l0 + ls, k = k0 + base + 4 * g + pos;
  };
  for (int idx = tid; idx < 432; idx += nt) {
    const uint32_t c0  = (w1[(2 * idx) >> 5] >> ((2 * idx) & 31)) & 1u, c1 = (w1[(2 * idx + 1) >> 5] >> ((2 * idx + 1) & 31)) & 1u;
    const uint32_t nat = ((uint32_t)(enc[2 * idx] & 1u) ^ c0) | (((uint32_t)(enc[2 * idx + 1] & 1u) ^ c1) << 1);
    const float2   x   = map_symbol(2, nat, (unsigned)idx);
    unsigned       l, k;
    place(idx, 3, l, k);
    for (int p = 0; p < pp->nof_ports; ++p)
      grid[pp->grid_offset + ((size_t)pp->ports[p] * 14 + l) * nsc + k] = x;
  }
  __syncthreads();
  // DM-RS for PBCH (dmrs_pbch_processor_impl.cpp:28-47)
  uint32_t i_ssb = (ssb_idx & 3u) + 4u * (pp->msg.hrf ? 1u : 0u);
  if (pp->msg.L_max == 8 || pp->msg.L_max == 64)
    i_ssb = ssb_idx & 7u;
  const uint32_t c_init = (((i_ssb + 1u) * ((N_id / 4u) + 1u)) << 11) + ((i_ssb + 1u) << 6) + (N_id % 4u);
  gold_long_block(*gt, c_init, 0, 10, w1, w2, w1, tid, nt);
  const float a = (float)0.70710678118654752440; // prg->generate(sequence, M_SQRT1_2)
  for (int idx = tid; idx < 144; idx += nt) {
    const float re = ((w1[(2 * idx) >> 5] >> ((2 * idx) & 31)) & 1u) ? -a : a;
    const float im = ((w1[(2 * idx + 1) >> 5] >> ((2 * idx + 1) & 31)) & 1u) ? -a : a;
    unsigned    l, k;
    place(idx, 1, l, k);
    for (int p = 0; p < pp->nof_ports; ++p)
      grid[pp->grid_offset + ((size_t)pp->ports[p] * 14 + l) * nsc + k] = make_float2(re, im);
  }
  // PSS (symbol 0) and SSS (symbol 2), subcarriers 56..182 of the block
  const unsigned nid1 = N_id / 3u, nid2 = N_id % 3u;
  const unsigned m = (43u * nid2) % 127u, m0 = 15u * (nid1 / 112u) + 5u * nid2, m1 = nid1 % 112u;
  const float    amp_pss = powf(10.0f, pp->beta_pss_dB / 20.0f); // convert_dB_to_amplitude(beta_pss)
  for (int n = tid; n < 127; n += nt) {
    const float dp = 1.0f - 2.0f * (float)xp[(n + m) % 127u];
    // srsvec::sc_prod(cf_t, float): both components are multiplied
    const float2 pss = make_float2(dp * amp_pss, 0.0f * amp_pss);
    const float  d0v = 1.0f - 2.0f * (float)x0[(n + m0) % 127u], d1v = 1.0f - 2.0f * (float)x1[(n + m1) % 127u];
    // sc_prod by amplitude 1, then the complex product with d1 (real-valued factors: the imaginary part is a signed zero)
    const float ar = d0v * 1.0f, ai = 0.0f * 1.0f, br = d1v, bi = 0.0f;
    const float2 sss = make_float2(ar * br - ai * bi, ar * bi + ai * br);
    for (int p = 0; p < pp->nof_ports; ++p) {
      float2* g = grid + pp->grid_offset + (size_t)pp->ports[p] * 14 * nsc + k0 + 56 + n;
      g[(size_t)(l0 + 0) * nsc] = pss;
      g[(size_t)(l0 + 2) * nsc] = sss;
    }
  }
}

// NZP-CSI-RS: one (job, port, OFDM symbol) per workgroup (nzp_csi_rs_generator_impl.cpp:34-296).
__global__ void __launch_bounds__(256) csi_rs_kernel(const miphy_csi_rs_job* __restrict__ jobs, const gold_tables* __restrict__ gt, float2* __restrict__ grid)
{
#pragma clang fp contract(off)
  __shared__ uint32_t w1[64], w2[64];
  const miphy_csi_rs_job* __restrict__ jp = jobs + blockIdx.x;
  const int port = blockIdx.y, l = blockIdx.z, tid = threadIdx.x, nt = blockDim.x;
  if (port >= jp->nof_ports || !((jp->symbol_mask[port] >> l) & 1u))
    return;
  const unsigned start_rb = jp->start_rb, nof_rb = jp->nof_rb, dens = jp->freq_density, cdm = jp->cdm;
  // sequence length of one symbol (:131-161) and the elements skipped below the first occupied PRB (:69-108)
  unsigned seq_len = nof_rb, first_prb = start_rb, adv;
  if (dens <= 1) {
    seq_len /= 2;
    if ((nof_rb & 1u) && (((start_rb & 1u) != 0) == (dens == 1)))
      ++seq_len;
    first_prb = dens == 0 ? start_rb + (start_rb & 1u) : start_rb + (1u - (start_rb & 1u));
    adv       = jp->mapping_row == 2 ? first_prb / 2 : first_prb;
  } else if (dens == 3) {
    seq_len *= 3;
    adv = 3 * first_prb;
  } else {
    adv = jp->mapping_row == 2 ? first_prb : 2 * first_prb;
  }
  if (cdm != 0)
    seq_len *= 2;
  const uint64_t t      = ((uint64_t)1024u * (14u * jp->slot_in_frame + (uint32_t)l + 1u) * (2ull * jp->scrambling_id + 1ull) + jp->scrambling_id) % (1ull << 31);
  gold_long_block(*gt, (uint32_t)t, 2u * adv, ((2 * (int)seq_len + 31) >> 5) + 1, w1, w2, w1, tid, nt);
  const float    amp   = (float)(0.70710678118654752440 * (double)jp->amplitude);
  const unsigned gsize = cdm == 0 ? 1u : (cdm == 1 ? 2u : (cdm == 2 ? 4u : 8u));
  const unsigned cidx  = (unsigned)port % gsize;                                  // index inside the CDM group
  const unsigned lidx  = (unsigned)__popc(jp->symbol_mask[port] & ((1u << l) - 1u)); // l' = position of this symbol in the port's pattern
  // w_f = {+1, (-1)^cidx}; w_t[l'] from the Hadamard rows of the tables (:34-57)
  const float wf1 = (cidx & 1u) ? -1.0f : 1.0f;
  float       wt  = 1.0f;
  if (cdm >= 2) {
    const unsigned row = cidx >> 1; // 0..1 (TD2) or 0..3 (TD4): rows {++++, +-+-, ++--, +--+}
    const unsigned neg = row == 0 ? 0x0u : (row == 1 ? 0xau : (row == 2 ? 0xcu : 0x6u));
    wt                 = ((neg >> lidx) & 1u) ? -1.0f : 1.0f;
  }
  const unsigned re_mask = jp->re_mask[port], n_re = (unsigned)__popc(re_mask);
  const unsigned stride = jp->rb_stride ? jp->rb_stride : 1u, nsc = jp->grid_nof_prb * 12u;
  float2*        g      = grid + jp->grid_offset + ((size_t)jp->ports[port] * 14 + l) * nsc;
  // pattern PRBs inside [start_rb, start_rb + nof_rb), ascending; element k of the sequence goes to the k-th set RE
  unsigned j0 = 0; // first pattern PRB index inside the window
  if (start_rb > jp->rb_begin)
    j0 = (start_rb - jp->rb_begin + stride - 1u) / stride;
  for (unsigned k = tid; k < seq_len; k += nt) {
    const unsigned j = k / n_re, r = k - j * n_re;
    const unsigned rb = jp->rb_begin + (j0 + j) * stride;
    if (rb >= jp->rb_end || rb >= start_rb + nof_rb)
      continue;
    unsigned m = re_mask; // r-th set bit
    for (unsigned q = 0; q < r; ++q)
      m &= m - 1u;
    const unsigned sc = (unsigned)__ffs((int)m) - 1u;
    float re = ((w1[(2 * k) >> 5] >> ((2 * k) & 31)) & 1u) ? -amp : amp;
    float im = ((w1[(2 * k + 1) >> 5] >> ((2 * k + 1) & 31)) & 1u) ? -amp : amp;
    if (cdm == 1) {
      const float w = (k & 1u) ? wf1 : 1.0f; // table.w_f[k'] * seq
      re = w * re, im = w * im;
    } else if (cdm >= 2) {
      const float w = wt * ((k & 1u) ? wf1 : 1.0f); // (w_t[l'] * w_f[k']) * seq
      re = w * re, im = w * im;
    }
    g[rb * 12u + sc] = make_float2(re, im);
  }
}


// ---------------------------------------------------------------------------------------------------- one codeword on 1..4 layers
// Beyond the 23.5 reference (whose layer mapper is broken), so the contract is the oracle's orc_pdsch_modulate.
constexpr int PDSCH_SEQ_CHUNK = PDSCH_SEQ_STRIDE / 2; // sequence words one workgroup of pdsch_seq_layers_kernel generates (x1 and x2 in LDS)
constexpr int PDSCH_LAYERS_INFO = 16;                 // ints per transmission: 14 symbol prefixes, the elements per layer, 1 = valid job

// What the fields of a modulator job j must satisfy, once: R(condition, message of the host, its arguments). The kernels skip a device-resident
// job that breaks a rule (pdsch_mod_fields_ok), the host refuses one with the rule's message (miphy_pdsch_mod_job_check).
#define PDSCH_MOD_FIELD_RULES(R)                                                                                                                       \
  R(j.mod == 1 || j.mod == 2 || j.mod == 4 || j.mod == 6 || j.mod == 8, "invalid modulation order %u", j.mod)                                         \
  R(j.nof_symbols >= 1 && j.start_symbol + j.nof_symbols <= 14, "invalid time allocation")                                                            \
  R(j.dmrs_type == 1 || j.dmrs_type == 2, "invalid DM-RS type")                                                                                       \
  R(j.nof_cdm_groups_without_data >= 1 && j.nof_cdm_groups_without_data <= (j.dmrs_type == 1 ? 2 : 3), "invalid number of CDM groups without data")   \
  R(j.grid_nof_prb >= 1 && j.grid_nof_prb <= 275 && j.bwp_start_rb + j.bwp_size_rb <= 275, "invalid grid / BWP")                                      \
  R(j.nof_reserved <= 4, "at most 4 reserved RE patterns (re_pattern_list::MAX_RE_PATTERN)")                                                          \
  R(j.n_id < 1024 && j.rnti < 65536, "invalid scrambling identifiers")

__host__ __device__ __forceinline__ bool pdsch_mod_fields_ok(const miphy_pdsch_mod_job& j)
{
#define PDSCH_RULE_HOLDS(cond, ...) &&(cond)
  return true PDSCH_MOD_FIELD_RULES(PDSCH_RULE_HOLDS);
#undef PDSCH_RULE_HOLDS
}

// What the kernels check of a job themselves (device-resident jobs reach them unseen by the host): a job that fails is skipped.
__device__ __forceinline__ bool layers_job_ok(const miphy_pdsch_mod_layers_job& j)
{
  const unsigned L = j.nof_layers;
  if (L < 1 || L > 4)
    return false;
  unsigned seen = 0;
  for (unsigned ly = 0; ly < L; ++ly) {
    const unsigned p = j.ports[ly];
    if (p >= 16 || ((seen >> p) & 1u))
      return false;
    seen |= 1u << p;
  }
  return pdsch_mod_fields_ok(j.base);
}

// One or two codewords on 1..8 layers (miphy_pdsch_mod_codewords_job, TS 38.211 Table 7.3.1.3-1): the layers of each codeword and its first layer.
struct pdsch_codewords_split {
  unsigned L0, L1; // L1 = 0: one codeword
};
__host__ __device__ __forceinline__ pdsch_codewords_split pdsch_codewords_split_of(unsigned L)
{
  const unsigned L0 = L > 4 ? L / 2 : L;
  return {L0, L - L0};
}

__host__ __device__ __forceinline__ bool pdsch_codewords_ports_ok(const miphy_pdsch_mod_codewords_job& c)
{
  unsigned seen = 0;
  for (unsigned ly = 0; ly < c.nof_layers && ly < 8; ++ly) {
    const unsigned p = c.ports[ly];
    if (p >= 16 || ((seen >> p) & 1u))
      return false;
    seen |= 1u << p;
  }
  return true;
}

__host__ __device__ __forceinline__ bool pdsch_mod_order_ok(unsigned mod) { return mod == 1 || mod == 2 || mod == 4 || mod == 6 || mod == 8; }

// What a codewords job c adds to the rules of its mapped job (the fields of c.mapped.layers.base, the list), once more for the kernels' predicate and the
// host's messages, evaluated in this order ...
#define PDSCH_MOD_CODEWORDS_RULES(R)                                                                                                                   \
  R(c.nof_layers >= 1 && c.nof_layers <= 8, "invalid number of layers %u (1..4: one codeword, 5..8: two)", (unsigned)c.nof_layers)                    \
  R(pdsch_codewords_ports_ok(c), "the layers need distinct grid ports below 16")                                                                      \
  R(c.nof_layers <= 4 || pdsch_mod_order_ok(c.mod1), "invalid modulation order %u of codeword 1", (unsigned)c.mod1)
// ... and, with nre = the data REs per layer of its allocation and cs = pdsch_codewords_split_of(c.nof_layers), of the size of each codeword.
#define PDSCH_MOD_CODEWORDS_SIZE_RULES(R)                                                                                                              \
  R(c.mapped.layers.base.nof_bits == (uint64_t)nre * cs.L0 * c.mapped.layers.base.mod, "codeword 0 of %u bits, the allocation holds %u on %u layers", \
    c.mapped.layers.base.nof_bits, (unsigned)(nre * cs.L0 * c.mapped.layers.base.mod), cs.L0)                                                          \
  R(cs.L1 == 0 || c.nof_bits1 == (uint64_t)nre * cs.L1 * c.mod1, "codeword 1 of %u bits, the allocation holds %u on %u layers", c.nof_bits1,          \
    (unsigned)(nre * cs.L1 * c.mod1), cs.L1)

#define PDSCH_RULE_HOLDS(cond, ...) &&(cond)
__host__ __device__ __forceinline__ bool pdsch_codewords_job_ok(const miphy_pdsch_mod_codewords_job& c)
{
  return true PDSCH_MOD_CODEWORDS_RULES(PDSCH_RULE_HOLDS) && pdsch_mod_fields_ok(c.mapped.layers.base);
}
__host__ __device__ __forceinline__ bool pdsch_codewords_sizes_ok(const miphy_pdsch_mod_codewords_job& c, const pdsch_codewords_split& cs, uint32_t nre)
{
  return true PDSCH_MOD_CODEWORDS_SIZE_RULES(PDSCH_RULE_HOLDS);
}
#undef PDSCH_RULE_HOLDS

// What the PRB list of a mapped job m must satisfy, once, for the same two readers. The rules of the list as a whole: nof_list_entries = entries of
// the batch's list array, rbm = the five words of the job's rb_mask (the job itself on the host, the copy in LDS on the device) ...
#define PDSCH_MOD_LIST_RULES(R)                                                                                                                        \
  R((uint64_t)m.prb_list_offset + m.nof_prb <= nof_list_entries, "PRB list [%u, %u + %u) exceeds the %u list entries", m.prb_list_offset,             \
    m.prb_list_offset, (unsigned)m.nof_prb, nof_list_entries)                                                                                         \
  R((unsigned)m.nof_prb == pdsch_mask_popcount(rbm), "PRB list of %u entries for the %u PRBs of rb_mask", (unsigned)m.nof_prb, pdsch_mask_popcount(rbm))
// ... and of its entry i, PRB e, evaluated in this order: test_and_set(e) marks e in a 5-word bitmap and returns whether it was marked before, and is
// reached only by an e below grid_nof_prb <= 275 (PDSCH_MOD_FIELD_RULES hold). A list that passes names every PRB of rb_mask once.
#define PDSCH_MOD_LIST_ENTRY_RULES(R)                                                                                                                  \
  R(e < m.layers.base.grid_nof_prb, "PRB list entry %u: PRB %u outside the grid of %u PRBs", i, e, (unsigned)m.layers.base.grid_nof_prb)               \
  R((rbm[e >> 6] >> (e & 63)) & 1ull, "PRB list entry %u: PRB %u is not in rb_mask", i, e)                                                             \
  R(!test_and_set(e), "PRB list entry %u: PRB %u appears twice", i, e)

__host__ __device__ __forceinline__ unsigned pdsch_mask_popcount(const uint64_t* rbm)
{
  unsigned c = 0;
  for (int w = 0; w < 5; ++w)
    c += (unsigned)__builtin_popcountll(rbm[w]);
  return c;
}

#define PDSCH_RULE_HOLDS(cond, ...) &&(cond)
__host__ __device__ __forceinline__ bool pdsch_list_ok(const miphy_pdsch_mod_mapped_job& m, uint32_t nof_list_entries, const uint64_t* rbm)
{
  return true PDSCH_MOD_LIST_RULES(PDSCH_RULE_HOLDS);
}
template <class F>
__host__ __device__ __forceinline__ bool pdsch_list_entry_ok(const miphy_pdsch_mod_mapped_job& m, const uint64_t* rbm, unsigned i, unsigned e, F&& test_and_set)
{
  return true PDSCH_MOD_LIST_ENTRY_RULES(PDSCH_RULE_HOLDS);
}

// What a precoding p must satisfy, once more for the same two readers: L = the layers of the job it belongs to (the modulator's nof_layers, the DM-RS
// job's nof_ports), rbm = the five words of the job's rb_mask, nof_weights = cf_t entries of the call's weights. Evaluated in this order; a precoding
// that passes indexes its weights only inside the array, for every PRB of rb_mask.
#define PDSCH_PRECODING_RULES(R)                                                                                                                       \
  R(p.nof_layers >= 1 && p.nof_layers <= 4, "precoding: invalid number of layers %u (1..4)", (unsigned)p.nof_layers)                                  \
  R(p.nof_layers == L, "precoding: %u layers for a job of %u", (unsigned)p.nof_layers, (unsigned)L)                                                   \
  R(p.nof_ports >= p.nof_layers && p.nof_ports <= 16, "precoding: invalid number of antenna ports %u (%u..16)", (unsigned)p.nof_ports,                \
    (unsigned)p.nof_layers)                                                                                                                           \
  R(precoding_ports_ok(p), "precoding: the antenna ports need distinct grid ports below 16")                                                          \
  R(p.prg_size >= 1 && p.nof_prg >= 1, "precoding: invalid PRG size %u or number of PRGs %u", (unsigned)p.prg_size, (unsigned)p.nof_prg)              \
  R((uint32_t)p.nof_prg * p.prg_size >= pdsch_mask_span(rbm), "precoding: %u PRGs of %u PRBs do not reach PRB %u of rb_mask", (unsigned)p.nof_prg,    \
    (unsigned)p.prg_size, pdsch_mask_span(rbm) - 1u)                                                                                                  \
  R((uint64_t)p.weights_offset + (uint64_t)p.nof_prg * p.nof_ports * p.nof_layers <= nof_weights,                                                     \
    "precoding: weights [%u, %u + %u x %u x %u) exceed the %u weights", p.weights_offset, p.weights_offset, (unsigned)p.nof_prg, (unsigned)p.nof_ports, \
    (unsigned)p.nof_layers, nof_weights)

__host__ __device__ __forceinline__ bool precoding_ports_ok(const miphy_precoding& p)
{
  unsigned seen = 0;
  for (unsigned a = 0; a < p.nof_ports && a < 16; ++a) {
    const unsigned q = p.ports[a];
    if (q >= 16 || ((seen >> q) & 1u))
      return false;
    seen |= 1u << q;
  }
  return true;
}

// One above the highest PRB set in the mask, 0 for an empty one.
__host__ __device__ __forceinline__ unsigned pdsch_mask_span(const uint64_t* rbm)
{
  for (int w = 4; w >= 0; --w)
    if (rbm[w])
      return (unsigned)(64 * w + 64 - __builtin_clzll(rbm[w]));
  return 0;
}

__host__ __device__ __forceinline__ bool pdsch_precoding_ok(const miphy_precoding& p, unsigned L, const uint64_t* rbm, uint32_t nof_weights)
{
  return true PDSCH_PRECODING_RULES(PDSCH_RULE_HOLDS);
}

// What a job j of miphy_channel_precode_batch must satisfy.
#define PRECODE_JOB_RULES(R)                                                                                                                           \
  R(j.nof_layers >= 1 && j.nof_layers <= 4, "invalid number of layers %u (1..4)", (unsigned)j.nof_layers)                                             \
  R(j.nof_ports >= j.nof_layers && j.nof_ports <= 16, "invalid number of antenna ports %u (%u..16)", (unsigned)j.nof_ports, (unsigned)j.nof_layers)   \
  R((uint64_t)j.weights_offset + (uint64_t)j.nof_ports * j.nof_layers <= nof_weights, "weights [%u, %u + %u x %u) exceed the %u weights",             \
    j.weights_offset, j.weights_offset, (unsigned)j.nof_ports, (unsigned)j.nof_layers, nof_weights)                                                   \
  R(j.nof_layers == 1 || j.in_stride >= j.nof_re, "input rows of %u REs overlap at a stride of %llu", j.nof_re, (unsigned long long)j.in_stride)      \
  R(j.nof_ports == 1 || j.out_stride >= j.nof_re, "output rows of %u REs overlap at a stride of %llu", j.nof_re, (unsigned long long)j.out_stride)

__host__ __device__ __forceinline__ bool precode_job_ok(const miphy_precode_job& j, uint32_t nof_weights)
{
  return true PRECODE_JOB_RULES(PDSCH_RULE_HOLDS);
}

// What the DM-RS part j of a precoded DM-RS job must satisfy: the rules of miphy_dmrs_pdsch_map_batch with the ports of one codeword.
#define DMRS_PRECODED_FIELD_RULES(R)                                                                                                                   \
  R(j.dmrs_type == 1 || j.dmrs_type == 2, "invalid DM-RS type")                                                                                       \
  R(j.nof_ports >= 1 && j.nof_ports <= 4, "invalid number of DM-RS ports %u (1..4 with precoding)", (unsigned)j.nof_ports)                            \
  R(j.grid_nof_prb >= 1 && j.grid_nof_prb <= 275 && j.reference_point_k_rb < j.grid_nof_prb, "invalid grid")                                          \
  R(j.symbols_mask < (1u << 14), "invalid symbol mask")

__host__ __device__ __forceinline__ bool dmrs_precoded_fields_ok(const miphy_dmrs_pdsch_job& j)
{
  return true DMRS_PRECODED_FIELD_RULES(PDSCH_RULE_HOLDS);
}
#undef PDSCH_RULE_HOLDS

// Sibling of pdsch_seq_kernel for transmissions on L layers, whose sequence is L times longer than the x1 table and than one workgroup's LDS:
// workgroup (transmission, chunk) generates PDSCH_SEQ_CHUNK words of it -- both LFSRs jump to the chunk's first bit (gold_state), one lane
// each runs the 31-word head, the word recurrences do the rest. `stride` = sequence words reserved per transmission. Chunk 0 also validates
// the job and counts its elements: info[0..13] = elements per layer before every OFDM symbol, info[14] = elements per layer, info[15] = 1 when
// the job is valid and its bit count is elements x L x mod.
// mj: the mapped job whose layers job lj is, null (a literal, so that everything about lists folds away) in the kernel of the entry point without
// lists. Chunk 0 of a mapped job with a list also holds the list to PDSCH_MOD_LIST_RULES and PDSCH_MOD_LIST_ENTRY_RULES -- one coalesced read of
// the list, the duplicate test an atomicOr on a 5-word bitmap in LDS -- and clears info[15] when it breaks one: pdsch_mod_mapped_kernel uses no
// entry of a list as an address unless info[15] is set.
// pc: the precoding of the job, null (a literal again) in the kernels of the entry points without one. Chunk 0 of a precoded job holds it to
// PDSCH_PRECODING_RULES as well, and does not look at the layers' ports, which such a job does not use: pdsch_mod_precoded_kernel reads no weight unless
// info[15] is set.
// cj: the codewords job whose mapped job mj is, null (a literal) in the kernels of one codeword. Workgroup (transmission, chunk, codeword q) of such a job
// generates the chunk of the sequence of codeword q (c_init + q 2^14) on that codeword's bit count, into sequence 2 x transmission + q of the scratch;
// chunk 0 of codeword 0 does the counting and the prefixes once and sets info[15] only if PDSCH_MOD_CODEWORDS_RULES and PDSCH_MOD_CODEWORDS_SIZE_RULES
// hold as well -- the job, its list and the bit counts of both codewords. A codeword has at most four layers, so `stride` is bounded as before.
__device__ __forceinline__ void pdsch_seq_layers_body(const miphy_pdsch_mod_layers_job* __restrict__ lj, const miphy_pdsch_mod_mapped_job* __restrict__ mj,
                                                      const uint16_t* __restrict__ prb_lists, uint32_t nof_list_entries,
                                                      const gold_tables* __restrict__ gt, uint32_t* __restrict__ seq, int* __restrict__ info_out,
                                                      uint32_t stride, const miphy_precoding* __restrict__ pc = nullptr, uint32_t nof_weights = 0,
                                                      const miphy_pdsch_mod_codewords_job* __restrict__ cj = nullptr)
{
  __shared__ uint32_t w1[PDSCH_SEQ_CHUNK], w2[PDSCH_SEQ_CHUNK];
  __shared__ uint64_t rbm[5], resm[4][5];
  __shared__ int      cnt[14];
  __shared__ unsigned long long seen[5];
  __shared__ int                list_bad;
  const miphy_pdsch_mod_job* __restrict__ jp = &lj->base;
  const int      tid = threadIdx.x, nt = blockDim.x, chunk = blockIdx.y;
  const unsigned q        = cj ? blockIdx.z : 0u; // the codeword of this workgroup
  const pdsch_codewords_split cs = pdsch_codewords_split_of(cj ? cj->nof_layers : 0u);
  const bool     ok       = cj ? pdsch_codewords_job_ok(*cj) : pc ? lj->nof_layers >= 1 && lj->nof_layers <= 4 && pdsch_mod_fields_ok(*jp) : layers_job_ok(*lj);
  const uint32_t nof_bits = (cj && q) ? cj->nof_bits1 : jp->nof_bits;
  const uint32_t seq_bits = 32u * (stride - 2u); // + the 64-bit window of the last resource element
  const bool     fits     = cj ? jp->nof_bits <= seq_bits && (cs.L1 == 0 || cj->nof_bits1 <= seq_bits) : nof_bits <= seq_bits;
  if (chunk == 0 && q == 0) {
    int* info = info_out + (size_t)blockIdx.x * PDSCH_LAYERS_INFO;
    if (!ok || !fits) {
      if (tid == 0)
        info[15] = 0;
      return;
    }
    pdsch_count_symbols(*jp, rbm, resm, cnt, tid, nt);
    bool list_ok = true;
    if (mj && mj->nof_prb != 0) {
      const miphy_pdsch_mod_mapped_job& m = *mj;
      list_ok = pdsch_list_ok(m, nof_list_entries, rbm); // (uniform: the entries are read only where the whole list lies inside the array)
      if (tid < 5)
        seen[tid] = 0;
      if (tid == 5)
        list_bad = 0;
      __syncthreads();
      if (list_ok) {
        const uint16_t* list = prb_lists + m.prb_list_offset;
        for (unsigned i = tid; i < m.nof_prb; i += nt) {
          const unsigned e = list[i];
          if (!pdsch_list_entry_ok(m, rbm, i, e, [&](unsigned q) { return (atomicOr(&seen[q >> 6], 1ull << (q & 63)) >> (q & 63)) & 1ull; }))
            list_bad = 1;
        }
      }
      __syncthreads();
      list_ok = list_ok && !list_bad;
    }
    if (pc)
      list_ok = list_ok && pdsch_precoding_ok(*pc, lj->nof_layers, rbm, nof_weights);
    if (tid == 0) {
      int run = 0;
      for (int s = 0; s < 14; ++s) {
        info[s] = run;
        run += cnt[s];
      }
      info[14] = run;
      const bool sized = cj ? pdsch_codewords_sizes_ok(*cj, cs, (uint32_t)run) : (uint64_t)run * lj->nof_layers * jp->mod == nof_bits;
      info[15]         = (list_ok && sized) ? 1 : 0;
    }
  }
  if (!ok || !fits || (q && cs.L1 == 0))
    return;
  const int nwords = (int)((nof_bits + 31u) >> 5) + 2;
  const int first  = chunk * PDSCH_SEQ_CHUNK;
  if (first >= nwords)
    return;
  const int n = min(PDSCH_SEQ_CHUNK, nwords - first);
  gold_piece(*gt, (jp->rnti << 15) + (q << 14) + jp->n_id, first, n, w1, w2, seq + ((size_t)blockIdx.x * (cj ? 2u : 1u) + q) * stride + first, tid, nt);
}

__global__ void __launch_bounds__(512) pdsch_seq_layers_kernel(const miphy_pdsch_mod_layers_job* __restrict__ jobs, const gold_tables* __restrict__ gt,
                                                               uint32_t* __restrict__ seq, int* __restrict__ info_out, uint32_t stride)
{
  pdsch_seq_layers_body(jobs + blockIdx.x, nullptr, nullptr, 0, gt, seq, info_out, stride);
}

__global__ void __launch_bounds__(512) pdsch_seq_mapped_kernel(const miphy_pdsch_mod_mapped_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                               uint32_t nof_list_entries, const gold_tables* __restrict__ gt, uint32_t* __restrict__ seq,
                                                               int* __restrict__ info_out, uint32_t stride)
{
  pdsch_seq_layers_body(&jobs[blockIdx.x].layers, jobs + blockIdx.x, prb_lists, nof_list_entries, gt, seq, info_out, stride);
}

// The sequence kernel of miphy_pdsch_modulate_codewords_batch: grid (transmission, chunk, codeword).
__global__ void __launch_bounds__(512) pdsch_seq_codewords_kernel(const miphy_pdsch_mod_codewords_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                                  uint32_t nof_list_entries, const gold_tables* __restrict__ gt, uint32_t* __restrict__ seq,
                                                                  int* __restrict__ info_out, uint32_t stride)
{
  const miphy_pdsch_mod_codewords_job* __restrict__ cj = jobs + blockIdx.x;
  pdsch_seq_layers_body(&cj->mapped.layers, &cj->mapped, prb_lists, nof_list_entries, gt, seq, info_out, stride, nullptr, 0, cj);
}

// The one mapping body of the three layered entry points: workgroup (transmission, OFDM symbol). list: the job's PRBs in mapping order (nof_list of
// them; the mapped and precoded kernels), null: rb_mask ascending. SINK: where the elements go (pdsch_no_precoding, pdsch_precoder); pc and weights are
// the job's precoding and the call's weights for the sink that takes them, null (literals) otherwise. The job, its list and its precoding were held to
// their rules by chunk 0 of the sequence kernel (info[15]).
// cj (CODEWORDS): the codewords job whose layers job lj is, null otherwise. Such a workgroup pays the symbol setup and the prefix once and then maps
// codeword 0 and, where the job has two, codeword 1 behind it: each with its own modulation, sequence, bytes and wide-load condition, through a sink built
// from its slice of the job's ports.
template <class SINK, bool CODEWORDS = false>
__device__ __forceinline__ void pdsch_mod_layers_body(const miphy_pdsch_mod_layers_job* __restrict__ lj, const uint16_t* list, int nof_list,
                                                      const miphy_precoding* __restrict__ pc, const float2* __restrict__ weights,
                                                      const uint8_t* __restrict__ cw_base, float2* __restrict__ grid, const uint32_t* __restrict__ seq_base,
                                                      const int* __restrict__ info_base, uint32_t stride,
                                                      const miphy_pdsch_mod_codewords_job* __restrict__ cj = nullptr)
{
  __shared__ pdsch_symbol_lds S;
  const miphy_pdsch_mod_job* __restrict__ jp = &lj->base;
  const int* info = info_base + (size_t)blockIdx.x * PDSCH_LAYERS_INFO;
  const int  sy = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (!info[15]) // invalid job, list or precoding (pdsch_seq_layers_body): skipped
    return;
  const int start_symbol = jp->start_symbol, nof_symbols = jp->nof_symbols;
  if (sy < start_symbol || sy >= start_symbol + nof_symbols)
    return;
  const int      prefix = info[sy]; // elements per layer of the transmission in earlier symbols
  const uint8_t* staged = SINK::stage(pc, tid);
  if (pdsch_symbol_setup(*jp, sy, S, tid, nt, list, nof_list) == 0)
    return;
  // (the dispatch of one codeword, written once for the two branches below: the wide-load sweeps where the codeword allows them -- 16QAM / 256QAM, the
  // symbol's first byte of the codeword aligned to words -- and the general loop otherwise; DONE leaves the codeword)
#define MIPHY_LAYERS_FAST(LL, MOD) pdsch_layers_fast<LL, MOD>(S, prefix, seq, cw, g, scale, scaling, tid)
#define MIPHY_MAP_CODEWORD(DONE)                                                                                                                       \
  if ((mod == 4 || mod == 8) && (((uintptr_t)(cw + (size_t)prefix * L * mod)) & 3u) == 0) {                                                           \
    switch (L * 16 + mod) {                                                                                                                           \
      case 1 * 16 + 4: MIPHY_LAYERS_FAST(1, 4); break;                                                                                                \
      case 2 * 16 + 4: MIPHY_LAYERS_FAST(2, 4); break;                                                                                                \
      case 3 * 16 + 4: MIPHY_LAYERS_FAST(3, 4); break;                                                                                                \
      case 4 * 16 + 4: MIPHY_LAYERS_FAST(4, 4); break;                                                                                                \
      case 1 * 16 + 8: MIPHY_LAYERS_FAST(1, 8); break;                                                                                                \
      case 2 * 16 + 8: MIPHY_LAYERS_FAST(2, 8); break;                                                                                                \
      case 3 * 16 + 8: MIPHY_LAYERS_FAST(3, 8); break;                                                                                                \
      default: MIPHY_LAYERS_FAST(4, 8); break;                                                                                                        \
    }                                                                                                                                                 \
    DONE;                                                                                                                                             \
  }                                                                                                                                                   \
  pdsch_map_elements(S, L, mod, prefix, seq, cw, g, scale, scaling, tid, nt);
  if constexpr (!CODEWORDS) {
    const int       mod = jp->mod, L = lj->nof_layers;
    const uint32_t* seq = seq_base + (size_t)blockIdx.x * stride;
    const float     scaling = jp->scaling;
    const bool      scale   = isnormal(scaling);
    const uint8_t*  cw      = cw_base + jp->cw_offset;
    const SINK      g(*lj, pc, weights, staged, grid + jp->grid_offset, sy, jp->grid_nof_prb * 12);
    MIPHY_MAP_CODEWORD(return)
  } else {
    // every field of the job into registers ahead of the first store: a load behind one is no scalar load any more
    // (nof_layers, mod1 and the eight ports as the three aligned words they lie in: byte loads would come back in vector registers and stay there across
    // the first codeword)
    static_assert(offsetof(miphy_pdsch_mod_codewords_job, nof_layers) % 4 == 0 && offsetof(miphy_pdsch_mod_codewords_job, mod1) == offsetof(miphy_pdsch_mod_codewords_job, nof_layers) + 1 &&
                      offsetof(miphy_pdsch_mod_codewords_job, ports) == offsetof(miphy_pdsch_mod_codewords_job, nof_layers) + 2,
                  "nof_layers, mod1 and ports[8] of a codewords job are read as three aligned words");
    const uint32_t* const       tail = reinterpret_cast<const uint32_t*>(&cj->nof_layers);
    const uint32_t              t0 = tail[0], t1 = tail[1], t2 = tail[2];
    const pdsch_codewords_split cs   = pdsch_codewords_split_of(t0 & 0xffu);
    const int                   mod0 = jp->mod, mod1 = (int)((t0 >> 8) & 0xffu), nsc = jp->grid_nof_prb * 12;
    const uint64_t              off0 = jp->cw_offset, off1 = cj->cw1_offset;
    float2* const               slot = grid + jp->grid_offset;
    const float                 scaling = jp->scaling;
    const bool                  scale   = isnormal(scaling);
    const uint64_t              ports   = (uint64_t)(t0 >> 16) | ((uint64_t)t1 << 16) | ((uint64_t)(t2 & 0xffffu) << 48); // ports[ly] in byte ly
    const uint32_t* const seq0 = seq_base + (size_t)blockIdx.x * 2u * stride;
    do {
      const int                mod = mod0, L = (int)cs.L0;
      const uint32_t*          seq = seq0;
      const uint8_t*           cw  = cw_base + off0;
      const pdsch_no_precoding g((uint32_t)ports, L, slot, sy, nsc);
      MIPHY_MAP_CODEWORD(break)
    } while (0);
    if (cs.L1) {
      const int                mod = mod1, L = (int)cs.L1;
      const uint32_t*          seq = seq0 + stride;
      const uint8_t*           cw  = cw_base + off1;
      const pdsch_no_precoding g((uint32_t)(ports >> (8u * cs.L0)), L, slot, sy, nsc);
      MIPHY_MAP_CODEWORD(return)
    }
  }
#undef MIPHY_MAP_CODEWORD
#undef MIPHY_LAYERS_FAST
}

__global__ void __launch_bounds__(256) pdsch_mod_layers_kernel(const miphy_pdsch_mod_layers_job* __restrict__ jobs, const uint8_t* __restrict__ cw_base,
                                                               float2* __restrict__ grid, const uint32_t* __restrict__ seq_base,
                                                               const int* __restrict__ info_base, uint32_t stride)
{
  pdsch_mod_layers_body<pdsch_no_precoding>(jobs + blockIdx.x, nullptr, 0, nullptr, nullptr, cw_base, grid, seq_base, info_base, stride);
}

// The mapping kernel of miphy_pdsch_modulate_mapped_batch: prb_of[] filled from the job's list. Only the order in which prb_of[] is filled differs, so
// everything behind it serves the list as it is. A job with nof_prb = 0 has no list.
__global__ void __launch_bounds__(256) pdsch_mod_mapped_kernel(const miphy_pdsch_mod_mapped_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                               const uint8_t* __restrict__ cw_base, float2* __restrict__ grid,
                                                               const uint32_t* __restrict__ seq_base, const int* __restrict__ info_base, uint32_t stride)
{
  const miphy_pdsch_mod_mapped_job* __restrict__ mj = jobs + blockIdx.x;
  const int nof_list = mj->nof_prb;
  pdsch_mod_layers_body<pdsch_no_precoding>(&mj->layers, nof_list ? prb_lists + mj->prb_list_offset : nullptr, nof_list, nullptr, nullptr, cw_base, grid, seq_base,
                                            info_base, stride);
}

// The mapping kernel of miphy_pdsch_modulate_codewords_batch: the mapped one, both codewords of a job in one workgroup.
__global__ void __launch_bounds__(256) pdsch_mod_codewords_kernel(const miphy_pdsch_mod_codewords_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                                  const uint8_t* __restrict__ cw_base, float2* __restrict__ grid,
                                                                  const uint32_t* __restrict__ seq_base, const int* __restrict__ info_base, uint32_t stride)
{
  const miphy_pdsch_mod_codewords_job* __restrict__ cj = jobs + blockIdx.x;
  const int nof_list = cj->mapped.nof_prb;
  pdsch_mod_layers_body<pdsch_no_precoding, true>(&cj->mapped.layers, nof_list ? prb_lists + cj->mapped.prb_list_offset : nullptr, nof_list, nullptr, nullptr,
                                                  cw_base, grid, seq_base, info_base, stride, cj);
}

// ---------------------------------------------------------------------------------------------------- precoding: layers to antenna ports
// Beyond the 23.5 reference, which has the precoder block (channel_precoder_generic.cpp:27-48, the contract of precode_sum) and the layout
// (precoding_configuration.h) and does not join them to its modulator.
__global__ void __launch_bounds__(512) pdsch_seq_precoded_kernel(const miphy_pdsch_mod_precoded_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                                 uint32_t nof_list_entries, uint32_t nof_weights, const gold_tables* __restrict__ gt,
                                                                 uint32_t* __restrict__ seq, int* __restrict__ info_out, uint32_t stride)
{
  const miphy_pdsch_mod_precoded_job* __restrict__ pj = jobs + blockIdx.x;
  pdsch_seq_layers_body(&pj->mapped.layers, &pj->mapped, prb_lists, nof_list_entries, gt, seq, info_out, stride, &pj->precoding, nof_weights);
}

// The mapping kernel of miphy_pdsch_modulate_precoded_batch: the mapped one whose elements go through a pdsch_precoder.
__global__ void __launch_bounds__(256) pdsch_mod_precoded_kernel(const miphy_pdsch_mod_precoded_job* __restrict__ jobs, const uint16_t* __restrict__ prb_lists,
                                                                 const float2* __restrict__ weights, const uint8_t* __restrict__ cw_base, float2* __restrict__ grid,
                                                                 const uint32_t* __restrict__ seq_base, const int* __restrict__ info_base, uint32_t stride)
{
  const miphy_pdsch_mod_precoded_job* __restrict__ pj = jobs + blockIdx.x;
  const int nof_list = pj->mapped.nof_prb;
  pdsch_mod_layers_body<pdsch_precoder>(&pj->mapped.layers, nof_list ? prb_lists + pj->mapped.prb_list_offset : nullptr, nof_list, &pj->precoding, weights, cw_base,
                                        grid, seq_base, info_base, stride);
}

// dmrs_pdsch_kernel for the L = nof_ports DM-RS ports 1000 .. 1000 + L - 1 of one codeword behind a precoding, through the same helpers: where that
// kernel stores r_ly on the grid port of DM-RS port ly, this one stores, on every antenna port,
// the sum over the layers of the RE's CDM group (layers 2 c and 2 c + 1 share group c, of type 1 and of type 2). A group without a layer is not written.
__global__ void __launch_bounds__(256) dmrs_pdsch_precoded_kernel(const miphy_dmrs_pdsch_precoded_job* __restrict__ jobs, const float2* __restrict__ weights,
                                                                  uint32_t nof_weights, const gold_tables* __restrict__ gt, float2* __restrict__ grid)
{
  __shared__ dmrs_pdsch_lds D;
  __shared__ uint64_t       full[5];
  __shared__ uint8_t        aports[16];
  const miphy_dmrs_pdsch_job* __restrict__ jp = &jobs[blockIdx.x].base;
  const miphy_precoding* __restrict__ pc      = &jobs[blockIdx.x].precoding;
  const int sy = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  if (!((jp->symbols_mask >> sy) & 1u) || !dmrs_precoded_fields_ok(*jp))
    return;
  dmrs_pdsch_load_mask(*jp, D, full, tid);
  if (tid >= 64 && tid < 80)
    aports[tid - 64] = pc->ports[tid - 64];
  __syncthreads();
  if (!pdsch_precoding_ok(*pc, jp->nof_ports, full, nof_weights)) // (uniform: before any weight is read)
    return;
  const dmrs_pdsch_symbol y = dmrs_pdsch_symbol_setup(*jp, sy, *gt, D, tid, nt);
  const int      nprb_grid = jp->grid_nof_prb, L = jp->nof_ports, P = pc->nof_ports;
  const unsigned prg_size = pc->prg_size;
  const float2*  W   = weights + pc->weights_offset;
  float2*        sym = grid + jp->grid_offset + (size_t)sy * (nprb_grid * 12);
  const size_t   pstride = (size_t)14 * (nprb_grid * 12);
  for (int idx = tid; idx < y.nprb * y.npr; idx += nt) {
    const dmrs_pdsch_re r  = dmrs_pdsch_re_of(D, y, idx);
    const float2*       wm = W + (size_t)((unsigned)r.rb / prg_size) * (unsigned)(P * L);
    for (int c = 0; 2 * c < L; ++c) { // CDM group c: DM-RS ports 2 c and 2 c + 1
      const int n = min(2, L - 2 * c);
      float2    x[4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float w = dmrs_pdsch_weight(2 * c + u, idx, y); // (ports below 4: w_t = 1)
        x[u]          = make_float2(r.re0 * w, r.im0 * w);
      }
      x[2] = x[3] = make_float2(0.f, 0.f);
      const int col = r.rb * 12 + r.k + (!y.type2 ? c : 2 * c);
      for (int a = 0; a < P; ++a)
        sym[aports[a] * pstride + col] = precode_sum(wm + a * L + 2 * c, x, n);
    }
  }
}

// channel_precoder::apply_precoding for a batch: workgroups (job, slice of its REs), one RE per thread and turn, all antenna ports in its loop -- the
// loads of a layer and the stores of a port run along the REs.
__global__ void __launch_bounds__(256) channel_precode_kernel(const miphy_precode_job* __restrict__ jobs, const float2* __restrict__ weights, uint32_t nof_weights,
                                                              const float2* __restrict__ in, float2* __restrict__ out)
{
  const miphy_precode_job& j = jobs[blockIdx.x];
  if (!precode_job_ok(j, nof_weights)) // (before any weight is read)
    return;
  const int      L = j.nof_layers, P = j.nof_ports;
  const uint32_t nof_re = j.nof_re;
  const float2*  w  = weights + j.weights_offset;
  const float2*  xi = in + j.in_offset;
  float2*        yo = out + j.out_offset;
  const uint64_t in_stride = j.in_stride, out_stride = j.out_stride;
  for (uint64_t i = blockIdx.y * blockDim.x + threadIdx.x; i < nof_re; i += gridDim.y * blockDim.x) {
    float2 x[4];
#pragma unroll
    for (int ly = 0; ly < 4; ++ly)
      x[ly] = ly < L ? xi[(uint64_t)ly * in_stride + i] : make_float2(0.f, 0.f);
    for (int a = 0; a < P; ++a)
      yo[(uint64_t)a * out_stride + i] = precode_sum(w + a * L, x, L);
  }
}

uint32_t host_nof_re(const miphy_pdsch_mod_job& j)
{
  const pdsch_keep_rule keep = pdsch_keep_rule_of(j);
  uint32_t              n    = 0;
  for (unsigned s = j.start_symbol; s < (unsigned)j.start_symbol + j.nof_symbols && s < 14; ++s)
    for (unsigned rb = 0; rb < j.grid_nof_prb; ++rb)
      if ((j.rb_mask[rb >> 6] >> (rb & 63)) & 1ull)
        n += (uint32_t)__builtin_popcount(pdsch_keep_mask(keep, s, rb, j.reserved[0].prb_mask, sizeof(miphy_re_pattern) / sizeof(uint64_t)));
  return n;
}

} // namespace

extern "C" uint32_t miphy_pdsch_mod_nof_re(const miphy_pdsch_mod_job* j)
{
  if (!j || (j->dmrs_type != 1 && j->dmrs_type != 2) || j->grid_nof_prb > 275 || j->nof_reserved > 4)
    return 0;
  return host_nof_re(*j);
}

int miphy_pdsch_mod_job_check(const char* who, const char* what, uint32_t i, const miphy_pdsch_mod_job& j, unsigned L, const uint8_t* ports, uint32_t nof_re)
{
  MIPHY_REQUIRE(L >= 1 && L <= 4, "%s: %s %u: invalid number of layers %u (one codeword: 1..4)", who, what, i, L);
  for (unsigned a = 0; ports && a < L; ++a) {
    MIPHY_REQUIRE(ports[a] < 16, "%s: %s %u: invalid port %u of layer %u", who, what, i, (unsigned)ports[a], a);
    for (unsigned b = 0; b < a; ++b)
      MIPHY_REQUIRE(ports[a] != ports[b], "%s: %s %u: layers %u and %u share port %u", who, what, i, b, a, (unsigned)ports[a]);
  }
#define PDSCH_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "%s: %s %u: " fmt, who, what, i, ##__VA_ARGS__);
  PDSCH_MOD_FIELD_RULES(PDSCH_RULE_REQUIRE)
#undef PDSCH_RULE_REQUIRE
  if (!ports)
    MIPHY_REQUIRE(j.port < 16, "%s: %s %u: invalid port", who, what, i);
  // pdsch_modulator_impl.cpp:158-160: every element of every layer must be mapped
  if (nof_re == 0)
    nof_re = host_nof_re(j);
  const uint32_t holds = nof_re * L * j.mod;
  if (!ports)
    MIPHY_REQUIRE(j.nof_bits == holds, "%s: %s %u: codeword of %u bits, the allocation holds %u", who, what, i, j.nof_bits, holds);
  else
    MIPHY_REQUIRE(j.nof_bits == holds, "%s: %s %u: codeword of %u bits, the allocation holds %u on %u layers", who, what, i, j.nof_bits, holds, L);
  return MIPHY_OK;
}

extern "C" int miphy_pdsch_modulate_batch(miphy_ctx* ctx, const miphy_pdsch_mod_job* jobs, int jobs_on_device, uint32_t n, const uint8_t* codewords,
                                          float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && codewords && grid, "miphy_pdsch_modulate_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "pdsch_modulate: batch too large (max 65535 transmissions per call)");
  for (uint32_t i = 0; !jobs_on_device && i < n; ++i)
    if (int rc = miphy_pdsch_mod_job_check("pdsch_modulate", "job", i, jobs[i], 1, nullptr, 0))
      return rc;
  hipStream_t        s  = (hipStream_t)stream;
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  const void* d_jobs = nullptr;
  rc                 = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pdsch_mod_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  void* seq = nullptr; // (the workspace the PUSCH demodulator keeps its sequences in)
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_SEQUENCES, miphy_pdsch_modulate_scratch_bytes(n), &seq)))
    return rc;
  return miphy_pdsch_modulate_launch((const miphy_pdsch_mod_job*)d_jobs, n, gt, codewords, grid, seq, s);
}

size_t miphy_pdsch_modulate_scratch_bytes(uint32_t n)
{
  return (size_t)n * PDSCH_SEQ_STRIDE * sizeof(uint32_t) + (size_t)n * 14 * sizeof(int);
}

int miphy_pdsch_modulate_launch(const miphy_pdsch_mod_job* d_jobs, uint32_t n, const gold_tables* gt, const uint8_t* codewords, float* grid, void* seq,
                                hipStream_t s)
{
  // seq: scrambling sequences of the transmissions, then their 14 symbol prefixes
  int* prefix = reinterpret_cast<int*>(static_cast<uint8_t*>(seq) + (size_t)n * PDSCH_SEQ_STRIDE * sizeof(uint32_t));
  hipLaunchKernelGGL(pdsch_seq_kernel, dim3(n), dim3(512), 0, s, d_jobs, gt, (uint32_t*)seq, prefix);
  hipLaunchKernelGGL(pdsch_mod_kernel, dim3(n, 14), dim3(256), 0, s, d_jobs, gt, codewords, (float2*)grid, (const uint32_t*)seq, (const int*)prefix);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- PDSCH modulator, 1..4 layers
extern "C" uint32_t miphy_pdsch_mod_layers_nof_re(const miphy_pdsch_mod_layers_job* j)
{
  if (!j || j->nof_layers < 1 || j->nof_layers > 4)
    return 0;
  return miphy_pdsch_mod_nof_re(&j->base);
}

namespace {
// The three layered entry points take one kind of job each -- miphy_pdsch_mod_layers_job, miphy_pdsch_mod_mapped_job (a layers job and its PRB list) or
// miphy_pdsch_mod_precoded_job (a mapped job and its precoding) -- and share everything else. The parts of a job: null where its kind has none.
struct pdsch_job_parts {
  const miphy_pdsch_mod_layers_job*    layers;
  const miphy_pdsch_mod_mapped_job*    mapped;
  const miphy_precoding*               precoding;
  const miphy_pdsch_mod_codewords_job* codewords; // (its layers part carries neither the layers nor the ports: the host holds it to its own check)
};
pdsch_job_parts parts_of(const miphy_pdsch_mod_layers_job& j) { return {&j, nullptr, nullptr, nullptr}; }
pdsch_job_parts parts_of(const miphy_pdsch_mod_mapped_job& j) { return {&j.layers, &j, nullptr, nullptr}; }
pdsch_job_parts parts_of(const miphy_pdsch_mod_precoded_job& j) { return {&j.mapped.layers, &j.mapped, &j.precoding, nullptr}; }
pdsch_job_parts parts_of(const miphy_pdsch_mod_codewords_job& j) { return {&j.mapped.layers, &j.mapped, nullptr, &j}; }

// The scratch of a layered call in MIPHY_WS_SEQUENCES: the scrambling sequences (a transmission on L layers has L times the bits of one layer: the stride
// grows with the batch's largest L), then PDSCH_LAYERS_INFO ints per transmission. A call on codewords jobs keeps nof_seq = 2 sequences per transmission,
// sequence 2 x transmission + q for codeword q, and max_layers is the largest layer count of one codeword (at most four).
struct pdsch_layers_scratch {
  uint32_t stride; // sequence words per transmission
  size_t   seq_bytes, bytes;
  int*     info(void* seq) const { return reinterpret_cast<int*>(static_cast<uint8_t*>(seq) + seq_bytes); }
};
pdsch_layers_scratch pdsch_layers_scratch_of(uint32_t n, uint32_t max_layers, uint32_t nof_seq = 1)
{
  const uint32_t stride    = max_layers * (uint32_t)PDSCH_SEQ_STRIDE;
  const size_t   seq_bytes = (size_t)n * nof_seq * stride * sizeof(uint32_t);
  return {stride, seq_bytes, seq_bytes + (size_t)n * PDSCH_LAYERS_INFO * sizeof(int)};
}

// What the three public functions do behind their null-argument test: the host's rules for every host job, in the order job, list, precoding (so the first
// message reported is that of the first rule the first bad job breaks), then the enqueue.
template <class JOB>
int pdsch_modulate_layered(const char* who, miphy_ctx* ctx, const JOB* jobs, int jobs_on_device, uint32_t n, const uint16_t* prb_lists, uint32_t nof_list_entries,
                           const float* weights, uint32_t nof_weights, const uint8_t* codewords, float* grid, void* stream)
{
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "%s: batch too large (max 65535 transmissions per call)", who);
  uint32_t max_layers = 4; // device-resident jobs: the kernels validate them, their lists and precodings; the scratch is sized for the most they may ask
                           // (a codewords job of eight layers among them: four layers per codeword)
  if (!jobs_on_device) {
    max_layers = 1;
    const uint8_t no_ports[4] = {0, 1, 2, 3}; // (a precoded job's layers.ports is ignored)
    for (uint32_t i = 0; i < n; ++i) {
      const pdsch_job_parts             j  = parts_of(jobs[i]);
      const miphy_pdsch_mod_layers_job& lj = *j.layers;
      if (j.codewords) { // (its own rules, those of the fields and of the list, in that order)
        if (int rc = miphy_pdsch_mod_codewords_check(who, "job", i, *j.codewords, prb_lists, nof_list_entries, 0))
          return rc;
        const pdsch_codewords_split cs = pdsch_codewords_split_of(j.codewords->nof_layers);
        max_layers                     = std::max(max_layers, std::max(cs.L0, cs.L1));
        continue;
      }
      int rc = miphy_pdsch_mod_job_check(who, "job", i, lj.base, lj.nof_layers, j.precoding ? no_ports : lj.ports, 0);
      if (!rc && j.mapped)
        rc = miphy_pdsch_mod_list_check(who, "job", i, *j.mapped, prb_lists, nof_list_entries);
      if (!rc && j.precoding)
        rc = miphy_precoding_check(who, "job", i, *j.precoding, lj.nof_layers, lj.base.rb_mask, nof_weights);
      if (rc)
        return rc;
      max_layers = lj.nof_layers > max_layers ? lj.nof_layers : max_layers;
    }
  }
  return miphy_pdsch_modulate_layered_enqueue(ctx, jobs, jobs_on_device, n, max_layers, prb_lists, nof_list_entries, weights, nof_weights, codewords, grid,
                                              (hipStream_t)stream);
}
} // namespace

template <class JOB>
int miphy_pdsch_modulate_layered_enqueue(miphy_ctx* ctx, const JOB* jobs, int jobs_on_device, uint32_t n, uint32_t max_layers, const uint16_t* prb_lists,
                                         uint32_t nof_list_entries, const float* weights, uint32_t nof_weights, const uint8_t* codewords, float* grid, hipStream_t s)
{
  constexpr bool     precoded = std::is_same<JOB, miphy_pdsch_mod_precoded_job>::value, cwjob = std::is_same<JOB, miphy_pdsch_mod_codewords_job>::value;
  constexpr bool     mapped   = precoded || cwjob || std::is_same<JOB, miphy_pdsch_mod_mapped_job>::value;
  const gold_tables* gt       = nullptr;
  int                rc       = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  const JOB*      d_jobs  = jobs;
  const uint16_t* d_lists = prb_lists;
  const float2*   d_w     = reinterpret_cast<const float2*>(weights);
  if (!jobs_on_device) { // host jobs with the host lists and host weights of their kind: one region of the staging ring, one upload
    device_image         img;
    const auto           js = img.put(jobs, (size_t)n);
    image_slot<uint16_t> ls;
    image_slot<float2>   ws;
    if (mapped)
      ls = img.put(prb_lists, (size_t)nof_list_entries);
    if (precoded)
      ws = img.put(d_w, (size_t)nof_weights);
    const void* base = nullptr;
    if ((rc = miphy_image_to_ring(ctx, img, s, &base)))
      return rc;
    d_jobs = js.at(base);
    if (mapped)
      d_lists = ls.at(base);
    if (precoded)
      d_w = ws.at(base);
  }
  const pdsch_layers_scratch sc  = pdsch_layers_scratch_of(n, max_layers, cwjob ? 2 : 1);
  void*                      seq = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_SEQUENCES, sc.bytes, &seq)))
    return rc;
  uint32_t* const sq = static_cast<uint32_t*>(seq);
  int* const      info = sc.info(seq);
  const dim3      chunks(n, 2 * max_layers, cwjob ? 2 : 1), symbols(n, 14);
  if constexpr (cwjob) {
    hipLaunchKernelGGL(pdsch_seq_codewords_kernel, chunks, dim3(512), 0, s, d_jobs, d_lists, nof_list_entries, gt, sq, info, sc.stride);
    hipLaunchKernelGGL(pdsch_mod_codewords_kernel, symbols, dim3(256), 0, s, d_jobs, d_lists, codewords, (float2*)grid, (const uint32_t*)sq, (const int*)info,
                       sc.stride);
  } else if constexpr (precoded) {
    hipLaunchKernelGGL(pdsch_seq_precoded_kernel, chunks, dim3(512), 0, s, d_jobs, d_lists, nof_list_entries, nof_weights, gt, sq, info, sc.stride);
    hipLaunchKernelGGL(pdsch_mod_precoded_kernel, symbols, dim3(256), 0, s, d_jobs, d_lists, d_w, codewords, (float2*)grid, (const uint32_t*)sq, (const int*)info,
                       sc.stride);
  } else if constexpr (mapped) {
    hipLaunchKernelGGL(pdsch_seq_mapped_kernel, chunks, dim3(512), 0, s, d_jobs, d_lists, nof_list_entries, gt, sq, info, sc.stride);
    hipLaunchKernelGGL(pdsch_mod_mapped_kernel, symbols, dim3(256), 0, s, d_jobs, d_lists, codewords, (float2*)grid, (const uint32_t*)sq, (const int*)info, sc.stride);
  } else {
    hipLaunchKernelGGL(pdsch_seq_layers_kernel, chunks, dim3(512), 0, s, d_jobs, gt, sq, info, sc.stride);
    hipLaunchKernelGGL(pdsch_mod_layers_kernel, symbols, dim3(256), 0, s, d_jobs, codewords, (float2*)grid, (const uint32_t*)sq, (const int*)info, sc.stride);
  }
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
#define PDSCH_ENQUEUE_FOR(JOB)                                                                                                                                 \
  template int miphy_pdsch_modulate_layered_enqueue<JOB>(miphy_ctx*, const JOB*, int, uint32_t, uint32_t, const uint16_t*, uint32_t, const float*, uint32_t,   \
                                                         const uint8_t*, float*, hipStream_t);
PDSCH_ENQUEUE_FOR(miphy_pdsch_mod_layers_job)
PDSCH_ENQUEUE_FOR(miphy_pdsch_mod_mapped_job)
PDSCH_ENQUEUE_FOR(miphy_pdsch_mod_precoded_job)
PDSCH_ENQUEUE_FOR(miphy_pdsch_mod_codewords_job)
#undef PDSCH_ENQUEUE_FOR

extern "C" int miphy_pdsch_modulate_layers_batch(miphy_ctx* ctx, const miphy_pdsch_mod_layers_job* jobs, int jobs_on_device, uint32_t n, const uint8_t* codewords,
                                                 float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && codewords && grid, "miphy_pdsch_modulate_layers_batch: null argument");
  return pdsch_modulate_layered("pdsch_modulate_layers", ctx, jobs, jobs_on_device, n, nullptr, 0, nullptr, 0, codewords, grid, stream);
}

// ---------------------------------------------------------------------------------------------------- PDSCH modulator, PRB lists in mapping order
extern "C" int miphy_vrb_to_prb_list(const miphy_vrb_to_prb* map, const uint64_t vrb_mask[5], uint16_t* prb_list, uint32_t cap, uint32_t* nof_prb,
                                     uint64_t prb_mask[5])
{
  MIPHY_REQUIRE(map && vrb_mask && nof_prb && (prb_list || cap == 0), "miphy_vrb_to_prb_list: null argument");
  const unsigned L = map->bundle_size, N = map->region_size_rb;
  MIPHY_REQUIRE(L == 0 || L == 2 || L == 4, "vrb_to_prb_list: invalid bundle size %u (0, 2 or 4)", L);
  MIPHY_REQUIRE(N >= 1 && N <= 275, "vrb_to_prb_list: invalid region size %u (1..275)", N);
  MIPHY_REQUIRE((unsigned)map->first_prb + N <= 275, "vrb_to_prb_list: the region [%u, %u + %u) exceeds 275 PRBs", (unsigned)map->first_prb,
                (unsigned)map->first_prb, N);
  unsigned count = 0;
  for (unsigned n = 0; n < 320; ++n)
    if ((vrb_mask[n >> 6] >> (n & 63)) & 1ull) {
      MIPHY_REQUIRE(n < N, "vrb_to_prb_list: VRB %u outside the region of %u", n, N);
      ++count;
    }
  *nof_prb = count;
  MIPHY_REQUIRE(count <= cap, "vrb_to_prb_list: %u PRBs for a list of %u", count, cap);
  // TS 38.211 7.3.1.6: bundles of L on a raster aligned to align_rb, the last one in place, the others through the 2 x C block interleaver
  const unsigned s = L ? map->align_rb % L : 0, nb = L ? (N + s + L - 1) / L : 0, C = nb / 2;
  uint64_t       set[5] = {};
  unsigned       i      = 0;
  for (unsigned n = 0; n < N; ++n) {
    if (!((vrb_mask[n >> 6] >> (n & 63)) & 1ull))
      continue;
    unsigned prb = map->first_prb + n;
    if (L) {
      const unsigned j = (n + s) / L, f = j == nb - 1 ? j : (j % 2) * C + j / 2;
      prb              = map->first_prb + f * L + (n + s) % L - s;
    }
    prb_list[i++] = (uint16_t)prb;
    set[prb >> 6] |= 1ull << (prb & 63);
  }
  for (int w = 0; prb_mask && w < 5; ++w)
    prb_mask[w] = set[w];
  return MIPHY_OK;
}

int miphy_pdsch_mod_list_check(const char* who, const char* what, uint32_t idx, const miphy_pdsch_mod_mapped_job& m, const uint16_t* prb_lists,
                               uint32_t nof_list_entries)
{
  if (m.nof_prb == 0)
    return MIPHY_OK;
  const uint64_t* rbm = m.layers.base.rb_mask;
  MIPHY_REQUIRE(prb_lists, "%s: %s %u: a PRB list and no list array", who, what, idx);
#define PDSCH_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "%s: %s %u: " fmt, who, what, idx, ##__VA_ARGS__);
  PDSCH_MOD_LIST_RULES(PDSCH_RULE_REQUIRE)
  uint64_t   seen[5]      = {};
  const auto test_and_set = [&seen](unsigned q) {
    const bool was = (seen[q >> 6] >> (q & 63)) & 1ull;
    seen[q >> 6] |= 1ull << (q & 63);
    return was;
  };
  for (unsigned i = 0; i < m.nof_prb; ++i) {
    const unsigned e = prb_lists[m.prb_list_offset + i];
    PDSCH_MOD_LIST_ENTRY_RULES(PDSCH_RULE_REQUIRE)
  }
#undef PDSCH_RULE_REQUIRE
  return MIPHY_OK;
}

extern "C" int miphy_pdsch_modulate_mapped_batch(miphy_ctx* ctx, const miphy_pdsch_mod_mapped_job* jobs, int jobs_on_device, uint32_t n, const uint16_t* prb_lists,
                                                 uint32_t nof_list_entries, const uint8_t* codewords, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && codewords && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_modulate_mapped_batch: null argument");
  return pdsch_modulate_layered("pdsch_modulate_mapped", ctx, jobs, jobs_on_device, n, prb_lists, nof_list_entries, nullptr, 0, codewords, grid, stream);
}

// ---------------------------------------------------------------------------------------------------- PDSCH modulator, one or two codewords on 1..8 layers
extern "C" uint32_t miphy_pdsch_mod_codewords_nof_re(const miphy_pdsch_mod_codewords_job* j)
{
  if (!j || j->nof_layers < 1 || j->nof_layers > 8)
    return 0;
  return miphy_pdsch_mod_nof_re(&j->mapped.layers.base);
}

int miphy_pdsch_mod_codewords_check(const char* who, const char* what, uint32_t i, const miphy_pdsch_mod_codewords_job& c, const uint16_t* prb_lists,
                                    uint32_t nof_list_entries, uint32_t nre)
{
#define PDSCH_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "%s: %s %u: " fmt, who, what, i, ##__VA_ARGS__);
  PDSCH_MOD_CODEWORDS_RULES(PDSCH_RULE_REQUIRE)
  const miphy_pdsch_mod_job& j = c.mapped.layers.base;
  PDSCH_MOD_FIELD_RULES(PDSCH_RULE_REQUIRE)
  if (int rc = miphy_pdsch_mod_list_check(who, what, i, c.mapped, prb_lists, nof_list_entries))
    return rc;
  if (nre == 0)
    nre = host_nof_re(j);
  const pdsch_codewords_split cs = pdsch_codewords_split_of(c.nof_layers);
  PDSCH_MOD_CODEWORDS_SIZE_RULES(PDSCH_RULE_REQUIRE)
#undef PDSCH_RULE_REQUIRE
  return MIPHY_OK;
}

extern "C" int miphy_pdsch_modulate_codewords_batch(miphy_ctx* ctx, const miphy_pdsch_mod_codewords_job* jobs, int jobs_on_device, uint32_t n,
                                                    const uint16_t* prb_lists, uint32_t nof_list_entries, const uint8_t* codewords, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && codewords && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_modulate_codewords_batch: null argument");
  return pdsch_modulate_layered("pdsch_modulate_codewords", ctx, jobs, jobs_on_device, n, prb_lists, nof_list_entries, nullptr, 0, codewords, grid, stream);
}

extern "C" int miphy_dmrs_pdsch_map_batch(miphy_ctx* ctx, const miphy_dmrs_pdsch_job* jobs, int jobs_on_device, uint32_t n, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && grid, "miphy_dmrs_pdsch_map_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "dmrs_pdsch_map: batch too large (max 65535 transmissions per call)");
  if (!jobs_on_device) {
    for (uint32_t i = 0; i < n; ++i) {
      const miphy_dmrs_pdsch_job& j = jobs[i];
      MIPHY_REQUIRE(j.dmrs_type == 1 || j.dmrs_type == 2, "dmrs_pdsch_map: job %u: invalid DM-RS type", i);
      MIPHY_REQUIRE(j.nof_ports >= 1 && j.nof_ports <= (j.dmrs_type == 1 ? 8 : 12), "dmrs_pdsch_map: job %u: invalid number of ports", i);
      MIPHY_REQUIRE(j.grid_nof_prb >= 1 && j.grid_nof_prb <= 275 && j.reference_point_k_rb < j.grid_nof_prb, "dmrs_pdsch_map: job %u: invalid grid", i);
      MIPHY_REQUIRE(j.symbols_mask < (1u << 14), "dmrs_pdsch_map: job %u: invalid symbol mask", i);
    }
  }
  hipStream_t        s  = (hipStream_t)stream;
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  const void* d_jobs = nullptr;
  rc                 = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_dmrs_pdsch_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  return miphy_dmrs_pdsch_map_launch((const miphy_dmrs_pdsch_job*)d_jobs, n, gt, grid, s);
}

int miphy_dmrs_pdsch_map_launch(const miphy_dmrs_pdsch_job* d_jobs, uint32_t n, const gold_tables* gt, float* grid, hipStream_t s)
{
  hipLaunchKernelGGL(dmrs_pdsch_kernel, dim3(n, 14), dim3(256), 0, s, d_jobs, gt, (float2*)grid);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- precoding
int miphy_precoding_check(const char* who, const char* what, uint32_t idx, const miphy_precoding& p, unsigned L, const uint64_t* rbm, uint32_t nof_weights)
{
#define PDSCH_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "%s: %s %u: " fmt, who, what, idx, ##__VA_ARGS__);
  PDSCH_PRECODING_RULES(PDSCH_RULE_REQUIRE)
#undef PDSCH_RULE_REQUIRE
  return MIPHY_OK;
}

extern "C" int miphy_channel_precode_batch(miphy_ctx* ctx, const miphy_precode_job* jobs, int jobs_on_device, uint32_t n, const float* weights,
                                           uint32_t nof_weights, const float* in, float* out, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && weights && in && out, "miphy_channel_precode_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "channel_precode: batch too large (max 65535 jobs per call)");
  hipStream_t              s       = (hipStream_t)stream;
  const miphy_precode_job* d_jobs  = jobs;
  const float2*            d_w     = reinterpret_cast<const float2*>(weights);
  uint32_t                 slices  = 16; // device-resident jobs: their sizes are not known here, every workgroup strides over its job's REs
  if (!jobs_on_device) {
    uint32_t max_re = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const miphy_precode_job& j = jobs[i];
#define PRECODE_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "channel_precode: job %u: " fmt, i, ##__VA_ARGS__);
      PRECODE_JOB_RULES(PRECODE_RULE_REQUIRE)
#undef PRECODE_RULE_REQUIRE
      max_re = j.nof_re > max_re ? j.nof_re : max_re;
    }
    if (max_re == 0)
      return MIPHY_OK;
    slices = (max_re + 255u) / 256u < 64u ? (max_re + 255u) / 256u : 64u;
    device_image img; // host jobs and host weights: one region of the staging ring, one upload
    const auto   js   = img.put(jobs, (size_t)n);
    const auto   ws   = img.put(d_w, (size_t)nof_weights);
    const void*  base = nullptr;
    if (int rc = miphy_image_to_ring(ctx, img, s, &base))
      return rc;
    d_jobs = js.at(base), d_w = ws.at(base);
  }
  hipLaunchKernelGGL(channel_precode_kernel, dim3(n, slices), dim3(256), 0, s, d_jobs, d_w, nof_weights, (const float2*)in, (float2*)out);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_pdsch_modulate_precoded_batch(miphy_ctx* ctx, const miphy_pdsch_mod_precoded_job* jobs, int jobs_on_device, uint32_t n,
                                                   const uint16_t* prb_lists, uint32_t nof_list_entries, const float* weights, uint32_t nof_weights,
                                                   const uint8_t* codewords, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && weights && codewords && grid && (prb_lists || nof_list_entries == 0), "miphy_pdsch_modulate_precoded_batch: null argument");
  return pdsch_modulate_layered("pdsch_modulate_precoded", ctx, jobs, jobs_on_device, n, prb_lists, nof_list_entries, weights, nof_weights, codewords, grid, stream);
}

int miphy_dmrs_pdsch_precoded_job_check(const char* who, const char* what, uint32_t i, const miphy_dmrs_pdsch_precoded_job& pj, uint32_t nof_weights)
{
  const miphy_dmrs_pdsch_job& j = pj.base;
#define DMRS_RULE_REQUIRE(cond, fmt, ...) MIPHY_REQUIRE(cond, "%s: %s %u: " fmt, who, what, i, ##__VA_ARGS__);
  DMRS_PRECODED_FIELD_RULES(DMRS_RULE_REQUIRE)
#undef DMRS_RULE_REQUIRE
  return miphy_precoding_check(who, what, i, pj.precoding, j.nof_ports, j.rb_mask, nof_weights);
}

extern "C" int miphy_dmrs_pdsch_map_precoded_batch(miphy_ctx* ctx, const miphy_dmrs_pdsch_precoded_job* jobs, int jobs_on_device, uint32_t n, const float* weights,
                                                   uint32_t nof_weights, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && weights && grid, "miphy_dmrs_pdsch_map_precoded_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "dmrs_pdsch_map_precoded: batch too large (max 65535 transmissions per call)");
  for (uint32_t i = 0; !jobs_on_device && i < n; ++i)
    if (int rc = miphy_dmrs_pdsch_precoded_job_check("dmrs_pdsch_map_precoded", "job", i, jobs[i], nof_weights))
      return rc;
  hipStream_t        s  = (hipStream_t)stream;
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  const miphy_dmrs_pdsch_precoded_job* d_jobs = jobs;
  const float2*                        d_w    = reinterpret_cast<const float2*>(weights);
  if (!jobs_on_device) {
    device_image img;
    const auto   js   = img.put(jobs, (size_t)n);
    const auto   ws   = img.put(d_w, (size_t)nof_weights);
    const void*  base = nullptr;
    if ((rc = miphy_image_to_ring(ctx, img, s, &base)))
      return rc;
    d_jobs = js.at(base), d_w = ws.at(base);
  }
  hipLaunchKernelGGL(dmrs_pdsch_precoded_kernel, dim3(n, 14), dim3(256), 0, s, d_jobs, d_w, nof_weights, gt, (float2*)grid);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- PDCCH processor
extern "C" int miphy_pdcch_process_batch(miphy_ctx* ctx, const miphy_pdcch_pdu* pdus, uint32_t n, const uint8_t* payloads, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && payloads && grid, "miphy_pdcch_process_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "pdcch_process: at most 65535 PDUs per call");
  hipStream_t                  s = (hipStream_t)stream;
  std::vector<miphy_pdcch_pdu> p(pdus, pdus + n);
  size_t                       enc_bytes = 0;
  for (uint32_t i = 0; i < n; ++i) {
    miphy_pdcch_pdu& q  = p[i];
    const unsigned   al = q.aggregation_level;
    MIPHY_REQUIRE(al == 1 || al == 2 || al == 4 || al == 8 || al == 16, "pdcch_process: PDU %u: invalid aggregation level %u", i, al);
    MIPHY_REQUIRE(q.duration >= 1 && q.duration <= 3 && q.start_symbol + q.duration <= 14, "pdcch_process: PDU %u: invalid CORESET duration", i);
    MIPHY_REQUIRE(q.payload_size >= 12 && q.payload_size <= 128, "pdcch_process: PDU %u: payload size %u out of range (12..128)", i, (unsigned)q.payload_size);
    MIPHY_REQUIRE(q.grid_nof_prb >= 1 && q.grid_nof_prb <= 275 && q.reference_point_k_rb < q.grid_nof_prb, "pdcch_process: PDU %u: invalid grid", i);
    MIPHY_REQUIRE(q.rnti <= 0xffff && q.n_rnti <= 0xffff && q.n_id_pdcch_data <= 0xffff && q.n_id_pdcch_dmrs <= 0xffff, "pdcch_process: PDU %u: identifier out of range", i);
    unsigned nprb = 0;
    for (unsigned r = 0; r < q.grid_nof_prb; ++r)
      nprb += (unsigned)((q.rb_mask[r >> 6] >> (r & 63)) & 1ull);
    // E = aggregation level x 6 REG x 9 RE x 2 bits must fill the PRBs of the mask over the CORESET symbols
    MIPHY_REQUIRE(nprb * q.duration == 6u * al, "pdcch_process: PDU %u: %u PRBs x %u symbols do not match aggregation level %u", i, nprb, (unsigned)q.duration, al);
    q.work_offset = enc_bytes;
    enc_bytes += (108u * al + 15u) & ~15u;
  }
  void* work = nullptr;
  int   rc   = miphy_get_workspace(ctx, MIPHY_WS_OUTPUT, enc_bytes + 64, &work);
  if (rc)
    return rc;
  const void* d_pdus = nullptr;
  if ((rc = miphy_stage_descs(ctx, p.data(), 0, sizeof(miphy_pdcch_pdu) * (size_t)n, s, &d_pdus)))
    return rc;
  const gold_tables* gt = nullptr;
  if ((rc = miphy_get_gold_tables(ctx, &gt)))
    return rc;
  uint8_t* d_enc = static_cast<uint8_t*>(work);
  for (uint32_t i = 0; i < n; ++i) { // a handful of PDUs per slot: one small launch each (the code depends on payload size and level)
    const miphy_pdcch_pdu* dq = static_cast<const miphy_pdcch_pdu*>(d_pdus) + i;
    if ((rc = miphy_pdcch_encode_batch(ctx, p[i].payload_size, 108u * p[i].aggregation_level, 1, payloads + p[i].payload_offset,
                                       reinterpret_cast<const uint16_t*>(&dq->rnti), d_enc + p[i].work_offset, s)))
      return rc;
  }
  hipLaunchKernelGGL(pdcch_map_kernel, dim3(n, 3), dim3(256), 0, s, (const miphy_pdcch_pdu*)d_pdus, gt, d_enc, (float2*)grid);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- SS/PBCH block processor
extern "C" int miphy_ssb_process_batch(miphy_ctx* ctx, const miphy_ssb_pdu* pdus, uint32_t n, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && pdus && grid, "miphy_ssb_process_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "ssb_process: at most 65535 blocks per call");
  hipStream_t                 s = (hipStream_t)stream;
  std::vector<miphy_pbch_msg> msgs(n);
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_ssb_pdu& q = pdus[i];
    MIPHY_REQUIRE(q.msg.N_id < 1008, "ssb_process: block %u: invalid physical cell identity %u", i, q.msg.N_id);
    MIPHY_REQUIRE(q.msg.L_max == 4 || q.msg.L_max == 8 || q.msg.L_max == 64, "ssb_process: block %u: invalid L_max %u", i, q.msg.L_max);
    MIPHY_REQUIRE(q.nof_ports >= 1 && q.nof_ports <= 4, "ssb_process: block %u: invalid number of ports", i);
    MIPHY_REQUIRE(q.grid_nof_prb >= 20 && q.grid_nof_prb <= 275 && q.ssb_first_subcarrier + 240u <= q.grid_nof_prb * 12u, "ssb_process: block %u: the block does not fit the grid",
                  i);
    MIPHY_REQUIRE(q.ssb_first_symbol + 4u <= 14u, "ssb_process: block %u: the block does not fit the slot", i);
    msgs[i] = q.msg;
  }
  void* work = nullptr; // encoded PBCH bits, 864 per block
  int   rc   = miphy_get_workspace(ctx, MIPHY_WS_OUTPUT, (size_t)n * 864 + 64, &work);
  if (rc)
    return rc;
  if ((rc = miphy_pbch_encode_batch(ctx, msgs.data(), n, static_cast<uint8_t*>(work), s)))
    return rc;
  const void* d_pdus = nullptr;
  if ((rc = miphy_stage_descs(ctx, pdus, 0, sizeof(miphy_ssb_pdu) * (size_t)n, s, &d_pdus)))
    return rc;
  const gold_tables* gt = nullptr;
  if ((rc = miphy_get_gold_tables(ctx, &gt)))
    return rc;
  hipLaunchKernelGGL(ssb_map_kernel, dim3(n), dim3(256), 0, s, (const miphy_ssb_pdu*)d_pdus, gt, static_cast<const uint8_t*>(work), (float2*)grid);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- NZP-CSI-RS generator
extern "C" int miphy_csi_rs_map_batch(miphy_ctx* ctx, const miphy_csi_rs_job* jobs, int jobs_on_device, uint32_t n, float* grid, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && grid, "miphy_csi_rs_map_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "csi_rs_map: at most 65535 jobs per call");
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i) {
      const miphy_csi_rs_job& j = jobs[i];
      MIPHY_REQUIRE(j.nof_ports >= 1 && j.nof_ports <= 16, "csi_rs_map: job %u: invalid number of ports %u", i, (unsigned)j.nof_ports);
      MIPHY_REQUIRE(j.cdm <= 3 && j.freq_density <= 3, "csi_rs_map: job %u: invalid CDM type or density", i);
      MIPHY_REQUIRE(j.grid_nof_prb >= 1 && j.grid_nof_prb <= 275 && (unsigned)j.start_rb + j.nof_rb <= j.grid_nof_prb && j.rb_end <= j.grid_nof_prb && j.nof_rb >= 1,
                    "csi_rs_map: job %u: the PRB range exceeds the grid", i);
      MIPHY_REQUIRE(j.rb_stride >= 1 && j.rb_begin <= j.rb_end, "csi_rs_map: job %u: invalid PRB pattern", i);
      const unsigned per_symbol = (j.freq_density == 3 ? 3u : 1u) * (j.cdm ? 2u : 1u) * j.nof_rb;
      MIPHY_REQUIRE(per_symbol <= 1000, "csi_rs_map: job %u: sequence too long", i);
      for (unsigned p = 0; p < j.nof_ports; ++p)
        MIPHY_REQUIRE(j.re_mask[p] != 0 && j.re_mask[p] < (1u << 12) && j.symbol_mask[p] != 0 && j.symbol_mask[p] < (1u << 14), "csi_rs_map: job %u: port %u: invalid pattern", i, p);
    }
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  int         rc     = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_csi_rs_job) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  const gold_tables* gt = nullptr;
  if ((rc = miphy_get_gold_tables(ctx, &gt)))
    return rc;
  hipLaunchKernelGGL(csi_rs_kernel, dim3(n, 16, 14), dim3(256), 0, s, (const miphy_csi_rs_job*)d_jobs, gt, (float2*)grid);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
