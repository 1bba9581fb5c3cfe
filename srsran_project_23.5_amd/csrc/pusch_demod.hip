// PUSCH demodulator: resource-element extraction, ZF / MRC equalisation over the receive ports, soft demapping to int8 LLRs and
// descrambling, fused in one pass over the resource grid -- one workgroup per (transmission, OFDM symbol).
//
// Behaviour contract:
//   lib/phy/upper/channel_processors/pusch_demodulator_impl.cpp:31-152, pusch_demodulator_impl.h:74-172 (which REs, in which order)
//   lib/phy/upper/equalization/channel_equalizer_zf_impl.cpp:123-162, equalize_zf_1xn.h:42-158 (one transmit layer)
//   lib/phy/upper/channel_modulation/demodulation_mapper_impl.cpp:34-106, demodulation_mapper_{qpsk,qam16,qam64,qam256}.cpp and
//   avx2_helpers.h:103-236 (interval functions, quantisation: scale by 120/range, clip, round to nearest even)
//   descrambling: c_init = rnti * 2^15 + n_id, TS 38.211 6.3.1.1 (no UCI placeholders).
// The equalised symbols and noise variances never leave registers; HBM sees the grid and the channel estimate once and the LLRs
// once. The descrambling sequence of the symbol is produced in LDS by jumping the two LFSRs to the symbol's first bit
// (gold_device.h). Floating point: single IEEE operations in a fixed order (no contraction), exact division,
// so the LLRs are reproducible bit for bit by a scalar CPU restatement; against the reference AVX2 build they are within one step.
// Beyond the reference: 1..4 layers (zero forcing, equalize_device.h), transform precoding, and MMSE-IRC on 1..4 layers (mmse_device.h) in the
// frame of the layered walk.
#define NR_DEMOD_TABLE_ATTR __device__
#include "gold_device.h"
#include "demod_device.h"
#include "equalize_device.h"
#include "mmse_device.h"
#include "mod_device.h"
#include "tp_device.h"
#include "miphy_ext.h"
#include "tables/nr_demod_tables.h"
#include <cmath>

namespace {

// LDS copy of the interval tables of one modulation: level k (bits 2k, 2k+1) at tab[16 k ...], {slope, intercept} pairs. In two steps:
// the lanes request their table entry from memory (demod_table_entry) as soon as the modulation is known, and put it into LDS
// (demod_table_store) after the work that does not need it -- the request is one of the dependent memory round trips at the head of every
// workgroup (arguments -> descriptor -> tables -> samples), this takes it off the chain.
struct demod_tab_entry {
  int    idx; // position in tab[], -1: this lane holds none
  float2 v;
};
__device__ __forceinline__ demod_tab_entry demod_table_entry(int mod, int tid)
{
  demod_tab_entry e;
  e.idx = -1, e.v = make_float2(0.f, 0.f);
  if (mod == 6) {
    if (tid < 8)
      e.idx = tid, e.v = make_float2(NR_DEMOD_QAM64_B0_SLOPE[tid], NR_DEMOD_QAM64_B0_INTERCEPT[tid]);
    else if (tid < 16)
      e.idx = 16 + tid - 8, e.v = make_float2(NR_DEMOD_QAM64_B1_SLOPE[tid - 8], NR_DEMOD_QAM64_B1_INTERCEPT[tid - 8]);
    else if (tid < 20)
      e.idx = 32 + tid - 16, e.v = make_float2(NR_DEMOD_QAM64_B2_SLOPE[tid - 16], NR_DEMOD_QAM64_B2_INTERCEPT[tid - 16]);
  } else if (mod == 8) {
    if (tid < 16)
      e.idx = tid, e.v = make_float2(NR_DEMOD_QAM256_B0_SLOPE[tid], NR_DEMOD_QAM256_B0_INTERCEPT[tid]);
    else if (tid < 32)
      e.idx = tid, e.v = make_float2(NR_DEMOD_QAM256_B1_SLOPE[tid - 16], NR_DEMOD_QAM256_B1_INTERCEPT[tid - 16]);
    else if (tid < 48)
      e.idx = tid, e.v = make_float2(NR_DEMOD_QAM256_B2_SLOPE[tid - 32], NR_DEMOD_QAM256_B2_INTERCEPT[tid - 32]);
    else if (tid < 56)
      e.idx = tid, e.v = make_float2(NR_DEMOD_QAM256_B3_SLOPE[tid - 48], NR_DEMOD_QAM256_B3_INTERCEPT[tid - 48]);
  }
  return e;
}
__device__ __forceinline__ void demod_table_store(float2* tab, const demod_tab_entry& e)
{
  if (e.idx >= 0)
    tab[e.idx] = e.v;
}

// The common case in one pass: finite symbol and noise (FAST above), no EVM, no placeholders, MOD >= 2. Descrambling is folded into
// the quantisation scale (chip b set: scale -> -scale; clip and round-to-nearest-even are symmetric, so the LLR is negated exactly),
// and rounding + conversion into adding 1.5 * 2^23: the sum is rounded to nearest even at unit spacing and its low mantissa byte is
// the two's complement int8 of the result. Returns the MOD bytes packed, LLR b in byte b. Same values as demod_symbol<MOD, true>
// followed by the sign flip.
__device__ __forceinline__ uint32_t demod_qbyte(float v, float scale, uint32_t chips, int b)
{
#pragma clang fp contract(off)
  const float sc = __uint_as_float(((chips << (31 - b)) & 0x80000000u) | __float_as_uint(scale));
  return __float_as_uint(__builtin_amdgcn_fmed3f(v * sc, -120.0f, 120.0f) + 12582912.0f);
}
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  const uint32_t ab = __builtin_amdgcn_perm(b, a, 0x0c0c0400u), cd = __builtin_amdgcn_perm(d, c, 0x0c0c0400u);
  return __builtin_amdgcn_perm(cd, ab, 0x05040100u);
}
template <int MOD>
__device__ __forceinline__ uint64_t demod_symbol_packed(float re, float im, float nvar, const float2* tab, uint32_t chips)
{
#pragma clang fp contract(off)
  const float rcp  = (nvar > 0.f) ? 1.0f / nvar : 0.0f;
  const float x[2] = {re, im};
  uint32_t    q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    if (MOD == 2) {
      q[d] = demod_qbyte((NR_DEMOD_QPSK_GAIN * x[d]) * rcp, 120.0f / 24.f, chips, d);
    } else if (MOD == 4) {
      const float first  = NR_DEMOD_QAM16_GAIN * x[d];
      const float second = 2.0f * first - copysignf(0.8f, x[d]);
      const float l01    = (fabsf(x[d]) > NR_DEMOD_QAM16_THRESHOLD) ? second : first;
      const float l23    = 0.8f - fabsf(first);
      q[d]               = demod_qbyte(l01 * rcp, 6.0f, chips, d);
      q[2 + d]           = demod_qbyte(l23 * rcp, 6.0f, chips, 2 + d);
    } else if (MOD == 6) {
      const int i0 = demod_interval_idx(x[d], NR_DEMOD_QAM64_B0_RCP_WIDTH, 8);
      const int i2 = demod_interval_idx(x[d], NR_DEMOD_QAM64_B2_RCP_WIDTH, 4);
      q[d]         = demod_qbyte(demod_interval_at(x[d], rcp, tab[i0]), 6.0f, chips, d);
      q[2 + d]     = demod_qbyte(demod_interval_at(x[d], rcp, tab[16 + i0]), 6.0f, chips, 2 + d);
      q[4 + d]     = demod_qbyte(demod_interval_at(x[d], rcp, tab[32 + i2]), 6.0f, chips, 4 + d);
    } else {
      const int i0 = demod_interval_idx(x[d], NR_DEMOD_QAM256_B0_RCP_WIDTH, 16);
      const int i3 = demod_interval_idx(x[d], NR_DEMOD_QAM256_B3_RCP_WIDTH, 8);
      q[d]         = demod_qbyte(demod_interval_at(x[d], rcp, tab[i0]), 6.0f, chips, d);
      q[2 + d]     = demod_qbyte(demod_interval_at(x[d], rcp, tab[16 + i0]), 6.0f, chips, 2 + d);
      q[4 + d]     = demod_qbyte(demod_interval_at(x[d], rcp, tab[32 + i0]), 6.0f, chips, 4 + d);
      q[6 + d]     = demod_qbyte(demod_interval_at(x[d], rcp, tab[48 + i3]), 6.0f, chips, 6 + d);
    }
  }
  const uint32_t lo = pack4(q[0], q[1], q[2], q[3]);
  const uint32_t hi = MOD > 4 ? pack4(q[4], q[5], q[6], q[7]) : 0u;
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// 12-bit mask of the REs of a PRB that carry DM-RS (dmrs_mapping.h:76-92).
__device__ __forceinline__ unsigned dmrs_prb_mask(int type, unsigned cdm)
{
  unsigned m = 0;
  for (unsigned k = 0; k < 12; ++k)
    m |= ((type == 1) ? ((k % 2) < cdm) : ((k % 6) < 2 * cdm)) ? (1u << k) : 0u;
  return m;
}

struct demod_args {
  int           nsc, nports, ce_nof_symbols;
  uint32_t      rxp; // rx_ports[0..3], one byte each
  const float2* grid;
  const float2* ce;
  int8_t*       llr;
  float         noise_var;
  const uint16_t* ph;  // repetition placeholders of this transmission (sorted RE indices), nph of them
  int             nph;
  float*          evm_part; // per (OFDM symbol, chunk) partial sums of |hard-decided symbol - equalised symbol|^2 of this transmission, or nullptr
  const uint32_t* seq;      // the transmission's scrambling sequence (pusch_seq_kernel)
  int             start_symbol, end_symbol, per_dm, nprb;
  int             prefix0; // data elements of the transmission before start_symbol (a workgroup may own a part of the symbols)
  unsigned        dmrs_syms;
};

constexpr int DEMOD_THREADS = 256;
constexpr int DEMOD_MAX_CHUNKS = (275 * 12 + DEMOD_THREADS - 1) / DEMOD_THREADS; // 13

// MOD soft bits packed in w (LLR b in byte b) to q: one wide store where q is aligned to it (demod_aligned), bytes otherwise. The one-layer
// walks test the first element of a symbol (uniform: a scalar branch), the layered ones q itself; the two agree for every MOD, since the
// elements of a symbol lie MOD bytes apart.
template <int MOD>
__device__ __forceinline__ bool demod_aligned(const int8_t* q)
{
  return ((uintptr_t)q % (MOD == 8 ? 8 : MOD == 4 ? 4 : MOD == 1 ? 1 : 2)) == 0;
}
template <int MOD>
__device__ __forceinline__ void demod_store(uint64_t w, int8_t* q, bool aligned)
{
  if (aligned) {
    if (MOD == 8)
      *reinterpret_cast<uint2*>(q) = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
    else if (MOD == 6) {
      uint16_t* q2 = reinterpret_cast<uint16_t*>(q);
      q2[0] = (uint16_t)w, q2[1] = (uint16_t)(w >> 16), q2[2] = (uint16_t)(w >> 32);
    } else if (MOD == 4)
      *reinterpret_cast<uint32_t*>(q) = (uint32_t)w;
    else if (MOD == 2)
      *reinterpret_cast<uint16_t*>(q) = (uint16_t)w;
    else
      q[0] = (int8_t)w;
  } else {
#pragma unroll
    for (int b = 0; b < MOD; ++b)
      q[b] = (int8_t)(w >> (8 * b));
  }
}

// The soft bits l[0 .. MOD - 1] descrambled with the low MOD bits of `bits` (chip set: negated), packed as demod_store takes them.
template <int MOD>
__device__ __forceinline__ uint64_t demod_descramble_pack(const int* l, uint32_t bits)
{
  uint64_t w = 0;
#pragma unroll
  for (int b = 0; b < MOD; ++b) {
    const int m = -(int)((bits >> b) & 1u); // 0 / -1
    w |= (uint64_t)(uint8_t)(int8_t)((l[b] ^ m) - m) << (8 * b);
  }
  return w;
}

// Whether element `re` of the codeword is in the transmission's placeholder list: binary search (pusch_demodulator_impl.cpp:117-149).
__device__ __forceinline__ bool demod_is_placeholder(const demod_args& a, unsigned re)
{
  for (int lo = 0, hi = a.nph - 1; lo <= hi;) {
    const int      mid = (lo + hi) >> 1;
    const unsigned v   = a.ph[mid];
    if (v == re)
      return true;
    if (v < re)
      lo = mid + 1;
    else
      hi = mid - 1;
  }
  return false;
}

// EVM partial of the workgroup for symbol sy from every thread's term, in one order whatever the launch: wavefront shuffle tree, then the four
// wavefronts in sequence; thread 0 writes it. Every thread of the workgroup calls it (barriers).
__device__ __forceinline__ void demod_evm_sum(const demod_args& a, int sy, float evm_acc, float* evm_red, int tid)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    evm_acc += __shfl_xor(evm_acc, off);
  __syncthreads();
  if ((tid & 63) == 0)
    evm_red[tid >> 6] = evm_acc;
  __syncthreads();
  if (tid == 0)
    a.evm_part[sy * DEMOD_MAX_CHUNKS + blockIdx.y] = ((evm_red[0] + evm_red[1]) + evm_red[2]) + evm_red[3];
}

// One thread = one allocated subcarrier, walked over the OFDM symbols of the allocation: with the compact estimate (one row per port,
// valid for every symbol) the channel coefficients, 1 / sum |h|^2, the post-equalisation noise variance and its reciprocal are
// computed ONCE and stay in registers -- per resource element only the received sample is loaded (the next symbol's is requested
// before the current one is worked on). The values are those of the per-element computation (same operations, same order).
// active: the thread owns a subcarrier; a_idx: its index among the allocated subcarriers (= its rank among the data elements of a
// symbol without DM-RS); r_dm: its rank among the data elements of a DM-RS symbol, -1 when it carries DM-RS there.
// The common case of demod_columns (below) with every memory request of the thread in flight at once: compact estimate, NP receive
// ports known at compile time, no EVM, no placeholders, MOD >= 2. The walk over the OFDM symbols is unrolled; the received samples of
// ALL symbols and their descrambling words are requested before the first one is worked on (one memory latency per thread instead of
// one per symbol: with a lookahead of one symbol the wavefronts of a CU spent 54 % of their cycles waiting), and are consumed in
// request order (the counter waits of the in-order returns fall out of the unrolled code). Same operations in the same order as the
// general walk, so the LLRs are identical. A descrambling window of MOD bits never straddles a word unless MOD == 6: one word then.
template <int MOD, int NP>
__device__ __forceinline__ void demod_columns_deep(const demod_args& a, bool active, int sc, int a_idx, int r_dm, const float2* tab)
{
#pragma clang fp contract(off)
  constexpr int NS  = 14;
  const int     nsc = a.nsc;
  const float2* gp[NP];
  float2        h[NP];
  // Every request is unconditional (a branch around a load makes the compiler wait for ALL outstanding loads where the paths join):
  // symbols behind the allocation repeat its last one, a lane without a subcarrier uses subcarrier sc = 0 and element 0, a DM-RS element
  // reads the word of element 0 of its symbol; what they compute is never stored.
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    gp[p] = a.grid + (size_t)((a.rxp >> (8 * p)) & 0xffu) * 14 * nsc + sc;
    h[p]  = a.ce[(size_t)p * nsc + sc];
  }
  const int a_ld = active ? a_idx : 0, r_ld = (active && r_dm >= 0) ? r_dm : 0;
  float2    y[NS][NP];
  uint32_t  w0[NS], w1[NS];
  {
    int prefix = a.prefix0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int  sy  = min(a.start_symbol + k, a.end_symbol - 1);
      const bool dm  = (a.dmrs_syms >> sy) & 1;
#pragma unroll
      for (int p = 0; p < NP; ++p)
        y[k][p] = gp[p][(size_t)sy * nsc];
      const uint32_t bo = (uint32_t)(prefix + (dm ? r_ld : a_ld)) * (uint32_t)MOD;
      w0[k]             = a.seq[bo >> 5];
      w1[k]             = (MOD == 6) ? a.seq[(bo >> 5) + 1] : 0u;
      if (a.start_symbol + k < a.end_symbol - 1) // uniform (scalar arithmetic)
        prefix += a.nprb * (dm ? a.per_dm : 12);
    }
  }
  // equalize_zf_1xn.h:120-158, the part that only depends on the estimate (as in demod_columns)
  float ch_mod_sq = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float t = h[p].x * h[p].x, u = h[p].y * h[p].y;
    ch_mod_sq     = ch_mod_sq + (t + u);
  }
  const float d_pinv  = 1.0f * ch_mod_sq;
  const float rcpd    = 1.0f / d_pinv;
  const float vv      = rcpd * (a.noise_var / 1.0f);
  const float nv      = (d_pinv > 0.f && d_pinv < INFINITY && vv > 0.f && vv < INFINITY) ? vv : INFINITY;
  const float rcp_chk = (nv > 0.f) ? 1.0f / nv : 0.0f;
  int         prefix  = a.prefix0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int  sy = a.start_symbol + k;
    const bool dm = (a.dmrs_syms >> min(sy, 13)) & 1;
    const int  r  = dm ? (a.per_dm ? r_dm : -1) : a_idx;
    float acc_re = 0.f, acc_im = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float2 c  = h[p];
      const float  aa = y[k][p].x * c.x, b = y[k][p].y * c.y, cc = y[k][p].y * c.x, d = y[k][p].x * c.y;
      acc_re          = acc_re + (aa + b);
      acc_im          = acc_im + (cc - d);
    }
    float z_re = 0.f, z_im = 0.f;
    if (nv < INFINITY) {
      z_re = acc_re * rcpd;
      z_im = acc_im * rcpd;
    }
    const bool     fast    = fabsf(z_re) < INFINITY && fabsf(z_im) < INFINITY && rcp_chk < INFINITY;
    const unsigned re      = (unsigned)(prefix + max(r, 0));
    int8_t*        q       = a.llr + (size_t)re * MOD;
    const bool     aligned = demod_aligned<MOD>(a.llr + (size_t)prefix * MOD); // uniform
    const uint32_t sh      = (re * (uint32_t)MOD) & 31u;
    const uint32_t bits    = (MOD == 6) ? (uint32_t)((((uint64_t)w1[k] << 32) | w0[k]) >> sh) : (w0[k] >> sh);
    const uint64_t w       = demod_symbol_packed<MOD>(z_re, z_im, nv, tab, bits); // (garbage where !fast: replaced below)
    const bool     has     = active && r >= 0 && sy < a.end_symbol;
    if (has) {
      if (fast && aligned) {
        demod_store<MOD>(w, q, true);
      } else { // (rare: the exact sequence and bytes; taking w for a fast lane here costs the walk two more spilled registers)
        int l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fast)
          demod_symbol<MOD, true>(z_re, z_im, nv, re, tab, l);
        else
          demod_symbol<MOD, false>(z_re, z_im, nv, re, tab, l);
        demod_store<MOD>(demod_descramble_pack<MOD>(l, bits), q, false);
      }
    }
    if (sy < a.end_symbol)
      prefix += a.nprb * (dm ? a.per_dm : 12);
  }
}

template <int MOD>
__device__ __forceinline__ void demod_columns(const demod_args& a, bool active, int sc, int a_idx, int r_dm, const float2* tab, float* evm_red, int tid)
{
#pragma clang fp contract(off)
#ifndef DEMOD_NO_DEEP
  if (MOD >= 2 && a.ce_nof_symbols == 1 && !a.evm_part && !a.nph && a.nports == 1) { // uniform
    demod_columns_deep<(MOD >= 2 ? MOD : 2), 1>(a, active, sc, a_idx, r_dm, tab);
    return;
  }
#endif
  const int   nsc = a.nsc, nports = a.nports;
  const float noise_var = a.noise_var;
  const bool  compact   = a.ce_nof_symbols == 1;
  const float2* gp[4];
  const float2* hp[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    gp[p] = a.grid + (size_t)((a.rxp >> (8 * p)) & 0xffu) * 14 * nsc + sc;
    hp[p] = a.ce + (size_t)p * a.ce_nof_symbols * nsc + sc;
  }
  float2 h[4], yn[4];
  float  ch_mod_sq = 0.f, rcpd = 0.f, nv = INFINITY, rcp_chk = 0.f;
  auto   channel = [&]() { // equalize_zf_1xn.h:120-158, the part that only depends on the estimate
    ch_mod_sq = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < nports) {
        const float t = h[p].x * h[p].x, u = h[p].y * h[p].y;
        ch_mod_sq     = ch_mod_sq + (t + u);
      }
    const float d_pinv = 1.0f * ch_mod_sq;
    rcpd               = 1.0f / d_pinv;
    const float v      = rcpd * (noise_var / 1.0f);
    nv                 = (d_pinv > 0.f && d_pinv < INFINITY && v > 0.f && v < INFINITY) ? v : INFINITY;
    rcp_chk            = (nv > 0.f) ? 1.0f / nv : 0.0f;
  };
#pragma unroll
  for (int p = 0; p < 4; ++p)
    h[p] = yn[p] = make_float2(0.f, 0.f);
  // Where symbol sy finds this thread's element in the codeword (rank r among the data elements of the symbol, -1: none).
  auto rank_in = [&](int sy) { return (((a.dmrs_syms >> sy) & 1) ? (a.per_dm ? r_dm : -1) : a_idx); };
  auto fetch   = [&](int sy, int prefix, uint64_t& two) { // samples of symbol sy and the 64-bit window of its descrambling chips
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < nports)
        yn[p] = gp[p][(size_t)sy * nsc];
    const int r = rank_in(sy);
    if (r >= 0) {
      const uint32_t bo = (uint32_t)(prefix + r) * (uint32_t)MOD;
      two               = (uint64_t)a.seq[bo >> 5] | ((uint64_t)a.seq[(bo >> 5) + 1] << 32);
    }
  };
  uint64_t two_n = 0;
  if (active) {
    if (compact) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < nports)
          h[p] = hp[p][0];
    }
    fetch(a.start_symbol, a.prefix0, two_n);
  }
  if (compact)
    channel();
  int prefix = a.prefix0; // data elements of the transmission before the current symbol
  for (int sy = a.start_symbol; sy < a.end_symbol; ++sy) {
    const bool is_dmrs = (a.dmrs_syms >> sy) & 1;
    const int  npp     = is_dmrs ? a.per_dm : 12;
    float2     y[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      y[p] = yn[p];
    const uint64_t two = two_n;
    if (active && sy + 1 < a.end_symbol)
      fetch(sy + 1, prefix + a.nprb * npp, two_n);
    const int  r   = rank_in(sy);
    const bool has = active && r >= 0;
    float      evm_acc = 0.f;
    if (has) {
      if (!compact) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p < nports)
            h[p] = hp[p][(size_t)sy * nsc];
        channel();
      }
      float acc_re = 0.f, acc_im = 0.f;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p < nports) {
          const float2 c = h[p];
          const float  aa = y[p].x * c.x, b = y[p].y * c.y, cc = y[p].y * c.x, d = y[p].x * c.y;
          acc_re         = acc_re + (aa + b);
          acc_im         = acc_im + (cc - d);
        }
      }
      float z_re = 0.f, z_im = 0.f;
      if (nv < INFINITY) {
        z_re = acc_re * rcpd;
        z_im = acc_im * rcpd;
      }
      // NaNs can only come from a non-finite symbol or an infinite reciprocal noise variance (0 * inf): rare, exact path.
      const bool     fast = fabsf(z_re) < INFINITY && fabsf(z_im) < INFINITY && rcp_chk < INFINITY;
      const unsigned re   = (unsigned)(prefix + r); // index of the element in the codeword
      int8_t*        q    = a.llr + (size_t)re * MOD;
      const bool     aligned = demod_aligned<MOD>(a.llr + (size_t)prefix * MOD); // uniform
      // descrambling chips: bit b of this element is sequence bit re * MOD + b (window requested one symbol ahead)
      uint32_t bits = (uint32_t)(two >> ((re * (uint32_t)MOD) & 31u));
      uint64_t w;
      if (MOD >= 2 && fast && !a.evm_part && !a.nph) { // the common case: quantise, descramble and pack in one go
        w = demod_symbol_packed<MOD>(z_re, z_im, nv, tab, bits);
      } else {
        int l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fast)
          demod_symbol<MOD, true>(z_re, z_im, nv, re, tab, l);
        else
          demod_symbol<MOD, false>(z_re, z_im, nv, re, tab, l);
        if (a.evm_part) { // evm_calculator_generic_impl.cpp:31-47 on the soft bits BEFORE descrambling: hard decision, modulation, error power
          uint32_t hb = 0;
#pragma unroll
          for (int b = 0; b < MOD; ++b)
            hb |= (uint32_t)(l[b] <= 0) << b;
          const float2 id = map_symbol(MOD, hb, re);
          const float  er = id.x - z_re, ei = id.y - z_im;
          evm_acc         = er * er + ei * ei;
        }
        if (demod_is_placeholder(a, re))
          bits = (bits & 1u) ? 3u : 0u; // y repeats the chip of bit 0, the x placeholders behind it are not scrambled
        w = demod_descramble_pack<MOD>(l, bits);
      }
      demod_store<MOD>(w, q, aligned);
    }
    if (a.evm_part && npp != 0) // uniform
      demod_evm_sum(a, sy, evm_acc, evm_red, tid);
    prefix += a.nprb * npp;
  }
}

// The descriptor as 30 dwords in scalar registers: its sub-dword fields read one by one become VECTOR byte / short loads with a wait
// each (there are no scalar sub-dword loads on gfx950) -- several dependent memory round trips at the head of every workgroup.
// Layout of miphy_pusch_demod_job (include/miphy.h; sizeof = 120 is checked by tests/test_cabi.py).
struct demod_job_words {
  uint32_t w[30];
  __device__ __forceinline__ int      mod() const { return (int)(w[2] & 0xffu); }
  __device__ __forceinline__ int      nof_rx_ports() const { return (int)((w[2] >> 8) & 0xffu); }
  __device__ __forceinline__ int      start_symbol() const { return (int)((w[2] >> 16) & 0xffu); }
  __device__ __forceinline__ int      nof_symbols() const { return (int)(w[2] >> 24); }
  __device__ __forceinline__ int      dmrs_type() const { return (int)(w[3] & 0xffu); }
  __device__ __forceinline__ unsigned cdm_groups() const { return (w[3] >> 8) & 0xffu; }
  __device__ __forceinline__ int      ce_nof_symbols() const { return (int)((w[3] >> 16) & 0xffu); }
  __device__ __forceinline__ bool     ce_compact() const { return (w[3] >> 24) != 0; }
  __device__ __forceinline__ uint32_t rx_ports() const { return w[4]; }
  __device__ __forceinline__ unsigned dmrs_symbols_mask() const { return w[5] & 0xffffu; }
  __device__ __forceinline__ int      grid_nof_prb() const { return (int)(w[5] >> 16); }
  __device__ __forceinline__ uint64_t rb_mask(int k) const { return (uint64_t)w[8 + 2 * k] | ((uint64_t)w[9 + 2 * k] << 32); }
  __device__ __forceinline__ int      nof_prb() const // allocated PRBs
  {
    const uint64_t m[5] = {rb_mask(0), rb_mask(1), rb_mask(2), rb_mask(3), rb_mask(4)};
    return (int)miphy_count_prb(m, (unsigned)grid_nof_prb());
  }
  __device__ __forceinline__ uint64_t grid_offset() const { return (uint64_t)w[18] | ((uint64_t)w[19] << 32); }
  __device__ __forceinline__ uint64_t ce_offset() const { return (uint64_t)w[20] | ((uint64_t)w[21] << 32); }
  __device__ __forceinline__ uint64_t scalars_offset() const { return (uint64_t)w[22] | ((uint64_t)w[23] << 32); }
  __device__ __forceinline__ uint64_t llr_offset() const { return (uint64_t)w[24] | ((uint64_t)w[25] << 32); }
  __device__ __forceinline__ uint32_t placeholders_offset() const { return w[26]; }
  __device__ __forceinline__ uint32_t nof_placeholders() const { return w[27]; }
  __device__ __forceinline__ uint64_t evm_offset() const { return (uint64_t)w[28] | ((uint64_t)w[29] << 32); }
};
static_assert(sizeof(miphy_pusch_demod_job) == 120 && offsetof(miphy_pusch_demod_job, rb_mask) == 32 && offsetof(miphy_pusch_demod_job, grid_offset) == 72 &&
                  offsetof(miphy_pusch_demod_job, placeholders_offset) == 104 && offsetof(miphy_pusch_demod_job, evm_offset) == 112 &&
                  offsetof(miphy_pusch_demod_job, rx_ports) == 16 && offsetof(miphy_pusch_demod_job, dmrs_symbols_mask) == 20,
              "demod_job_words follows the layout of miphy_pusch_demod_job");
__device__ __forceinline__ demod_job_words demod_load_job(const miphy_pusch_demod_job* __restrict__ jp)
{
  const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(jp);
  demod_job_words j;
#pragma unroll
  for (int i = 0; i < 30; ++i)
    j.w[i] = s[i];
  return j;
}

// Allocated PRBs of a job for the lanes of a workgroup: the compact list prb_of[rank] (LDS).
__device__ __forceinline__ void demod_prb_list(const demod_job_words& j, uint64_t* rbm, uint16_t* prb_of, int tid, int nt)
{
  const int nprb_grid = j.grid_nof_prb();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
      rbm[k] = j.rb_mask(k);
  }
  __syncthreads();
  for (int r = tid; r < nprb_grid; r += nt) {
    const int      wd = r >> 6, bt = r & 63;
    const uint64_t m  = rbm[wd];
    if ((m >> bt) & 1ull) {
      int idx = __popcll(m & ((1ull << bt) - 1ull));
      for (int w = 0; w < wd; ++w)
        idx += __popcll(rbm[w]);
      prb_of[idx] = (uint16_t)r;
    }
  }
  __syncthreads();
}

// Per-symbol EVM sums of a transmission from the per-chunk partials, chunks added in order (deterministic); symbols without data: 0.
// part: the transmission's [14][DEMOD_MAX_CHUNKS] partials.
__device__ __forceinline__ void evm_reduce_symbol(const miphy_pusch_demod_job* __restrict__ jp, const float* __restrict__ part, float* __restrict__ evm_sums, int sy)
{
  const int      nprb  = (int)miphy_count_prb(jp->rb_mask, jp->grid_nof_prb);
  const unsigned dmask = dmrs_prb_mask(jp->dmrs_type, jp->nof_cdm_groups_without_data);
  const int      npp   = ((jp->dmrs_symbols_mask >> sy) & 1) ? 12 - __popc(dmask) : 12;
  float          s     = 0.f;
  if (sy >= jp->start_symbol && sy < jp->start_symbol + jp->nof_symbols && npp != 0) {
    const int    nch = (nprb * 12 + DEMOD_THREADS - 1) / DEMOD_THREADS;
    const float* p   = part + (size_t)sy * DEMOD_MAX_CHUNKS;
    for (int c = 0; c < nch; ++c)
      s += p[c];
  }
  evm_sums[jp->evm_offset + sy] = s;
}

// ------------------------------------------------------------------------------------------------ one codeword on 1..4 transmit layers
// Beyond the 23.5 reference (pusch_demodulator_impl.h asserts one layer): L x P zero forcing (equalize_device.h) and the layer demapping of
// TS 38.211 6.3.1.3 -- element i of layer ly is codeword symbol L i + ly -- in front of the same soft demapper and descrambler.

// Data elements per layer of a job whose fields hold the rules below (popcounts: the kernels evaluate it once per workgroup).
__host__ __device__ __forceinline__ unsigned pusch_demod_count_re(const miphy_pusch_demod_job& j)
{
  const unsigned dm = (j.dmrs_type == 1 ? 6u : 4u) * j.nof_cdm_groups_without_data; // DM-RS elements per PRB (dmrs_prb_mask)
  const unsigned nprb = miphy_count_prb(j.rb_mask, j.grid_nof_prb);
  unsigned       nsym_dmrs = 0;
  for (unsigned s = j.start_symbol; s < (unsigned)j.start_symbol + j.nof_symbols; ++s)
    nsym_dmrs += (j.dmrs_symbols_mask >> s) & 1u;
  return nprb * (12u * (j.nof_symbols - nsym_dmrs) + (12u - dm) * nsym_dmrs);
}

// The two records of a job, miphy_pusch_demod_job and miphy_pusch_demod_layers_job: the base record and the layer count. A base record is on one layer.
__host__ __device__ __forceinline__ const miphy_pusch_demod_job& pusch_demod_base(const miphy_pusch_demod_job& job) { return job; }
__host__ __device__ __forceinline__ const miphy_pusch_demod_job& pusch_demod_base(const miphy_pusch_demod_layers_job& job) { return job.base; }
__host__ __device__ __forceinline__ unsigned pusch_demod_layers(const miphy_pusch_demod_job&) { return 1; }
__host__ __device__ __forceinline__ unsigned pusch_demod_layers(const miphy_pusch_demod_layers_job& job) { return job.nof_tx_layers; }
// (the MMSE record: a layered record and where its covariance matrices are)
__host__ __device__ __forceinline__ const miphy_pusch_demod_job& pusch_demod_base(const miphy_pusch_demod_mmse_job& job) { return job.base.base; }
__host__ __device__ __forceinline__ unsigned pusch_demod_layers(const miphy_pusch_demod_mmse_job& job) { return job.base.nof_tx_layers; }

// What a job (j = its base record, L = its layers) must satisfy, once, evaluated in this order: R(condition, message of the host, its arguments).
// The host refuses a job that breaks a rule with the rule's message; the kernels skip a device-resident layered job that does
// (pusch_demod_layers_job_ok), and take a device-resident base record as it is.
// have_ph: the call came with a placeholder list (never through miphy_pusch_demodulate_layers_batch); ex: the host's entry point is an _ex one.
#define PUSCH_DEMOD_LAYERS_RULES(R)                                                                                                                    \
  R(L >= 1 && L <= 4, "invalid number of transmit layers %u", L)                                                                                      \
  R(j.nof_rx_ports >= 1 && j.nof_rx_ports <= 4, "invalid number of receive ports")                                                                    \
  R(L <= j.nof_rx_ports, "%u transmit layers on %u receive ports", L, (unsigned)j.nof_rx_ports)                                                       \
  R(j.mod == 1 || j.mod == 2 || j.mod == 4 || j.mod == 6 || j.mod == 8, "invalid modulation order %u", (unsigned)j.mod)                               \
  R(j.nof_symbols >= 1 && j.start_symbol + j.nof_symbols <= 14, "invalid time allocation")                                                            \
  R(j.ce_compact || (j.ce_nof_symbols >= j.start_symbol + j.nof_symbols && j.ce_nof_symbols <= 14), "channel estimate too short")                     \
  R(j.dmrs_type == 1 || j.dmrs_type == 2, "invalid DM-RS type")                                                                                       \
  R(j.nof_cdm_groups_without_data >= 1 && j.nof_cdm_groups_without_data <= (j.dmrs_type == 1 ? 2 : 3), "invalid number of CDM groups without data")   \
  R(j.grid_nof_prb >= 1 && j.grid_nof_prb <= 275, "invalid grid width")                                                                               \
  R(j.n_id < 1024, "invalid scrambling identifier")                                                                                                   \
  R(j.rnti < 65536, "invalid RNTI")                                                                                                                   \
  R(j.nof_placeholders == 0 || (have_ph && j.mod >= 2), "%s",                                                                                         \
    ex ? "placeholders need the list and a modulation order of at least 2" : "UCI placeholders are not supported on this entry point")                \
  /* pusch_demodulator_impl.cpp:76-80: the codeword length must match the number of data REs */                                                       \
  R(j.nof_llr == pusch_demod_count_re(j) * L * j.mod, "%u LLRs requested, the allocation holds %u on %u layers", j.nof_llr,                           \
    pusch_demod_count_re(j) * L * j.mod, L)

__host__ __device__ __forceinline__ bool pusch_demod_layers_job_ok(const miphy_pusch_demod_layers_job& lj, bool have_ph)
{
  const miphy_pusch_demod_job& j = lj.base;
  const unsigned               L = lj.nof_tx_layers;
#define PUSCH_RULE_HOLDS(cond, ...) &&(cond)
  return true PUSCH_DEMOD_LAYERS_RULES(PUSCH_RULE_HOLDS);
#undef PUSCH_RULE_HOLDS
}
__device__ __forceinline__ bool pusch_demod_layers_job_ok(const miphy_pusch_demod_job&, bool) { return true; } // (a base record is not checked on the device)
__host__ __device__ __forceinline__ bool pusch_demod_layers_job_ok(const miphy_pusch_demod_mmse_job& mj, bool have_ph) { return pusch_demod_layers_job_ok(mj.base, have_ph); }

// Per-symbol EVM sums of every transmission; a job the demodulator skipped keeps its 14 floats.
template <typename JOB>
__global__ void __launch_bounds__(64) pusch_evm_reduce_kernel(const JOB* __restrict__ jobs, const float* __restrict__ evm_part, float* __restrict__ evm_sums, bool have_ph)
{
  if (threadIdx.x < 14 && pusch_demod_layers_job_ok(jobs[blockIdx.x], have_ph))
    evm_reduce_symbol(&pusch_demod_base(jobs[blockIdx.x]), evm_part + (size_t)blockIdx.x * 14 * DEMOD_MAX_CHUNKS, evm_sums, threadIdx.x);
}

// Scrambling sequence of every transmission: c(0 .. nof_llr - 1) from c_init = rnti * 2^15 + n_id. The OFDM symbols of a transmission use
// consecutive pieces of it, so no jump-ahead is needed; inside the demodulator the generation was a serial chain that held three of four
// wavefronts of every (transmission, symbol) workgroup at a barrier (0.13 of 0.37 ms per 1024 slots).
// A sequence of up to SEQ_STRIDE words (every one-layer transmission) fits the x1 table and one workgroup's LDS: workgroup (transmission, 0) makes it
// whole, x1 from the table, x2 by the doubling word recurrence (gold_device.h). A layered transmission has up to four times as much: a longer sequence
// is made in pieces of SEQ_PIECE words, workgroup (transmission, piece) jumping both shift registers to the piece's first bit (gold_piece).
// seq: [transmission][stride] words; a call with base records has stride = SEQ_STRIDE and one workgroup per transmission.
constexpr int SEQ_STRIDE = GOLD_X1_WORDS;
constexpr int SEQ_PIECE  = SEQ_STRIDE / 2;
#ifndef SCR_THREADS
#define SCR_THREADS 512
#endif
template <typename JOB>
__global__ void __launch_bounds__(SCR_THREADS) pusch_seq_kernel(const JOB* __restrict__ jobs, const gold_tables* __restrict__ gt, uint32_t* __restrict__ seq,
                                                                uint32_t stride, bool have_ph)
{
  __shared__ uint32_t w[SEQ_STRIDE]; // one sequence, or w1 | w2 of a piece
  if (!pusch_demod_layers_job_ok(jobs[blockIdx.x], have_ph)) // uniform
    return;
  const miphy_pusch_demod_job* __restrict__ jp = &pusch_demod_base(jobs[blockIdx.x]);
  const int      tid = threadIdx.x, nt = blockDim.x;
  const int      nwords = min((int)((jp->nof_llr + 31u) >> 5) + 2, (int)stride); // + the 64-bit window of the last resource element
  const uint32_t c_init = (jp->rnti << 15) + jp->n_id;
  uint32_t*      o      = seq + (size_t)blockIdx.x * stride;
  if (nwords <= SEQ_STRIDE) {
    if (blockIdx.y != 0)
      return;
    gold_x2_sequence(*gt, c_init, nwords, w, tid, nt);
    for (int i = tid; i < nwords; i += nt)
      o[i] = w[i] ^ gt->x1_seq[i];
    return;
  }
  const int first = (int)blockIdx.y * SEQ_PIECE;
  if (first >= nwords)
    return;
  gold_piece(*gt, c_init, first, min(SEQ_PIECE, nwords - first), w, w + SEQ_PIECE, o + first, tid, nt);
}

// MOD soft bits of one equalised symbol, descrambled with the low MOD bits of `bits`, to q: the packed demapper where no NaN can appear, the exact
// sequence otherwise; one wide store where q is aligned to it, bytes otherwise.
template <int MOD>
__device__ __forceinline__ void demod_emit(float re, float im, float nvar, unsigned sym_idx, uint32_t bits, const float2* tab, int8_t* q)
{
#pragma clang fp contract(off)
  const float rcp_chk = (nvar > 0.f) ? 1.0f / nvar : 0.0f;
  const bool  fast    = fabsf(re) < INFINITY && fabsf(im) < INFINITY && rcp_chk < INFINITY;
  uint64_t    w       = 0;
  bool        packed  = false;
  if constexpr (MOD >= 2) {
    if (fast) {
      w      = demod_symbol_packed<MOD>(re, im, nvar, tab, bits);
      packed = true;
    }
  }
  if (!packed) {
    int l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (fast)
      demod_symbol<MOD, true>(re, im, nvar, sym_idx, tab, l);
    else
      demod_symbol<MOD, false>(re, im, nvar, sym_idx, tab, l);
    w = demod_descramble_pack<MOD>(l, bits);
  }
  demod_store<MOD>(w, q, demod_aligned<MOD>(q));
}

// The variant of demod_emit behind UCI placeholders and the EVM: always the exact sequence, whose soft bits l[] the EVM needs before they are
// descrambled (as demod_columns does for such jobs; the bytes are those of demod_emit). placeholder: the symbol holds [c0 y x ..], bit 1 takes the
// chip of bit 0 and the bits behind it none. Returns |hard-decided symbol - equalised symbol|^2 (evm_calculator_generic_impl.cpp:31-47).
template <int MOD>
__device__ __forceinline__ float demod_emit_exact(float re, float im, float nvar, unsigned sym_idx, uint32_t bits, bool placeholder, const float2* tab, int8_t* q)
{
#pragma clang fp contract(off)
  const float rcp_chk = (nvar > 0.f) ? 1.0f / nvar : 0.0f;
  const bool  fast    = fabsf(re) < INFINITY && fabsf(im) < INFINITY && rcp_chk < INFINITY;
  int         l[8]    = {0, 0, 0, 0, 0, 0, 0, 0};
  if (fast)
    demod_symbol<MOD, true>(re, im, nvar, sym_idx, tab, l);
  else
    demod_symbol<MOD, false>(re, im, nvar, sym_idx, tab, l);
  uint32_t hb = 0;
#pragma unroll
  for (int b = 0; b < MOD; ++b)
    hb |= (uint32_t)(l[b] <= 0) << b;
  const float2 id = map_symbol(MOD, hb, sym_idx);
  const float  er = id.x - re, ei = id.y - im;
  if (placeholder)
    bits = (bits & 1u) ? 3u : 0u;
  demod_store<MOD>(demod_descramble_pack<MOD>(l, bits), q, demod_aligned<MOD>(q));
  return er * er + ei * ei;
}

// One thread = one allocated subcarrier walked over the OFDM symbols, as demod_columns: with the compact estimate zf_prepare runs once and its result
// stays in registers, per element only the samples are loaded and zf_apply runs. The L symbols of an element are L consecutive symbols of the
// codeword: L MOD consecutive bytes, descrambled with L MOD (<= 32) consecutive chips.
// EX: for a batch with placeholders or EVM. The list is searched once per element: a listed element carries the pattern in each of its L codeword
// symbols. EVM: the terms of an element's layers are added in layer order, then demod_evm_sum and (pusch_evm_reduce_kernel) the chunks in order, as
// demod_columns does, so a symbol's sum has one value. Every thread of the workgroup reaches the barriers of the sum; without EX a lane that owns
// no subcarrier leaves at once.
// MMSE: mmse_prepare / mmse_apply (mmse_device.h) in place of zf_prepare / zf_apply. cm: the covariance matrix of this thread's PRG, [P][P]; a subcarrier
// stays in its PRG, so the matrix is loaded and factored once, in front of the walk. a.noise_var is not used.
template <int MOD, int L, bool EX, bool MMSE = false>
__device__ __forceinline__ void demod_layers_columns(const demod_args& a, bool active, int sc, int a_idx, int r_dm, const float2* tab, float* evm_red, int tid,
                                                     const float2* cm = nullptr)
{
#pragma clang fp contract(off)
  const int  nsc = a.nsc, np = a.nports;
  const bool compact = a.ce_nof_symbols == 1;
  float2     h[L][4];
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int p = 0; p < 4; ++p)
      h[l][p] = make_float2(0.f, 0.f);
  auto load_h = [&](int row) { // estimate [layer][rx port][ce_nof_symbols][nsc]
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < np)
          h[l][p] = a.ce[((size_t)(l * np + p) * a.ce_nof_symbols + row) * nsc + sc];
  };
  std::conditional_t<MMSE, mmse_prepared<L>, zf_prepared<L>> q;
  mmse_factored                                              f; // (MMSE only)
  if (!EX && !active)
    return;
  if constexpr (MMSE) {
    if (active) {
      float2 c[4][4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k <= p; ++k)
          c[p][k] = (p < np) ? cm[p * np + k] : make_float2(0.f, 0.f);
      mmse_factor(c, np, f);
    }
  }
  if (active && compact) {
    load_h(0);
    if constexpr (MMSE)
      mmse_prepare<L>(h, np, f, 1.0f, q);
    else
      zf_prepare<L>(h, np, a.noise_var, 1.0f, q);
  }
  int prefix = a.prefix0; // data elements per layer of the transmission before the current symbol
  for (int sy = a.start_symbol; sy < a.end_symbol; ++sy) { // (uniform)
    const bool is_dmrs = (a.dmrs_syms >> sy) & 1;
    const int  npp     = is_dmrs ? a.per_dm : 12;
    const int  r       = is_dmrs ? (a.per_dm ? r_dm : -1) : a_idx;
    float      evm_acc = 0.f;
    if (active && r >= 0) {
      float2 y[4], x[L];
#pragma unroll
      for (int p = 0; p < 4; ++p)
        y[p] = (p < np) ? a.grid[((size_t)((a.rxp >> (8 * p)) & 0xffu) * 14 + sy) * nsc + sc] : make_float2(0.f, 0.f);
      if (!compact) {
        load_h(sy);
        if constexpr (MMSE)
          mmse_prepare<L>(h, np, f, 1.0f, q);
        else
          zf_prepare<L>(h, np, a.noise_var, 1.0f, q);
      }
      if constexpr (MMSE)
        mmse_apply<L>(np, f, y, q, x);
      else
        zf_apply<L>(h, np, y, q, x);
      const unsigned el   = (unsigned)(prefix + r);  // the element's index in the codeword, what the placeholder list holds
      const uint32_t e0   = el * (uint32_t)L;        // first of the element's L codeword symbols
      const uint32_t bo   = e0 * (uint32_t)MOD;
      const uint64_t two  = (uint64_t)a.seq[bo >> 5] | ((uint64_t)a.seq[(bo >> 5) + 1] << 32);
      const uint32_t bits = (uint32_t)(two >> (bo & 31u));
      int8_t*        q0   = a.llr + (size_t)bo;
      if constexpr (EX) {
        const bool found = demod_is_placeholder(a, el);
#pragma unroll
        for (int l = 0; l < L; ++l) {
          const float t = demod_emit_exact<MOD>(x[l].x, x[l].y, q.nvar[l], e0 + l, bits >> (l * MOD), found, tab, q0 + l * MOD);
          evm_acc       = l ? evm_acc + t : t;
        }
      } else {
#pragma unroll
        for (int l = 0; l < L; ++l)
          demod_emit<MOD>(x[l].x, x[l].y, q.nvar[l], e0 + l, bits >> (l * MOD), tab, q0 + l * MOD);
      }
    }
    if constexpr (EX) {
      if (a.evm_part && npp != 0) // uniform
        demod_evm_sum(a, sy, evm_acc, evm_red, tid);
    }
    prefix += a.nprb * npp;
  }
}

// ONE_LAYER: the one-layer walk (demod_columns), which follows the reference operation for operation; otherwise L = 2..4. EX: with placeholders and EVM.
// MMSE: every layer count, one included, goes through demod_layers_columns with the thread's covariance matrix cm.
template <int MOD, bool ONE_LAYER, bool EX, bool MMSE = false>
__device__ __forceinline__ void demod_dispatch(int L, const demod_args& a, bool active, int sc, int a_idx, int r_dm, const float2* tab, float* evm_red, int tid,
                                               const float2* cm = nullptr)
{
  if constexpr (MMSE) {
    switch (L) { // uniform
      case 1:
        demod_layers_columns<MOD, 1, EX, true>(a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
        break;
      case 2:
        demod_layers_columns<MOD, 2, EX, true>(a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
        break;
      case 3:
        demod_layers_columns<MOD, 3, EX, true>(a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
        break;
      default:
        demod_layers_columns<MOD, 4, EX, true>(a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
        break;
    }
    return;
  }
  if constexpr (ONE_LAYER) {
    demod_columns<MOD>(a, active, sc, a_idx, r_dm, tab, evm_red, tid);
    return;
  }
  switch (L) { // uniform
    case 2:
      demod_layers_columns<MOD, 2, EX>(a, active, sc, a_idx, r_dm, tab, evm_red, tid);
      break;
    case 3:
      demod_layers_columns<MOD, 3, EX>(a, active, sc, a_idx, r_dm, tab, evm_red, tid);
      break;
    default:
      demod_layers_columns<MOD, 4, EX>(a, active, sc, a_idx, r_dm, tab, evm_red, tid);
      break;
  }
}

// grid (transmissions, chunks of 256 allocated subcarriers, parts of the OFDM symbols): a batch that fills the chip walks all symbols of a
// chunk in one workgroup (the channel row is set up once); a small one (a single slot: 13 chunks) is cut along the symbols as well, which
// shortens the dependent walk of every thread. seq: [transmission][stride] words. evm_part: [transmission][14][DEMOD_MAX_CHUNKS].
// JOB: miphy_pusch_demod_job or miphy_pusch_demod_layers_job. The jobs of a batch go to up to two instances: ONE_LAYER takes those on one layer
// (every base record), the other those on two to four layers (four 4 x 4 matrices in registers: a lower occupancy); a workgroup leaves at once when
// the job belongs to the other instance.
// EX: the instances of a call with a placeholder list or EVM sums, which take the exact demapper; the others never see `placeholders` and `evm_part`,
// so the throughput path keeps its registers.
#ifndef DEMOD_MIN_WAVES
#define DEMOD_MIN_WAVES 6 // 80 registers (four of them spilled outside the walk): 0.207 against 0.214 ms per 1024 slots at five
#endif
// The body of both kernels below. A miphy_pusch_demod_mmse_job batch has one instance for every layer count (ONE_LAYER = false), which takes the
// covariance matrices `cov` and never reads `scalars`.
template <typename JOB, bool ONE_LAYER, bool EX>
__device__ __forceinline__ void pusch_demod_body(const JOB* __restrict__ jobs, const float2* __restrict__ grid, const float2* __restrict__ ce,
                                                 const float* __restrict__ scalars, int8_t* __restrict__ llr, const uint32_t* __restrict__ seq, uint32_t stride,
                                                 const uint16_t* __restrict__ placeholders, float* __restrict__ evm_part, const float2* __restrict__ cov)
{
  constexpr bool MMSE = std::is_same<JOB, miphy_pusch_demod_mmse_job>::value;
  static_assert(!MMSE || !ONE_LAYER, "the MMSE walk is the layered one");
  __shared__ uint16_t prb_of[276];
  __shared__ float2   tab[64];
  __shared__ uint64_t rbm[5];
  __shared__ float    evm_red[4];
  const int L = (int)pusch_demod_layers(jobs[blockIdx.x]);
  if (!MMSE && (L == 1) != ONE_LAYER) // uniform
    return;
  if (!pusch_demod_layers_job_ok(jobs[blockIdx.x], EX && placeholders)) // uniform: a device-resident job the host has not seen is skipped
    return;
  const demod_job_words j    = demod_load_job(&pusch_demod_base(jobs[blockIdx.x]));
  const int             tid  = threadIdx.x;
  const int             nprb = j.nof_prb(); // scalar popcounts of the descriptor words
  // A chunk behind the allocation leaves before it has requested or built anything (the grid is sized for the widest allocation of the
  // batch: in a slot shared by eight UEs most workgroups of the narrow ones are such chunks).
  if ((int)blockIdx.y * DEMOD_THREADS >= nprb * 12)
    return; // uniform
  const demod_tab_entry te        = demod_table_entry(j.mod(), tid);            // requested now, stored behind the PRB list
  float                 noise_var = 0.f;
  if constexpr (!MMSE)
    noise_var = scalars[j.scalars_offset() + 2]; // likewise
  demod_prb_list(j, rbm, prb_of, tid, DEMOD_THREADS);
  demod_table_store(tab, te); // (made visible by the barrier in front of the walk)
  const unsigned dmask = dmrs_prb_mask(j.dmrs_type(), j.cdm_groups());
  demod_args     a;
  a.per_dm         = 12 - __popc(dmask);
  a.dmrs_syms      = j.dmrs_symbols_mask();
  a.start_symbol   = j.start_symbol();
  a.end_symbol     = a.start_symbol + j.nof_symbols();
  a.nprb           = nprb;
  a.prefix0        = 0;
  if (gridDim.z > 1) { // uniform
    const int per = (a.end_symbol - a.start_symbol + (int)gridDim.z - 1) / (int)gridDim.z;
    const int f = a.start_symbol + (int)blockIdx.z * per, l = min(a.end_symbol, f + per);
    if (f >= l)
      return;
    for (int sy = a.start_symbol; sy < f; ++sy)
      a.prefix0 += nprb * (((a.dmrs_syms >> sy) & 1u) ? a.per_dm : 12);
    a.start_symbol = f;
    a.end_symbol   = l;
  }
  a.nsc            = j.grid_nof_prb() * 12;
  a.nports         = j.nof_rx_ports();
  a.ce_nof_symbols = j.ce_compact() ? 1 : j.ce_nof_symbols(); // compact estimate: one row per port, valid for every symbol
  a.rxp            = j.rx_ports();
  a.grid           = grid + j.grid_offset();
  a.ce             = ce + j.ce_offset();
  a.llr            = llr + j.llr_offset();
  a.noise_var      = noise_var;
  a.nph            = 0;
  a.ph             = nullptr;
  a.evm_part       = nullptr;
  if constexpr (EX) {
    a.nph      = placeholders ? (int)j.nof_placeholders() : 0;
    a.ph       = placeholders ? placeholders + j.placeholders_offset() : nullptr;
    a.evm_part = evm_part ? evm_part + (size_t)blockIdx.x * 14 * DEMOD_MAX_CHUNKS : nullptr;
  }
  a.seq            = seq + (size_t)blockIdx.x * stride;
  // this thread's subcarrier
  const int  a_idx  = (int)blockIdx.y * DEMOD_THREADS + tid;
  const bool active = a_idx < nprb * 12;
  const int  pr     = a_idx / 12, k = a_idx - 12 * pr;
  const int  sc     = active ? (int)prb_of[pr] * 12 + k : 0;
  const int  r_dm   = ((dmask >> k) & 1u) ? -1 : pr * a.per_dm + __popc(~dmask & ((1u << k) - 1u));
  const float2* cm = nullptr; // MMSE: the matrix of this thread's PRG = rank of its PRB among the allocated ones / prg_size
  if constexpr (MMSE) {
    const unsigned prg_size = jobs[blockIdx.x].prg_size;
    cm = cov + jobs[blockIdx.x].cov_offset + (size_t)((active && prg_size) ? (unsigned)pr / prg_size : 0u) * (unsigned)(a.nports * a.nports);
  }
  __syncthreads(); // interval tables in LDS
  switch (j.mod()) {
    case 8:
      demod_dispatch<8, ONE_LAYER, EX, MMSE>(L, a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
      break;
    case 6:
      demod_dispatch<6, ONE_LAYER, EX, MMSE>(L, a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
      break;
    case 4:
      demod_dispatch<4, ONE_LAYER, EX, MMSE>(L, a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
      break;
    case 2:
      demod_dispatch<2, ONE_LAYER, EX, MMSE>(L, a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
      break;
    default:
      demod_dispatch<1, ONE_LAYER, EX, MMSE>(L, a, active, sc, a_idx, r_dm, tab, evm_red, tid, cm);
      break;
  }
}

template <typename JOB, bool ONE_LAYER, bool EX>
__global__ void __launch_bounds__(DEMOD_THREADS, ONE_LAYER ? DEMOD_MIN_WAVES : 1) pusch_demod_kernel(const JOB* __restrict__ jobs, const float2* __restrict__ grid,
                                                                                     const float2* __restrict__ ce, const float* __restrict__ scalars,
                                                                                     int8_t* __restrict__ llr, const uint32_t* __restrict__ seq, uint32_t stride,
                                                                                     const uint16_t* __restrict__ placeholders, float* __restrict__ evm_part)
{
  pusch_demod_body<JOB, ONE_LAYER, EX>(jobs, grid, ce, scalars, llr, seq, stride, placeholders, evm_part, nullptr);
}

template <bool EX>
__global__ void __launch_bounds__(DEMOD_THREADS, 1) pusch_demod_mmse_kernel(const miphy_pusch_demod_mmse_job* __restrict__ jobs, const float2* __restrict__ grid,
                                                                            const float2* __restrict__ ce, const float2* __restrict__ cov, int8_t* __restrict__ llr,
                                                                            const uint32_t* __restrict__ seq, uint32_t stride,
                                                                            const uint16_t* __restrict__ placeholders, float* __restrict__ evm_part)
{
  pusch_demod_body<miphy_pusch_demod_mmse_job, false, EX>(jobs, grid, ce, nullptr, llr, seq, stride, placeholders, evm_part, cov);
}

// All four entry points: `who` names the entry in the messages, ex: it is an _ex one (only the message of the placeholder rule depends on it). The EX
// instances run when the call has EVM sums or a job with placeholders; device-resident jobs cannot be looked at, there the two pointers decide.
template <typename JOB>
int pusch_demodulate(const char* who, miphy_ctx* ctx, const JOB* jobs, int jobs_on_device, uint32_t n, const float* grid, const float* ce, const float* scalars,
                     const float* cov, int8_t* llr, const uint16_t* placeholders, float* evm_sums, bool ex, void* stream)
{
  constexpr bool mmse    = std::is_same<JOB, miphy_pusch_demod_mmse_job>::value; // scalars: not read, may be null; cov: the matrices
  constexpr bool layered = mmse || std::is_same<JOB, miphy_pusch_demod_layers_job>::value;
  MIPHY_REQUIRE(ctx && jobs && grid && ce && (mmse ? cov != nullptr : scalars != nullptr) && llr, "miphy_%s_batch: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "%s: batch too large (max 65535 transmissions per call)", who);
  // device-resident jobs: the widest grid, layered records on four layers and in both instances
  uint32_t   max_chunks = DEMOD_MAX_CHUNKS, max_layers = layered ? 4 : 1, max_words = max_layers * SEQ_STRIDE;
  bool       one_layer = true, more_layers = layered;
  const bool have_ph = placeholders != nullptr;
  bool       extras  = have_ph || evm_sums;
  if (!jobs_on_device) {
    uint32_t max_prb = 1, max_llr = 0;
    max_layers = 1, one_layer = more_layers = false;
    extras     = evm_sums != nullptr;
    for (uint32_t i = 0; i < n; ++i) {
      const miphy_pusch_demod_job& j = pusch_demod_base(jobs[i]);
      const unsigned               L = pusch_demod_layers(jobs[i]);
#define PUSCH_RULE_REQUIRE(cond, msg, ...) MIPHY_REQUIRE(cond, "%s: job %u: " msg, who, i, ##__VA_ARGS__);
      PUSCH_DEMOD_LAYERS_RULES(PUSCH_RULE_REQUIRE)
#undef PUSCH_RULE_REQUIRE
      max_prb    = std::max(max_prb, miphy_count_prb(j.rb_mask, j.grid_nof_prb));
      max_layers = std::max(max_layers, L);
      one_layer |= L == 1, more_layers |= L > 1;
      max_llr    = std::max(max_llr, j.nof_llr);
      extras |= j.nof_placeholders != 0;
    }
    max_chunks = (max_prb * 12 + DEMOD_THREADS - 1) / DEMOD_THREADS;
    max_words  = ((max_llr + 31u) >> 5) + 2;
  }
  hipStream_t        s  = (hipStream_t)stream;
  const gold_tables* gt = nullptr;
  int                rc = miphy_get_gold_tables(ctx, &gt);
  if (rc)
    return rc;
  const void* d_jobs = nullptr;
  rc                 = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(JOB) * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  const uint32_t stride = max_layers * (uint32_t)SEQ_STRIDE;
  void*          work   = nullptr;
  const size_t   seq_bytes = (size_t)n * stride * sizeof(uint32_t);
  const size_t   evm_bytes = evm_sums ? (size_t)n * 14 * DEMOD_MAX_CHUNKS * sizeof(float) : 0; // per-(symbol, chunk) partials behind the sequences
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_SEQUENCES, seq_bytes + evm_bytes, &work)))
    return rc;
  uint32_t*   seq      = static_cast<uint32_t*>(work);
  float*      evm_part = evm_sums ? reinterpret_cast<float*>(static_cast<uint8_t*>(work) + seq_bytes) : nullptr;
  const auto* dj       = (const JOB*)d_jobs;
  hipLaunchKernelGGL(pusch_seq_kernel<JOB>, dim3(n, max_words <= (uint32_t)SEQ_STRIDE ? 1u : (max_words + SEQ_PIECE - 1) / SEQ_PIECE), dim3(SCR_THREADS), 0, s, dj, gt,
                     seq, stride, have_ph);
  const uint32_t sym_parts = std::max(1u, std::min(4u, (uint32_t)ctx->num_cus / (n * max_chunks)));
  const dim3 blocks(n, max_chunks, sym_parts);
  if constexpr (mmse) { // one instance for every layer count
    hipLaunchKernelGGL(extras ? pusch_demod_mmse_kernel<true> : pusch_demod_mmse_kernel<false>, blocks, dim3(DEMOD_THREADS), 0, s, dj, (const float2*)grid,
                       (const float2*)ce, (const float2*)cov, llr, (const uint32_t*)seq, stride, placeholders, evm_part);
  } else {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, blocks, dim3(DEMOD_THREADS), 0, s, dj, (const float2*)grid, (const float2*)ce, scalars, llr, (const uint32_t*)seq, stride,
                         placeholders, evm_part);
    };
    if (one_layer)
      launch(extras ? pusch_demod_kernel<JOB, true, true> : pusch_demod_kernel<JOB, true, false>);
    if constexpr (layered) {
      if (more_layers)
        launch(extras ? pusch_demod_kernel<JOB, false, true> : pusch_demod_kernel<JOB, false, false>);
    }
  }
  if (evm_sums)
    hipLaunchKernelGGL(pusch_evm_reduce_kernel<JOB>, dim3(n), dim3(64), 0, s, dj, (const float*)evm_part, evm_sums, have_ph);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ------------------------------------------------------------------------------------------------ transform precoding (DFT-s-OFDM, TS 38.211 6.3.1.4)
// Beyond the 23.5 reference: one workgroup per (transmission, data OFDM symbol) equalises the symbol's M = 12 N_PRB elements into LDS (zf_prepare / zf_apply
// on one layer: the arithmetic of the stand-alone equaliser), de-precodes them there (tp_device.h: the function of the stand-alone de-precoder) and
// runs the soft demapper and descrambler above on y[n] with the symbol's one noise variance. Every data symbol has M elements (no data on a DM-RS symbol), so
// the r-th data symbol owns the codeword elements r M ... r M + M - 1.

// What a transform-precoded job must satisfy beyond PUSCH_DEMOD_LAYERS_RULES on one layer (contiguous, nprb: what tp_contiguous found).
#define PUSCH_DEMOD_TP_RULES(R)                                                                                                             \
  R(j.dmrs_type == 1, "transform precoding needs DM-RS type 1")                                                                             \
  R(j.nof_cdm_groups_without_data == 2, "transform precoding needs two CDM groups without data (no data on a DM-RS symbol)")                \
  R(contiguous, "transform precoding needs a contiguous allocation")                                                                        \
  R(tp_nprb_ok(nprb), "transform precoding needs 2^a*3^b*5^c <= 270 PRBs, the allocation holds %u", nprb)

__device__ __forceinline__ bool pusch_demod_tp_job_ok(const miphy_pusch_demod_job& j, bool have_ph, unsigned& first, unsigned& nprb)
{
  const unsigned L = 1;
#define PUSCH_RULE_HOLDS(cond, ...) &&(cond)
  if (!(true PUSCH_DEMOD_LAYERS_RULES(PUSCH_RULE_HOLDS)))
    return false;
  const bool contiguous = tp_contiguous(j.rb_mask, j.grid_nof_prb, first, nprb);
  return true PUSCH_DEMOD_TP_RULES(PUSCH_RULE_HOLDS);
#undef PUSCH_RULE_HOLDS
}

// The M de-precoded symbols of a data symbol (x: tp_deprecode_symbol ran) to soft bits: lane t takes n = t, t + TP_THREADS, ... e0: the symbol's first
// codeword element. EX: placeholders and the EVM term of every symbol, added per lane in ascending n, then over the wavefront by the xor tree, then
// the four wavefronts in sequence.
template <int MOD, bool EX>
__device__ __forceinline__ void demod_tp_symbols(const demod_args& a, const cplx* x, int M, float scale, float v, unsigned e0, const float2* tab, float* evm_out,
                                                 float* red, int tid)
{
  float evm_acc = 0.f;
  for (int n = tid; n < M; n += TP_THREADS) {
    const float2   y   = tp_symbol(x, n, scale);
    const unsigned re  = e0 + (unsigned)n;
    const uint32_t bo  = re * (uint32_t)MOD;
    const uint64_t two = (uint64_t)a.seq[bo >> 5] | ((uint64_t)a.seq[(bo >> 5) + 1] << 32);
    const uint32_t bits = (uint32_t)(two >> (bo & 31u));
    int8_t*        q    = a.llr + (size_t)bo;
    if constexpr (EX) {
      const float t = demod_emit_exact<MOD>(y.x, y.y, v, re, bits, a.nph && demod_is_placeholder(a, re), tab, q);
      evm_acc       = evm_acc + t;
    } else {
      demod_emit<MOD>(y.x, y.y, v, re, bits, tab, q);
    }
  }
  if constexpr (EX) {
    if (evm_out) { // uniform
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        evm_acc += __shfl_xor(evm_acc, off);
      if ((tid & 63) == 0)
        red[tid >> 6] = evm_acc;
      __syncthreads();
      if (tid == 0)
        *evm_out = ((red[0] + red[1]) + red[2]) + red[3];
    }
  }
}

// grid (transmissions, 14 OFDM symbols); dynamic LDS: the padded buffer of the widest allocation of the batch.
template <bool EX>
__global__ void __launch_bounds__(TP_THREADS) pusch_demod_tp_kernel(const miphy_pusch_demod_job* __restrict__ jobs, const float2* __restrict__ grid,
                                                                    const float2* __restrict__ ce, const float* __restrict__ scalars, int8_t* __restrict__ llr,
                                                                    const uint32_t* __restrict__ seq, uint32_t stride, const float* const* __restrict__ tws,
                                                                    const uint16_t* __restrict__ placeholders, float* __restrict__ evm_sums)
{
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
  __shared__ float2 tab[64];
  __shared__ float  red[8];
  cplx*             x = reinterpret_cast<cplx*>(tp_smem);
  unsigned          first = 0, nprb = 0;
  if (!pusch_demod_tp_job_ok(jobs[blockIdx.x], EX && placeholders, first, nprb)) // uniform: a device-resident job the host has not seen is skipped
    return;
  const demod_job_words j   = demod_load_job(jobs + blockIdx.x);
  const int             tid = threadIdx.x, sy = blockIdx.y;
  const int             start = j.start_symbol(), end = start + j.nof_symbols();
  const unsigned        dm    = j.dmrs_symbols_mask();
  float*                evm_out = nullptr;
  if constexpr (EX)
    evm_out = evm_sums ? evm_sums + j.evm_offset() + sy : nullptr;
  if (sy < start || sy >= end || ((dm >> sy) & 1u)) { // no data on this symbol
    if (evm_out && tid == 0)
      *evm_out = 0.f;
    return;
  }
  const int             M  = 12 * (int)nprb;
  const unsigned        r  = (unsigned)__popc(~dm & ((1u << sy) - 1u) & ~((1u << start) - 1u)); // data symbols in front of this one
  const demod_tab_entry te = demod_table_entry(j.mod(), tid);
  const float           noise_var = scalars[j.scalars_offset() + 2];
  const int             nsc = j.grid_nof_prb() * 12, np = j.nof_rx_ports();
  const int             rows = j.ce_compact() ? 1 : j.ce_nof_symbols(), row = j.ce_compact() ? 0 : sy;
  const float2*         g  = grid + j.grid_offset();
  const float2*         hc = ce + j.ce_offset();
  const uint32_t        rxp = j.rx_ports();
  tp_var_acc            acc;
  // four elements of a lane at a time: their samples and coefficients are requested together (unconditionally: a lane behind the end repeats the last
  // element and drops what it computes), then equalised in ascending order
  constexpr int B = 4;
#pragma unroll 1
  for (int k0 = tid; k0 < M; k0 += B * TP_THREADS) {
    float2 h[B][1][4], y[B][4];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int sc = (int)first * 12 + min(k0 + b * TP_THREADS, M - 1);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        h[b][0][p] = (p < np) ? hc[((size_t)p * rows + row) * nsc + sc] : make_float2(0.f, 0.f);
        y[b][p]    = (p < np) ? g[((size_t)((rxp >> (8 * p)) & 0xffu) * 14 + sy) * nsc + sc] : make_float2(0.f, 0.f);
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int k = k0 + b * TP_THREADS;
      if (k < M) {
        float2         xo[1];
        zf_prepared<1> q;
        zf_prepare<1>(h[b], np, noise_var, 1.0f, q);
        zf_apply<1>(h[b], np, y[b], q, xo);
        tp_put(x, k, xo[0], q.nvar[0], acc);
      }
    }
  }
  demod_table_store(tab, te); // (made visible by the barriers of the transform)
  const float v     = tp_deprecode_symbol(x, M, reinterpret_cast<const cplx*>(tws[nprb]), acc, red, tid);
  const float scale = tp_scale(M);
  demod_args  a;
  a.llr = llr + j.llr_offset();
  a.seq = seq + (size_t)blockIdx.x * stride;
  a.nph = 0, a.ph = nullptr;
  if constexpr (EX) {
    a.nph = placeholders ? (int)j.nof_placeholders() : 0;
    a.ph  = placeholders ? placeholders + j.placeholders_offset() : nullptr;
  }
  const unsigned e0 = r * (unsigned)M;
  switch (j.mod()) {
    case 8:
      demod_tp_symbols<8, EX>(a, x, M, scale, v, e0, tab, evm_out, red, tid);
      break;
    case 6:
      demod_tp_symbols<6, EX>(a, x, M, scale, v, e0, tab, evm_out, red, tid);
      break;
    case 4:
      demod_tp_symbols<4, EX>(a, x, M, scale, v, e0, tab, evm_out, red, tid);
      break;
    case 2:
      demod_tp_symbols<2, EX>(a, x, M, scale, v, e0, tab, evm_out, red, tid);
      break;
    default:
      demod_tp_symbols<1, EX>(a, x, M, scale, v, e0, tab, evm_out, red, tid);
      break;
  }
}

int pusch_demodulate_tp(const char* who, miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid, const float* ce,
                        const float* scalars, int8_t* llr, const uint16_t* placeholders, float* evm_sums, bool ex, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && grid && ce && scalars && llr, "miphy_%s_batch: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= 65535, "%s: batch too large (max 65535 transmissions per call)", who);
  uint32_t   max_nprb = TP_MAX_PRB; // device-resident jobs: the widest allocation
  const bool have_ph  = placeholders != nullptr;
  bool       extras   = have_ph || evm_sums;
  if (!jobs_on_device) {
    max_nprb = 1;
    extras   = evm_sums != nullptr;
    for (uint32_t i = 0; i < n; ++i) {
      const miphy_pusch_demod_job& j = jobs[i];
      const unsigned               L = 1;
#define PUSCH_RULE_REQUIRE(cond, msg, ...) MIPHY_REQUIRE(cond, "%s: job %u: " msg, who, i, ##__VA_ARGS__);
      PUSCH_DEMOD_LAYERS_RULES(PUSCH_RULE_REQUIRE)
      unsigned   first, nprb;
      const bool contiguous = tp_contiguous(j.rb_mask, j.grid_nof_prb, first, nprb);
      PUSCH_DEMOD_TP_RULES(PUSCH_RULE_REQUIRE)
#undef PUSCH_RULE_REQUIRE
      max_nprb = std::max(max_nprb, nprb);
      extras |= j.nof_placeholders != 0;
    }
  }
  hipStream_t         s   = (hipStream_t)stream;
  const gold_tables*  gt  = nullptr;
  const float* const* tws = nullptr;
  int                 rc;
  if ((rc = miphy_get_gold_tables(ctx, &gt)) || (rc = miphy_tp_twiddles(ctx, &tws)))
    return rc;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_demod_job) * (size_t)n, s, &d_jobs)))
    return rc;
  const uint32_t stride = (uint32_t)SEQ_STRIDE;
  void*          work   = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_SEQUENCES, (size_t)n * stride * sizeof(uint32_t), &work)))
    return rc;
  uint32_t*   seq = static_cast<uint32_t*>(work);
  const auto* dj  = (const miphy_pusch_demod_job*)d_jobs;
  hipLaunchKernelGGL(pusch_seq_kernel<miphy_pusch_demod_job>, dim3(n, 1), dim3(SCR_THREADS), 0, s, dj, gt, seq, stride, have_ph);
  const size_t lds = fft_lds_bytes(12 * (size_t)max_nprb);
  if (extras)
    hipLaunchKernelGGL(pusch_demod_tp_kernel<true>, dim3(n, 14), dim3(TP_THREADS), lds, s, dj, (const float2*)grid, (const float2*)ce, scalars, llr,
                       (const uint32_t*)seq, stride, tws, placeholders, evm_sums);
  else
    hipLaunchKernelGGL(pusch_demod_tp_kernel<false>, dim3(n, 14), dim3(TP_THREADS), lds, s, dj, (const float2*)grid, (const float2*)ce, scalars, llr,
                       (const uint32_t*)seq, stride, tws, placeholders, evm_sums);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

} // namespace

extern "C" int miphy_pusch_demodulate_tp_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                  const float* ce, const float* scalars, int8_t* llr, const uint16_t* placeholders, float* evm_sums, void* stream)
{
  return pusch_demodulate_tp("pusch_demodulate_tp", ctx, jobs, jobs_on_device, n, grid, ce, scalars, llr, placeholders, evm_sums, true, stream);
}

extern "C" int miphy_pusch_demodulate_tp_batch(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                               const float* ce, const float* scalars, int8_t* llr, void* stream)
{
  return pusch_demodulate_tp("pusch_demodulate_tp", ctx, jobs, jobs_on_device, n, grid, ce, scalars, llr, nullptr, nullptr, false, stream);
}

extern "C" uint32_t miphy_pusch_demod_nof_llr(const miphy_pusch_demod_job* j)
{
  if (!j || (j->dmrs_type != 1 && j->dmrs_type != 2) || j->grid_nof_prb > 275)
    return 0;
  unsigned dm = 0;
  for (unsigned k = 0; k < 12; ++k)
    dm += (j->dmrs_type == 1) ? ((k % 2) < j->nof_cdm_groups_without_data) : ((k % 6) < 2u * j->nof_cdm_groups_without_data);
  const unsigned nprb = miphy_count_prb(j->rb_mask, j->grid_nof_prb);
  unsigned       n    = 0;
  for (unsigned s = j->start_symbol; s < (unsigned)j->start_symbol + j->nof_symbols && s < 14; ++s)
    n += nprb * (((j->dmrs_symbols_mask >> s) & 1) ? 12 - dm : 12);
  return n * j->mod;
}

extern "C" uint32_t miphy_pusch_demod_layers_nof_llr(const miphy_pusch_demod_layers_job* lj)
{
  if (!lj || lj->nof_tx_layers < 1 || lj->nof_tx_layers > 4 || lj->nof_tx_layers > lj->base.nof_rx_ports)
    return 0;
  return miphy_pusch_demod_nof_llr(&lj->base) * lj->nof_tx_layers;
}

extern "C" int miphy_pusch_demodulate_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                               const float* ce, const float* scalars, int8_t* llr, const uint16_t* placeholders, float* evm_sums,
                                               void* stream)
{
  return pusch_demodulate("pusch_demodulate", ctx, jobs, jobs_on_device, n, grid, ce, scalars, nullptr, llr, placeholders, evm_sums, true, stream);
}

extern "C" int miphy_pusch_demodulate_batch(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                            const float* ce, const float* scalars, int8_t* llr, void* stream)
{
  return miphy_pusch_demodulate_batch_ex(ctx, jobs, jobs_on_device, n, grid, ce, scalars, llr, nullptr, nullptr, stream);
}

extern "C" int miphy_pusch_demodulate_layers_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_layers_job* jobs, int jobs_on_device, uint32_t n,
                                                      const float* grid, const float* ce, const float* scalars, int8_t* llr, const uint16_t* placeholders,
                                                      float* evm_sums, void* stream)
{
  return pusch_demodulate("pusch_demodulate_layers", ctx, jobs, jobs_on_device, n, grid, ce, scalars, nullptr, llr, placeholders, evm_sums, true, stream);
}

extern "C" int miphy_pusch_demodulate_layers_batch(miphy_ctx* ctx, const miphy_pusch_demod_layers_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                   const float* ce, const float* scalars, int8_t* llr, void* stream)
{
  return pusch_demodulate("pusch_demodulate_layers", ctx, jobs, jobs_on_device, n, grid, ce, scalars, nullptr, llr, nullptr, nullptr, false, stream);
}

extern "C" int miphy_pusch_demodulate_layers_mmse_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_mmse_job* jobs, int jobs_on_device, uint32_t n,
                                                           const float* grid, const float* ce, const float* scalars, const float* cov, int8_t* llr,
                                                           const uint16_t* placeholders, float* evm_sums, void* stream)
{
  return pusch_demodulate("pusch_demodulate_layers_mmse", ctx, jobs, jobs_on_device, n, grid, ce, scalars, cov, llr, placeholders, evm_sums, true, stream);
}

extern "C" int miphy_pusch_demodulate_layers_mmse_batch(miphy_ctx* ctx, const miphy_pusch_demod_mmse_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                        const float* ce, const float* scalars, const float* cov, int8_t* llr, void* stream)
{
  return pusch_demodulate("pusch_demodulate_layers_mmse", ctx, jobs, jobs_on_device, n, grid, ce, scalars, cov, llr, nullptr, nullptr, false, stream);
}
