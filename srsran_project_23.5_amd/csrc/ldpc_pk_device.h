// Device code shared by the LDPC decoder kernels: the packed row update of ldpc_decode_pk.hip (one codeblock per workgroup) and
// ldpc_decode_pkw.hip (several small codeblocks per wavefront), and the hard decision, checksum and write-back that these two and the
// one-row-per-lane kernel of ldpc_decode_row.hip have in common. Arithmetic contract: ldpc_decoder_impl.cpp:60-146 +
// ldpc_decoder_avx2.cpp:66-243, avx2_support.h:65-106 of the reference; every kernel built from these functions is bit-identical to it.
#pragma once
#include "miphy_internal.h"
#include <type_traits>

namespace {

typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 as_s2(uint32_t x)
{
  return __builtin_bit_cast(s16x2, x);
}
__device__ __forceinline__ uint32_t as_u(s16x2 x)
{
  return __builtin_bit_cast(uint32_t, x);
}
__device__ __forceinline__ s16x2 splat(int c)
{
  return s16x2{(short)c, (short)c};
}
__device__ __forceinline__ s16x2 pk_min(s16x2 a, s16x2 b)
{
  return __builtin_elementwise_min(a, b);
}
__device__ __forceinline__ s16x2 pk_max(s16x2 a, s16x2 b)
{
  return __builtin_elementwise_max(a, b);
}
__device__ __forceinline__ s16x2 pk_ashr15(s16x2 a)
{
  return a >> splat(15);
}
// two sign-extended bytes -> one register with two int16 (bytes 1:0 of each source)
__device__ __forceinline__ s16x2 pk_pair(int lo, int hi)
{
  return as_s2(__builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u));
}
// Message dword {A1, A0, B1, B0} (bytes 0..3) -> edge 0 = (sext A0, sext B0), edge 1 = (sext A1, sext B1).
// v_perm_b32 selectors 8 / 9 replicate the sign of byte 1 / 3 of the low source (10 / 11: of the high source).
__device__ __forceinline__ s16x2 c2v_even(uint32_t w)
{
  return as_s2(__builtin_amdgcn_perm(w, w, 0x09030801u));
}
__device__ __forceinline__ s16x2 c2v_odd(uint32_t w)
{
  const uint32_t h = w << 8; // bytes {0, A1, A0, B1}: A1 -> byte 1, B1 -> byte 3
  return as_s2(__builtin_amdgcn_perm(h, h, 0x09030801u));
}
__device__ __forceinline__ uint32_t c2v_pack(s16x2 c0, s16x2 c1)
{
  // {S0 = c0 -> bytes 4..7, S1 = c1 -> bytes 0..3}: out = {c1.A, c0.A, c1.B, c0.B}
  return __builtin_amdgcn_perm(as_u(c0), as_u(c1), 0x06020400u);
}

// Finer stamps inside a layer of the latency form (tools/ldpc_phase_probe.py --inner; debug build with -DLDPC_PK_PROFILE2 only).
#ifdef LDPC_PK_PROFILE2
__device__ unsigned long long g_ldpc_prof2[8];
#define P2_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define P2_ADD(slot, a, b)                                                 \
  do {                                                                     \
    if (threadIdx.x == 0)                                                  \
      atomicAdd(&g_ldpc_prof2[slot], (unsigned long long)((b) - (a)));     \
  } while (0)
#else
#define P2_T(var)
#define P2_ADD(slot, a, b)
#endif

// Wavefront priorities of the packed decoders (s_setprio, 0 = lowest). The SIMD's arbiter otherwise favours the oldest ready wavefront; a
// wavefront that is about to REQUEST the soft bits and messages of a layer should go first (its LDS round trip then runs under the other
// wavefronts' arithmetic), the long first phase of the row update last, the second phase (stores, then the barrier the codeblock's other
// wavefronts wait at) and the phases around the layer loop in between. Measured on the headline launch (38 912 codeblocks, same box):
// no priorities 3.72 ms, request 1 alone 3.64, request 2 + second phase 1 3.46-3.52, request 3 + second phase 2 3.47, the same + outside 2
// 3.43 (the values below), outside 3 3.45, second phase 3 3.52, first phase 1 3.48. -D overrides keep the A-B of tools/ab_bench.py possible.
#ifndef LDPC_PK_SETPRIO
#define LDPC_PK_SETPRIO 3
#endif
#ifndef LDPC_PK_SETPRIO1
#define LDPC_PK_SETPRIO1 0
#endif
#ifndef LDPC_PK_SETPRIO2
#define LDPC_PK_SETPRIO2 2
#endif
#ifndef LDPC_PK_SETPRIO_OUT
#define LDPC_PK_SETPRIO_OUT 2
#endif

constexpr int LLR_MAX = 120;
constexpr int LLR_INF = 127;
constexpr int INF_MUL = 255; // an infinite soft bit (|s| > 120) becomes a message of magnitude >= 255 + 24
// The smallest |v| an infinite soft bit can give: 255 |d| + t with |d| >= 1 and |t| <= 120 against it. A finite one gives |v| <= 120, so
// "min |v| >= 135" says that every soft bit a row read was infinite ("saturated rows").
constexpr int V_INF_MIN = INF_MUL - LLR_MAX;
// The smallest magnitude of an infinite soft bit: "every |v + c| >= 121" says that every soft bit a row WRITES is infinite.
constexpr int S_INF_MIN = LLR_MAX + 1;
// Scaled 120: the message every edge of a row gets whose inputs are all infinite (both minima clipped at 120).
constexpr int C_SAT = (LLR_MAX * 52428) >> 16;
// What the detection of saturated rows takes off the unclipped first minimum of a row of odd parity, so that min1u + C_SAT - it reaches
// S_INF_MIN exactly when min1u reaches V_INF_MIN, and a finite min1u (<= 120, with any scaled second minimum <= C_SAT) stays below.
constexpr int ODD_PARITY_DROP = V_INF_MIN + C_SAT - S_INF_MIN;
static_assert(C_SAT == 95 && ODD_PARITY_DROP == 109 && LLR_MAX + C_SAT - ODD_PARITY_DROP < S_INF_MIN, "saturated rows: the odd-parity term");

// Stage A of a row update, shared by its forms: both rows' soft-bit addresses of every edge of the layer with packed 16-bit arithmetic:
// {l, l + H} + shift, wrap at Z by the unsigned minimum of p and p - Z -- three packed instructions for the two rows. The pair has to be
// split into two 32-bit addresses, one instruction per row that selects a half (v_add_u32_sdwa); the column offset is the other operand
// of that very addition, so that it costs no instruction of its own (a packed "+ {co, co}" before the split left the split adding zero).
// LDS addresses stay below 2^16.
// FOLD = false adds the column offset to the pair first and `base` in the split, four packed instructions and the two of the split.
// It is the form of the instances that the other one does not shorten (VALU instructions of a 19-edge visit, FOLD = false / true):
//  - the wave kernel, request phase 114 / 152: its `base` is a per-lane group offset, and co + base a vector addition per edge on top
//    of the split;
//  - the latency form, 6 / 7 per edge: its {shift, column} words are scalar registers fetched a layer ahead, and the compiler leaves
//    the split as an addition of zero and adds the offset in an instruction of its own;
//  - the throughput form that does not dematch, compiled for 128 registers: 630 / 628 in its 19-edge visit that reads messages (the
//    request phase saves its instructions, the allocator spends them again in the second phase), and the kernel spills one vector
//    register and six scalar ones more (its other visits would gain; the spill is not accepted).
// The throughput form that dematches while it loads (168 registers, both message homes) takes FOLD = true: request phase 116 -> 95, a
// 19-edge visit 602 -> 581 (tools/visit_valu_count.py).
template <int D, bool FOLD>
__device__ __forceinline__ void pk_edge_addresses(uint32_t (&adrA)[D], uint32_t (&adrB)[D], const uint32_t* __restrict__ edges, int l, int H, int Z, uint32_t base)
{
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 X  = {(unsigned short)l, (unsigned short)(l + H)};
  const u16x2 Zs = {(unsigned short)Z, (unsigned short)Z};
#pragma unroll
  for (int j = 0; j < D; ++j) {
#ifdef LDPC_PK_EMU_NOSLOAD // timing-only (WRONG results): no scalar loads of the edge table
    const unsigned short sh = (unsigned short)(7 * j + (l & 1)), co = (unsigned short)(j * Z);
#else
    const unsigned short sh = (unsigned short)edges[2 * j], co = (unsigned short)edges[2 * j + 1];
#endif
    const u16x2 T = X + u16x2{sh, sh};
    const u16x2 R = __builtin_elementwise_min(T, (u16x2)(T - Zs));
    if (FOLD) {
      const uint32_t P = __builtin_bit_cast(uint32_t, R), cb = (uint32_t)co + base;
      adrA[j] = (P & 0xffffu) + cb;
      adrB[j] = (P >> 16) + cb;
    } else {
      const uint32_t P = __builtin_bit_cast(uint32_t, (u16x2)(R + u16x2{co, co}));
      adrA[j] = (P & 0xffffu) + base;
      adrB[j] = (P >> 16) + base;
    }
  }
}

// The same addresses read from a table (ATAB instances of the throughput form): they depend on lane, base graph, lifting size, layer and
// edge only, so the host computes them once per (base graph, Z, layers) -- miphy_ldpc_address_table, the arithmetic above with base = 0 --
// as adr[layer][edge quad][lane] of four dwords, component k = edge 4 q + k as adrA | adrB << 16 (a layer is padded to a multiple of four
// edges). A visit holds its ceil(D / 4) quads in registers, splits each component with a mask and a shift -- two VALU instructions per
// edge instead of five -- and requests the quads of the NEXT visit at the start of its second phase, where the raw soft bits of this
// one are dead: the loads (coalesced, 1 KB per wavefront each, served by L2) return under the second phase and the layer barrier.
typedef uint32_t pk_adr_quad __attribute__((ext_vector_type(4)));
// A table is read through a buffer descriptor: the layer and quad offsets are scalar operands of the load and the lane offset its one
// vector operand, so that a request issues no address arithmetic (a global_load took a 64-bit vector addition per quad), and the
// descriptor bounds every access by the size of the table.
struct pk_adr_row {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t               soff; // byte offset of the layer's first quad (wave-uniform)
};
// TIE: an empty asm keeps the split in the visit, behind its s_setprio (the compiler otherwise hoists it out of the instances of a visit, in
// front of the priority). Not in the instances that can leave a visit out (saturated rows, ldpc_decode_pk.hip): with a path through the
// layer loop that does not pass through the asm, the tie costs a register copy per word, 19 more VALU instructions per visit.
template <int D, bool TIE = true>
__device__ __forceinline__ void pk_table_addresses(uint32_t (&adrA)[D], uint32_t (&adrB)[D], const pk_adr_quad* q)
{
#pragma unroll
  for (int j = 0; j < D; ++j) {
    uint32_t w = q[j >> 2][j & 3];
    if constexpr (TIE)
      asm volatile("" : "+v"(w));
    adrA[j] = w & 0xffffu;
    adrB[j]          = w >> 16;
  }
}
// A soft bit of an ATAB visit: the table holds LDS addresses, and the soft bits are the first array of the workgroup's LDS (ldpc_decode_pk.hip:
// the kernel has no static LDS), so an entry IS the address. Through `soft` the compiler adds the array's base to every half it selects
// (the value is zero, the instruction stays: one slow-class v_add_u32_sdwa per half); as an absolute LDS address the halves are an AND
// with a literal (fast class, tools/valu_probe) and a shift.
template <bool ATAB>
__device__ __forceinline__ int8_t& pk_soft_bit(int8_t* soft, uint32_t adr)
{
  if constexpr (ATAB)
    return *(int8_t*)(__attribute__((address_space(3))) int8_t*)(uintptr_t)adr;
  else
    return soft[adr];
}
// `voff` = this lane's byte offset in a quad, `stride` = bytes of a quad. Of a last quad with three edges only three words are loaded:
// nothing reads the fourth, and a register the allocator knows to be free is reused while the load is in flight -- behind a wait for it.
template <int D>
__device__ __forceinline__ void pk_table_request(pk_adr_quad* q, pk_adr_row row, uint32_t voff, uint32_t stride)
{
  typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
#pragma unroll
  for (int k = 0; k < (D + 3) / 4; ++k) {
    if (4 * k + 3 == D) {
      const u32x3 t = __builtin_amdgcn_raw_buffer_load_b96(row.rsrc, (int)voff, (int)(row.soff + k * stride), 0);
      q[k]          = pk_adr_quad{t.x, t.y, t.z, 0u};
    } else {
      q[k] = __builtin_amdgcn_raw_buffer_load_b128(row.rsrc, (int)voff, (int)(row.soff + k * stride), 0);
    }
  }
}

// Where the soft-bit addresses of a visit come from. Computed: the layer's {shift, column * Z} words (pk_edge_addresses), this lane's row
// pair (l, l + H) and `base` = LDS byte offset of the codeblock's soft bits (0 where a workgroup holds one codeblock: the term then folds away).
struct pk_adr_computed {
  static constexpr bool TABLE = false;
  const uint32_t*       edges;
  int                   l, H, Z;
  uint32_t              base;
};
// From a table (ATAB instances): the addresses of this visit arrive in `q` (pk_table_addresses), which leaves with those of the layer at
// `next`, requested with this lane's `voff` and the quad `stride` (pk_table_request).
struct pk_adr_table {
  static constexpr bool TABLE = true;
  pk_adr_quad*          q;
  pk_adr_row            next;
  uint32_t              voff, stride;
};
// PARTS > 1 (latency form of the packed kernel: PARTS times the wavefronts per codeblock, each part of the workgroup owns a share of
// the edges of a layer): D is the number of edges of THIS part; between the two phases the parts exchange their partial {min1, min2,
// sign parity} through LDS (`xch` = this lane's column of the exchange area [part][3][xs], `part` = this part) and merge them -- the
// two smallest magnitudes of a union are min(a1, b1) and min(max(a1, b1), min(a2, b2)), an associative rule. The function then
// contains a workgroup barrier: EVERY thread calls it, `active` = the lane owns rows (an idle lane computes on soft bits it may read
// but stores nothing).
// `mid` is called once between the two phases (the latency form issues the scalar loads of the next layer's edges there: behind the last LDS
// read of the layer, so that they do not turn the partial lgkmcnt waits on the in-order LDS returns into waits for everything).
template <typename MID>
struct pk_exchange {
  uint32_t* xch;
  int       part, xs;
  bool      active;
  MID       mid;
};
struct pk_no_exchange {}; // PARTS == 1: every other caller
// DETECT (PARTS == 1; the instances of the packed throughput kernel that leave out visits -- every other caller gets the update as it was,
// instruction for instruction) returns: every one of the 2 D soft bits this lane WRITES is infinite. An infinite soft bit stays infinite
// with its sign, so the next visit of these rows reads infinite soft bits only and is frozen -- it and every later one of the layer
// rewrites each of them to +-127 with the sign it has, whatever the messages are -- so a wavefront whose lanes all say so may leave out
// its later visits of the layer (ldpc_decode_pk.hip, "saturated rows"). No per-edge work: with min1 <= min2 the two smallest |v| clipped
// at 120, s1 / s2 their scaled values and min1u the unclipped min1,
//   every output infinite  <=>  min1u >= V_INF_MIN (every INPUT infinite), or the sign parity is even and min(min1 + s2, min2 + s1) >= 121:
// with even parity a message has the sign of its own v, |r| = min(127, |v| + |c|); the edge that holds the minimum gets s2, every other
// one has |v| >= min2 and gets s1 (a tie at the minimum: min2 = min1); with odd parity a finite edge is pulled towards zero and stays finite.
// Merged into one comparison: min1u may stand for min1 in the first term (min1u > 120 means min1 = 120, s2 = 95: the term is >= 121 either
// way), and odd parity takes ODD_PARITY_DROP off that term -- it then reaches 121 exactly when every input is infinite. Eight instructions
// per visit: the running minima start from 0x7fff instead of 120 and are clipped behind the edge loop (three packed minima; 120 twice in a
// running minimum IS the clip: the same min1 / min2), then a packed multiply-add, two additions, two minima and a compare.
template <int D, bool FIRST, int PARTS = 1, bool FOLD, bool DETECT = false, typename ADR, typename XCH = pk_no_exchange>
__device__ __forceinline__ bool update_rows_pk(int8_t* __restrict__ soft,
                                               uint32_t* __restrict__ c2v, // this lane's message dword of edges 0,1 of the layer
                                               ADR adr,
                                               XCH x = XCH())
{
  constexpr bool SPLIT = PARTS > 1, ATAB = ADR::TABLE;
  static_assert(SPLIT != std::is_same<XCH, pk_no_exchange>::value, "the latency form, and nobody else, exchanges partial results");
  s16x2    v2c[D], mabs[D];
  uint32_t adrA[D], adrB[D];
  int      rawA[D], rawB[D];
  uint32_t cw[(D + 1) / 2];
  P2_T(q0);
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO); // the address arithmetic and the LDS requests of a layer
  // Stage A: every address of the layer, then every LDS read of the layer in one go (2 soft bits per edge + the old
  // messages): the latency of the LDS pipe is paid once per layer instead of once per group of edges.
  static_assert(!(DETECT && SPLIT), "the latency form runs every visit");
  if constexpr (ATAB)
    pk_table_addresses<D, !DETECT>(adrA, adrB, adr.q);
  else
    pk_edge_addresses<D, FOLD>(adrA, adrB, adr.edges, adr.l, adr.H, adr.Z, adr.base);
  P2_T(q1);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    rawA[j] = pk_soft_bit<ATAB>(soft, adrA[j]);
    rawB[j] = pk_soft_bit<ATAB>(soft, adrB[j]);
  }
  if (!FIRST) {
#pragma unroll
    for (int jj = 0; jj < (D + 1) / 2; ++jj)
      cw[jj] = c2v[64 * jj];
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO1);
  __builtin_amdgcn_sched_barrier(0);
  P2_T(q2);
  s16x2    mag1 = splat(DETECT ? 0x7fff : LLR_MAX), mag2 = mag1;
  uint32_t spx  = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const s16x2 s = pk_pair(rawA[j], rawB[j]);
    // |s| > 120: infinite soft bit -> "infinite" message with the same sign: d != 0 only then, and 255 * d dominates.
    const s16x2 sc = pk_min(pk_max(s, splat(-LLR_MAX)), splat(LLR_MAX));
    const s16x2 d  = s - sc;
    s16x2       t  = sc;
    if (!FIRST) {
      const uint32_t w = cw[j >> 1];
      const s16x2    c = (j & 1) ? c2v_odd(w) : c2v_even(w);
      t                = pk_min(pk_max(sc - c, splat(-LLR_MAX)), splat(LLR_MAX));
    }
    const s16x2 v = d * splat(INF_MUL) + t;
    v2c[j]        = v;
    spx ^= as_u(v);
    const s16x2 av   = pk_max(v, -v);
    mabs[j]          = av;
    const s16x2 help = pk_max(mag1, av);
    mag1             = pk_min(mag1, av);
    mag2             = pk_min(mag2, help);
  }
  bool                   all_inf = false;
  [[maybe_unused]] s16x2 mag1u;
  if constexpr (DETECT) {
    mag1u   = mag1;
    mag1    = pk_min(mag1, splat(LLR_MAX));
    mag2    = pk_min(mag2, splat(LLR_MAX));
  }
  P2_T(q3);
#ifdef LDPC_PK_PROFILE2
  unsigned long long q4 = q3;
#endif
  if constexpr (SPLIT) {
    uint32_t* const xch = x.xch;
    const int       part = x.part, xs = x.xs;
    uint32_t*       xw = xch + 3 * part * xs;
    xw[0] = as_u(mag1), xw[xs] = as_u(mag2), xw[2 * xs] = spx;
#ifndef LDPC_PK_EMU_NOXBAR // timing-only (WRONG results): no barrier in the exchange
    __syncthreads();
#endif
#ifdef LDPC_PK_PROFILE2
    q4 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
    for (int o = 1; o < PARTS; ++o) {
      const int       other = (part + o) & (PARTS - 1); // the merge is commutative: any order gives the same two minima
      const uint32_t* xr    = xch + 3 * other * xs;
      const s16x2     o1 = as_s2(xr[0]), o2 = as_s2(xr[xs]);
      spx ^= xr[2 * xs];
      mag2 = pk_min(pk_max(mag1, o1), pk_min(mag2, o2));
      mag1 = pk_min(mag1, o1);
    }
  }
  P2_T(q5);
  bool active = true;
  if constexpr (SPLIT) {
    x.mid();
    active = x.active;
  }
  // FENCE (the table instance that detects): the scaling and the test come in front of the second phase's address request, fenced off
  // from it, so that the unclipped minimum is dead before the next visit's quads arrive -- with both alive the allocator, at its limit
  // of 168 registers there, rebuilds 32 constants of the checksum in front of every visit. Not in the instances that compute their
  // addresses: the plain one spills more with the fence than without it.
  constexpr bool FENCE = DETECT && ATAB;
  if constexpr (!FENCE) {
    __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO2); // the second phase: messages, soft-bit stores, then the layer barrier
    if constexpr (ATAB)
      pk_table_request<D>(adr.q, adr.next, adr.voff, adr.stride);
  }
  // Scaling by 0.8 = floor(x * 52428 / 65536), per row (avx2_support.h:65-106).
  const uint32_t s1A = ((uint32_t)(uint16_t)mag1.x * 52428u) >> 16, s1B = ((uint32_t)(uint16_t)mag1.y * 52428u) >> 16;
  const uint32_t s2A = ((uint32_t)(uint16_t)mag2.x * 52428u) >> 16, s2B = ((uint32_t)(uint16_t)mag2.y * 52428u) >> 16;
  // The product of ALL signs is folded into the two candidate magnitudes once per layer; an edge then only applies its own sign.
  const s16x2 pm  = pk_ashr15(as_s2(spx));
  const s16x2 s2u = as_s2(s2A | (s2B << 16));
  const s16x2 s1u = as_s2(s1A | (s1B << 16));
  const s16x2 s2p = as_s2(as_u(s2u) ^ as_u(pm)) - pm;
  const s16x2 dsp = (as_s2(as_u(s1u) ^ as_u(pm)) - pm) - s2p; // +-(min1 - min2), scaled
  if constexpr (DETECT) { // every soft bit these two rows write is infinite (see above; pm = -1 where the parity is odd)
    const s16x2 low = pk_min(pm * splat(ODD_PARITY_DROP) + mag1u + s2u, mag2 + s1u);
    all_inf         = as_u(pk_min(low, splat(S_INF_MIN))) == as_u(splat(S_INF_MIN));
  }
  if constexpr (FENCE) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO2);
    pk_table_request<D>(adr.q, adr.next, adr.voff, adr.stride);
  }
  s16x2 cprev = splat(0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const s16x2 v = v2c[j];
    // x = 0 where |v| == min1 (this edge provided the minimum, or ties it: then min1 == min2), 1 elsewhere
    const s16x2 x   = pk_min(mabs[j] - mag1, splat(1));
    const s16x2 mag = x * dsp + s2p;
    const s16x2 m   = pk_ashr15(v); // -1 where this edge's own message is negative
    const s16x2 c   = as_s2(as_u(mag) ^ as_u(m)) - m;
    const uint32_t r = as_u(pk_min(pk_max(c + v, splat(-LLR_INF)), splat(LLR_INF)));
    if (!SPLIT || active) {
      if (j & 1)
        c2v[64 * (j >> 1)] = c2v_pack(cprev, c);
      else if (j == D - 1)
        c2v[64 * (j >> 1)] = c2v_pack(c, c);
      pk_soft_bit<ATAB>(soft, adrA[j]) = (int8_t)r;
      pk_soft_bit<ATAB>(soft, adrB[j]) = (int8_t)(r >> 16);
    }
    cprev = c;
  }
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO1);
  P2_T(q6);
  P2_ADD(0, q0, q1); // scalar edge loads + address arithmetic
  P2_ADD(1, q1, q2); // LDS reads issued and returned
  P2_ADD(2, q2, q3); // phase 1
  P2_ADD(3, q3, q4); // exchange: stores + barrier
  P2_ADD(4, q4, q5); // exchange: loads + merge
  P2_ADD(5, q5, q6); // scaling + phase 2 + stores
  P2_ADD(6, q0, q6);
  return all_inf;
}

// The row update of layers 1 and 2 in the FIRST iteration of the throughput form and the wave kernel, where one edge of the row is known
// to read a soft bit of zero (ZE = its position in the row: 0 in layer 1, 1 in layer 2) and no message of the layer exists yet.
// What makes it exact ("first iteration"):
//  - Every decode starts with the two punctured columns, soft bits [0, 2Z), at zero: ldpc_decode_pk.hip pk_fused_load ("the two punctured
//    nodes"), ldpc_frame_device.h cb_plain_load ("soft[k] = 0" for k < 2 Z), ldpc_decode_pkw.hip ("clear the group's soft bits").
//  - Layer 0 of both base graphs holds columns 0 AND 1: two zero inputs, min1 = min2 = 0, every message 0, no soft bit changes -- the
//    kernels do not visit it in iteration 0 at all, and visit it in iteration 1 with the FIRST instance (no message read = zeros read).
//  - Layer 1 has column 0 as its edge 0 and lacks column 1; layer 2 has columns 0, 1 as edges 0, 1, and layer 1 has left column 1 at
//    zero (miphy_ctx.hip asserts these facts of the tables at compile time). With a zero at edge ZE, min1 = 0: the general update gives
//    every OTHER edge the message 0 and leaves its soft bit as it is; edge ZE gets the product of the other signs times
//    floor(0.8 min(120, min |s| of the others)) as its message, and, being zero before, as its soft bit too. A further zero among the
//    other edges (column 0 in layer 2, a zero input) gives min = 0 here and min1 = min2 = 0 there: the same zeros.
//  - "As it is" has one exception: the general update rewrites a raw input of +-121 ... +-126 to +-127. No output sees it: every
//    |s| > 120 is treated alike (d != 0 above: same sign, minima clipped at 120, x = 1, stored as +-127 at its next general visit), and
//    soft bits are not an output -- hard bits, CRC verdict and iteration count are.
// So: the soft bits of the other D - 1 edges are read, one packed minimum of |s| and the sign parity are accumulated, the value goes to
// edge ZE's soft bits and byte slots of the layer's message dwords (layout of update_rows_pk, zeros elsewhere); no other soft bit is stored.
template <int D, int ZE, bool FOLD, typename ADR>
__device__ __forceinline__ void update_rows_pk_zero(int8_t* __restrict__ soft, uint32_t* __restrict__ c2v, ADR adr)
{
  constexpr bool ATAB = ADR::TABLE;
  static_assert((ZE == 0 || ZE == 1) && D > 2, "the known-zero edge is edge 0 or 1 of its row, and other edges exist");
  uint32_t adrA[D], adrB[D];
  int      rawA[D], rawB[D];
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO);
  if constexpr (ATAB)
    pk_table_addresses<D>(adrA, adrB, adr.q);
  else
    pk_edge_addresses<D, FOLD>(adrA, adrB, adr.edges, adr.l, adr.H, adr.Z, adr.base);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if (j != ZE) {
      rawA[j] = pk_soft_bit<ATAB>(soft, adrA[j]);
      rawB[j] = pk_soft_bit<ATAB>(soft, adrB[j]);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO1);
  __builtin_amdgcn_sched_barrier(0);
  s16x2    mag = splat(LLR_MAX);
  uint32_t spx = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if (j != ZE) {
      const s16x2 s = pk_pair(rawA[j], rawB[j]);
      spx ^= as_u(s);
      mag = pk_min(mag, pk_max(s, -s));
    }
  }
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO2);
  if constexpr (ATAB)
    pk_table_request<D>(adr.q, adr.next, adr.voff, adr.stride);
  const uint32_t sA = ((uint32_t)(uint16_t)mag.x * 52428u) >> 16, sB = ((uint32_t)(uint16_t)mag.y * 52428u) >> 16;
  const s16x2    pm = pk_ashr15(as_s2(spx));
  const s16x2    c  = as_s2((sA | (sB << 16)) ^ as_u(pm)) - pm; // |c| <= 96: no clamp
  const uint32_t r  = as_u(c);
  c2v[0] = ZE ? c2v_pack(splat(0), c) : c2v_pack(c, splat(0));
#pragma unroll
  for (int jj = 1; jj < (D + 1) / 2; ++jj)
    c2v[64 * jj] = 0u; // (an odd degree's last dword holds its last edge twice: zero either way)
  pk_soft_bit<ATAB>(soft, adrA[ZE]) = (int8_t)r;
  pk_soft_bit<ATAB>(soft, adrB[ZE]) = (int8_t)(r >> 16);
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO1);
}

// A part without edges in this layer (a low-degree layer split four ways): it contributes the neutral partial result and takes part in
// the exchange barrier.
template <typename MID>
__device__ __forceinline__ void update_rows_pk_none(pk_exchange<MID> x)
{
  uint32_t* xw = x.xch + 3 * x.part * x.xs;
  xw[0] = as_u(splat(LLR_MAX)), xw[x.xs] = as_u(splat(LLR_MAX)), xw[2 * x.xs] = 0u;
  __syncthreads();
  x.mid();
}

// The latency form: this part's edges of a layer of degree d. The ceil(d / 2) message pairs of the layer are dealt to the parts in
// contiguous runs (part i takes pairs [P i / PARTS, P (i + 1) / PARTS)), so every split falls on a message pair and the message layout
// is that of the throughput form. A part's share is at most PK_PART_EDGES edges (degree <= 19: 10 of two parts, 6 of four).
// Its {shift, column} words are fetched ONE LAYER AHEAD as scalar values (load_part_edges): with one codeblock per CU nothing hides the
// scalar-load round trip at the head of a layer (0.14 us per layer visit, measured by replacing the table with constants).
template <int PARTS>
struct part_edges {
  static constexpr int EMAX = PARTS == 4 ? 6 : 10;
  uint32_t             w[2 * EMAX]; // {shift, column * Z} of this part's edges (words behind its share belong to the next edges: unused)
  int                  da;          // edges of this part in the layer
  int                  p0;          // first message pair of this part in the layer
};

template <int PARTS>
__device__ __forceinline__ void load_part_edges(part_edges<PARTS>& pe, const uint32_t* __restrict__ edges_g, uint32_t li, int part)
{
  const int d = (int)((li >> 10) & 0x3fu), P = (d + 1) >> 1;
  const int p0 = (P * part) / PARTS, p1 = (P * (part + 1)) / PARTS;
  pe.p0 = p0, pe.da = min(2 * p1, d) - 2 * p0;
  const uint32_t* e = edges_g + 2 * ((int)(li & 0x3ffu) + 2 * p0); // (reads past a layer's or the table's last edge stay inside miphy_graph_tables)
#pragma unroll
  for (int k = 0; k < 2 * part_edges<PARTS>::EMAX; ++k)
    pe.w[k] = e[k];
}

template <bool FIRST, int PARTS, typename MID>
__device__ __forceinline__ void update_rows_pk_split(const part_edges<PARTS>& pe, int8_t* soft, uint32_t* c2v, int l, int H, int Z, pk_exchange<MID> x)
{
  const pk_adr_computed adr = {pe.w, l, H, Z, 0};
  c2v += 64 * pe.p0;
  switch (pe.da) {
#define PK_SPLIT_CASE(N)                                                                            \
  case N:                                                                                           \
    if (N <= part_edges<PARTS>::EMAX)                                                               \
      update_rows_pk<(N <= part_edges<PARTS>::EMAX ? N : 1), FIRST, PARTS, false>(soft, c2v, adr, x); \
    break;
    PK_SPLIT_CASE(10)
    PK_SPLIT_CASE(9)
    PK_SPLIT_CASE(6)
    PK_SPLIT_CASE(5)
    PK_SPLIT_CASE(4)
    PK_SPLIT_CASE(3)
    PK_SPLIT_CASE(2)
    PK_SPLIT_CASE(1)
    default:
      update_rows_pk_none(x);
      break;
#undef PK_SPLIT_CASE
  }
}

template <bool FIRST, bool FOLD, bool DETECT = false>
__device__ __forceinline__ bool update_rows_pk_any(int d, int8_t* soft, uint32_t* c2v, pk_adr_computed adr)
{
  switch (d) {
#define PK_ANY_CASE(N) \
  case N:              \
    return update_rows_pk<N, FIRST, 1, FOLD, DETECT>(soft, c2v, adr);
    PK_ANY_CASE(19)
    PK_ANY_CASE(10)
    PK_ANY_CASE(9)
    PK_ANY_CASE(8)
    PK_ANY_CASE(7)
    PK_ANY_CASE(6)
    PK_ANY_CASE(5)
    PK_ANY_CASE(4)
#undef PK_ANY_CASE
    default:
      return update_rows_pk<3, FIRST, 1, FOLD, DETECT>(soft, c2v, adr);
  }
}

// Layers m = 1 and 2 of the first iteration: the degrees these two layers have in the two base graphs (miphy_ctx.hip asserts them).
template <bool FOLD>
__device__ __forceinline__ void update_rows_pk_zero_any(int m, int d, int8_t* soft, uint32_t* c2v, pk_adr_computed adr)
{
  if (m == 1) {
    if (d == 19)
      update_rows_pk_zero<19, 0, FOLD>(soft, c2v, adr);
    else
      update_rows_pk_zero<10, 0, FOLD>(soft, c2v, adr);
  } else {
    if (d == 19)
      update_rows_pk_zero<19, 1, FOLD>(soft, c2v, adr);
    else
      update_rows_pk_zero<8, 1, FOLD>(soft, c2v, adr);
  }
}

// One layer visit of the throughput form and the wave kernel. Iteration 0 starts at layer 1 (see update_rows_pk_zero: layer 0 changes
// nothing there), so layer 0's messages are first written in iteration 1, by the instance that reads none. FOLD: pk_edge_addresses.
// Returns what update_rows_pk does; the known-zero visits read a zero and never say that their rows are saturated.
template <bool FOLD, bool DETECT = false>
__device__ __forceinline__ bool update_rows_pk_visit(int it, int m, int d, int8_t* soft, uint32_t* c2v, pk_adr_computed adr)
{
  bool r = false;
  if (it == 0 && (m == 1 || m == 2))
    update_rows_pk_zero_any<FOLD>(m, d, soft, c2v, adr);
  else if (it == 0 || (it == 1 && m == 0))
    r = update_rows_pk_any<true, FOLD, DETECT>(d, soft, c2v, adr);
  else
    r = update_rows_pk_any<false, FOLD, DETECT>(d, soft, c2v, adr);
  return r;
}

// The same visit of an ATAB instance: every layer the launch can reach has degree D (the launch planner sees to that).
template <int D, bool DETECT = false>
__device__ __forceinline__ bool update_rows_pk_visit_tab(int it, int m, int8_t* soft, uint32_t* c2v, pk_adr_table adr)
{
  if (it == 0 && m == 1) {
    update_rows_pk_zero<D, 0, true>(soft, c2v, adr);
    return false;
  }
  if (it == 0 && m == 2) {
    update_rows_pk_zero<D, 1, true>(soft, c2v, adr);
    return false;
  }
  if (it == 0 || (it == 1 && m == 0))
    return update_rows_pk<D, true, 1, true, DETECT>(soft, c2v, adr);
  return update_rows_pk<D, false, 1, true, DETECT>(soft, c2v, adr);
}

__device__ __forceinline__ uint32_t gf2_mulmod(uint32_t a, uint32_t b, uint32_t poly, uint32_t order)
{
  uint32_t       r   = 0;
  const uint32_t top = 1u << order;
  for (int k = (int)order - 1; k >= 0; --k) {
    r <<= 1;
    r ^= (r & top) ? poly : 0u;
    r ^= ((b >> k) & 1u) ? a : 0u;
  }
  return r;
}

// Hard decision of the 32 consecutive soft bits starting at soft[32 t] (16-byte aligned); returns the big-endian numeric value (first bit
// in bit 31). Positions >= K are masked to 0. bit = (llr <= 0), log_likelihood_ratio.h:86.
// Four soft bytes per operation: bit 7 of a byte of ((x & 0x7f..) + 0x7f..) says "low seven bits non-zero", and the byte is > 0 when that
// bit is set and its sign bit is clear. v_dot4_u32_u8 then gathers the four flags of a dword (0x80 or 0 per byte) MSB first: with the byte
// weights {0x80, 0x40, 0x20, 0x10} for an even dword and {8, 4, 2, 1} for the odd one behind it, two chained dot products give 128 times
// the eight bits of a byte of the word, and the accumulator input takes the byte in front of it. The word is the complement of the
// "> 0" bits. It is the word of crc_zmask as well (miphy_internal.h): checksum and output share one decision.
__device__ __forceinline__ uint32_t hard_word(const int8_t* soft, int t, int K)
{
  const uint4*   p  = reinterpret_cast<const uint4*>(soft) + 2 * t;
  const uint4    lo = p[0], hi = p[1];
  const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t       h[2]; // 128 times bits 0..15 and bits 16..31 of the word, as numbers
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t acc = 0;
#pragma unroll
    for (int q = 4 * k; q < 4 * k + 4; ++q) {
      const uint32_t xq  = x[q ^ 1]; // the odd dword of a pair first: its byte is the inner accumulator
      const uint32_t nz  = (xq & 0x7f7f7f7fu) + 0x7f7f7f7fu;
      const uint32_t pos = ~xq & nz & 0x80808080u;
      if (q == 4 * k + 2)
        acc <<= 8;
      acc = __builtin_amdgcn_udot4(pos, (q & 1) ? 0x10204080u : 0x01020408u, acc, false);
    }
    h[k] = acc;
  }
  uint32_t  w   = ~((h[0] << 9) | (h[1] >> 7));
  const int rem = K - 32 * t;
  if (rem < 32)
    w &= (rem <= 0) ? 0u : (0xffffffffu << (32 - rem));
  return w;
}

// Checksum of the first L hard bits in the mask / popcount form (crc_zmask in miphy_internal.h: no bit-serial division, no position
// weights): this lane's parity word over the message words first, first + stride, ... The XOR of the lanes' words is zero exactly when
// the checksum is. zi = table index of the polynomial, order = its degree.
// KEEP (the packed kernel's evaluation in front of the output): the lane decides every word of the K >= L message bits it is about to
// store -- the same words on the same lanes as store_hard_words -- and returns its first two in `kept`, masked at K, so that the output
// does not read and decide the soft bits again (store_kept_words).
template <bool KEEP = false>
__device__ __forceinline__ uint32_t crc_zmask_partial(const int8_t* soft, const miphy_graph_tables* __restrict__ tab, int zi, int order, int L, int first,
                                                      int stride, int K = 0, uint32_t* kept = nullptr)
{
  const int nw = (L + 31) >> 5, nk = KEEP ? (K + 31) >> 5 : nw;
  uint32_t  acc[24];
#pragma unroll
  for (int k = 0; k < 24; ++k)
    acc[k] = 0;
  [[maybe_unused]] uint32_t k0 = 0, k1 = 0;
  [[maybe_unused]] int      i  = 0;
  for (int t = first; t < nk; t += stride) {
    uint32_t w = hard_word(soft, t, KEEP ? K : L);
    if constexpr (KEEP) {
      k0 = (i == 0) ? w : k0;
      k1 = (i == 1) ? w : k1;
      ++i;
      if (t >= nw)
        continue;
      const int rem = L - 32 * t;
      if (rem < 32) // last word of the checksum: positions >= L are not message bits
        w &= 0xffffffffu << (32 - rem);
    }
    const uint4* m = reinterpret_cast<const uint4*>(tab->crc_zmask[zi][nw - 1 - t]);
#pragma unroll
    for (int g = 0; g < 6; ++g) {
      const uint4 mk = m[g];
      acc[4 * g + 0] += __builtin_popcount(w & mk.x);
      acc[4 * g + 1] += __builtin_popcount(w & mk.y);
      acc[4 * g + 2] += __builtin_popcount(w & mk.z);
      acc[4 * g + 3] += __builtin_popcount(w & mk.w);
    }
  }
  if constexpr (KEEP)
    kept[0] = k0, kept[1] = k1;
  // bit 0 of every count, one funnel shift each: count k enters at bit 31 and ends at bit 8 + k
  uint32_t par = 0;
#pragma unroll
  for (int k = 0; k < 24; ++k)
    par = __builtin_amdgcn_alignbit(acc[k], par, 1);
  return (par >> 8) & ((1u << order) - 1u);
}

// The same by division, for polynomials without a mask table (CRC24C, CRC11): the partial remainder of each 32-bit word times its
// position weight x^(32 (nfull - 1 - t) + rbits) mod P. The XOR of the lanes' words is the checksum.
__device__ __forceinline__ uint32_t crc_div_partial(const int8_t* soft, const miphy_graph_tables* __restrict__ tab, int crc_id, uint32_t poly, uint32_t order,
                                                    int K, int L, int first, int stride)
{
  const int      nfull = L >> 5, rbits = L & 31, nwords = (L + 31) >> 5;
  const uint32_t top   = 1u << order;
  uint32_t       part  = 0;
  for (int t = first; t < nwords; t += stride) {
    const uint32_t w   = hard_word(soft, t, K);
    const int      len = min(32, L - 32 * t);
    uint32_t       reg = 0;
    for (int b = 0; b < len; ++b) {
      reg = (reg << 1) ^ (((w >> (31 - b)) & 1u) << order);
      reg ^= (reg & top) ? poly : 0u;
    }
    reg &= top - 1u;
    if (t < nfull) {
      reg = gf2_mulmod(reg, tab->crc_pow32[crc_id][nfull - 1 - t], poly, order);
      for (int b = 0; b < rbits; ++b) {
        reg <<= 1;
        reg ^= (reg & top) ? poly : 0u;
      }
    }
    part ^= reg;
  }
  return part;
}

// XOR of a partial checksum over the workgroup (every thread must call): wavefront shuffles, then red[2 ...] of the reduction words.
__device__ __forceinline__ uint32_t block_xor(uint32_t part, uint32_t* red, int tid, int nt)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    part ^= __shfl_xor(part, off);
  if ((tid & 63) == 0)
    red[2 + (tid >> 6)] = part;
  __syncthreads();
  uint32_t crc = 0;
  for (int w = 0; w < (nt >> 6); ++w)
    crc ^= red[2 + w];
  __syncthreads();
  return crc;
}

// One word of the final hard bits (MSB first) to its place among the K message bits: a dword where the output allows it, bytes otherwise.
__device__ __forceinline__ void store_hard_word(uint8_t* out, bool out_aligned, uint32_t w, int t, int K)
{
  const int nbytes = min(4, (K - 32 * t + 7) / 8);
  if (nbytes == 4 && out_aligned) {
    reinterpret_cast<uint32_t*>(out)[t] = __builtin_bswap32(w); // MSB-first bytes
  } else {
    for (int q = 0; q < nbytes; ++q)
      out[4 * t + q] = (uint8_t)(w >> (24 - 8 * q));
  }
}

// The final hard bits of a codeblock, MSB first, words first, first + stride, ... of the K message bits. `base` as in update_rows_pk
// (the wave kernel's group offset: added per word, which is the code the kernel had with the loop written out).
__device__ __forceinline__ void store_hard_words(const int8_t* soft, uint8_t* out, int K, int first, int stride, uint32_t base = 0)
{
  const bool out_aligned = ((uintptr_t)out & 3u) == 0;
  const int  kwords      = (K + 31) >> 5;
  for (int t = first; t < kwords; t += stride)
    store_hard_word(out, out_aligned, hard_word(soft + base, t, K), t, K);
}

// The same where the checksum in front of the output has decided this lane's words already (crc_zmask_partial<true>): the first two come
// from `kept`; a lane with more words (no geometry of the packed kernel has one: K / 32 <= 0.6875 Z + 1 words on >= Z / 2 lanes) decides
// the others here.
__device__ __forceinline__ void store_kept_words(const int8_t* soft, uint8_t* out, int K, int first, int stride, const uint32_t* kept)
{
  const bool out_aligned = ((uintptr_t)out & 3u) == 0;
  const int  kwords      = (K + 31) >> 5;
  if (first < kwords)
    store_hard_word(out, out_aligned, kept[0], first, K);
  if (first + stride < kwords)
    store_hard_word(out, out_aligned, kept[1], first + stride, K);
  for (int t = first + 2 * stride; t < kwords; t += stride)
    store_hard_word(out, out_aligned, hard_word(soft, t, K), t, K);
}

} // namespace
