// LDPC decoder, packed variant: every lane owns TWO lifted check rows (l and l + Z/2) and processes them with the packed
// 16-bit VALU instructions of CDNA (v_pk_add/sub/min/max/mad), halving both the instruction count per codeblock and the
// number of wavefronts a codeblock occupies. Same arithmetic contract as ldpc_decode_row.hip (reference:
// ldpc_decoder_impl.cpp:60-146 + ldpc_decoder_avx2.cpp:66-243, avx2_support.h:65-106); results are bit-identical.
//
// Check-to-variable messages are kept EXPLICITLY in LDS, one int8 per (edge, row), no VALU work to rebuild a message from
// compressed min/argmin/sign state (which dominated an earlier formulation). A lane packs the messages of two consecutive
// edges into one dword {A(j+1), A(j), B(j+1), B(j)} (bytes 0..3): edge j sits in the odd bytes, where v_perm_b32 can
// sign-extend it to two int16 in ONE instruction; edge j+1 needs one extra shift. Per wave the dwords of an edge pair are
// 64 consecutive words: conflict-free, immediate offsets, and only one LDS read and one LDS write per TWO edges (measured on
// gfx950: a DS write costs ~5 cycles of the CU's LDS pipe whatever its width, a read ~2.8 -- tools/lds_probe.hip).
#include "miphy_internal.h"
#include "rdm_device.h"
#include "ldpc_frame_device.h"
#include <algorithm>
#include <cstdlib>

namespace {

// Is the checksum of the first L hard bits zero? (every thread of the block must call) Mask / popcount form where the polynomial has a
// table (zi >= 0), by division otherwise; words strided over the block's threads.
// `kept` receives this lane's words of the K message bits, decided on the way (crc_zmask_partial<true>): every evaluation stands in front of
// the output or of another evaluation, so the words of the last one are the output (store_kept_words).
template <bool KEEP>
__device__ __forceinline__ bool block_crc_is_zero(const int8_t* soft, const miphy_graph_tables* __restrict__ tab, int zi, int order, int L, int K,
                                                  uint32_t* kept, uint32_t* red, int tid, int nt)
{
  return block_xor(crc_zmask_partial<KEEP>(soft, tab, zi, order, L, tid, nt, K, kept), red, tid, nt) == 0;
}

__device__ __forceinline__ uint32_t block_crc(const int8_t* soft, const miphy_graph_tables* __restrict__ tab, int crc_id, uint32_t poly,
                                              uint32_t order, int K, int L, uint32_t* red, int tid, int nt)
{
  return block_xor(crc_div_partial(soft, tab, crc_id, poly, order, K, L, tid, nt), red, tid, nt);
}

// Phase timing for tools/ldpc_phase_probe.py (debug build with -DLDPC_PK_PROFILE only; never compiled into libmiphy.so).
#ifdef LDPC_PK_PROFILE
__device__ unsigned long long g_ldpc_prof[2048 * 8]; // per workgroup: 7 phase sums + codeblock count (no atomics: one writer per row)
#define PROF_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define PROF_ADD(slot, a, b) prof_acc[slot] += (unsigned long long)((b) - (a))
#define PROF_COUNT()                                              \
  do {                                                            \
    if (tid == 0 && blockIdx.x < 2048) {                          \
      for (int q = 0; q < 7; ++q)                                 \
        g_ldpc_prof[blockIdx.x * 8 + q] += prof_acc[q];           \
      g_ldpc_prof[blockIdx.x * 8 + 7] += 1;                       \
    }                                                             \
    for (int q = 0; q < 7; ++q)                                   \
      prof_acc[q] = 0;                                            \
  } while (0)
#else
#define PROF_T(var)
#define PROF_ADD(slot, a, b)
#define PROF_COUNT()
#endif

// Wavefronts per SIMD the register allocation is held to: 4 (128 registers, five 3-wavefront codeblocks per CU with the messages in
// global memory) measured 11 % faster for the plain decoder. The variant that dematches while loading runs at 3: its load phase is a
// function of its own (pk_fused_load) and the prefetch registers are reassigned unconditionally, which leaves the kernel at 160
// registers without a single spill (3.89 ms per 38 912 codeblocks; 3.95 with the load phase inlined and 20 spills); at 4 wavefronts the
// launcher moves the messages to global memory for a fifth codeblock per CU, and that traffic next to the soft-buffer image stream
// costs more than the occupancy gives (4.63 ms).
#define LDPC_PK_MIN_WAVES_PLAIN 4
#ifndef LDPC_PK_MIN_WAVES_SPLIT
#define LDPC_PK_MIN_WAVES_SPLIT 3 // the latency form: its launches never fill a CU, the register budget is free
#endif
#ifndef LDPC_PK_MIN_WAVES_FUSED
#define LDPC_PK_MIN_WAVES_FUSED 3
#endif
// Raw form of load_in16(): the dword-aligned 16 bytes and the following dword of input vector v, not yet funnel-shifted, so that a
// prefetch keeps them in flight (the shift happens where the vector is consumed).
struct raw_in16 {
  uint32_t a0, a1, a2, a3, e;
};
__device__ __forceinline__ raw_in16 load_in16_raw(const int8_t* __restrict__ in, int mb, int v)
{
  const uint32_t* p4 = reinterpret_cast<const uint32_t*>(in - mb) + 4 * v;
  const rdm_u4    a  = *reinterpret_cast<const rdm_u4*>(p4);
  raw_in16        r;
  r.a0 = a.x, r.a1 = a.y, r.a2 = a.z, r.a3 = a.w;
  r.e  = (mb != 0) ? p4[4] : 0u;
  return r;
}
__device__ __forceinline__ uint4 shift_in16(const raw_in16& r, int mb)
{
  if (mb == 0)
    return make_uint4(r.a0, r.a1, r.a2, r.a3);
  return make_uint4(__builtin_amdgcn_alignbyte(r.a1, r.a0, mb), __builtin_amdgcn_alignbyte(r.a2, r.a1, mb), __builtin_amdgcn_alignbyte(r.a3, r.a2, mb),
                    __builtin_amdgcn_alignbyte(r.e, r.a3, mb));
}
constexpr int PK_PRE = 3; // rate-matched input vectors per lane fetched one codeblock ahead (3 x 192 lanes x 16 B = 9216 B)

// Whole 16-byte vectors of an input of E bytes whose address is mb bytes past a dword boundary (load_in16 reads a dword beyond a vector
// that is not aligned).
__device__ __forceinline__ int pk_in16_vectors(int mb, int E)
{
  return (mb == 0) ? (E >> 4) : ((E >= 4) ? ((E - 4) >> 4) : 0);
}
// (Re)fills pre[] with the first input vectors of codeblock c of the launch, zeros where there is no such codeblock or vector: every
// element is always assigned -- an old value must not stay live across the decode of a codeblock.
__device__ __forceinline__ void pk_prefetch(raw_in16 (&pre)[PK_PRE], uint32_t c, uint32_t n, const miphy_ldpc_rdm_desc* __restrict__ rdm,
                                            const int8_t* __restrict__ rm_in_base, const uint32_t* __restrict__ cb_order, int tid, int nt)
{
#pragma unroll
  for (int k = 0; k < PK_PRE; ++k)
    pre[k] = raw_in16{0, 0, 0, 0, 0};
  if (c < n) {
    const miphy_ldpc_rdm_desc r  = load_words(rdm + (cb_order ? cb_order[c] : c));
    const int8_t*             in = rm_in_base + r.in_offset;
    const int                 mb = (int)(((uintptr_t)in) & 3), nq = pk_in16_vectors(mb, (int)r.E);
#pragma unroll
    for (int k = 0; k < PK_PRE; ++k) {
      pre[k] = raw_in16{0, 0, 0, 0, 0};
      if (tid + k * nt < nq)
        pre[k] = load_in16_raw(in, mb, tid + k * nt);
    }
  }
}

// FUSED = the codeblock's first transmission is rate-dematched while it is loaded (ldpc_rate_dematcher_impl.cpp:43-254 for
// new data, redundancy version 0, full circular buffer, E + fillers <= N): `llr_base` is then the HARQ soft-buffer array, which
// receives the dematched codeblock exactly as the reference's dematcher leaves it (data, fillers at +127, zeros behind), and the
// rate-matched LLRs come from `rm_in_base` through the descriptors `rdm` (same index as `descs`). The input of the NEXT codeblock
// of the workgroup is fetched into registers while the current one decodes.
// GMSG = the check-to-variable messages live in global memory instead of LDS (`gmsg`: per resident workgroup
// [wave][edge pair][64 lanes] dwords, `gmsg_pairs` pairs per wave): a lane only ever touches its own messages, one coalesced dword
// per two edges and layer visit, re-read an iteration later out of L2 / Infinity Cache. Low-rate codeblocks (many layers) then
// need LDS for their soft bits only, so that four of them stay resident per CU instead of one.
// The load phase of the variant that dematches while loading, as a function of its own (never inlined): its staging needs far more
// registers than the layer loop, and inlined it decides the register allocation of the whole kernel; out of line the kernel holds
// LDPC_PK_MIN_WAVES_FUSED wavefronts per SIMD with a layer loop free of scratch accesses, and only this phase pays for its spills.
// A plain pointer argument of a function that is not inlined is a generic one (flat_load: both wait counters, aperture test); the
// rate-matched input is global memory, and a parameter that says so gives global_load.
typedef __attribute__((address_space(1))) const int8_t* global_ci8;
__device__ __attribute__((noinline)) void pk_fused_load(int8_t* __restrict__ soft, global_ci8 in_global, int E, int F, int mod, int Z, int bgK, int soft_bytes,
                                                        raw_in16 p0, raw_in16 p1, raw_in16 p2, int tid, int nt)
{
  static_assert(PK_PRE == 3, "three prefetched vectors are passed by value");
  const int8_t* __restrict__ in = (const int8_t*)in_global;
    // ---- rate dematching into the LDS image soft[2Z + j] = buffer position j
    // (the lane index is made opaque here: the compiler would otherwise hoist every per-lane staging address out of the
    // codeblock loop and keep dozens of them alive across the decoder)
    int stid = tid;
    asm volatile("" : "+v"(stid));
    const int                 mb  = (int)(((uintptr_t)in) & 3);
    const int                 nq  = pk_in16_vectors(mb, E);
    int8_t*                   img = soft + 2 * Z;
    rm_geom                   g;
    g.r0 = 0, g.f1 = (bgK - 2) * Z, g.f0 = g.f1 - F, g.F = F, g.E = E, g.mod = mod, g.Kq = E / mod;
    image_access ia;
    ia.jbase = 0;
    {
      uint4* z4 = reinterpret_cast<uint4*>(soft);
      for (int k = stid; k < (2 * Z) >> 4; k += nt) // the two punctured nodes (Z is a multiple of 16 for every Z >= 128)
        z4[k] = make_uint4(0, 0, 0, 0);
      for (int k = g.f0 + stid; k < g.f1; k += nt)
        img[k] = 127; // fillers
      for (int k = 2 * Z + E + F + stid; k < soft_bytes; k += nt)
        soft[k] = 0; // never transmitted
    }
    switch (mod) {
#define PK_STAGE(MOD)                                                                         \
  case MOD:                                                                                   \
    _Pragma("unroll") for (int k = 0; k < PK_PRE; ++k) if (stid + k * nt < nq)                 \
        stage_vector<MOD>(ia, img, g, F, stid + k * nt, shift_in16(k == 0 ? p0 : (k == 1 ? p1 : p2), mb));               \
    for (int v = stid + PK_PRE * nt; v < nq; v += nt)                                          \
      stage_vector<MOD>(ia, img, g, F, v, load_in16(in, mb, v));                              \
    break;
      PK_STAGE(8)
      PK_STAGE(6)
      PK_STAGE(4)
      PK_STAGE(2)
      default:
        PK_STAGE(1)
#undef PK_STAGE
    }
    for (int k = (nq << 4) + stid; k < E; k += nt) {
      const int p = k / (int)mod, q = k - p * (int)mod;
      const int r = q * g.Kq + p;
      img[r + ((r >= g.f0) ? F : 0)] = in[k];
    }
    __syncthreads();
}

// The image goes to the HARQ soft buffer (what the reference's dematcher leaves there) while the last non-zero soft bit is found
// (ldpc_decoder_impl.cpp:86-99). Inlined into the kernel: a function has to wait for its stores before it returns (25 KB per
// codeblock on their way to HBM), here they drain under the first layers. Returns this lane's candidate for the position behind the
// last non-zero soft bit.
// The search starts at the end of the data, `end` = E + F (everything behind it was just written as zero, pk_fused_load), and goes back
// until a vector holds a non-zero byte -- in practice the last one: every wavefront looks at the same 64 vectors per step, highest vector
// in lane 0, and stops on a wave-uniform test, so that no wavefront waits for another and every lane reaches the caller's atomicMax.
__device__ __forceinline__ int pk_fused_image_out(const int8_t* __restrict__ soft, int8_t* __restrict__ llr_img, int Z, int bgi, int in_len, int end, int tid, int nt)
{
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4*       dst  = reinterpret_cast<u32x4*>(llr_img);
  const uint4* src  = reinterpret_cast<const uint4*>(soft + 2 * Z);
  const int    nimg = in_len >> 4, nall = ((miphy_bg_N_short(bgi) * Z) >> 4);
  // (the lane index is made opaque, as in pk_fused_load: the compiler otherwise hoists this lane's share of the store address out of the
  // codeblock loop and carries it across the decoder in scratch)
  asm volatile("" : "+v"(tid));
  for (int q = tid; q < nimg; q += nt) {
    const uint4 v = src[q];
    const u32x4 o = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(o, dst + q);
  }
  const u32x4 zero = {0, 0, 0, 0};
  for (int q = nimg + tid; q < nall; q += nt)
    __builtin_nontemporal_store(zero, dst + q);
  int last = 0;
  for (int hi = __builtin_amdgcn_readfirstlane((min(end, in_len) - 1) >> 4); hi >= 0; hi -= 64) {
    const int q = hi - (tid & 63);
    if (q >= 0)
      last = last_nonzero_behind(src[q], q, 0);
    if (__builtin_amdgcn_ballot_w64(last != 0))
      break;
  }
  return last;
}

// PARTS > 1 = the latency form for launches that leave most of the chip idle (a single slot is 38 codeblocks on 256 CUs): PARTS times the
// wavefronts per codeblock, the PARTS parts of the workgroup share the edges of every layer (update_rows_pk, PARTS) -- about 1 / PARTS of the
// instructions per wavefront and layer for one more barrier, same results, same LDS image (messages always in LDS).
// ATAB = the soft-bit addresses of a visit are read from a table instead of computed (pk_table_addresses, ldpc_pk_device.h): throughput
// form of launches whose reachable layers all have PK_ATAB_DEGREE edges. `adr_by_z[Z / 16]` is the table of lifting size Z,
// [layer][quad][lane of the workgroup]. The quads of the first layer visited are requested in front of the load phase, every other
// visit's by the visit before it (across the iteration's CRC and the layer barrier: 19 registers, the raw soft bits are dead there).
//
// Saturated rows (RSKIP instances of the throughput forms; every other instance runs every visit with the row update as it was -- the launch
// planner takes RSKIP where a launch can profit, ldpc_decode.hip; the argument is DESIGN.md section 4): a general row update reports per lane that every soft
// bit it WROTE is infinite (update_rows_pk: a closed form of the two minima and the sign parity, no per-edge work). An infinite soft bit stays
// infinite with its sign, so these rows read infinite soft bits only from their next visit on, and such rows are frozen: every later update of
// them rewrites each soft bit to +-127 with the sign it has and needs no message of theirs, so no hard bit, checksum or iteration count can
// come out of it differently. (Reporting at the visit that READ infinite soft bits only, the first form of the test, paid for one visit per
// wavefront and layer that was already frozen.) A wavefront whose
// row-owning lanes ALL report it at a visit of layer m sets bit m of a mask of its own (scalar registers, cleared per codeblock) and from
// then on leaves out the body of its visits of layer m: no request, no arithmetic, no message or soft-bit traffic -- straight to the
// layer's barrier. Nothing is shared between wavefronts and no wavefront leaves a loop early: each executes exactly the barriers it would
// without the mask.
// ATAB and the mask: a visit's addresses are requested by the visit that runs before it, so a visit that runs requests those of the NEXT
// VISIT THAT RUNS: the next layer in turn whose bit is clear (layer m + 1, or layer 0 behind the last one, while no bit is set). A visit
// that is left out touches neither the quads nor the table. A layer's bit changes only at its own visits, and the layers between two
// visits that run have their bits set for good, so the layer named at the request is the one whose visit consumes the quads: no visit
// ever splits the addresses of another layer. (Once every bit is set the last request names layer 0 and nothing consumes it.)
constexpr int PK_ATAB_DEGREE = MIPHY_LDPC_ADR_TABLE_DEGREE, PK_ATAB_QUADS = (PK_ATAB_DEGREE + 3) / 4;
template <bool FUSED, bool GMSG, int PARTS = 1, bool ATAB = false, bool RSKIP = false>
__global__ void __launch_bounds__(192 * PARTS, PARTS > 1 ? LDPC_PK_MIN_WAVES_SPLIT : (FUSED ? LDPC_PK_MIN_WAVES_FUSED : LDPC_PK_MIN_WAVES_PLAIN))
ldpc_decode_pk_kernel(const miphy_ldpc_dec_desc* __restrict__ descs,
                      const miphy_graph_tables* __restrict__ tab,
                      const int8_t* __restrict__ llr_base,
                      uint8_t* __restrict__ out_base,
                      int32_t* __restrict__ iters_out,
                      int max_nodes,
                      const uint32_t* __restrict__ harq_slot,
                      uint8_t* __restrict__ harq_crc_ok,
                      uint32_t n,
                      uint32_t* __restrict__ queue,
                      const miphy_ldpc_rdm_desc* __restrict__ rdm,
                      const int8_t* __restrict__ rm_in_base,
                      uint32_t* __restrict__ gmsg,
                      int gmsg_pairs,
                      int lds_pairs, // GMSG: the first lds_pairs message dwords of a lane stay in LDS (a layer boundary), the other gmsg_pairs are global
                      const uint32_t* __restrict__ cb_order, // optional: the launch decodes codeblocks order[0 .. n) of the arrays (one class of a sorted batch)
                      const pk_adr_quad* const* __restrict__ adr_by_z) // ATAB: the address table of every lifting size of the launch, at [Z / 16]
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int nt  = blockDim.x;
  constexpr bool SPLIT = PARTS > 1;
  constexpr bool KEEPW = FUSED && !SPLIT; // the checksum's words are kept for the output (crc_zmask_partial<true>)
  static_assert(PARTS == 1 || PARTS == 2 || PARTS == 4, "parts of the latency form");
  static_assert(!(SPLIT && GMSG), "the latency form keeps its messages in LDS");
  static_assert(!ATAB || (FUSED && !GMSG && !SPLIT), "address tables: the throughput form that dematches, messages in LDS");
  static_assert(!(RSKIP && (SPLIT || GMSG)), "visits are left out by the throughput forms with their messages in LDS");
  const int nth  = nt / PARTS;                   // threads that own rows: the whole workgroup, or each part of it
  // (wave-uniform by construction -- nth is a multiple of 64 --, and said so: the part selects the edges of a layer, which must stay scalar loads)
  const int part = SPLIT ? __builtin_amdgcn_readfirstlane((tid >= nth) + (PARTS > 2 ? (tid >= 2 * nth) + (tid >= 3 * nth) : 0)) : 0;
  const int lr   = tid - part * nth;             // row pair (lr, lr + H) of this lane
  raw_in16  pre[PK_PRE];
  if (FUSED)
    pk_prefetch(pre, blockIdx.x, n, rdm, rm_in_base, cb_order, tid, nt);
  // Persistent workgroups: the grid is what the chip holds at once; a workgroup decodes codeblock blockIdx.x first and then takes
  // codeblocks gridDim.x, gridDim.x + 1, ... from the launch's queue counter until the batch is exhausted (every wave reaches the
  // exit: the counter only grows). No workgroup launch / LDS allocation between codeblocks, and heterogeneous batches balance.
#ifdef LDPC_PK_PROFILE
  unsigned long long prof_acc[7] = {};
#endif
  for (uint32_t q = blockIdx.x; q < n;) {
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO_OUT); // the phases around the layer loop (load / dematch, CRC, output): ldpc_pk_device.h
  PROF_T(p_start);
  const uint32_t cb = cb_order ? cb_order[q] : q;
  const miphy_ldpc_dec_desc dsc = load_words(descs + cb);
  const int                 Z   = dsc.Z;
  const int                 H   = (Z + 1) >> 1;
  const int                 bgi = (dsc.bg == 1) ? 0 : 1;
  const int                 bgK = miphy_bg_K(bgi);
  const int                 bgM = miphy_bg_M(bgi);
  const int                 K   = bgK * Z;
  const int                 zp  = tab->z_pos[Z];

  // Soft bits come FIRST in the dynamic LDS block: the kernel has no static LDS, so their base is the constant 0 and folds
  // into the DS instructions (a run-time base would cost one v_add per access). Then the check-to-variable messages,
  // [wave][edge pair][64 lanes] dwords, then a few reduction words. Everything is sized by the layers the batch can reach, so
  // a high-rate batch (4 layers, 76 edges) packs 4 codeblocks = 12 waves per CU.
  int8_t*   soft       = reinterpret_cast<int8_t*>(smem);
  const int lay_alloc  = miphy_ldpc_layers(bgi, max_nodes);
  const int soft_bytes = miphy_ldpc_soft_bytes(bgi, lay_alloc, Z);
  const int pairs_all  = tab->pair_start[bgi][lay_alloc];
  const int pairs_lds  = GMSG ? lds_pairs : pairs_all;
  uint32_t* c2v_lane   = reinterpret_cast<uint32_t*>(smem + soft_bytes) + (lr >> 6) * (pairs_lds * 64) + (lr & 63);
  uint32_t* c2v_glob   = GMSG ? gmsg + ((size_t)blockIdx.x * (nt >> 6) + (tid >> 6)) * ((size_t)gmsg_pairs * 64) + (tid & 63) - 64 * (size_t)pairs_lds : nullptr;
  uint32_t* red        = reinterpret_cast<uint32_t*>(smem + soft_bytes) + (nth >> 6) * (pairs_lds * 64);
  // latency form: exchange slots behind the reduction words, [part][3][nth] dwords
  uint32_t* xch = red + 16 + lr;

  // Next codeblock of this workgroup (taken now so that the queue round trip is off the critical path).
  __syncthreads(); // the previous codeblock's readers of red[] / soft[] are done
  if (tid == 0) {
    // One ticket per codeblock processed: the launch draws exactly n tickets (0 .. n - 1), so the workgroup that draws the last one
    // knows nobody else will touch the counter and leaves it at zero for the next launch (no clearing memset per launch, and a
    // captured launch can be replayed).
    const uint32_t ticket = atomicAdd(queue, 1u);
    if (ticket == n - 1u)
      *queue = 0u;
    red[15] = gridDim.x + ticket;
  }
  if (!FUSED && harq_crc_ok && harq_crc_ok[harq_slot[cb]]) {
    if (tid == 0)
      iters_out[cb] = -1;
    __syncthreads();
    q = red[15];
    continue;
  }
  const int8_t* llr    = llr_base + dsc.llr_offset;
  uint8_t*      out    = out_base + dsc.out_offset;
  const int     in_len = (int)dsc.in_len;

  if (tid < 15)
    red[tid] = 0;
  int last = 0;
  // (bound once, by reference, for the two sites below: the closure is what the register allocation of the instances that do not dematch was
  // tuned with -- without it <false, true> spills two more vector registers)
  auto prefetch = [&](uint32_t c) { pk_prefetch(pre, c, n, rdm, rm_in_base, cb_order, tid, nt); };
  pk_adr_quad    anx[ATAB ? PK_ATAB_QUADS : 1]; // ATAB: the soft-bit addresses of the next layer visit
  pk_adr_row     atab    = pk_adr_row();        // ... the table of this lifting size
  const uint32_t astride = 16u * (uint32_t)nt, alayer = PK_ATAB_QUADS * astride; // ... bytes of a quad and of a layer
  if (ATAB) {
    // (wave-uniform, and said so: the codeblock index comes out of LDS, and a descriptor the compiler takes for divergent is a loop per load)
    const int zq = __builtin_amdgcn_readfirstlane(Z >> 4), bytes = __builtin_amdgcn_readfirstlane(lay_alloc * (int)alayer);
    atab.rsrc    = __builtin_amdgcn_make_buffer_rsrc(const_cast<pk_adr_quad*>(adr_by_z[zq]), 0, bytes, 0x00020000);
    atab.soff = alayer; // layer 1: the first one visited
    pk_table_request<PK_ATAB_DEGREE>(anx, atab, 16u * (uint32_t)tid, astride);
  }
  if (FUSED) {
    const miphy_ldpc_rdm_desc rd = load_words(rdm + cb);
    pk_fused_load(soft, (global_ci8)(rm_in_base + rd.in_offset), (int)rd.E, (int)dsc.nof_filler_bits, (int)rd.mod, Z, bgK, soft_bytes, pre[0], pre[1], pre[2], tid, nt);
    last = pk_fused_image_out(soft, const_cast<int8_t*>(llr), Z, bgi, in_len, (int)rd.E + (int)dsc.nof_filler_bits, tid, nt);
  } else {
    last = cb_plain_load(soft, llr, in_len, Z, soft_bytes, tid, nt);
  }
  atomicMax(reinterpret_cast<int*>(&red[0]), last);
  __syncthreads();
  last = (int)red[0];

  const bool use_crc = dsc.crc_poly != MIPHY_CRC_NONE;
  if (last == 0) {
    if (!use_crc) {
      store_all_ones(out, K, tid, nt);
    }
    if (tid == 0) {
      iters_out[cb] = 0;
      if (FUSED && harq_crc_ok)
        harq_crc_ok[harq_slot[cb]] = 0;
    }
    if (FUSED)
      prefetch(red[15]);
    q = red[15];
    continue;
  }
  const int nof_layers = cb_nof_layers(last, Z, bgi);

  const uint32_t* edges_g   = tab->edge_sb[bgi][zp];
  // Per-layer constants of the base graph, one layer per lane (loaded once per codeblock): first edge (bits 0-9), degree (10-15),
  // first message pair (16-31). Inside the layer loop they come out with v_readlane instead of three dependent 16-bit loads at the
  // head of every layer.
  uint32_t lay_info = 0;
  {
    const int ml = tid & 63;
    if (ml < bgM) {
      const uint32_t e0 = tab->row_start[bgi][ml];
      lay_info          = e0 | (((uint32_t)tab->row_start[bgi][ml + 1] - e0) << 10) | ((uint32_t)tab->pair_start[bgi][ml] << 16);
    }
  }
  uint32_t        poly = 0, order = 0;
  int             L = 0;
  if (use_crc) {
    poly  = tab->crc_poly[dsc.crc_poly];
    order = tab->crc_order[dsc.crc_poly];
    L     = K - dsc.nof_filler_bits;
  }
  const bool final_only = use_crc && (dsc.flags & 1u);
  // mask form of the CRC zero test where the polynomial has a table (every polynomial a codeblock carries)
  const int zi = (use_crc && L <= 32 * MIPHY_CRC_ZMASK_WORDS) ? miphy_crc_zmask_index(dsc.crc_poly) : -1;

  int       result_iters = 0;
  const int max_iter     = dsc.max_iter;
  uint32_t  kept[2]      = {0, 0}; // this lane's words of the hard bits, as the last checksum evaluation decided them
  PROF_T(p_loaded);
  PROF_ADD(0, p_start, p_loaded);
  // The two wrap constants of the address computations live in VECTOR registers: a VOP2 add / sub with a scalar operand issues at
  // the rate of the three-operand encodings (2.88 instead of 1.93 cycles at three waves per SIMD, tools/valu_probe), and three of
  // the eight address instructions per edge only have Z or Z/2 as their second operand.
  // Odd lifting size: the last lane would own rows H - 1 and Z (= row 0 again, a lane's second row is l + H). Its distance to the
  // second row is set to zero instead: both halves of its packed registers then carry row H - 1, read the same soft bits, compute
  // the same values and store them to the same addresses -- no row is visited twice and no instruction is added.
  int Zv = Z, Hv = (lr + H < Z) ? H : 0;
#ifndef LDPC_PK_SCALAR_WRAP
  asm volatile("" : "+v"(Zv), "+v"(Hv));
#endif
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO1);
  part_edges<PARTS> pe; // latency form: this part's edges of the layer about to run, fetched while the layer before it runs
  // Iteration 0 starts at layer 1: layer 0 reads both punctured columns, which are zero then, so all its messages are zero and no
  // soft bit changes (update_rows_pk_zero, ldpc_pk_device.h). Its messages are first written in iteration 1, by the FIRST instance.
  if (SPLIT)
    load_part_edges<PARTS>(pe, edges_g, (uint32_t)__builtin_amdgcn_readlane((int)lay_info, 1), part); // the first layer visited
  [[maybe_unused]] uint64_t sat_layers = 0; // bit m: this wavefront's rows of layer m are saturated (wave-uniform; bgM <= 46 layers)
  for (int it = 0; it < max_iter; ++it) {
    for (int m = (it == 0) ? 1 : 0; m < nof_layers; ++m) {
      const uint32_t  li    = (uint32_t)__builtin_amdgcn_readlane((int)lay_info, m);
      const int       e0    = (int)(li & 0x3ffu);
      const int       d     = (int)((li >> 10) & 0x3fu);
      const uint32_t* edges = edges_g + 2 * e0;
      PROF_T(p_l0);
      if constexpr (SPLIT) { // every thread: the function holds the barrier of the exchange
        part_edges<PARTS> pn;
        const uint32_t    lin  = (uint32_t)__builtin_amdgcn_readlane((int)lay_info, (m + 1 < nof_layers) ? m + 1 : 0);
        auto              next = [&]() { load_part_edges<PARTS>(pn, edges_g, lin, part); };
        const pk_exchange<decltype(next)> x = {xch, part, nth, lr < H, next};
        uint32_t* cl = c2v_lane + 64 * (li >> 16);
        if (it == 0 || (it == 1 && m == 0)) // (the latency form keeps the general first-visit instance for layers 1 and 2)
          update_rows_pk_split<true, PARTS>(pe, soft, cl, lr, Hv, Zv, x);
        else
          update_rows_pk_split<false, PARTS>(pe, soft, cl, lr, Hv, Zv, x);
        pe = pn;
      } else if constexpr (!RSKIP) {
        if (ATAB) {
          if (tid < H)
            update_rows_pk_visit_tab<PK_ATAB_DEGREE>(it, m, soft, c2v_lane + 64 * (li >> 16),
                                                     pk_adr_table{anx, {atab.rsrc, (uint32_t)__builtin_amdgcn_readfirstlane((m + 1 < nof_layers) ? m + 1 : 0) * alayer},
                                                                  16u * (uint32_t)tid, astride});
        } else if (tid < H) { // (<FUSED>: the address form of pk_edge_addresses that adds the column offset in the split pays in the 168-register instances only)
          if (GMSG && (int)(li >> 16) >= pairs_lds) { // this layer's messages live in global memory (separate code: the address space is part of the instruction)
            update_rows_pk_visit<FUSED>(it, m, d, soft, c2v_glob + 64 * (li >> 16), pk_adr_computed{edges, tid, Hv, Zv, 0});
          } else {
            update_rows_pk_visit<FUSED>(it, m, d, soft, c2v_lane + 64 * (li >> 16), pk_adr_computed{edges, tid, Hv, Zv, 0});
          }
        }
      } else if (!((sat_layers >> m) & 1u)) { // RSKIP (a set bit: saturated rows, the visit changes nothing anybody reads)
        bool all_inf = false; // this lane's rows wrote infinite soft bits only
        if (ATAB) {
          // the addresses of the next visit that RUNS: the next layer in turn whose bit is clear (the next one, and layer 0 behind the last, while no bit is set)
          const uint64_t live = ~sat_layers & (((uint64_t)1 << nof_layers) - 1u), above = live & ~(((uint64_t)2 << m) - 1u);
          const int      mn   = __builtin_amdgcn_readfirstlane(above ? __builtin_ctzll(above) : __builtin_ctzll(live));
          if (tid < H)
            all_inf = update_rows_pk_visit_tab<PK_ATAB_DEGREE, true>(it, m, soft, c2v_lane + 64 * (li >> 16),
                                                                     pk_adr_table{anx, {atab.rsrc, (uint32_t)mn * alayer}, 16u * (uint32_t)tid, astride});
        } else if (tid < H) {
          if (GMSG && (int)(li >> 16) >= pairs_lds) {
            all_inf = update_rows_pk_visit<FUSED, true>(it, m, d, soft, c2v_glob + 64 * (li >> 16), pk_adr_computed{edges, tid, Hv, Zv, 0});
          } else {
            all_inf = update_rows_pk_visit<FUSED, true>(it, m, d, soft, c2v_lane + 64 * (li >> 16), pk_adr_computed{edges, tid, Hv, Zv, 0});
          }
        }
        // one ballot over the lanes that own rows (a lane of a partial last wavefront that owns none does not count against it)
        if (__builtin_amdgcn_ballot_w64(tid < H && !all_inf) == 0)
          sat_layers |= (uint64_t)1 << m;
      }
      PROF_T(p_l1);
      __syncthreads();
      PROF_T(p_l2);
      PROF_ADD(1, p_l0, p_l1);
      PROF_ADD(2, p_l1, p_l2);
    }
    if (use_crc && !final_only) {
      if (zi >= 0 ? block_crc_is_zero<KEEPW>(soft, tab, zi, (int)order, L, K, kept, red, tid, nt) : block_crc(soft, tab, dsc.crc_poly, poly, order, K, L, red, tid, nt) == 0) {
        result_iters = it + 1;
        break;
      }
    }
  }
  PROF_T(p_dec);
  __builtin_amdgcn_s_setprio(LDPC_PK_SETPRIO_OUT);
  if (FUSED) {
    // The input of this workgroup's next codeblock is requested now: the loads fly while the CRC and the hard decision run, and
    // the registers that hold them are not live inside the layer loop.
    prefetch(red[15]);
  }
  if (final_only)
    result_iters = (zi >= 0 ? block_crc_is_zero<KEEPW>(soft, tab, zi, (int)order, L, K, kept, red, tid, nt) : block_crc(soft, tab, dsc.crc_poly, poly, order, K, L, red, tid, nt) == 0)
                       ? max_iter
                       : 0;
  PROF_T(p_crc);
  PROF_ADD(3, p_dec, p_crc);

  // A mask-table checksum has decided this lane's words of the output: its last evaluation is the one after the last layer visit.
  if (KEEPW && zi >= 0 && (final_only || max_iter > 0))
    store_kept_words(soft, out, K, tid, nt, kept);
  else
    store_hard_words(soft, out, K, tid, nt);
  if (tid == 0) {
    iters_out[cb] = result_iters;
    // A codeblock that is dematched here is a first transmission: its flag is written either way, which is the reset the caller
    // would otherwise launch before the decoder (pusch_decoder_impl.cpp:146-149).
    if (harq_crc_ok && (FUSED || result_iters > 0))
      harq_crc_ok[harq_slot[cb]] = result_iters > 0;
  }
  PROF_T(p_end);
  PROF_ADD(4, p_crc, p_end);
  PROF_ADD(5, p_start, p_end);
  PROF_COUNT();
  q = red[15];
  } // codeblock loop
}

// The instances of the kernel that exist, by what selects them. A row comes from ONE set of template arguments, so a key cannot name another
// instance's kernel; miphy_ldpc_pk_launch takes the row that matches its launch exactly.
struct pk_instance_key {
  bool fused, gmsg;
  int  parts;
  bool atab, row_skip;
  constexpr bool operator==(const pk_instance_key& o) const { return fused == o.fused && gmsg == o.gmsg && parts == o.parts && atab == o.atab && row_skip == o.row_skip; }
};
typedef decltype(&ldpc_decode_pk_kernel<false, false>) pk_kernel_fn;
struct pk_instance {
  pk_instance_key key;
  pk_kernel_fn    kernel;
};
template <bool FUSED, bool GMSG, int PARTS = 1, bool ATAB = false, bool RSKIP = false>
constexpr pk_instance pk_instance_of()
{
  return {{FUSED, GMSG, PARTS, ATAB, RSKIP}, ldpc_decode_pk_kernel<FUSED, GMSG, PARTS, ATAB, RSKIP>};
}
constexpr pk_instance pk_instances[] = {
    pk_instance_of<false, false>(),        pk_instance_of<false, true>(),         pk_instance_of<true, false>(),         pk_instance_of<true, true>(),
    pk_instance_of<false, false, 2>(),     pk_instance_of<true, false, 2>(),      pk_instance_of<false, false, 4>(),     pk_instance_of<true, false, 4>(),
    pk_instance_of<true, false, 1, true>(), pk_instance_of<false, false, 1, false, true>(), pk_instance_of<true, false, 1, false, true>(),
    pk_instance_of<true, false, 1, true, true>(),
};

} // namespace

#ifdef LDPC_PK_PROFILE
extern "C" int miphy_debug_ldpc_profile(unsigned long long out[8], int reset)
{
  static unsigned long long h[2048 * 8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ldpc_prof), sizeof(h)) != hipSuccess)
    return -1;
  for (int q = 0; q < 8; ++q) {
    out[q] = 0;
    for (int b = 0; b < 2048; ++b)
      out[q] += h[b * 8 + q];
  }
  if (reset) {
    for (auto& v : h)
      v = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ldpc_prof), h, sizeof(h)) != hipSuccess)
      return -1;
  }
  return 0;
}
#endif

#ifdef LDPC_PK_PROFILE2
extern "C" int miphy_debug_ldpc_profile2(unsigned long long out[8], int reset)
{
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ldpc_prof2), 8 * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  if (reset) {
    unsigned long long z[8] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_ldpc_prof2), z, sizeof(z)) != hipSuccess)
      return -1;
  }
  return 0;
}
#endif

int miphy_ldpc_pk_waves_per_cu(bool fused, int parts)
{
#ifdef LDPC_PK_REPORT_WAVES_FUSED // A-B: the register allocation of one occupancy run at another
  if (fused && parts <= 1)
    return 4 * LDPC_PK_REPORT_WAVES_FUSED;
#endif
  return 4 * (parts > 1 ? LDPC_PK_MIN_WAVES_SPLIT : (fused ? LDPC_PK_MIN_WAVES_FUSED : LDPC_PK_MIN_WAVES_PLAIN)); // what __launch_bounds__ of the kernel guarantees per CU
}

// LDS bytes the packed kernel needs for a given geometry (Zt >= Z of every codeblock, lay = layer bound, pairs_all = message
// dwords per lane of those layers).
size_t miphy_ldpc_pk_lds_bytes(int bgi, int lay, size_t Zt, int pairs_all, int parts)
{
  const size_t waves = ((Zt + 1) / 2 + 63) / 64;
  return (size_t)miphy_ldpc_soft_bytes(bgi, lay, (int)Zt) + waves * (size_t)pairs_all * 256 + 64 + (parts > 1 ? (size_t)parts * 3 * 64 * waves * 4 : 0);
}

// Resident workgroups per CU: LDS, the wavefronts per CU the register budget of the kernel allows (__launch_bounds__; at most the 32 slots).
int miphy_ldpc_pk_per_cu(size_t lds, int waves, bool fused, int parts)
{
  return std::max(1, std::min((int)((size_t)160 * 1024 / lds), miphy_ldpc_pk_waves_per_cu(fused, parts) / waves));
}

uint32_t miphy_ldpc_pk_grid(const miphy_ctx* ctx, uint32_t n, int threads, size_t lds, bool fused, int parts)
{
  // (threads = those of the launch: the latency form counts every part)
  return std::min<uint32_t>(n, (uint32_t)(ctx->num_cus * miphy_ldpc_pk_per_cu(lds, threads / 64, fused, parts)));
}

int miphy_ldpc_pk_launch(miphy_ctx* ctx, const miphy_ldpc_launch& L, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order, const int8_t* llr,
                         uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot, uint8_t* harq_crc_ok, const miphy_ldpc_rdm_desc* d_rdm,
                         const int8_t* rm_in, void* gmsg, hipStream_t s)
{
  // (the geometry is the launch table's: L.threads counts every part of the latency form, whose L.lds holds the exchange slots)
  const bool fused = (L.used & MIPHY_LDPC_KERNEL_FUSED) != 0, gm = L.gmsg_pairs > 0;
  MIPHY_REQUIRE(L.threads <= 1024, "ldpc_decode: workgroup of %d threads", L.threads);
  const pk_instance_key want = {fused, gm, L.parts, L.adr_by_z != nullptr, L.row_skip};
  pk_kernel_fn          kern = nullptr;
  for (const pk_instance& i : pk_instances)
    if (i.key == want)
      kern = i.kernel;
  MIPHY_REQUIRE(kern, "ldpc_decode: no packed kernel instance {fused %d, global messages %d, parts %d, address table %d, row skip %d}", want.fused, want.gmsg, want.parts,
                want.atab, want.row_skip);
  // Above the default 64 KB of dynamic LDS the limit has to be raised; it is a per-device attribute of the kernel, so it is set on
  // every such launch (a cache per thread would be wrong for a thread that drives several devices).
  if (L.lds > 48 * 1024) {
    MIPHY_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
  }
  uint32_t* queue = nullptr;
  int       rc    = miphy_next_queue_counter(ctx, &queue);
  if (rc)
    return rc;
  hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, s, d_descs, ctx->d_tables, llr, out_bits, iters, L.nodes, harq_slot, harq_crc_ok, L.c.count, queue, d_rdm,
                     rm_in, (uint32_t*)gmsg, L.gmsg_pairs, gm ? L.lds_pairs : 0, d_order, (const pk_adr_quad* const*)L.adr_by_z);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
