// LDPC decoder, one-row-per-lane variant -- layered normalised min-sum on int8 LLRs, one workgroup per codeblock. The kernel of the
// A-B knob and of batches whose geometry leaves the packed kernel (ldpc_decode_pk.hip) one small workgroup per CU.
//
// Behaviour contract: srsran::ldpc_decoder_impl::decode (lib/phy/upper/channel_coding/ldpc/ldpc_decoder_impl.cpp:60-146)
// with the arithmetic of the AVX2 hooks (ldpc_decoder_avx2.cpp:66-243, avx2_support.h:65-106).
//
// MI355X mapping (not a translation of the CPU data flow):
//   * thread i of the workgroup owns lifted check row i of every layer; a cyclic shift is an LDS address rotation,
//     so no data is ever moved to "rotate" a node;
//   * the soft bits of the whole codeblock (<= 68*384 B) live in LDS for the lifetime of the decode;
//   * check-to-variable messages are NOT stored: a check row's messages are fully determined by
//     (scaled min1, scaled min2, argmin, per-edge sign), which is packed in one 32-bit word per (layer,row)
//     (two words for the four degree-19 rows of BG1) -- exact, not an approximation;
//   * the v2c values of a row stay in registers between the min search and the soft-bit update (the per-degree
//     template makes every index static);
//   * hard decision + CRC run in-kernel: each lane reduces one 32-bit word of the message to a partial remainder,
//     multiplies it by x^(32k) mod P and the partial remainders are XOR-reduced with wavefront shuffles.
#include "miphy_internal.h"
#include "ldpc_frame_device.h"

namespace {

// State word layout: [6:0] scaled min1, [13:7] scaled min2, [18:14] argmin edge, [31:19] c2v sign of edges 0..12.
// Second word (degree > 13 only): c2v sign of edges 13...
//
// Inside a row update an infinite LLR (|x| > 120, i.e. +-127 in memory) is carried as +-INF_INT so that the
// promotion rules of the reference (ldpc_decoder_avx2.cpp:85-105,205-243: "infinity is sticky", "|sum| > 120 becomes
// infinity") collapse into one clamp: c2v magnitudes are <= 95, so INF_INT + c2v always stays beyond +-120.
constexpr int INF_INT = 255;

template <int D, bool FIRST>
__device__ __forceinline__ void
update_row(int8_t* __restrict__ soft, uint32_t& w0, uint32_t& w1, const uint32_t* __restrict__ edges, int i, int Z)
{
  int v2c[D];
  int addr[D];
  int mag1 = LLR_MAX, mag2 = LLR_MAX; // running min / second min of |v2c|
  int spx  = 0;                       // XOR of all v2c values: bit 31 = sign product
  const int      old_m1  = w0 & 127;
  const int      old_m2  = (w0 >> 7) & 127;
  const int      old_arg = (w0 >> 14) & 31;
  const uint32_t old_sgn = (w0 >> 19) | (D > 13 ? (w1 << 13) : 0u);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const uint32_t e   = edges[j];
    uint32_t       pos = (uint32_t)i + (e >> 16);
    pos                = min(pos, pos - (uint32_t)Z); // (i + shift) mod Z
    const int a        = (int)((e & 0xffffu) + pos);
    addr[j]            = a;
    const int s        = soft[a];
    int       v;
    if (FIRST) {
      v = s; // first visit of the layer: plain copy (ldpc_decoder_impl.cpp:181-185)
    } else {
      const int mag   = (old_arg == j) ? old_m2 : old_m1;
      const int smask = (int)__builtin_amdgcn_sbfe((int)old_sgn, j, 1); // 0 or -1
      const int c     = (mag ^ smask) - smask;
      v               = min(max(s - c, -LLR_MAX), LLR_MAX); // ldpc_decoder_avx2.cpp:85-92
    }
    // |s| > 120 <=> infinite soft bit: the message is infinite with the same sign (avx2.cpp:94-104).
    const bool inf = (uint32_t)(s + LLR_MAX) > (uint32_t)(2 * LLR_MAX);
    v              = inf ? ((s >> 31) ^ INF_INT) : v;
    v2c[j]         = v;
    spx ^= v;
    const int av   = max(v, -v);
    const int help = max(mag1, av); // strict "<" tie rule is value-equivalent: ties make min1 == min2
    mag1           = min(mag1, av);
    mag2           = min(mag2, help);
  }
  // Scaling by 0.8: floor(x * 52428 / 65536) (avx2_support.h:65-106).
  const int s1    = (mag1 * 52428) >> 16;
  const int s2    = (mag2 * 52428) >> 16;
  const int spm   = spx & (int)0x80000000;
  int       arg   = 0;
  uint32_t  cs    = 0;
#pragma unroll
  for (int j = D - 1; j >= 0; --j) {
    const int  v     = v2c[j];
    const bool ismin = max(v, -v) == mag1;
    const int  mag   = ismin ? s2 : s1;
    arg              = ismin ? j : arg;
    const int smask  = (v ^ spm) >> 31; // sign of the product of all other messages
    const int c      = (mag ^ smask) - smask;
    cs |= (uint32_t)(smask & 1) << j;
    const int r   = min(max(c + v, -LLR_INF), LLR_INF); // avx2.cpp:205-243 in the +-INF_INT encoding
    soft[addr[j]] = (int8_t)r;
  }
  w0 = (uint32_t)s1 | ((uint32_t)s2 << 7) | ((uint32_t)arg << 14) | (cs << 19);
  if (D > 13)
    w1 = cs >> 13;
}

template <bool FIRST>
__device__ __forceinline__ void update_row_any(int            d,
                                               int8_t*        soft,
                                               uint32_t&      w0,
                                               uint32_t&      w1,
                                               const uint32_t* edges,
                                               int            i,
                                               int            Z)
{
  switch (d) {
    case 19:
      update_row<19, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 10:
      update_row<10, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 9:
      update_row<9, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 8:
      update_row<8, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 7:
      update_row<7, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 6:
      update_row<6, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 5:
      update_row<5, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    case 4:
      update_row<4, FIRST>(soft, w0, w1, edges, i, Z);
      break;
    default:
      update_row<3, FIRST>(soft, w0, w1, edges, i, Z);
      break;
  }
}

#ifndef LDPC_MIN_WAVES
#define LDPC_MIN_WAVES 1
#endif
__global__ void __launch_bounds__(MIPHY_MAX_Z, LDPC_MIN_WAVES)
ldpc_decode_kernel(const miphy_ldpc_dec_desc* __restrict__ descs,
                   const miphy_graph_tables* __restrict__ tab,
                   const int8_t* __restrict__ llr_base,
                   uint8_t* __restrict__ out_base,
                   int32_t* __restrict__ iters_out,
                   int max_nodes, // host bound on ceil((in_len + 2Z) / Z) over the batch
                   const uint32_t* __restrict__ harq_slot, // optional: per-descriptor codeblock slot in harq_crc_ok
                   uint8_t* __restrict__ harq_crc_ok,      // optional: skip codeblocks already decoded, flag new successes
                   const uint32_t* __restrict__ cb_order)     // optional: workgroup b decodes codeblock order[b] of the arrays
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t            cbx = cb_order ? cb_order[blockIdx.x] : blockIdx.x;
  const miphy_ldpc_dec_desc dsc = descs[cbx];
  const int                 tid = threadIdx.x;
  const int                 nt  = blockDim.x;
  const int                 Z   = dsc.Z;
  const int                 bgi = (dsc.bg == 1) ? 0 : 1;
  const int                 K   = miphy_bg_K(bgi) * Z;
  const int                 zp  = tab->z_pos[Z];

  int8_t*   soft = reinterpret_cast<int8_t*>(smem);
  const int lay_alloc  = miphy_ldpc_layers(bgi, max_nodes);
  const int soft_bytes = miphy_ldpc_soft_bytes(bgi, lay_alloc, Z);
  // Check-row state is only allocated for the layers this launch can reach (host-side bound from in_len).
  uint32_t* st0  = reinterpret_cast<uint32_t*>(smem + soft_bytes);
  uint32_t* st1  = st0 + lay_alloc * Z;
  uint32_t* red  = st1 + 4 * Z; // 16 words of scratch

  const int8_t* llr = llr_base + dsc.llr_offset;
  uint8_t*      out = out_base + dsc.out_offset;
  const int     in_len = (int)dsc.in_len;

  if (harq_crc_ok && harq_crc_ok[harq_slot[cbx]]) { // pusch_decoder_impl.cpp:184: CRC already OK, keep the message
    if (tid == 0)
      iters_out[cbx] = -1;
    return;
  }
  if (tid < 16)
    red[tid] = 0;
  // Stage LLRs into LDS (variable nodes 0,1 are punctured -> 0) and find the last non-zero input.
  int last = cb_plain_load(soft, llr, in_len, Z, soft_bytes, tid, nt);
  atomicMax(reinterpret_cast<int*>(&red[0]), last);
  __syncthreads();
  last = (int)red[0];

  const bool use_crc = dsc.crc_poly != MIPHY_CRC_NONE;

  if (last == 0) { // ldpc_decoder_impl.cpp:88-94
    if (!use_crc)
      store_all_ones(out, K, tid, nt);
    if (tid == 0)
      iters_out[cbx] = 0;
    return;
  }

  const int nof_layers = cb_nof_layers(last, Z, bgi);

  const uint32_t* edges_g   = tab->edge[bgi][zp];
  const uint16_t* row_start = tab->row_start[bgi];

  // CRC constants. The checksum is the division form for every polynomial: K / 32 < Z <= nt, so a lane divides one word at most.
  uint32_t poly = 0, order = 0;
  int      L = 0;
  if (use_crc) {
    poly  = tab->crc_poly[dsc.crc_poly];
    order = tab->crc_order[dsc.crc_poly];
    L     = K - dsc.nof_filler_bits; // ldpc_decoder_impl.cpp:55
  }
  const bool final_only = use_crc && (dsc.flags & 1u);

  int result_iters = 0;
  const int max_iter = dsc.max_iter;
  for (int it = 0; it < max_iter; ++it) {
    for (int m = 0; m < nof_layers; ++m) {
      const int       e0    = row_start[m];
      const int       d     = row_start[m + 1] - e0;
      const uint32_t* edges = edges_g + e0;
      if (tid < Z) {
        uint32_t w0 = 0, w1 = 0;
        if (it == 0) {
          update_row_any<true>(d, soft, w0, w1, edges, tid, Z);
        } else {
          w0 = st0[m * Z + tid];
          if (d > 13)
            w1 = st1[m * Z + tid];
          update_row_any<false>(d, soft, w0, w1, edges, tid, Z);
        }
        st0[m * Z + tid] = w0;
        if (d > 13)
          st1[m * Z + tid] = w1;
      }
      __syncthreads();
    }
    if (use_crc && !final_only) { // ldpc_decoder_impl.cpp:126-133
      if (block_xor(crc_div_partial(soft, tab, dsc.crc_poly, poly, order, K, L, tid, nt), red, tid, nt) == 0) {
        result_iters = it + 1;
        break;
      }
    }
  }
  if (final_only) // pusch_decoder_impl.cpp:105-118: decode without early stop, then check the CRC once
    result_iters = (block_xor(crc_div_partial(soft, tab, dsc.crc_poly, poly, order, K, L, tid, nt), red, tid, nt) == 0) ? max_iter : 0;

  // Final hard bits (identical to what the reference leaves in `output`: the bits of the last iteration run).
  store_hard_words(soft, out, K, tid, nt);
  if (tid == 0) {
    iters_out[cbx] = result_iters;
    if (harq_crc_ok && result_iters > 0)
      harq_crc_ok[harq_slot[cbx]] = 1;
  }
}

} // namespace

// LDS bytes of a workgroup of `threads` (>= Z of every codeblock) lanes whose codeblocks reach `lay` layers: soft bits, one state word per
// (layer, row) + the second word of the four degree-19 rows, 16 reduction words. The kernel carves the same block up from its node bound.
size_t miphy_ldpc_row_lds_bytes(int bgi, int lay, size_t threads)
{
  return (size_t)miphy_ldpc_soft_bytes(bgi, lay, (int)threads) + (size_t)(lay + 4) * threads * 4 + 64;
}

void miphy_ldpc_row_geometry(miphy_ldpc_launch& L)
{
  const miphy_ldpc_class& c   = L.c;
  L.used    = MIPHY_LDPC_KERNEL_SCALAR;
  L.threads = ((c.max_Z + 63) / 64) * 64;
  L.nodes   = miphy_bg_K(c.bgi) + c.lay;
  L.lds     = miphy_ldpc_row_lds_bytes(c.bgi, c.lay, (size_t)L.threads);
  L.grid    = c.count;
}

int miphy_ldpc_row_launch(miphy_ctx* ctx, const miphy_ldpc_launch& L, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order, const int8_t* llr,
                          uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot, uint8_t* harq_crc_ok, hipStream_t s)
{
  // Above the default 64 KB of dynamic LDS the limit has to be raised; it is a per-device attribute of the kernel, so it is set on
  // every such launch (a cache per thread would be wrong for a thread that drives several devices).
  if (L.lds > 48 * 1024)
    MIPHY_HIP_CHECK(hipFuncSetAttribute((const void*)ldpc_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
  hipLaunchKernelGGL(ldpc_decode_kernel, dim3(L.grid), dim3(L.threads), L.lds, s, d_descs, ctx->d_tables, llr, out_bits, iters, L.nodes, harq_slot,
                     harq_crc_ok, d_order);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
