// Polar coding chains (PDCCH / PBCH / UCI): code construction on the host, one wavefront per codeword on the device.
//
// Behaviour contract (all under lib/phy/upper/channel_coding/polar/): polar_code_impl.cpp:325-490 (sets, n, nPC),
// polar_allocator_impl.cpp:28-70, polar_encoder_impl.cpp:32-86, polar_rate_matcher_impl.cpp:31-106,
// polar_rate_dematcher_impl.cpp:29-118, polar_decoder_impl.cpp:32-350 (simplified successive cancellation),
// polar_deallocator_impl.cpp:27-42, polar_interleaver_impl.cpp:27-56; PDCCH: channel_processors/pdcch_encoder_impl.cpp:33-98.
//
// MI355X mapping: the decoding tree only depends on the frozen set, so the host flattens the recursion into a pruned
// schedule (f / g / rate-1 / combine ops); a 64-lane wavefront executes it with all LLR stages, partial sums and
// decisions resident in LDS (2N + 2N bytes per codeword). Rate matching and its inverse are single gathers through
// host-composed index tables (sub-block interleaver o bit selection o channel interleaver).
#include "crc_device.h"
#include "miphy_ext.h"
#include "polar_device.h"

namespace {

template <typename T>
int upload(miphy_ctx* ctx, const std::vector<T>& v, T** d)
{
  return miphy_keep_device_copy(ctx, v.data(), v.size(), d);
}

int get_plan(miphy_ctx* ctx, const miphy_polar_code* c, const polar_plan** out)
{
  auto key = std::make_tuple(c->K, c->E, c->nMax, c->ibil ? 1u : 0u);
  auto it  = ctx->ext->polar_plans.find(key);
  if (it != ctx->ext->polar_plans.end()) {
    *out = &it->second;
    return MIPHY_OK;
  }
  polar_host_code h;
  int       rc = polar_build_code(c, h);
  if (rc)
    return rc;
  polar_host_tables t;
  polar_build_tables(h, c->ibil != 0, t);
  polar_plan p = {};
  p.K = h.K, p.E = h.E, p.n = h.n, p.N = h.N, p.nPC = h.nPC;
  p.sched_len = (uint32_t)t.sched.size();
  if ((rc = upload(ctx, t.info_pos, &p.d_info_pos)) || (rc = upload(ctx, t.is_pc, &p.d_is_pc)) || (rc = upload(ctx, t.tx_src, &p.d_tx_src)) ||
      (rc = upload(ctx, t.rx_first, &p.d_rx_first)) || (rc = upload(ctx, t.rx_fidx, &p.d_rx_fidx)) || (rc = upload(ctx, t.sched, &p.d_sched)) ||
      (rc = upload(ctx, t.pi_il, &p.d_pi_il)))
    return rc;
  auto ins = ctx->ext->polar_plans.emplace(key, p);
  *out     = &ins.first->second;
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- device side
__device__ __forceinline__ void polar_transform_lds(uint8_t* x, int n, int lane)
{ // polar_encoder_impl.cpp:32-52: x[i] ^= x[i + half] for every level, natural order.
  const int N = 1 << n;
  for (int half = 1; half < N; half <<= 1) {
    for (int t = lane; t < N / 2; t += 64) {
      const int b = ((t / half) * 2 * half) + (t % half);
      x[b] ^= x[b + half];
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void polar_tx_chain(const polar_plan& p, uint8_t* u, const uint8_t* msg_lds, uint8_t* __restrict__ out,
                                               uint8_t* __restrict__ alloc_tap, uint8_t* __restrict__ enc_tap, int lane)
{
  const int N = (int)p.N, KP = (int)(p.K + p.nPC);
  for (int i = lane; i < N; i += 64)
    u[i] = 0;
  __syncthreads();
  if (p.nPC == 0) { // polar_allocator_impl.cpp:37-41
    for (int i = lane; i < KP; i += 64)
      u[p.d_info_pos[i]] = msg_lds[i];
  } else if (lane == 0) { // :42-68, five-stage cyclic shift register, inherently serial and only used for K <= 25
    unsigned y[5] = {0, 0, 0, 0, 0};
    int      iK = 0, ip = 0;
    for (int q = 0; q < N; ++q) {
      const unsigned t = y[0];
      y[0] = y[1], y[1] = y[2], y[2] = y[3], y[3] = y[4], y[4] = t;
      if (ip < KP && p.d_info_pos[ip] == q) {
        if (p.d_is_pc[ip]) {
          u[q] = (uint8_t)y[0];
        } else {
          u[q] = msg_lds[iK];
          y[0] ^= msg_lds[iK];
          ++iK;
        }
        ++ip;
      }
    }
  }
  __syncthreads();
  if (alloc_tap)
    for (int i = lane; i < N; i += 64)
      alloc_tap[i] = u[i];
  polar_transform_lds(u, (int)p.n, lane);
  if (enc_tap)
    for (int i = lane; i < N; i += 64)
      enc_tap[i] = u[i];
  for (int o = lane; o < (int)p.E; o += 64) // sub-block interleaver, bit selection, channel interleaver: one gather
    out[o] = u[p.d_tx_src[o]];
}

__global__ void __launch_bounds__(64) polar_encode_kernel(polar_plan p, const uint8_t* __restrict__ msg, uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ alloc_tap, uint8_t* __restrict__ enc_tap)
{
  __shared__ uint8_t u[1024];
  __shared__ uint8_t m[1024];
  const int          lane = threadIdx.x;
  const size_t       cw   = blockIdx.x;
  for (int i = lane; i < (int)p.K; i += 64)
    m[i] = msg[cw * p.K + i];
  __syncthreads();
  polar_tx_chain(p, u, m, out + cw * p.E, alloc_tap ? alloc_tap + cw * p.N : nullptr, enc_tap ? enc_tap + cw * p.N : nullptr, lane);
}

// PDCCH (ones = 24 leading ones, RNTI mask) and PBCH (ones = 0, rnti == nullptr) share the CRC24C + interleave + polar chain.
__global__ void __launch_bounds__(64) pdcch_encode_kernel(polar_plan p, uint32_t A, const uint8_t* __restrict__ payload,
                                                          const uint16_t* __restrict__ rnti, uint8_t* __restrict__ out, int ones)
{
  __shared__ uint8_t u[1024];
  __shared__ uint8_t c[24 + 164];
  __shared__ uint8_t cp[164];
  const int          lane = threadIdx.x;
  const size_t       cw   = blockIdx.x;
  const int          K    = (int)p.K;
  // pdcch_encoder_impl.cpp:33-59: 24 leading ones, payload, CRC24C, RNTI mask on the last 16 parity bits.
  for (int i = lane; i < 24 + (int)A; i += 64)
    c[i] = (i < 24) ? 1 : payload[cw * A + (i - 24)];
  __syncthreads();
  if (lane == 0) {
    uint32_t reg = 0;
    for (int i = 24 - ones; i < 24 + (int)A; ++i) {
      reg = (reg << 1) ^ ((uint32_t)(c[i] & 1u) << 24);
      reg ^= (reg & 0x1000000u) ? 0x1B2B117u : 0u;
    }
    const uint32_t r = rnti ? rnti[cw] : 0u;
    for (int i = 0; i < 24; ++i) {
      uint32_t b = (reg >> (23 - i)) & 1u;
      if (i >= 8)
        b ^= (r >> (15 - (i - 8))) & 1u;
      c[24 + A + i] = (uint8_t)b;
    }
  }
  __syncthreads();
  for (int k = lane; k < K; k += 64) // CRC interleaver (polar_interleaver_impl.cpp:37-56), tx direction
    cp[k] = c[24 + p.d_pi_il[k]];
  __syncthreads();
  polar_tx_chain(p, u, cp, out + cw * p.E, nullptr, nullptr, lane);
}

#ifndef POLAR_SSC_CW
#define POLAR_SSC_CW 4
#endif

// C codewords per wavefront, W = 64 / C lanes each. Every codeword of a batch has the same code, hence the same pruned schedule: the codewords of a
// wavefront run it in lockstep, each on its own LDS slice. One codeword per wavefront kept 23 % of the lanes busy (SQ_THREAD_CYCLES_VALU, profiles/r03):
// below stage 6 an operation is narrower than the wavefront, and the pruned schedule spends most of its operations there; with C codewords the narrow
// operations fill C times the lanes and every operation's fixed cost (schedule word, barrier) is shared by C codewords.
template <int C>
__global__ void __launch_bounds__(64) polar_decode_kernel(polar_plan p, uint32_t ncw, const int8_t* __restrict__ llr_in, uint8_t* __restrict__ msg_out,
                                                          int8_t* __restrict__ dem_tap, uint8_t* __restrict__ u_tap)
{
  constexpr int W = 64 / C;
  __shared__ int8_t  L_all[C][2048]; // stage s buffer at offset 2^s (size 2^s)
  __shared__ uint8_t est_all[C][1024];
  __shared__ uint8_t u_all[C][1024];
  const int          c = threadIdx.x / W, lane = threadIdx.x % W;
  const size_t       cw = (size_t)blockIdx.x * C + c;
  const bool         live = cw < ncw;
  int8_t*            L    = L_all[c];
  uint8_t*           est  = est_all[c];
  uint8_t*           u    = u_all[c];
  const int          N = (int)p.N, n = (int)p.n, E = (int)p.E;
  const int8_t*      f = llr_in + (live ? cw : 0) * p.E;
  // Rate dematching (polar_rate_dematcher_impl.cpp:29-118) as a gather: repetitions are accumulated in order.
  for (int q = lane; q < N; q += W) {
    const int v = polar_dematch_value(p.d_rx_first[q], N, E, f, p.d_rx_fidx);
    L[N + q] = (int8_t)v;
    est[q]   = 0;
    u[q]     = 0;
    if (dem_tap && live)
      dem_tap[cw * N + q] = (int8_t)v;
  }
  __syncthreads();
  polar_ssc_run<W>(L, est, u, p.d_sched, p.sched_len, lane);
  if (!live)
    return;
  if (u_tap)
    for (int i = lane; i < N; i += W)
      u_tap[cw * N + i] = u[i];
  // Deallocation (polar_deallocator_impl.cpp:27-42): K-set positions that are not parity checks, ascending.
  if (p.nPC == 0) {
    for (int i = lane; i < (int)p.K; i += W)
      msg_out[cw * p.K + i] = u[p.d_info_pos[i]];
  } else if (lane == 0) {
    int iK = 0;
    for (int i = 0; i < (int)(p.K + p.nPC); ++i)
      if (!p.d_is_pc[i])
        msg_out[cw * p.K + iK++] = u[p.d_info_pos[i]];
  }
  (void)n;
}


// ---- single blocks of the chain, for the block-level interfaces of the reference (polar_allocator / polar_encoder /
// polar_rate_matcher / polar_rate_dematcher / polar_decoder / polar_deallocator / polar_interleaver): the same device code as the
// chains above, entered and left at one stage. One wavefront per codeword.
__global__ void __launch_bounds__(64) polar_block_kernel(polar_plan p, int op, int param, const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                         const uint8_t* __restrict__ pi_il_max)
{
  __shared__ int8_t  L[2048];
  __shared__ uint8_t est[1024];
  __shared__ uint8_t u[1024];
  const int          lane = threadIdx.x;
  const size_t       cw   = blockIdx.x;
  const int          N = (int)p.N, E = (int)p.E, K = (int)p.K, KP = (int)(p.K + p.nPC);
  switch (op) {
    case MIPHY_POLAR_OP_ALLOCATE: { // polar_allocator_impl.cpp:28-70
      uint8_t* m = est;
      for (int i = lane; i < K; i += 64)
        m[i] = in[cw * K + i];
      for (int i = lane; i < N; i += 64)
        u[i] = 0;
      __syncthreads();
      if (p.nPC == 0) {
        for (int i = lane; i < KP; i += 64)
          u[p.d_info_pos[i]] = m[i];
      } else if (lane == 0) {
        unsigned y[5] = {0, 0, 0, 0, 0};
        int      iK = 0, ip = 0;
        for (int q = 0; q < N; ++q) {
          const unsigned t = y[0];
          y[0] = y[1], y[1] = y[2], y[2] = y[3], y[3] = y[4], y[4] = t;
          if (ip < KP && p.d_info_pos[ip] == q) {
            if (p.d_is_pc[ip]) {
              u[q] = (uint8_t)y[0];
            } else {
              u[q] = m[iK];
              y[0] ^= m[iK];
              ++iK;
            }
            ++ip;
          }
        }
      }
      __syncthreads();
      for (int i = lane; i < N; i += 64)
        out[cw * N + i] = u[i];
      break;
    }
    case MIPHY_POLAR_OP_ENCODE: { // polar_encoder_impl.cpp:32-86, param = log2 of the code size
      const int NN = 1 << param;
      for (int i = lane; i < NN; i += 64)
        u[i] = in[cw * NN + i];
      __syncthreads();
      polar_transform_lds(u, param, lane);
      for (int i = lane; i < NN; i += 64)
        out[cw * NN + i] = u[i];
      break;
    }
    case MIPHY_POLAR_OP_RATE_MATCH: // polar_rate_matcher_impl.cpp:31-106 as one gather
      for (int o = lane; o < E; o += 64)
        out[cw * E + o] = in[cw * N + p.d_tx_src[o]];
      break;
    case MIPHY_POLAR_OP_RATE_DEMATCH: { // polar_rate_dematcher_impl.cpp:29-118
      const int8_t* f = reinterpret_cast<const int8_t*>(in) + cw * E;
      for (int q = lane; q < N; q += 64) {
        const int v = polar_dematch_value(p.d_rx_first[q], N, E, f, p.d_rx_fidx);
        reinterpret_cast<int8_t*>(out)[cw * N + q] = (int8_t)v;
      }
      break;
    }
    case MIPHY_POLAR_OP_DECODE: { // polar_decoder_impl.cpp:179-350 (simplified successive cancellation), output in the u domain
      for (int q = lane; q < N; q += 64) {
        L[N + q] = reinterpret_cast<const int8_t*>(in)[cw * N + q];
        est[q]   = 0;
        u[q]     = 0;
      }
      __syncthreads();
      polar_ssc_run<64>(L, est, u, p.d_sched, p.sched_len, lane);
      for (int i = lane; i < N; i += 64)
        out[cw * N + i] = u[i];
      break;
    }
    case MIPHY_POLAR_OP_DEALLOCATE: // polar_deallocator_impl.cpp:27-42
      if (p.nPC == 0) {
        for (int i = lane; i < K; i += 64)
          out[cw * K + i] = in[cw * N + p.d_info_pos[i]];
      } else if (lane == 0) {
        int iK = 0;
        for (int i = 0; i < KP; ++i)
          if (!p.d_is_pc[i])
            out[cw * K + iK++] = in[cw * N + p.d_info_pos[i]];
      }
      break;
    default: { // MIPHY_POLAR_OP_INTERLEAVE_TX / _RX: polar_interleaver_impl.cpp:27-56, param = K
      const int KK = param;
      if (lane == 0) { // K <= 164: the selection of the pattern entries is a serial scan
        int k = 0;
        for (int m = 0; m < (int)NR_POLAR_K_MAX_IL; ++m)
          if ((int)pi_il_max[m] >= (int)NR_POLAR_K_MAX_IL - KK) {
            const int pi_k = (int)pi_il_max[m] - ((int)NR_POLAR_K_MAX_IL - KK);
            if (op == MIPHY_POLAR_OP_INTERLEAVE_TX)
              out[cw * KK + k] = in[cw * KK + pi_k];
            else
              out[cw * KK + pi_k] = in[cw * KK + k];
            ++k;
          }
      }
      break;
    }
  }
}

} // namespace

extern "C" int miphy_polar_code_info(const miphy_polar_code* code, uint32_t* n, uint32_t* N, uint32_t* nPC)
{
  if (!code) {
    miphy_set_error("miphy_polar_code_info: null argument");
    return MIPHY_EINVAL;
  }
  polar_host_code h;
  int       rc = polar_build_code(code, h);
  if (rc)
    return rc;
  if (n)
    *n = h.n;
  if (N)
    *N = h.N;
  if (nPC)
    *nPC = h.nPC;
  return MIPHY_OK;
}

extern "C" int miphy_polar_encode_batch(miphy_ctx*              ctx,
                                        const miphy_polar_code* code,
                                        uint32_t                n,
                                        const uint8_t*          msg,
                                        uint8_t*                rm_out,
                                        uint8_t*                allocated_tap,
                                        uint8_t*                encoded_tap,
                                        void*                   stream)
{
  MIPHY_REQUIRE(ctx && code && msg && rm_out, "miphy_polar_encode_batch: null argument");
  const polar_plan* p  = nullptr;
  int               rc = get_plan(ctx, code, &p);
  if (rc || n == 0)
    return rc;
  hipLaunchKernelGGL(polar_encode_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, *p, msg, rm_out, allocated_tap, encoded_tap);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_polar_decode_batch(miphy_ctx*              ctx,
                                        const miphy_polar_code* code,
                                        uint32_t                n,
                                        const int8_t*           llr,
                                        uint8_t*                msg_out,
                                        int8_t*                 dematched_tap,
                                        uint8_t*                decoded_u_tap,
                                        void*                   stream)
{
  MIPHY_REQUIRE(ctx && code && llr && msg_out, "miphy_polar_decode_batch: null argument");
  const polar_plan* p  = nullptr;
  int               rc = get_plan(ctx, code, &p);
  if (rc || n == 0)
    return rc;
  // Codewords per wavefront: four (16 lanes each) once the batch fills the chip several times over, fewer for small batches (a lone codeword
  // keeps the whole wavefront: its wide stages finish in fewer steps).
  const uint32_t per_chip = (uint32_t)ctx->num_cus * 8u;
  if (n >= 4u * per_chip)
    hipLaunchKernelGGL((polar_decode_kernel<POLAR_SSC_CW>), dim3((n + POLAR_SSC_CW - 1) / POLAR_SSC_CW), dim3(64), 0, (hipStream_t)stream, *p, n, llr, msg_out, dematched_tap, decoded_u_tap);
  else if (n >= 2u * per_chip)
    hipLaunchKernelGGL((polar_decode_kernel<2>), dim3((n + 1) / 2), dim3(64), 0, (hipStream_t)stream, *p, n, llr, msg_out, dematched_tap, decoded_u_tap);
  else
    hipLaunchKernelGGL((polar_decode_kernel<1>), dim3(n), dim3(64), 0, (hipStream_t)stream, *p, n, llr, msg_out, dematched_tap, decoded_u_tap);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_polar_block_batch(miphy_ctx* ctx, const miphy_polar_code* code, uint32_t op, uint32_t param, uint32_t n, const void* in, void* out,
                                       void* stream)
{
  MIPHY_REQUIRE(ctx && in && out, "miphy_polar_block_batch: null argument");
  MIPHY_REQUIRE(op <= MIPHY_POLAR_OP_INTERLEAVE_RX, "miphy_polar_block_batch: invalid operation %u", op);
  polar_plan        none = {};
  const polar_plan* p    = &none;
  const bool        needs_code = !(op == MIPHY_POLAR_OP_ENCODE || op == MIPHY_POLAR_OP_INTERLEAVE_TX || op == MIPHY_POLAR_OP_INTERLEAVE_RX);
  if (needs_code) {
    MIPHY_REQUIRE(code, "miphy_polar_block_batch: operation %u needs the code", op);
    int rc = get_plan(ctx, code, &p);
    if (rc)
      return rc;
  } else if (op == MIPHY_POLAR_OP_ENCODE) {
    MIPHY_REQUIRE(param >= 5 && param <= 10, "miphy_polar_block_batch: code size 2^%u out of range", param); // polar_code.h:52-61
  } else {
    MIPHY_REQUIRE(param >= 1 && param <= NR_POLAR_K_MAX_IL, "miphy_polar_block_batch: interleaver length %u out of range (K_MAX_IL = 164)", param);
  }
  if (n == 0)
    return MIPHY_OK;
  // the interleaver pattern (TS 38.212 Table 5.3.1.1-1) lives with the device tables of the context
  static_assert(sizeof(NR_POLAR_PI_IL_MAX[0]) == 1, "pattern entries are bytes");
  auto& ext = *ctx->ext;
  if (!ext.d_pi_il_max)
    if (int rc = miphy_keep_device_copy(ctx, NR_POLAR_PI_IL_MAX, NR_POLAR_K_MAX_IL, &ext.d_pi_il_max))
      return rc;
  hipLaunchKernelGGL(polar_block_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, *p, (int)op, (int)param, (const uint8_t*)in, (uint8_t*)out,
                     (const uint8_t*)ext.d_pi_il_max);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

extern "C" int miphy_pdcch_encode_batch(miphy_ctx*      ctx,
                                        uint32_t        A,
                                        uint32_t        E,
                                        uint32_t        n,
                                        const uint8_t*  payload,
                                        const uint16_t* rnti,
                                        uint8_t*        out,
                                        void*           stream)
{
  MIPHY_REQUIRE(ctx && payload && rnti && out, "miphy_pdcch_encode_batch: null argument");
  MIPHY_REQUIRE(A >= 12 && A <= 128, "pdcch_encode: payload size %u out of range (12..MAX_DCI_PAYLOAD_SIZE = 128)", A);
  miphy_polar_code  code = {A + 24, E, 9, 0};
  const polar_plan* p    = nullptr;
  int               rc   = get_plan(ctx, &code, &p);
  if (rc || n == 0)
    return rc;
  hipLaunchKernelGGL(pdcch_encode_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, *p, A, payload, rnti, out, 24);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// ---------------------------------------------------------------------------------------------------- SCL list decoder
namespace {

// One wavefront per codeword: rate dematching, the list recursion of polar_device.h (polar_scl_run, shared with uci_polar.hip; the LDS
// layout is stated there) and the selection among the survivors.
__global__ void __launch_bounds__(64) polar_scl_kernel(polar_plan p, int L, int crc_mode, const int8_t* __restrict__ llr_in,
                                                       const uint16_t* __restrict__ rnti, const uint8_t* __restrict__ k_set,
                                                       uint8_t* __restrict__ msg_out, uint8_t* __restrict__ crc_ok_out,
                                                       int32_t* __restrict__ metric_out)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int    lane = threadIdx.x;
  const size_t cw   = blockIdx.x;
  const int    N = (int)p.N, n = (int)p.n, E = (int)p.E, K = (int)p.K;
  int8_t*      ch     = reinterpret_cast<int8_t*>(smem);
  const int    PSZ    = 3 * N; // bytes per path
  uint8_t*     bankA  = smem + N;
  uint8_t*     bankB  = bankA + (size_t)L * PSZ;
  int*         pm     = reinterpret_cast<int*>(bankB + (size_t)L * PSZ); // [L]
  int*         sel    = pm + 8;                                           // parent[8], bit[8], pm[8]
  uint8_t*     kset   = reinterpret_cast<uint8_t*>(sel + 24);             // [N] information-set flags: one LDS read per leaf
                                                                          // instead of a dependent global load (~1.5 us each)
  const int8_t* f_in  = llr_in + cw * p.E;
  for (int q = lane; q < 2 * N; q += 64)
    kset[q] = k_set[q]; // [0, N): information-set flags, [N, 2N): rate-0 block exponents
  // Rate dematching (same gather as polar_decode_kernel).
  for (int q = lane; q < N; q += 64) {
    const int v = polar_dematch_value(p.d_rx_first[q], N, E, f_in, p.d_rx_fidx);
    ch[q] = (int8_t)v;
  }
  if (lane < 8)
    pm[lane] = 0;
  __syncthreads();
  uint8_t* P = bankA;
  uint8_t* Q = bankB;
  const int active = polar_scl_run(ch, P, Q, pm, sel, kset, N, n, L, lane);
  // ---- selection: extract the K bits of every path (into bank Q), optional de-interleave + CRC, best metric wins
  int      my_pm = 0x7fffffff, my_ok = 0;
  uint8_t* cand  = Q + (lane < 8 ? lane : 0) * PSZ;     // K bits at cand[0..K), K-set order at cand[N..N+K)
  if (lane < active) {
    const uint8_t* u  = P + lane * PSZ + 2 * N;
    int            iK = 0;
    for (int i = 0; i < (int)(p.K + p.nPC); ++i)
      if (!p.d_is_pc[i])
        cand[N + iK++] = u[p.d_info_pos[i]];
    my_pm = pm[lane];
    if (crc_mode == 0) {
      for (int k = 0; k < K; ++k)
        cand[k] = cand[N + k];
    } else {
      for (int k = 0; k < K; ++k) // polar_interleaver, rx direction: out[pi(k)] = in[k]
        cand[p.d_pi_il[k]] = cand[N + k];
      const int A    = K - 24;
      uint32_t  reg  = 0;
      const int ones = (crc_mode == 1) ? 24 : 0;
      for (int b = 0; b < ones + A; ++b) {
        const uint32_t bitv = (b < ones) ? 1u : cand[b - ones];
        reg                 = (reg << 1) ^ (bitv << 24);
        reg ^= (reg & 0x1000000u) ? 0x1B2B117u : 0u;
      }
      uint32_t rx = 0;
      for (int b = 0; b < 24; ++b)
        rx = (rx << 1) | cand[A + b];
      if (crc_mode == 1)
        rx ^= (uint32_t)rnti[cw];
      my_ok = (reg & 0xffffffu) == rx;
    }
  }
  // winner: smallest metric among CRC passes (if any), else smallest metric; ties -> lowest slot
  const unsigned long long okmask = __ballot(my_ok != 0);
  const bool               any_ok = okmask != 0ull;
  int                      key    = (lane < active && (!any_ok || my_ok)) ? my_pm : 0x7fffffff;
  int                      best   = key, best_lane = lane;
#pragma unroll
  for (int off = 4; off >= 1; off >>= 1) {
    const int ok = __shfl_xor(best, off), ol = __shfl_xor(best_lane, off);
    if (ok < best || (ok == best && ol < best_lane)) {
      best      = ok;
      best_lane = ol;
    }
  }
  best_lane = __shfl(best_lane, 0);
  best      = __shfl(best, 0);
  __syncthreads();
  const uint8_t* win = Q + best_lane * PSZ;
  for (int k = lane; k < K; k += 64)
    msg_out[cw * p.K + k] = win[k];
  if (lane == 0) {
    crc_ok_out[cw] = any_ok ? 1 : 0;
    if (metric_out)
      metric_out[cw] = best;
  }
}

} // namespace

extern "C" int miphy_polar_decode_list_batch(miphy_ctx*              ctx,
                                             const miphy_polar_code* code,
                                             uint32_t                list_size,
                                             uint32_t                crc_mode,
                                             uint32_t                n,
                                             const int8_t*           llr,
                                             const uint16_t*         rnti,
                                             uint8_t*                msg_out,
                                             uint8_t*                crc_ok_out,
                                             int32_t*                metric_out,
                                             void*                   stream)
{
  MIPHY_REQUIRE(ctx && code && llr && msg_out && crc_ok_out, "miphy_polar_decode_list_batch: null argument");
  MIPHY_REQUIRE(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "polar_decode_list: list size %u not in {1,2,4,8}", list_size);
  MIPHY_REQUIRE(crc_mode <= 2, "polar_decode_list: invalid crc_mode %u", crc_mode);
  MIPHY_REQUIRE(crc_mode != 1 || rnti, "polar_decode_list: PDCCH CRC mode needs the RNTI array");
  MIPHY_REQUIRE(crc_mode == 0 || (code->K > 24 && code->K <= 164), "polar_decode_list: CRC-aided modes need 24 < K <= 164");
  const polar_plan* p  = nullptr;
  int               rc = get_plan(ctx, code, &p);
  if (rc || n == 0)
    return rc;
  // K-set membership per position (frozen / information), uploaded once per plan.
  auto key = std::make_tuple(code->K, code->E, code->nMax, code->ibil ? 1u : 0u);
  auto it  = ctx->ext->polar_kset.find(key);
  if (it == ctx->ext->polar_kset.end()) {
    polar_host_code h;
    if ((rc = polar_build_code(code, h)))
      return rc;
    std::vector<uint8_t> tab;
    polar_build_list_flags(h, tab);
    uint8_t* d = nullptr;
    if ((rc = upload(ctx, tab, &d)))
      return rc;
    it = ctx->ext->polar_kset.emplace(key, d).first;
  }
  const size_t lds = polar_scl_lds_bytes(p->N, list_size);
  // Above the default 64 KB of dynamic LDS the limit has to be raised; it is a per-device attribute of the kernel, so it is set on
  // every such launch (a cache per thread would be wrong for a thread that drives several devices).
  if (lds > 48 * 1024) {
    MIPHY_HIP_CHECK(hipFuncSetAttribute((const void*)polar_scl_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(polar_scl_kernel, dim3(n), dim3(64), lds, (hipStream_t)stream, *p, (int)list_size, (int)crc_mode, llr, rnti, it->second, msg_out,
                     crc_ok_out, metric_out);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

namespace {
// TS 38.211 5.2.1 Gold sequence bit c(n) on the host (PBCH scrambling needs at most a few hundred bits).
void host_gold(uint32_t c_init, uint32_t offset, uint32_t nbits, uint8_t* out)
{
  const uint32_t       total = 1600 + offset + nbits + 31;
  std::vector<uint8_t> x1(total + 31, 0), x2(total + 31, 0);
  x1[0] = 1;
  for (int i = 0; i < 31; ++i)
    x2[i] = (c_init >> i) & 1u;
  for (uint32_t n = 0; n + 31 < total + 31; ++n) {
    x1[n + 31] = x1[n + 3] ^ x1[n];
    x2[n + 31] = x2[n + 3] ^ x2[n + 2] ^ x2[n + 1] ^ x2[n];
  }
  for (uint32_t n = 0; n < nbits; ++n)
    out[n] = x1[n + offset + 1600] ^ x2[n + offset + 1600];
}
} // namespace

extern "C" int miphy_pbch_encode_batch(miphy_ctx* ctx, const miphy_pbch_msg* msgs, uint32_t n, uint8_t* out, void* stream)
{
  MIPHY_REQUIRE(ctx && msgs && out, "miphy_pbch_encode_batch: null argument");
  if (n == 0)
    return MIPHY_OK;
  // TS 38.212 Table 7.1.1-1, payload interleaver pattern G(j) (pbch_encoder_impl.cpp:33-35).
  static const uint8_t G[32] = {16, 23, 18, 17, 8, 30, 10, 6, 24, 7, 0, 5, 3, 2, 1, 4, 9, 11, 12, 13, 14, 15, 19, 20, 21, 22, 25, 26, 27, 28, 29, 31};
  std::vector<uint8_t> ap((size_t)n * 32);
  for (uint32_t m = 0; m < n; ++m) {
    const miphy_pbch_msg& msg = msgs[m];
    MIPHY_REQUIRE(msg.N_id <= 1007, "pbch_encode: message %u: invalid N_id %u", m, msg.N_id);
    MIPHY_REQUIRE(msg.L_max == 4 || msg.L_max == 8 || msg.L_max == 64, "pbch_encode: message %u: invalid L_max %u", m, msg.L_max);
    uint8_t a[32] = {0};
    // payload_generate (pbch_encoder_impl.cpp:42-86)
    uint32_t j_sfn = 0, j_other = 14;
    for (uint32_t i = 0; i < 24; ++i) {
      if (i >= 1 && i < 7)
        a[G[j_sfn++]] = msg.payload[i] & 1u;
      else
        a[G[j_other++]] = msg.payload[i] & 1u;
    }
    a[G[j_sfn++]] = (msg.sfn >> 3) & 1u;
    a[G[j_sfn++]] = (msg.sfn >> 2) & 1u;
    a[G[j_sfn++]] = (msg.sfn >> 1) & 1u;
    a[G[j_sfn++]] = (msg.sfn >> 0) & 1u;
    a[G[10]]      = msg.hrf ? 1 : 0;
    if (msg.L_max == 64) {
      a[G[11]] = (msg.ssb_idx >> 5) & 1u;
      a[G[12]] = (msg.ssb_idx >> 4) & 1u;
      a[G[13]] = (msg.ssb_idx >> 3) & 1u;
    } else {
      a[G[11]] = (msg.k_ssb >> 4) & 1u;
      a[G[12]] = 0;
      a[G[13]] = 0;
    }
    // scramble (pbch_encoder_impl.cpp:88-129)
    const uint32_t M = (msg.L_max == 64) ? 32 - 6 : 32 - 3;
    const uint32_t v = 2 * a[G[7]] + a[G[8]]; // 3rd and 2nd LSB of the SFN
    uint8_t        c[32];
    host_gold(msg.N_id, M * v, 32, c);
    uint32_t j = 0;
    for (uint32_t i = 0; i < 32; ++i) {
      uint8_t    s_i        = c[j];
      const bool is_ssb_idx = (i == G[11] || i == G[12] || i == G[13]) && msg.L_max == 64;
      if (is_ssb_idx || i == G[10] || i == G[8] || i == G[7])
        s_i = 0;
      else
        ++j;
      ap[(size_t)m * 32 + i] = a[i] ^ s_i;
    }
  }
  miphy_polar_code  code = {56, 864, 9, 0};
  const polar_plan* p    = nullptr;
  int               rc   = get_plan(ctx, &code, &p);
  if (rc)
    return rc;
  hipStream_t s  = (hipStream_t)stream;
  void*       ws = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_GENERAL, ap.size(), &ws)))
    return rc;
  if ((rc = miphy_upload(ctx, ws, ap.data(), ap.size(), s))) // `ap` is a local buffer
    return rc;
  hipLaunchKernelGGL(pdcch_encode_kernel, dim3(n), dim3(64), 0, s, *p, 32u, (const uint8_t*)ws, (const uint16_t*)nullptr, out, 0);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
