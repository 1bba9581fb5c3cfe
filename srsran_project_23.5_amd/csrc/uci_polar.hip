// Polar-coded UCI fields of 12 to 1706 bits: the TS 38.212 framing of uci_polar_info.h around the reference's polar receive chain
// (polar_rate_dematcher_impl.cpp:29-118, polar_decoder_impl.cpp:32-350, polar_deallocator_impl.cpp:27-42: the device code of
// polar_decode_kernel in polar_device.h). The 23.5 reference decodes no such field; the tests pin this file to the oracle's polar
// chains composed with a restatement of the framing (tests/uci_polar.py).
//
// Every field of a call may have a code of its own, so nothing is cached on the device: the host constructs the codes of the call (a
// bounded host cache keeps recent ones), and the tasks and code tables travel with the call through the staging ring in pieces.
//
// Kernel: one workgroup per field, one wavefront per segment, each on its own LDS slice (4 KB). One- and two-segment fields go out in
// SEPARATE launches (64 and 128 threads): sizing every workgroup for two would park an idle wavefront and 4 KB of LDS with each of
// the one-segment fields, which are the common ones, and a one-wavefront workgroup needs no hardware barrier at all. The two segments
// of a field have the same (K_r, E_r), hence the same schedule: the two wavefronts run it in lockstep and every barrier of the
// schedule loop is uniform across the workgroup, the property polar_decode_kernel relies on for the codewords of a wavefront.
// CRC: the remainder of the K_r decoded bits (payload followed by the received CRC bits) is zero exactly when the CRC recomputed
// over the first K_r - L bits equals the last L; the lanes take ceil(K_r / 64) <= 16 consecutive bits each, weigh their chunk's
// remainder with x^(bits behind the chunk) mod g and the wavefront XORs the 64 parts (linearity), so no lane runs more than 16
// serial steps plus one square-and-multiply.
//
// CRC-aided list decoding (miphy_uci_polar_decode_list_batch, list sizes 2 / 4 / 8, fields of 20 bits and more): uci_polar_scl_kernel
// runs the list recursion of polar_device.h (polar_scl_run, the one polar_scl_kernel of polar.hip runs) on one SEGMENT per one-wave
// workgroup, so a task is a segment there, and picks among the survivors by CRC11. Its LDS grows with N and the list size (52.5 KB at
// N = 1024, L = 8): the list tasks of a piece are grouped by N and each group is a launch with its own dynamic LDS size. The verdict
// of a field needs no ordering between its segments: a fill launch sets the status of the piece's list-decoded fields to VALID, and
// a segment without a passing survivor stores INVALID over it.
#include "crc_device.h"
#include "miphy_ext.h"
#include "polar_device.h"
#include "uci_polar_info.h"
#include <atomic>
#include <cstring>
#include <map>

namespace {

// Header of a code block; the tables follow at the byte offsets it names (from the header, each a multiple of four).
struct uci_polar_code_hdr {
  uint32_t K, E, N, nPC, L, sched_len;
  uint32_t off_info_pos; // uint16 [K + nPC]: positions of the K-set, ascending
  uint32_t off_is_pc;    // uint8  [K + nPC]: 1 = parity-check position
  uint32_t off_rx_first; // int32  [N]
  uint32_t off_rx_fidx;  // uint16 [E]
  uint32_t off_sched;    // uint32 [sched_len]
  uint32_t off_list;     // uint8  [2 N]: information-set flags and rate-0 block exponents of the list recursion (polar_build_list_flags)
  uint32_t bytes;        // the whole block, a multiple of 16
};
struct uci_polar_task {
  uint32_t code_off; // byte offset of the field's code block in the piece
  uint32_t job;      // the field's status byte: status[job] (the index of the field in the call, or the caller's status_index of it)
  uint32_t seg, pad; // seg: the segment a task of the list kernel decodes (the SSC kernel's workgroup takes every segment of its field)
  uint64_t llr_offset, payload_offset;
};
static_assert(sizeof(uci_polar_code_hdr) == 52 && sizeof(uci_polar_task) == 32, "dword records");

constexpr size_t UCI_POLAR_PIECE_BYTES = 1u << 20; // tasks + code tables of one staging and one launch (pair), see include/miphy.h
constexpr size_t UCI_POLAR_PIECE_MAX   = 4u << 20; // a piece is one region of the 8 MiB ring
// Test hooks of the public header, process-wide like the other debug knobs: atomics, so calls on two contexts from two threads do not
// race; the piece count is the one of whichever call finished last.
std::atomic<size_t>   g_piece_bytes{0}; // 0 = default
std::atomic<unsigned> g_last_pieces{0};
std::atomic<unsigned> g_last_ssc_segments{0}, g_last_list_segments{0};

template <int C>
__global__ void __launch_bounds__(64 * C) uci_polar_decode_kernel(const uint8_t* __restrict__ piece, uint32_t first_task, const int8_t* __restrict__ llr,
                                                                  uint8_t* __restrict__ payload, uint8_t* __restrict__ status)
{
  __shared__ int8_t   L_all[C][2048]; // stage s buffer at offset 2^s (size 2^s)
  __shared__ uint8_t  est_all[C][1024];
  __shared__ uint8_t  u_all[C][1024];
  __shared__ uint32_t crc_rem[C];
  const int                seg = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uci_polar_task     t    = load_words(reinterpret_cast<const uci_polar_task*>(piece) + first_task + blockIdx.x);
  const uint8_t*           code = piece + t.code_off;
  const uci_polar_code_hdr h    = load_words(reinterpret_cast<const uci_polar_code_hdr*>(code));
  const uint16_t* __restrict__ info_pos = reinterpret_cast<const uint16_t*>(code + h.off_info_pos);
  const uint8_t* __restrict__  is_pc    = code + h.off_is_pc;
  const int32_t* __restrict__  rx_first = reinterpret_cast<const int32_t*>(code + h.off_rx_first);
  const uint16_t* __restrict__ rx_fidx  = reinterpret_cast<const uint16_t*>(code + h.off_rx_fidx);
  const uint32_t* __restrict__ sched    = reinterpret_cast<const uint32_t*>(code + h.off_sched);
  int8_t*        L   = L_all[seg];
  uint8_t*       est = est_all[seg];
  uint8_t*       u   = u_all[seg];
  const int      N = (int)h.N, E = (int)h.E, K = (int)h.K;
  const int8_t*  f = llr + t.llr_offset + (size_t)seg * h.E; // segment r owns soft bits [r E_r, (r + 1) E_r)
  for (int q = lane; q < N; q += 64) {
    L[N + q] = (int8_t)polar_dematch_value(rx_first[q], N, E, f, rx_fidx);
    est[q]   = 0;
    u[q]     = 0;
  }
  __syncthreads();
  polar_ssc_run<64>(L, est, u, sched, h.sched_len, lane);
  // Deallocation (polar_deallocator_impl.cpp:27-42) into the partial-sum array, which the schedule has finished with.
  uint8_t* msg = est;
  if (h.nPC == 0) {
    for (int i = lane; i < K; i += 64)
      msg[i] = u[info_pos[i]];
  } else if (lane == 0) {
    int iK = 0;
    for (int i = 0; i < (int)(h.K + h.nPC); ++i)
      if (!is_pc[i])
        msg[iK++] = u[info_pos[i]];
  }
  __syncthreads();
  // Remainder of the K decoded bits modulo the segment's CRC polynomial.
  const uint32_t order = h.L, poly = (h.L == 6) ? (uint32_t)UCI_POLAR_CRC6_POLY : (uint32_t)UCI_POLAR_CRC11_POLY, top = 1u << order;
  const int      chunk = (K + 63) >> 6, a = lane * chunk, b = min(a + chunk, K);
  uint32_t       reg = 0;
  for (int i = a; i < b; ++i) {
    reg = (reg << 1) | msg[i];
    reg ^= (reg & top) ? poly : 0u;
  }
  if (a < K) {
    uint32_t pw = 1, base = 2; // x^(K - b) mod g by square and multiply
    for (uint32_t d = (uint32_t)(K - b); d != 0; d >>= 1) {
      if (d & 1u)
        pw = crc_gf2_mulmod(pw, base, poly, order);
      base = crc_gf2_mulmod(base, base, poly, order);
    }
    reg = crc_gf2_mulmod(reg, pw, poly, order);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    reg ^= __shfl_xor(reg, off);
  if (lane == 0)
    crc_rem[seg] = reg;
  // The field's payload: the segments one after the other without the pad bit in front of the first.
  const int A_seg = K - (int)h.L;
  for (int i = lane; i < A_seg; i += 64) {
    const int o = seg * A_seg + i - (int)t.pad;
    if (o >= 0)
      payload[t.payload_offset + o] = msg[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t rem = crc_rem[0];
    if (C == 2)
      rem |= crc_rem[C - 1];
    status[t.job] = rem == 0 ? MIPHY_UCI_STATUS_VALID : MIPHY_UCI_STATUS_INVALID;
  }
}

// The status bytes of the fields whose segments are tasks [first_task, first_task + count) of the list kernel.
__global__ void __launch_bounds__(64) uci_polar_status_fill_kernel(const uint8_t* __restrict__ piece, uint32_t first_task, uint32_t count, uint8_t* __restrict__ status)
{
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i < count)
    status[reinterpret_cast<const uci_polar_task*>(piece)[first_task + i].job] = MIPHY_UCI_STATUS_VALID;
}

// One segment of a CRC11 field (nPC = 0) per one-wave workgroup: rate dematching, the list recursion, then among the survivors the
// smallest (metric, slot) whose CRC11 checks, or the smallest overall where none does. LDS: polar_scl_lds_bytes(N, L), dynamic.
__global__ void __launch_bounds__(64) uci_polar_scl_kernel(const uint8_t* __restrict__ piece, uint32_t first_task, int L, const int8_t* __restrict__ llr,
                                                           uint8_t* __restrict__ payload, uint8_t* __restrict__ status)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int                lane = threadIdx.x;
  const uci_polar_task     t    = load_words(reinterpret_cast<const uci_polar_task*>(piece) + first_task + blockIdx.x);
  const uint8_t*           code = piece + t.code_off;
  const uci_polar_code_hdr h    = load_words(reinterpret_cast<const uci_polar_code_hdr*>(code));
  const uint16_t* __restrict__ info_pos = reinterpret_cast<const uint16_t*>(code + h.off_info_pos);
  const int32_t* __restrict__  rx_first = reinterpret_cast<const int32_t*>(code + h.off_rx_first);
  const uint16_t* __restrict__ rx_fidx  = reinterpret_cast<const uint16_t*>(code + h.off_rx_fidx);
  const uint8_t* __restrict__  flags    = code + h.off_list;
  const int     N = (int)h.N, n = __ffs(N) - 1, E = (int)h.E, K = (int)h.K;
  const int     PSZ   = 3 * N;
  int8_t*       ch    = reinterpret_cast<int8_t*>(smem);
  uint8_t*      bankA = smem + N;
  uint8_t*      bankB = bankA + (size_t)L * PSZ;
  int*          pm    = reinterpret_cast<int*>(bankB + (size_t)L * PSZ);
  int*          sel   = pm + 8;
  uint8_t*      kset  = reinterpret_cast<uint8_t*>(sel + 24);
  const int8_t* f     = llr + t.llr_offset + (size_t)t.seg * h.E; // segment r owns soft bits [r E_r, (r + 1) E_r)
  for (int q = lane; q < 2 * N; q += 64)
    kset[q] = flags[q];
  for (int q = lane; q < N; q += 64)
    ch[q] = (int8_t)polar_dematch_value(rx_first[q], N, E, f, rx_fidx);
  if (lane < 8)
    pm[lane] = 0;
  __syncthreads();
  uint8_t*  P      = bankA;
  uint8_t*  Q      = bankB;
  const int active = polar_scl_run(ch, P, Q, pm, sel, kset, N, n, L, lane);
  // The K bits of every survivor in K-set order (no parity-check positions, no interleaver) into bank Q, which the recursion is done with.
  for (int idx = lane; idx < active * K; idx += 64) {
    const int q = idx / K, k = idx - q * K;
    Q[q * PSZ + k] = P[q * PSZ + 2 * N + info_pos[k]];
  }
  __syncthreads();
  // Lane q takes survivor q: the remainder of its K bits modulo the CRC11 polynomial is zero exactly when the CRC over the first K - 11
  // equals the last 11.
  int my_pm = 0x7fffffff, my_ok = 0;
  if (lane < active) {
    const uint8_t* cand = Q + lane * PSZ;
    uint32_t       reg  = 0;
    for (int k = 0; k < K; ++k) {
      reg = (reg << 1) | cand[k];
      reg ^= (reg & (1u << 11)) ? (uint32_t)UCI_POLAR_CRC11_POLY : 0u;
    }
    my_pm = pm[lane];
    my_ok = reg == 0;
  }
  const bool any_ok = __ballot(my_ok != 0) != 0ull;
  int        best = (lane < active && (!any_ok || my_ok)) ? my_pm : 0x7fffffff, best_lane = lane;
#pragma unroll
  for (int off = 4; off >= 1; off >>= 1) {
    const int ok = __shfl_xor(best, off), ol = __shfl_xor(best_lane, off);
    if (ok < best || (ok == best && ol < best_lane)) {
      best      = ok;
      best_lane = ol;
    }
  }
  best_lane = __shfl(best_lane, 0);
  // The segment's share of the payload: the first segment drops the pad bit.
  const uint8_t* win   = Q + best_lane * PSZ;
  const int      A_seg = K - 11;
  for (int i = lane; i < A_seg; i += 64) {
    const int o = (int)t.seg * A_seg + i - (int)t.pad;
    if (o >= 0)
      payload[t.payload_offset + o] = win[i];
  }
  if (!any_ok && lane == 0)
    status[t.job] = MIPHY_UCI_STATUS_INVALID; // the other segment may store the same value: benign
}

template <typename T>
uint32_t append(std::vector<uint8_t>& blob, const std::vector<T>& v)
{
  const uint32_t off = (uint32_t)blob.size();
  blob.resize(off + ((v.size() * sizeof(T) + 3) & ~(size_t)3), 0);
  if (!v.empty())
    memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
  return off;
}

// The code block of (K_r, E_r, nMax = 10, ibil = 1) from the context's host cache, or constructed now. (K_r, E_r) is the whole key:
// the CRC length the block carries follows from K_r (uci_polar_crc_bits_of_K).
int get_code(miphy_ctx* ctx, uint32_t K, uint32_t E, std::shared_ptr<const std::vector<uint8_t>>& out)
{
  auto&          ext = *ctx->ext;
  const uint32_t key = K << 16 | E;
  for (auto& e : ext.uci_polar_codes)
    if (e.key == key) {
      e.used = ++ext.uci_polar_clock;
      out    = e.blob;
      return MIPHY_OK;
    }
  const miphy_polar_code c = {K, E, 10, 1};
  polar_host_code        h;
  int                    rc = polar_build_code(&c, h);
  if (rc)
    return rc;
  polar_host_tables t;
  polar_build_tables(h, true, t);
  std::vector<uint8_t> list_flags;
  polar_build_list_flags(h, list_flags);
  auto               blob = std::make_shared<std::vector<uint8_t>>(sizeof(uci_polar_code_hdr), 0);
  uci_polar_code_hdr hd   = {};
  hd.K = h.K, hd.E = h.E, hd.N = h.N, hd.nPC = h.nPC, hd.L = uci_polar_crc_bits_of_K(K), hd.sched_len = (uint32_t)t.sched.size();
  hd.off_info_pos = append(*blob, t.info_pos), hd.off_is_pc = append(*blob, t.is_pc), hd.off_rx_first = append(*blob, t.rx_first);
  hd.off_rx_fidx = append(*blob, t.rx_fidx), hd.off_sched = append(*blob, t.sched);
  hd.off_list = append(*blob, list_flags);
  blob->resize((blob->size() + 15) & ~(size_t)15, 0);
  hd.bytes = (uint32_t)blob->size();
  memcpy(blob->data(), &hd, sizeof(hd));
  out = blob;
  if (ext.uci_polar_codes.size() < UCI_POLAR_HOST_CACHE_ENTRIES) {
    ext.uci_polar_codes.emplace_back();
    ext.uci_polar_codes.back() = {key, ++ext.uci_polar_clock, blob};
  } else {
    auto lru = std::min_element(ext.uci_polar_codes.begin(), ext.uci_polar_codes.end(),
                                [](const uci_polar_host_code& x, const uci_polar_host_code& y) { return x.used < y.used; });
    *lru     = {key, ++ext.uci_polar_clock, blob};
  }
  return MIPHY_OK;
}

// One piece: the SSC tasks of its one-segment fields, those of its two-segment fields, the list tasks (one per segment) grouped by
// code size, so that every launch of the list kernel reserves the LDS of its own N only, and one copy of every code block they use.
struct piece_builder {
  std::vector<uci_polar_task>                     tasks[2];
  std::map<uint32_t, std::vector<uci_polar_task>> list; // N -> segments
  size_t                                          nof_list = 0;
  std::vector<uint8_t>                            codes;
  std::map<uint32_t, uint32_t>                    code_off; // key -> offset in `codes`
  size_t bytes() const { return (tasks[0].size() + tasks[1].size() + nof_list) * sizeof(uci_polar_task) + codes.size(); }
  bool   empty() const { return tasks[0].empty() && tasks[1].empty() && nof_list == 0; }
  void   clear() { tasks[0].clear(), tasks[1].clear(), list.clear(), nof_list = 0, codes.clear(), code_off.clear(); }
};

int flush(miphy_ctx* ctx, piece_builder& p, std::vector<uint8_t>& buf, uint32_t list_size, const int8_t* llr, uint8_t* payload, uint8_t* status, hipStream_t s,
          unsigned& pieces)
{
  if (p.empty())
    return MIPHY_OK;
  const uint32_t n1 = (uint32_t)p.tasks[0].size(), n2 = (uint32_t)p.tasks[1].size(), nl = (uint32_t)p.nof_list;
  const size_t   tb = (size_t)(n1 + n2 + nl) * sizeof(uci_polar_task);
  buf.resize(tb + p.codes.size());
  auto* t   = reinterpret_cast<uci_polar_task*>(buf.data());
  auto  put = [&](const std::vector<uci_polar_task>& v) {
    for (const uci_polar_task& x : v) {
      *t = x;
      t->code_off += (uint32_t)tb;
      ++t;
    }
  };
  put(p.tasks[0]), put(p.tasks[1]);
  for (const auto& g : p.list)
    put(g.second);
  memcpy(buf.data() + tb, p.codes.data(), p.codes.size());
  const void* d  = nullptr;
  int         rc = miphy_stage_descs(ctx, buf.data(), 0, buf.size(), s, &d);
  if (rc)
    return rc;
  if (n1)
    hipLaunchKernelGGL((uci_polar_decode_kernel<1>), dim3(n1), dim3(64), 0, s, (const uint8_t*)d, 0u, llr, payload, status);
  if (n2)
    hipLaunchKernelGGL((uci_polar_decode_kernel<2>), dim3(n2), dim3(128), 0, s, (const uint8_t*)d, n1, llr, payload, status);
  if (nl) {
    hipLaunchKernelGGL(uci_polar_status_fill_kernel, dim3((nl + 63) / 64), dim3(64), 0, s, (const uint8_t*)d, n1 + n2, nl, status);
    uint32_t first = n1 + n2;
    for (const auto& g : p.list) {
      const size_t lds = polar_scl_lds_bytes(g.first, list_size);
      // Above 48 KB of dynamic LDS the limit is raised; it is a per-device attribute of the kernel, so it is set on every such launch.
      if (lds > 48 * 1024) {
        MIPHY_HIP_CHECK(hipFuncSetAttribute((const void*)uci_polar_scl_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      }
      hipLaunchKernelGGL(uci_polar_scl_kernel, dim3((uint32_t)g.second.size()), dim3(64), lds, s, (const uint8_t*)d, first, (int)list_size, llr, payload, status);
      first += (uint32_t)g.second.size();
    }
  }
  MIPHY_HIP_CHECK(hipGetLastError());
  ++pieces;
  p.clear();
  return MIPHY_OK;
}

} // namespace

extern "C" void miphy_debug_set_uci_polar_piece_bytes(size_t bytes)
{
  g_piece_bytes = std::min(bytes, UCI_POLAR_PIECE_MAX);
}

extern "C" unsigned miphy_debug_uci_polar_pieces(void)
{
  return g_last_pieces;
}

extern "C" int miphy_uci_polar_info(uint32_t nof_bits, uint32_t nof_llr, miphy_uci_polar_info_t* out)
{
  MIPHY_REQUIRE(out, "miphy_uci_polar_info: null argument");
  uci_polar_framing f;
  int               rc = uci_polar_frame_or_error("uci_polar_info", 0, nof_bits, nof_llr, f);
  if (rc)
    return rc;
  out->C = f.C, out->L = f.L, out->K_r = f.K_r, out->E_r = f.E_r, out->n = polar_code_n(f.K_r, f.E_r, 10), out->nPC = f.nPC;
  return MIPHY_OK;
}

namespace {

// Every entry point. List size 1 is the SSC kernel for every field; above it the CRC6 fields (12..19 bits, parity-check bits) stay with
// the SSC kernel and every segment of a CRC11 field becomes a task of the list kernel. The verdict of field i goes to status[i], or to
// status[status_index[i]] where the caller keeps its status bytes inside records of its own (the PUCCH processor).
int decode_fields(const char* who, miphy_ctx* ctx, const miphy_uci_polar_job* jobs, uint32_t n, uint32_t list_size, const int8_t* llr, uint8_t* payload,
                  uint8_t* status, const uint32_t* status_index, void* stream)
{
  MIPHY_REQUIRE(ctx && jobs && llr && payload && status, "%s: null argument", who);
  MIPHY_REQUIRE(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "%s: list size %u not in {1,2,4,8}", who, list_size);
  MIPHY_REQUIRE(n <= (1u << 24), "uci_polar_decode: at most 2^24 fields per call");
  unsigned pieces = 0, ssc_segments = 0, list_segments = 0;
  if (n == 0) {
    g_last_pieces = 0, g_last_ssc_segments = 0, g_last_list_segments = 0;
    return MIPHY_OK;
  }
  // Every job is framed and every code of the call constructed before anything is staged. The call holds its codes itself: the
  // host cache may evict one while the call is still being put together.
  std::vector<uci_polar_framing>                                      fr(n);
  std::map<uint32_t, std::shared_ptr<const std::vector<uint8_t>>>     codes;
  int                                                                 rc;
  for (uint32_t i = 0; i < n; ++i) {
    if ((rc = uci_polar_frame_or_error("uci_polar_decode", i, jobs[i].nof_bits, jobs[i].nof_llr, fr[i])))
      return rc;
    auto& blob = codes[fr[i].K_r << 16 | fr[i].E_r];
    if (!blob && (rc = get_code(ctx, fr[i].K_r, fr[i].E_r, blob)))
      return rc;
  }
  const size_t         piece_bytes = g_piece_bytes.load();
  const size_t         limit       = piece_bytes ? piece_bytes : UCI_POLAR_PIECE_BYTES;
  hipStream_t          s     = (hipStream_t)stream;
  piece_builder        p;
  std::vector<uint8_t> buf;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t key  = fr[i].K_r << 16 | fr[i].E_r;
    const auto&    blob = *codes[key];
    const bool     have = p.code_off.count(key) != 0;
    const bool     list = list_size > 1 && fr[i].L == 11;
    const size_t   need = (list ? fr[i].C : 1) * sizeof(uci_polar_task) + (have ? 0 : blob.size()); // the segments of a field share a piece
    if (!p.empty() && p.bytes() + need > limit) {
      if ((rc = flush(ctx, p, buf, list_size, llr, payload, status, s, pieces))) // a HIP or staging failure here leaves the earlier pieces enqueued
        return rc;
    }
    auto it = p.code_off.find(key);
    if (it == p.code_off.end()) {
      it = p.code_off.emplace(key, (uint32_t)p.codes.size()).first;
      p.codes.insert(p.codes.end(), blob.begin(), blob.end());
    }
    uci_polar_task t = {};
    t.code_off = it->second, t.job = status_index ? status_index[i] : i, t.pad = fr[i].pad;
    t.llr_offset = jobs[i].llr_offset, t.payload_offset = jobs[i].payload_offset;
    if (list) {
      auto& group = p.list[reinterpret_cast<const uci_polar_code_hdr*>(blob.data())->N];
      for (t.seg = 0; t.seg < fr[i].C; ++t.seg)
        group.push_back(t);
      p.nof_list += fr[i].C;
      list_segments += fr[i].C;
    } else {
      p.tasks[fr[i].C - 1].push_back(t);
      ssc_segments += fr[i].C;
    }
  }
  rc            = flush(ctx, p, buf, list_size, llr, payload, status, s, pieces);
  g_last_pieces = pieces, g_last_ssc_segments = ssc_segments, g_last_list_segments = list_segments;
  return rc;
}

} // namespace

extern "C" void miphy_debug_uci_polar_list_segments(unsigned* ssc, unsigned* list)
{
  if (ssc)
    *ssc = g_last_ssc_segments;
  if (list)
    *list = g_last_list_segments;
}

extern "C" int miphy_uci_polar_decode_batch(miphy_ctx* ctx, const miphy_uci_polar_job* jobs, uint32_t n, const int8_t* llr, uint8_t* payload, uint8_t* status,
                                            void* stream)
{
  return decode_fields("miphy_uci_polar_decode_batch", ctx, jobs, n, 1, llr, payload, status, nullptr, stream);
}

extern "C" int miphy_uci_polar_decode_list_batch(miphy_ctx* ctx, const miphy_uci_polar_job* jobs, uint32_t n, uint32_t list_size, const int8_t* llr,
                                                 uint8_t* payload, uint8_t* status, void* stream)
{
  return decode_fields("miphy_uci_polar_decode_list_batch", ctx, jobs, n, list_size, llr, payload, status, nullptr, stream);
}

int miphy_uci_polar_decode_fields(const char* who, miphy_ctx* ctx, const miphy_uci_polar_job* jobs, uint32_t n, uint32_t list_size, const int8_t* llr,
                                  uint8_t* payload, uint8_t* status, const uint32_t* status_index, hipStream_t s)
{
  return decode_fields(who, ctx, jobs, n, list_size, llr, payload, status, status_index, s);
}
