// Internal definitions shared by the HIP translation units of libmiphy.so (gfx950 only).
#pragma once
#include "../../include/miphy.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#define MIPHY_MAX_Z 384
#define MIPHY_NOF_Z 51
#define MIPHY_BG1_EDGES 316
#define MIPHY_BG2_EDGES 197
#define MIPHY_MAX_EDGES 316
#define MIPHY_CRC_ZMASK_WORDS 264 // 8448 bits: the largest codeblock
#define MIPHY_NOF_SIDE_STREAMS 3

// Per-(base graph, lifting size) edge table entry: low 16 bits = column*Z (LDS byte offset of the variable node),
// high 16 bits = cyclic shift (already reduced modulo Z).
struct miphy_graph_tables {
  uint32_t edge[2][MIPHY_NOF_Z][MIPHY_MAX_EDGES];
  uint32_t edge_sb[2][MIPHY_NOF_Z][2 * MIPHY_MAX_EDGES]; // the same, unpacked: {shift, column*Z} per edge (scalar operands as loaded)
  uint16_t row_start[2][48];
  uint16_t pair_start[2][48]; // prefix sum of ceil(degree / 2) over the layers (packed decoder message storage)
  uint16_t z_pos[MIPHY_MAX_Z + 1]; // position of Z in the list of lifting sizes, 0xffff if invalid
  uint8_t  i_ls[MIPHY_MAX_Z + 1];  // lifting-size set index
  // CRC: pow32[p][k] = x^(32k) mod poly_p for k in [0, 320); poly/order per id.
  uint32_t crc_pow32[5][320];
  uint32_t crc_pow2[5][24]; // x^(32 * 2^b) mod poly
  uint32_t crc_pow32_hi[5][256]; // x^(32 * 256 * k) mod poly: with crc_pow32[k & 255] covers messages up to 2 Mbit in one product
  uint32_t crc_poly[5];
  uint32_t crc_order[5];
  // Zero test of a codeblock CRC by masks (LDPC decoders): for the polynomials a codeblock can carry (index 0 = CRC24A, 1 = CRC24B,
  // 2 = CRC16) and word u counted from the END of the message padded with zeros to a multiple of 32 bits, crc_zmask[.][u][k] selects
  // the bits of that word whose weight x^(distance to the end + order) mod P has bit k set; bit k of the checksum of the padded
  // message is the parity of the sum over u of popcount(word & mask). (M(x) x^r mod P == 0 <=> M(x) mod P == 0, so the padding
  // does not change the verdict.) Word layout: MSB first, bit 31 - i of a word is message bit i of its group of 32 (hard_word(): the word of the output).
  // ([k][u], coalesced across the lanes, was measured: 24 dword loads per lane instead of 6 x 16 bytes cost the decoder 1 %; the 25 KB
  // table is cache resident either way.)
  uint32_t crc_zmask[3][MIPHY_CRC_ZMASK_WORDS][24];
  // The same for CRC24A over PACKED message bytes read as little-endian dwords (transport-block assembly): bit 8 k + 7 - j of a
  // word is message bit 8 k + j of its group of 32.
  uint32_t crc_zmask_packed24a[MIPHY_CRC_ZMASK_WORDS][24];
};
// index into crc_zmask for a MIPHY_CRC_* id, -1 if the polynomial has no mask table
static inline __host__ __device__ int miphy_crc_zmask_index(int crc_id)
{
  return crc_id == 0 ? 0 : (crc_id == 1 ? 1 : (crc_id == 3 ? 2 : -1));
}

// Allocated PRBs of a five-word mask on a grid of grid_nof_prb PRBs: word popcounts, the bits behind the grid masked off. Whatever
// grid_nof_prb holds, no word behind the fifth is read. (Uniform arguments: scalar popcounts on the device.)
static inline __host__ __device__ unsigned miphy_count_prb(const uint64_t* rb_mask, unsigned grid_nof_prb)
{
  unsigned n = 0;
#pragma unroll
  for (int w = 0; w < 5; ++w) {
    const int left = (int)grid_nof_prb - 64 * w;
    if (left > 0)
      n += (unsigned)__builtin_popcountll(rb_mask[w] & (left >= 64 ? ~0ull : ((1ull << left) - 1ull)));
  }
  return n;
}

// Geometry of an LDPC codeblock, for host and device alike: the kernels carve their LDS up with the very functions the launch planner
// sizes it with. bgi = base graph - 1.
static constexpr __host__ __device__ int miphy_bg_K(int bgi) // systematic columns
{
  return bgi ? 10 : 22;
}
static constexpr __host__ __device__ int miphy_bg_M(int bgi) // layers (rows of the base graph)
{
  return bgi ? 42 : 46;
}
static constexpr __host__ __device__ int miphy_bg_N_short(int bgi) // columns without the two punctured ones: the longest input, in units of Z
{
  return bgi ? 50 : 66;
}
// Variable nodes an input of in_len soft bits reaches: ceil((in_len + 2 Z) / Z), the punctured nodes in front (ldpc_decoder_impl.cpp:101-114).
static constexpr __host__ __device__ int miphy_ldpc_nodes(unsigned in_len, unsigned Z)
{
  return (int)((in_len + 2u * Z + Z - 1u) / Z);
}
// Layers a launch can reach from its bound on the variable nodes (no decode runs fewer than four).
static constexpr __host__ __device__ int miphy_ldpc_layers(int bgi, int nodes)
{
  const int M = miphy_bg_M(bgi), lay = nodes - miphy_bg_K(bgi), lo = 4 > lay ? 4 : lay;
  return M < lo ? M : lo;
}
// Bytes of the soft bits of a codeblock that reaches `lay` layers, as a 16-byte multiple (Zt >= Z: the launch's bound or the lifting size).
static constexpr __host__ __device__ int miphy_ldpc_soft_bytes(int bgi, int lay, int Zt)
{
  return ((miphy_bg_K(bgi) + lay) * Zt + 15) & ~15;
}

// Scratch workspaces of a context, one per user group: calls that run one inside another take different slots.
enum miphy_workspace {
  MIPHY_WS_GENERAL = 0,  // staged descriptors of the transport-block level entry points (PUSCH decode, PDSCH encode), the UL-SCH
                         // demultiplexer's plans, the four-step DFT, the PBCH encoder
  MIPHY_WS_PUSCH_PROC,   // intermediate buffers of miphy_pusch_process_batch (estimates, LLRs, EVM sums)
  MIPHY_WS_OUTPUT,       // codewords of miphy_pdsch_process_batch, encoded PDCCH / PBCH bits, compacted results of miphy_pusch_process_batch
  MIPHY_WS_LDPC_MSGS,    // check-to-variable messages of the LDPC decoder when they do not stay in LDS (per-call entry points)
  MIPHY_WS_SEQUENCES,    // scrambling sequences of the PUSCH demodulator and of the PDSCH modulator (per-call entry point)
  MIPHY_WS_PUCCH_LLR,    // soft bits of the long format-2 PDUs of miphy_pucch_process_batch_ex when the caller passes no llr_out
  MIPHY_NOF_WORKSPACES
};

struct miphy_ctx_ext; // C++ side caches (twiddle tables, OFDM plans), see miphy_ext.h

struct miphy_ctx {
  int                  device;
  miphy_ctx_ext*       ext;
  miphy_graph_tables*  d_tables; // device copy
  miphy_graph_tables*  h_tables; // host copy
  void*                d_desc_staging; // descriptor staging: a RING of desc_staging_bytes on the device and the same in pinned host memory,
  size_t               desc_staging_bytes; // handed out front to back (miphy_stage_descs, miphy_upload); the device is synchronised only when
  void*                h_desc_staging; // pinned    // the ring wraps, so a call with host descriptors never waits for the stream
  size_t               staging_head;
  void*                ring_streams[4]; // streams that regions of the ring were staged for since its last wrap (the wrap waits for them)
  int                  nof_ring_streams; // 5 = more than four
  void*                d_work[MIPHY_NOF_WORKSPACES];     // scratch workspaces, grown on demand (miphy_get_workspace)
  size_t               work_bytes[MIPHY_NOF_WORKSPACES];
  int                  num_cus; // compute units of the device (persistent-kernel grid sizing)
  uint32_t*            d_queue; // work-queue counters of the persistent kernels: a ring of MIPHY_NOF_QUEUE_COUNTERS words, one per launch
  uint32_t             queue_next;
  // Side streams of the class-sorted LDPC decoder launches (created on first use): the launch classes of one call are independent, and the
  // small ones are latency-bound chains that leave the chip idle -- they run next to the large ones, forked from / joined to the caller's
  // stream with events (a pattern a HIP graph capture records as is).
  void*                side_stream[MIPHY_NOF_SIDE_STREAMS];
  void*                ev_fork;
  void*                ev_join[MIPHY_NOF_SIDE_STREAMS];
};
#define MIPHY_NOF_QUEUE_COUNTERS 256

void miphy_set_error(const char* fmt, ...);

#define MIPHY_HIP_CHECK(expr)                                                                 \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      miphy_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
      return MIPHY_EHIP;                                                                      \
    }                                                                                         \
  } while (0)

#define MIPHY_REQUIRE(cond, ...)          \
  do {                                    \
    if (!(cond)) {                        \
      miphy_set_error(__VA_ARGS__);       \
      return MIPHY_EINVAL;                \
    }                                     \
  } while (0)

#ifdef __HIPCC__
// A descriptor through dword loads: read field by field, its 8- and 16-bit members become vector loads with a wait each (gfx950 has no
// scalar sub-dword loads); as dwords the whole record arrives in scalar registers with one request and the fields are shifts.
template <class T>
__device__ __forceinline__ T load_words(const T* __restrict__ p)
{
  static_assert(sizeof(T) % 4 == 0, "dword multiple");
  uint32_t                     w[sizeof(T) / 4];
  const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i)
    w[i] = s[i];
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}
#endif

// Ensures the descriptor array is on the device; returns the device pointer through *out. Host descriptors are copied into the
// context's staging ring (pinned host -> device, asynchronous on `s`): the call does not wait for the stream, and the caller's array
// can be reused as soon as it returns.
int miphy_stage_descs(miphy_ctx* ctx, const void* descs, int on_device, size_t bytes, hipStream_t s, const void** out);
// Asynchronous upload of a host buffer of any kind (pageable, a local vector) to device memory `dst`, ordered on `s`: the bytes travel
// through the pinned ring, so `src` can be released when the call returns and the stream is not waited for. (Buffers larger than half
// the ring are copied directly and the stream is synchronised, as every upload was before.)
int miphy_upload(miphy_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);

#ifdef __cplusplus
#include <vector>
// Launch classes of a batch whose descriptors the host can see (ldpc_decode.hip, the host side of the decoder): codeblocks sorted so that each class shares a
// workgroup size and an LDS size.
struct miphy_ldpc_class {
  uint8_t  kind;  // 0 = wave kernel (Z <= 64, several codeblocks per wavefront); 1..3 = packed kernel with that many wavefronts per codeblock
  uint8_t  bgi;   // base graph - 1
  uint8_t  fused; // every codeblock can be rate-dematched by the decoder while it loads
  uint8_t  lay;   // layers a codeblock of the class can reach at most
  uint8_t  runs_all_iterations; // some codeblock of the class cannot stop early (no CRC, or a CRC checked behind the last iteration only)
  uint16_t max_Z, min_Z;
  uint32_t first, count;               // the class's range of `order`
  uint32_t bundle_first, bundle_count; // kind 0: its range of `bundles` (pairs of words)
  uint32_t soft_total;                 // kind 0: LDS bytes for the soft bits of a bundle
};
struct miphy_ldpc_classes {
  std::vector<uint32_t>         order;   // codeblock indices, class after class; classes that are not fused come first
  std::vector<uint32_t>         bundles; // wave kernel: {first position in order, count} per bundle
  std::vector<miphy_ldpc_class> classes;
  uint32_t                      nof_unfused = 0; // order[0 .. nof_unfused) need the rate dematcher as a launch of its own
  bool                          identity    = true;
};
// fusable: optional flag per codeblock ("the decoder may dematch it"); descriptors must be valid (validated by the caller).
void miphy_ldpc_build_classes(const miphy_ldpc_dec_desc* descs, uint32_t n, const uint8_t* fusable, miphy_ldpc_classes& C);
// One decoder launch per class, its geometry decided on the host once (miphy_ldpc_plan_launches) and enqueued by miphy_ldpc_run_launches.
struct miphy_ldpc_launch {
  miphy_ldpc_class c;
  unsigned         used;       // MIPHY_LDPC_KERNEL_*: SCALAR, WAVE or PACKED names the kernel, the other bits its form
  int              stream;     // 0 = the caller's, 1 .. = the context's side streams
  int              threads;    // workgroup size (the latency form: every part)
  int              nodes;      // variable nodes a codeblock can reach: the kernels size their arrays by it
  int              parts;      // packed kernel: 1, or 2 / 4 in the latency form
  int              gmsg_pairs; // message dwords per lane in global memory (0: all in LDS)
  int              lds_pairs;  // ... and those that stay in LDS in front of them (a layer boundary of the base graph)
  size_t           lds;
  uint32_t         grid;
  bool             ordered;    // decodes order[c.first ...] (false: the codeblocks in array order)
  bool             atab;       // packed kernel: the instance that reads its soft-bit addresses from a table (ldpc_pk_device.h, pk_table_addresses)
  const void*      adr_by_z;   // ... device array of the tables of the class, at [Z / 16] (miphy_ldpc_address_tables; owned by the context)
  bool             row_skip;   // packed kernel: the instance whose wavefronts leave out the visits of layers with saturated rows (ldpc_decode_pk.hip, RSKIP)
  size_t           gmsg_off, gmsg_bytes; // the launch's part of the message scratch
};
struct miphy_ldpc_launches {
  std::vector<miphy_ldpc_launch> l;
  size_t                         gmsg_bytes   = 0;     // message scratch of all launches together (they run side by side)
  bool                           side_streams = false; // launches fork to the context's side streams (miphy_side_streams first)
  bool                           scalar       = false; // the one-row-per-lane kernel is forced: nothing is dematched in the decoder
};
#define MIPHY_LDPC_ADR_TABLE_DEGREE 19 // edges per layer of the classes that read their soft-bit addresses from a table (PK_ATAB_DEGREE of ldpc_decode_pk.hip)
// Modes of miphy_debug_force_ldpc_kernel (include/miphy.h): a mode in the low byte, plus flag bits.
enum miphy_ldpc_force_mode {
  MIPHY_LDPC_FORCE_AUTO        = 0,
  MIPHY_LDPC_FORCE_ROW         = 1, // the one-row-per-lane kernel: one launch per call, every class of a table
  MIPHY_LDPC_FORCE_PACKED_ONE  = 2, // the packed kernel as ONE launch per call (tables: as AUTO)
  MIPHY_LDPC_FORCE_CLASSES     = 3, // class-sorted launches (what AUTO does with host descriptors)
  MIPHY_LDPC_FORCE_THROUGHPUT  = 4, // class-sorted, the geometry of a batch that fills the chip: no latency form, messages global wherever that buys residency
  MIPHY_LDPC_FORCE_LATENCY_ALL = 5, // class-sorted, the latency form in two parts on every packed class
  MIPHY_LDPC_FORCE_LATENCY2    = 6, // AUTO with the latency form in two parts instead of four
  MIPHY_LDPC_FORCE_MODE_MASK   = 0xff,
  MIPHY_LDPC_FORCE_ALL_GMSG    = 0x100, // flag: a GMSG launch keeps ALL its messages in global memory
  MIPHY_LDPC_FORCE_NO_ADR_TABLE = 0x200, // flag: no launch reads its soft-bit addresses from a table (every class computes them)
  MIPHY_LDPC_FORCE_NO_ROW_SKIP  = 0x400  // flag: no launch takes an instance that leaves out the layer visits of saturated rows
};
// Host only: the launch table of the classes C (their order / bundles are device arrays by then). fuse: the fused classes dematch while
// they load (the caller then passes rate-dematcher descriptors to the run). The debug knobs of miphy_debug_force_ldpc_kernel and
// miphy_debug_set_ldpc_class_streams are read when a table is made -- one snapshot per table -- and nowhere else.
// A launch that takes the address-table instance gets the tables of its class from the context's cache (built on first use).
int miphy_ldpc_plan_launches(miphy_ctx* ctx, const miphy_ldpc_classes& C, bool fuse, miphy_ldpc_launches& T);
// The soft-bit address tables of the lifting sizes min_Z ... max_Z (multiples of 16) of base graph bgi + 1 with `lay` layers, on the
// device: *out = device array of table pointers indexed by Z / 16. Built once per (base graph, Z, layers) and kept until miphy_destroy,
// so that launch tables and prepared plans may hold the pointer; a key the cache holds is never rebuilt.
int miphy_ldpc_address_tables(miphy_ctx* ctx, int bgi, int lay, int min_Z, int max_Z, const void** out);
// Enqueues the table on `s`: the fork to the side streams (created by then), one launch per class, the join -- on every path after the
// fork. d_order / d_bundles = device copies of C.order / C.bundles; gmsg = T.gmsg_bytes of message scratch; d_rdm / rm_in: rate-dematcher
// descriptors (same index as d_descs) and rate-matched input of the fused classes.
int miphy_ldpc_run_launches(miphy_ctx* ctx, const miphy_ldpc_launches& T, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order,
                            const uint32_t* d_bundles, const int8_t* llr, uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot,
                            uint8_t* harq_crc_ok, const miphy_ldpc_rdm_desc* d_rdm, const int8_t* rm_in, void* gmsg, hipStream_t s);
// One-row-per-lane kernel (ldpc_decode_row.hip): LDS bytes of a workgroup of `threads` lanes whose codeblocks reach `lay` layers, geometry
// of L.c, and the launch of L.grid codeblocks (d_order: codeblocks d_order[0 .. grid) of the arrays, null: the first grid).
size_t miphy_ldpc_row_lds_bytes(int bgi, int lay, size_t threads);
void   miphy_ldpc_row_geometry(miphy_ldpc_launch& L);
int    miphy_ldpc_row_launch(miphy_ctx* ctx, const miphy_ldpc_launch& L, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order, const int8_t* llr,
                             uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot, uint8_t* harq_crc_ok, hipStream_t s);
// Wave kernel (ldpc_decode_pkw.hip): geometry of L.c (lds, grid, messages in global memory or not), and its launch. throughput_form (A-B
// knob): the geometry of a launch that fills the chip, whatever its size.
void miphy_ldpc_pkw_geometry(const miphy_ctx* ctx, bool throughput_form, miphy_ldpc_launch& L);
int  miphy_ldpc_pkw_launch(miphy_ctx* ctx, const miphy_ldpc_launch& L, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order,
                           const uint32_t* d_bundles, const int8_t* llr, uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot,
                           uint8_t* harq_crc_ok, void* gmsg, hipStream_t s);
// Packed (two rows per lane) kernel (ldpc_decode_pk.hip): LDS bytes of a geometry (pairs_all = 0: messages in global memory; parts = 2 / 4:
// + exchange slots of the latency form), wavefronts per CU its register budget allows, resident workgroups per CU (of `waves` wavefronts
// and `lds` bytes each) and of a launch, and the launch of
// L.c.count codeblocks (d_order: codeblocks d_order[0 .. count) of the arrays, null: the first count). d_rdm / rm_in with FUSED only.
size_t   miphy_ldpc_pk_lds_bytes(int bgi, int lay, size_t Zt, int pairs_all, int parts = 1);
int      miphy_ldpc_pk_waves_per_cu(bool fused, int parts = 1);
int      miphy_ldpc_pk_per_cu(size_t lds, int waves, bool fused, int parts = 1);
uint32_t miphy_ldpc_pk_grid(const miphy_ctx* ctx, uint32_t n, int threads, size_t lds, bool fused, int parts = 1);
int      miphy_ldpc_pk_launch(miphy_ctx* ctx, const miphy_ldpc_launch& L, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order,
                              const int8_t* llr, uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot, uint8_t* harq_crc_ok,
                              const miphy_ldpc_rdm_desc* d_rdm, const int8_t* rm_in, void* gmsg, hipStream_t s);
#endif

// A device scratch buffer of at least `bytes` in the context's workspace `slot`. A slot that has to grow gets a new block of at least
// twice the size; the old one is kept until miphy_destroy (work enqueued or captured earlier may still use it), so nothing waits.
int miphy_get_workspace(miphy_ctx* ctx, miphy_workspace slot, size_t bytes, void** out);

// Factors of the four-step DFT sizes 4608 ... 49152 (ofdm.hip; both multiples of the 16-wide tile of fft_device.h's step 1); false for any other size.
bool miphy_four_step_factors(uint32_t N, uint32_t& N1, uint32_t& N2);

// The context's side streams and fork / join events, created on first use (before a run of a table that uses them).
int miphy_side_streams(miphy_ctx* ctx);
// The next work-queue counter of the context (zero: every launch leaves its counter cleared).
int miphy_next_queue_counter(miphy_ctx* ctx, uint32_t** out);

// ---- device buffers laid out with device_image.h ----
#include "device_image.h"
#include <memory>
// Owner of one hipMalloc block (move only): the block is freed with its owner.
struct miphy_hip_free {
  void operator()(void* p) const { (void)hipFree(p); }
};
using miphy_device_block = std::unique_ptr<void, miphy_hip_free>;
// A block of img.total_bytes() with the staged part copied into it (the call waits for the copy): what a prepared plan keeps.
// MIPHY_EHIP and a message that begins with `who` when the allocation or the copy fails; nothing is left allocated then.
int miphy_image_to_block(const char* who, const device_image& img, miphy_device_block& out);
// Per call: the image in the context's workspace `slot`, its staged part uploaded on `s` (miphy_upload).
int miphy_image_to_workspace(miphy_ctx* ctx, miphy_workspace slot, const device_image& img, hipStream_t s, void** base);
// Per call, an image of staged arrays only: in the staging ring (miphy_stage_descs).
int miphy_image_to_ring(miphy_ctx* ctx, const device_image& img, hipStream_t s, const void** base);
