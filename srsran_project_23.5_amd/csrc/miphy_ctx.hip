// Context: device tables (TS 38.212 graphs, CRC constants), descriptor staging, error reporting.
#include "miphy_internal.h"
#include "miphy_ext.h"
#include "tables/nr_ldpc_tables.h"
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <new>

static thread_local char g_err[512] = "";

void miphy_set_error(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* miphy_last_error(void)
{
  return g_err;
}

extern "C" int miphy_version(void)
{
  return MIPHY_VERSION;
}

static int lifting_set(int Z)
{
  static const int A[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  for (int i = 7; i >= 0; --i) {
    if (Z % A[i])
      continue;
    int q = Z / A[i];
    if ((q & (q - 1)) == 0)
      return i;
  }
  return -1;
}

static uint32_t gf2_mulmod(uint32_t a, uint32_t b, uint32_t poly, unsigned order)
{
  // a*b mod poly over GF(2), operands < 2^order.
  uint32_t r = 0, top = 1u << order;
  for (int i = (int)order - 1; i >= 0; --i) {
    r <<= 1;
    if (r & top)
      r ^= poly;
    if ((b >> i) & 1u)
      r ^= a;
  }
  return r;
}

// What the decoders' first iteration takes for granted about the first three layers of a base graph (update_rows_pk_zero,
// ldpc_pk_device.h): layer 0 holds the punctured columns 0 and 1; layer 1 has column 0 as its edge 0, no column 1 and degree d1;
// layer 2 has columns 0 and 1 as its edges 0 and 1, nowhere else, and degree d2. Checked when a context is made (the generated tables
// are plain const arrays, which a static_assert cannot read): with a table that stops saying so, miphy_create fails.
static bool first_layers_as_decoded(const uint16_t* row_start, const uint8_t* col, int d1, int d2)
{
  bool has0 = false, has1 = false;
  for (int e = row_start[0]; e < row_start[1]; ++e)
    has0 |= col[e] == 0, has1 |= col[e] == 1;
  bool ok = has0 && has1 && row_start[2] - row_start[1] == d1 && row_start[3] - row_start[2] == d2;
  ok &= col[row_start[1]] == 0 && col[row_start[2]] == 0 && col[row_start[2] + 1] == 1;
  for (int e = row_start[1] + 1; e < row_start[2]; ++e)
    ok &= col[e] > 1;
  for (int e = row_start[2] + 2; e < row_start[3]; ++e)
    ok &= col[e] > 1;
  return ok;
}

static void build_tables(miphy_graph_tables* t)
{
  memset(t, 0, sizeof(*t));
  for (int z = 0; z <= MIPHY_MAX_Z; ++z) {
    t->z_pos[z] = 0xffff;
    t->i_ls[z]  = 0xff;
  }
  for (int p = 0; p < MIPHY_NOF_Z; ++p) {
    int Z        = NR_LDPC_LIFTING_SIZES[p];
    t->z_pos[Z]  = (uint16_t)p;
    int ils      = lifting_set(Z);
    t->i_ls[Z]   = (uint8_t)ils;
    for (int e = 0; e < NR_LDPC_BG1_NOF_EDGES; ++e)
      t->edge[0][p][e] = (uint32_t)(NR_LDPC_BG1_COL[e] * Z) | ((uint32_t)(NR_LDPC_BG1_SHIFT[ils][e] % Z) << 16);
    for (int e = 0; e < NR_LDPC_BG2_NOF_EDGES; ++e)
      t->edge[1][p][e] = (uint32_t)(NR_LDPC_BG2_COL[e] * Z) | ((uint32_t)(NR_LDPC_BG2_SHIFT[ils][e] % Z) << 16);
  }
  for (int b = 0; b < 2; ++b)
    for (int p = 0; p < MIPHY_NOF_Z; ++p)
      for (int e = 0; e < (b ? NR_LDPC_BG2_NOF_EDGES : NR_LDPC_BG1_NOF_EDGES); ++e) {
        t->edge_sb[b][p][2 * e]     = t->edge[b][p][e] >> 16;
        t->edge_sb[b][p][2 * e + 1] = t->edge[b][p][e] & 0xffffu;
      }
  for (int m = 0; m <= NR_LDPC_BG1_M; ++m)
    t->row_start[0][m] = NR_LDPC_BG1_ROW_START[m];
  for (int m = 0; m <= NR_LDPC_BG2_M; ++m)
    t->row_start[1][m] = NR_LDPC_BG2_ROW_START[m];
  for (int b = 0; b < 2; ++b) {
    t->pair_start[b][0] = 0;
    for (int m = 0; m < (b ? NR_LDPC_BG2_M : NR_LDPC_BG1_M); ++m)
      t->pair_start[b][m + 1] = (uint16_t)(t->pair_start[b][m] + (t->row_start[b][m + 1] - t->row_start[b][m] + 1) / 2);
  }
  static const uint32_t POLY[5]  = {0x1864CFB, 0x1800063, 0x1B2B117, 0x11021, 0xE21};
  static const uint32_t ORDER[5] = {24, 24, 24, 16, 11};
  for (int p = 0; p < 5; ++p) {
    t->crc_poly[p]  = POLY[p];
    t->crc_order[p] = ORDER[p];
    // x^32 mod poly
    uint32_t x32 = 1, top = 1u << ORDER[p];
    for (int i = 0; i < 32; ++i) {
      x32 <<= 1;
      if (x32 & top)
        x32 ^= POLY[p];
    }
    uint32_t v = 1;
    for (int k = 0; k < 320; ++k) {
      t->crc_pow32[p][k] = v;
      v                  = gf2_mulmod(v, x32, POLY[p], ORDER[p]);
    }
    {
      const uint32_t x8192 = gf2_mulmod(t->crc_pow32[p][255], x32, POLY[p], ORDER[p]); // x^(32*256)
      uint32_t       h     = 1;
      for (int k = 0; k < 256; ++k) {
        t->crc_pow32_hi[p][k] = h;
        h                     = gf2_mulmod(h, x8192, POLY[p], ORDER[p]);
      }
    }
    v = x32;
    for (int b = 0; b < 24; ++b) {
      t->crc_pow2[p][b] = v;
      v                 = gf2_mulmod(v, v, POLY[p], ORDER[p]);
    }
    const int zi = miphy_crc_zmask_index(p);
    if (zi >= 0) {
      // weight of the bit at distance j from the end of the message: x^(j + order) mod P
      uint32_t c = 1;
      for (unsigned i = 0; i < ORDER[p]; ++i) {
        c <<= 1;
        if (c & top)
          c ^= POLY[p];
      }
      for (int u = 0; u < MIPHY_CRC_ZMASK_WORDS; ++u)
        for (int jl = 0; jl < 32; ++jl) { // j = 32 u + jl
          const int i_local = 31 - jl;
          for (unsigned k = 0; k < ORDER[p]; ++k)
            if ((c >> k) & 1u) {
              t->crc_zmask[zi][u][k] |= 1u << jl;
              if (p == 0)
                t->crc_zmask_packed24a[u][k] |= 1u << (8 * (i_local >> 3) + 7 - (i_local & 7));
            }
          c <<= 1;
          if (c & top)
            c ^= POLY[p];
        }
    }
  }
}

// The arithmetic of pk_edge_addresses<D, true> (ldpc_pk_device.h) with base = 0, for every lane, layer and edge.
extern "C" int miphy_ldpc_address_table(int bg, int Z, int layers, uint32_t* out)
{
  MIPHY_REQUIRE(bg == 1 || bg == 2, "miphy_ldpc_address_table: invalid base graph %d", bg);
  MIPHY_REQUIRE(Z >= 2 && Z <= MIPHY_MAX_Z && lifting_set(Z) >= 0, "miphy_ldpc_address_table: invalid lifting size %d", Z);
  MIPHY_REQUIRE(layers >= 1 && layers <= (bg == 1 ? NR_LDPC_BG1_M : NR_LDPC_BG2_M), "miphy_ldpc_address_table: invalid number of layers %d", layers);
  const uint16_t* row_start = bg == 1 ? NR_LDPC_BG1_ROW_START : NR_LDPC_BG2_ROW_START;
  const uint8_t*  col       = bg == 1 ? NR_LDPC_BG1_COL : NR_LDPC_BG2_COL;
  const int       ils = lifting_set(Z), H = (Z + 1) / 2, lanes = 64 * ((H + 63) / 64);
  size_t          quad = 0;
  for (int m = 0; m < layers; ++m) {
    const int e0 = row_start[m], d = row_start[m + 1] - e0, nq = (d + 3) / 4;
    if (out) {
      for (int j = 0; j < 4 * nq; ++j) {
        const int      e  = e0 + std::min(j, d - 1); // a pad entry repeats the last edge
        const uint32_t sh = (uint32_t)((bg == 1 ? NR_LDPC_BG1_SHIFT[ils][e] : NR_LDPC_BG2_SHIFT[ils][e]) % Z), co = (uint32_t)col[e] * Z;
        for (int l = 0; l < lanes; ++l) {
          uint32_t w = 0;
          if (l < H) {
            const uint16_t Hv = (l + H < Z) ? (uint16_t)H : 0; // odd Z: the last lane's second row is its first
            const uint16_t tA = (uint16_t)(l + sh), tB = (uint16_t)(l + Hv + sh);
            const uint16_t rA = std::min<uint16_t>(tA, (uint16_t)(tA - Z)), rB = std::min<uint16_t>(tB, (uint16_t)(tB - Z));
            w                 = ((uint32_t)rA + co) | (((uint32_t)rB + co) << 16);
          }
          out[((quad + j / 4) * lanes + l) * 4 + j % 4] = w;
        }
      }
    }
    quad += nq;
  }
  return (int)(quad * lanes * 4);
}

int miphy_ldpc_address_tables(miphy_ctx* ctx, int bgi, int lay, int min_Z, int max_Z, const void** out)
{
  constexpr int    NZ = MIPHY_MAX_Z / 16 + 1;
  ldpc_adr_tables& T  = ctx->ext->ldpc_adr[{bgi, lay}];
  if (!T.d_ptr) {
    const void* none[NZ] = {};
    if (int rc = miphy_keep_device_copy(ctx, none, sizeof(none), (void**)&T.d_ptr))
      return rc;
  }
  for (int Z = min_Z; Z <= max_Z; ++Z) {
    if (ctx->h_tables->z_pos[Z] == 0xffff || T.h_ptr[Z / 16])
      continue;
    MIPHY_REQUIRE(Z % 16 == 0, "ldpc address tables: lifting size %d has no table index of its own", Z); // (every size from 128 on has)
    const int words = miphy_ldpc_address_table(bgi + 1, Z, lay, nullptr);
    if (words < 0)
      return words;
    std::vector<uint32_t> h((size_t)words);
    (void)miphy_ldpc_address_table(bgi + 1, Z, lay, h.data());
    void* d = nullptr;
    if (int rc = miphy_keep_device_copy(ctx, h.data(), h.size() * 4, &d))
      return rc;
    MIPHY_HIP_CHECK(hipMemcpy(T.d_ptr + Z / 16, &d, sizeof(void*), hipMemcpyHostToDevice)); // (an entry no launch in flight reads: its key was not held)
    T.h_ptr[Z / 16] = d;
  }
  *out = T.d_ptr;
  return MIPHY_OK;
}

extern "C" int miphy_create(int device, miphy_ctx** out)
{
  if (!out) {
    miphy_set_error("miphy_create: null out pointer");
    return MIPHY_EINVAL;
  }
  *out = nullptr;
  MIPHY_REQUIRE(first_layers_as_decoded(NR_LDPC_BG1_ROW_START, NR_LDPC_BG1_COL, 19, 19) && first_layers_as_decoded(NR_LDPC_BG2_ROW_START, NR_LDPC_BG2_COL, 10, 8),
                "miphy_create: layers 0-2 of the LDPC base graph tables are not what the decoders' first iteration relies on");
  MIPHY_HIP_CHECK(hipSetDevice(device));
  miphy_ctx* c = new (std::nothrow) miphy_ctx();
  if (!c)
    return MIPHY_ENOMEM;
  c->device   = device;
  c->num_cus  = 256;
  (void)hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device);
  c->ext      = new miphy_ctx_ext();
  c->h_tables = (miphy_graph_tables*)malloc(sizeof(miphy_graph_tables));
  build_tables(c->h_tables);
  MIPHY_HIP_CHECK(hipMalloc((void**)&c->d_tables, sizeof(miphy_graph_tables)));
  MIPHY_HIP_CHECK(hipMemcpy(c->d_tables, c->h_tables, sizeof(miphy_graph_tables), hipMemcpyHostToDevice));
  c->desc_staging_bytes = 8u << 20;
  c->staging_head       = 0;
  MIPHY_HIP_CHECK(hipMalloc(&c->d_desc_staging, c->desc_staging_bytes));
  MIPHY_HIP_CHECK(hipHostMalloc(&c->h_desc_staging, c->desc_staging_bytes, hipHostMallocDefault));
  MIPHY_HIP_CHECK(hipMalloc((void**)&c->d_queue, MIPHY_NOF_QUEUE_COUNTERS * sizeof(uint32_t)));
  MIPHY_HIP_CHECK(hipMemset(c->d_queue, 0, MIPHY_NOF_QUEUE_COUNTERS * sizeof(uint32_t)));
  c->queue_next = 0;
  *out = c;
  return MIPHY_OK;
}

extern "C" void miphy_destroy(miphy_ctx* c)
{
  if (!c)
    return;
  (void)hipSetDevice(c->device);
  (void)hipFree(c->d_tables);
  for (void* p : c->ext->to_free)
    (void)hipFree(p);
  delete c->ext;
  for (int k = 0; k < MIPHY_NOF_SIDE_STREAMS; ++k) {
    if (c->side_stream[k])
      (void)hipStreamDestroy((hipStream_t)c->side_stream[k]);
    if (c->ev_join[k])
      (void)hipEventDestroy((hipEvent_t)c->ev_join[k]);
  }
  if (c->ev_fork)
    (void)hipEventDestroy((hipEvent_t)c->ev_fork);
  (void)hipFree(c->d_desc_staging);
  (void)hipFree(c->d_queue);
  for (void* w : c->d_work)
    (void)hipFree(w);
  (void)hipHostFree(c->h_desc_staging);
  free(c->h_tables);
  delete c;
}

int miphy_side_streams(miphy_ctx* ctx)
{
  if (ctx->ev_fork)
    return MIPHY_OK;
  for (int k = 0; k < MIPHY_NOF_SIDE_STREAMS; ++k) {
    hipStream_t st = nullptr;
    hipEvent_t  e  = nullptr;
    MIPHY_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    MIPHY_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->side_stream[k] = st, ctx->ev_join[k] = e;
  }
  hipEvent_t f = nullptr;
  MIPHY_HIP_CHECK(hipEventCreateWithFlags(&f, hipEventDisableTiming));
  ctx->ev_fork = f;
  return MIPHY_OK;
}

int miphy_next_queue_counter(miphy_ctx* ctx, uint32_t** out)
{
  // A launch owns its counter until MIPHY_NOF_QUEUE_COUNTERS later launches of this context have been enqueued. The counters are
  // zero when the context is created and every launch leaves its counter at zero (the workgroup that draws the last ticket).
  *out = ctx->d_queue + (ctx->queue_next++ % MIPHY_NOF_QUEUE_COUNTERS);
  return MIPHY_OK;
}

// Front-to-back allocation in the staging ring. Regions handed out since the last wrap are never overwritten; on a wrap every
// consumer of the old regions must be done. The consumers run on the streams the regions were staged for, so the wrap waits for
// THOSE streams (up to four are remembered between wraps; more than that falls back to the device-wide wait) -- not for the other
// contexts and cells that share the device -- once per desc_staging_bytes of descriptors, not once per call. A stream that is being
// captured cannot be waited for: the wrap then fails with MIPHY_EUNSUPP (capture with device-resident descriptors or a prepared plan).
static int staging_take(miphy_ctx* ctx, size_t bytes, hipStream_t s, size_t* off)
{
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (ctx->staging_head + need > ctx->desc_staging_bytes) {
    if (ctx->nof_ring_streams > 4) {
      MIPHY_HIP_CHECK(hipDeviceSynchronize());
    } else {
      for (int i = 0; i < ctx->nof_ring_streams; ++i) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (ctx->ring_streams[i] && hipStreamIsCapturing((hipStream_t)ctx->ring_streams[i], &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
          miphy_set_error("descriptor staging ring wrapped while a stream that consumes it is being captured");
          return MIPHY_EUNSUPP;
        }
        MIPHY_HIP_CHECK(hipStreamSynchronize((hipStream_t)ctx->ring_streams[i]));
      }
    }
    ctx->staging_head     = 0;
    ctx->nof_ring_streams = 0;
  }
  int k = 0;
  while (k < ctx->nof_ring_streams && k < 4 && ctx->ring_streams[k] != (void*)s)
    ++k;
  if (k == ctx->nof_ring_streams || k == 4) {
    if (k < 4)
      ctx->ring_streams[k] = (void*)s;
    ctx->nof_ring_streams = k < 4 ? k + 1 : 5;
  }
  *off = ctx->staging_head;
  ctx->staging_head += need;
  return MIPHY_OK;
}

int miphy_stage_descs(miphy_ctx* ctx, const void* descs, int on_device, size_t bytes, hipStream_t s, const void** out)
{
  if (on_device) {
    *out = descs;
    return MIPHY_OK;
  }
  MIPHY_REQUIRE(bytes <= ctx->desc_staging_bytes, "descriptor batch too large (%zu bytes > %zu)", bytes, ctx->desc_staging_bytes);
  size_t off = 0;
  int    rc  = staging_take(ctx, bytes, s, &off);
  if (rc)
    return rc;
  uint8_t* h = static_cast<uint8_t*>(ctx->h_desc_staging) + off;
  uint8_t* d = static_cast<uint8_t*>(ctx->d_desc_staging) + off;
  memcpy(h, descs, bytes);
  MIPHY_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  *out = d;
  return MIPHY_OK;
}

int miphy_upload(miphy_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s)
{
  if (bytes == 0)
    return MIPHY_OK;
  if (bytes > ctx->desc_staging_bytes / 2) {
    MIPHY_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    MIPHY_HIP_CHECK(hipStreamSynchronize(s)); // `src` may be pageable or about to go out of scope
    return MIPHY_OK;
  }
  size_t off = 0;
  int    rc  = staging_take(ctx, bytes, s, &off);
  if (rc)
    return rc;
  uint8_t* h = static_cast<uint8_t*>(ctx->h_desc_staging) + off;
  memcpy(h, src, bytes);
  MIPHY_HIP_CHECK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, s));
  return MIPHY_OK;
}

int miphy_get_workspace(miphy_ctx* ctx, miphy_workspace slot, size_t bytes, void** out)
{
  if (bytes > ctx->work_bytes[slot]) {
    // the old block stays valid for what was enqueued or captured with it: freed in miphy_destroy. Doubling keeps the blocks held back
    // smaller than the live one together.
    const size_t want = std::max(bytes + bytes / 4 + (1u << 20), 2 * ctx->work_bytes[slot]);
    void*        w    = nullptr;
    MIPHY_HIP_CHECK(hipMalloc(&w, want));
    if (ctx->d_work[slot])
      ctx->ext->to_free.push_back(ctx->d_work[slot]);
    ctx->d_work[slot]     = w;
    ctx->work_bytes[slot] = want;
  }
  *out = ctx->d_work[slot];
  return MIPHY_OK;
}

int miphy_image_to_block(const char* who, const device_image& img, miphy_device_block& out)
{
  MIPHY_REQUIRE(img.ok(), "%s: an array was appended to the device image behind its reserved regions", who);
  const std::vector<uint8_t> host = img.staged();
  void*                      d = nullptr;
  hipError_t                 e = hipMalloc(&d, img.total_bytes());
  miphy_device_block         blk(e == hipSuccess ? d : nullptr);
  if (e == hipSuccess)
    e = hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    miphy_set_error("%s: device buffer of %zu bytes (%zu uploaded) -> %s", who, img.total_bytes(), host.size(), hipGetErrorString(e));
    return MIPHY_EHIP;
  }
  out = std::move(blk);
  return MIPHY_OK;
}

int miphy_image_to_workspace(miphy_ctx* ctx, miphy_workspace slot, const device_image& img, hipStream_t s, void** base)
{
  MIPHY_REQUIRE(img.ok(), "workspace %d: an array was appended to the device image behind its reserved regions", (int)slot);
  if (int rc = miphy_get_workspace(ctx, slot, img.total_bytes(), base))
    return rc;
  const std::vector<uint8_t> host = img.staged();
  return miphy_upload(ctx, *base, host.data(), host.size(), s); // through the pinned ring: the stream is not waited for
}

int miphy_image_to_ring(miphy_ctx* ctx, const device_image& img, hipStream_t s, const void** base)
{
  MIPHY_REQUIRE(img.ok() && img.total_bytes() == img.staged_bytes(), "staging ring: the device image holds more than staged arrays");
  const std::vector<uint8_t> host = img.staged();
  return miphy_stage_descs(ctx, host.data(), 0, host.size(), s, base);
}

int miphy_keep_device_copy(miphy_ctx* ctx, const void* src, size_t bytes, void** out)
{
  void* d = nullptr;
  MIPHY_HIP_CHECK(hipMalloc(&d, bytes ? bytes : 1));
  const hipError_t e = bytes ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  if (e != hipSuccess) {
    (void)hipFree(d);
    MIPHY_HIP_CHECK(e);
  }
  ctx->ext->to_free.push_back(d);
  *out = d;
  return MIPHY_OK;
}

#include "gold_device.h"
int miphy_get_gold_tables(miphy_ctx* ctx, const gold_tables** out)
{
  if (!ctx->ext->d_gold) {
    std::unique_ptr<gold_tables> t(new gold_tables);
    gold_tables_init(*t);
    if (int rc = miphy_keep_device_copy(ctx, t.get(), sizeof(gold_tables), &ctx->ext->d_gold))
      return rc;
  }
  if (out)
    *out = (const gold_tables*)ctx->ext->d_gold;
  return MIPHY_OK;
}
