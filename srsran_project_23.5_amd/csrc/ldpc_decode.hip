// LDPC decoder, host side: from descriptors to kernel launches. The kernels live in files of their own, each with its LDS formula, its
// geometry and its launch: ldpc_decode_row.hip (one check row per lane), ldpc_decode_pk.hip (two rows per lane, one codeblock per
// workgroup), ldpc_decode_pkw.hip (Z <= 64, several codeblocks per wavefront). Top to bottom:
//   * the debug knobs;
//   * launch classes: a batch the host can see is sorted into classes that share a workgroup size and an LDS size
//     (miphy_ldpc_build_classes);
//   * the launch table, one launch per class (miphy_ldpc_plan_launches), or ONE launch for a batch the host cannot sort;
//   * enqueueing a table (miphy_ldpc_run_launches);
//   * the entry points: per call (miphy_ldpc_decode_batch) and prepared (miphy_ldpc_decode_plan_*).
#include "miphy_internal.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef LDPC_HYBRID_LDS_MARGIN
#define LDPC_HYBRID_LDS_MARGIN 2048
#endif

namespace {
// Debug knobs. Setters may run on any thread; whoever makes a launch table takes ONE snapshot and decides everything from it.
struct ldpc_knob_values {
  int  force;         // miphy_ldpc_force_mode (miphy_debug_force_ldpc_kernel, low byte)
  bool hybrid_msgs;   // false (mode | MIPHY_LDPC_FORCE_ALL_GMSG): all messages of a GMSG launch in global memory
  int  class_streams; // streams the launch classes of a call are spread over (miphy_debug_set_ldpc_class_streams)
  bool adr_tables;    // false (mode | MIPHY_LDPC_FORCE_NO_ADR_TABLE): every launch computes its soft-bit addresses
  bool row_skip;      // false (mode | MIPHY_LDPC_FORCE_NO_ROW_SKIP): every wavefront of the packed kernel runs every layer visit
};
struct {
  std::atomic<int>  force{MIPHY_LDPC_FORCE_AUTO};
  std::atomic<bool> hybrid_msgs{true};
  std::atomic<int>  class_streams{1 + MIPHY_NOF_SIDE_STREAMS};
  std::atomic<bool> adr_tables{true};
  std::atomic<bool> row_skip{true};
  ldpc_knob_values  snapshot() const { return {force.load(), hybrid_msgs.load(), class_streams.load(), adr_tables.load(), row_skip.load()}; }
} g_knobs;
std::atomic<unsigned> g_kernels_used{0}; // MIPHY_LDPC_KERNEL_* of every decoder launch since the last reset (miphy_debug_ldpc_kernels_used)
std::atomic<unsigned> g_adr_table_launches{0}; // launches of the address-table instance since the last reset
std::atomic<unsigned> g_row_skip_launches{0};  // launches of an instance that leaves out the visits of saturated rows
} // namespace

extern "C" void miphy_debug_force_ldpc_kernel(int mode)
{
  g_knobs.force       = mode & MIPHY_LDPC_FORCE_MODE_MASK;
  g_knobs.hybrid_msgs = !(mode & MIPHY_LDPC_FORCE_ALL_GMSG);
  g_knobs.adr_tables  = !(mode & MIPHY_LDPC_FORCE_NO_ADR_TABLE);
  g_knobs.row_skip    = !(mode & MIPHY_LDPC_FORCE_NO_ROW_SKIP);
}

extern "C" void miphy_debug_set_ldpc_class_streams(int n)
{
  g_knobs.class_streams = std::min(std::max(n, 1), 1 + MIPHY_NOF_SIDE_STREAMS);
}

extern "C" unsigned miphy_debug_ldpc_kernels_used(int reset)
{
  return reset ? g_kernels_used.exchange(0) : g_kernels_used.load();
}

extern "C" unsigned miphy_debug_ldpc_row_skip_launches(int reset)
{
  return reset ? g_row_skip_launches.exchange(0) : g_row_skip_launches.load();
}

extern "C" unsigned miphy_debug_ldpc_address_table_launches(int reset)
{
  return reset ? g_adr_table_launches.exchange(0) : g_adr_table_launches.load();
}

// ---- class-sorted launches ------------------------------------------------------------------------------------------------------
// The reference decoder scales its work with the lifting size of each codeblock (ldpc_decoder_avx2.cpp:59-64). A launch has ONE
// workgroup size and ONE LDS size, so a batch that mixes lifting sizes and code rates is sorted on the host into classes that share
// both, and every class gets a launch of its own:
//   * kind 0: Z <= 64 -- the wave kernel (ldpc_decode_pkw.hip), several codeblocks of one (base graph, Z) per wavefront;
//   * kind 1..3: the packed kernel with 1, 2 or 3 wavefronts per codeblock (Z <= 128 / 256 / 384);
//   * per base graph and per bucket of reachable layers (LDS per codeblock, hence codeblocks per CU, follows the layers);
//   * codeblocks the decoder can rate-dematch while it loads (first transmissions, see sch.hip) apart from those it cannot.
static int layer_bucket(int lay)
{
  static const int bound[6] = {4, 6, 10, 16, 26, 46};
  int              b        = 0;
  while (lay > bound[b])
    ++b;
  return b;
}

void miphy_ldpc_build_classes(const miphy_ldpc_dec_desc* descs, uint32_t n, const uint8_t* fusable, miphy_ldpc_classes& C)
{
  struct item {
    uint64_t key;
    uint32_t idx;
  };
  std::vector<item> it(n);
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_ldpc_dec_desc& d   = descs[i];
    const int                  bgi   = d.bg == 1 ? 0 : 1;
    const int                  lay   = miphy_ldpc_layers(bgi, miphy_ldpc_nodes(d.in_len, d.Z));
    const int                  H     = (d.Z + 1) / 2;
    const int                  kind  = d.Z <= 64 ? 0 : (H + 63) / 64;
    const bool                 fus   = fusable && fusable[i] && kind != 0;
    // class: fused | kind | base graph | layer bucket; below it the fields a bundle of the wave kernel must share; then the layer bound
    uint64_t key = ((uint64_t)(fus ? 1 : 0) << 63) | ((uint64_t)kind << 61) | ((uint64_t)bgi << 60) | ((uint64_t)layer_bucket(lay) << 57);
    if (kind == 0)
      key |= ((uint64_t)d.Z << 40) | ((uint64_t)(d.crc_poly & 0xff) << 32) | ((uint64_t)(d.flags & 1u) << 31) | ((uint64_t)d.max_iter << 8);
    key |= (uint64_t)lay; // 6 bits, read back below
    it[i].key = key, it[i].idx = i;
  }
  std::stable_sort(it.begin(), it.end(), [](const item& a, const item& b) { return (a.key >> 8) < (b.key >> 8); });
  C.order.resize(n);
  C.bundles.clear();
  C.classes.clear();
  C.nof_unfused = 0;
  C.identity    = true;
  const uint64_t class_mask = ~(uint64_t)0 << 57;
  for (uint32_t p = 0; p < n;) {
    uint32_t q = p;
    while (q < n && (it[q].key & class_mask) == (it[p].key & class_mask))
      ++q;
    miphy_ldpc_class c = {};
    c.fused            = (uint8_t)(it[p].key >> 63);
    c.kind             = (uint8_t)((it[p].key >> 61) & 3);
    c.bgi              = (uint8_t)((it[p].key >> 60) & 1);
    c.first = p, c.count = q - p;
    c.min_Z        = 0xffff;
    c.bundle_first = (uint32_t)C.bundles.size() / 2;
    for (uint32_t k = p; k < q; ++k) {
      const miphy_ldpc_dec_desc& d = descs[it[k].idx];
      c.lay                        = std::max<uint8_t>(c.lay, (uint8_t)(it[k].key & 63));
      c.max_Z                      = std::max<uint16_t>(c.max_Z, d.Z);
      c.min_Z                      = std::min<uint16_t>(c.min_Z, d.Z);
      c.runs_all_iterations |= (d.crc_poly == MIPHY_CRC_NONE || (d.flags & 1u)) ? 1 : 0;
      C.order[k]                   = it[k].idx;
      C.identity &= it[k].idx == k;
    }
    if (!c.fused)
      C.nof_unfused += c.count;
    if (c.kind == 0) {
      for (uint32_t k = p; k < q;) { // bundles: runs of identical (Z, CRC, mode, iterations), G codeblocks at most
        const miphy_ldpc_dec_desc& d = descs[it[k].idx];
        const uint32_t             G = 64u / ((d.Z + 1u) / 2u);
        uint32_t                   e = k;
        while (e < q && e - k < G && ((it[e].key ^ it[k].key) >> 8) == 0)
          ++e;
        C.bundles.push_back(k);
        C.bundles.push_back(e - k);
        const uint32_t sstride = (uint32_t)miphy_ldpc_soft_bytes(c.bgi, c.lay, d.Z);
        c.soft_total           = std::max(c.soft_total, G * sstride);
        k                      = e;
      }
    }
    c.bundle_count = (uint32_t)C.bundles.size() / 2 - c.bundle_first;
    C.classes.push_back(c);
    p = q;
  }
}

namespace {
// A class of the packed kernel: message placement, throughput or latency form, grid.
void pk_class_geometry(const miphy_ctx* ctx, const ldpc_knob_values& k, bool fuse, miphy_ldpc_launch& q)
{
  const miphy_ldpc_class& c     = q.c;
  const bool              fused = c.fused && fuse;
  const int               pairs = ctx->h_tables->pair_start[c.bgi][c.lay];
  const size_t lds_l = miphy_ldpc_pk_lds_bytes(c.bgi, c.lay, c.max_Z, pairs), lds_g = miphy_ldpc_pk_lds_bytes(c.bgi, c.lay, c.max_Z, 0);
  // messages in LDS while that keeps as many codeblocks resident per CU as the registers allow; otherwise in global memory
  auto per_cu = [&](size_t lds) { return miphy_ldpc_pk_per_cu(lds, c.kind, fused); };
  // (and only where the class has more codeblocks than stay resident with the messages in LDS: otherwise the global round trip per
  // layer visit buys nothing)
  bool gm = per_cu(lds_g) > per_cu(lds_l) && (k.force == MIPHY_LDPC_FORCE_THROUGHPUT || c.count > (uint32_t)(ctx->num_cus * per_cu(lds_l)));
  q.lds   = gm ? lds_g : lds_l;
  // Only as many layers' messages leave LDS as that residency needs: the first layers keep theirs (a lane's messages are private to it,
  // so the split is free), the global round trip and its L2 traffic are paid for the rest.
  if (gm && k.force != MIPHY_LDPC_FORCE_THROUGHPUT && k.hybrid_msgs) {
    for (int m = c.lay - 1; m > 0; --m) {
      const int    pk_ = ctx->h_tables->pair_start[c.bgi][m];
      const size_t l_  = miphy_ldpc_pk_lds_bytes(c.bgi, c.lay, c.max_Z, pk_);
      if (per_cu(l_ + LDPC_HYBRID_LDS_MARGIN) == per_cu(lds_g)) { // (margin: a CU filled to the last byte of the sum held one workgroup fewer -- allocation granularity)
        q.lds_pairs = pk_, q.lds = l_;
        break;
      }
    }
  }
  // Latency form where the class cannot fill the chip anyway (at most one codeblock per CU): twice the wavefronts per codeblock,
  // messages in LDS (residency is no concern then).
  // (four parts while the codeblocks of the class still find a CU each and the workgroup stays within 1024 threads; forced latency modes: two)
  const int    parts = (k.force == MIPHY_LDPC_FORCE_LATENCY_ALL || k.force == MIPHY_LDPC_FORCE_LATENCY2) ? 2 : 4;
  const size_t lds_s = miphy_ldpc_pk_lds_bytes(c.bgi, c.lay, c.max_Z, pairs, parts);
  if (k.force != MIPHY_LDPC_FORCE_THROUGHPUT && (c.count <= (uint32_t)ctx->num_cus || k.force == MIPHY_LDPC_FORCE_LATENCY_ALL) && lds_s <= (size_t)160 * 1024)
    q.parts = parts, gm = false, q.lds = lds_s, q.lds_pairs = 0;
  q.threads    = 64 * c.kind * q.parts;
  q.gmsg_pairs = gm ? pairs - q.lds_pairs : 0;
  q.grid       = miphy_ldpc_pk_grid(ctx, c.count, q.threads, q.lds, fused, q.parts);
  q.gmsg_bytes = gm ? (size_t)q.grid * (q.threads / 64) * (size_t)q.gmsg_pairs * 256 : 0;
  q.used       = MIPHY_LDPC_KERNEL_PACKED | (fused ? MIPHY_LDPC_KERNEL_FUSED : 0u) | (gm ? MIPHY_LDPC_KERNEL_GMSG : 0u) |
           (q.parts > 1 ? MIPHY_LDPC_KERNEL_SPLIT : 0u) | ((gm && q.lds_pairs > 0) ? MIPHY_LDPC_KERNEL_GMSG_PART : 0u);
  // Soft-bit addresses from a table (ldpc_pk_device.h, pk_table_addresses): the throughput form that dematches, messages in LDS, where every
  // layer the class can reach has the degree the instance is built for (BG1 up to four layers: high-rate codeblocks) and every lifting size a
  // table index of its own (multiples of 16: all sizes from 128 on). Every other class computes its addresses.
  bool one_degree = true;
  for (int m = 0; m < c.lay; ++m)
    one_degree &= ctx->h_tables->row_start[c.bgi][m + 1] - ctx->h_tables->row_start[c.bgi][m] == MIPHY_LDPC_ADR_TABLE_DEGREE;
  q.atab = k.adr_tables && fused && !gm && q.parts == 1 && one_degree && c.min_Z >= 128;
  // The instance that leaves out the visits of saturated rows (ldpc_decode_pk.hip, RSKIP) where the launch can profit: the throughput form
  // (the parts of the latency form share a layer's rows), codeblocks that run all their iterations (one that stops at its first good
  // checksum leaves before its rows saturate -- a row counts as saturated from the visit that WRITES infinite soft bits only), messages in LDS (the classes with messages in global memory are the low rates: most of their
  // layers hold a parity column with a single check, whose soft bit stays finite unless the channel value itself is clipped). The layer
  // loop of that instance compiles to slower visits, so every other launch keeps the instance without it.
  q.row_skip = k.row_skip && q.parts == 1 && !gm && c.runs_all_iterations;
}

void plan_classes(const miphy_ctx* ctx, const miphy_ldpc_classes& C, bool fuse, const ldpc_knob_values& k, miphy_ldpc_launches& T)
{
  const size_t nc = C.classes.size();
  T               = miphy_ldpc_launches{};
  T.scalar        = k.force == MIPHY_LDPC_FORCE_ROW;
  T.l.resize(nc);
  // Geometry of every class first: the launches of one call run side by side, so each needs message scratch of its own.
  for (size_t i = 0; i < nc; ++i) {
    miphy_ldpc_launch& q = T.l[i];
    q.c                  = C.classes[i];
    q.nodes              = miphy_bg_K(q.c.bgi) + q.c.lay;
    q.parts              = 1;
    q.ordered            = !(C.identity && nc == 1);
    if (T.scalar) // A-B knob: the one-row-per-lane kernel on every class (the caller has dematched: nothing is fused then)
      miphy_ldpc_row_geometry(q);
    else if (q.c.kind == 0)
      miphy_ldpc_pkw_geometry(ctx, k.force == MIPHY_LDPC_FORCE_THROUGHPUT, q);
    else
      pk_class_geometry(ctx, k, fuse, q);
    q.gmsg_off = T.gmsg_bytes;
    T.gmsg_bytes += (q.gmsg_bytes + 255) & ~(size_t)255;
  }
  // Classes to streams. A class whose whole grid is a fraction of the chip (at most four wavefronts per CU: a few hundred small
  // codeblocks) is a latency chain -- one after another such classes each cost their full latency with the chip idle, next to a
  // large class they cost nothing: they go to the side streams, round robin. The large classes stay on the caller's stream one
  // after another: two chip-filling persistent grids side by side was measured slower and erratic (4.6 ms in sequence, 4.1 to 6.7
  // side by side on the mixed slot of bench.py), each holds the registers and LDS the other was tuned to have.
  if (nc > 1 && k.class_streams > 1) {
    int small = 0;
    for (miphy_ldpc_launch& q : T.l) {
      const uint64_t waves = q.c.kind == 0 ? q.c.bundle_count : (uint64_t)q.c.count * q.c.kind * q.parts;
      if (waves <= (uint64_t)ctx->num_cus * 4)
        q.stream = 1 + (small++ % (k.class_streams - 1));
    }
    if (small == (int)nc) // nothing large: the first small class takes the caller's stream
      T.l[0].stream = 0;
    T.side_streams = small > 0;
  }
}

// What a batch the host cannot sort is sized by: the largest lifting size (as threads: rounded up to wavefronts) and, per base graph,
// the largest number of variable nodes ceil((in_len + 2Z) / Z) a codeblock can reach (nof_layers <= nodes - bg_K,
// ldpc_decoder_impl.cpp:101-114); pk_ok = the packed kernel may be chosen (the bounds are the caller's, not a worst case).
struct batch_bounds {
  int  threads      = 64;
  int  max_nodes[2] = {0, 0};
  bool pk_ok        = false;
  void account(unsigned bg, unsigned Z, unsigned in_len)
  {
    threads           = std::max(threads, (int)((Z + 63) / 64) * 64);
    max_nodes[bg - 1] = std::max(max_nodes[bg - 1], miphy_ldpc_nodes(in_len, Z));
  }
};

// ONE launch for the whole batch (device-resident descriptors, which the host cannot sort, and the single-kernel modes of the A-B knob).
// The packed kernel (two check rows per lane, explicit messages in LDS) executes ~1.6x fewer instructions per row but needs more LDS
// per codeblock; at low code rates / mid lifting sizes that leaves one small workgroup per CU, and the one-row-per-lane kernel
// (compressed messages, twice the wavefronts) wins. Both are scored by the check rows a CU holds in flight (workgroups per CU limited
// by LDS, wavefront slots and registers), the packed one weighted by its instruction advantage; measured crossovers:
// tools/ldpc_rate_sweep.py. Any lifting size is legal in the packed kernel (an odd one folds its unpaired last row onto itself).
int rows_in_flight(size_t lds, int threads, int waves_per_simd_by_regs, int rows_per_lane)
{
  const int waves = threads / 64;
  int       wgs   = (int)((size_t)160 * 1024 / (lds ? lds : 1));
  wgs             = std::min(wgs, 32 / waves);                         // 8 wavefront slots per SIMD
  wgs             = std::min(wgs, 4 * waves_per_simd_by_regs / waves); // register file
  wgs             = std::max(wgs, 1);
  return wgs * threads * rows_per_lane;
}

void plan_one_launch(const miphy_ctx* ctx, const ldpc_knob_values& k, const batch_bounds& b, uint32_t n, miphy_ldpc_launches& T)
{
  const bool forced_row = k.force == MIPHY_LDPC_FORCE_ROW, forced_pk = k.force != MIPHY_LDPC_FORCE_AUTO && !forced_row;
  const int  nodes_all  = std::max(b.max_nodes[0], b.max_nodes[1]);
  const int  pk_threads = ((b.threads / 2 + 63) / 64) * 64, pk_waves = pk_threads / 64;
  size_t     row_lds = 0, pk_lds = 0, pk_lds_g = 0; // packed: with the messages in LDS / in global memory
  int        pk_pairs = 0;
  for (int bgi = 0; bgi < 2; ++bgi) { // the base graph of device descriptors is not visible here: the larger need of the two
    if (!b.max_nodes[bgi])
      continue;
    const int lay = miphy_ldpc_layers(bgi, nodes_all); // the kernels size their arrays from the batch-wide node bound
    row_lds       = std::max(row_lds, miphy_ldpc_row_lds_bytes(bgi, lay, (size_t)b.threads));
    if (b.pk_ok) {
      const int pairs = ctx->h_tables->pair_start[bgi][lay];
      pk_lds          = std::max(pk_lds, miphy_ldpc_pk_lds_bytes(bgi, lay, (size_t)b.threads, pairs));
      pk_lds_g        = std::max(pk_lds_g, miphy_ldpc_pk_lds_bytes(bgi, lay, (size_t)b.threads, 0));
      pk_pairs        = std::max(pk_pairs, pairs);
    }
  }
  // Messages in LDS while that keeps as many codeblocks resident per CU as the registers allow; otherwise (more than ~6 layers at
  // Z = 384) in global memory, where they cost an L2 round trip per layer visit but leave room for four codeblocks per CU: measured
  // 2.0x at rate 1/3, tools/ldpc_rate_sweep.py.
  auto       per_cu  = [&](size_t lds) { return miphy_ldpc_pk_per_cu(lds, pk_waves, false); };
  const bool pk_gmsg = b.pk_ok && per_cu(pk_lds_g) > per_cu(pk_lds) && (forced_pk || n > (uint32_t)(ctx->num_cus * per_cu(pk_lds)));
  if (pk_gmsg)
    pk_lds = pk_lds_g;
  bool use_pk = b.pk_ok && 1.6 * rows_in_flight(pk_lds, pk_threads, 4, 2) >= 1.0 * rows_in_flight(row_lds, b.threads, 8, 1);
  if (forced_row)
    use_pk = false;
  if (forced_pk)
    use_pk = b.pk_ok;
  T        = miphy_ldpc_launches{};
  T.scalar = forced_row;
  T.l.resize(1);
  miphy_ldpc_launch& L = T.l[0]; // (ordered = false: the codeblocks in array order)
  L.c.count            = n;
  L.nodes = nodes_all, L.parts = 1;
  if (use_pk) {
    L.used    = MIPHY_LDPC_KERNEL_PACKED | (pk_gmsg ? MIPHY_LDPC_KERNEL_GMSG : 0u); // (row_skip stays false: whether these codeblocks stop early is not visible here)
    L.threads = pk_threads, L.lds = pk_lds, L.gmsg_pairs = pk_gmsg ? pk_pairs : 0;
    L.grid       = miphy_ldpc_pk_grid(ctx, n, pk_threads, pk_lds, false);
    L.gmsg_bytes = pk_gmsg ? (size_t)L.grid * pk_waves * (size_t)pk_pairs * 256 : 0;
  } else {
    L.used    = MIPHY_LDPC_KERNEL_SCALAR;
    L.threads = b.threads, L.lds = row_lds, L.grid = n;
  }
  T.gmsg_bytes = L.gmsg_bytes;
}
} // namespace

int miphy_ldpc_plan_launches(miphy_ctx* ctx, const miphy_ldpc_classes& C, bool fuse, miphy_ldpc_launches& T)
{
  plan_classes(ctx, C, fuse, g_knobs.snapshot(), T);
  for (miphy_ldpc_launch& q : T.l) {
    int rc;
    if (q.atab && (rc = miphy_ldpc_address_tables(ctx, q.c.bgi, q.c.lay, q.c.min_Z, q.c.max_Z, &q.adr_by_z)))
      return rc;
  }
  return MIPHY_OK;
}

namespace {
// The launches of a table, the side-stream classes first: they start while the large ones are being enqueued.
int enqueue_launches(miphy_ctx* ctx, const miphy_ldpc_launches& T, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order,
                     const uint32_t* d_bundles, const int8_t* llr, uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot,
                     uint8_t* harq_crc_ok, const miphy_ldpc_rdm_desc* d_rdm, const int8_t* rm_in, void* gmsg, hipStream_t s)
{
  const size_t nc = T.l.size();
  for (size_t k2 = 0; k2 < 2 * nc; ++k2) {
    const miphy_ldpc_launch& L = T.l[k2 % nc];
    if ((L.stream != 0) != (k2 < nc))
      continue;
    hipStream_t     st  = L.stream == 0 ? s : (hipStream_t)ctx->side_stream[L.stream - 1];
    void*           gb  = L.gmsg_bytes ? (uint8_t*)gmsg + L.gmsg_off : nullptr;
    const uint32_t* ord = L.ordered ? d_order + L.c.first : nullptr;
    int             rc;
    if (L.used & MIPHY_LDPC_KERNEL_SCALAR) {
      rc = miphy_ldpc_row_launch(ctx, L, d_descs, ord, llr, out_bits, iters, harq_slot, harq_crc_ok, st);
    } else if (L.used & MIPHY_LDPC_KERNEL_WAVE) {
      rc = miphy_ldpc_pkw_launch(ctx, L, d_descs, d_order, d_bundles + 2 * (size_t)L.c.bundle_first, llr, out_bits, iters, harq_slot, harq_crc_ok, gb, st);
    } else {
      const bool fused = (L.used & MIPHY_LDPC_KERNEL_FUSED) != 0;
      rc = miphy_ldpc_pk_launch(ctx, L, d_descs, ord, llr, out_bits, iters, harq_slot, harq_crc_ok, fused ? d_rdm : nullptr, fused ? rm_in : nullptr, gb, st);
    }
    if (rc)
      return rc;
    g_kernels_used.fetch_or(L.used);
    g_adr_table_launches.fetch_add(L.adr_by_z ? 1u : 0u);
    g_row_skip_launches.fetch_add((L.row_skip && (L.used & MIPHY_LDPC_KERNEL_PACKED)) ? 1u : 0u);
  }
  return MIPHY_OK;
}

int hip_status(hipError_t e, const char* what)
{
  if (e == hipSuccess)
    return MIPHY_OK;
  miphy_set_error("ldpc_decode: %s -> %s", what, hipGetErrorString(e));
  return MIPHY_EHIP;
}
} // namespace

int miphy_ldpc_run_launches(miphy_ctx* ctx, const miphy_ldpc_launches& T, const miphy_ldpc_dec_desc* d_descs, const uint32_t* d_order,
                            const uint32_t* d_bundles, const int8_t* llr, uint8_t* out_bits, int32_t* iters, const uint32_t* harq_slot,
                            uint8_t* harq_crc_ok, const miphy_ldpc_rdm_desc* d_rdm, const int8_t* rm_in, void* gmsg, hipStream_t s)
{
  if (!T.side_streams)
    return enqueue_launches(ctx, T, d_descs, d_order, d_bundles, llr, out_bits, iters, harq_slot, harq_crc_ok, d_rdm, rm_in, gmsg, s);
  MIPHY_REQUIRE(ctx->ev_fork, "ldpc_decode: the side streams of the context have not been created");
  int rc = hip_status(hipEventRecord((hipEvent_t)ctx->ev_fork, s), "fork");
  for (int k = 0; k < MIPHY_NOF_SIDE_STREAMS && !rc; ++k)
    rc = hip_status(hipStreamWaitEvent((hipStream_t)ctx->side_stream[k], (hipEvent_t)ctx->ev_fork, 0), "fork");
  if (!rc)
    rc = enqueue_launches(ctx, T, d_descs, d_order, d_bundles, llr, out_bits, iters, harq_slot, harq_crc_ok, d_rdm, rm_in, gmsg, s);
  // the join on every path after the fork: the caller's stream (and a capture on it) takes back whatever reached the side streams
  for (int k = 0; k < MIPHY_NOF_SIDE_STREAMS; ++k) {
    int jc = hip_status(hipEventRecord((hipEvent_t)ctx->ev_join[k], (hipStream_t)ctx->side_stream[k]), "join");
    if (!jc)
      jc = hip_status(hipStreamWaitEvent(s, (hipEvent_t)ctx->ev_join[k], 0), "join");
    rc = rc ? rc : jc;
  }
  return rc;
}

namespace {
// The reference asserts the same conditions (ldpc_decoder_impl.cpp:66-84).
int validate_descs(const miphy_ctx* ctx, const miphy_ldpc_dec_desc* descs, uint32_t n)
{
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_ldpc_dec_desc& d = descs[i];
    MIPHY_REQUIRE(d.bg == 1 || d.bg == 2, "ldpc_decode: desc %u: invalid base graph %u", i, d.bg);
    MIPHY_REQUIRE(d.Z <= MIPHY_MAX_Z && ctx->h_tables->z_pos[d.Z] != 0xffff, "ldpc_decode: desc %u: invalid lifting size %u", i, d.Z);
    const unsigned bgK = miphy_bg_K(d.bg != 1), nshort = miphy_bg_N_short(d.bg != 1);
    MIPHY_REQUIRE(d.in_len >= (bgK + 2) * d.Z && d.in_len <= nshort * d.Z, "ldpc_decode: desc %u: input length %u out of range", i, d.in_len);
    MIPHY_REQUIRE(d.max_iter > 0, "ldpc_decode: desc %u: max_iter must be > 0", i);
    MIPHY_REQUIRE(d.crc_poly == MIPHY_CRC_NONE || d.crc_poly <= MIPHY_CRC11, "ldpc_decode: desc %u: invalid CRC", i);
    MIPHY_REQUIRE(d.nof_filler_bits < bgK * d.Z, "ldpc_decode: desc %u: invalid number of filler bits", i);
  }
  return MIPHY_OK;
}

// A class-sorted batch on the device: [descriptors | order | bundles], the staged part of one image.
struct class_arrays {
  image_slot<miphy_ldpc_dec_desc> descs;
  image_slot<uint32_t>            order, bundles;
};
class_arrays class_image(const miphy_ldpc_dec_desc* descs, uint32_t n, const miphy_ldpc_classes& C, device_image& img)
{
  return {img.put(descs, n), img.put(C.order), img.put(C.bundles)};
}
} // namespace

// ---- per call: host descriptors are sorted into launch classes; device-resident descriptors, which the host cannot sort, and the
// single-kernel modes of the A-B knob are ONE launch for the whole batch. Either way a launch table, scratch from the context ------
extern "C" int miphy_ldpc_decode_batch(miphy_ctx*                   ctx,
                                       const miphy_ldpc_dec_desc*   descs,
                                       int                          descs_on_device,
                                       uint32_t                     n,
                                       const int8_t*                llr,
                                       uint8_t*                     out_bits,
                                       int32_t*                     iters,
                                       const miphy_ldpc_dec_limits* limits,
                                       void*                        stream)
{
  MIPHY_REQUIRE(ctx && descs && llr && out_bits && iters, "ldpc_decode: null argument");
  if (n == 0)
    return MIPHY_OK;
  hipStream_t            s = (hipStream_t)stream;
  int                    rc;
  const ldpc_knob_values k = g_knobs.snapshot();
  // Host descriptors are validated here; for device descriptors the caller vouches for validity and may pass `limits`.
  if (!descs_on_device && (rc = validate_descs(ctx, descs, n)))
    return rc;
  miphy_ldpc_launches T;
  miphy_ldpc_classes  C;
  device_image        img; // class-sorted: [descriptors | order | bundles], staged as one region
  class_arrays        a;   // (one launch: the descriptors alone, in array order)
  const bool          one_launch = descs_on_device || k.force == MIPHY_LDPC_FORCE_ROW || k.force == MIPHY_LDPC_FORCE_PACKED_ONE;
  if (one_launch) {
    batch_bounds b;
    b.pk_ok = !descs_on_device || limits;
    if (!descs_on_device) {
      for (uint32_t i = 0; i < n; ++i)
        b.account(descs[i].bg, descs[i].Z, descs[i].in_len);
    } else if (limits) {
      MIPHY_REQUIRE(limits->max_Z >= 2 && limits->max_Z <= MIPHY_MAX_Z, "ldpc_decode: limits: invalid max_Z");
      b.account(1, limits->max_Z, limits->max_in_len);
      b.account(2, limits->max_Z, limits->max_in_len);
    } else { // worst case
      b.account(1, MIPHY_MAX_Z, 66 * MIPHY_MAX_Z);
      b.account(2, MIPHY_MAX_Z, 50 * MIPHY_MAX_Z);
    }
    plan_one_launch(ctx, k, b, n, T);
  } else {
    miphy_ldpc_build_classes(descs, n, nullptr, C);
    plan_classes(ctx, C, false, k, T);
    a = class_image(descs, n, C, img);
  }
  const void* d = nullptr;
  if ((rc = one_launch ? miphy_stage_descs(ctx, descs, descs_on_device, sizeof(miphy_ldpc_dec_desc) * (size_t)n, s, &d) : miphy_image_to_ring(ctx, img, s, &d)))
    return rc;
  void* gmsg = nullptr;
  if (T.gmsg_bytes && (rc = miphy_get_workspace(ctx, MIPHY_WS_LDPC_MSGS, T.gmsg_bytes, &gmsg)))
    return rc;
  if (T.side_streams && (rc = miphy_side_streams(ctx)))
    return rc;
  return miphy_ldpc_run_launches(ctx, T, a.descs.at(d), one_launch ? nullptr : a.order.at(d), one_launch ? nullptr : a.bundles.at(d), llr, out_bits, iters, nullptr,
                                 nullptr, nullptr, nullptr, gmsg, s);
}

// ---- prepared form: descriptors validated, sorted into launch classes and uploaded once, the launch table and its message scratch
// made once; every run is launches only -------------------------------------------------------------------------------------------
struct miphy_ldpc_decode_plan {
  miphy_ctx*          ctx = nullptr;
  miphy_ldpc_launches T;
  miphy_device_block  buf; // [descriptors | order | bundles | message scratch]
  class_arrays        a;
  void*               d_gmsg = nullptr;
};

extern "C" int miphy_ldpc_decode_plan_create(miphy_ctx* ctx, const miphy_ldpc_dec_desc* descs, uint32_t n, miphy_ldpc_decode_plan** out)
{
  MIPHY_REQUIRE(ctx && descs && out && n > 0, "miphy_ldpc_decode_plan_create: null argument or empty batch");
  int rc = validate_descs(ctx, descs, n);
  if (rc)
    return rc;
  miphy_ldpc_classes C;
  miphy_ldpc_build_classes(descs, n, nullptr, C);
  std::unique_ptr<miphy_ldpc_decode_plan> p(new miphy_ldpc_decode_plan());
  p->ctx = ctx;
  if ((rc = miphy_ldpc_plan_launches(ctx, C, false, p->T)) || (p->T.side_streams && (rc = miphy_side_streams(ctx))))
    return rc;
  device_image img;
  p->a                           = class_image(descs, n, C, img);
  const image_slot<uint8_t> gmsg = img.reserve<uint8_t>(p->T.gmsg_bytes, 256);
  if ((rc = miphy_image_to_block("miphy_ldpc_decode_plan_create", img, p->buf)))
    return rc;
  p->d_gmsg = p->T.gmsg_bytes ? gmsg.at(p->buf.get()) : nullptr;
  *out      = p.release();
  return MIPHY_OK;
}

extern "C" int miphy_ldpc_decode_plan_run(miphy_ldpc_decode_plan* p, const int8_t* llr, uint8_t* out_bits, int32_t* iters, void* stream)
{
  MIPHY_REQUIRE(p && llr && out_bits && iters, "miphy_ldpc_decode_plan_run: null argument");
  void* d = p->buf.get();
  return miphy_ldpc_run_launches(p->ctx, p->T, p->a.descs.at(d), p->a.order.at(d), p->a.bundles.at(d), llr, out_bits, iters, nullptr, nullptr, nullptr, nullptr, p->d_gmsg,
                                 (hipStream_t)stream);
}

extern "C" uint32_t miphy_ldpc_decode_plan_nof_launches(const miphy_ldpc_decode_plan* p)
{
  return p ? (uint32_t)p->T.l.size() : 0u;
}

extern "C" void miphy_ldpc_decode_plan_destroy(miphy_ldpc_decode_plan* p)
{
  delete p;
}
