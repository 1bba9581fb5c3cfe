// DM-RS based PUSCH channel estimator.
//
// Behaviour contract: lib/phy/upper/signal_processors/dmrs_pusch_estimator_impl.cpp:71-212 and
// port_channel_estimator_average_impl.cpp:97-347 (LS at the pilots, average over DM-RS symbols, RSRP / EPRE / noise /
// SNR, time alignment from the peak of a zero-padded 4096-point IDFT, linear interpolation, copy to all symbols).
// Everything stays on chip: Gold-sequence pilots are generated into LDS, the LS estimates and the IDFT buffer live in LDS, HBM sees the DM-RS
// resource elements once and the estimate once.
//
// Two kernels serve the four entry points:
//   chest_kernel<false>  workgroup per (job, rx port, layer): miphy_dmrs_pusch_estimate_batch, one-layer jobs of miphy_dmrs_pusch_estimate_layers_batch;
//   chest_kernel<true>   the same with the caller's pilots and hopping: miphy_port_channel_estimate_batch, miphy_dmrs_pusch_estimate_tp_batch;
//   chest_layers_kernel  workgroup per (job, rx port, CDM group), the group's layers separated: jobs on two to four layers of the layered entry.
// A third kernel, ncov_kernel (wavefront per (job, PRG)), forms the same DM-RS residuals again and turns them into the noise-plus-interference
// covariance across the ports: miphy_pusch_noise_covariance_batch. It takes the helpers and the job rules from here and writes no estimate.
// Behind them, cfo_corr_kernel and chest_cfo_kernel (workgroup per (job, rx port, CDM group), two launches): chest_layers_kernel for 1..4 layers with a
// carrier frequency offset estimated from consecutive DM-RS symbols, taken out of the DM-RS elements and put back per OFDM symbol:
// miphy_dmrs_pusch_estimate_cfo_batch. chest_tv_kernel takes chest_cfo_kernel's place where the channel changes within the slot: the fits of the DM-RS
// symbols are kept apart and interpolated in time: miphy_dmrs_pusch_estimate_tv_batch.
// What they share stands once, in front of them: the thread count, the LDS layout (chest_lds, which also sizes the launches), the job rules
// (chest_job_rule: chest_validate on the host, device-resident jobs of the layered entry on the device) and the chest_* helpers. What differs
// stays in the kernels: pilot ownership, despreading, the two-parameter noise fit, external pilots, hopping. Behind the kernels: chest_prologue
// (arguments, hints, rules), chest_resources (twiddles, Gold tables), one launch function per kernel.
#include "fft_device.h"
#include "gold_device.h"
#include "miphy_ext.h"
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

constexpr int CE_DFT = 4096;                       // port_channel_estimator_average_impl::DFT_SIZE
constexpr int HALF_CP = ((144 / 2) * CE_DFT) / 2048; // 144
constexpr int MAX_PILOTS = 275 * 6;
// Both kernels, both launches: the 4096-point IDFT has compile-time strides on 512 threads (256 threads were measured slower).
constexpr int CHEST_THREADS = 512;

// The dynamic LDS of both kernels: where each array starts, in bytes, and the pointers a workgroup takes from that.
struct chest_lds {
  static constexpr size_t LSE = fft_lds_bytes(CE_DFT), CBITS = LSE + MAX_PILOTS * sizeof(cplx), RBM = CBITS + 4 * 104 * sizeof(uint32_t),
                          PRB_OF = RBM + 5 * sizeof(uint64_t), RED = PRB_OF + 276 * sizeof(uint16_t), BYTES = RED + 64;
  static_assert(RBM % 8 == 0 && RED % 8 == 0, "64-bit words");
  cplx*     fbuf;   // 4096 (padded): IDFT buffer
  cplx*     lse;    // MAX_PILOTS: LS estimates, the anchors of the interpolation
  uint32_t* cbits;  // 4 symbols x 104 words: Gold sequences
  uint64_t* rbm;    // 5: the hop's PRB mask without the bits behind the grid
  uint16_t* prb_of; // 276: allocated PRB list
  float*    red;    // 8 partial sums of block_sum; the two 64-bit keys of chest_ta_peak
  __device__ __forceinline__ explicit chest_lds(unsigned char* s)
    : fbuf(reinterpret_cast<cplx*>(s)), lse(reinterpret_cast<cplx*>(s + LSE)), cbits(reinterpret_cast<uint32_t*>(s + CBITS)),
      rbm(reinterpret_cast<uint64_t*>(s + RBM)), prb_of(reinterpret_cast<uint16_t*>(s + PRB_OF)), red(reinterpret_cast<float*>(s + RED))
  {
  }
};

// ---- the job rules, for host and device alike
enum chest_rule {
  CHEST_RULE_NONE = 0,
  CHEST_RULE_NUMEROLOGY,
  CHEST_RULE_LAYERS,
  CHEST_RULE_PORTS,
  CHEST_RULE_GRID,
  CHEST_RULE_SYMBOLS,
  CHEST_RULE_SCALING,
  CHEST_RULE_DMRS,
  CHEST_RULE_NO_HOPPING,
  CHEST_RULE_HOP_SYMBOL,
  CHEST_RULE_HOP_COMPACT,
  CHEST_RULE_HOP_DMRS,
  CHEST_RULE_HOP_PRBS,
  CHEST_RULE_EMPTY
};

__host__ __device__ inline unsigned chest_nof_dmrs(unsigned symbols_mask, unsigned lo, unsigned hi) // DM-RS symbols in [lo, hi), hi <= 14
{
  return (unsigned)__builtin_popcount(symbols_mask & ((1u << hi) - 1u) & ~((1u << lo) - 1u));
}

// The first rule the job breaks, in the order chest_validate reports them. The bounds of every LDS array and loop of the kernels hang on these rules.
// pilots: the caller brings them (the port estimator, the only entry point that hops).
__host__ __device__ inline chest_rule chest_job_rule(const miphy_pusch_chest_job& j, bool pilots)
{
  if (j.numerology > 4)
    return CHEST_RULE_NUMEROLOGY;
  if (j.nof_tx_layers < 1 || j.nof_tx_layers > 4)
    return CHEST_RULE_LAYERS;
  if (j.nof_rx_ports < 1 || j.nof_rx_ports > 4)
    return CHEST_RULE_PORTS;
  if (j.grid_nof_prb < 1 || j.grid_nof_prb > 275)
    return CHEST_RULE_GRID;
  const unsigned first = j.first_symbol, last = first + j.nof_symbols;
  if (last > 14 || j.nof_symbols == 0)
    return CHEST_RULE_SYMBOLS;
  if (!(j.scaling > 0.f))
    return CHEST_RULE_SCALING;
  const unsigned nds = chest_nof_dmrs(j.symbols_mask, first, last);
  if (nds < 1 || nds > 4)
    return CHEST_RULE_DMRS;
  if (!pilots && j.hop_symbol != 0)
    return CHEST_RULE_NO_HOPPING;
  const unsigned nprb = miphy_count_prb(j.rb_mask, j.grid_nof_prb);
  if (j.hop_symbol != 0) { // intra-slot frequency hopping (port_channel_estimator_average_impl.cpp:118-124,153-163)
    if (!(j.hop_symbol > first && j.hop_symbol < last))
      return CHEST_RULE_HOP_SYMBOL;
    if (j.ce_compact)
      return CHEST_RULE_HOP_COMPACT;
    if (chest_nof_dmrs(j.symbols_mask, first, j.hop_symbol) < 1 || chest_nof_dmrs(j.symbols_mask, j.hop_symbol, last) < 1)
      return CHEST_RULE_HOP_DMRS;
    if (miphy_count_prb(j.rb_mask2, j.grid_nof_prb) != nprb)
      return CHEST_RULE_HOP_PRBS;
  }
  return nprb >= 1 ? CHEST_RULE_NONE : CHEST_RULE_EMPTY;
}

// ---- device helpers of both kernels

// Gold sequences c(0..nbits-1) of `nseq` <= 4 initial values (one per DM-RS symbol), bit-packed LSB-first, 104 words apart in `out`:
// every word on a lane of its own from the tables (x1 is a constant sequence, x2 is linear in c_init: gold_device.h) -- 31 independent
// loads per lane instead of the serial 31-word LFSR head and three recurrence steps.
__device__ __forceinline__ void gold_bits_block(const gold_tables& gt, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int nseq, int nbits, uint32_t* out, int tid)
{
  const int nwords = (nbits + 31) >> 5; // <= GOLD_BASIS_WORDS (3 300 bits)
  for (int k = tid; k < nseq * nwords; k += CHEST_THREADS) {
    const int      q  = k / nwords, i = k - q * nwords;
    const uint32_t ci = q == 0 ? c0 : (q == 1 ? c1 : (q == 2 ? c2 : c3));
    out[q * 104 + i]  = gt.x1_seq[i] ^ gold_x2_word(gt, ci, i);
  }
  __syncthreads();
}

__device__ __forceinline__ float block_sum(float v, float* red, int tid)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    v += __shfl_xor(v, off);
  __syncthreads();
  if ((tid & 63) == 0)
    red[tid >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma nounroll // (unrolled, the eight loads at once cost chest_layers_kernel spills at its 128 registers)
  for (int w = 1; w < CHEST_THREADS / 64; ++w)
    r += red[w];
  return r;
}

// DM-RS symbols of [lo, hi): the first four into dsym, the count returned.
__device__ __forceinline__ int chest_dmrs_symbols(unsigned symbols_mask, int lo, int hi, int (&dsym)[4])
{
  int nds = 0;
  for (int l = lo; l < hi; ++l)
    if ((symbols_mask >> l) & 1) {
      if (nds < 4)
        dsym[nds] = l;
      ++nds;
    }
  return nds;
}

__device__ __forceinline__ uint64_t rb_word_in_grid(uint64_t w, int wd, int nprb_grid) // a word of rb_mask without the bits behind the grid
{
  const int left = nprb_grid - wd * 64;
  return left <= 0 ? 0ull : (left >= 64 ? w : (w & ((1ull << left) - 1ull)));
}

// Allocated PRB list (compact) of the five mask words of a job in memory: PRB r goes to slot popcount(mask bits below r). Returns their number
// (every thread: the same popcounts). Ends in a barrier: prb_of[] may be read.
__device__ __forceinline__ int chest_prb_list(const uint64_t* __restrict__ mask_words, int nprb_grid, uint64_t* rbm, uint16_t* prb_of, int tid)
{
  if (tid < 5)
    rbm[tid] = rb_word_in_grid(mask_words[tid], tid, nprb_grid);
  __syncthreads();
  for (int r = tid; r < nprb_grid; r += CHEST_THREADS) {
    const int wd = r >> 6, bt = r & 63;
    if ((rbm[wd] >> bt) & 1ull) {
      int idx = __popcll(rbm[wd] & ((1ull << bt) - 1ull));
      for (int w = 0; w < wd; ++w)
        idx += __popcll(rbm[w]);
      prb_of[idx] = (uint16_t)r;
    }
  }
  int nprb = 0;
  for (int w = 0; w < 5; ++w)
    nprb += __popcll(rbm[w]);
  __syncthreads();
  return nprb;
}

// Initial values of the Gold sequences of the job's first four DM-RS symbols (dmrs_pusch_estimator_impl.cpp:158-162).
__device__ __forceinline__ void chest_c_init(const miphy_pusch_chest_job& job, const int (&dsym)[4], int nds, uint32_t (&c_init)[4])
{
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c_init[q] = 0;
    if (q >= nds)
      continue;
    const uint64_t t = ((uint64_t)(14u * job.slot_in_frame + (uint32_t)dsym[q] + 1u) * (2ull * job.scrambling_id + 1ull)) % (1ull << 31);
    c_init[q]        = (uint32_t)((t * (1ull << 17) + (2ull * job.scrambling_id + (job.n_scid ? 1u : 0u))) % (1ull << 31));
  }
}

// Layer 0's pilot (no frequency weight: the caller's) of DM-RS symbol d at pilot gp counted from PRB 0 (dmrs_helper.h:45-96).
__device__ __forceinline__ cplx chest_qpsk_pilot(const uint32_t* cbits, int d, int gp)
{
  const float     amp = 0.70710678118654752440f;
  const uint32_t* cb  = cbits + d * 104;
  const int       b0  = 2 * gp;
  return cplx{amp * (1.f - 2.f * (float)((cb[b0 >> 5] >> (b0 & 31)) & 1u)), amp * (1.f - 2.f * (float)((cb[(b0 + 1) >> 5] >> ((b0 + 1) & 31)) & 1u))};
}

// The grid of the job's receive port `port`. (A chain of selects: an array of the register copy of the job indexed at run time would live in
// scratch memory.)
__device__ __forceinline__ const float2* chest_port_grid(const float2* grid, const miphy_pusch_chest_job& job, int port)
{
  const unsigned grid_port = port == 0 ? job.rx_ports[0] : (port == 1 ? job.rx_ports[1] : (port == 2 ? job.rx_ports[2] : job.rx_ports[3]));
  return grid + job.grid_offset + (size_t)grid_port * 14 * ((size_t)job.grid_nof_prb * 12);
}

// Least squares at one pilot: rx * conj(pilot(d)) summed over the DM-RS symbols; the received energy goes to epre_acc.
template <class Pilot>
__device__ __forceinline__ cplx chest_ls(const float2 (&x)[4], int nds, float& epre_acc, const Pilot& pilot)
{
  cplx acc = {0.f, 0.f};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (d >= nds)
      continue;
    const cplx p = pilot(d);
    acc.x += x[d].x * p.x + x[d].y * p.y;
    acc.y += x[d].y * p.x - x[d].x * p.y;
    epre_acc += x[d].x * x[d].x + x[d].y * x[d].y;
  }
  return acc;
}

// The residual at one pilot of one DM-RS symbol: rx + h * pilot, h = -(the predicted channel).
__device__ __forceinline__ cplx chest_residual_at(float2 x, cplx h, cplx pilot)
{
  const cplx pred = cmul(h, pilot);
  return cplx{pred.x + x.x, pred.y + x.y};
}

// Residual energy at one pilot: |rx + h * pilot(d)|^2 over the DM-RS symbols, added to noise_acc term by term.
template <class Pilot>
__device__ __forceinline__ void chest_residual(const float2 (&x)[4], int nds, cplx h, float& noise_acc, const Pilot& pilot)
{
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (d >= nds)
      continue;
    const cplx e = chest_residual_at(x[d], h, pilot(d));
    noise_acc += e.x * e.x + e.y * e.y;
  }
}

__device__ __forceinline__ void chest_clear_idft(cplx* fbuf, int tid)
{
  for (int i = tid; i < (int)(fft_lds_bytes(CE_DFT) / 8); i += CHEST_THREADS)
    fbuf[i] = {0.f, 0.f};
}

// Peak of the first / last HALF_CP taps of the IDFT in fbuf, in taps (negative: advance); the first occurrence wins, like std::max_element. One
// LDS atomic per window on a 64-bit key = (value bits << 32) | (0xffffffff - tap): the largest value, then the smallest tap. Ends in a barrier,
// which the next clearing of fbuf relies on.
__device__ __forceinline__ float chest_ta_peak(const cplx* fbuf, float* red, int tid)
{
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(red);
  __syncthreads();
  if (tid < 2)
    keys[tid] = 0ull;
  __syncthreads();
  if (tid < 2 * HALF_CP) { // 288 taps on 512 threads: delay window 0 .. 143, then the advance window
    const cplx  v = fbuf[fpad(tid < HALF_CP ? tid : CE_DFT - 2 * HALF_CP + tid)];
    const float a = v.x * v.x + v.y * v.y;
    atomicMax(&keys[tid >= HALF_CP ? 1 : 0], ((unsigned long long)__float_as_uint(a) << 32) | (0xffffffffu - (unsigned)tid));
  }
  __syncthreads();
  const float md = __uint_as_float((unsigned)(keys[0] >> 32)), ma = __uint_as_float((unsigned)(keys[1] >> 32));
  const int   id = (int)(0xffffffffu - (unsigned)(keys[0] & 0xffffffffu));
  const int   ia = (int)(0xffffffffu - (unsigned)(keys[1] & 0xffffffffu)) - HALF_CP;
  __syncthreads();
  return (md >= ma) ? (float)id : -(float)(HALF_CP - ia);
}

// Linear interpolation over the concatenated allocated PRBs (interpolator_linear_impl.cpp:58-78, edges held): subcarrier k of the allocation from
// `ninp` anchors at off + i << sh (sh = 1: every second subcarrier, 2: every fourth). COPY_AT_ANCHOR: on an anchor's own subcarrier chest_kernel
// copies it, chest_layers_kernel evaluates a0 + (a1 - a0) * 0, which turns -0.0 into +0.0 and a non-finite neighbour into NaN: each keeps its bytes.
template <bool COPY_AT_ANCHOR, class Anchor>
__device__ __forceinline__ cplx chest_interpolate(const Anchor& anchor, int k, int sh, int off, int ninp)
{
  const int kk = k - off;
  if (kk <= 0)
    return anchor(0);
  const int i = kk >> sh, j = kk & ((1 << sh) - 1);
  if (i >= ninp - 1)
    return anchor(ninp - 1);
  if (COPY_AT_ANCHOR && j == 0)
    return anchor(i);
  const cplx  a0 = anchor(i), a1 = anchor(i + 1);
  const float f  = (float)j / (float)(1 << sh);
  return {a0.x + (a1.x - a0.x) * f, a0.y + (a1.y - a0.y) * f};
}

// First row of the estimate of (layer, port): one row in the compact form, rows 0 .. first_symbol + nof_symbols - 1 otherwise.
__device__ __forceinline__ float2* chest_ce_rows(float2* ce_out, const miphy_pusch_chest_job& job, int layer, int port)
{
  const int rows = job.ce_compact ? 1 : job.first_symbol + job.nof_symbols;
  return ce_out + job.ce_offset + ((size_t)(layer * job.nof_rx_ports + port) * rows) * ((size_t)job.grid_nof_prb * 12);
}

// Subcarrier k of the allocation to its column of the one compact row, or of every symbol of [lo, hi) (:216-224).
__device__ __forceinline__ void chest_store(float2* rows, const uint16_t* prb_of, int k, cplx v, bool compact, int lo, int hi, int nsc)
{
  const size_t col = (size_t)prb_of[k / 12] * 12 + (k % 12);
  if (compact) {
    rows[col] = make_float2(v.x, v.y);
  } else {
    for (int l = lo; l < hi; ++l)
      rows[(size_t)l * nsc + col] = make_float2(v.x, v.y);
  }
}

// The side-band scalars of (port, layer) (:118-144): RSRP, EPRE, noise variance, SNR (`main`); time alignment in seconds from taps (`ta`).
__device__ __forceinline__ void chest_scalars(float* scalars, const miphy_pusch_chest_job& job, int port, int layer, float rsrp, float epre, float noise_var,
                                              float ta_taps, bool main, bool ta)
{
  const float beta = job.scaling, datarp = rsrp / beta / beta;
  const float scs_khz = 15.f * (float)(1u << job.numerology);
  float*      sc      = scalars + job.scalars_offset + 5 * ((size_t)port * job.nof_tx_layers + layer);
  if (main) {
    sc[0] = rsrp;
    sc[1] = epre;
    sc[2] = noise_var;
    sc[3] = (noise_var != 0.f) ? datarp / noise_var : 1000.f;
  }
  if (ta)
    sc[4] = ta_taps / ((float)CE_DFT * scs_khz * 1000.0f);
}

// GENERAL = false: the PUSCH DM-RS estimator proper (pilots generated from the job, one hop: dmrs_pusch_estimator_impl.cpp never
// configures hopping); true: pilots from the caller and intra-slot frequency hopping (the port estimator on its own).
template <bool GENERAL>
__global__ void __launch_bounds__(CHEST_THREADS, GENERAL ? 2 : 4) chest_kernel(const miphy_pusch_chest_job* __restrict__ jobs,
                                                    const gold_jump* __restrict__ gj,
                                                    const cplx* __restrict__ tw,
                                                    const float2* __restrict__ grid,
                                                    float2* __restrict__ ce_out,
                                                    float* __restrict__ scalars,
                                                    const float2* __restrict__ ext_pilots_arg,
                                                    int ports_dim) // blockIdx.y = layer * ports_dim + port
{
  const float2* ext_pilots = GENERAL ? ext_pilots_arg : nullptr;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const chest_lds lds(smem);

  // static fields from a dword copy in scalar registers (load_words), the mask words from the record in memory: a private copy of the
  // descriptor indexed at run time would live in scratch memory.
  const miphy_pusch_chest_job& jmem = jobs[blockIdx.x];
  const miphy_pusch_chest_job  job  = load_words(jobs + blockIdx.x);
  constexpr int nt  = CHEST_THREADS;
  const int     tid = threadIdx.x;
  const int port = blockIdx.y % ports_dim, layer = blockIdx.y / ports_dim;
  // gridDim.z == 2 (launches that leave most of the chip idle -- a single slot): the time-alignment step -- the 4096-point IDFT and its peak
  // search, which only the side-band scalar sc[4] needs -- runs in a workgroup of its own (z = 1: LS estimates, IDFT, peak) next to the one
  // that estimates, interpolates and stores (z = 0): the demodulator behind this kernel waits for the shorter of the two chains + sc[2].
  const bool ta_only = gridDim.z == 2 && blockIdx.z == 1, do_ta = gridDim.z == 1 || ta_only, do_main = !ta_only;
  if (port >= job.nof_rx_ports || layer >= job.nof_tx_layers)
    return;
  const int nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  const int first = job.first_symbol, nsymb_out = first + job.nof_symbols;
  const int hop_symbol = (GENERAL && job.hop_symbol > first && job.hop_symbol < nsymb_out) ? job.hop_symbol : 0;
  const int nhops      = hop_symbol ? 2 : 1;
  // DM-RS symbols of the whole allocation (the pilots of the second hop follow those of the first in an external pilot list)
  int         dsym_all[4]; // (only their number is used)
  const int   nds_all = chest_dmrs_symbols(job.symbols_mask, first, nsymb_out, dsym_all);
  const int   delta = ext_pilots ? ((job.re_odd_mask >> layer) & 1) : ((layer >> 1) & 1); // RE pattern: even subcarriers for ports 0,1 ; odd for 2,3
  const float wf1 = (layer & 1) ? -1.f : 1.f;       // frequency weight on odd pilots (layers > 0)
  const float2* g = chest_port_grid(grid, job, port);
  const float   beta = job.scaling;
  const bool    compact = job.ce_compact != 0;
  float2*       dst0    = chest_ce_rows(ce_out, job, layer, port);
  // accumulated over the hops (port_channel_estimator_average_impl.cpp:110-124)
  float epre_tot = 0.f, rsrp_tot = 0.f, noise_tot = 0.f, ta_tot = 0.f;
  int   np_sym = 0; // pilots per DM-RS symbol (the same in both hops)
  for (int hop = 0; hop < nhops; ++hop) {
  const int h_first = (hop == 1) ? hop_symbol : first, h_last = (hop == 0 && hop_symbol) ? hop_symbol : nsymb_out;
  __syncthreads(); // the first hop's readers of rbm[], prb_of[] and lse[]
  int       dsym[4];
  const int nds        = chest_dmrs_symbols(job.symbols_mask, h_first, h_last, dsym);
  const int hop_offset = (hop == 1) ? nds_all - nds : 0; // compute_layer_hop: pilots.size().nof_symbols - nof_dmrs_symbols
  const int nprb       = chest_prb_list(hop == 1 ? jmem.rb_mask2 : jmem.rb_mask, nprb_grid, lds.rbm, lds.prb_of, tid);
  const int np = nprb * 6;
  np_sym       = np;
  if (do_ta) // the IDFT buffer of the time-alignment step, cleared here: nothing waits for it
    chest_clear_idft(lds.fbuf, tid);
  // The received DM-RS elements of this thread's pilots (at most four per thread and DM-RS symbol: 1 650 pilots on 512 threads) are
  // requested NOW, before the pilot sequences are put together: the two memory round trips overlap, and both the LS phase and the noise
  // phase then work from registers (they used to fetch the same elements one after the other).
  constexpr int XK = 4;
  float2        xq[XK][4];
#pragma unroll
  for (int kk = 0; kk < XK; ++kk) {
    const int i = tid + kk * nt;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      xq[kk][d] = make_float2(0.f, 0.f);
      if (i < np && d < nds) {
        const int r = lds.prb_of[i / 6], q = i % 6;
        xq[kk][d]   = g[(size_t)dsym[d] * nsc + r * 12 + 2 * q + delta];
      }
    }
  }
  if (!ext_pilots) {
    uint32_t c_init[4];
    chest_c_init(job, dsym, nds, c_init);
    gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], min(nds, 4), 12 * nprb_grid, lds.cbits, tid);
  } else {
    __syncthreads();
  }
  // pilot of DM-RS symbol d (of this hop), pilot i of the allocation: generated from the Gold sequence counted from PRB 0 with the layer's
  // frequency weight, or read from the caller's list
  const float2* xp = ext_pilots ? ext_pilots + job.pilots_offset + ((size_t)layer * nds_all + hop_offset) * np : nullptr;
  auto pilot = [&](int d, int i, int gp) -> cplx {
    if (xp) {
      const float2 v = xp[(size_t)d * np + i];
      return cplx{v.x, v.y};
    }
    const cplx  p = chest_qpsk_pilot(lds.cbits, d, gp);
    const float w = (layer != 0 && (i & 1)) ? wf1 : 1.f;
    return cplx{p.x * w, p.y * w};
  };

  // ---- LS estimate, EPRE (port_channel_estimator_average_impl.cpp:180-201)
  float epre_acc = 0.f, rsrp_acc = 0.f;
#pragma unroll
  for (int kk = 0; kk < XK; ++kk) {
    const int i = tid + kk * nt;
    if (i >= np)
      continue;
    const int r = lds.prb_of[i / 6], q = i % 6;
    const int gp = r * 6 + q;                      // pilot index counted from PRB 0
    const cplx acc = chest_ls(xq[kk], nds, epre_acc, [&](int d) { return pilot(d, i, gp); });
    rsrp_acc += acc.x * acc.x + acc.y * acc.y;
    const float ts = 1.0f / ((float)nds * beta);
    lds.lse[i]         = {acc.x * ts, acc.y * ts};
  }
  epre_tot += block_sum(epre_acc, lds.red, tid);
  rsrp_tot += block_sum(rsrp_acc, lds.red, tid) / (float)nds;
  __syncthreads();

  // ---- noise (:271-310): per-PRB mean of the estimates, predicted observation, residual power (symbol group 0 only)
  float noise_acc = 0.f;
#pragma unroll
  for (int kk = 0; kk < XK; ++kk) {
    const int i = tid + kk * nt;
    if (i >= (do_main ? np : 0))
      continue;
    const int b = (i / 6) * 6;
    cplx      avg = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 6; ++k)
      avg = cadd(avg, lds.lse[b + k]);
    avg = {avg.x / 6.f * -beta, avg.y / 6.f * -beta};
    const int r = lds.prb_of[i / 6], q = i % 6, gp = r * 6 + q;
    chest_residual(xq[kk], nds, avg, noise_acc, [&](int d) { return pilot(d, i, gp); });
  }
  noise_tot += block_sum(noise_acc, lds.red, tid) / (float)np * 6.f; // = sum over symbols of |residual|^2 / np * window (:300-309)

  // ---- time alignment (:312-347): zero-padded IDFT of the LS estimates at their RE positions
  if (do_ta) {
  // (fbuf was cleared at the head of the hop, under the memory requests; the barriers of the reductions above order it)
  for (int i = tid; i < np; i += nt)
    lds.fbuf[fpad(lds.prb_of[i / 6] * 12 + 2 * (i % 6) + delta)] = lds.lse[i];
  __syncthreads();
  fft4096_lds<true>(lds.fbuf, tw, tid);
  ta_tot += chest_ta_peak(lds.fbuf, lds.red, tid);
  } // do_ta

  // ---- interpolation (anchors lse[i] at subcarrier 2 i + delta), written straight to every OFDM symbol of the hop
  const int  nout   = do_main ? nprb * 12 : 0;
  const auto anchor = [&](int i) -> cplx { return lds.lse[i]; };
  for (int k = tid; k < nout; k += nt)
    chest_store(dst0, lds.prb_of, k, chest_interpolate<true>(anchor, k, 1, delta, np), compact, h_first, h_last, nsc);
  } // hops

  // ---- side-band scalars (:118-144)
  if (tid == 0) {
    const float ndp  = (float)(np_sym * nds_all);
    const float epre = epre_tot / ndp;
    // noise_var = sum over hops and symbols of the residual energy / (window * all DM-RS symbols - 1)
    float noise_var = noise_tot / (float)(6 * nds_all - 1);
    if (nds_all < 3 || nhops == 2)
      noise_var = 0.001f * epre; // convert_dB_to_power(-30) * epre
    chest_scalars(scalars, job, port, layer, rsrp_tot / ndp, epre, noise_var, nhops == 2 ? ta_tot / 2.0f : ta_tot, do_main, do_ta);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// PUSCH on two to four layers (DM-RS type 1, single-symbol DM-RS, layer ly = DM-RS port ly) -- beyond the 23.5 reference, whose estimator runs
// every layer through the one-layer fit above and never undoes the frequency-domain OCC: layers 2g and 2g+1 share CDM group g and its resource
// elements, so its estimates come out as h_2g +- h_2g+1. Here one workgroup serves (job, rx port, CDM group): the received elements, the Gold
// sequences and the PRB list are fetched once for both layers of the group. A thread owns PAIRS of neighbouring pilots (three per PRB, none
// across a PRB edge): z = least squares against layer 0's pilot, s_a = (z_even + z_odd) / 2, s_b = (z_even - z_odd) / 2 -- all in registers; the
// LS vector in LDS holds s_a / s_b interleaved where chest_kernel holds z, so the second layer costs no LDS. A layer alone in its group (layer 2
// of three) keeps z and follows chest_kernel's arithmetic. Arithmetic: include/miphy.h, DESIGN.md section 7 (f1d).
constexpr int CL_PK = 2; // pairs per thread: 825 pairs of 1 650 pilots on 512 threads
static_assert(CL_PK * CHEST_THREADS * 2 >= MAX_PILOTS, "every pilot pair has a thread");

// Device-resident jobs of a layered batch, for the one-layer launch of chest_kernel: a copy in which the jobs on more layers, and the jobs that
// break a rule (nobody has checked them), have no receive port -- their workgroups leave at once.
__global__ void chest_solo_jobs_kernel(const miphy_pusch_chest_job* __restrict__ jobs, miphy_pusch_chest_job* __restrict__ out, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  miphy_pusch_chest_job j = jobs[i];
  if (j.nof_tx_layers != 1 || chest_job_rule(j, false) != CHEST_RULE_NONE)
    j.nof_rx_ports = 0;
  out[i] = j;
}

__global__ void __launch_bounds__(CHEST_THREADS, 4) chest_layers_kernel(const miphy_pusch_chest_job* __restrict__ jobs,
                                                                        const gold_jump* __restrict__ gj,
                                                                        const cplx* __restrict__ tw,
                                                                        const float2* __restrict__ grid,
                                                                        float2* __restrict__ ce_out,
                                                                        float* __restrict__ scalars,
                                                                        int ports_dim) // blockIdx.y = CDM group * ports_dim + port
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const chest_lds lds(smem);
  constexpr int nt = CHEST_THREADS;
  const int     tid = threadIdx.x;
  const miphy_pusch_chest_job& jmem = jobs[blockIdx.x];
  const int port = blockIdx.y % ports_dim, grp = blockIdx.y / ports_dim;
  const int L    = jmem.nof_tx_layers;
  // (uniform) one-layer jobs belong to chest_kernel; a job without this port or group; a device-resident job that breaks a rule
  if (L < 2 || L > 4 || port >= jmem.nof_rx_ports || 2 * grp >= L || chest_job_rule(jmem, false) != CHEST_RULE_NONE)
    return;
  const miphy_pusch_chest_job job = load_words(jobs + blockIdx.x);
  const bool pair = 2 * grp + 1 < L; // both layers of the group are present
  const int  nlay = pair ? 2 : 1;
  const int  nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  const int  first = job.first_symbol, nsymb_out = first + job.nof_symbols;
  int        dsym[4];
  const int  nds  = chest_dmrs_symbols(job.symbols_mask, first, nsymb_out, dsym);
  const int  nprb = chest_prb_list(jmem.rb_mask, nprb_grid, lds.rbm, lds.prb_of, tid);
  const int  np = nprb * 6, npairs = nprb * 3;
  const float2* g = chest_port_grid(grid, job, port);
  const float   beta = job.scaling;
  // The received DM-RS elements of this thread's pairs, requested before the pilot sequences are put together (as chest_kernel does): the LS
  // and the noise phase work from these registers.
  float2 xq[CL_PK][2][4];
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * nt;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      xq[kk][0][d] = xq[kk][1][d] = make_float2(0.f, 0.f);
      if (m < npairs && d < nds) {
        const float2* src = g + (size_t)dsym[d] * nsc + lds.prb_of[m / 3] * 12 + 4 * (m % 3) + grp;
        xq[kk][0][d] = src[0];
        xq[kk][1][d] = src[2];
      }
    }
  }
  uint32_t c_init[4];
  chest_c_init(job, dsym, nds, c_init);
  gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], nds, 12 * nprb_grid, lds.cbits, tid);

  // ---- least squares against layer 0's pilot, despreading, EPRE, RSRP
  const float ts = 1.0f / ((float)nds * beta);
  float       epre_acc = 0.f, ra_acc = 0.f, rb_acc = 0.f;
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * nt;
    if (m >= npairs)
      continue;
    const int gp0 = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
    cplx      z[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const cplx acc = chest_ls(xq[kk][e], nds, epre_acc, [&](int d) { return chest_qpsk_pilot(lds.cbits, d, gp0 + e); });
      z[e]           = {acc.x * ts, acc.y * ts};
    }
    if (pair) {
      const cplx sa = {(z[0].x + z[1].x) * 0.5f, (z[0].y + z[1].y) * 0.5f}, sb = {(z[0].x - z[1].x) * 0.5f, (z[0].y - z[1].y) * 0.5f};
      lds.lse[2 * m] = sa, lds.lse[2 * m + 1] = sb;
      ra_acc += sa.x * sa.x + sa.y * sa.y;
      rb_acc += sb.x * sb.x + sb.y * sb.y;
    } else {
      lds.lse[2 * m] = z[0], lds.lse[2 * m + 1] = z[1];
      ra_acc += z[0].x * z[0].x + z[0].y * z[0].y + z[1].x * z[1].x + z[1].y * z[1].y;
    }
  }
  const float epre    = block_sum(epre_acc, lds.red, tid) / (float)(np * nds);
  const float rs_norm = beta * beta / (float)(pair ? npairs : np);
  float       rsrp[2];
  rsrp[0] = block_sum(ra_acc, lds.red, tid) * rs_norm;
  rsrp[1] = pair ? block_sum(rb_acc, lds.red, tid) * rs_norm : 0.f;
  __syncthreads(); // lse[]

  // ---- interpolation, straight to every OFDM symbol. Both layers present: anchors s_l[m] at subcarrier 4 m + 1 + group (stride 4); a layer
  // alone: z[i] at 2 i + group (stride 2), as chest_kernel.
  const bool compact = job.ce_compact != 0;
  const int  sh = pair ? 2 : 1, off = pair ? 1 + grp : grp, ninp = pair ? npairs : np;
  for (int l = 0; l < nlay; ++l) {
    float2*    dst0   = chest_ce_rows(ce_out, job, 2 * grp + l, port);
    const auto anchor = [&](int i) -> cplx { return pair ? lds.lse[2 * i + l] : lds.lse[i]; };
    for (int k = tid; k < nprb * 12; k += nt)
      chest_store(dst0, lds.prb_of, k, chest_interpolate<false>(anchor, k, sh, off, ninp), compact, first, nsymb_out, nsc);
  }

  // ---- noise: the per-PRB means of s_a and s_b predict the observations, a + (-1)^i b on pilot i; two parameters are fitted per window of six
  // pilots against chest_kernel's one (:271-310). Measured from three DM-RS symbols on only; below, the forced value does not need it.
  float noise_var = 0.001f * epre; // convert_dB_to_power(-30) * epre
  if (nds >= 3) {
    float noise_acc = 0.f;
#pragma unroll
    for (int kk = 0; kk < CL_PK; ++kk) {
      const int m = tid + kk * nt;
      if (m >= npairs)
        continue;
      const int  b  = (m / 3) * 6;
      const cplx ea = cadd(cadd(lds.lse[b], lds.lse[b + 2]), lds.lse[b + 4]), eo = cadd(cadd(lds.lse[b + 1], lds.lse[b + 3]), lds.lse[b + 5]);
      cplx       ma, mb; // a layer alone: the mean of its six z, no second parameter
      if (pair)
        ma = {ea.x / 3.f, ea.y / 3.f}, mb = {eo.x / 3.f, eo.y / 3.f};
      else
        ma = {(ea.x + eo.x) / 6.f, (ea.y + eo.y) / 6.f}, mb = {0.f, 0.f};
      const cplx h[2] = {{(ma.x + mb.x) * -beta, (ma.y + mb.y) * -beta}, {(ma.x - mb.x) * -beta, (ma.y - mb.y) * -beta}};
      const int  gp0  = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
#pragma unroll
      for (int e = 0; e < 2; ++e)
        chest_residual(xq[kk][e], nds, h[e], noise_acc, [&](int d) { return chest_qpsk_pilot(lds.cbits, d, gp0 + e); });
    }
    noise_var = block_sum(noise_acc, lds.red, tid) / (float)np * 6.f / (float)(6 * nds - nlay);
  }

  // ---- time alignment per layer (:312-347): zero-padded IDFT with s_l[m] on both pilot subcarriers of pair m
  float ta[2] = {0.f, 0.f};
  for (int l = 0; l < nlay; ++l) {
    chest_clear_idft(lds.fbuf, tid);
    __syncthreads();
    for (int i = tid; i < np; i += nt)
      lds.fbuf[fpad(lds.prb_of[i / 6] * 12 + 2 * (i % 6) + grp)] = pair ? lds.lse[(i & ~1) + l] : lds.lse[i];
    __syncthreads();
    fft4096_lds<true>(lds.fbuf, tw, tid);
    ta[l] = chest_ta_peak(lds.fbuf, lds.red, tid);
  }

  // ---- side-band scalars, per layer; the noise variance is the group's
  if (tid < nlay)
    chest_scalars(scalars, job, port, 2 * grp + tid, tid ? rsrp[1] : rsrp[0], epre, noise_var, tid ? ta[1] : ta[0], true, true);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Noise-plus-interference covariance across the receive ports, from the residuals whose energy chest_layers_kernel turns into noise_var
// (miphy_pusch_noise_covariance_batch; include/miphy.h has the formula). A workgroup serves (job, eight PRGs): the PRB list and the Gold
// sequences are put together once, as in the estimator, then every wavefront takes one PRG. Its lanes own pilot pairs, 63 per pass -- 21 whole
// PRBs, so the three pairs of a PRB sit on neighbouring lanes and the per-PRB means come from three lane reads, summed in the estimator's order.
// Per CDM group a lane holds the residuals of its two pilots on every port and DM-RS symbol and adds their P (P + 1) / 2 products to its own
// accumulators (groups, pilots of the pair, DM-RS symbols: ascending); the lanes are then summed in a fixed butterfly. No atomics: a PRG's matrix
// has the same bits whatever else is in the batch.
constexpr int NCOV_PAIRS = 63, NCOV_PRG_PER_BLOCK = CHEST_THREADS / 64;

__host__ __device__ inline bool ncov_job_ok(const miphy_pusch_ncov_job& j)
{
  return chest_job_rule(j.base, false) == CHEST_RULE_NONE && j.loading >= 0.f && j.loading <= 3.402823466e+38f; // (NaN fails both)
}

__host__ __device__ inline unsigned ncov_nof_prg(unsigned nprb, unsigned prg_size)
{
  return prg_size ? (nprb + prg_size - 1) / prg_size : 1u;
}

__global__ void __launch_bounds__(CHEST_THREADS) ncov_kernel(const miphy_pusch_ncov_job* __restrict__ jobs, const gold_jump* __restrict__ gj,
                                                             const float2* __restrict__ grid, float2* __restrict__ cov)
{
  __shared__ uint32_t cbits[4 * 104];
  __shared__ uint64_t rbm[5];
  __shared__ uint16_t prb_of[276];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const miphy_pusch_ncov_job& jm = jobs[blockIdx.x];
  if (!ncov_job_ok(jm)) // (uniform) a device-resident job that breaks a rule
    return;
  const miphy_pusch_chest_job job = load_words(&jm.base);
  const int L = job.nof_tx_layers, P = job.nof_rx_ports;
  const int nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  int       dsym[4];
  const int nds  = chest_dmrs_symbols(job.symbols_mask, job.first_symbol, job.first_symbol + job.nof_symbols, dsym);
  const int nprb = chest_prb_list(jm.base.rb_mask, nprb_grid, rbm, prb_of, tid);
  const int per  = jm.prg_size ? (int)jm.prg_size : nprb;
  const int nprg = (nprb + per - 1) / per;
  if ((int)blockIdx.y * NCOV_PRG_PER_BLOCK >= nprg) // (uniform) the launch is sized for the job with the most PRGs
    return;
  uint32_t c_init[4];
  chest_c_init(job, dsym, nds, c_init);
  gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], nds, 12 * nprb_grid, cbits, tid);
  const int prg = blockIdx.y * NCOV_PRG_PER_BLOCK + wave;
  if (prg >= nprg) // (per wavefront; no barrier follows)
    return;
  const int   prb0 = prg * per, n_j = min(per, nprb - prb0), npairs = 3 * n_j;
  const int   ngrp = (L + 1) / 2;
  const float beta = job.scaling, ts = 1.0f / ((float)nds * beta);
  float       cd[4] = {0.f, 0.f, 0.f, 0.f}; // C_pp
  cplx        co[6];                        // C_pq, p > q, at p (p - 1) / 2 + q
#pragma unroll
  for (int k = 0; k < 6; ++k)
    co[k] = {0.f, 0.f};
  const int b3 = lane - lane % 3; // the first lane of this lane's PRB
  for (int base = 0; base < npairs; base += NCOV_PAIRS) {
    const int  m    = base + lane;
    const bool live = lane < NCOV_PAIRS && m < npairs;
    const int  r    = prb_of[prb0 + (live ? m / 3 : 0)], t3 = m % 3;
    const int  gp0  = r * 6 + 2 * t3;
    cplx       pil[2][4];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int d = 0; d < 4; ++d)
        pil[e][d] = d < nds ? chest_qpsk_pilot(cbits, d, gp0 + e) : cplx{0.f, 0.f};
#pragma nounroll
    for (int grp = 0; grp < ngrp; ++grp) {
      const bool pair = 2 * grp + 1 < L; // both layers of the group are present
      cplx       res[4][2][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float2 x[2][4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          x[0][d] = x[1][d] = make_float2(0.f, 0.f);
          if (live && p < P && d < nds) {
            const float2* src = chest_port_grid(grid, job, p) + (size_t)dsym[d] * nsc + r * 12 + 4 * t3 + grp;
            x[0][d] = src[0];
            x[1][d] = src[2];
          }
        }
        cplx z[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          float      unused = 0.f;
          const cplx acc    = chest_ls(x[e], nds, unused, [&](int d) { return pil[e][d]; });
          z[e]              = {acc.x * ts, acc.y * ts};
        }
        if (pair) { // s_a, s_b of the pair
          const cplx sa = {(z[0].x + z[1].x) * 0.5f, (z[0].y + z[1].y) * 0.5f}, sb = {(z[0].x - z[1].x) * 0.5f, (z[0].y - z[1].y) * 0.5f};
          z[0] = sa, z[1] = sb;
        }
        cplx s[2]; // the PRB's sums of the even and of the odd entries, lanes in order
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const cplx v0 = {__shfl(z[e].x, b3), __shfl(z[e].y, b3)}, v1 = {__shfl(z[e].x, b3 + 1), __shfl(z[e].y, b3 + 1)},
                     v2 = {__shfl(z[e].x, b3 + 2), __shfl(z[e].y, b3 + 2)};
          s[e] = cadd(cadd(v0, v1), v2);
        }
        cplx ma, mb; // a layer alone: the mean of its six z, no second parameter
        if (pair)
          ma = {s[0].x / 3.f, s[0].y / 3.f}, mb = {s[1].x / 3.f, s[1].y / 3.f};
        else
          ma = {(s[0].x + s[1].x) / 6.f, (s[0].y + s[1].y) / 6.f}, mb = {0.f, 0.f};
        const cplx h[2] = {{(ma.x + mb.x) * -beta, (ma.y + mb.y) * -beta}, {(ma.x - mb.x) * -beta, (ma.y - mb.y) * -beta}};
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int d = 0; d < 4; ++d)
            res[p][e][d] = (live && p < P && d < nds) ? chest_residual_at(x[e][d], h[e], pil[e][d]) : cplx{0.f, 0.f};
      }
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const cplx a = res[p][e][d];
            cd[p] += a.x * a.x + a.y * a.y;
#pragma unroll
            for (int q = 0; q < p; ++q) { // a conj(b)
              const cplx b = res[q][e][d];
              co[p * (p - 1) / 2 + q].x += a.x * b.x + a.y * b.y;
              co[p * (p - 1) / 2 + q].y += a.y * b.x - a.x * b.y;
            }
          }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      cd[p] += __shfl_xor(cd[p], off);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      co[k].x += __shfl_xor(co[k].x, off);
      co[k].y += __shfl_xor(co[k].y, off);
    }
  }
  if (lane != 0)
    return;
  int fitted = 0; // sum over the groups of 6 nds - f_g
  for (int grp = 0; grp < ngrp; ++grp)
    fitted += 6 * nds - (2 * grp + 1 < L ? 2 : 1);
  const float div = (float)n_j * (float)fitted;
  float       tr  = 0.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    cd[p] = cd[p] / div;
    if (p < P)
      tr += cd[p];
  }
  const float load = jm.loading * tr / (float)P;
  float2*     out  = cov + jm.cov_offset + (size_t)prg * P * P;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p >= P)
      continue;
    out[p * P + p] = make_float2(cd[p] + load, 0.f);
#pragma unroll
    for (int q = 0; q < p; ++q) {
      const float2 v = make_float2(co[p * (p - 1) / 2 + q].x / div, co[p * (p - 1) / 2 + q].y / div);
      out[p * P + q] = v;
      out[q * P + p] = make_float2(v.x, -v.y);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Carrier frequency offset (miphy_dmrs_pusch_estimate_cfo_batch; include/miphy.h has the arithmetic). The offset of a job is a sum over the
// workgroups of (job, port, CDM group), so there are two launches and no atomics: cfo_corr_kernel leaves, per (job, port, layer, gap between
// consecutive DM-RS symbols), the correlation of the per-symbol fits and the root of the product of their energies in a workspace;
// chest_cfo_kernel -- every workgroup of the job, in the same fixed order, so all get the same bits -- adds them up to cfo_hz and rho, turns the
// offset into one phasor per OFDM symbol and then follows chest_layers_kernel on derotated DM-RS elements, storing every symbol rotated back.
constexpr int CFO_PART_FLOATS = 4;                       // Re C, Im C, sqrt(energy product), spare: one 16-byte store
constexpr int CFO_JOB_FLOATS  = 4 * 4 * 3 * CFO_PART_FLOATS; // [port][layer][gap]
constexpr int CFO_LDS_BYTES   = 128;                     // behind chest_lds: 14 phasors, cfo_hz, rho

__host__ __device__ inline bool cfo_job_ok(const miphy_pusch_chest_cfo_job& j)
{
  return chest_job_rule(j.base, false) == CHEST_RULE_NONE && j.base.ce_compact == 0;
}

__host__ __device__ inline bool tv_job_ok(const miphy_pusch_chest_tv_job& j)
{
  bool ok = cfo_job_ok(j.base) && (j.time_mode == MIPHY_TIME_INTERPOLATE || j.time_mode == MIPHY_TIME_LINE);
  for (int i = 0; i < 7; ++i)
    ok = ok && j.reserved[i] == 0;
  return ok;
}

// What cfo_corr_kernel sees of either record: the rules it is held to and the CFO record in front.
__host__ __device__ inline bool cfo_record_ok(const miphy_pusch_chest_cfo_job& j)
{
  return cfo_job_ok(j);
}
__host__ __device__ inline bool cfo_record_ok(const miphy_pusch_chest_tv_job& j)
{
  return tv_job_ok(j);
}
__host__ __device__ inline const miphy_pusch_chest_cfo_job& cfo_record(const miphy_pusch_chest_cfo_job& j)
{
  return j;
}
__host__ __device__ inline const miphy_pusch_chest_cfo_job& cfo_record(const miphy_pusch_chest_tv_job& j)
{
  return j.base;
}

// tau_l - tau_ref in samples at 2048 * 2^mu * 15 kHz, tau the start of the useful part of an OFDM symbol of the slot (normal cyclic prefix): a
// symbol lasts 2048 + 144 samples, 16 * 2^mu more where (14 slot + j) mod (7 * 2^mu) = 0 (the rule of miphy_ofdm_symbol_size).
__host__ __device__ inline int cfo_symbol_delta(unsigned mu, unsigned slot, int ref, int l)
{
  const auto extra = [&](int j) -> int { return (14u * slot + (unsigned)j) % (7u << mu) == 0 ? (16 << mu) : 0; };
  const int  lo = l < ref ? l : ref, hi = l < ref ? ref : l;
  int        d  = extra(hi) - extra(lo);
  for (int j = lo; j < hi; ++j)
    d += 2048 + 144 + extra(j);
  return l < ref ? -d : d;
}

__device__ __forceinline__ float cfo_sample_rate(unsigned mu)
{
  return 2048.f * 15000.f * (float)(1u << mu);
}

// The DM-RS elements of the pilot pairs of this thread (the fetch of chest_layers_kernel).
__device__ __forceinline__ void cfo_fetch(float2 (&xq)[CL_PK][2][4], const float2* g, const uint16_t* prb_of, const int (&dsym)[4], int nds, int npairs, int nsc, int grp,
                                          int tid)
{
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * CHEST_THREADS;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      xq[kk][0][d] = xq[kk][1][d] = make_float2(0.f, 0.f);
      if (m < npairs && d < nds) {
        const float2* src = g + (size_t)dsym[d] * nsc + prb_of[m / 3] * 12 + 4 * (m % 3) + grp;
        xq[kk][0][d] = src[0];
        xq[kk][1][d] = src[2];
      }
    }
  }
}

// cfo_hz and rho of the job (blockIdx.x) into cfo_s[0..1] from the partials of every (port, layer, gap) (thread 0, in a fixed order: every workgroup of the job gets
// the same bits), then exp(+j phi_l) of the fourteen symbols into ph[]; returns cfo_hz. The text of chest_cfo_kernel, which keeps its own: called from here the compiler
// fuses three of that kernel's multiply-adds differently, and its bytes are pinned. Holds one barrier; ph[] may be read after the caller's next one.
__device__ __forceinline__ float cfo_offset_phasors(const miphy_pusch_chest_job& job, const float* parts, const int (&dsym)[4], int nds, int L, float2* ph, float* cfo_s,
                                                   int tid)
{
  if (tid == 0) {
    cplx  c[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    float e[3] = {0.f, 0.f, 0.f};
    const float* pj = parts + (size_t)blockIdx.x * CFO_JOB_FLOATS;
    for (int p = 0; p < (nds >= 2 ? (int)job.nof_rx_ports : 0); ++p)
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (d >= nds - 1)
            continue;
          const float4 v = *reinterpret_cast<const float4*>(pj + ((p * 4 + l) * 3 + d) * CFO_PART_FLOATS);
          c[d].x += v.x, c[d].y += v.y, e[d] += v.z;
        }
    float num = 0.f, sum_c = 0.f, sum_e = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= nds - 1)
        continue;
      const float mag = sqrtf(c[d].x * c[d].x + c[d].y * c[d].y);
      const int   ds  = cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[d], dsym[d + 1]);
      if (mag > 0.f)
        num += mag * (atan2f(c[d].y, c[d].x) * 0.15915494309189533577f) * (cfo_sample_rate(job.numerology) / (float)ds);
      sum_c += mag, sum_e += e[d];
    }
    const bool have = sum_c > 0.f;
    cfo_s[0] = have ? num / sum_c : 0.f;
    cfo_s[1] = have ? sum_c / sum_e : 0.f;
  }
  __syncthreads();
  const float cfo_hz = cfo_s[0];
  if (tid < 14) {
    float sn, cs;
    sincospif(2.f * cfo_hz * ((float)cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[0], tid) / cfo_sample_rate(job.numerology)), &sn, &cs);
    ph[tid] = make_float2(cs, sn);
  }
  return cfo_hz;
}

// x_d exp(-j phi_d) on the fetched DM-RS elements.
__device__ __forceinline__ void cfo_derotate(float2 (&xq)[CL_PK][2][4], const float2* ph, const int (&dsym)[4], int nds)
{
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (d >= nds)
      continue;
    const float2 r = ph[dsym[d]];
#pragma unroll
    for (int kk = 0; kk < CL_PK; ++kk)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float2 x = xq[kk][e][d];
        xq[kk][e][d]   = make_float2(x.x * r.x + x.y * r.y, x.y * r.x - x.x * r.y);
      }
  }
}

// Workgroup per (job, rx port, CDM group), the grid of chest_layers_kernel; no IDFT buffer and no LS vector, so 2.3 KB of LDS.
// JOB: miphy_pusch_chest_cfo_job or miphy_pusch_chest_tv_job (the stride of the records and the rules differ, nothing else).
template <class JOB>
__global__ void __launch_bounds__(CHEST_THREADS) cfo_corr_kernel(const JOB* __restrict__ jobs, const gold_jump* __restrict__ gj,
                                                                 const float2* __restrict__ grid, float* __restrict__ parts, int ports_dim)
{
  __shared__ uint32_t cbits[4 * 104];
  __shared__ uint64_t rbm[5];
  __shared__ uint16_t prb_of[276];
  __shared__ float    red[CHEST_THREADS / 64];
  const int tid = threadIdx.x;
  const miphy_pusch_chest_cfo_job& jm = cfo_record(jobs[blockIdx.x]);
  const int port = blockIdx.y % ports_dim, grp = blockIdx.y / ports_dim;
  const int L    = jm.base.nof_tx_layers;
  // (uniform) a job without this port or group; a device-resident job that breaks a rule
  if (port >= jm.base.nof_rx_ports || 2 * grp >= L || !cfo_record_ok(jobs[blockIdx.x]))
    return;
  const miphy_pusch_chest_job job = load_words(&jm.base);
  int       dsym[4];
  const int nds = chest_dmrs_symbols(job.symbols_mask, job.first_symbol, job.first_symbol + job.nof_symbols, dsym);
  if (nds < 2) // no gap: chest_cfo_kernel reads nothing
    return;
  const bool pair = 2 * grp + 1 < L; // both layers of the group are present
  const int  nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  const int  nprb = chest_prb_list(jm.base.rb_mask, nprb_grid, rbm, prb_of, tid);
  const int  npairs = nprb * 3;
  float2     xq[CL_PK][2][4];
  cfo_fetch(xq, chest_port_grid(grid, job, port), prb_of, dsym, nds, npairs, nsc, grp, tid);
  uint32_t c_init[4];
  chest_c_init(job, dsym, nds, c_init);
  gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], nds, 12 * nprb_grid, cbits, tid);

  // s[e]: both layers present, s_a and s_b of the pair; a layer alone, its z on the two pilots of the pair
  const float ib = 1.0f / job.scaling;
  cplx        cacc[2][3];
  float       eacc[2][4];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
#pragma unroll
    for (int d = 0; d < 3; ++d)
      cacc[e][d] = {0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d)
      eacc[e][d] = 0.f;
  }
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * CHEST_THREADS;
    if (m >= npairs)
      continue;
    const int gp0 = prb_of[m / 3] * 6 + 2 * (m % 3);
    cplx      prev[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (d >= nds)
        continue;
      cplx s[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const cplx   p = chest_qpsk_pilot(cbits, d, gp0 + e);
        const float2 x = xq[kk][e][d];
        s[e]           = {(x.x * p.x + x.y * p.y) * ib, (x.y * p.x - x.x * p.y) * ib};
      }
      if (pair) {
        const cplx sa = {(s[0].x + s[1].x) * 0.5f, (s[0].y + s[1].y) * 0.5f}, sb = {(s[0].x - s[1].x) * 0.5f, (s[0].y - s[1].y) * 0.5f};
        s[0] = sa, s[1] = sb;
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        eacc[e][d] += s[e].x * s[e].x + s[e].y * s[e].y;
        if (d > 0) { // s_{d} conj(s_{d-1})
          cacc[e][d - 1].x += s[e].x * prev[e].x + s[e].y * prev[e].y;
          cacc[e][d - 1].y += s[e].y * prev[e].x - s[e].x * prev[e].y;
        }
        prev[e] = s[e];
      }
    }
  }
  // a layer alone: the sums over its even and odd pilots are one sum
  if (!pair) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      eacc[0][d] += eacc[1][d];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      cacc[0][d] = cadd(cacc[0][d], cacc[1][d]);
  }
  const int nlay = pair ? 2 : 1;
  float*    out  = parts + (size_t)blockIdx.x * CFO_JOB_FLOATS + (size_t)(port * 4 + 2 * grp) * 3 * CFO_PART_FLOATS;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (e >= nlay) // (uniform)
      continue;
    float en[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < nds)
        en[d] = block_sum(eacc[e][d], red, tid);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= nds - 1)
        continue;
      const float cr = block_sum(cacc[e][d].x, red, tid), ci = block_sum(cacc[e][d].y, red, tid);
      if (tid == 0)
        *reinterpret_cast<float4*>(out + (e * 3 + d) * CFO_PART_FLOATS) = make_float4(cr, ci, sqrtf(en[d + 1] * en[d]), 0.f);
    }
  }
}

// chest_layers_kernel for jobs on one to four layers, with the offset taken out of the DM-RS elements and put back into every stored symbol.
__global__ void __launch_bounds__(CHEST_THREADS, 4) chest_cfo_kernel(const miphy_pusch_chest_cfo_job* __restrict__ jobs,
                                                                     const gold_jump* __restrict__ gj,
                                                                     const cplx* __restrict__ tw,
                                                                     const float2* __restrict__ grid,
                                                                     float2* __restrict__ ce_out,
                                                                     float* __restrict__ scalars,
                                                                     const float* __restrict__ parts,
                                                                     float* __restrict__ cfo_out,
                                                                     int ports_dim) // blockIdx.y = CDM group * ports_dim + port
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const chest_lds lds(smem);
  float2*         ph    = reinterpret_cast<float2*>(smem + chest_lds::BYTES); // 14: exp(+j phi_l)
  float*          cfo_s = reinterpret_cast<float*>(ph + 14);                   // cfo_hz, rho
  constexpr int nt = CHEST_THREADS;
  const int     tid = threadIdx.x;
  const miphy_pusch_chest_cfo_job& jm = jobs[blockIdx.x];
  const int port = blockIdx.y % ports_dim, grp = blockIdx.y / ports_dim;
  const int L    = jm.base.nof_tx_layers;
  // (uniform) a job without this port or group; a device-resident job that breaks a rule
  if (port >= jm.base.nof_rx_ports || 2 * grp >= L || !cfo_job_ok(jm))
    return;
  const miphy_pusch_chest_job job = load_words(&jm.base);
  const bool pair = 2 * grp + 1 < L; // both layers of the group are present
  const int  nlay = pair ? 2 : 1;
  const int  nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  const int  first = job.first_symbol, nsymb_out = first + job.nof_symbols;
  int        dsym[4];
  const int  nds  = chest_dmrs_symbols(job.symbols_mask, first, nsymb_out, dsym);
  const int  nprb = chest_prb_list(jm.base.rb_mask, nprb_grid, lds.rbm, lds.prb_of, tid);
  const int  np = nprb * 6, npairs = nprb * 3;
  const float beta = job.scaling;
  float2      xq[CL_PK][2][4];
  cfo_fetch(xq, chest_port_grid(grid, job, port), lds.prb_of, dsym, nds, npairs, nsc, grp, tid);

  // ---- the offset from the partials of every (port, layer, gap) of the job, under the memory requests above
  if (tid == 0) {
    cplx  c[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    float e[3] = {0.f, 0.f, 0.f};
    const float* pj = parts + (size_t)blockIdx.x * CFO_JOB_FLOATS;
    for (int p = 0; p < (nds >= 2 ? (int)job.nof_rx_ports : 0); ++p)
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (d >= nds - 1)
            continue;
          const float4 v = *reinterpret_cast<const float4*>(pj + ((p * 4 + l) * 3 + d) * CFO_PART_FLOATS);
          c[d].x += v.x, c[d].y += v.y, e[d] += v.z;
        }
    float num = 0.f, sum_c = 0.f, sum_e = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= nds - 1)
        continue;
      const float mag = sqrtf(c[d].x * c[d].x + c[d].y * c[d].y);
      const int   ds  = cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[d], dsym[d + 1]);
      if (mag > 0.f)
        num += mag * (atan2f(c[d].y, c[d].x) * 0.15915494309189533577f) * (cfo_sample_rate(job.numerology) / (float)ds);
      sum_c += mag, sum_e += e[d];
    }
    const bool have = sum_c > 0.f;
    cfo_s[0] = have ? num / sum_c : 0.f;
    cfo_s[1] = have ? sum_c / sum_e : 0.f;
  }
  __syncthreads();
  const float cfo_hz = cfo_s[0];
  if (tid < 14) {
    float sn, cs;
    sincospif(2.f * cfo_hz * ((float)cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[0], tid) / cfo_sample_rate(job.numerology)), &sn, &cs);
    ph[tid] = make_float2(cs, sn);
  }
  uint32_t c_init[4];
  chest_c_init(job, dsym, nds, c_init);
  gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], nds, 12 * nprb_grid, lds.cbits, tid); // (barrier: ph[])
  if (tid == 0 && port == 0 && grp == 0) {
    float* o = cfo_out + jm.cfo_offset;
    o[0] = cfo_hz, o[1] = cfo_s[1];
  }
  cfo_derotate(xq, ph, dsym, nds); // x_d exp(-j phi_d)

  // ---- from here chest_layers_kernel: least squares against layer 0's pilot, despreading, EPRE, RSRP
  const float ts = 1.0f / ((float)nds * beta);
  float       epre_acc = 0.f, ra_acc = 0.f, rb_acc = 0.f;
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * nt;
    if (m >= npairs)
      continue;
    const int gp0 = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
    cplx      z[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const cplx acc = chest_ls(xq[kk][e], nds, epre_acc, [&](int d) { return chest_qpsk_pilot(lds.cbits, d, gp0 + e); });
      z[e]           = {acc.x * ts, acc.y * ts};
    }
    if (pair) {
      const cplx sa = {(z[0].x + z[1].x) * 0.5f, (z[0].y + z[1].y) * 0.5f}, sb = {(z[0].x - z[1].x) * 0.5f, (z[0].y - z[1].y) * 0.5f};
      lds.lse[2 * m] = sa, lds.lse[2 * m + 1] = sb;
      ra_acc += sa.x * sa.x + sa.y * sa.y;
      rb_acc += sb.x * sb.x + sb.y * sb.y;
    } else {
      lds.lse[2 * m] = z[0], lds.lse[2 * m + 1] = z[1];
      ra_acc += z[0].x * z[0].x + z[0].y * z[0].y + z[1].x * z[1].x + z[1].y * z[1].y;
    }
  }
  const float epre    = block_sum(epre_acc, lds.red, tid) / (float)(np * nds);
  const float rs_norm = beta * beta / (float)(pair ? npairs : np);
  float       rsrp[2];
  rsrp[0] = block_sum(ra_acc, lds.red, tid) * rs_norm;
  rsrp[1] = pair ? block_sum(rb_acc, lds.red, tid) * rs_norm : 0.f;
  __syncthreads(); // lse[]

  // ---- interpolation, to every OFDM symbol with the symbol's phasor
  const int sh = pair ? 2 : 1, off = pair ? 1 + grp : grp, ninp = pair ? npairs : np;
  for (int l = 0; l < nlay; ++l) {
    float2*    dst0   = chest_ce_rows(ce_out, job, 2 * grp + l, port);
    const auto anchor = [&](int i) -> cplx { return pair ? lds.lse[2 * i + l] : lds.lse[i]; };
    for (int k = tid; k < nprb * 12; k += nt) {
      const cplx   v   = chest_interpolate<false>(anchor, k, sh, off, ninp);
      const size_t col = (size_t)lds.prb_of[k / 12] * 12 + (k % 12);
      for (int sy = first; sy < nsymb_out; ++sy) {
        const float2 r = ph[sy];
        dst0[(size_t)sy * nsc + col] = make_float2(v.x * r.x - v.y * r.y, v.x * r.y + v.y * r.x);
      }
    }
  }

  // ---- noise, as chest_layers_kernel, on the derotated elements
  float noise_var = 0.001f * epre; // convert_dB_to_power(-30) * epre
  if (nds >= 3) {
    float noise_acc = 0.f;
#pragma unroll
    for (int kk = 0; kk < CL_PK; ++kk) {
      const int m = tid + kk * nt;
      if (m >= npairs)
        continue;
      const int  b  = (m / 3) * 6;
      const cplx ea = cadd(cadd(lds.lse[b], lds.lse[b + 2]), lds.lse[b + 4]), eo = cadd(cadd(lds.lse[b + 1], lds.lse[b + 3]), lds.lse[b + 5]);
      cplx       ma, mb; // a layer alone: the mean of its six z, no second parameter
      if (pair)
        ma = {ea.x / 3.f, ea.y / 3.f}, mb = {eo.x / 3.f, eo.y / 3.f};
      else
        ma = {(ea.x + eo.x) / 6.f, (ea.y + eo.y) / 6.f}, mb = {0.f, 0.f};
      const cplx h[2] = {{(ma.x + mb.x) * -beta, (ma.y + mb.y) * -beta}, {(ma.x - mb.x) * -beta, (ma.y - mb.y) * -beta}};
      const int  gp0  = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
#pragma unroll
      for (int e = 0; e < 2; ++e)
        chest_residual(xq[kk][e], nds, h[e], noise_acc, [&](int d) { return chest_qpsk_pilot(lds.cbits, d, gp0 + e); });
    }
    noise_var = block_sum(noise_acc, lds.red, tid) / (float)np * 6.f / (float)(6 * nds - nlay);
  }

  // ---- time alignment per layer
  float ta[2] = {0.f, 0.f};
  for (int l = 0; l < nlay; ++l) {
    chest_clear_idft(lds.fbuf, tid);
    __syncthreads();
    for (int i = tid; i < np; i += nt)
      lds.fbuf[fpad(lds.prb_of[i / 6] * 12 + 2 * (i % 6) + grp)] = pair ? lds.lse[(i & ~1) + l] : lds.lse[i];
    __syncthreads();
    fft4096_lds<true>(lds.fbuf, tw, tid);
    ta[l] = chest_ta_peak(lds.fbuf, lds.red, tid);
  }

  // ---- side-band scalars, per layer; the noise variance is the group's
  if (tid < nlay)
    chest_scalars(scalars, job, port, 2 * grp + tid, tid ? rsrp[1] : rsrp[0], epre, noise_var, tid ? ta[1] : ta[0], true, true);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// A channel that changes within the slot (miphy_dmrs_pusch_estimate_tv_batch; include/miphy.h has the arithmetic). chest_cfo_kernel up to the
// derotated DM-RS elements; then the fits of the DM-RS symbols are kept apart, one vector per symbol in LDS, and blended in time with the weights
// w[l][d]. Frequency interpolation and the time blend are both linear, so a thread interpolates the nds vectors once per subcarrier, keeps the nds
// values in registers and runs the loop over the symbols from them: no barrier in the store loop, every store 512 consecutive columns of one row.
// LDS: the fit vectors (4 x 1 650 pilots, 52.8 KB) lie over the IDFT buffer and the LS vector of chest_lds, which are idle until the time
// alignment; the time mean waits in registers until the fits are dead and then takes the LS vector's place. 55.5 KB: two workgroups on a CU.
struct tv_lds {
  static constexpr size_t FITS_BYTES = 4 * MAX_PILOTS * sizeof(cplx), TAIL = chest_lds::BYTES - chest_lds::CBITS, PH = FITS_BYTES + TAIL,
                          WT = PH + CFO_LDS_BYTES, BYTES = WT + 14 * 4 * sizeof(float);
  static_assert(FITS_BYTES >= chest_lds::CBITS && FITS_BYTES % 16 == 0 && WT % 16 == 0, "the IDFT buffer and the LS vector lie inside the fit vectors");
  cplx*     fits;   // nds vectors of np fits, vector d at d * np; s_a / s_b interleaved like chest_lds::lse
  cplx*     fbuf;   // over fits: the IDFT buffer
  cplx*     lse;    // over fits, behind fbuf: the time mean, for the time alignment
  uint32_t* cbits;  // from here the arrays of chest_lds
  uint64_t* rbm;
  uint16_t* prb_of;
  float*    red;
  float2*   ph;     // 14: exp(+j phi_l)
  float*    cfo_s;  // cfo_hz, rho
  float*    wt;     // 14 x 4: w[l][d]
  __device__ __forceinline__ explicit tv_lds(unsigned char* s)
    : fits(reinterpret_cast<cplx*>(s)), fbuf(reinterpret_cast<cplx*>(s)), lse(reinterpret_cast<cplx*>(s + chest_lds::LSE)),
      cbits(reinterpret_cast<uint32_t*>(s + FITS_BYTES)), rbm(reinterpret_cast<uint64_t*>(s + FITS_BYTES + (chest_lds::RBM - chest_lds::CBITS))),
      prb_of(reinterpret_cast<uint16_t*>(s + FITS_BYTES + (chest_lds::PRB_OF - chest_lds::CBITS))),
      red(reinterpret_cast<float*>(s + FITS_BYTES + (chest_lds::RED - chest_lds::CBITS))), ph(reinterpret_cast<float2*>(s + PH)),
      cfo_s(reinterpret_cast<float*>(s + PH) + 28), wt(reinterpret_cast<float*>(s + WT))
  {
  }
};

// w[l][0..3] of OFDM symbol l, from differences of the symbol times only (samples are whole numbers below 2^24: exact in single precision).
__device__ __forceinline__ float4 tv_weights(const miphy_pusch_chest_job& job, const int (&dsym)[4], int nds, int mode, int l)
{
  float w[4] = {1.f, 0.f, 0.f, 0.f};
  if (nds >= 2 && mode == MIPHY_TIME_INTERPOLATE) {
    int j = 0;
#pragma unroll
    for (int d = 1; d < 3; ++d)
      if (d < nds - 1 && dsym[d] <= l)
        j = d;
    int lo = dsym[0], hi = dsym[1];
#pragma unroll
    for (int d = 1; d < 3; ++d)
      if (d == j)
        lo = dsym[d], hi = dsym[d + 1];
    const float u = (float)cfo_symbol_delta(job.numerology, job.slot_in_frame, lo, l) / (float)cfo_symbol_delta(job.numerology, job.slot_in_frame, lo, hi);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      w[d] = d == j ? 1.f - u : (d == j + 1 ? u : 0.f);
  } else if (nds >= 2) {
    float t[4], tm = 0.f, q = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      t[d] = d < nds ? (float)cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[0], dsym[d]) : 0.f;
      tm += t[d];
    }
    tm /= (float)nds;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < nds)
        q += (t[d] - tm) * (t[d] - tm);
    const float tl = (float)cfo_symbol_delta(job.numerology, job.slot_in_frame, dsym[0], l) - tm;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      w[d] = d < nds ? 1.f / (float)nds + tl * (t[d] - tm) / q : 0.f;
  }
  return make_float4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(CHEST_THREADS, 4) chest_tv_kernel(const miphy_pusch_chest_tv_job* __restrict__ jobs,
                                                                    const gold_jump* __restrict__ gj,
                                                                    const cplx* __restrict__ tw,
                                                                    const float2* __restrict__ grid,
                                                                    float2* __restrict__ ce_out,
                                                                    float* __restrict__ scalars,
                                                                    const float* __restrict__ parts,
                                                                    float* __restrict__ cfo_out,
                                                                    float* __restrict__ var_out,
                                                                    int ports_dim) // blockIdx.y = CDM group * ports_dim + port
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const tv_lds  lds(smem);
  constexpr int nt = CHEST_THREADS;
  const int     tid = threadIdx.x;
  const miphy_pusch_chest_tv_job& jm = jobs[blockIdx.x];
  const int port = blockIdx.y % ports_dim, grp = blockIdx.y / ports_dim;
  const int L    = jm.base.base.nof_tx_layers;
  // (uniform) a job without this port or group; a device-resident job that breaks a rule
  if (port >= jm.base.base.nof_rx_ports || 2 * grp >= L || !tv_job_ok(jm))
    return;
  const miphy_pusch_chest_job job = load_words(&jm.base.base);
  const int  mode = jm.time_mode;
  const bool pair = 2 * grp + 1 < L; // both layers of the group are present
  const int  nlay = pair ? 2 : 1;
  const int  nprb_grid = job.grid_nof_prb, nsc = nprb_grid * 12;
  const int  first = job.first_symbol, nsymb_out = first + job.nof_symbols;
  int        dsym[4];
  const int  nds  = chest_dmrs_symbols(job.symbols_mask, first, nsymb_out, dsym);
  const int  nprb = chest_prb_list(jm.base.base.rb_mask, nprb_grid, lds.rbm, lds.prb_of, tid);
  const int  np = nprb * 6, npairs = nprb * 3;
  const float beta = job.scaling;
  float2      xq[CL_PK][2][4];
  cfo_fetch(xq, chest_port_grid(grid, job, port), lds.prb_of, dsym, nds, npairs, nsc, grp, tid);

  // ---- the offset and the phasors as chest_cfo_kernel, the time weights next to them
  const float cfo_hz = cfo_offset_phasors(job, parts, dsym, nds, L, lds.ph, lds.cfo_s, tid);
  if (tid < 14)
    *reinterpret_cast<float4*>(lds.wt + 4 * tid) = tv_weights(job, dsym, nds, mode, tid);
  uint32_t c_init[4];
  chest_c_init(job, dsym, nds, c_init);
  gold_bits_block(*reinterpret_cast<const gold_tables*>(gj), c_init[0], c_init[1], c_init[2], c_init[3], nds, 12 * nprb_grid, lds.cbits, tid); // (barrier: ph[], wt[])
  if (tid == 0 && port == 0 && grp == 0) {
    float* o = cfo_out + jm.base.cfo_offset;
    o[0] = cfo_hz, o[1] = lds.cfo_s[1];
  }
  cfo_derotate(xq, lds.ph, dsym, nds); // x_d exp(-j phi_d)

  // ---- the fit of every DM-RS symbol on its own: least squares against layer 0's pilot, despreading; the time mean, EPRE, RSRP and the energy the
  // mean leaves over. S[e]: both layers present, S_a and S_b of the pair; a layer alone, its z on the two pilots of the pair.
  const float ib = 1.0f / beta, inds = 1.0f / (float)nds;
  cplx        mean[CL_PK][2];
  float       epre_acc = 0.f, r_acc[2] = {0.f, 0.f}, dev_acc[2] = {0.f, 0.f}, en_acc[2] = {0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * nt;
    mean[kk][0] = mean[kk][1] = {0.f, 0.f};
    if (m >= npairs)
      continue;
    const int gp0 = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
    cplx      S[4][2];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      S[d][0] = S[d][1] = {0.f, 0.f};
      if (d >= nds)
        continue;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const cplx   p = chest_qpsk_pilot(lds.cbits, d, gp0 + e);
        const float2 x = xq[kk][e][d];
        S[d][e]        = {(x.x * p.x + x.y * p.y) * ib, (x.y * p.x - x.x * p.y) * ib};
        epre_acc += x.x * x.x + x.y * x.y;
      }
      if (pair) {
        const cplx sa = {(S[d][0].x + S[d][1].x) * 0.5f, (S[d][0].y + S[d][1].y) * 0.5f}, sb = {(S[d][0].x - S[d][1].x) * 0.5f, (S[d][0].y - S[d][1].y) * 0.5f};
        S[d][0] = sa, S[d][1] = sb;
      }
      lds.fits[d * np + 2 * m] = S[d][0], lds.fits[d * np + 2 * m + 1] = S[d][1];
#pragma unroll
      for (int e = 0; e < 2; ++e)
        mean[kk][e] = cadd(mean[kk][e], S[d][e]);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      mean[kk][e] = {mean[kk][e].x * inds, mean[kk][e].y * inds};
      r_acc[e] += mean[kk][e].x * mean[kk][e].x + mean[kk][e].y * mean[kk][e].y;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (d >= nds)
          continue;
        const cplx dv = {S[d][e].x - mean[kk][e].x, S[d][e].y - mean[kk][e].y};
        dev_acc[e] += dv.x * dv.x + dv.y * dv.y;
        en_acc[e] += S[d][e].x * S[d][e].x + S[d][e].y * S[d][e].y;
      }
    }
  }
  if (!pair) // a layer alone: the sums over its even and odd pilots are one sum
    r_acc[0] += r_acc[1], dev_acc[0] += dev_acc[1], en_acc[0] += en_acc[1];
  const float epre    = block_sum(epre_acc, lds.red, tid) / (float)(np * nds);
  const float rs_norm = beta * beta / (float)(pair ? npairs : np);
  float       rsrp[2] = {0.f, 0.f}, var[2] = {0.f, 0.f};
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    if (l >= nlay) // (uniform)
      continue;
    rsrp[l] = block_sum(r_acc[l], lds.red, tid) * rs_norm;
    const float dev = block_sum(dev_acc[l], lds.red, tid), en = block_sum(en_acc[l], lds.red, tid);
    var[l] = (nds >= 2 && en > 0.f) ? dev / en : 0.f;
  }
  __syncthreads(); // fits[]

  // ---- frequency interpolation of every fit vector, once per subcarrier; then every OFDM symbol from registers: the blend in time, the symbol's phasor
  const int sh = pair ? 2 : 1, off = pair ? 1 + grp : grp, ninp = pair ? npairs : np;
  for (int l = 0; l < nlay; ++l) {
    float2* dst0 = chest_ce_rows(ce_out, job, 2 * grp + l, port);
    for (int k = tid; k < nprb * 12; k += nt) {
      cplx v[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        v[d] = {0.f, 0.f};
        if (d >= nds)
          continue;
        const cplx* f      = lds.fits + d * np;
        const auto  anchor = [&](int i) -> cplx { return pair ? f[2 * i + l] : f[i]; };
        v[d]               = chest_interpolate<false>(anchor, k, sh, off, ninp);
      }
      const size_t col = (size_t)lds.prb_of[k / 12] * 12 + (k % 12);
      for (int sy = first; sy < nsymb_out; ++sy) {
        const float4 w = *reinterpret_cast<const float4*>(lds.wt + 4 * sy);
        const float2 r = lds.ph[sy];
        const cplx   a = {w.x * v[0].x + w.y * v[1].x + w.z * v[2].x + w.w * v[3].x, w.x * v[0].y + w.y * v[1].y + w.z * v[2].y + w.w * v[3].y};
        dst0[(size_t)sy * nsc + col] = make_float2(a.x * r.x - a.y * r.y, a.x * r.y + a.y * r.x);
      }
    }
  }

  // ---- noise against the fit in time: F_d = sum_d' w[dsym[d]][d'] S_d', its per-PRB means predict the observations of DM-RS symbol d
  float noise_var = 0.001f * epre; // convert_dB_to_power(-30) * epre
  if (nds >= 2) {
    float noise_acc = 0.f;
#pragma unroll
    for (int kk = 0; kk < CL_PK; ++kk) {
      const int m = tid + kk * nt;
      if (m >= npairs)
        continue;
      const int b = (m / 3) * 6;
      cplx      ea[4], eo[4]; // per-PRB sums of the even and odd entries of every fit vector
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        ea[d] = eo[d] = {0.f, 0.f};
        if (d >= nds)
          continue;
        const cplx* f = lds.fits + d * np + b;
        ea[d] = cadd(cadd(f[0], f[2]), f[4]), eo[d] = cadd(cadd(f[1], f[3]), f[5]);
      }
      const int gp0 = lds.prb_of[m / 3] * 6 + 2 * (m % 3);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (d >= nds)
          continue;
        const float4 w  = *reinterpret_cast<const float4*>(lds.wt + 4 * dsym[d]);
        const cplx   fa = {w.x * ea[0].x + w.y * ea[1].x + w.z * ea[2].x + w.w * ea[3].x, w.x * ea[0].y + w.y * ea[1].y + w.z * ea[2].y + w.w * ea[3].y};
        const cplx   fo = {w.x * eo[0].x + w.y * eo[1].x + w.z * eo[2].x + w.w * eo[3].x, w.x * eo[0].y + w.y * eo[1].y + w.z * eo[2].y + w.w * eo[3].y};
        cplx         ma, mb; // a layer alone: the mean of its six, no second parameter
        if (pair)
          ma = {fa.x / 3.f, fa.y / 3.f}, mb = {fo.x / 3.f, fo.y / 3.f};
        else
          ma = {(fa.x + fo.x) / 6.f, (fa.y + fo.y) / 6.f}, mb = {0.f, 0.f};
        const cplx h[2] = {{(ma.x + mb.x) * -beta, (ma.y + mb.y) * -beta}, {(ma.x - mb.x) * -beta, (ma.y - mb.y) * -beta}};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const cplx r = chest_residual_at(xq[kk][e][d], h[e], chest_qpsk_pilot(lds.cbits, d, gp0 + e));
          noise_acc += r.x * r.x + r.y * r.y;
        }
      }
    }
    const int fitted = mode == MIPHY_TIME_INTERPOLATE ? nds : 2; // parameters in time per layer and PRB (nds >= 2 here)
    noise_var        = block_sum(noise_acc, lds.red, tid) / (float)nprb / (float)(6 * nds - nlay * fitted);
  }

  // ---- the fits are dead: the time mean takes the place of the LS vector, and from here chest_layers_kernel's time alignment per layer
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < CL_PK; ++kk) {
    const int m = tid + kk * nt;
    if (m < npairs)
      lds.lse[2 * m] = mean[kk][0], lds.lse[2 * m + 1] = mean[kk][1];
  }
  float ta[2] = {0.f, 0.f};
  for (int l = 0; l < nlay; ++l) {
    chest_clear_idft(lds.fbuf, tid);
    __syncthreads(); // (lse[] too)
    for (int i = tid; i < np; i += nt)
      lds.fbuf[fpad(lds.prb_of[i / 6] * 12 + 2 * (i % 6) + grp)] = pair ? lds.lse[(i & ~1) + l] : lds.lse[i];
    __syncthreads();
    fft4096_lds<true>(lds.fbuf, tw, tid);
    ta[l] = chest_ta_peak(lds.fbuf, lds.red, tid);
  }

  // ---- side-band scalars and the variation, per layer; the noise variance is the group's
  if (tid < nlay) {
    chest_scalars(scalars, job, port, 2 * grp + tid, tid ? rsrp[1] : rsrp[0], epre, noise_var, tid ? ta[1] : ta[0], true, true);
    var_out[jm.var_offset + (size_t)port * L + 2 * grp + tid] = tid ? var[1] : var[0];
  }
}

} // namespace

// The rules a batch of host jobs is held to (chest_job_rule), and its largest port and layer counts.
static int chest_validate(const miphy_pusch_chest_job* jobs, uint32_t n, bool pilots, unsigned& max_ports, unsigned& max_layers, const char* what = "pusch_chest")
{
  max_ports = max_layers = 1;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_pusch_chest_job& j = jobs[i];
    const chest_rule r = chest_job_rule(j, pilots);
    MIPHY_REQUIRE(r != CHEST_RULE_NUMEROLOGY, "%s: job %u: invalid numerology", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_LAYERS, "%s: job %u: invalid number of layers %u", what, i, j.nof_tx_layers);
    MIPHY_REQUIRE(r != CHEST_RULE_PORTS, "%s: job %u: invalid number of rx ports %u", what, i, j.nof_rx_ports);
    MIPHY_REQUIRE(r != CHEST_RULE_GRID, "%s: job %u: invalid grid width", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_SYMBOLS, "%s: job %u: invalid symbol range", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_SCALING, "%s: job %u: the DM-RS to data scaling factor should be a positive number", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_DMRS, "%s: job %u: %u DM-RS symbols (1..4 supported)", what, i,
                  chest_nof_dmrs(j.symbols_mask, j.first_symbol, j.first_symbol + j.nof_symbols));
    MIPHY_REQUIRE(r != CHEST_RULE_NO_HOPPING, "%s: job %u: intra-slot frequency hopping is served by miphy_port_channel_estimate_batch", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_HOP_SYMBOL, "%s: job %u: hop symbol outside the allocation", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_HOP_COMPACT, "%s: job %u: the compact estimate holds one hop only", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_HOP_DMRS, "%s: job %u: every hop needs a DM-RS symbol", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_HOP_PRBS, "%s: job %u: the hops have different numbers of PRBs", what, i);
    MIPHY_REQUIRE(r != CHEST_RULE_EMPTY, "%s: job %u: empty allocation", what, i);
    max_ports  = j.nof_rx_ports > max_ports ? j.nof_rx_ports : max_ports;
    max_layers = j.nof_tx_layers > max_layers ? j.nof_tx_layers : max_layers;
  }
  return MIPHY_OK;
}

// What every entry point does first: arguments, the empty batch, the hints of device-resident jobs -- which the host cannot inspect: bits 8-11 /
// 12-15 of jobs_on_device may carry the largest nof_rx_ports / nof_tx_layers of the batch (0 = unknown: the grid is sized for 4 x 4 and the surplus
// workgroups exit at once) -- and the rules of host jobs (host_rules(max_ports, max_layers)). The caller returns when the result or n is 0.
template <class Rules>
static int chest_prologue(const char* what, bool args, uint32_t n, uint32_t max_n, int& jobs_on_device, unsigned& max_ports, unsigned& max_layers, Rules&& host_rules)
{
  MIPHY_REQUIRE(args, "%s: null argument", what);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= max_n, "%s: at most %u jobs per call", what, max_n);
  const unsigned hint_ports = ((unsigned)jobs_on_device >> 8) & 0xfu, hint_layers = ((unsigned)jobs_on_device >> 12) & 0xfu;
  jobs_on_device &= 0xff;
  MIPHY_REQUIRE(hint_ports <= 4 && hint_layers <= 4, "%s: invalid port / layer hint", what);
  max_ports = hint_ports ? hint_ports : 4, max_layers = hint_layers ? hint_layers : 4;
  return jobs_on_device ? MIPHY_OK : host_rules(max_ports, max_layers);
}

static int chest_resources(miphy_ctx* ctx, const cplx** tw, const gold_jump** gold)
{
  const float* t  = nullptr;
  int          rc = miphy_get_twiddles(ctx, CE_DFT, &t);
  if (!rc && !ctx->ext->d_gold)
    rc = miphy_get_gold_tables(ctx, nullptr);
  *tw = (const cplx*)t, *gold = (const gold_jump*)ctx->ext->d_gold;
  return rc;
}

// chest_kernel on staged jobs. One workgroup per (job, port, layer); two -- the time-alignment chain on its own -- where the launch leaves most of
// the chip idle anyway.
static int chest_enqueue(miphy_ctx* ctx, const void* d_jobs, uint32_t n, unsigned max_ports, unsigned max_layers, const float* grid, const float* pilots,
                         float* ce, float* scalars, hipStream_t s)
{
  const cplx*      tw;
  const gold_jump* gold;
  int              rc = chest_resources(ctx, &tw, &gold);
  if (rc)
    return rc;
  const int ngrp = ((uint64_t)n * max_ports * max_layers * 2 <= (uint64_t)ctx->num_cus) ? 2 : 1;
  hipLaunchKernelGGL(pilots ? chest_kernel<true> : chest_kernel<false>, dim3(n, max_ports * max_layers, ngrp), dim3(CHEST_THREADS), chest_lds::BYTES, s,
                     (const miphy_pusch_chest_job*)d_jobs, gold, tw, (const float2*)grid, (float2*)ce, scalars, (const float2*)pilots, (int)max_ports);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// chest_layers_kernel on staged jobs. One workgroup per (job, port, CDM group): the second group exists from three layers on.
static int chest_layers_enqueue(miphy_ctx* ctx, const void* d_jobs, uint32_t n, unsigned max_ports, unsigned max_layers, const float* grid, float* ce,
                                float* scalars, hipStream_t s)
{
  const cplx*      tw;
  const gold_jump* gold;
  int              rc = chest_resources(ctx, &tw, &gold);
  if (rc)
    return rc;
  hipLaunchKernelGGL(chest_layers_kernel, dim3(n, max_ports * (max_layers > 2 ? 2 : 1)), dim3(CHEST_THREADS), chest_lds::BYTES, s,
                     (const miphy_pusch_chest_job*)d_jobs, gold, tw, (const float2*)grid, (float2*)ce, scalars, (int)max_ports);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

static int chest_launch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n, const float* grid, const float* pilots, float* ce,
                        float* scalars, void* stream, const char* what)
{
  unsigned max_ports, max_layers;
  int      rc = chest_prologue(what, ctx && jobs && grid && ce && scalars, n, UINT32_MAX, jobs_on_device, max_ports, max_layers,
                               [&](unsigned& mp, unsigned& ml) { return chest_validate(jobs, n, pilots != nullptr, mp, ml); });
  if (rc || n == 0)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_job) * (size_t)n, s, &d_jobs)))
    return rc;
  return chest_enqueue(ctx, d_jobs, n, max_ports, max_layers, grid, pilots, ce, scalars, s);
}

// Layers that share a CDM group are separated (chest_layers_kernel); jobs on one layer go through chest_kernel<false> in a launch of their own, so
// they come out byte for byte as from miphy_dmrs_pusch_estimate_batch. Host jobs: that launch gets a list of the one-layer jobs only. Device-resident
// jobs: it gets a copy in which every other job has no receive port (chest_solo_jobs_kernel), whose workgroups leave at once.
extern "C" int miphy_dmrs_pusch_estimate_layers_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                      float* ce, float* scalars, void* stream)
{
  unsigned max_ports, max_layers;
  int      rc = chest_prologue("miphy_dmrs_pusch_estimate_layers_batch", ctx && jobs && grid && ce && scalars, n, UINT32_MAX, jobs_on_device, max_ports, max_layers,
                               [&](unsigned& mp, unsigned& ml) { return chest_validate(jobs, n, false, mp, ml); });
  if (rc || n == 0)
    return rc;
  hipStream_t                        s = (hipStream_t)stream;
  std::vector<miphy_pusch_chest_job> solo;
  if (!jobs_on_device)
    for (uint32_t i = 0; i < n; ++i)
      if (jobs[i].nof_tx_layers == 1)
        solo.push_back(jobs[i]);
  const uint32_t nsolo   = jobs_on_device ? n : (uint32_t)solo.size();
  const bool     layered = max_layers >= 2; // (host jobs: some job has more than one layer)
  const void*    d_jobs  = nullptr;
  if (layered || jobs_on_device)
    if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_job) * (size_t)n, s, &d_jobs)))
      return rc;
  if (nsolo) {
    const void* d_solo = d_jobs;
    if (!jobs_on_device) {
      if ((rc = miphy_stage_descs(ctx, solo.data(), 0, sizeof(miphy_pusch_chest_job) * (size_t)nsolo, s, &d_solo)))
        return rc;
    } else {
      void* work = nullptr;
      if ((rc = miphy_get_workspace(ctx, MIPHY_WS_GENERAL, sizeof(miphy_pusch_chest_job) * (size_t)n, &work)))
        return rc;
      hipLaunchKernelGGL(chest_solo_jobs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const miphy_pusch_chest_job*)d_jobs, (miphy_pusch_chest_job*)work, n);
      MIPHY_HIP_CHECK(hipGetLastError());
      d_solo = work;
    }
    if ((rc = chest_enqueue(ctx, d_solo, nsolo, max_ports, 1, grid, nullptr, ce, scalars, s)))
      return rc;
  }
  return layered ? chest_layers_enqueue(ctx, d_jobs, n, max_ports, max_layers, grid, ce, scalars, s) : MIPHY_OK;
}

// The rules of the estimators behind cfo_corr_kernel on host jobs: those of the layered estimator on base_of(job), and an estimate per symbol.
template <class Job, class Base>
static int chest_cfo_validate(const Job* jobs, uint32_t n, Base&& base_of, const char* what, unsigned& max_ports, unsigned& max_layers)
{
  std::vector<miphy_pusch_chest_job> base(n);
  for (uint32_t i = 0; i < n; ++i)
    base[i] = base_of(jobs[i]);
  const int r = chest_validate(base.data(), n, false, max_ports, max_layers, what);
  if (r)
    return r;
  for (uint32_t i = 0; i < n; ++i)
    MIPHY_REQUIRE(base[i].ce_compact == 0, "%s: job %u: the estimate differs from symbol to symbol, ce_compact must be 0", what, i);
  return MIPHY_OK;
}

// The two launches of the estimators with a carrier frequency offset on staged jobs (records of job_bytes each, a miphy_pusch_chest_cfo_job in front):
// cfo_corr_kernel, whose partials live in a workspace of the context, then the estimate kernel (var: chest_tv_kernel, else chest_cfo_kernel) on the
// grid of chest_layers_kernel; jobs on one layer run there too (a layer alone in its group).
static int chest_cfo_enqueue(miphy_ctx* ctx, const void* jobs, int jobs_on_device, size_t job_bytes, uint32_t n, unsigned max_ports, unsigned max_layers,
                             const float* grid, float* ce, float* scalars, float* cfo, float* var, hipStream_t s)
{
  const void* d_jobs = nullptr;
  int         rc     = miphy_stage_descs(ctx, jobs, jobs_on_device, job_bytes * (size_t)n, s, &d_jobs);
  if (rc)
    return rc;
  void* parts = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_GENERAL, sizeof(float) * CFO_JOB_FLOATS * (size_t)n, &parts)))
    return rc;
  const cplx*      tw;
  const gold_jump* gold;
  if ((rc = chest_resources(ctx, &tw, &gold)))
    return rc;
  const dim3 blocks(n, max_ports * (max_layers > 2 ? 2 : 1));
  if (var) {
    hipLaunchKernelGGL(cfo_corr_kernel<miphy_pusch_chest_tv_job>, blocks, dim3(CHEST_THREADS), 0, s, (const miphy_pusch_chest_tv_job*)d_jobs, gold,
                       (const float2*)grid, (float*)parts, (int)max_ports);
    MIPHY_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(chest_tv_kernel, blocks, dim3(CHEST_THREADS), tv_lds::BYTES, s, (const miphy_pusch_chest_tv_job*)d_jobs, gold, tw, (const float2*)grid,
                       (float2*)ce, scalars, (const float*)parts, cfo, var, (int)max_ports);
  } else {
    hipLaunchKernelGGL(cfo_corr_kernel<miphy_pusch_chest_cfo_job>, blocks, dim3(CHEST_THREADS), 0, s, (const miphy_pusch_chest_cfo_job*)d_jobs, gold,
                       (const float2*)grid, (float*)parts, (int)max_ports);
    MIPHY_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(chest_cfo_kernel, blocks, dim3(CHEST_THREADS), chest_lds::BYTES + CFO_LDS_BYTES, s, (const miphy_pusch_chest_cfo_job*)d_jobs, gold, tw,
                       (const float2*)grid, (float2*)ce, scalars, (const float*)parts, cfo, (int)max_ports);
  }
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}

// The layered estimator with the carrier frequency offset estimated and compensated.
extern "C" int miphy_dmrs_pusch_estimate_cfo_batch(miphy_ctx* ctx, const miphy_pusch_chest_cfo_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                   float* ce, float* scalars, float* cfo, void* stream)
{
  const char* what = "miphy_dmrs_pusch_estimate_cfo_batch";
  unsigned    max_ports, max_layers;
  int         rc = chest_prologue(what, ctx && jobs && grid && ce && scalars && cfo, n, UINT32_MAX, jobs_on_device, max_ports, max_layers,
                                  [&](unsigned& mp, unsigned& ml) -> int {
                            return chest_cfo_validate(jobs, n, [](const miphy_pusch_chest_cfo_job& j) -> const miphy_pusch_chest_job& { return j.base; }, what, mp, ml);
                          });
  if (rc || n == 0)
    return rc;
  return chest_cfo_enqueue(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_cfo_job), n, max_ports, max_layers, grid, ce, scalars, cfo, nullptr, (hipStream_t)stream);
}

// The same for a channel that changes within the slot: the fits of the DM-RS symbols kept apart and interpolated in time (chest_tv_kernel).
extern "C" int miphy_dmrs_pusch_estimate_tv_batch(miphy_ctx* ctx, const miphy_pusch_chest_tv_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                  float* ce, float* scalars, float* cfo, float* var, void* stream)
{
  const char* what = "miphy_dmrs_pusch_estimate_tv_batch";
  unsigned    max_ports, max_layers;
  int         rc = chest_prologue(what, ctx && jobs && grid && ce && scalars && cfo && var, n, UINT32_MAX, jobs_on_device, max_ports, max_layers,
                                  [&](unsigned& mp, unsigned& ml) -> int {
                            const int r =
                                chest_cfo_validate(jobs, n, [](const miphy_pusch_chest_tv_job& j) -> const miphy_pusch_chest_job& { return j.base.base; }, what, mp, ml);
                            if (r)
                              return r;
                            for (uint32_t i = 0; i < n; ++i)
                              MIPHY_REQUIRE(tv_job_ok(jobs[i]), "%s: job %u: time_mode must be MIPHY_TIME_INTERPOLATE or MIPHY_TIME_LINE, the reserved bytes 0", what, i);
                            return (int)MIPHY_OK;
                          });
  if (rc || n == 0)
    return rc;
  return chest_cfo_enqueue(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_tv_job), n, max_ports, max_layers, grid, ce, scalars, cfo, var, (hipStream_t)stream);
}

extern "C" int miphy_dmrs_pusch_estimate_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n, const float* grid, float* ce,
                                               float* scalars, void* stream)
{
  return chest_launch(ctx, jobs, jobs_on_device, n, grid, nullptr, ce, scalars, stream, "miphy_dmrs_pusch_estimate_batch");
}

// Transform-precoded PUSCH (TS 38.211 6.4.1.1.1.2): the low-PAPR pilots of every job into a workspace of the context (transform_precoding.hip), then
// chest_kernel<true> on a copy of the base records that points at them -- the estimate and scalars of miphy_port_channel_estimate_batch fed those pilots.
extern "C" int miphy_dmrs_pusch_estimate_tp_batch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* jobs, int jobs_on_device, uint32_t n, const float* grid, float* ce,
                                                  float* scalars, void* stream)
{
  const char* what = "miphy_dmrs_pusch_estimate_tp_batch";
  unsigned    max_ports, max_layers, max_nprb = 270;
  int         rc = chest_prologue(what, ctx && jobs && grid && ce && scalars, n, 65535, jobs_on_device, max_ports, max_layers,
                                  [&](unsigned& mp, unsigned&) { return miphy_tp_chest_validate(what, jobs, n, max_nprb, mp); });
  if (rc || n == 0)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_chest_tp_job) * (size_t)n, s, &d_jobs)))
    return rc;
  // [base records | pilots: per job four DM-RS symbols of the widest allocation]
  const uint32_t stride     = 4u * 6u * max_nprb;
  const size_t   base_bytes = (sizeof(miphy_pusch_chest_job) * (size_t)n + 255) & ~(size_t)255;
  void*          work       = nullptr;
  if ((rc = miphy_get_workspace(ctx, MIPHY_WS_GENERAL, base_bytes + (size_t)n * stride * sizeof(float2), &work)))
    return rc;
  auto*  base   = static_cast<miphy_pusch_chest_job*>(work);
  float* pilots = reinterpret_cast<float*>(static_cast<uint8_t*>(work) + base_bytes);
  if ((rc = miphy_tp_pilots_launch(ctx, (const miphy_pusch_chest_tp_job*)d_jobs, n, pilots, base, stride, s)))
    return rc;
  return chest_enqueue(ctx, base, n, max_ports, 1, grid, pilots, ce, scalars, s);
}

extern "C" int miphy_port_channel_estimate_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                 const float* pilots, float* ce, float* scalars, void* stream)
{
  MIPHY_REQUIRE(pilots, "miphy_port_channel_estimate_batch: null pilots");
  return chest_launch(ctx, jobs, jobs_on_device, n, grid, pilots, ce, scalars, stream, "miphy_port_channel_estimate_batch");
}

extern "C" uint32_t miphy_pusch_noise_covariance_nof_prg(const miphy_pusch_ncov_job* job)
{
  if (!job || !ncov_job_ok(*job))
    return 0;
  return ncov_nof_prg(miphy_count_prb(job->base.rb_mask, job->base.grid_nof_prb), job->prg_size);
}

// One matrix per PRG of every job, straight from the grid: the estimator's residuals are formed again (same helpers), nothing of its output is read.
extern "C" int miphy_pusch_noise_covariance_batch(miphy_ctx* ctx, const miphy_pusch_ncov_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                  float* cov, void* stream)
{
  const char* what = "miphy_pusch_noise_covariance_batch";
  unsigned    max_ports, max_layers, max_prg = 275; // device-resident jobs: one PRB per PRG on the widest grid
  int         rc = chest_prologue(what, ctx && jobs && grid && cov, n, UINT32_MAX, jobs_on_device, max_ports, max_layers, [&](unsigned& mp, unsigned& ml) -> int {
    std::vector<miphy_pusch_chest_job> base(n);
    for (uint32_t i = 0; i < n; ++i)
      base[i] = jobs[i].base;
    const int r = chest_validate(base.data(), n, false, mp, ml);
    if (r)
      return r;
    max_prg = 1;
    for (uint32_t i = 0; i < n; ++i) {
      MIPHY_REQUIRE(ncov_job_ok(jobs[i]), "pusch_noise_covariance: job %u: the diagonal loading should be finite and not negative", i);
      const unsigned g = ncov_nof_prg(miphy_count_prb(jobs[i].base.rb_mask, jobs[i].base.grid_nof_prb), jobs[i].prg_size);
      max_prg          = g > max_prg ? g : max_prg;
    }
    return (int)MIPHY_OK;
  });
  if (rc || n == 0)
    return rc;
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if ((rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_pusch_ncov_job) * (size_t)n, s, &d_jobs)))
    return rc;
  const cplx*      tw;
  const gold_jump* gold;
  if ((rc = chest_resources(ctx, &tw, &gold)))
    return rc;
  hipLaunchKernelGGL(ncov_kernel, dim3(n, (max_prg + NCOV_PRG_PER_BLOCK - 1) / NCOV_PRG_PER_BLOCK), dim3(CHEST_THREADS), 0, s,
                     (const miphy_pusch_ncov_job*)d_jobs, gold, (const float2*)grid, (float2*)cov);
  MIPHY_HIP_CHECK(hipGetLastError());
  return MIPHY_OK;
}
