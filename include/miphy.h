/*
 * miphy.h -- C ABI of the MI355X-native 5G NR upper-PHY hot path (libmiphy.so).
 *
 * This is the drop-in boundary: plain C, POD arguments, caller-owned DEVICE pointers (HBM resident), an explicit
 * HIP stream passed as void*.  Every entry point is batched -- the per-call C++ adapters that implement the
 * reference's abstract classes (srsran_project_23.5_amd/adapters/) wrap these with a batch of one.
 *
 * Each function cites the reference interface it replaces (paths relative to the srsRAN_Project 23.5 tree).
 * Return value: 0 on success, negative MIPHY_E* on error (the reference aborts through srsran_assert on the same
 * precondition violations; C has no asserts, so the adapters turn a non-zero code into report_fatal_error).
 *
 * Data conventions equal the reference's:
 *   - LLR: int8, finite range [-120,120], +-127 = +-infinity (include/srsran/phy/upper/log_likelihood_ratio.h:46-240)
 *   - packed bits: MSB first in each byte (include/srsran/adt/bit_buffer.h:35-44)
 *   - unpacked bits: one bit per byte, filler bit = 254 (include/srsran/phy/upper/channel_coding/ldpc/ldpc.h:107)
 *   - cf_t: interleaved fp32 (re, im)
 *   - resource grid: [port][symbol][subcarrier], subcarrier fastest (lib/phy/support/resource_grid_impl.h:42-46)
 */
#ifndef MIPHY_H
#define MIPHY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPHY_VERSION 1

enum {
  MIPHY_OK        = 0,
  MIPHY_EINVAL    = -1, /* invalid argument (would be an srsran_assert in the reference) */
  MIPHY_EHIP      = -2, /* HIP runtime error, see miphy_last_error() */
  MIPHY_ENOMEM    = -3,
  MIPHY_EUNSUPP   = -4
};

/* CRC polynomials, same order as srsran::crc_generator_poly (include/srsran/phy/upper/channel_coding/crc_calculator.h:31-38). */
enum { MIPHY_CRC24A = 0, MIPHY_CRC24B = 1, MIPHY_CRC24C = 2, MIPHY_CRC16 = 3, MIPHY_CRC11 = 4, MIPHY_CRC_NONE = 255 };

typedef struct miphy_ctx miphy_ctx;

/* Creates a context on HIP device `device`: uploads the TS 38.212 graph tables, CRC tables and polar tables and
 * allocates the scratch workspace.  One context per host thread (the reference's processors are single-threaded
 * objects, one per worker: lib/phy/upper/uplink_processor_concurrent.h:41-54).
 * Execution model of every *_batch entry point: the work is ENQUEUED on `stream` and the call returns; nothing waits for the
 * stream. Descriptor arrays in host memory are copied when the call is made (pinned staging ring of the context: the array can be
 * reused at once; the device is synchronised only when the 8 MB ring wraps) -- or pass descriptors that already live on the device
 * (`*_on_device` = 1). Scratch workspaces belong to the context and are reused by its next call in stream order: use one stream
 * at a time per context. A workspace that has to grow gets a new block; the old one stays allocated until miphy_destroy.
 * HIP graph capture (bench.py replays the single-slot pipeline that way):
 *  - a prepared plan (*_plan_create / *_plan_run) owns its descriptors, scratch and side streams: it can be captured from its
 *    first run, and a replay stays valid whatever the context runs later;
 *  - a per-call entry point with device-resident descriptors can be captured once it has run at that size on the context (its
 *    first runs may grow a workspace or build a cache, e.g. OFDM plans, polar codes, Gold tables); it then stays valid after
 *    later, larger calls;
 *  - host descriptors must not be captured: a replay would read a staging slot that has been reused since. */
int         miphy_create(int device, miphy_ctx** ctx);
void        miphy_destroy(miphy_ctx* ctx);
const char* miphy_last_error(void);
int         miphy_version(void);

/* ------------------------------------------------------------------------------------------------------------------
 * LDPC decoder  --  replaces srsran::ldpc_decoder::decode
 *   include/srsran/phy/upper/channel_coding/ldpc/ldpc_decoder.h:73-74
 *   lib/phy/upper/channel_coding/ldpc/ldpc_decoder_impl.cpp:60-146 with the AVX2 arithmetic of ldpc_decoder_avx2.cpp.
 * One descriptor per codeblock.  `iters[i]` receives the value of the optional<unsigned> the reference returns:
 * the iteration count (>=1) when crc_poly != NONE and the CRC matched, 0 for nullopt.
 * The output holds bg_K*Z bits per codeblock, packed.  All-zero input: output all ones when crc_poly == NONE,
 * untouched otherwise (ldpc_decoder_impl.cpp:88-94).
 * Input LLR domain: [-127,127]; `in_len` should be a multiple of Z for bit-exact parity. */
typedef struct {
  uint8_t  bg;              /* 1 or 2 */
  uint8_t  crc_poly;        /* MIPHY_CRC*; MIPHY_CRC_NONE = no early stop (crc == nullptr) */
  uint16_t Z;               /* lifting size */
  uint16_t max_iter;        /* algorithm_conf.max_iterations (default 6) */
  uint16_t nof_filler_bits; /* cb_specific.nof_filler_bits */
  uint32_t in_len;          /* number of input LLRs (first one belongs to variable node 2) */
  uint32_t flags;           /* bit 0: check the CRC only after the last iteration (pusch_decoder_impl.cpp:105-118) */
  uint64_t llr_offset;      /* element offset of this codeblock's LLRs inside `llr` */
  uint64_t out_offset;      /* byte offset of this codeblock's packed message inside `out_bits` */
} miphy_ldpc_dec_desc;

/* Optional launch bounds for device-resident descriptors (which the host cannot inspect): the largest lifting size
 * and input length in the batch. NULL = worst case (Z = 384, full-length codeblocks: one workgroup per CU).
 * The library sizes its on-chip buffers for ceil((max_in_len + 2 max_Z) / max_Z) variable nodes. When the batch mixes lifting
 * sizes, a codeblock with a smaller Z reaches more nodes per LLR: pass max_in_len = (n_max - 2) * max_Z with
 * n_max = max over codeblocks of ceil((in_len + 2 Z) / Z). A bound that is too small corrupts the result.
 * Any mix of lifting sizes up to max_Z, odd ones included, is legal in one batch. Device-resident descriptors are decoded by ONE
 * launch sized for max_Z (a codeblock with a small Z then leaves most lanes of its workgroup idle); hand the descriptors over in host
 * memory, or use the transport-block level entry points, to have the batch sorted into per-lifting-size launch classes. */
typedef struct {
  uint32_t max_Z;
  uint32_t max_in_len;
} miphy_ldpc_dec_limits;

int miphy_ldpc_decode_batch(miphy_ctx*                 ctx,
                            const miphy_ldpc_dec_desc* descs, /* n descriptors; host memory unless descs_on_device */
                            int                        descs_on_device,
                            uint32_t                   n,
                            const int8_t*              llr,      /* device */
                            uint8_t*                   out_bits, /* device */
                            int32_t*                   iters,    /* device, n entries */
                            const miphy_ldpc_dec_limits* limits, /* may be NULL */
                            void*                      stream);
/* Prepared form of miphy_ldpc_decode_batch for batches whose geometry repeats (same descriptors slot after slot): the descriptors
 * are validated, sorted into launch classes and uploaded once, and the launch geometry and message scratch of every class are fixed;
 * a run only launches (no host synchronisation, no staging, no allocation). */
typedef struct miphy_ldpc_decode_plan miphy_ldpc_decode_plan;
int      miphy_ldpc_decode_plan_create(miphy_ctx* ctx, const miphy_ldpc_dec_desc* descs /* host */, uint32_t n, miphy_ldpc_decode_plan** out);
int      miphy_ldpc_decode_plan_run(miphy_ldpc_decode_plan* plan, const int8_t* llr, uint8_t* out_bits, int32_t* iters, void* stream);
uint32_t miphy_ldpc_decode_plan_nof_launches(const miphy_ldpc_decode_plan* plan); /* kernel launches per run = launch classes */
void     miphy_ldpc_decode_plan_destroy(miphy_ldpc_decode_plan* plan);

/* Test / A-B knob: 0 = automatic choice (host descriptors: sorted into launch classes by lifting size and code rate, one launch per
 * class; device descriptors: one launch), 1 = one-row-per-lane kernel, 2 = packed two-rows-per-lane kernel as one launch,
 * 3 = class-sorted launches, 4 = class-sorted launches with the geometry of a batch that fills the chip whatever its size (no latency form, messages in global
 * memory wherever that buys residency), 5 = class-sorted launches with the latency form of the packed kernel (two parts) on every class (A-B measurement only),
 * 6 = automatic choice with the latency form in two parts instead of four. Adding 0x100 keeps ALL messages of a GMSG launch in global memory (A-B of the
 * split between LDS and global memory). Adding 0x200 keeps every launch computing its soft-bit addresses (no launch reads them from
 * the table of miphy_ldpc_address_table; A-B of that instance). Adding 0x400 keeps every launch on the instances of the packed kernel
 * that run every layer visit (none takes the instance that leaves out the visits of layers whose rows are saturated; A-B of that skip). All kernels produce identical results. Prepared plans keep the choice in force when they were
 * created: the knob applies to plans created after it is set (and to every per-call decode). */
void miphy_debug_force_ldpc_kernel(int mode);
/* Launches since the last reset of the packed kernel's instance whose wavefronts leave out the layer visits of saturated rows (taken for
 * launches whose codeblocks run all their iterations, throughput form, messages in LDS): */
unsigned miphy_debug_ldpc_row_skip_launches(int reset);
/* Which decoder kernels have been launched since the last reset (tests assert that a forced choice really ran): */
#define MIPHY_LDPC_KERNEL_SCALAR 1u /* one check row per lane */
#define MIPHY_LDPC_KERNEL_PACKED 2u /* two check rows per lane, one codeblock per workgroup */
#define MIPHY_LDPC_KERNEL_FUSED  4u /* ... that rate-dematches while it loads */
#define MIPHY_LDPC_KERNEL_GMSG   8u /* ... with check-to-variable messages (all, or the layers behind a boundary) in global memory */
#define MIPHY_LDPC_KERNEL_WAVE  16u /* several small codeblocks per wavefront (Z <= 64) */
#define MIPHY_LDPC_KERNEL_SPLIT 32u /* packed kernel in its latency form: four (or two) times the wavefronts per codeblock (launches of at most one codeblock per CU) */
#define MIPHY_LDPC_KERNEL_GMSG_PART 64u /* ... a GMSG launch that kept the first layers' messages in LDS (only the layers behind a boundary in global memory) */
unsigned miphy_debug_ldpc_kernels_used(int reset);
/* Decoder launches since the last reset that read their soft-bit addresses from a table (the instance of the packed kernel for
 * high-rate codeblocks that are dematched while they load). */
unsigned miphy_debug_ldpc_address_table_launches(int reset);
/* Host only (no device needed): the soft-bit address table of base graph `bg` (1 / 2), lifting size Z and the first `layers` layers,
 * as the decoder reads it. Lane l < ceil(Z / 2) of a codeblock's workgroup owns check rows l and l + ceil(Z / 2) of every layer (an odd
 * Z: its last lane owns row l twice); the table has 64 ceil(Z / 128) lanes. Layer after layer, ceil(degree / 4) quads of four words each
 * per layer: word ((first quad of the layer + q) * lanes + l) * 4 + k belongs to edge 4 q + k of the layer (beyond the degree: the last
 * edge again) and holds the LDS byte address of the soft bit of row l in its low half, of row l + ceil(Z / 2) in its high half:
 * ((row + shift) mod Z) + column * Z. Lanes without rows hold zeros. Returns the number of 32-bit words (out may be NULL to ask for
 * it), or a negative error code. */
int miphy_ldpc_address_table(int bg, int Z, int layers, uint32_t* out);
/* A-B knob: streams the launch classes of one call are spread over (1 = one after another on the caller's stream). Like
 * miphy_debug_force_ldpc_kernel, it applies to plans created after it is set. */
void miphy_debug_set_ldpc_class_streams(int n);
/* Test hook: codeblocks of the PDSCH encoder launches since the last reset that the bit-packed kernel took (out[0]) and in total (out[1]). */
void miphy_debug_pdsch_cb_counts(unsigned out[2], int reset);

/* ------------------------------------------------------------------------------------------------------------------
 * LDPC rate dematcher  --  replaces srsran::ldpc_rate_dematcher::rate_dematch
 *   include/srsran/phy/upper/channel_coding/ldpc/ldpc_rate_dematcher.h:52-55
 *   lib/phy/upper/channel_coding/ldpc/ldpc_rate_dematcher_impl.cpp:43-254, AVX2 combine rule
 *   (ldpc_rate_dematcher_avx2_impl.cpp:45-58: saturating add clamped to +-120).
 * One descriptor per codeblock. The output is the HARQ soft buffer view of the FULL codeblock (N = 66Z / 50Z LLRs),
 * read-modify-written exactly like the reference does: with new_data the same positions are cleared / set to +inf
 * (fillers) / left untouched, otherwise the new LLRs are combined into the existing ones. */
typedef struct {
  uint8_t  bg;              /* 1 or 2 */
  uint8_t  rv;              /* redundancy version 0..3 */
  uint8_t  mod;             /* bits per symbol: 1, 2, 4, 6, 8 */
  uint8_t  new_data;        /* 1: first transmission (copy mode), 0: combine with the soft buffer */
  uint16_t Z;
  uint16_t nof_filler_bits;
  uint32_t Nref;            /* limited-buffer length, 0 = unlimited */
  uint32_t E;               /* rate-matched length of this codeblock (multiple of mod) */
  uint64_t in_offset;       /* element offset of the E input LLRs inside `llr_in` */
  uint64_t out_offset;      /* element offset of the N-LLR soft buffer inside `softbuf` */
} miphy_ldpc_rdm_desc;

/* Optional launch bound for device-resident descriptors: the largest E in the batch (sizes the LDS staging buffer;
 * NULL = assume up to 60 KiB, which limits residency). */
typedef struct {
  uint32_t max_E;
} miphy_ldpc_rdm_limits;

int miphy_ldpc_rate_dematch_batch(miphy_ctx*                   ctx,
                                  const miphy_ldpc_rdm_desc*   descs,
                                  int                          descs_on_device,
                                  uint32_t                     n,
                                  const int8_t*                llr_in,  /* device */
                                  int8_t*                      softbuf, /* device, in/out */
                                  const miphy_ldpc_rdm_limits* limits,  /* may be NULL */
                                  void*                        stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LDPC rate matcher  --  replaces srsran::ldpc_rate_matcher::rate_match
 *   include/srsran/phy/upper/channel_coding/ldpc/ldpc_rate_matcher.h:46
 *   lib/phy/upper/channel_coding/ldpc/ldpc_rate_matcher_impl.cpp:42-182.
 * in: full codeblock, N = 66Z / 50Z bytes, one bit per byte (fillers = 254 are skipped positionally);
 * out: E bytes, one bit per byte. Uses the same descriptor as the dematcher (new_data ignored;
 * in_offset -> codeblock inside `cb_in`, out_offset -> E output bytes inside `out`). */
int miphy_ldpc_rate_match_batch(miphy_ctx*                 ctx,
                                const miphy_ldpc_rdm_desc* descs,
                                int                        descs_on_device,
                                uint32_t                   n,
                                const uint8_t*             cb_in, /* device */
                                uint8_t*                   out,   /* device */
                                void*                      stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LDPC encoder  --  replaces srsran::ldpc_encoder::encode
 *   include/srsran/phy/upper/channel_coding/ldpc/ldpc_encoder.h:46-47
 *   lib/phy/upper/channel_coding/ldpc/ldpc_encoder_impl.cpp:44-81, ldpc_encoder_generic.cpp:30-223.
 * in: bg_K*Z bytes, one bit per byte (filler bits = 254, copied through to the output);
 * out: out_len <= N_short*Z bytes (codeblock without the first 2Z punctured bits). */
typedef struct {
  uint8_t  bg;
  uint8_t  reserved0;
  uint16_t Z;
  uint32_t out_len;
  uint64_t in_offset;  /* byte offset of the message inside `msg_in` */
  uint64_t out_offset; /* byte offset of the codeblock inside `cb_out` */
} miphy_ldpc_enc_desc;

int miphy_ldpc_encode_batch(miphy_ctx*                 ctx,
                            const miphy_ldpc_enc_desc* descs,
                            int                        descs_on_device,
                            uint32_t                   n,
                            const uint8_t*             msg_in, /* device */
                            uint8_t*                   cb_out, /* device */
                            void*                      stream);

/* ------------------------------------------------------------------------------------------------------------------
 * CRC calculator  --  replaces srsran::crc_calculator::calculate / calculate_bit / calculate_byte
 *   include/srsran/phy/upper/channel_coding/crc_calculator.h:45-67, lib/phy/upper/channel_coding/crc_calculator_lut_impl.cpp.
 * One descriptor per message; messages are MSB-first packed (bit_offset may be unaligned). */
typedef struct {
  uint64_t bit_offset; /* first bit of the message inside `data` */
  uint32_t nbits;
  uint32_t poly;       /* MIPHY_CRC* */
} miphy_crc_desc;

int miphy_crc_batch(miphy_ctx*            ctx,
                    const miphy_crc_desc* descs,
                    int                   descs_on_device,
                    uint32_t              n,
                    const uint8_t*        data,      /* device, packed */
                    uint32_t*             checksums, /* device, n entries */
                    void*                 stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DFT processor  --  replaces srsran::dft_processor (get_input/run), batched
 *   include/srsran/phy/generic_functions/dft_processor.h:34-73, lib/phy/generic_functions/dft_processor_generic_impl.cpp.
 * Unnormalised; DIRECT uses exp(-j...), INVERSE exp(+j...). `n` transforms stored back to back (size cf_t each).
 * Supported sizes: every 2^a * 3^b <= 4096 in one LDS pass, and 4608 ... 49152 of the reference's list through a four-step
 * transform (all 18 sizes of dft_processor_generic_impl.cpp:193-210); anything else -> MIPHY_EUNSUPP. */
int miphy_dft_batch(miphy_ctx* ctx, uint32_t size, int inverse, uint32_t n, const float* in /* device cf_t */,
                    float* out /* device cf_t */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * OFDM slot (de)modulator  --  replaces srsran::ofdm_slot_demodulator::demodulate / ofdm_slot_modulator::modulate
 *   include/srsran/phy/lower/modulation/ofdm_demodulator.h:33-102, lib/phy/lower/modulation/ofdm_demodulator_impl.cpp:34-170
 *   include/srsran/phy/lower/modulation/ofdm_modulator.h,          lib/phy/lower/modulation/ofdm_modulator_impl.cpp:55-138
 *   phase compensation: include/srsran/phy/lower/modulation/phase_compensation_lut.h:49-96 (TS 38.211 5.4).
 * The configuration struct has the fields of srsran::ofdm_demodulator_configuration / ofdm_modulator_configuration
 * (normal cyclic prefix). One job = one (slot, port): 14 symbols. */
typedef struct {
  uint32_t numerology;                /* mu: SCS = 15 kHz * 2^mu (0..2) */
  uint32_t bw_rb;                     /* resource grid width in PRB */
  uint32_t dft_size;
  uint32_t nof_samples_window_offset; /* demodulator only; 0 for the modulator */
  float    scale;
  float    reserved;
  double   center_freq_hz;
} miphy_ofdm_config;

typedef struct {
  uint64_t samples_offset; /* cf_t element offset of the first sample of the slot inside the time-domain buffer */
  uint64_t grid_offset;    /* cf_t element offset of this port's [14][bw_rb*12] grid inside the grid buffer */
  uint32_t slot_index;     /* slot index within the subframe */
  uint32_t grid_empty;     /* modulator: non-zero reproduces the empty-grid shortcut (output zeros) */
} miphy_ofdm_job;

int miphy_ofdm_demodulate_slots(miphy_ctx* ctx, const miphy_ofdm_config* cfg, const miphy_ofdm_job* jobs, int jobs_on_device,
                                uint32_t n, const float* samples /* device cf_t */, float* grid /* device cf_t */, void* stream);
int miphy_ofdm_modulate_slots(miphy_ctx* ctx, const miphy_ofdm_config* cfg, const miphy_ofdm_job* jobs, int jobs_on_device,
                              uint32_t n, const float* grid /* device cf_t */, float* samples /* device cf_t */, void* stream);

/* The same transforms one OFDM symbol at a time, for the symbol-granular interfaces of the lower PHY
 * (srsran::ofdm_symbol_demodulator / ofdm_symbol_modulator, ofdm_demodulator.h:55-74, ofdm_modulator.h:55-74; callers
 * lib/phy/lower/processors/uplink/puxch/puxch_processor_impl.cpp:64-76, downlink/pdxch/pdxch_processor_impl.cpp:76-82).
 * A job is one symbol: slot_index = symbol index within the SUBFRAME (0 .. 14 * 2^numerology - 1), samples_offset = cf_t offset of
 * the symbol's first sample (cyclic prefix included), grid_offset = cf_t offset of its row of bw_rb * 12 subcarriers. */
uint32_t miphy_ofdm_symbol_size(const miphy_ofdm_config* cfg, uint32_t symbol_index); /* cyclic prefix + dft_size samples; host only */
int miphy_ofdm_demodulate_symbols(miphy_ctx* ctx, const miphy_ofdm_config* cfg, const miphy_ofdm_job* jobs, int jobs_on_device, uint32_t n,
                                  const float* samples /* device cf_t */, float* grid /* device cf_t */, void* stream);
int miphy_ofdm_modulate_symbols(miphy_ctx* ctx, const miphy_ofdm_config* cfg, const miphy_ofdm_job* jobs, int jobs_on_device, uint32_t n,
                                const float* grid /* device cf_t */, float* samples /* device cf_t */, void* stream);
/* Number of samples of slot `slot_index` (ofdm_slot_demodulator::get_slot_size). Returns 0 on invalid configuration. */
uint32_t miphy_ofdm_slot_size(const miphy_ofdm_config* cfg, uint32_t slot_index);

/* ------------------------------------------------------------------------------------------------------------------
 * DM-RS based PUSCH channel estimator  --  replaces srsran::dmrs_pusch_estimator::estimate (which drives
 * srsran::port_channel_estimator::compute for every receive port)
 *   include/srsran/phy/upper/signal_processors/dmrs_pusch_estimator.h:39-85
 *   lib/phy/upper/signal_processors/dmrs_pusch_estimator_impl.cpp:71-212      (Gold-sequence pilots, layer weights)
 *   include/srsran/phy/upper/signal_processors/port_channel_estimator.h:45-107
 *   lib/phy/upper/signal_processors/port_channel_estimator_average_impl.cpp:97-347 (LS, averaging, RSRP/EPRE/noise/SNR,
 *   time alignment through a 4096-point IDFT, linear interpolation, broadcast to all symbols).
 * One job = one PUSCH allocation in one slot; the kernel runs one workgroup per (job, rx port, layer).
 * DM-RS type 1 only (the reference's estimator asserts out of bounds for type 2); no intra-slot frequency hopping
 * (dmrs_pusch_estimator_impl.cpp never configures it). */
typedef struct {
  uint32_t numerology;     /* slot.numerology() */
  uint32_t slot_in_frame;  /* slot.slot_index(): slot number within the radio frame */
  uint32_t scrambling_id;
  float    scaling;        /* beta_DMRS amplitude scaling */
  uint8_t  n_scid;
  uint8_t  nof_tx_layers;  /* 1..4 */
  uint8_t  nof_rx_ports;   /* 1..4, port p is grid port rx_ports[p] */
  uint8_t  first_symbol;
  uint8_t  nof_symbols;
  uint8_t  rx_ports[4];
  uint8_t  ce_compact;     /* 0: the estimate is copied to every symbol of the allocation like the reference does
                              (port_channel_estimator_average_impl.cpp:216-224); 1: one row per (layer, rx port) -- the copies are
                              identical, so a consumer that knows it (miphy_pusch_demodulate_batch with ce_compact) needs no more */
  uint8_t  reserved[2];
  uint16_t symbols_mask;   /* bit l = OFDM symbol l carries DM-RS */
  uint16_t grid_nof_prb;   /* width of the resource grid / rb_mask.size() */
  uint64_t rb_mask[5];     /* bit i = PRB i belongs to the allocation */
  uint64_t grid_offset;    /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
  uint64_t ce_offset;      /* cf_t offset of the estimate: [layer][rx port][first_symbol+nof_symbols][grid_nof_prb*12];
                              only the allocated PRBs of symbols [first_symbol, first_symbol+nof_symbols) are written.
                              With ce_compact: [layer][rx port][grid_nof_prb*12] */
  uint64_t scalars_offset; /* float offset: per (rx port, layer) {rsrp, epre, noise_var, snr, time_alignment_s} */
  /* port_channel_estimator::configuration beyond what dmrs_pusch_estimator_impl fills in (port_channel_estimator.h:45-107,
   * port_channel_estimator_average_impl.cpp:97-224): intra-slot frequency hopping and externally generated pilots. */
  uint64_t rb_mask2[5];    /* layer_dmrs_pattern::rb_mask2: allocation of the second hop (used when hop_symbol != 0) */
  uint64_t pilots_offset;  /* cf_t offset into `pilots` of miphy_port_channel_estimate_batch: dmrs_symbol_list
                              [layer][DM-RS symbol][pilot of the allocated PRBs]; ignored by miphy_dmrs_pusch_estimate_batch */
  uint8_t  hop_symbol;     /* layer_dmrs_pattern::hopping_symbol_index: first OFDM symbol of the second hop, 0 = no hopping;
                              honoured by miphy_port_channel_estimate_batch only (the reference's PUSCH estimator never hops) */
  uint8_t  re_odd_mask;    /* with external pilots: bit ly = layer ly has its DM-RS on the odd subcarriers (layer_dmrs_pattern::re_pattern of
                              DM-RS type 1); the PUSCH estimator derives it from the layer number instead */
  uint8_t  reserved2[6];
} miphy_pusch_chest_job;

/* The port estimator on its own: the same kernel with the pilots given by the caller (device, cf_t) instead of generated from
 * (slot, scrambling_id, n_scid) -- srsran::port_channel_estimator::compute (port_channel_estimator.h:102-106). slot_in_frame,
 * scrambling_id and n_scid of the jobs are ignored; hop_symbol / rb_mask2 select intra-slot frequency hopping (per-hop least squares,
 * interpolation and mapping, time alignment averaged over the hops, noise variance = epre / 1000 as the reference forces it with
 * hopping: port_channel_estimator_average_impl.cpp:118-138). */
/* jobs_on_device: 0 = host array (validated), 1 = device array; with a device array bits 8-11 / 12-15 may carry the largest nof_rx_ports /
 * nof_tx_layers of the batch (0 = unknown: workgroups for 4 x 4 are launched and the surplus ones exit at once). */
#define MIPHY_JOBS_ON_HOST 0
#define MIPHY_JOBS_ON_DEVICE 1
#define MIPHY_JOBS_ON_DEVICE_HINT(max_ports, max_layers) (1 | ((int)(max_ports) << 8) | ((int)(max_layers) << 12))
int miphy_port_channel_estimate_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n, const float* grid /* device cf_t */,
                                      const float* pilots /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */, void* stream);
int miphy_dmrs_pusch_estimate_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n,
                                    const float* grid /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */,
                                    void* stream);

/* DM-RS estimator for PUSCH on 1..4 transmit layers  --  beyond the 23.5 reference, whose estimator runs each layer through the one-layer
 * least-squares fit and never undoes the frequency-domain OCC: layers 2g and 2g+1 share CDM group g and its resource elements, so its
 * estimates of a shared group come out as h_2g +- h_2g+1. Same jobs, arguments and output layouts as miphy_dmrs_pusch_estimate_batch;
 * DM-RS type 1, single-symbol DM-RS, layer ly = DM-RS port ly, no hopping, no external pilots. Per (job, rx port, CDM group g), over the
 * np = 6 nprb pilots i of the allocated PRBs (ascending, concatenated; subcarriers 12 r + 2 q + g), r_d[i] = layer 0's pilot:
 *   z[i]   = (sum_d x_d[i] conj(r_d[i])) / (nds beta)
 *   only layer 2g present (one layer; layer 2 of three): as miphy_dmrs_pusch_estimate_batch; a job on one layer gives its bytes.
 *   both present: s_a[m] = (z[2m] + z[2m+1]) / 2, s_b[m] = (z[2m] - z[2m+1]) / 2, m = 0 .. np/2 - 1 (three pairs per PRB, none across PRBs);
 *     estimate: the reference's linear interpolator over the 12 nprb concatenated subcarriers with anchors s_l[m] at 4m + 1 + g (edges held)
 *     epre = sum |x|^2 / (np nds); rsrp_l = beta^2 sum_m |s_l[m]|^2 / (np/2)
 *     noise_var = (sum |x_d[i] - beta r_d[i] (A + (-1)^i B)|^2 / np * 6) / (6 nds - 2), A, B = per-PRB means of s_a, s_b, the same for both
 *     layers; with nds < 3 noise_var = 0.001 epre as on one layer; snr_l = (rsrp_l / beta^2) / noise_var (1000 when noise_var is 0)
 *     time alignment per layer: the 4096-point IDFT and peak rule of the one-layer estimator with s_l[m] on both pilot subcarriers of pair m
 * A host job with hop_symbol != 0 (or breaking a rule of miphy_dmrs_pusch_estimate_batch) is MIPHY_EINVAL with nothing enqueued; a
 * device-resident one is skipped. Out: double-symbol DM-RS (TD-OCC), DM-RS type 2, hopping. */
int miphy_dmrs_pusch_estimate_layers_batch(miphy_ctx* ctx, const miphy_pusch_chest_job* jobs, int jobs_on_device, uint32_t n,
                                           const float* grid /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */,
                                           void* stream);

/* The layered estimator with carrier frequency offset (CFO) estimation and compensation  --  beyond the 23.5 reference, whose estimator
 * averages the DM-RS symbols and copies one estimate to every OFDM symbol. A residual offset of the UE's oscillator (or a line-of-sight Doppler
 * shift) f rotates OFDM symbol l by the common phase 2 pi f tau_l; the average then fits no symbol but one and shrinks. Here the offset is
 * estimated from the DM-RS symbols of the job, the fit of the layered estimator is run on derotated DM-RS, and the estimate is written per symbol,
 * rotated back. The model is a common phase per OFDM symbol: inter-carrier interference inside a symbol is ignored.
 *   symbol times: tau_l = start of the useful part of OFDM symbol l in the slot, normal cyclic prefix: symbol j lasts 2048 + 144 samples at
 *     2048 * 2^mu * 15 kHz, and 16 * 2^mu samples more where (14 slot_in_frame + j) mod (7 * 2^mu) = 0 (the rule of miphy_ofdm_symbol_size). Only
 *     differences of tau enter. Extended CP cannot be expressed by the job.
 *   per-symbol fits, per (rx port p, CDM group g, DM-RS symbol d): z_d[i] = x_d[i] conj(r_d[i]) / beta over the pilots of the allocated PRBs;
 *     both layers of the group present: s_{a,d}[m] = (z_d[2m] + z_d[2m+1]) / 2, s_{b,d}[m] = (z_d[2m] - z_d[2m+1]) / 2; a layer alone: s_d = z_d
 *   correlation, per pair of consecutive DM-RS symbols (d, d+1) of the allocation, all ports and layers in one sum (a UE has one oscillator):
 *     C_d = sum_p sum_layers sum_m s_{l,d+1}[m] conj(s_{l,d}[m]),   E_d = sum_p sum_layers sqrt(sum_m |s_{l,d+1}|^2 sum_m |s_{l,d}|^2)
 *     added in the fixed order (port, layer, gap) ascending, without atomics: a job gives the same bits whatever else is in the batch
 *   offset, dt_d = tau_{d+1} - tau_d:  cfo_hz = sum_d |C_d| arg(C_d) / (2 pi dt_d) / sum_d |C_d|,   rho = sum_d |C_d| / sum_d E_d  (0 <= rho <= 1:
 *     how much of the DM-RS energy the common rotation explains); one DM-RS symbol, or sum |C_d| = 0: cfo_hz = 0, rho = 0.
 *     Unambiguous for |f| < 1 / (2 max dt_d): +-1.56 kHz for DM-RS on symbols 2 and 11 at 30 kHz, +-7 kHz for neighbouring DM-RS symbols at 15 kHz.
 *   estimate: phi_l = 2 pi cfo_hz (tau_l - tau_ref), tau_ref = the first DM-RS symbol of the allocation. The arithmetic of
 *     miphy_dmrs_pusch_estimate_layers_batch (least squares, despreading, interpolation, EPRE, RSRP, noise residual, SNR, time alignment; a job on
 *     one layer follows the rule of a layer alone in its group; noise_var = 0.001 epre below three DM-RS symbols) on x_d exp(-j phi_d) gives H[k]
 *     and the scalars; H_l[k] = H[k] exp(+j phi_l) is written to every symbol l of the allocation. The scalars are those of the derotated fit: the
 *     noise variance does not contain the energy of the rotation.
 * base.ce_compact must be 0 (the estimate differs from symbol to symbol); base.nof_tx_layers 1..4; otherwise the rules, hints
 * (MIPHY_JOBS_ON_DEVICE_HINT) and output layouts of miphy_dmrs_pusch_estimate_layers_batch. A host job that breaks a rule (ce_compact != 0 and
 * hopping included) is MIPHY_EINVAL with nothing enqueued; a device-resident one is skipped. Two launches on the stream: the correlation partials
 * of every (job, port, layer, gap) go to a workspace of the context, the estimate kernel adds them up.
 * Out: offsets beyond the unambiguous range, extended CP, MMSE-IRC and transform-precoded variants, prepared plans. A channel whose magnitude
 * changes between the DM-RS symbols is followed by miphy_dmrs_pusch_estimate_tv_batch below. */
typedef struct {
  miphy_pusch_chest_job base;   /* ce_compact must be 0; nof_tx_layers 1..4; the rules of the layered estimator otherwise */
  uint64_t cfo_offset;          /* float offset: {cfo_hz, rho} of the job */
} miphy_pusch_chest_cfo_job;
int miphy_dmrs_pusch_estimate_cfo_batch(miphy_ctx* ctx, const miphy_pusch_chest_cfo_job* jobs, int jobs_on_device, uint32_t n,
                                        const float* grid /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */,
                                        float* cfo /* device */, void* stream);

/* The estimator above for a channel that changes within the slot (Doppler spread: magnitude and phase move differently per path and per receive
 * port, which one common phase per symbol does not follow)  --  beyond the 23.5 reference. The DM-RS symbols are not averaged: the per-symbol fits
 * are kept apart, derotated by the common offset, and interpolated in time. Notation (tau_l, dsym[d], nds, beta, s_{l,d}[m], phi_l) as above;
 * cfo_hz and rho are exactly those of miphy_dmrs_pusch_estimate_cfo_batch (the same correlation launch and partials).
 *   per-symbol fits, per (rx port p, CDM group g, DM-RS symbol d): S_d[m] = s_{.,d}[m] exp(-j phi_{dsym[d]}), despread where both layers of the group
 *     are present, z_d on all six pilots of a PRB for a layer alone
 *   time weights w[l][d], for every OFDM symbol l of the allocation and DM-RS symbol d, from differences of tau only; rows sum to 1; nds = 1: w = 1
 *     MIPHY_TIME_INTERPOLATE: j = the largest index with dsym[j] <= l, clamped to 0 .. nds - 2; u = (tau_l - tau_dsym[j]) / (tau_dsym[j+1] - tau_dsym[j]);
 *       w[l][j] = 1 - u, w[l][j+1] = u, every other weight 0. u outside [0, 1] extrapolates from the nearest two DM-RS symbols.
 *     MIPHY_TIME_LINE: w[l][d] = 1 / nds + (tau_l - tm)(tau_dsym[d] - tm) / sum_d' (tau_dsym[d'] - tm)^2, tm the mean of the DM-RS symbol times: one
 *       least-squares line over all DM-RS symbols. With two DM-RS symbols the two modes coincide.
 *   estimate: A_l[m] = sum_d w[l][d] S_d[m] are the anchors of symbol l; H_l[k] = the layered estimator's frequency interpolation of A_l (the same
 *     anchor positions, edges held) times exp(+j phi_l), written to every symbol l of the allocation, allocated PRBs only. The fits are derotated
 *     before they are blended: a linear blend of two rotated phasors shrinks.
 *   scalars: epre, rsrp and time alignment from the time mean sum_d S_d / nds (what the least squares of the estimator above computes). The noise is
 *     measured against the fit in time, not against the mean: F_d = sum_d' w[dsym[d]][d'] S_d'; A_d, B_d = the per-PRB means of F_{a,d}, F_{b,d} (a layer
 *     alone: the per-PRB mean of its six, B_d = 0); e_d[i] = x'_d[i] - beta r_d[i] (A_d + (-1)^i B_d) with x'_d the derotated element;
 *     noise_var = sum |e|^2 / nprb / (6 nds - nlay R), nlay the layers of the group, R = nds for INTERPOLATE and min(nds, 2) for LINE (the parameters
 *     fitted per layer and PRB), from two DM-RS symbols on; one DM-RS symbol: noise_var = 0.001 epre. snr by the rule of the other estimators.
 *   variation, per (rx port, layer): var = sum_m sum_d |S_d[m] - mean_d S[m]|^2 / sum_m sum_d |S_d[m]|^2, the share of the derotated DM-RS energy that
 *     the time average does not explain: near 0 for a UE that stands still, towards 1 for a fast one. 0 with one DM-RS symbol or no energy.
 * Every sum runs in a fixed order without atomics: a job gives the same bits alone and inside any batch. Rules, hints, refusals and output layouts
 * of miphy_dmrs_pusch_estimate_cfo_batch, and time_mode one of the two values with the reserved bytes 0: a host job that breaks a rule is
 * MIPHY_EINVAL with nothing enqueued, a device-resident one is skipped. Two launches on the stream, as above.
 * Out: more than a line or a polygon in time (no Wiener filter, no smoothing across slots), extended CP, MMSE-IRC and transform-precoded variants,
 * prepared plans. */
#define MIPHY_TIME_INTERPOLATE 1 /* piecewise linear between DM-RS symbols */
#define MIPHY_TIME_LINE 2        /* one least-squares line over all DM-RS symbols */
typedef struct {
  miphy_pusch_chest_cfo_job base; /* every rule of the CFO estimator holds */
  uint64_t var_offset;            /* float offset: per (rx port, layer) one float at port * nof_tx_layers + layer */
  uint8_t  time_mode;             /* MIPHY_TIME_INTERPOLATE or MIPHY_TIME_LINE */
  uint8_t  reserved[7];           /* 0 */
} miphy_pusch_chest_tv_job;       /* 176 bytes */
int miphy_dmrs_pusch_estimate_tv_batch(miphy_ctx* ctx, const miphy_pusch_chest_tv_job* jobs, int jobs_on_device, uint32_t n,
                                       const float* grid /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */,
                                       float* cfo /* device */, float* var /* device */, void* stream);

/* Noise-plus-interference covariance across the receive ports, from the DM-RS residuals of the estimator above  --  beyond the 23.5 reference,
 * which has no MMSE equaliser to feed ("MMSE equalizer is not implemented yet"). Reads the grid only. With e[g][p][d][i] the residual whose
 * energy the estimator turns into noise_var (g the CDM group, p the receive port, d the DM-RS symbol, i the pilot of the allocated PRBs):
 *   both layers of the group present:  e = x_d[i] - beta r_d[i] (A + (-1)^i B),  A, B the per-PRB means of s_a, s_b
 *   a layer alone in its group:        e = x_d[i] - beta r_d[i] (per-PRB mean of z)
 * the allocated PRBs, in ascending order, are cut into PRGs of prg_size PRBs (the last one may be short; prg_size 0: one PRG), and for PRG j of
 * n_j PRBs, with f_g = 2 where group g carries two layers, else 1:
 *   C_j[p][q] = (sum_g sum_d sum_{i in PRG j} e[g][p][d][i] conj(e[g][q][d][i])) / (n_j sum_g (6 nds - f_g))
 *   C_j[p][p] += loading (sum_p C_j[p][p]) / P
 * Without loading the whole-allocation diagonal is the estimator's noise_var of the port (one layer, two layers), from three DM-RS symbols on;
 * the 0.001 epre substitution below three does not apply here: the divisor is positive from one DM-RS symbol on. The sums run in one fixed
 * order without atomics: a PRG's matrix has the same bits whatever else is in the batch. Every matrix is written in full, Hermitian, with
 * diagonal imaginary parts 0. Rules: those of miphy_dmrs_pusch_estimate_layers_batch on `base` (hopping included), and loading finite and
 * >= 0: a host job that breaks one is MIPHY_EINVAL with nothing enqueued, a device-resident one is skipped; the hints of
 * MIPHY_JOBS_ON_DEVICE_HINT are accepted. Out: more than 4 receive ports, DM-RS type 2, double-symbol DM-RS, frequency hopping, a covariance
 * per OFDM symbol. */
typedef struct {
  miphy_pusch_chest_job base; /* ce_offset, scalars_offset and ce_compact are ignored */
  uint64_t cov_offset;        /* cf_t offset: [PRG][P][P], row p, column q: C[p][q] ~ E[n_p conj(n_q)], P = base.nof_rx_ports */
  float    loading;           /* >= 0, finite */
  uint16_t prg_size;          /* PRBs per matrix, counted over the ALLOCATED PRBs in ascending order; 0 = one matrix for the allocation */
  uint8_t  reserved[2];
} miphy_pusch_ncov_job;
uint32_t miphy_pusch_noise_covariance_nof_prg(const miphy_pusch_ncov_job* job); /* host; matrices the job writes, 0 on an invalid job */
int      miphy_pusch_noise_covariance_batch(miphy_ctx* ctx, const miphy_pusch_ncov_job* jobs, int jobs_on_device, uint32_t n,
                                            const float* grid /* device cf_t */, float* cov /* device cf_t */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH demodulator  --  replaces srsran::pusch_demodulator::demodulate (the block between the channel estimator
 * and the decoder), i.e. channel_equalizer::equalize + demodulation_mapper::demodulate_soft + descrambling in one pass
 *   include/srsran/phy/upper/channel_processors/pusch_demodulator.h:40-108
 *   lib/phy/upper/channel_processors/pusch_demodulator_impl.cpp:31-152, pusch_demodulator_impl.h:74-172
 *   lib/phy/upper/equalization/channel_equalizer_zf_impl.cpp:123-162, equalize_zf_1xn.h:42-158
 *   lib/phy/upper/channel_modulation/demodulation_mapper_impl.cpp:34-106 and demodulation_mapper_q*.cpp
 * One transmit layer (the reference asserts the same, pusch_demodulator_impl.cpp:83), 1..4 receive ports, pi/2-BPSK .. 256QAM,
 * DM-RS type 1 or 2, no UCI placeholders, no EVM report. One job = one PUSCH transmission; the LLRs are the codeword in the order
 * the decoder expects (symbol-major, subcarrier ascending). The channel estimate and the noise variance are read where
 * miphy_dmrs_pusch_estimate_batch wrote them (layer 0 block; noise variance of rx port 0: scalars[scalars_offset + 2]). */
typedef struct {
  uint32_t rnti;
  uint32_t n_id;           /* scrambling identity, c_init = rnti * 2^15 + n_id */
  uint8_t  mod;            /* bits per symbol: 1 (pi/2-BPSK), 2, 4, 6, 8 */
  uint8_t  nof_rx_ports;   /* 1..4, port p is grid port rx_ports[p] */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;
  uint8_t  dmrs_type;      /* 1 or 2 */
  uint8_t  nof_cdm_groups_without_data;
  uint8_t  ce_nof_symbols; /* symbols per (port) block of the channel estimate = first_symbol + nof_symbols of the estimator job */
  uint8_t  ce_compact;     /* 1: the channel estimate has one row per rx port ([rx port][grid_nof_prb*12], an estimator job with
                              ce_compact) used for every symbol; ce_nof_symbols is then ignored */
  uint8_t  rx_ports[4];
  uint16_t dmrs_symbols_mask; /* bit l = OFDM symbol l carries DM-RS */
  uint16_t grid_nof_prb;
  uint32_t nof_llr;        /* codeword length; must equal miphy_pusch_demod_nof_llr() */
  uint64_t rb_mask[5];
  uint64_t grid_offset;    /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
  uint64_t ce_offset;      /* cf_t offset of the channel estimate: [rx port][ce_nof_symbols][grid_nof_prb*12] */
  uint64_t scalars_offset; /* float offset of the estimator scalars of this transmission */
  uint64_t llr_offset;     /* int8 offset of the output codeword */
  /* UCI multiplexed on the PUSCH (pusch_demodulator::configuration::placeholders, pusch_demodulator_impl.cpp:99-152): indices, in
   * codeword order, of the resource elements that carry a repetition placeholder (ulsch_placeholder_list; from
   * miphy_ulsch_placeholders). In such an element bit 0 is descrambled normally, bit 1 with the chip of bit 0, the others not at all. */
  uint32_t placeholders_offset; /* uint16 offset into the `placeholders` array of miphy_pusch_demodulate_batch_ex */
  uint32_t nof_placeholders;    /* 0: none */
  uint64_t evm_offset;          /* float offset into `evm_sums` of 14 per-symbol sums of |hard-decided symbol - equalised symbol|^2
                                   (pusch_demodulator_impl.cpp:89-90, evm_calculator_generic_impl.cpp:31-47): EVM = sqrt(sum / data REs) */
} miphy_pusch_demod_job;

/* Number of LLRs the allocation of `job` produces (data REs x mod); 0 on an invalid job. Host function. */
uint32_t miphy_pusch_demod_nof_llr(const miphy_pusch_demod_job* job);
/* _ex: with the placeholder lists (device, may be NULL when no job has any) and the EVM sums (device, may be NULL: no EVM). */
int miphy_pusch_demodulate_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                    const float* ce, const float* scalars, int8_t* llr, const uint16_t* placeholders, float* evm_sums, void* stream);
int miphy_pusch_demodulate_batch(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n,
                                 const float* grid /* device cf_t */, const float* ce /* device cf_t */, const float* scalars /* device */,
                                 int8_t* llr_out /* device */, void* stream);

/* PUSCH demodulator for one codeword on 1..4 transmit layers  --  beyond the 23.5 reference, whose demodulator asserts one layer
 * (pusch_demodulator_impl.h, "layer demapping is not implemented"): zero forcing of L layers on P >= L receive ports (the arithmetic of
 * miphy_channel_equalize_layers_batch, tx_scaling = 1) and the layer demapping of TS 38.211 6.3.1.3 in front of the same soft demapper.
 *   estimate: as miphy_dmrs_pusch_estimate_batch writes it, [layer][rx port][ce_nof_symbols][nsc], with ce_compact [layer][rx port][nsc];
 *             noise variance at scalars[scalars_offset + 2]
 *   output:   data element i (ranked symbol-major, subcarrier ascending, as on one layer), layer ly, bit b at
 *             llr_offset + (L i + ly) mod + b, descrambled with c((L i + ly) mod + b), c_init = rnti * 2^15 + n_id; pi/2-BPSK rotates
 *             with the parity of L i + ly
 * base.nof_llr must equal miphy_pusch_demod_layers_nof_llr(). A batch may mix layer counts; a job on one layer writes the bytes of
 * miphy_pusch_demodulate_batch. A host job that breaks a rule is MIPHY_EINVAL with nothing enqueued, a device-resident one is skipped.
 * miphy_pusch_demodulate_layers_batch takes no UCI placeholders and reports no EVM (base.nof_placeholders = 0, evm_offset ignored); _ex does:
 *   placeholders: as on one layer, the list of a job (base.placeholders_offset, base.nof_placeholders) holds resource element indices in
 *             codeword order, ascending, as miphy_ulsch_placeholders(nof_layers = L) returns them. Listed element i carries the pattern
 *             [c0 y x ..] in each of its L codeword symbols L i + ly: there bit 0 is descrambled with its own chip c((L i + ly) mod), bit 1
 *             with that same chip, the others not at all (TS 38.211 6.3.1.1, TS 38.212 6.3.2). nof_placeholders != 0 needs the list and
 *             mod >= 2.
 *   EVM:      evm_sums[base.evm_offset + sy], sy = 0..13, receives the sum over the data elements of OFDM symbol sy and their L layers of
 *             |hard-decided symbol - equalised symbol|^2, the hard decision taken on the soft bits before descrambling, the pi/2-BPSK
 *             rotation by the parity of L i + ly; 0 for a symbol without data. EVM = sqrt(sum over symbols / (data REs x L)). The order of
 *             the additions is fixed, so two runs give the same bits, whatever the size of the batch.
 * The LLRs of a job do not depend on whether EVM is asked for; without placeholders they are those of the plain entry point. A job on one layer
 * gives the LLRs and the sums of miphy_pusch_demodulate_batch_ex. */
typedef struct {
  miphy_pusch_demod_job base;
  uint8_t               nof_tx_layers; /* 1..4, <= base.nof_rx_ports */
  uint8_t               reserved[7];
} miphy_pusch_demod_layers_job;
/* Number of LLRs of `job` (data REs x layers x mod); 0 on an invalid job. Host function. */
uint32_t miphy_pusch_demod_layers_nof_llr(const miphy_pusch_demod_layers_job* job);
int miphy_pusch_demodulate_layers_batch(miphy_ctx* ctx, const miphy_pusch_demod_layers_job* jobs, int jobs_on_device, uint32_t n,
                                        const float* grid /* device cf_t */, const float* ce /* device cf_t */, const float* scalars /* device */,
                                        int8_t* llr_out /* device */, void* stream);
int miphy_pusch_demodulate_layers_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_layers_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                           const float* ce, const float* scalars, int8_t* llr_out, const uint16_t* placeholders /* device, may be NULL */,
                                           float* evm_sums /* device, may be NULL */, void* stream);

/* The same demodulator with MMSE-IRC in place of zero forcing (beyond the reference, like the layers themselves): the equaliser is
 * miphy_channel_equalize_mmse_batch at tx_scaling 1 (declared further down; csrc/mmse_device.h), fed one covariance matrix per PRG as
 * miphy_pusch_noise_covariance_batch writes them. The bytes are those of extraction, that equaliser, the soft demapper and the descrambler
 * one after the other; placeholders and EVM of _ex follow the rules above unchanged. 1..4 layers, ONE LAYER INCLUDED: interference rejection on
 * one layer with two or four ports is the common case (such a job does not give the bytes of miphy_pusch_demodulate_batch: another equaliser).
 * The scalar noise variance is not read: `scalars` may be NULL and base.base.scalars_offset is ignored. With a compact estimate the matrices
 * A and B of a subcarrier are set up once for all its symbols. The LLR count is miphy_pusch_demod_layers_nof_llr(&job.base). Rules and
 * refusals: those of the layered entry points. Out: MMSE for the transform-precoded path, a covariance per OFDM symbol. */
typedef struct {
  miphy_pusch_demod_layers_job base;
  uint64_t cov_offset;   /* cf_t offset into cov: [PRG][P][P], P = base.base.nof_rx_ports */
  uint16_t prg_size;     /* as in miphy_pusch_ncov_job: PRG of a subcarrier = rank of its PRB among the allocated ones / prg_size; 0 = matrix 0 */
  uint8_t  reserved[6];
} miphy_pusch_demod_mmse_job;
int miphy_pusch_demodulate_layers_mmse_batch(miphy_ctx* ctx, const miphy_pusch_demod_mmse_job* jobs, int jobs_on_device, uint32_t n,
                                             const float* grid /* device cf_t */, const float* ce /* device cf_t */,
                                             const float* scalars /* device, not read, may be NULL */, const float* cov /* device cf_t */,
                                             int8_t* llr_out /* device */, void* stream);
int miphy_pusch_demodulate_layers_mmse_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_mmse_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                                const float* ce, const float* scalars /* may be NULL */, const float* cov, int8_t* llr_out,
                                                const uint16_t* placeholders /* device, may be NULL */, float* evm_sums /* device, may be NULL */,
                                                void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH with transform precoding (DFT-s-OFDM, TS 38.211 6.3.1.4)  --  beyond the 23.5 reference, which has no transform precoding anywhere
 * in its uplink chain. The waveform is single-layer by specification. Restated in numpy from the standard in tests/pusch_tp_ref.py.
 *
 * The de-precoder on its own: row s of a job holds the M = 12 N_PRB equalised elements x[k] of one data OFDM symbol and their noise
 * variances v[k]; it gives
 *   y[n] = (1 / sqrt(M)) sum_k x[k] e^(+j 2 pi k n / M), n = 0 .. M-1, and one noise variance per row,
 *   v = (sum over the normal elements of v[k]) / (number of normal elements); +inf when no element is normal.
 * An element is normal when v[k] is positive and finite. Any other element (the equalisers mark an element they could not invert with
 * symbol 0 and variance +inf) enters the IDFT as 0, whatever its symbol holds, and is left out of the mean. The additions of the mean run
 * in one fixed order (csrc/tp_device.h), so a row has one value whatever the batch. N_PRB = 2^a 3^b 5^c <= 270: the 53 sizes M = 12 ... 3240.
 * A host job with another M is MIPHY_EUNSUPP, one with nof_symbols > 14 MIPHY_EINVAL, with nothing enqueued; a device-resident one is skipped. */
typedef struct {
  uint32_t M;                     /* elements per row */
  uint32_t nof_symbols;           /* rows, at most 14 */
  uint64_t eq_symbols_offset;     /* cf_t offset into eq_symbols: [row][M] */
  uint64_t eq_noise_vars_offset;  /* float offset into eq_noise_vars: [row][M] */
  uint64_t out_symbols_offset;    /* cf_t offset into out_symbols: [row][M] */
  uint64_t out_noise_var_offset;  /* float offset into out_noise_var: [row] */
} miphy_transform_deprecode_job;
int miphy_transform_deprecode_batch(miphy_ctx* ctx, const miphy_transform_deprecode_job* jobs, int jobs_on_device, uint32_t n,
                                    const float* eq_symbols /* device cf_t */, const float* eq_noise_vars /* device */,
                                    float* out_symbols /* device cf_t */, float* out_noise_var /* device */, void* stream);

/* The demodulator of a transform-precoded PUSCH: miphy_pusch_demod_job unchanged, and beyond the rules of miphy_pusch_demodulate_batch
 *   rb_mask is contiguous and holds N_PRB = 2^a 3^b 5^c <= 270 PRBs; dmrs_type = 1; nof_cdm_groups_without_data = 2 (a DM-RS symbol carries
 *   no data, so every data symbol has exactly M = 12 N_PRB elements).
 * A host job that breaks a rule is MIPHY_EINVAL with nothing enqueued; a device-resident one is skipped. One workgroup per (transmission,
 * data OFDM symbol): the M elements of the 1..4 ports are equalised as miphy_channel_equalize_batch does (one layer, tx_scaling = 1, noise
 * variance scalars[scalars_offset + 2], compact or per-symbol estimate), de-precoded as miphy_transform_deprecode_batch does, and y[n] with
 * the symbol's v goes through the soft demapper and descrambler of miphy_pusch_demodulate_batch:
 *   bit b of y[n] of the r-th data symbol at llr_offset + (r M + n) mod + b, descrambled with c((r M + n) mod + b); pi/2-BPSK rotates by the
 *   parity of r M + n. A symbol without a normal element gives zero LLRs.
 * The bytes are those of the composition extraction, miphy_channel_equalize_batch, miphy_transform_deprecode_batch, soft demapper, descrambler.
 * _ex: placeholders as miphy_pusch_demodulate_batch_ex (element indices r M + n in codeword order, mod >= 2); evm_sums[evm_offset + sy] is
 * the sum over the M de-precoded symbols of OFDM symbol sy of |hard-decided symbol - y[n]|^2, added in a fixed order, 0 for a symbol
 * without data. The LLRs do not depend on whether EVM is asked for. miphy_pusch_demod_nof_llr gives nof_llr. */
int miphy_pusch_demodulate_tp_batch(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n,
                                    const float* grid /* device cf_t */, const float* ce /* device cf_t */, const float* scalars /* device */,
                                    int8_t* llr_out /* device */, void* stream);
int miphy_pusch_demodulate_tp_batch_ex(miphy_ctx* ctx, const miphy_pusch_demod_job* jobs, int jobs_on_device, uint32_t n, const float* grid,
                                       const float* ce, const float* scalars, int8_t* llr_out, const uint16_t* placeholders /* device, may be NULL */,
                                       float* evm_sums /* device, may be NULL */, void* stream);

/* Low-PAPR sequence r_{u,v}(n) with alpha = 0 (TS 38.211 5.2.2), n = 0 .. length-1, u = 0..29, v = 0..1. Host function, `out` on the host.
 *   length 12: Table 5.2.2.2-2 (the table PUCCH formats 0 and 1 use); v is not looked at
 *   length 30: exp(-j pi (u+1)(n+1)(n+2) / 31); v is not looked at
 *   length 6 N >= 36: x_q(n mod N_ZC), x_q(m) = exp(-j pi q m (m+1) / N_ZC), N_ZC the largest prime below the length,
 *     q = floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = N_ZC (u+1) / 31 (the standard uses v = 1 from length 72 on only; the formula is evaluated as given). The phase q m (m+1) is reduced
 *     modulo 2 N_ZC in integers before it is turned into an angle.
 * Lengths 6, 18 and 24 (allocations of 1, 3 and 4 PRBs) are defined by Tables 5.2.2.2-1, -3 and -4, which this library does not hold:
 * MIPHY_EUNSUPP here and in the two entry points below. Such an allocation is estimated by miphy_port_channel_estimate_batch with pilots
 * of the caller and demodulated by miphy_pusch_demodulate_tp_batch. Any other length or index is MIPHY_EINVAL. */
int miphy_low_papr_sequence(uint32_t u, uint32_t v, uint32_t length, float* out /* host cf_t */);

/* DM-RS of a transform-precoded PUSCH (TS 38.211 6.4.1.1.1.2): one layer on DM-RS port 0 (even subcarriers), type 1, no intra-slot hopping.
 * Of `base`: scrambling_id = n_ID^RS (0..1007), n_scid = 0, nof_tx_layers = 1, hop_symbol = 0, re_odd_mask = 0, rb_mask contiguous with a PRB
 * count 2^a 3^b 5^c <= 270 other than 1, 3 and 4 (MIPHY_EUNSUPP, above). DM-RS symbol l of slot n_s = base.slot_in_frame carries
 * r_{u,v}(n), n < 6 N_PRB, with u = (f_gh + n_ID^RS) mod 30 and
 *   hopping 0: f_gh = 0, v = 0
 *   hopping 1 (group):    f_gh = (sum_{m<8} 2^m c(8 (14 n_s + l) + m)) mod 30 with c_init = floor(n_ID^RS / 30), v = 0
 *   hopping 2 (sequence): f_gh = 0, v = c(14 n_s + l) with c_init = n_ID^RS where 6 N_PRB >= 72, else 0.
 * miphy_dmrs_pusch_tp_pilots_batch writes the pilots of every job at pilots[base.pilots_offset ...] in the layout miphy_port_channel_estimate_batch
 * reads: [DM-RS symbol][6 N_PRB]. miphy_dmrs_pusch_estimate_tp_batch is that kernel, the pilots in a workspace of the context, followed by the
 * kernel of miphy_port_channel_estimate_batch: its estimate and scalars are those of that entry point fed the pilots (base.pilots_offset is
 * ignored). A host job that breaks a rule is MIPHY_EINVAL (MIPHY_EUNSUPP for 1, 3 and 4 PRBs) with nothing enqueued; a device-resident one is
 * skipped (jobs_on_device as miphy_port_channel_estimate_batch, the port hint included). */
typedef struct {
  miphy_pusch_chest_job base;
  uint8_t               hopping; /* 0 neither, 1 group hopping, 2 sequence hopping */
  uint8_t               reserved[7];
} miphy_pusch_chest_tp_job;
int miphy_dmrs_pusch_tp_pilots_batch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* jobs, int jobs_on_device, uint32_t n, float* pilots /* device cf_t */,
                                     void* stream);
int miphy_dmrs_pusch_estimate_tp_batch(miphy_ctx* ctx, const miphy_pusch_chest_tp_job* jobs, int jobs_on_device, uint32_t n,
                                       const float* grid /* device cf_t */, float* ce /* device cf_t */, float* scalars /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Channel equalizer on its own--  replaces srsran::channel_equalizer::equalize of the zero-forcing equalizer
 * (include/srsran/phy/upper/equalization/channel_equalizer.h:27-114, lib/phy/upper/equalization/channel_equalizer_zf_impl.cpp:123-162).
 * Topologies are the reference's: one transmit layer with 1..4 receive ports (equalize_zf_1xn.h:120-158) and two layers on two ports
 * (equalize_zf_2x2.cpp:30-117); anything else is MIPHY_EINVAL where the reference asserts. The noise variance is the one of the
 * first receive port, as the reference takes it (channel_equalizer_zf_impl.cpp:141-142). Abnormal elements (zero / non-finite
 * denominator, non-positive or non-finite noise variance) give symbol 0 and noise variance +inf.
 * Note: in 23.5 the PUSCH demodulator never calls the equalizer with two layers (pusch_demodulator_impl.h asserts one layer, "layer
 * demapping is not implemented"), so the 2 x 2 case only exists behind this entry point; miphy_pusch_demodulate_batch fuses the
 * 1 x N case. Tensors are the reference's re_measurement layouts, resource element fastest. */
typedef struct {
  uint32_t nof_re;
  uint8_t  nof_rx_ports;        /* 1..4 */
  uint8_t  nof_tx_layers;       /* 1, or 2 with nof_rx_ports == 2 */
  uint8_t  reserved[2];
  float    noise_var;           /* noise_var_estimates[0] */
  float    tx_scaling;          /* > 0 */
  uint64_t ch_symbols_offset;   /* cf_t offset: [rx port][nof_re] */
  uint64_t ch_estimates_offset; /* cf_t offset: [tx layer][rx port][nof_re] */
  uint64_t eq_symbols_offset;   /* cf_t offset: [tx layer][nof_re] */
  uint64_t eq_noise_vars_offset; /* float offset: [tx layer][nof_re] */
} miphy_equalizer_job;
int miphy_channel_equalize_batch(miphy_ctx* ctx, const miphy_equalizer_job* jobs, int jobs_on_device, uint32_t n, const float* ch_symbols /* device cf_t */,
                                 const float* ch_estimates /* device cf_t */, float* eq_symbols /* device cf_t */, float* eq_noise_vars /* device */,
                                 void* stream);
/* The same jobs and tensor layouts for 1..4 transmit layers on nof_rx_ports = layers..4 receive ports (beyond the reference, which stops
 * at 1 x N and 2 x 2): x = (H^H H)^-1 H^H y / tx_scaling, noise variance noise_var [(H^H H)^-1]_ll / tx_scaling^2, in single precision
 * in a fixed order of operations (csrc/equalize_device.h: one layer and two layers as the reference, so 1 x N and 2 x 2 give the bytes of
 * miphy_channel_equalize_batch; three and four layers by an LDL^H factorisation without square roots). If a determinant or pivot is not
 * a normal number, or noise_var is not normal and positive, every layer of the element gets symbol 0 and noise variance +inf. Any other
 * topology, or tx_scaling <= 0, is MIPHY_EINVAL for host jobs and skipped for device-resident ones. */
int miphy_channel_equalize_layers_batch(miphy_ctx* ctx, const miphy_equalizer_job* jobs, int jobs_on_device, uint32_t n,
                                        const float* ch_symbols /* device cf_t */, const float* ch_estimates /* device cf_t */,
                                        float* eq_symbols /* device cf_t */, float* eq_noise_vars /* device */, void* stream);
/* MMSE with interference rejection (MMSE-IRC) on the same topologies and tensor layouts  --  beyond the reference, whose equaliser tests say
 * "MMSE equalizer is not implemented yet". Model y = t H x + n with E[n n^H] = C (t = tx_scaling), one P x P matrix per run of re_per_cov
 * elements, as miphy_pusch_noise_covariance_batch writes them; only C's lower triangle and the real parts of its diagonal are read:
 *   W = C^-1;  A = t^2 H^H W H + I;  B = A^-1;  x~ = t B H^H W y
 *   gamma_l = 1 - B_ll;  x_l = x~_l / gamma_l (unbiased);  nvar_l = B_ll / gamma_l
 * in single precision in a fixed order of operations (csrc/mmse_device.h: LDL^H factorisations of C and of A without square roots, gamma
 * taken as (B t^2 H^H W H)_ll, which does not cancel at low SINR). With C = noise_var I the symbols tend to those of the zero-forcing entry
 * point as noise_var -> 0; on one layer they are its maximum-ratio combination at every noise_var. If a pivot of either factorisation or a
 * gamma_l is not a normal positive number, every layer of the element gets symbol 0 and noise variance +inf. base.noise_var is ignored.
 * Invalid topologies and tx_scaling <= 0: as miphy_channel_equalize_layers_batch. */
typedef struct {
  miphy_equalizer_job base; /* nof_tx_layers 1..4 on nof_rx_ports = layers..4 */
  uint64_t cov_offset;      /* cf_t offset into cov: [matrix][P][P], P = base.nof_rx_ports */
  uint32_t re_per_cov;      /* element i uses matrix i / re_per_cov; 0 = matrix 0 for every element */
  uint32_t reserved;
} miphy_equalizer_mmse_job;
int miphy_channel_equalize_mmse_batch(miphy_ctx* ctx, const miphy_equalizer_mmse_job* jobs, int jobs_on_device, uint32_t n,
                                      const float* ch_symbols /* device cf_t */, const float* ch_estimates /* device cf_t */,
                                      const float* cov /* device cf_t */, float* eq_symbols /* device cf_t */, float* eq_noise_vars /* device */,
                                      void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH modulator and PDSCH DM-RS  --  replace srsran::pdsch_modulator::modulate and srsran::dmrs_pdsch_processor::map
 * (after the encoder, before the OFDM modulator)
 *   include/srsran/phy/upper/channel_processors/pdsch_modulator.h:40-99, lib/.../pdsch_modulator_impl.cpp:30-282
 *   lib/phy/upper/channel_modulation/modulation_mapper_impl.cpp:31-146
 *   include/srsran/phy/upper/signal_processors/dmrs_pdsch_processor.h:36-66, lib/.../dmrs_pdsch_processor_impl.cpp:30-169
 * Modulator: one codeword on one layer, PRBs mapped in ascending order (what 23.5 supports: its layer mapper and its
 * non-contiguous mapping path are broken, see csrc/pdsch_mod.hip; 1..4 layers and PRB lists in another mapping order are further
 * down: miphy_pdsch_modulate_layers_batch, miphy_pdsch_modulate_mapped_batch); DM-RS pattern of the bandwidth part and up to four reserved RE
 * patterns are skipped. The codeword is one bit per byte (the layout miphy_pdsch_encode_batch writes). Only the mapped REs of
 * the grid are written. */
typedef struct {
  uint64_t prb_mask[5]; /* PRBs (grid numbering) the pattern applies to */
  uint16_t re_mask;     /* bit k = subcarrier k of each of these PRBs */
  uint16_t symbols;     /* bit l = OFDM symbol l */
  uint32_t pad;
} miphy_re_pattern;

typedef struct {
  uint32_t rnti;
  uint32_t n_id;
  float    scaling;        /* applied when std::isnormal(scaling), like the reference */
  uint8_t  mod;            /* bits per symbol: 1 (pi/2-BPSK), 2, 4, 6, 8 */
  uint8_t  port;           /* grid port of the (single) layer */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;
  uint8_t  dmrs_type;      /* 1 or 2 */
  uint8_t  nof_cdm_groups_without_data;
  uint8_t  nof_reserved;   /* 0..4 */
  uint8_t  reserved0;
  uint16_t dmrs_symbols_mask;
  uint16_t grid_nof_prb;
  uint16_t bwp_start_rb;   /* the DM-RS pattern covers [bwp_start_rb, bwp_start_rb + bwp_size_rb) */
  uint16_t bwp_size_rb;
  uint32_t nof_bits;       /* codeword length; must equal miphy_pdsch_mod_nof_re() * mod */
  uint64_t rb_mask[5];     /* allocated PRBs, grid numbering (rb_allocation::get_prb_mask) */
  miphy_re_pattern reserved[4];
  uint64_t cw_offset;      /* byte offset of the codeword (one bit per byte) */
  uint64_t grid_offset;    /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
} miphy_pdsch_mod_job;

uint32_t miphy_pdsch_mod_nof_re(const miphy_pdsch_mod_job* job); /* host: data REs of the allocation; 0 on an invalid job */
int miphy_pdsch_modulate_batch(miphy_ctx* ctx, const miphy_pdsch_mod_job* jobs, int jobs_on_device, uint32_t n,
                               const uint8_t* codewords /* device */, float* grid /* device cf_t */, void* stream);

typedef struct {
  uint32_t slot_in_frame;         /* slot.slot_index() */
  uint32_t reference_point_k_rb;
  uint32_t scrambling_id;
  float    amplitude;             /* linear amplitude of the DM-RS (the sequence is +-amplitude/sqrt(2)) */
  uint8_t  dmrs_type;             /* 1 or 2 */
  uint8_t  n_scid;
  uint8_t  nof_ports;             /* DM-RS ports 1000 .. 1000 + nof_ports - 1 */
  uint8_t  reserved0;
  uint8_t  ports[12];             /* grid port of each DM-RS port */
  uint16_t symbols_mask;
  uint16_t grid_nof_prb;
  uint32_t pad;
  uint64_t rb_mask[5];
  uint64_t grid_offset;           /* cf_t offset of grid port 0 */
} miphy_dmrs_pdsch_job;

int miphy_dmrs_pdsch_map_batch(miphy_ctx* ctx, const miphy_dmrs_pdsch_job* jobs, int jobs_on_device, uint32_t n, float* grid /* device cf_t */,
                               void* stream);

/* PDSCH modulator, one codeword on 1..4 layers (beyond the 23.5 reference; the contract is the oracle's orc_pdsch_modulate). Layer
 * mapping of TS 38.211 7.3.1.3, x^(ly)(i) = d(L i + ly): the resource element of rank i carries codeword symbol L i + ly on grid port
 * ports[ly], as it is. Everything else as miphy_pdsch_modulate_batch: same scrambling, constellations, scaling and RE selection, only
 * the mapped REs of the named ports are written. The pi/2-BPSK rotation follows the parity of the codeword symbol L i + ly. A batch of
 * one-layer jobs writes the bytes miphy_pdsch_modulate_batch writes. Host jobs are checked before anything is enqueued (1..4 layers,
 * distinct ports below 16, nof_bits = REs x L x mod and the rules of the one-layer entry point); a device-resident job that breaks a
 * rule is skipped by the kernels. PRBs are mapped in ascending order here; any other order, the interleaved VRB-to-PRB mapping of TS 38.211
 * 7.3.1.6 among them, goes through miphy_pdsch_modulate_mapped_batch below, precoding matrices through miphy_pdsch_modulate_precoded_batch.
 * Two codewords (5..8 layers): miphy_pdsch_modulate_codewords_batch below. */
typedef struct {
  miphy_pdsch_mod_job base; /* base.port is ignored; base.nof_bits = miphy_pdsch_mod_layers_nof_re() x nof_layers x mod */
  uint8_t nof_layers;       /* 1..4 */
  uint8_t ports[4];         /* grid port of each layer, distinct, < 16 */
  uint8_t pad[3];
} miphy_pdsch_mod_layers_job;

uint32_t miphy_pdsch_mod_layers_nof_re(const miphy_pdsch_mod_layers_job* job); /* host: data REs per layer; 0 on an invalid job */
int miphy_pdsch_modulate_layers_batch(miphy_ctx* ctx, const miphy_pdsch_mod_layers_job* jobs, int jobs_on_device, uint32_t n,
                                      const uint8_t* codewords /* device */, float* grid /* device cf_t */, void* stream);

/* VRB-to-PRB mapping of TS 38.211 7.3.1.6 (host function): the PRBs of the set VRBs of vrb_mask, in ascending VRB order -- the mapping
 * order miphy_pdsch_modulate_mapped_batch and miphy_pdsch_process_mapped_batch take. (The contract is the standard, not the 23.5
 * reference: its vrb_to_prb_mapper takes the size of the first bundle from the BWP size where 7.3.1.6 takes it from the BWP start, and
 * starts the last bundle one PRB too low.)
 * With L = bundle_size, N = region_size_rb and s = align_rb mod L there are N_bundle = ceil((N + s) / L) bundles; VRB n lies in bundle
 * j = floor((n + s) / L) at position (n + s) mod L. Bundle N_bundle - 1 maps to itself; any other j = 2 c + r (r < 2) maps to
 * f(j) = r C + c with C = floor(N_bundle / 2). PRB(n) = first_prb + f(j) L + (n + s) mod L - s; with L = 0, PRB(n) = first_prb + n.
 * The three cases of 7.3.1.6:
 *   DCI 1_0 in the Type0-PDCCH common search space of CORESET 0: L = 2, align_rb = 0, N = N_BWP,init^size,
 *                                                               first_prb = BWP start + N_CORESET^start;
 *   DCI 1_0 in any other common search space:                   the same with align_rb = N_BWP,i^start + N_CORESET^start;
 *   every other case:                                           L = L_i, align_rb = N_BWP,i^start, N = N_BWP,i^size, first_prb = BWP start.
 * prb_list[0 .. *nof_prb - 1] receives the PRBs (grid numbering), prb_mask (may be NULL) their set. MIPHY_EINVAL, no list or mask
 * written, for: L outside {0, 2, 4}; N outside 1..275; first_prb + N > 275; a set bit of vrb_mask at or above N; cap < the number of set
 * VRBs -- *nof_prb is that number then too, so that the caller can size the list. */
typedef struct {
  uint8_t  bundle_size;    /* L: 0 = non-interleaved, 2 or 4 */
  uint8_t  pad;
  uint16_t align_rb;       /* the bundle raster is aligned to this RB number: only align_rb mod L matters */
  uint16_t region_size_rb; /* N: VRBs 0 .. N-1 exist */
  uint16_t first_prb;      /* grid PRB that PRB 0 of the region is */
} miphy_vrb_to_prb;
int miphy_vrb_to_prb_list(const miphy_vrb_to_prb* map, const uint64_t vrb_mask[5], uint16_t* prb_list, uint32_t cap, uint32_t* nof_prb,
                          uint64_t prb_mask[5] /* may be NULL */);

/* PDSCH modulator with the PRBs of a job in a mapping order of the caller's: miphy_pdsch_modulate_layers_batch, except that within each OFDM
 * symbol the data REs are taken PRB by PRB in the order of the job's list (subcarriers ascending inside a PRB) -- position i of the list is
 * the i-th PRB in mapping order, what orc_pdsch_modulate calls prb_list. Which REs carry data, the layer mapping, scrambling, constellations,
 * scaling and ports do not depend on the order, and miphy_pdsch_mod_layers_nof_re(&job.layers) stays the size function. The list of job j is
 * prb_lists[prb_list_offset .. prb_list_offset + nof_prb - 1]; prb_lists lives where the jobs live (host lists are staged with host jobs).
 * nof_prb = 0: no list, the PRBs of rb_mask ascending -- the bytes miphy_pdsch_modulate_layers_batch writes. A list must satisfy:
 * prb_list_offset + nof_prb <= nof_list_entries; every entry is below grid_nof_prb, has its bit set in rb_mask and appears once; nof_prb
 * is the number of set bits of rb_mask. A host job that breaks a rule is refused with MIPHY_EINVAL and the rule's message, nothing enqueued;
 * a device-resident job that breaks one is skipped by the kernels before any entry is used as an address. */
typedef struct {
  miphy_pdsch_mod_layers_job layers; /* layers.base.rb_mask = the PRBs of the list, as before */
  uint32_t prb_list_offset;          /* uint16 index into prb_lists */
  uint16_t nof_prb;                  /* 0: no list -- ascending order of rb_mask */
  uint16_t pad;
} miphy_pdsch_mod_mapped_job;
int miphy_pdsch_modulate_mapped_batch(miphy_ctx* ctx, const miphy_pdsch_mod_mapped_job* jobs, int jobs_on_device, uint32_t n,
                                      const uint16_t* prb_lists /* where the jobs are; may be NULL when nof_list_entries is 0 */,
                                      uint32_t nof_list_entries, const uint8_t* codewords /* device */, float* grid /* device cf_t */, void* stream);

/* PDSCH modulator on one or two codewords, 1..8 layers (TS 38.211 Table 7.3.1.3-1; the contract is orc_pdsch_modulate with two codeword
 * arguments). With L = nof_layers = 5..8, codeword 0 has L0 = floor(L / 2) layers and codeword 1 has L1 = L - L0: layer ly < L0 carries
 * d0(L0 i + ly) and layer L0 + m carries d1(L1 i + m) on the resource element of rank i, layer ly on grid port ports[ly]. Codeword q is
 * scrambled with c_init = rnti 2^15 + q 2^14 + n_id; the pi/2-BPSK rotation follows the parity of the symbol index within its own codeword;
 * one scaling applies to both. RE selection, the list and its order, and "only the mapped REs of the named ports are written" are as in
 * miphy_pdsch_modulate_mapped_batch, and one job costs one symbol setup and one launch pair for both codewords. With L = 1..4 the job is
 * one codeword: mod1, nof_bits1 and cw1_offset are ignored and the call writes the bytes miphy_pdsch_modulate_mapped_batch writes.
 * Rules: those of the fields and the list of the mapped entry point; L in 1..8; ports[0 .. L - 1] distinct and below 16; with L >= 5 mod1
 * valid; nof_bits = REs x L0 x mod (L0 = L up to four layers) and nof_bits1 = REs x L1 x mod1. A host job that breaks one is refused with
 * MIPHY_EINVAL and "pdsch_modulate_codewords: job <i>: ...", nothing enqueued; a device-resident job that breaks any rule of either
 * codeword is skipped whole. Still out: precoding of two codewords (miphy_precoding stays one codeword on 1..4 layers). */
typedef struct {
  miphy_pdsch_mod_mapped_job mapped; /* codeword 0 (base.mod, base.nof_bits, base.cw_offset) and everything the two codewords share;
                                        mapped.layers.nof_layers and mapped.layers.ports are ignored */
  uint8_t  nof_layers;               /* 1..8; 1..4: one codeword, 5..8: two */
  uint8_t  mod1;                     /* codeword 1: bits per symbol */
  uint8_t  ports[8];                 /* grid port of each layer, distinct, < 16 */
  uint8_t  pad[2];
  uint32_t nof_bits1;                /* codeword 1: miphy_pdsch_mod_codewords_nof_re() x L1 x mod1 */
  uint64_t cw1_offset;               /* codeword 1: byte offset (one bit per byte) */
} miphy_pdsch_mod_codewords_job;
typedef char miphy_pdsch_mod_codewords_job_is_320_bytes[sizeof(miphy_pdsch_mod_codewords_job) == 320 ? 1 : -1];

uint32_t miphy_pdsch_mod_codewords_nof_re(const miphy_pdsch_mod_codewords_job* job); /* host: data REs per layer; 0 on an invalid job */
int miphy_pdsch_modulate_codewords_batch(miphy_ctx* ctx, const miphy_pdsch_mod_codewords_job* jobs, int jobs_on_device, uint32_t n,
                                         const uint16_t* prb_lists /* where the jobs are; may be NULL when nof_list_entries is 0 */,
                                         uint32_t nof_list_entries, const uint8_t* codewords /* device */, float* grid /* device cf_t */,
                                         void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Precoding  --  layers to antenna ports through one weight matrix per PRG
 *   include/srsran/ran/precoding/precoding_configuration.h (the layout: weights per layer, port and PRG, PRG 0 starts at CRB 0),
 *   include/srsran/phy/upper/precoding/channel_precoder.h, lib/phy/upper/precoding/channel_precoder_generic.cpp:27-48 (the arithmetic:
 *   the product of the first layer, then the other layers accumulated).
 * The 23.5 reference has the precoder block and the configuration and does not join them (its resource_grid_mapper asserts one layer and
 * one port), so the fused entry points below go beyond its processors; their contract is y_a = sum_ly W[prg][a][ly] x_ly in the order of
 * channel_precoder_generic, every product and sum in single precision (fused multiply-adds: each real or imaginary part is a dot product
 * of 2 L real terms, within 2 L 2^-24 of the sum of the absolute values of its terms from the exact value). Every entry point computes
 * the sum with the same sequence of operations, so the same inputs give the same bits through each of them.
 * PRG g covers the grid PRBs [g prg_size, (g + 1) prg_size); W[g][a][ly] is weights[weights_offset + (g nof_ports + a) nof_layers + ly]
 * (cf_t), the memory order of precoding_configuration (layer fastest, then port, then PRG). Antenna port a is grid port ports[a].
 * The rules of a precoding: nof_layers 1..4 and equal to the job's; nof_ports nof_layers..16; ports distinct and below 16;
 * prg_size >= 1, nof_prg >= 1; nof_prg x prg_size above the highest PRB of rb_mask; weights_offset + nof_prg x nof_ports x nof_layers <=
 * nof_weights. A host job that breaks one is refused with MIPHY_EINVAL and the rule's message, nothing enqueued; a device-resident job that
 * breaks one is skipped before any weight is read. The weights themselves are not judged. */
typedef struct {
  uint8_t  nof_layers;     /* 1..4 */
  uint8_t  nof_ports;      /* nof_layers..16 */
  uint8_t  ports[16];      /* grid port of each antenna port, distinct, < 16 */
  uint16_t prg_size;       /* PRBs per PRG, >= 1 (wideband: nof_prg = 1 and prg_size = the grid) */
  uint16_t nof_prg;        /* >= 1 */
  uint16_t pad0;
  uint32_t weights_offset; /* cf_t index of W[0][0][0] in the call's weights */
  uint32_t pad1;
} miphy_precoding;
typedef char miphy_precoding_is_32_bytes[sizeof(miphy_precoding) == 32 ? 1 : -1];

/* channel_precoder::apply_precoding for a batch: out[a][i] = sum_ly W[a][ly] in[ly][i], i < nof_re, with one matrix per job. Jobs and
 * weights live in the same place, host or device. A job of nof_re = 0 writes nothing and is held to the rules all the same. Rules: the
 * layer and port ranges above; weights_offset + nof_ports x nof_layers <= nof_weights; in_stride >= nof_re where nof_layers > 1 and
 * out_stride >= nof_re where nof_ports > 1. */
typedef struct {
  uint32_t nof_re;
  uint8_t  nof_layers;     /* 1..4 */
  uint8_t  nof_ports;      /* nof_layers..16 */
  uint16_t pad0;
  uint32_t weights_offset; /* cf_t index of W[0][0]: [port][layer] */
  uint32_t pad1;
  uint64_t in_offset;      /* cf_t offset of layer 0 in `in`: [layer][in_stride] */
  uint64_t in_stride;
  uint64_t out_offset;     /* cf_t offset of antenna port 0 in `out`: [port][out_stride] */
  uint64_t out_stride;
} miphy_precode_job;
int miphy_channel_precode_batch(miphy_ctx* ctx, const miphy_precode_job* jobs, int jobs_on_device, uint32_t n,
                                const float* weights /* cf_t, where the jobs are */, uint32_t nof_weights, const float* in /* device cf_t */,
                                float* out /* device cf_t */, void* stream);

/* PDSCH modulator with precoding: miphy_pdsch_modulate_mapped_batch (with or without a list), except that the data RE of rank i, in grid
 * PRB r, receives y_a = sum_ly W[r / prg_size][a][ly] x^(ly)(i) on grid port precoding.ports[a] for every antenna port a. mapped.layers.ports
 * is ignored. Every data RE of every one of the nof_ports ports is stored (a zero matrix row stores zeros), nothing else is touched. The
 * PRG of an RE follows the place of its PRB in the grid, never its place in the list. miphy_pdsch_mod_layers_nof_re(&job.mapped.layers)
 * stays the size function. Jobs, lists and weights live in the same place. Two codewords (5..8 layers) go through
 * miphy_pdsch_modulate_codewords_batch, without precoding; still out: precoding of two codewords. */
typedef struct {
  miphy_pdsch_mod_mapped_job mapped;
  miphy_precoding            precoding; /* precoding.nof_layers = mapped.layers.nof_layers */
} miphy_pdsch_mod_precoded_job;
int miphy_pdsch_modulate_precoded_batch(miphy_ctx* ctx, const miphy_pdsch_mod_precoded_job* jobs, int jobs_on_device, uint32_t n,
                                        const uint16_t* prb_lists /* where the jobs are; may be NULL when nof_list_entries is 0 */,
                                        uint32_t nof_list_entries, const float* weights /* cf_t, where the jobs are */, uint32_t nof_weights,
                                        const uint8_t* codewords /* device */, float* grid /* device cf_t */, void* stream);

/* PDSCH DM-RS with precoding. base.nof_ports = precoding.nof_layers (1..4) DM-RS ports 1000.. of type 1 or 2; base.ports is ignored. On an
 * RE of a CDM group that holds at least one of these DM-RS ports, antenna port a receives sum W[prg][a][ly] r_ly over the layers ly of that
 * group, r_ly being what miphy_dmrs_pdsch_map_batch writes for DM-RS port ly; REs of a CDM group without a layer are not written. Host
 * jobs are held to the rules of miphy_dmrs_pdsch_map_batch too; a device-resident job is held to those that keep its addresses in bounds. */
typedef struct {
  miphy_dmrs_pdsch_job base;
  miphy_precoding      precoding;
} miphy_dmrs_pdsch_precoded_job;
int miphy_dmrs_pdsch_map_precoded_batch(miphy_ctx* ctx, const miphy_dmrs_pdsch_precoded_job* jobs, int jobs_on_device, uint32_t n,
                                        const float* weights /* cf_t, where the jobs are */, uint32_t nof_weights, float* grid /* device cf_t */,
                                        void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Polar code chains  --  replace the chain of srsran::polar_code::set + polar_allocator::allocate + polar_encoder::encode
 * + polar_rate_matcher::rate_match (transmit) and polar_rate_dematcher::rate_dematch + polar_decoder::decode +
 * polar_deallocator::deallocate (receive), as wired in tests/unittests/phy/upper/channel_coding/polar/polar_chain_test.cpp:156-210
 *   include/srsran/phy/upper/channel_coding/polar/polar_{code,allocator,encoder,rate_matcher,rate_dematcher,decoder,deallocator}.h
 *   lib/phy/upper/channel_coding/polar/polar_code_impl.cpp:325-490 and the *_impl.cpp files next to it.
 * The decoder is the reference's simplified successive cancellation (list size 1) with rate-0 / rate-1 node pruning.
 * All codewords of one call share the code (K, E, nMax, ibil), like one polar_code object does.
 * msg: n x K bytes (one bit per byte); rm: n x E bytes / LLRs. Optional taps (may be NULL) expose the intermediate
 * results with the layouts of the single reference blocks: `allocated` / `encoded` / `decoded_u`: n x N bytes,
 * `dematched`: n x N LLRs. */
typedef struct {
  uint32_t K;    /* message length incl. CRC */
  uint32_t E;    /* rate-matched length */
  uint32_t nMax; /* 9 (downlink) or 10 (uplink) */
  uint32_t ibil; /* channel interleaver present (uplink) */
} miphy_polar_code;

/* Single blocks of the chains, for the block-level interfaces (one wavefront per codeword, n codewords back to back):
 *   ALLOCATE      polar_allocator::allocate        (polar_allocator.h:42-43)        in: n x K bits      out: n x N bits
 *   ENCODE        polar_encoder::encode            (polar_encoder.h:43)             in: n x 2^param     out: n x 2^param   (code may be NULL)
 *   RATE_MATCH    polar_rate_matcher::rate_match   (polar_rate_matcher.h:42-43)     in: n x N bits      out: n x E bits
 *   RATE_DEMATCH  polar_rate_dematcher::rate_dematch (polar_rate_dematcher.h:45-47) in: n x E LLRs      out: n x N LLRs
 *   DECODE        polar_decoder::decode            (polar_decoder.h:47-48)          in: n x N LLRs      out: n x N bits (u domain)
 *   DEALLOCATE    polar_deallocator::deallocate    (polar_deallocator.h:41-42)      in: n x N bits      out: n x K bits
 *   INTERLEAVE_TX / _RX  polar_interleaver::interleave (polar_interleaver.h:45-46)  in / out: n x param bits, param = K <= 164 (code may be NULL)
 * One bit per byte, LLRs int8, everything in device memory. */
enum {
  MIPHY_POLAR_OP_ALLOCATE = 0,
  MIPHY_POLAR_OP_ENCODE,
  MIPHY_POLAR_OP_RATE_MATCH,
  MIPHY_POLAR_OP_RATE_DEMATCH,
  MIPHY_POLAR_OP_DECODE,
  MIPHY_POLAR_OP_DEALLOCATE,
  MIPHY_POLAR_OP_INTERLEAVE_TX,
  MIPHY_POLAR_OP_INTERLEAVE_RX
};
/* Host-side query of the derived code parameters (polar_code::get_n / get_N / get_nPC). Returns 0 or MIPHY_EINVAL. */
int miphy_polar_code_info(const miphy_polar_code* code, uint32_t* n, uint32_t* N, uint32_t* nPC);

int miphy_polar_encode_batch(miphy_ctx* ctx, const miphy_polar_code* code, uint32_t n, const uint8_t* msg /* device */,
                             uint8_t* rm_out /* device */, uint8_t* allocated_tap, uint8_t* encoded_tap, void* stream);
int miphy_polar_block_batch(miphy_ctx* ctx, const miphy_polar_code* code, uint32_t op, uint32_t param, uint32_t n, const void* in /* device */,
                            void* out /* device */, void* stream);
int miphy_polar_decode_batch(miphy_ctx* ctx, const miphy_polar_code* code, uint32_t n, const int8_t* llr /* device */,
                             uint8_t* msg_out /* device */, int8_t* dematched_tap, uint8_t* decoded_u_tap, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PDCCH encoder  --  replaces srsran::pdcch_encoder::encode
 *   include/srsran/phy/upper/channel_processors/pdcch_encoder.h:36-53, lib/phy/upper/channel_processors/pdcch_encoder_impl.cpp:33-98
 * (CRC24C over 24 leading ones + payload, RNTI scrambling of the last 16 CRC bits, CRC interleaver, polar chain with
 * nMax = 9). payload: n x A bytes (one bit per byte); rnti: n entries; out: n x E bytes. */
int miphy_pdcch_encode_batch(miphy_ctx* ctx, uint32_t A, uint32_t E, uint32_t n, const uint8_t* payload /* device */,
                             const uint16_t* rnti /* device */, uint8_t* out /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH decoder (whole transport blocks)  --  replaces srsran::pusch_decoder::decode
 *   include/srsran/phy/upper/channel_processors/pusch_decoder.h:41-78
 *   lib/phy/upper/channel_processors/pusch_decoder_impl.cpp:121-225 (segment_rx -> per codeblock rate-dematch + LDPC decode
 *   with the per-codeblock CRC, skip of codeblocks already decoded in a previous transmission, TB assembly, TB CRC24A,
 *   reset of the codeblock CRC flags when the TB CRC fails), ldpc_segmenter_impl.cpp:253-334 for the segmentation.
 * The HARQ state the reference keeps in an rx_softbuffer (include/srsran/phy/upper/rx_softbuffer.h:42-72) lives in three
 * caller-owned DEVICE arrays: soft bits [codeblock][N], decoded codeblock messages [codeblock][ceil(K/8)] and CRC flags
 * [codeblock]; a transport block addresses its slice through `harq_cb_index` (index of its first codeblock).
 * The transport block bytes are written only when every codeblock CRC passed (like the reference). */
typedef struct {
  uint8_t  bg;                  /* segmenter_cfg.base_graph: 1 or 2 */
  uint8_t  rv;                  /* segmenter_cfg.rv */
  uint8_t  mod;                 /* bits per symbol of segmenter_cfg.mod */
  uint8_t  nof_layers;          /* segmenter_cfg.nof_layers */
  uint8_t  new_data;            /* configuration::new_data */
  uint8_t  use_early_stop;      /* configuration::use_early_stop */
  uint16_t nof_ldpc_iterations; /* configuration::nof_ldpc_iterations */
  uint32_t Nref;                /* segmenter_cfg.Nref */
  uint32_t nof_ch_symbols;      /* segmenter_cfg.nof_ch_symbols */
  uint32_t tb_bytes;            /* transport_block.size() */
  uint32_t harq_cb_index;       /* first codeblock slot of this TB in the HARQ arrays */
  uint64_t llr_offset;          /* element offset of the nof_ch_symbols*mod codeword LLRs inside `llrs` */
  uint64_t tb_offset;           /* byte offset of the transport block inside `tb_out` */
} miphy_pusch_tb_desc;

typedef struct {              /* srsran::pusch_decoder_result */
  int32_t  tb_crc_ok;
  uint32_t nof_codeblocks_total;
  uint32_t iters_min;           /* ldpc_decoder_stats over the codeblocks decoded in this call (0 when none) */
  uint32_t iters_max;
  float    iters_mean;
  uint32_t nof_decoded;         /* number of observations */
} miphy_pusch_result;

/* Segmentation parameters of a transport block (ldpc::compute_nof_codeblocks / compute_lifting_size /
 * compute_codeblock_size, include/srsran/phy/upper/channel_coding/ldpc/ldpc.h:128-207). Host only. */
typedef struct {
  uint32_t nof_cbs, Z, K, N, nof_filler_bits, nof_tb_crc_bits, nof_cb_crc_bits, cb_info_bits, zero_pad;
} miphy_sch_segmentation;
int miphy_sch_segmentation_info(uint32_t tb_bytes, uint32_t bg, miphy_sch_segmentation* out);

int miphy_pusch_decode_batch(miphy_ctx*                 ctx,
                             const miphy_pusch_tb_desc* tbs, /* host */
                             uint32_t                   n,
                             const int8_t*              llrs,          /* device */
                             int8_t*                    harq_softbits, /* device, in/out, stride 66*384 per codeblock slot */
                             uint8_t*                   harq_msgs,     /* device, in/out, stride 1056 B per codeblock slot */
                             uint8_t*                   harq_crc_ok,   /* device, in/out, 1 B per codeblock slot */
                             uint8_t*                   tb_out,        /* device */
                             miphy_pusch_result*        results,       /* device, n entries */
                             void*                      stream);

/* Prepared form of miphy_pusch_decode_batch for allocations that repeat (semi-static scheduling, benchmarks): _create runs the
 * segmentation (ldpc_segmenter_impl.cpp:253-334), uploads the codeblock descriptors and fixes the decoder's launch tables and message
 * scratch once; every _run is kernel launches only
 * (CRC-flag reset, rate dematching, LDPC decoding, transport-block assembly + TB CRC + result records) with no host
 * synchronisation, on the arrays passed to that run. A plan belongs to the context it was created on and must not run
 * concurrently with itself. */
typedef struct miphy_pusch_decode_plan miphy_pusch_decode_plan;
int  miphy_pusch_decode_plan_create(miphy_ctx* ctx, const miphy_pusch_tb_desc* tbs /* host */, uint32_t n, miphy_pusch_decode_plan** out);
int  miphy_pusch_decode_plan_run(miphy_pusch_decode_plan* plan,
                                 const int8_t*            llrs,          /* device */
                                 int8_t*                  harq_softbits, /* device, in/out */
                                 uint8_t*                 harq_msgs,     /* device, in/out */
                                 uint8_t*                 harq_crc_ok,   /* device, in/out */
                                 uint8_t*                 tb_out,        /* device */
                                 miphy_pusch_result*      results,       /* device, n entries */
                                 void*                    stream);
void miphy_pusch_decode_plan_destroy(miphy_pusch_decode_plan* plan);
/* Optional per-kernel timing of the runs of a plan (measurement aid, e.g. bench.py's roofline): _enable_timing makes every run
 * record HIP events on its stream around the rate dematcher, the LDPC decoder and the transport-block assembly (a ring of max_runs
 * runs; batches above 65535 codeblocks are refused); _read_timing waits for the recorded runs, returns their mean durations in
 * milliseconds {rate dematch, LDPC decode, TB assembly} and starts a new series. */
int  miphy_pusch_decode_plan_enable_timing(miphy_pusch_decode_plan* plan, uint32_t max_runs);
int  miphy_pusch_decode_plan_read_timing(miphy_pusch_decode_plan* plan, float ms_out[3], uint32_t* runs_out);
/* What the plan will launch: info[0] = codeblocks, info[1] = 1 when every codeblock is rate-dematched while the decoder loads it (one
 * kernel reads the rate-matched LLRs and writes the soft-buffer image; the "rate dematch" time of _read_timing is then only the HARQ
 * flag reset), 0 when the dematcher runs as its own launch, info[2] = largest number of variable nodes a codeblock can reach. */
int  miphy_pusch_decode_plan_info(const miphy_pusch_decode_plan* plan, uint32_t info[3]);
/* LDPC decoder launches per run: the codeblocks of the batch are sorted into launch classes (lifting size, base graph, reachable
 * layers, dematch-in-decoder or not), one launch each. A batch of identical allocations has one. */
uint32_t miphy_pusch_decode_plan_nof_launches(const miphy_pusch_decode_plan* plan);

/* ------------------------------------------------------------------------------------------------------------------
 * PUSCH processor  --  replaces srsran::pusch_processor::process for PDUs without UCI
 *   include/srsran/phy/upper/channel_processors/pusch_processor.h:84-162
 *   lib/phy/upper/channel_processors/pusch_processor_impl.cpp:108-330
 * One call = channel estimation + demodulation + transport-block decoding of n PDUs; channel estimates and LLRs never leave the
 * device. Restrictions of the reference apply (pusch_processor_impl.cpp:96-104): DM-RS type 1, two CDM groups without data, one
 * transmit layer. HARQ arrays and `results` as in miphy_pusch_decode_batch; scalars_out: per PDU [4 rx ports][5] floats
 * {rsrp, epre, noise_var, snr, time_alignment_s} of layer 0 (what channel_estimate::get_channel_state_information averages). */
typedef struct {
  uint32_t numerology;
  uint32_t slot_in_frame;
  uint32_t rnti;
  uint32_t n_id;
  uint32_t dmrs_scrambling_id;
  uint32_t Nref;                /* tbs_lbrm_bytes * 8 */
  uint32_t tb_bytes;
  uint32_t harq_cb_index;
  uint8_t  n_scid;
  uint8_t  mod;                 /* bits per symbol */
  uint8_t  nof_rx_ports;
  uint8_t  start_symbol;
  uint8_t  nof_symbols;
  uint8_t  bg;                  /* codeword.ldpc_base_graph */
  uint8_t  rv;
  uint8_t  new_data;
  uint8_t  rx_ports[4];
  uint8_t  use_early_stop;
  uint8_t  reserved0;
  uint16_t nof_ldpc_iterations;
  uint16_t dmrs_symbols_mask;
  uint16_t grid_nof_prb;
  uint32_t pad;
  uint64_t rb_mask[5];          /* freq_alloc.get_prb_mask(bwp_start_rb, bwp_size_rb) */
  uint64_t grid_offset;         /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
  uint64_t tb_offset;           /* byte offset of the transport block inside `tb_out` */
} miphy_pusch_pdu;

/* UCI multiplexed on the PUSCH of a PDU (pusch_processor::uci_description + the lengths ulsch_information derives from it,
 * include/srsran/ran/pusch/ulsch_info.h: the caller -- the adapter through the reference's own get_ulsch_information() -- supplies them). */
typedef struct {
  uint32_t nof_harq_ack_bits, nof_csi_part1_bits, nof_csi_part2_bits;             /* O: information bits (0: field absent) */
  uint32_t nof_enc_harq_ack_bits, nof_enc_csi_part1_bits, nof_enc_csi_part2_bits; /* G: encoded, rate-matched bits */
  uint32_t nof_harq_ack_rvd;                                                      /* G^HARQ-ACK_rvd */
  uint32_t has_codeword;                                                          /* 0: the PDU carries no transport block (UCI only) */
  uint64_t harq_ack_offset, csi_part1_offset, csi_part2_offset;                   /* int8 offsets of the three soft-bit streams in uci_llr_out */
} miphy_pusch_uci;

/* _ex: PDUs with multiplexed UCI and the EVM. `uci`: NULL or n entries (host). The soft bits of the UCI fields go to `uci_llr_out`
 * (device; miphy_pusch_uci_field_jobs + miphy_uci_decode_batch enqueued behind this call on the same stream decode them there), `evm_out` (device, n floats, may be NULL) receives
 * the error vector magnitude of every PDU (pusch_demodulator::demodulation_status::evm). PDUs without codeword are demodulated and
 * demultiplexed only; their result record is zero. */
int miphy_pusch_process_batch_ex(miphy_ctx* ctx, const miphy_pusch_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */, uint32_t n,
                                 const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                 miphy_pusch_result* results, float* scalars_out, int8_t* uci_llr_out, float* evm_out, void* stream);
int miphy_pusch_process_batch(miphy_ctx* ctx, const miphy_pusch_pdu* pdus /* host */, uint32_t n, const float* grid /* device cf_t */,
                              int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out /* device */,
                              miphy_pusch_result* results /* device, n */, float* scalars_out /* device, n x 20 */, void* stream);

/* PUSCH processor for one codeword on 1..4 transmit layers  --  beyond the 23.5 reference (pusch_processor_impl.cpp asserts one layer). One
 * call chains, on one stream, miphy_dmrs_pusch_estimate_layers_batch (compact estimate), miphy_pusch_demodulate_layers_batch and
 * miphy_pusch_decode_batch (nof_layers = nof_tx_layers); estimates and LLRs stay in a workspace of the context. DM-RS type 1, single-symbol
 * DM-RS, two CDM groups without data. A batch may mix layer
 * counts; a PDU on one layer gives the bytes of miphy_pusch_process_batch for its base record (transport block, result, first 20 scalars).
 * scalars_out: per PDU 80 floats, [rx port][layer][5] at 5 * (port * nof_tx_layers + layer) as the estimator writes them. A PDU that breaks
 * a rule is MIPHY_EINVAL with nothing enqueued.
 * _ex: with multiplexed UCI and the EVM, as miphy_pusch_process_batch_ex: miphy_pusch_demodulate_layers_batch_ex in the middle, the EVM of a PDU
 * is sqrt(sum of its 14 sums / (data REs x nof_tx_layers)), miphy_ulsch_demultiplex_batch with nof_layers = nof_tx_layers in front of the
 * decoder. PDUs without codeword are demodulated and demultiplexed only, their result record is zero; one with neither codeword nor UCI is
 * refused. A PDU on one layer gives the bytes of miphy_pusch_process_batch_ex (UCI soft bits and EVM included). miphy_pusch_uci_jobs and
 * miphy_pusch_uci_field_jobs read only `mod` of a PDU record: pass them the `base` records (contiguous) to decode the fields behind this call.
 * Still out above one layer: the slot batch of the uplink processor, a prepared plan, double-symbol DM-RS, DM-RS type 2, frequency hopping. */
typedef struct {
  miphy_pusch_pdu base;
  uint8_t         nof_tx_layers; /* 1..4, <= base.nof_rx_ports */
  uint8_t         reserved[7];
} miphy_pusch_layers_pdu;
int miphy_pusch_process_layers_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus /* host */, uint32_t n, const float* grid /* device cf_t */,
                                     int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out /* device */,
                                     miphy_pusch_result* results /* device, n */, float* scalars_out /* device, n x 80 */, void* stream);
int miphy_pusch_process_layers_batch_ex(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */,
                                        uint32_t n, const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                        miphy_pusch_result* results, float* scalars_out /* n x 80 */, int8_t* uci_llr_out,
                                        float* evm_out /* device, n, may be NULL */, void* stream);

/* The layered processor for a UE with a carrier frequency offset  --  beyond the reference. miphy_pusch_process_layers_batch_ex with
 * miphy_dmrs_pusch_estimate_cfo_batch in front: the estimate is kept per OFDM symbol in the workspace of the context ([layer][port]
 * [start_symbol + nof_symbols][grid_nof_prb * 12] per PDU, up to fourteen times the compact one) and the demodulator jobs read it with
 * ce_compact = 0; every other stage is unchanged. Transport blocks, results, scalars, UCI soft bits and EVM are the bytes of the stages called
 * one by one. cfo_out: per PDU {cfo_hz, rho}. Rules and refusals: those of the layered processor; a PDU that breaks one is MIPHY_EINVAL with
 * nothing enqueued. Out: MMSE-IRC and transform precoding with an offset, the slot batch of the uplink processor, a prepared plan. */
int miphy_pusch_process_layers_cfo_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */,
                                         uint32_t n, const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                         miphy_pusch_result* results, float* scalars_out /* n x 80 */, int8_t* uci_llr_out,
                                         float* evm_out /* device, n, may be NULL */, float* cfo_out /* device, n x 2 */, void* stream);

/* The layered processor for a UE whose channel changes within the slot  --  beyond the reference. miphy_pusch_process_layers_cfo_batch with
 * miphy_dmrs_pusch_estimate_tv_batch in front (time_mode: MIPHY_TIME_INTERPOLATE or MIPHY_TIME_LINE, one value for the batch); the per-symbol
 * estimate in the workspace and everything behind it are unchanged. Transport blocks, results, scalars, UCI soft bits, EVM, cfo_out and var_out
 * are the bytes of the stages called one by one. var_out: 16 floats per PDU, the variation of (port, layer) at port * nof_tx_layers + layer, the
 * rest untouched. Rules and refusals: those of the layered processor, and the mode; a PDU that breaks one is MIPHY_EINVAL with nothing enqueued.
 * Out: MMSE-IRC and transform precoding, the slot batch of the uplink processor, a prepared plan, extended CP. */
int miphy_pusch_process_layers_tv_batch(miphy_ctx* ctx, const miphy_pusch_layers_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */,
                                        uint32_t n, const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                        miphy_pusch_result* results, float* scalars_out /* n x 80 */, int8_t* uci_llr_out,
                                        float* evm_out /* device, n, may be NULL */, float* cfo_out /* device, n x 2 */, uint32_t time_mode,
                                        float* var_out /* device, n x 16 */, void* stream);

/* The layered processor with MMSE-IRC  --  beyond the reference. The arguments of miphy_pusch_process_layers_batch_ex; one call chains, on one
 * stream, miphy_dmrs_pusch_estimate_layers_batch (compact estimate), miphy_pusch_noise_covariance_batch (the PDU's prg_size and loading; the
 * matrices stay in the workspace of the context next to estimates and LLRs), miphy_pusch_demodulate_layers_mmse_batch_ex,
 * miphy_ulsch_demultiplex_batch where UCI is multiplexed and miphy_pusch_decode_batch: transport blocks, result records, scalars, UCI soft bits
 * and EVM are the bytes of the stages called one by one. scalars_out is that of the layered processor: the estimator's scalar noise_var stays what
 * it is (forced to 0.001 epre below three DM-RS symbols), the demodulator does not read it. 1..4 layers; IRC needs more ports than layers to
 * null anything. Rules and refusals: those of the layered processor, and loading finite and >= 0; a PDU that breaks one is MIPHY_EINVAL with
 * nothing enqueued. Out: more than 4 receive ports, DM-RS type 2, double-symbol DM-RS, frequency hopping, MMSE for the transform-precoded
 * path, a covariance per OFDM symbol, the slot batch of the uplink processor, a prepared plan, the srsRAN adapters (23.5 has no MMSE factory
 * to implement). */
typedef struct {
  miphy_pusch_layers_pdu base;
  float    loading;  /* as in miphy_pusch_ncov_job */
  uint16_t prg_size; /* PRBs per covariance matrix, counted over the allocated PRBs; 0 = one matrix for the allocation */
  uint8_t  reserved[2];
} miphy_pusch_mmse_pdu;
int miphy_pusch_process_layers_mmse_batch(miphy_ctx* ctx, const miphy_pusch_mmse_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */,
                                          uint32_t n, const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                          miphy_pusch_result* results, float* scalars_out /* n x 80 */, int8_t* uci_llr_out,
                                          float* evm_out /* device, n, may be NULL */, void* stream);

/* PUSCH processor for a transform-precoded PUSCH (DFT-s-OFDM)  --  beyond the 23.5 reference, whose pusch_processor::pdu_t cannot express the
 * waveform. One call chains, on one stream, miphy_dmrs_pusch_estimate_tp_batch (compact estimate, scaling 10^(3/20), base.dmrs_scrambling_id =
 * n_ID^RS, base.n_scid = 0, `hopping` as in miphy_pusch_chest_tp_job), miphy_pusch_demodulate_tp_batch_ex, miphy_ulsch_demultiplex_batch when
 * UCI is multiplexed and miphy_pusch_decode_batch; the bytes are those of the stages called one by one. One layer, DM-RS type 1, two CDM
 * groups without data, a contiguous allocation of 2^a 3^b 5^c <= 270 PRBs other than 1, 3 and 4 (MIPHY_EUNSUPP: their DM-RS tables are not in
 * the library; such a PDU is served by miphy_port_channel_estimate_batch with the caller's pilots, miphy_pusch_demodulate_tp_batch and
 * miphy_pusch_decode_batch). Outputs, scalars_out (20 per PDU), UCI soft bits and EVM as miphy_pusch_process_batch_ex. A PDU that breaks a
 * rule is MIPHY_EINVAL with nothing enqueued. Out: a prepared plan, graph capture, the slot batch of the uplink processor. */
typedef struct {
  miphy_pusch_pdu base;
  uint8_t         hopping; /* 0 neither, 1 group hopping, 2 sequence hopping (TS 38.211 6.4.1.1.1.2) */
  uint8_t         reserved[7];
} miphy_pusch_tp_pdu;
int miphy_pusch_process_tp_batch(miphy_ctx* ctx, const miphy_pusch_tp_pdu* pdus /* host */, uint32_t n, const float* grid /* device cf_t */,
                                 int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out /* device */,
                                 miphy_pusch_result* results /* device, n */, float* scalars_out /* device, n x 20 */, void* stream);
int miphy_pusch_process_tp_batch_ex(miphy_ctx* ctx, const miphy_pusch_tp_pdu* pdus /* host */, const miphy_pusch_uci* uci /* host or NULL */, uint32_t n,
                                    const float* grid, int8_t* harq_softbits, uint8_t* harq_msgs, uint8_t* harq_crc_ok, uint8_t* tb_out,
                                    miphy_pusch_result* results, float* scalars_out /* n x 20 */, int8_t* uci_llr_out,
                                    float* evm_out /* device, n, may be NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * UL-SCH demultiplexer  --  replaces srsran::ulsch_demultiplex::demultiplex / get_placeholders (UCI multiplexed on PUSCH)
 *   include/srsran/phy/upper/channel_processors/ulsch_demultiplex.h:38-110, ulsch_placeholder_list.h:35-105
 *   lib/phy/upper/channel_processors/ulsch_demultiplex_impl.cpp:74-453 (TS 38.212 6.2.7)
 * One job = one PUSCH codeword: the descrambled LLRs of the demodulator are split into the UL-SCH data stream (all-zero
 * elements where HARQ-ACK punctures reserved resource elements) and the HARQ-ACK / CSI part 1 / CSI part 2 streams. */
typedef struct {
  uint8_t  mod;                         /* bits per symbol */
  uint8_t  nof_layers;                  /* 1..4 */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;
  uint8_t  dmrs_type;                   /* 1 or 2 */
  uint8_t  nof_cdm_groups_without_data;
  uint16_t dmrs_symbols_mask;           /* bit l = OFDM symbol l carries DM-RS */
  uint16_t nof_prb;                     /* PRBs allocated to the transmission */
  uint16_t reserved;
  uint32_t nof_harq_ack_rvd;            /* G^HARQ-ACK_rvd: bits reserved for HARQ-ACK (0 when more than two HARQ-ACK bits are sent) */
  uint32_t nof_enc_harq_ack_bits;       /* G^HARQ-ACK: encoded, rate-matched bits of each field = length of its output stream */
  uint32_t nof_enc_csi_part1_bits;
  uint32_t nof_enc_csi_part2_bits;
  uint32_t nof_harq_ack_bits;           /* O: information bits of each field (a field with exactly one bit has repetition placeholders) */
  uint32_t nof_csi_part1_bits;
  uint32_t nof_csi_part2_bits;
  uint64_t in_offset;                   /* int8 offset of the codeword LLRs */
  uint64_t sch_offset;                  /* int8 offsets of the four output streams */
  uint64_t harq_ack_offset;
  uint64_t csi_part1_offset;
  uint64_t csi_part2_offset;
} miphy_ulsch_demux_job;

/* Host: number of LLRs of the codeword (input) and of the UL-SCH data stream (output) of a job. MIPHY_EINVAL for an impossible
 * configuration (the reference asserts: fields that do not fit the allocation). */
int miphy_ulsch_demux_sizes(const miphy_ulsch_demux_job* job, uint32_t* nof_in_llr, uint32_t* nof_sch_llr);
/* Host: ulsch_demultiplex::get_placeholders -- indices (in the order of the input resource elements) of the elements that carry a
 * repetition placeholder; at most `cap` are written, *n is the full count. */
int miphy_ulsch_placeholders(const miphy_ulsch_demux_job* job, uint16_t* re_indices, uint32_t cap, uint32_t* n);
int miphy_ulsch_demultiplex_batch(miphy_ctx* ctx, const miphy_ulsch_demux_job* jobs /* host */, uint32_t n, const int8_t* llr_in /* device */,
                                  int8_t* sch_out, int8_t* harq_ack_out, int8_t* csi_part1_out, int8_t* csi_part2_out /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * UCI decoder (short-block detector)  --  replaces srsran::uci_decoder::decode / srsran::short_block_detector::detect
 *   include/srsran/phy/upper/channel_processors/uci_decoder.h:38-56, lib/phy/upper/channel_processors/uci_decoder_impl.cpp:41-50,
 *   lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:58-199 (TS 38.212 5.3.3 / 5.4.3)
 * One job = one UCI field of 1 to 11 bits (the reference decodes no longer field): rate dematch of its nof_llr soft bits with the
 * saturating LLR sum, ML detection over the codewords of the short block code and the GLRT verdict, bit-exact with the reference.
 * `payload` receives nof_bits bytes per job (one bit per byte, like span<uint8_t> in the reference), `status[i]` the
 * srsran::uci_status of job i (include/srsran/phy/upper/channel_processors/uci_status.h:28-41): MIPHY_UCI_STATUS_VALID or _INVALID.
 * Host jobs are checked first (MIPHY_EINVAL, nothing enqueued: nof_bits outside 1..11, mod not 1/2/4/6/8, and the reference's
 * preconditions nof_llr > nof_bits for 3..11 bits, nof_llr >= mod for 1 bit, nof_llr >= 3 mod for 2 bits); a device job that fails
 * them is skipped (its payload and status are not written). n == 0 enqueues nothing. */
enum { MIPHY_UCI_STATUS_UNKNOWN = 0, MIPHY_UCI_STATUS_VALID = 1, MIPHY_UCI_STATUS_INVALID = 2 };
typedef struct {
  uint8_t  nof_bits;       /* K: 1..11 */
  uint8_t  mod;            /* bits per symbol of the modulation the field was sent with (uci_decoder::configuration::modulation) */
  uint16_t reserved;
  uint32_t nof_llr;        /* E: soft bits of the field */
  uint64_t llr_offset;     /* int8 offset of the field's soft bits inside `llr` (any alignment) */
  uint64_t payload_offset; /* byte offset of the field's nof_bits payload bytes inside `payload` */
} miphy_uci_field_job;

int miphy_uci_decode_batch(miphy_ctx* ctx, const miphy_uci_field_job* jobs, int jobs_on_device, uint32_t n, const int8_t* llr /* device */,
                           uint8_t* payload /* device */, uint8_t* status /* device, n */, void* stream);
/* Host: the field jobs of n PUSCH PDUs over the `uci_llr_out` layout miphy_pusch_process_batch_ex writes: one job per present field
 * (nof_*_bits != 0), PDU after PDU in the order HARQ-ACK, CSI part 1, CSI part 2, payloads packed from byte 0 in job order. `jobs`
 * holds up to 3 n entries; job_field (NULL or as many entries) receives 3 * pdu + field (0 HARQ-ACK, 1 CSI part 1, 2 CSI part 2) per
 * job, *nof_jobs the count. MIPHY_EINVAL for a field above 11 bits or one the detector refuses. With these jobs, _ex and
 * miphy_uci_decode_batch go on one stream without a host synchronisation in between. */
int miphy_pusch_uci_field_jobs(const miphy_pusch_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, miphy_uci_field_job* jobs, uint32_t* job_field,
                               uint32_t* nof_jobs);

/* ------------------------------------------------------------------------------------------------------------------
 * UCI decoder, polar-coded fields of 12 to 1706 bits  --  beyond the 23.5 reference, whose uci_decoder_impl.cpp:44 stops at 11 bits
 * while lib/ran/pusch/ulsch_info.cpp:29-42 already sizes these fields. Framing of TS 38.212 6.3.1.2-6.3.1.5 / 6.3.2 (5.2.1, 5.3.1):
 *   C = 2 if (A >= 360 and E >= 1088) or A >= 1013, else 1; L = 6 (CRC6) for A <= 19, else 11 (CRC11); A' = ceil(A / C) C; with
 *   C = 2 and odd A one zero bit is prepended; segment r = a'[r A'/C, (r + 1) A'/C) followed by the L CRC bits of the segment alone;
 *   K_r = A'/C + L, E_r = floor(E / C); segment r owns soft bits [r E_r, (r + 1) E_r) of the field (with C = 2 and odd E the last
 *   soft bit is never read); polar code (K_r, E_r, nMax = 10, ibil = 1), nPC = 3 for K_r <= 25, CRC bits not interleaved.
 * A field is accepted when K_r + nPC < E_r and E_r <= 8192. Each segment goes through the reference's rate dematcher, its
 * list-size-1 SSC decoder and its deallocator (bit-exact with miphy_polar_decode_batch), then its CRC is checked. `payload` always
 * receives the A decoded bits (one per byte, segments concatenated, pad bit dropped); `status[i]` is MIPHY_UCI_STATUS_VALID when the
 * CRC of every segment matches, else MIPHY_UCI_STATUS_INVALID. DECISION: the decoded value of the pad bit is not checked.
 * Jobs are HOST memory only (the polar codes of a call are constructed on the host); device-resident jobs and stream capture of this
 * entry point are out of scope. The call only enqueues on `stream`. Every job is checked before anything is staged: a bad job gives
 * MIPHY_EINVAL with the rule in miphy_last_error() and nothing is enqueued; so do null arguments and n > 2^24. n == 0 enqueues
 * nothing. (A HIP or staging failure between two pieces of a large call, MIPHY_EHIP, leaves the earlier pieces enqueued.) The tables
 * of a call travel with it through the context's staging ring in pieces of at most 1 MiB (tasks and code tables of the piece
 * together; a piece is one or two launches); no device allocation is made for a code. */
#define MIPHY_UCI_POLAR_MIN_BITS 12
#define MIPHY_UCI_POLAR_MAX_BITS 1706
typedef struct {
  uint16_t nof_bits;       /* A: 12..1706 */
  uint16_t reserved;
  uint32_t nof_llr;        /* E */
  uint64_t llr_offset;     /* int8 offset inside `llr`, any alignment */
  uint64_t payload_offset; /* byte offset of the A payload bytes inside `payload` */
} miphy_uci_polar_job;
typedef struct {
  uint32_t C;   /* segments: 1 or 2 */
  uint32_t L;   /* CRC bits per segment: 6 or 11 */
  uint32_t K_r; /* polar message length of a segment, CRC included */
  uint32_t E_r; /* rate-matched length of a segment */
  uint32_t n;   /* log2 of the mother code size */
  uint32_t nPC; /* parity-check bits: 3 or 0 */
} miphy_uci_polar_info_t;
/* Host: the framing of a field of nof_bits bits received as nof_llr soft bits; 0, or MIPHY_EINVAL with the rule's message. */
int miphy_uci_polar_info(uint32_t nof_bits, uint32_t nof_llr, miphy_uci_polar_info_t* out);
int miphy_uci_polar_decode_batch(miphy_ctx* ctx, const miphy_uci_polar_job* jobs /* host */, uint32_t n, const int8_t* llr /* device */,
                                 uint8_t* payload /* device */, uint8_t* status /* device, n */, void* stream);
/* Host: like miphy_pusch_uci_field_jobs, but a PDU's fields of 1..11 bits go to `short_jobs` and those of 12..1706 bits to
 * `polar_jobs` (up to 3 n entries each), payloads packed from byte 0 of ONE payload buffer in (PDU, field) order whichever list a
 * field lands in; short_field / polar_field (NULL or as many entries) receive 3 * pdu + field per job as job_field does. With these
 * jobs, _ex, miphy_uci_decode_batch and miphy_uci_polar_decode_batch go on one stream without a host synchronisation in between
 * (each decoder with its own status array). */
int miphy_pusch_uci_jobs(const miphy_pusch_pdu* pdus, const miphy_pusch_uci* uci, uint32_t n, miphy_uci_field_job* short_jobs, uint32_t* short_field,
                         uint32_t* nof_short, miphy_uci_polar_job* polar_jobs, uint32_t* polar_field, uint32_t* nof_polar);
/* Test hooks, process-wide: bytes a piece of miphy_uci_polar_decode_batch may take (0 = the default, 1 MiB; a piece always holds at
 * least one field), and the number of pieces of the call that finished last, on whichever context. */
void     miphy_debug_set_uci_polar_piece_bytes(size_t bytes);
unsigned miphy_debug_uci_polar_pieces(void);
/* CRC-aided list decoding of the same fields: jobs, framing, checks, staging in pieces, outputs and error behaviour are those of
 * miphy_uci_polar_decode_batch. list_size must be 1, 2, 4 or 8; anything else is MIPHY_EINVAL with nothing enqueued. DECISIONS:
 *   - list_size == 1 is miphy_uci_polar_decode_batch byte for byte, that is the SSC kernel, not the list recursion at L = 1, which
 *     breaks the tie of a zero LLR at an information bit differently.
 *   - Fields of 12..19 bits (CRC6, three parity-check bits) go through the SSC kernel at every list size: a list that forks on
 *     parity-check positions without enforcing them is not what TS 38.212 intends, and six CRC bits leave no margin for eight
 *     candidates. One call still takes every field.
 *   - Fields of 20..1706 bits (CRC11, nPC = 0) at list sizes 2 / 4 / 8, per segment: rate dematching as above, then the list recursion
 *     of the oracle's orc_polar_scl_decode (LLR path metric, ties to the lower candidate index); the K_r bits of every survivor are
 *     taken in K-set order (no interleaver, no leading ones, no mask) and CRC11 of the first K_r - 11 is tested against the last 11.
 *     The segment's result is the survivor with the smallest (metric, slot) among those that pass, or the smallest (metric, slot)
 *     overall where none passes. The field is VALID when every segment has a passing survivor; `payload` always receives the chosen
 *     survivors' bits. The call sets the status bytes of these fields on `stream` before the segments, decoded independently of one
 *     another, overwrite them.
 * Beyond the 23.5 reference, which has no list decoder; pinned to the oracle through tests/polar_scl_ref.py. */
int miphy_uci_polar_decode_list_batch(miphy_ctx* ctx, const miphy_uci_polar_job* jobs /* host */, uint32_t n, uint32_t list_size,
                                      const int8_t* llr /* device */, uint8_t* payload /* device */, uint8_t* status /* device, n */, void* stream);
/* Test hook, process-wide: the segments the call that finished last sent to the SSC kernel and to the list kernel. */
void miphy_debug_uci_polar_list_segments(unsigned* ssc, unsigned* list);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH processor, formats 1 and 2  --  replaces srsran::pucch_processor::process(grid, format1_configuration / format2_configuration)
 *   lib/phy/upper/channel_processors/pucch_processor_impl.cpp:28-189 (estimate, detect or demodulate + decode, CSI),
 *   lib/phy/upper/signal_processors/pucch/dmrs_pucch_processor_format{1,2}_impl.cpp + port_channel_estimator_average_impl.cpp:97-347
 *   (pilots, LS, averaging per hop, noise, RSRP / EPRE / SNR, time alignment, interpolation),
 *   lib/phy/upper/channel_processors/pucch_detector_impl.cpp:155-415 (format 1: ZF 1x1, w* and conj(r_uv), detect_bits, threshold 2.33),
 *   lib/phy/upper/channel_processors/pucch_demodulator_impl.cpp:28-90 (format 2: ZF 1xN, QPSK soft demapping, descrambling with
 *   c_init = rnti 2^15 + n_id) followed by the short-block detector of miphy_uci_decode_batch.
 * All PDUs read one device grid through their own window: grid + grid_offset (cf_t units) laid out [port][14][grid_nprb * 12], the
 * layout of the rest of the uplink, receive ports 0 .. nof_ports - 1 of the window. A contiguous range of ports is reached through
 * grid_offset; an arbitrary list of the reference's `ports` (e.g. {0, 2}) cannot be expressed and has to be gathered into a grid of
 * its own first (pucch_processor_hip does). Normal cyclic prefix, no group or sequence hopping.
 * Results: `payload` receives one bit per byte from payload_offset in pucch_uci_message order (HARQ-ACK, SR, CSI part 1); format 1
 * writes nof_harq_ack bytes (none for SR alone: the verdict is the status, VALID for a positive SR, UNKNOWN when the detected bit is 1,
 * as in the reference). `results[i]` gets the status, the detection metric (format 1, divided by the threshold as in the reference;
 * 0 for format 2) and the channel state information: EPRE, RSRP and SINR averaged linearly over the ports before the conversion to
 * dB, time alignment averaged over the ports (channel_estimation.h:211-233). `llr_out` (device, may be NULL) receives the 16 nof_prb
 * nof_symbols format-2 soft bits from llr_offset. Host jobs are checked first (MIPHY_EINVAL, nothing enqueued) against the
 * reference's assertions (pucch_processor_impl.cpp:191-285, pucch_detector_impl.cpp:155-186, and the detector's w* table which
 * asserts an OCC index below each hop's data-symbol count); a device job that fails them is skipped (nothing of it is written).
 * n == 0 enqueues nothing. The call only enqueues, so it can be captured in a HIP graph. */
typedef struct {
  uint8_t  format;               /* 1 or 2 */
  uint8_t  numerology;           /* slot_point numerology, 0..4 */
  uint16_t slot;                 /* slot index within the frame */
  uint8_t  nof_ports;            /* receive ports 1..4 (ports 0 .. nof_ports - 1 of the grid window) */
  uint8_t  start_symbol;         /* start_symbol_index */
  uint8_t  nof_symbols;          /* format 1: 4..14, format 2: 1..2 */
  uint8_t  intra_slot_hopping;   /* format 1: second_hop_prb.has_value(); format 2: must be 0 */
  uint16_t bwp_start_rb, bwp_size_rb;
  uint16_t starting_prb;         /* within the BWP */
  uint16_t second_hop_prb;       /* within the BWP, format 1 with hopping */
  uint8_t  nof_prb;              /* format 2: 1..16 */
  uint8_t  initial_cyclic_shift; /* format 1: 0..11 */
  uint8_t  time_domain_occ;      /* format 1: 0..6 */
  uint8_t  nof_harq_ack;         /* format 1: 0..2 */
  uint8_t  nof_sr, nof_csi_part1, nof_csi_part2; /* format 2: 3..11 bits in all (_ex: 3 and more), CSI part 2 must be 0 */
  uint8_t  reserved0;
  uint16_t n_id;                 /* format 1: 0..1023 (group u = n_id mod 30, v = 0, cyclic-shift hopping c_init); format 2: scrambling */
  uint16_t n_id_0;               /* format 2: DM-RS scrambling identity */
  uint16_t rnti;                 /* format 2 */
  uint16_t reserved1;
  uint32_t grid_nprb;            /* width of the grid window in PRBs (>= bwp_start_rb + bwp_size_rb) */
  uint64_t grid_offset;          /* cf_t offset of the window in `grid` */
  uint64_t payload_offset;       /* byte offset in `payload` */
  uint64_t llr_offset;           /* int8 offset in `llr_out` (format 2) */
} miphy_pucch_job;

typedef struct {
  uint8_t status; /* MIPHY_UCI_STATUS_* */
  uint8_t reserved[3];
  float   detection_metric; /* format 1, normalised like the reference (metric / 2.33) */
  float   epre_db, rsrp_db, sinr_db, time_alignment_s; /* channel_state_information */
} miphy_pucch_result;

int miphy_pucch_process_batch(miphy_ctx* ctx, const miphy_pucch_job* jobs, int jobs_on_device, uint32_t n, const float* grid /* device cf_t */,
                              uint8_t* payload /* device */, miphy_pucch_result* results /* device, n */, int8_t* llr_out /* device or NULL */,
                              void* stream);
/* Format 2 above 11 bits  --  beyond the 23.5 reference, whose processor asserts on such a PDU (pucch_processor_impl.cpp:282-287) and
 * whose uci_decoder stops at 11 bits. A batch may mix format-1 PDUs, format-2 PDUs of 3..11 bits and format-2 PDUs of K = nof_harq_ack
 * + nof_sr + nof_csi_part1 >= 12 bits ("long"); jobs and results keep their layout. For format-1 and short format-2 PDUs payload, record
 * and soft bits are those of miphy_pucch_process_batch byte for byte, whatever list_size is. For a long PDU estimation, channel state
 * information, equalisation, demapping and descrambling are the same kernel's (the soft bits do not depend on K); its E = 16 nof_prb
 * nof_symbols soft bits are then decoded as ONE polar-coded UCI field of A = K bits exactly as miphy_uci_polar_decode_list_batch
 * decodes it (E <= 512, so always one segment): `payload` gets the K decoded bits, one per byte, in the order HARQ-ACK, SR, CSI part 1,
 * whatever the verdict; results[i].status is MIPHY_UCI_STATUS_VALID or _INVALID from the CRC; detection_metric is 0. list_size 1 is
 * the SSC kernel; 2 / 4 / 8 the list kernel from 20 bits, while 12..19 bits stay with the SSC kernel at every list size.
 * The call enqueues the PUCCH kernel once for all n PDUs and the polar decoder behind it on the same stream, which stores its verdict
 * over the status byte the kernel wrote; nothing waits for the device. Without `llr_out` the soft bits of the long PDUs pass through
 * a workspace of the context (512 bytes per long PDU); payload and status are the same either way.
 * Jobs are HOST memory only (the polar codes are constructed on the host; no stream capture). Every job is checked before anything is
 * enqueued; MIPHY_EINVAL with the rule in miphy_last_error() and nothing written for: list_size not 1, 2, 4 or 8; a null argument; a
 * job miphy_pucch_process_batch refuses for another reason than its bit count above 11; nof_csi_part2 != 0; a long PDU whose (K, E)
 * miphy_uci_polar_info refuses (12 bits on 16 soft bits, 21 on 32, 501 on 512). n == 0 enqueues nothing. (A HIP or staging failure
 * behind the PUCCH kernel, MIPHY_EHIP, leaves that kernel enqueued, as between two pieces of miphy_uci_polar_decode_batch.) The code
 * rate limit of the reference's validator (0.8) is not a rule here: pucch_pdu_validator_hip applies it. */
int miphy_pucch_process_batch_ex(miphy_ctx* ctx, const miphy_pucch_job* jobs /* HOST */, uint32_t n, uint32_t list_size,
                                 const float* grid /* device cf_t */, uint8_t* payload /* device */, miphy_pucch_result* results /* device, n */,
                                 int8_t* llr_out /* device or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH processor, formats 3 and 4 (DFT-s-OFDM, TS 38.211 6.3.2.6 and 6.4.1.3.3)  --  beyond the 23.5 reference, whose demodulator asserts
 * "PUCCH Format 3 not supported" / "PUCCH Format 4 not supported" (pucch_demodulator_impl.cpp) and whose format3_configuration and
 * format4_configuration hold nothing but the cyclic prefix. The contract is the standard, restated in numpy in tests/pucch_f34_tx.py
 * (transmitter) and tests/pucch_f34_ref.py (receiver); the arithmetic of the receiver is stated at the top of csrc/pucch_f34.hip.
 * n PDUs read one device grid through their windows as the PDUs of miphy_pucch_process_batch do, one workgroup each: channel estimation
 * per port and hop on the DM-RS symbols of Table 6.4.1.3.3.2-1 (all 12 REs of a PRB, low-PAPR sequence of 12 nof_prb elements with the
 * cyclic-shift hopping of format 1), zero forcing 1 x N, de-precoding, format-4 despreading, QPSK or pi/2-BPSK soft demapping and
 * descrambling (c_init = rnti 2^15 + n_id_scrambling). The K = nof_harq_ack + nof_sr + nof_csi_part1 bits are decoded by the short-block
 * detector inside the kernel (3..11 bits) or by the polar decoder behind it on the same stream (12 bits and more, list size `list_size`
 * with the meaning it has in miphy_pucch_process_batch_ex), which stores its verdict over the status byte. Nothing waits for the device.
 * Rules (miphy_pucch_f34_info, and therefore the batch call; MIPHY_EINVAL unless stated, the rule in miphy_last_error()):
 * format 3 with nof_prb in {1, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16}; nof_prb = 2 needs the length-24 table the library does not hold:
 * MIPHY_EUNSUPP, as miphy_low_papr_sequence answers; format 4 with nof_prb = 1, occ_length 2 or 4, occ_index < occ_length; nof_symbols
 * 4..14; K >= 3; nof_csi_part2 == 0 (the two-part multiplexing of TS 38.212 6.3.1.6 is not done); K <= 11: K < E; K >= 12: what
 * miphy_uci_polar_info(K, E) says; numerology, slot, ports, BWP, PRBs and grid as for miphy_pucch_job. Normal cyclic prefix, no group
 * or sequence hopping (u = n_id_hopping mod 30, v = 0). The code-rate limit is not a rule.
 * E = Qm 12 nof_prb (data symbols) for format 3 and Qm (12 / occ_length) (data symbols) for format 4, Qm = 1 for pi/2-BPSK, else 2.
 * Outputs: `payload` K bytes from payload_offset (HARQ-ACK, SR, CSI part 1), results[i] as for format 2 (detection_metric 0),
 * `llr_out` (device or NULL) the E soft bits from llr_offset, `est_out` (device float or NULL) from est_offset (in floats) the estimate
 * the data path used: cf_t [port][hop: 1 or 2][12 nof_prb], then nof_ports floats of noise variance. Without llr_out the soft bits of the
 * polar-coded PDUs pass through a workspace of the context. Jobs are HOST memory only; every job is checked before anything is enqueued;
 * n == 0 enqueues nothing. */
typedef struct {
  uint8_t  format;             /* 3 or 4 */
  uint8_t  numerology;         /* 0..4 */
  uint16_t slot;               /* slot index within the frame */
  uint8_t  nof_ports;          /* receive ports 1..4 (ports 0 .. nof_ports - 1 of the grid window) */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;        /* 4..14 */
  uint8_t  intra_slot_hopping; /* 1: the first floor(nof_symbols / 2) symbols on starting_prb, the others on second_hop_prb */
  uint16_t bwp_start_rb, bwp_size_rb;
  uint16_t starting_prb;       /* within the BWP */
  uint16_t second_hop_prb;     /* within the BWP, with hopping */
  uint8_t  nof_prb;            /* format 3: see above; format 4: 1 */
  uint8_t  pi2_bpsk;           /* 0: QPSK, 1: pi/2-BPSK */
  uint8_t  additional_dmrs;    /* 0 or 1 */
  uint8_t  occ_length;         /* format 4: 2 or 4 */
  uint8_t  occ_index;          /* format 4: below occ_length */
  uint8_t  reserved0[3];
  uint16_t nof_harq_ack, nof_sr, nof_csi_part1, nof_csi_part2; /* K = the first three, 3 and more; CSI part 2 must be 0 */
  uint16_t n_id_hopping;       /* 0..1023: u and the cyclic-shift hopping */
  uint16_t n_id_scrambling;    /* 0..1023 */
  uint16_t rnti;
  uint16_t reserved1;
  uint32_t grid_nprb;          /* width of the grid window in PRBs (>= bwp_start_rb + bwp_size_rb) */
  uint32_t reserved2;
  uint64_t grid_offset;        /* cf_t offset of the window in `grid` */
  uint64_t payload_offset;     /* byte offset in `payload` */
  uint64_t llr_offset;         /* int8 offset in `llr_out` */
  uint64_t est_offset;         /* float offset in `est_out` */
} miphy_pucch_f34_job;

typedef struct {
  uint32_t dmrs_symbols_mask;   /* bit l: symbol l of the slot carries DM-RS */
  uint32_t nof_dmrs_symbols[2]; /* per hop ([1] = 0 without hopping) */
  uint32_t nof_data_symbols[2]; /* per hop */
  uint32_t M;                   /* 12 nof_prb */
  uint32_t E;                   /* soft bits */
  uint32_t polar;               /* 0: short block code (K <= 11), 1: polar code */
} miphy_pucch_f34_info_t;

/* Host function, no device. */
int miphy_pucch_f34_info(const miphy_pucch_f34_job* job, miphy_pucch_f34_info_t* out);
int miphy_pucch_process_f34_batch(miphy_ctx* ctx, const miphy_pucch_f34_job* jobs /* HOST */, uint32_t n, uint32_t list_size,
                                  const float* grid /* device cf_t */, uint8_t* payload /* device */, miphy_pucch_result* results /* device, n */,
                                  int8_t* llr_out /* device or NULL */, float* est_out /* device or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PUCCH processor, format 0 (TS 38.211 6.3.2.3, TS 38.213 9.2.3)  --  beyond the 23.5 reference, whose pucch_detector::format0_configuration is an
 * empty struct and whose pucch_processor::format0_configuration cannot express a PDU. The contract is the standard, restated in numpy in
 * tests/pucch_f0_tx.py (transmitter) and tests/pucch_f0_ref.py (receiver, thresholds included); the arithmetic of the detector is stated at the top of
 * csrc/pucch_f0.hip. Format 0 has no DM-RS: the detector decides between the cyclic shifts of the PDU's hypotheses without a channel estimate, against a
 * noise level that is either given (noise_var) or estimated from the cyclic shifts of the PRB that nobody uses (used_shifts_mask: bit k' set = some PDU
 * of this resource may use the unhopped shift k'; the scheduler knows). n PDUs read one device grid through their windows as the PDUs of
 * miphy_pucch_process_batch do, one wavefront each, four to a workgroup, in one launch.
 * Hypotheses, in this order (m_cs of TS 38.213 9.2.3 added to initial_cyclic_shift modulo 12): one HARQ-ACK bit: 0 -> 0, 1 -> 6; two (b0, b1):
 * (0,0) -> 0, (0,1) -> 3, (1,1) -> 6, (1,0) -> 9; SR alone: 0; SR with HARQ-ACK: those hypotheses (negative SR) followed by the positive-SR ones, one
 * bit: 0 -> 3, 1 -> 9, two bits: (0,0) -> 1, (0,1) -> 4, (1,1) -> 7, (1,0) -> 10. H = 1, 2, 4, 4 or 8.
 * Results: `payload` receives the best hypothesis whatever the verdict, nof_harq_ack bytes then nof_sr bytes from payload_offset (SR alone: 1 when the
 * verdict is VALID, else 0); results[i].status is MIPHY_UCI_STATUS_VALID when the metric (energy of the best hypothesis over the noise energy of one
 * shift) reaches the threshold, else _INVALID; detection_metric = metric / threshold, as format 1 normalises it; epre_db = 10 log10 of the energy per
 * (port, symbol) summed over the twelve shifts, rsrp_db of the best hypothesis, sinr_db of that over the per-RE noise variance; time_alignment_s = 0 (a
 * delay and a cyclic shift cannot be told apart without DM-RS). `energy_out` (device float or NULL) receives the twelve unhopped shift energies E[k']
 * from energy_offset. The detector assumes a channel that is flat over the PRB; a timing offset leaks energy into neighbouring shifts.
 * threshold = 0 asks for the default: a false-alarm probability of 1 % per PDU, union bound over the H hypotheses, in closed form from the degrees of
 * freedom D = nof_ports nof_symbols and F = free shifts (miphy_pucch_f0_info reports it). The default is host arithmetic: host jobs get it filled in,
 * device-resident jobs must carry a threshold > 0.
 * Rules (miphy_pucch_f0_info, and therefore the batch call; MIPHY_EINVAL with the rule in miphy_last_error()): format 0; numerology, slot, ports, BWP,
 * PRBs and grid as for miphy_pucch_job; nof_symbols 1..2 within the slot; intra_slot_hopping only with two symbols; initial_cyclic_shift 0..11;
 * nof_harq_ack 0..2, nof_sr 0..1, not both 0; used_shifts_mask below 2^12; n_id 0..1023; threshold and noise_var finite and not negative; with
 * noise_var = 0 at least one shift outside used_shifts_mask and the PDU's own hypotheses. Normal cyclic prefix, no group or sequence hopping
 * (u = n_id mod 30, v = 0). Host jobs are all checked before anything is enqueued; a device job that fails a rule, or carries threshold 0, is skipped
 * (nothing of it is written). n == 0 enqueues nothing. The call only enqueues and allocates nothing on the device once the context holds the Gold
 * tables (any earlier PUCCH call), so with device jobs it can be captured in a HIP graph. */
typedef struct {
  uint8_t  format;               /* 0 */
  uint8_t  numerology;           /* 0..4 */
  uint16_t slot;                 /* slot index within the frame */
  uint8_t  nof_ports;            /* receive ports 1..4 (ports 0 .. nof_ports - 1 of the grid window) */
  uint8_t  start_symbol;         /* 0..13 */
  uint8_t  nof_symbols;          /* 1..2 */
  uint8_t  intra_slot_hopping;   /* 1 (two symbols only): the second symbol is on second_hop_prb */
  uint16_t bwp_start_rb, bwp_size_rb;
  uint16_t starting_prb;         /* within the BWP */
  uint16_t second_hop_prb;       /* within the BWP, with hopping */
  uint8_t  initial_cyclic_shift; /* 0..11 */
  uint8_t  nof_harq_ack;         /* 0..2 */
  uint8_t  nof_sr;               /* 0..1 */
  uint8_t  reserved0;
  uint16_t used_shifts_mask;     /* bit k': the unhopped shift k' may carry a signal of some PDU of this PRB */
  uint16_t n_id;                 /* 0..1023: group u = n_id mod 30 and the cyclic-shift hopping c_init */
  float    threshold;            /* on the metric; 0 = the default (host jobs only) */
  float    noise_var;            /* per-RE noise variance; 0 = estimate it from the free shifts */
  uint32_t grid_nprb;            /* width of the grid window in PRBs (>= bwp_start_rb + bwp_size_rb) */
  uint32_t reserved1;
  uint64_t grid_offset;          /* cf_t offset of the window in `grid` */
  uint64_t payload_offset;       /* byte offset in `payload` */
  uint64_t energy_offset;        /* float offset in `energy_out` */
} miphy_pucch_f0_job;

typedef struct {
  uint32_t nof_hypotheses; /* H */
  uint8_t  shifts[8];      /* unhopped cyclic shift of every hypothesis, in the order above */
  uint32_t D;              /* nof_ports nof_symbols */
  uint32_t free_mask;      /* shifts neither in used_shifts_mask nor among the hypotheses */
  uint32_t F;              /* their number */
  float    threshold;      /* what the batch call would compare the metric with */
} miphy_pucch_f0_info_t;

/* Host function, no device. */
int miphy_pucch_f0_info(const miphy_pucch_f0_job* job, miphy_pucch_f0_info_t* out);
int miphy_pucch_process_f0_batch(miphy_ctx* ctx, const miphy_pucch_f0_job* jobs, int jobs_on_device, uint32_t n, const float* grid /* device cf_t */,
                                 uint8_t* payload /* device */, miphy_pucch_result* results /* device, n */, float* energy_out /* device or NULL */,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * SRS channel estimator (TS 38.211 6.4.1.4)  --  beyond the 23.5 reference, which has no SRS code. The contract is the standard, restated in numpy in
 * tests/srs_tx.py (transmitter) and tests/srs_ref.py (float64 receiver); the arithmetic is stated at the top of csrc/srs.hip. It measures what the
 * precoding entry points consume: one channel matrix per PRG (and the per-UE time alignment); miphy_precoding_weights_batch computes the weights from it.
 * One job is the symbols of one SRS resource that lie on the same PRBs, in one slot. Decision: the job carries the resolved frequency position
 * (start_prb, nof_prb). The hopping pattern, C_SRS / B_SRS / n_shift / n_RRC and TS 38.211 Table 6.4.1.4.3-1 stay with the scheduler, and a
 * frequency-hopping resource is submitted as one job per hop. n jobs read one device grid through their windows as the PDUs of
 * miphy_pucch_process_f0_batch do (receive port r, symbol l of the slot, subcarrier k at grid_offset + (14 r + l) 12 grid_nprb + k; start_prb in
 * grid numbering), one workgroup each, in one launch.
 * The signal, normal cyclic prefix: n_cs_max = 8 (comb 2) or 12 (comb 4); transmit port i has n_cs,i = (cyclic_shift + n_cs_max i / N_ap) mod n_cs_max
 * and the comb offset (comb_offset + K / 2) mod K when N_ap = 4, i is 1 or 3 and cyclic_shift >= n_cs_max / 2, else comb_offset; M = 12 nof_prb / K
 * elements per symbol; u = (f_gh + n_id) mod 30 with f_gh from group hopping (hopping = 1) and v from sequence hopping (hopping = 2, M >= 72), both with
 * c_init = n_id and the symbol index in the slot. M = 12 is the table of the PUCCH kernels, M >= 36 Zadoff-Chu (N_ZC up to 1627: nof_prb 272 at comb 2
 * has M = 1632, above what miphy_low_papr_sequence serves, whose limit stays); M = 24 is MIPHY_EUNSUPP (TS 38.211 Table 5.2.2.2-4 is not held).
 * Estimates: with P = the transmit ports that share a comb (N_ap, or 2 when four ports split over two combs), Q = 12 prg_size / K comb elements per PRG
 * and G = nof_prb / prg_size PRGs, `h_out` receives H[g][rx][tx] as cf_t from h_offset (G nof_rx_ports nof_tx_ports of them): the channel at the centre
 * element of the PRG on the port's comb, as the grid shows it (the delay is not removed from it). results[i]: h_wb[rx][tx] the mean over the PRGs of
 * the delay-compensated estimates (unused entries 0); noise_var (linear, per element) from the residual of the fit; epre_db of the SRS elements;
 * rsrp_db[tx] (unused entries 0); sinr_db of the mean RSRP over noise_var; time_alignment_s, one delay per job from the phase of the lag-P correlation
 * of the comb elements. The unambiguous delay range is |tau| < 1 / (2 delta_f K P) (miphy_srs_info reports it): a larger delay wraps. The estimator
 * takes a comb to carry the job's ports and nothing else; UEs that share a comb at cyclic shifts n_cs_max / P apart are estimated as the ports of one
 * job with that P, and UEs on other comb offsets or PRBs do not enter.
 * Rules (miphy_srs_info, and therefore the batch calls; MIPHY_EINVAL, or MIPHY_EUNSUPP for M = 24, with the rule in miphy_last_error()): numerology
 * 0..4 and the slot within its frame; nof_rx_ports 1..4; nof_tx_ports 1, 2 or 4; nof_symbols 1, 2 or 4 within the slot; comb_size 2 or 4, comb_offset
 * below it; cyclic_shift below n_cs_max; n_id 0..1023; hopping 0..2; prg_size 1, 2 or 4; nof_prb a multiple of 4 in 4..272; start_prb + nof_prb within
 * grid_nprb <= 275; Q a multiple of P (the ports of a comb are separated over whole periods of their relative cyclic shifts).
 * miphy_srs_pilots_batch writes the transmitted sequences [symbol][tx port][M] of every job from pilots_offset: it pins sequence, hopping and cyclic
 * shifts independently of the estimator. Host jobs are all checked before anything is enqueued; a device job that fails a rule is skipped (nothing of it
 * is written). n == 0 enqueues nothing. The calls only enqueue and allocate nothing on the device once the context holds the Gold tables (any earlier
 * PUCCH or SRS call), so with device jobs they can be captured in a HIP graph. */
typedef struct {
  uint8_t  numerology;    /* 0..4 */
  uint8_t  nof_rx_ports;  /* receive ports 1..4 (ports 0 .. nof_rx_ports - 1 of the grid window) */
  uint16_t slot;          /* slot index within the frame */
  uint8_t  nof_tx_ports;  /* N_ap: 1, 2 or 4 */
  uint8_t  start_symbol;  /* 0..13 */
  uint8_t  nof_symbols;   /* 1, 2 or 4 */
  uint8_t  comb_size;     /* K: 2 or 4 */
  uint8_t  comb_offset;   /* below comb_size */
  uint8_t  cyclic_shift;  /* n_cs: below 8 (comb 2) or 12 (comb 4) */
  uint8_t  hopping;       /* 0 neither, 1 group, 2 sequence */
  uint8_t  prg_size;      /* PRBs per estimate: 1, 2 or 4 */
  uint16_t start_prb;     /* first PRB of the allocation, in grid numbering */
  uint16_t nof_prb;       /* a multiple of 4 in 4..272 */
  uint16_t n_id;          /* 0..1023: sequence identity */
  uint16_t reserved0;
  uint32_t grid_nprb;     /* width of the grid window in PRBs (>= start_prb + nof_prb) */
  uint64_t grid_offset;   /* cf_t offset of the window in `grid` */
  uint64_t h_offset;      /* cf_t offset in `h_out` */
  uint64_t pilots_offset; /* cf_t offset in `pilots` (miphy_srs_pilots_batch) */
} miphy_srs_job;

typedef struct {
  uint32_t M;                /* sequence length, 12 nof_prb / comb_size */
  uint32_t Q;                /* comb elements per PRG */
  uint32_t P;                /* transmit ports that share a comb */
  uint32_t G;                /* PRGs */
  uint32_t nof_combs;        /* 1, or 2 when four ports split */
  uint8_t  cyclic_shifts[4]; /* n_cs,i per transmit port (unused entries 0) */
  uint8_t  comb_offsets[4];  /* comb offset per transmit port (unused entries 0) */
  uint32_t nof_h;            /* cf_t of the job in `h_out`: G nof_rx_ports nof_tx_ports */
  float    max_delay_s;      /* the estimate is unambiguous for |delay| below this: 1 / (2 delta_f K P) */
} miphy_srs_info_t;

typedef struct {
  float    h_wb[4][4][2];    /* [rx][tx][re, im]: mean over the PRGs of the delay-compensated estimates; unused entries 0 */
  float    noise_var;        /* linear, per element */
  float    epre_db;
  float    rsrp_db[4];       /* per transmit port; unused entries 0 */
  float    sinr_db;
  float    time_alignment_s;
  uint32_t reserved[2];      /* not written */
} miphy_srs_result;

/* Host function, no device. */
int miphy_srs_info(const miphy_srs_job* job, miphy_srs_info_t* out);
int miphy_srs_pilots_batch(miphy_ctx* ctx, const miphy_srs_job* jobs, int jobs_on_device, uint32_t n, float* pilots /* device cf_t */, void* stream);
int miphy_srs_estimate_batch(miphy_ctx* ctx, const miphy_srs_job* jobs, int jobs_on_device, uint32_t n, const float* grid /* device cf_t */,
                             float* h_out /* device cf_t */, miphy_srs_result* results /* device, n */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Precoding weights from SRS channel matrices  --  beyond the 23.5 reference, which computes no precoding. The contract is restated in numpy in
 * tests/precoding_weights_ref.py (float64, and float32 in the kernel's operation order); the arithmetic is stated at the top of
 * csrc/precoding_weights.hip. It joins miphy_srs_estimate_batch to the precoding entry points without leaving the device.
 * A job serves nof_ues = 1..4 co-scheduled UEs on A = nof_ports = 1..4 gNB antenna ports (the SRS jobs' nof_rx_ports). UE k: h_offset names the block
 * H_k[g][a][u] as miphy_srs_estimate_batch wrote it for a sounding of nof_prb PRBs from start_prb (grid numbering) at prg_size 1, 2 or 4, with
 * nof_ue_ports U_k = 1, 2 or 4 (the SRS job's nof_tx_ports); it is served nof_layers l_k = 1..U_k layers. L = sum l_k <= 4 and <= A.
 * The output PRGs are those of miphy_precoding: PRG j covers the grid PRBs [j prg_size, (j + 1) prg_size), j < nof_prg. For every one of them:
 *  1. R_k = (sum_i w_i conj(H_k[i]) H_k[i]^T) / sum_i w_i (A x A) over the SRS PRGs i whose PRBs meet PRG j, w_i = the PRBs they share; where none
 *     does, the nearest sounded SRS PRG alone (the band edge). Gram matrices are averaged, never H: the estimate keeps the UE's delay as a phase ramp.
 *  2. Eigen-decomposition of R_k by cyclic Jacobi: five sweeps over (p, q) = (0,1), (0,2), .. (A-2, A-1); a rotation is skipped when |R_pq|^2 is not a
 *     positive normal number. Eigenvalues descending, on a tie the lower column first; a negative one (rounding) counts as 0.
 *  3. Rows g_(k,i) = sqrt(lambda_(k,i)) v_(k,i)^H, i < l_k, stacked UE by UE into G (L x A).
 *  4. W = G^H (G G^H + reg I)^-1 (regularised zero forcing; for one UE plain eigen-beamforming), every column scaled to 2-norm `amplitude`, then turned
 *     so that its entry on antenna port 0 is real and not negative (left as it is where that entry is below 2^-10 of the norm).
 *  5. Abnormal rule: if a pivot of the factorisation or the squared norm of a column is not a positive normal number (more layers than the channel has
 *     rank at reg = 0; a zero matrix), every UE gets zero weights and zero sig / leak for that PRG. Nothing else is affected.
 * UE k receives W[j][a][i] at weights[weights_offset + (j A + a) l_k + i] (cf_t): the memory order of miphy_precoding, so a PDSCH job of that UE with
 * nof_ports = A and this prg_size / nof_prg points straight at it; and, where `metrics` is not NULL, three floats per PRG and layer at
 * metrics[metrics_offset + 3 (j l_k + i)]: lambda, sig = |g w_own|^2 and leak = sum over the job's other columns of |g w_other|^2.
 * Rules (miphy_precoding_weights_info, and therefore the batch call; MIPHY_EINVAL with the rule in miphy_last_error()): nof_ues 1..4; nof_ports 1..4;
 * prg_size and nof_prg >= 1; reg finite and >= 0; amplitude a positive normal number; per UE prg_size 1, 2 or 4, nof_prb a multiple of 4 in 4..272 with
 * start_prb + nof_prb <= 275, nof_ue_ports 1, 2 or 4, nof_layers 1..nof_ue_ports; L <= 4 and <= nof_ports; and, in the batch call,
 * weights_offset + nof_prg A l_k <= nof_weights. Host jobs are all checked before anything is enqueued; a device-resident job that breaks a rule is
 * skipped with nothing written. n == 0 enqueues nothing. The call only enqueues and allocates nothing, so with device jobs it can be captured in a HIP
 * graph. A job's bits depend on the job alone: it takes the lane form (one lane per output PRG) when no output PRG meets more than 8 SRS PRGs of a
 * UE, else the wave form (one wavefront per output PRG); miphy_precoding_weights_info reports which. */
typedef struct {
  uint64_t h_offset;       /* cf_t offset of H_k[0][0][0] in `h` */
  uint32_t weights_offset; /* cf_t index of this UE's W[0][0][0] in `weights` */
  uint32_t metrics_offset; /* float index of this UE's first metric in `metrics` */
  uint16_t start_prb;      /* first PRB of the sounding, in grid numbering */
  uint16_t nof_prb;        /* a multiple of 4 in 4..272 */
  uint8_t  prg_size;       /* PRBs per SRS estimate: 1, 2 or 4 */
  uint8_t  nof_ue_ports;   /* U: 1, 2 or 4 */
  uint8_t  nof_layers;     /* 1..U */
  uint8_t  reserved0;
} miphy_precoding_weights_ue;

typedef struct {
  uint8_t  nof_ues;   /* 1..4 */
  uint8_t  nof_ports; /* A: 1..4 */
  uint16_t prg_size;  /* PRBs per output PRG, >= 1 (wideband: nof_prg = 1 and prg_size = the grid) */
  uint16_t nof_prg;   /* >= 1 */
  uint16_t reserved0;
  float    reg;       /* >= 0, in units of |h|^2 */
  float    amplitude; /* > 0: the 2-norm of every column */
  miphy_precoding_weights_ue ue[4]; /* entries from nof_ues on are not read */
} miphy_precoding_weights_job;

typedef struct {
  uint32_t nof_layers;     /* L */
  uint32_t nof_weights[4]; /* cf_t per UE: nof_prg A l_k (unused entries 0) */
  uint32_t nof_metrics[4]; /* floats per UE: 3 nof_prg l_k (unused entries 0) */
  uint32_t max_srs_prg;    /* the largest number of SRS PRGs of one UE under one output PRG */
  uint32_t wave_form;      /* 0: lane form, 1: wave form */
} miphy_precoding_weights_info_t;

/* Host function, no device. */
int miphy_precoding_weights_info(const miphy_precoding_weights_job* job, miphy_precoding_weights_info_t* out);
int miphy_precoding_weights_batch(miphy_ctx* ctx, const miphy_precoding_weights_job* jobs, int jobs_on_device, uint32_t n,
                                  const float* h /* device cf_t */, float* weights /* device cf_t */, uint32_t nof_weights,
                                  float* metrics /* device float, or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PRACH detector and generator  --  replace srsran::prach_detector::detect and srsran::prach_generator::generate
 *   lib/phy/upper/channel_processors/prach_detector_simple_impl.cpp:35-169 (RSSI, per preamble: correlation in the frequency domain,
 *   unnormalised IDFT, peak of |c|^2, metric peak / (rssi preamble_power L L) against 0.07, delay sign and window),
 *   lib/phy/upper/channel_processors/prach_generator_impl.cpp:105-301 (closed-form y_u,v, logical root index modulo the table size),
 *   lib/ran/prach/prach_cyclic_shifts.cpp (N_CS), lib/ran/prach/prach_preamble_information.cpp (L, RA subcarrier spacing, N_CP).
 * One job is one PRACH occasion: the detector reads one symbol of L = 839 (formats 0..3) or 139 (the others) cf_t at symbol_offset in
 * `symbols` -- prach_buffer::get_symbol(0, 0, 0, 0), one port, no combining -- and tests the preamble indices start_preamble_index ..
 * start_preamble_index + nof_preamble_indices - 1. Unrestricted sets only. Formats and RA subcarrier spacings are numbered like the
 * reference's enums (MIPHY_PRACH_FORMAT_*, ra_scs 0..3 = 15..120 kHz, read for short formats only).
 * `results[i]` gets what the detector derives per occasion: the linear RSSI, delay_n_maximum (the smaller of the cyclic prefix in
 * samples at ra_scs * idft_size and, for N_CS != 0, N_CS idft_size / L), N_CS and whether the N_CS bound was the limiting one (then
 * time_advance_max = from_seconds(delay_n_maximum / sampling rate), else the cyclic prefix). `preambles` gets one record per
 * requested preamble index from preamble_offset, detected or not: the index of the peak, delay_n (the peak index, or peak index -
 * idft_size above idft_size / 2), the peak power (power_dB = 10 log10 of it), the metric, and `detected` = 1 only when the metric is not
 * below 0.07 and |delay_n| < delay_n_maximum; the reference's result lists those in preamble-index order, with time_advance =
 * from_seconds(delay_n / sampling rate) and snr_dB = 0. An RSSI that is not a normal float (an all-zero symbol) gives records with
 * detected = 0 and zero index, power and metric.
 * idft_size: 1536 or 3072 (the reference asserts a multiple of 1536; these are the ones one LDS pass transforms).
 * Host jobs are checked first (MIPHY_EINVAL, nothing enqueued) against the reference's assertions: a format it serves (and ra_scs
 * 0..3 for a short one), an unrestricted set, a zone whose N_CS is not reserved (0..15), start + number <= 64, idft_size; a device job
 * that fails them is skipped (nothing of it is written). n == 0 enqueues nothing. The call only enqueues and uses no scratch, so it
 * can be captured in a HIP graph (once the context holds the twiddles of the IDFT size: any earlier call with it). */
enum {
  MIPHY_PRACH_FORMAT_0 = 0, MIPHY_PRACH_FORMAT_1, MIPHY_PRACH_FORMAT_2, MIPHY_PRACH_FORMAT_3, MIPHY_PRACH_FORMAT_A1, MIPHY_PRACH_FORMAT_A2,
  MIPHY_PRACH_FORMAT_A3, MIPHY_PRACH_FORMAT_B1, MIPHY_PRACH_FORMAT_B4, MIPHY_PRACH_FORMAT_C0, MIPHY_PRACH_FORMAT_C2, MIPHY_PRACH_FORMAT_A1_B1,
  MIPHY_PRACH_FORMAT_A2_B2, MIPHY_PRACH_FORMAT_A3_B3, MIPHY_PRACH_NOF_FORMATS
};
#define MIPHY_PRACH_MAX_PREAMBLES 64

typedef struct {
  uint32_t format;                /* MIPHY_PRACH_FORMAT_* */
  uint32_t ra_scs;                /* short formats: 0..3 = 15, 30, 60, 120 kHz */
  uint32_t root_sequence_index;   /* logical; root_sequence_index + preamble offset wraps modulo 838 / 138 */
  uint32_t zero_correlation_zone; /* 0..15 */
  uint32_t restricted_set;        /* 0 = unrestricted (the only one served) */
  uint32_t start_preamble_index;
  uint32_t nof_preamble_indices;  /* 0..64, start + number <= 64 */
  uint32_t idft_size;             /* 1536 or 3072 */
  uint32_t symbol_offset;         /* cf_t offset of the symbol in `symbols` */
  uint32_t preamble_offset;       /* record offset of the first preamble result in `preambles` */
} miphy_prach_job;

typedef struct {
  float    rssi;            /* linear; rssi_dB = 10 log10 */
  uint32_t delay_n_maximum; /* samples of the IDFT grid */
  uint32_t n_cs;
  uint32_t n_cs_limited;    /* 1: delay_n_maximum comes from N_CS, 0: from the cyclic prefix */
} miphy_prach_result;

typedef struct {
  uint32_t peak_index;
  int32_t  delay_n;    /* signed */
  float    peak_power; /* max |c|^2 */
  float    metric;     /* peak_power / (rssi preamble_power L L) */
  uint32_t detected;
} miphy_prach_preamble_result;

int miphy_prach_detect_batch(miphy_ctx* ctx, const miphy_prach_job* jobs, int jobs_on_device, uint32_t n, const float* symbols /* device cf_t */,
                             miphy_prach_result* results /* device, n */, miphy_prach_preamble_result* preambles /* device */, void* stream);

/* Frequency-domain preambles y_u,v of n (format, root_sequence_index, zero_correlation_zone, preamble_index): L cf_t each at out_offset
 * (cf_t units) in `out`. Same checks and conventions as above (restricted_set must be 0; ra_scs plays no part). */
typedef struct {
  uint32_t format;
  uint32_t root_sequence_index;
  uint32_t zero_correlation_zone;
  uint32_t restricted_set;
  uint32_t preamble_index; /* 0..63 */
  uint32_t out_offset;     /* cf_t offset in `out` */
} miphy_prach_gen_job;

int miphy_prach_generate_batch(miphy_ctx* ctx, const miphy_prach_gen_job* jobs, int jobs_on_device, uint32_t n, float* out /* device cf_t */,
                               void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * OFDM PRACH demodulator  --  replaces srsran::ofdm_prach_demodulator::demodulate
 *   lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:31-199 (per time-domain occasion: start, cyclic prefix with the 16 kappa
 *   extensions at 0 and 0.5 ms, one DFT of sampling_rate / RA spacing points per symbol, per frequency-domain occasion the L bins from
 *   k_start, the lower half of the PRACH grid being the top of the spectrum), lib/ran/prach/prach_preamble_information.cpp (symbol and
 *   cyclic-prefix lengths, the B value of an A/B pair on the last occasion, get_prach_window_duration),
 *   lib/ran/prach/prach_frequency_mapping.cpp (nof_rb_ra, k_bar).
 * One job is one window of baseband samples of one port: nof_samples cf_t at samples_offset in `samples`, the first one being the start
 * of the slot the configuration counts its start_symbol from. The job's nof_td_occasions x nof_fd_occasions x symbols rows of L cf_t go
 * to `buffer` laid out like prach_buffer_impl, [td][fd][symbol][L] with the strides max_nof_fd_occasions and max_nof_symbols from
 * buffer_offset = get_symbol(port, 0, 0, 0): row (td, fd, symbol) starts at buffer_offset + ((td max_nof_fd_occasions + fd)
 * max_nof_symbols + symbol) L, which is where miphy_prach_job.symbol_offset of a detector job on the same stream can point (symbol 0).
 * Nothing else of `buffer` is written. DFT sizes: the ones miphy_dft_batch serves; up to 4096 a symbol is one workgroup's transform in
 * LDS, above (4608 ... 49152) the four-step transform whose second step produces only the bins of the occasions.
 * JOBS ARE HOST MEMORY in this entry point: launch geometry, DFT sizes, twiddle tables and scratch follow from them. `samples` and
 * `buffer` are device memory. Every job is checked with miphy_prach_demod_info before anything is enqueued; the table of symbol tasks
 * travels through the context's staging ring and the call only enqueues. n == 0 does nothing.
 * miphy_prach_demod_info (host only, no device needed) returns what the reference derives from a job at a sampling rate, or
 * MIPHY_EINVAL where the reference asserts: a format that is not a PRACH format or a PUSCH spacing above 120 kHz; a long format with
 * nof_td_occasions != 1; zero occasions; occasions beyond MIPHY_PRACH_MAX_TD_OCCASIONS / MIPHY_PRACH_MAX_FD_OCCASIONS or the buffer's
 * strides (fd occasions, symbols); a reserved (RA spacing, PUSCH spacing) pair; dft_size <= nof_prb_ul_grid K 12; k_start + L >= that
 * grid size; a start, cyclic prefix or (short formats) window that is not a whole number of samples at the sampling rate; a sampling
 * rate the RA spacing does not divide; a window shorter than what an occasion reads or (short formats) than the window duration.
 * A stride above MIPHY_PRACH_MAX_STRIDE is MIPHY_EINVAL too (this interface's own bound; products of job fields are formed in 64 bits).
 * MIPHY_EUNSUPP: everything above holds and the DFT size is not one the device transforms (e.g. format 0 at 122.88 MHz).
 * Size of a call: any n. The task table (64 bytes per window, time-domain occasion and symbol) is staged in pieces of at most 1 MiB, one
 * launch (pair) per piece, so it never outgrows the ring. Scratch: none up to 4096 points; above, dft_size * 8 bytes per symbol in
 * flight from the context's general workspace, at most 64 MiB (a piece holds as many symbols as fit: 341 of 24576 points, 170 of 49152),
 * which the context keeps until it is destroyed. */
#define MIPHY_PRACH_MAX_TD_OCCASIONS 7
#define MIPHY_PRACH_MAX_FD_OCCASIONS 8
#define MIPHY_PRACH_MAX_STRIDE 65535u /* max_nof_fd_occasions, max_nof_symbols */
typedef struct {
  uint32_t format;               /* MIPHY_PRACH_FORMAT_* */
  uint32_t pusch_scs;            /* 0..3 = 15..120 kHz, as srsran::subcarrier_spacing; short formats use it as RA spacing too */
  uint32_t nof_td_occasions, nof_fd_occasions, start_symbol, rb_offset, nof_prb_ul_grid;
  uint32_t nof_samples;          /* length of the window at samples_offset */
  uint64_t samples_offset;       /* cf_t offset of the window (slot start) in `samples` */
  uint64_t buffer_offset;        /* cf_t offset of get_symbol(port, 0, 0, 0) in `buffer` */
  uint32_t max_nof_fd_occasions, max_nof_symbols; /* buffer strides: [td][fd][symbol][L], as prach_buffer_impl */
} miphy_prach_demod_job;          /* one job = one window of one port */

typedef struct {
  uint32_t L;              /* 839 or 139 */
  uint32_t ra_scs_hz;      /* 1250, 5000, 15000 << pusch_scs */
  uint32_t dft_size;       /* sampling rate / ra_scs_hz */
  uint32_t nof_symbols;    /* per occasion */
  uint32_t K;              /* PUSCH spacing / RA spacing */
  uint32_t k_bar, nof_rb_ra;
  uint32_t window_samples; /* get_prach_window_duration in samples */
  uint32_t td_sample_offset[MIPHY_PRACH_MAX_TD_OCCASIONS]; /* start of the occasion (its cyclic prefix) in the window */
  uint32_t td_cp_samples[MIPHY_PRACH_MAX_TD_OCCASIONS];    /* cyclic prefix with the 16 kappa extensions */
  uint32_t k_start[MIPHY_PRACH_MAX_FD_OCCASIONS];          /* first subcarrier of the occasion in the PRACH grid */
} miphy_prach_demod_info_t;

int miphy_prach_demod_info(uint32_t sampling_rate_hz, const miphy_prach_demod_job* job, miphy_prach_demod_info_t* out); /* host only */
int miphy_prach_demodulate_batch(miphy_ctx* ctx, uint32_t sampling_rate_hz, const miphy_prach_demod_job* jobs /* host */, uint32_t n,
                                 const float* samples /* device cf_t */, float* buffer /* device cf_t */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH encoder (whole transport blocks)  --  replaces srsran::pdsch_encoder::encode
 *   include/srsran/phy/upper/channel_processors/pdsch_encoder.h, lib/phy/upper/channel_processors/pdsch_encoder_impl.cpp:28-65
 *   (segment_tx: TB CRC16/24A, CB CRC24B, zero padding, fillers -> LDPC encode -> rate match into the codeword),
 *   ldpc_segmenter_impl.cpp:89-234.
 * tb_in: packed transport blocks; codeword_out: one bit per byte, nof_ch_symbols*mod bytes per TB. */
typedef struct {
  uint8_t  bg;
  uint8_t  rv;
  uint8_t  mod;
  uint8_t  nof_layers;
  uint32_t Nref;
  uint32_t nof_ch_symbols;
  uint32_t tb_bytes;
  uint64_t tb_offset;       /* byte offset of the packed transport block inside `tb_in` */
  uint64_t codeword_offset; /* byte offset of the codeword inside `codeword_out` */
} miphy_pdsch_tb_desc;

int miphy_pdsch_encode_batch(miphy_ctx* ctx, const miphy_pdsch_tb_desc* tbs /* host */, uint32_t n, const uint8_t* tb_in /* device */,
                             uint8_t* codeword_out /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PDSCH processor (whole PDUs)  --  replaces srsran::pdsch_processor::process
 *   include/srsran/phy/upper/channel_processors/pdsch_processor.h:64-165, lib/phy/upper/channel_processors/pdsch_processor_impl.cpp:110-305
 * Transport block -> resource grid in one call: the number of data REs of the allocation (reserved patterns and the DM-RS
 * pattern of the bandwidth part excluded, pdsch_processor_impl.cpp:198-220), pdsch_encoder (Nref = 8 * tbs_lbrm_bytes),
 * pdsch_modulator with scaling 10^(-ratio_pdsch_data_to_sss_dB / 20) and dmrs_pdsch_processor with amplitude
 * 10^(-ratio_pdsch_dmrs_to_sss_dB / 20) on the same port. The codewords stay on the device. Same restrictions as the
 * reference (pdsch_processor_impl.cpp:143-196): DM-RS type 1, one codeword on one layer, contiguous allocation. */
typedef struct {
  uint32_t slot_in_frame;              /* pdu.slot.slot_index() */
  uint32_t rnti;
  uint32_t n_id;                       /* data scrambling identity */
  uint32_t dmrs_scrambling_id;
  uint32_t tbs_lbrm_bytes;             /* 1 .. 66*384/8 */
  uint32_t tb_bytes;
  float    ratio_pdsch_dmrs_to_sss_dB;
  float    ratio_pdsch_data_to_sss_dB;
  uint8_t  bg;                         /* 1 or 2 */
  uint8_t  rv;
  uint8_t  mod;                        /* bits per symbol */
  uint8_t  port;                       /* grid port of the layer */
  uint8_t  start_symbol;
  uint8_t  nof_symbols;
  uint8_t  nof_cdm_groups_without_data;
  uint8_t  n_scid;
  uint8_t  ref_point_prb0;             /* 1: DM-RS reference point is the first PRB of the BWP (pdu_t::PRB0), 0: CRB0 */
  uint8_t  nof_reserved;               /* 0..4 */
  uint16_t dmrs_symbols_mask;
  uint16_t grid_nof_prb;
  uint16_t bwp_start_rb;
  uint16_t bwp_size_rb;
  uint16_t pad;
  uint64_t rb_mask[5];                 /* allocated PRBs, grid numbering */
  miphy_re_pattern reserved[4];
  uint64_t tb_offset;                  /* byte offset of the packed transport block inside `tb_in` */
  uint64_t grid_offset;                /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
} miphy_pdsch_pdu;

/* Data REs of the allocation (pdsch_processor_impl::compute_nof_data_re); 0 on an invalid PDU. Host function. */
uint32_t miphy_pdsch_pdu_nof_re(const miphy_pdsch_pdu* pdu);
int miphy_pdsch_process_batch(miphy_ctx* ctx, const miphy_pdsch_pdu* pdus /* host */, uint32_t n, const uint8_t* tb_in /* device */,
                              float* grid /* device cf_t; only the mapped REs are written */, void* stream);
/* Prepared form for allocations that repeat slot after slot: PDU validation, segmentation and descriptor uploads once, a run only
 * launches (TB CRC, codeblock preparation, LDPC encoder, rate matcher, modulator, DM-RS) on buffers the plan owns, no staging, no
 * allocation, no host synchronisation. */
typedef struct miphy_pdsch_process_plan miphy_pdsch_process_plan;
int  miphy_pdsch_process_plan_create(miphy_ctx* ctx, const miphy_pdsch_pdu* pdus /* host */, uint32_t n, miphy_pdsch_process_plan** out);
int  miphy_pdsch_process_plan_run(miphy_pdsch_process_plan* plan, const uint8_t* tb_in /* device */, float* grid /* device cf_t */, void* stream);
void miphy_pdsch_process_plan_destroy(miphy_pdsch_process_plan* plan);

/* PDSCH processor, one codeword on 1..4 layers (beyond the 23.5 reference; the contract is the oracle chain orc_pdsch_encode with
 * nof_layers = L and nof_ch_symbols = REs x L -> orc_pdsch_modulate -> orc_dmrs_pdsch_map on the same port list). As
 * miphy_pdsch_process_batch with the data-RE count per layer, miphy_pdsch_modulate_layers_batch and the DM-RS of type 1 on DM-RS ports
 * 1000 .. 1000 + L - 1, DM-RS port p on grid port ports[p]; the two scalings are those of the one-layer processor. base.port is ignored.
 * One stream, no host synchronisation, the codewords stay on the device. Every PDU is checked before anything is enqueued: the rules of
 * miphy_pdsch_process_batch and of miphy_pdsch_modulate_layers_batch, and the encoder's limit on the transport block -- at most 52
 * codeblocks (ldpc::MAX_NOF_SEGMENTS), that is tb_bytes <= 54753 on base graph 1 and <= 24801 on base graph 2, and at least one RE per
 * layer for each codeblock. A batch of one-layer PDUs writes the bytes miphy_pdsch_process_batch writes. There is no prepared plan for
 * this entry point (miphy_pdsch_process_plan_* stays one-layer). */
typedef struct {
  miphy_pdsch_pdu base;
  uint8_t nof_layers; /* 1..4 */
  uint8_t ports[4];   /* grid port of each layer (and of DM-RS port 1000 + layer), distinct, < 16 */
  uint8_t pad[3];
} miphy_pdsch_layers_pdu;

/* Data REs of the allocation per layer; 0 on an invalid PDU. Host function. */
uint32_t miphy_pdsch_layers_pdu_nof_re(const miphy_pdsch_layers_pdu* pdu);
int miphy_pdsch_process_layers_batch(miphy_ctx* ctx, const miphy_pdsch_layers_pdu* pdus /* host */, uint32_t n, const uint8_t* tb_in /* device */,
                                     float* grid /* device cf_t; only the mapped REs are written */, void* stream);

/* PDSCH processor with the PRBs of a PDU in a mapping order of the caller's (interleaved VRB-to-PRB mapping, TS 38.211 7.3.1.6: the list
 * miphy_vrb_to_prb_list gives). miphy_pdsch_process_layers_batch with miphy_pdsch_modulate_mapped_batch in the middle; the contract is the
 * oracle chain orc_pdsch_encode -> orc_pdsch_modulate(the list) -> orc_dmrs_pdsch_map(rb_mask): the DM-RS does not depend on the mapping
 * order. The list of PDU p is prb_lists[prb_list_offset .. + nof_prb - 1] (host memory) and obeys the list rule of
 * miphy_pdsch_modulate_mapped_batch; nof_prb = 0: no list, and a batch without lists writes the bytes miphy_pdsch_process_layers_batch
 * writes. Every PDU and every list is checked before anything is enqueued or allocated, with the limits of the layered processor. PDUs are
 * host records; there is no prepared plan for this entry point. Precoding: miphy_pdsch_process_precoded_batch. Two codewords (5..8 layers):
 * miphy_pdsch_process_codewords_batch. */
typedef struct {
  miphy_pdsch_layers_pdu layers; /* layers.base.rb_mask = the PRBs of the list */
  uint32_t prb_list_offset;      /* uint16 index into prb_lists */
  uint16_t nof_prb;              /* 0: no list -- ascending order of rb_mask */
  uint16_t pad;
} miphy_pdsch_mapped_pdu;
int miphy_pdsch_process_mapped_batch(miphy_ctx* ctx, const miphy_pdsch_mapped_pdu* pdus /* host */, uint32_t n, const uint16_t* prb_lists /* host */,
                                     uint32_t nof_list_entries, const uint8_t* tb_in /* device */,
                                     float* grid /* device cf_t; only the mapped REs are written */, void* stream);

/* PDSCH processor on one or two transport blocks, 1..8 layers: miphy_pdsch_process_mapped_batch with miphy_pdsch_modulate_codewords_batch in
 * the middle. With L = nof_layers = 5..8 the PDU carries two transport blocks: block q is encoded on its own L_q layers (L0 = floor(L / 2),
 * L1 = L - L0) with its own base graph, redundancy version and modulation; tbs_lbrm_bytes, the scrambling identities, the two power ratios
 * and the allocation are shared (pdsch_processor::pdu_t). The contract is the oracle chain: orc_pdsch_encode per transport block with
 * nof_layers = L_q and nof_ch_symbols = REs x L_q, orc_pdsch_modulate with both codewords and the list, orc_dmrs_pdsch_map on DM-RS ports
 * 1000 .. 1000 + L - 1 of type 1, DM-RS port p on grid port ports[p]. Every PDU, list and both transport blocks are checked before anything
 * is enqueued or allocated ("pdsch_process_codewords: PDU <i>: ..."; the rules of the PDU record that every processor words as
 * "pdsch_process: PDU <i>: ..." keep that wording, for either transport block): per transport block at most 52 codeblocks, at least one RE
 * per layer for each codeblock, rv <= 3. DM-RS ports 1004 .. 1007 of type 1 exist only on a double-symbol DM-RS, so for L >= 5 two more rules apply:
 * nof_cdm_groups_without_data = 2, and every set bit of dmrs_symbols_mask belongs to a run of exactly two adjacent symbols. With L <= 4 the
 * fields of transport block 1 are ignored, and the call writes the bytes miphy_pdsch_process_mapped_batch writes and refuses what it
 * refuses. mapped.layers.nof_layers and mapped.layers.ports are ignored. Still out: precoding of two codewords, a prepared plan,
 * device-resident PDUs, more than 52 codeblocks per transport block. */
typedef struct {
  miphy_pdsch_mapped_pdu mapped; /* transport block 0 (base.bg, rv, mod, tb_bytes, tb_offset) and everything the two share */
  uint8_t  nof_layers;           /* 1..8; 1..4: one transport block, 5..8: two */
  uint8_t  ports[8];             /* grid port of each layer (and of DM-RS port 1000 + layer), distinct, < 16 */
  uint8_t  bg1;                  /* transport block 1 */
  uint8_t  rv1;
  uint8_t  mod1;
  uint32_t tb_bytes1;
  uint64_t tb_offset1;
} miphy_pdsch_codewords_pdu;
typedef char miphy_pdsch_codewords_pdu_is_344_bytes[sizeof(miphy_pdsch_codewords_pdu) == 344 ? 1 : -1];

/* Data REs of the allocation per layer; 0 on an invalid PDU. Host function. */
uint32_t miphy_pdsch_codewords_pdu_nof_re(const miphy_pdsch_codewords_pdu* pdu);
int miphy_pdsch_process_codewords_batch(miphy_ctx* ctx, const miphy_pdsch_codewords_pdu* pdus /* host */, uint32_t n, const uint16_t* prb_lists /* host */,
                                        uint32_t nof_list_entries, const uint8_t* tb_in /* device */,
                                        float* grid /* device cf_t; only the mapped REs are written */, void* stream);

/* PDSCH processor with precoding: miphy_pdsch_process_mapped_batch with miphy_pdsch_modulate_precoded_batch and
 * miphy_dmrs_pdsch_map_precoded_batch in the middle -- the same matrices for the data and its DM-RS, the two scalings of the one-layer
 * processor. mapped.layers.ports is ignored: antenna port a is grid port precoding.ports[a]. PDUs, lists and weights are host memory; every
 * PDU, list and precoding is checked before anything is enqueued or allocated. Still out: precoding of two codewords (they go, without
 * precoding, through miphy_pdsch_process_codewords_batch), a prepared plan, device-resident PDUs. */
typedef struct {
  miphy_pdsch_mapped_pdu mapped;
  miphy_precoding        precoding; /* precoding.nof_layers = mapped.layers.nof_layers */
} miphy_pdsch_precoded_pdu;
int miphy_pdsch_process_precoded_batch(miphy_ctx* ctx, const miphy_pdsch_precoded_pdu* pdus /* host */, uint32_t n, const uint16_t* prb_lists /* host */,
                                       uint32_t nof_list_entries, const float* weights /* host cf_t */, uint32_t nof_weights,
                                       const uint8_t* tb_in /* device */, float* grid /* device cf_t; only the mapped REs are written */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PDCCH processor (whole PDUs)  --  replaces srsran::pdcch_processor::process after the CCE-to-PRB mapping
 *   include/srsran/phy/upper/channel_processors/pdcch_processor.h:41-152, lib/phy/upper/channel_processors/pdcch_processor_impl.cpp:65-117,
 *   pdcch_modulator_impl.cpp:30-91, lib/phy/upper/signal_processors/dmrs_pdcch_processor_impl.cpp:30-101, dmrs_helper.h:44-96
 * DCI payload -> resource-grid REs in one call: pdcch_encoder (CRC24C with the RNTI mask, interleaver, polar code, E = 108 x
 * aggregation level), scrambling with c_init = (n_rnti << 16) + n_id_data, QPSK, scaling 10^(data_power_offset_dB / 20), mapping on
 * REs {0,2,3,4,6,7,8,10,11} of the PRBs of `rb_mask` over `duration` symbols (symbol by symbol, ascending subcarrier), and the DM-RS
 * of every symbol (c_init from slot, symbol and n_id_dmrs; three pilots per PRB on REs 1, 5, 9, sequence counted from the
 * reference point, amplitude 10^(dmrs_power_offset_dB / 20) / sqrt(2)). rb_mask is the result of the reference's CCE-to-PRB
 * mapping (pdcch_processor_impl::compute_rb_mask, host bookkeeping that stays with the caller). Normal cyclic prefix, one port. */
typedef struct {
  uint32_t slot_in_frame;         /* pdu.slot.slot_index() */
  uint32_t rnti;                  /* dci.rnti: CRC mask */
  uint32_t n_id_pdcch_data;
  uint32_t n_rnti;
  uint32_t n_id_pdcch_dmrs;
  uint32_t reference_point_k_rb;  /* bwp_start_rb for CORESET 0, else 0 (pdcch_processor_impl.cpp:98-99) */
  float    data_power_offset_dB;
  float    dmrs_power_offset_dB;
  uint16_t payload_size;          /* 12..128 bits */
  uint8_t  aggregation_level;     /* 1, 2, 4, 8 or 16 */
  uint8_t  start_symbol;          /* coreset.start_symbol_index */
  uint8_t  duration;              /* 1..3 */
  uint8_t  port;                  /* grid port */
  uint16_t grid_nof_prb;
  uint64_t rb_mask[5];            /* 6 x aggregation_level / duration PRBs */
  uint64_t payload_offset;        /* byte offset of the payload bits (one per byte) inside `payloads` */
  uint64_t grid_offset;           /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
  uint64_t work_offset;           /* set by the library */
} miphy_pdcch_pdu;

int miphy_pdcch_process_batch(miphy_ctx* ctx, const miphy_pdcch_pdu* pdus /* host */, uint32_t n, const uint8_t* payloads /* device */,
                              float* grid /* device cf_t; only the mapped REs are written */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PBCH encoder  --  replaces srsran::pbch_encoder::encode
 *   include/srsran/phy/upper/channel_processors/pbch_encoder.h:53-80, lib/phy/upper/channel_processors/pbch_encoder_impl.cpp:41-190
 * (payload interleaving G(j) with SFN / half-frame / SSB-index bits, Gold-sequence scrambling, CRC24C, CRC interleaver,
 * polar chain K = 56, E = 864). The 32-bit payload generation and scrambling are bit bookkeeping done on the host; CRC,
 * interleaving and the polar chain run on the device. msgs: host array; out: n x 864 bytes (one bit per byte), device. */
typedef struct {
  uint32_t N_id;        /* physical cell identifier */
  uint32_t ssb_idx;
  uint32_t L_max;       /* 4, 8 or 64 */
  uint32_t hrf;         /* half-frame flag */
  uint32_t sfn;
  uint32_t k_ssb;
  uint8_t  payload[32]; /* one bit per byte (only the first 24 are used, like the reference) */
} miphy_pbch_msg;

int miphy_pbch_encode_batch(miphy_ctx* ctx, const miphy_pbch_msg* msgs /* host */, uint32_t n, uint8_t* out /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * SS/PBCH block processor  --  replaces srsran::ssb_processor::process after the position look-up
 *   include/srsran/phy/upper/channel_processors/ssb_processor.h:41-80, lib/phy/upper/channel_processors/ssb_processor_impl.cpp:30-106,
 *   pbch_modulator_impl.cpp:28-113, lib/phy/upper/signal_processors/dmrs_pbch_processor_impl.cpp:28-100, pss_processor_impl.cpp:28-91,
 *   sss_processor_impl.cpp:28-119
 * One call: PBCH encoding (miphy_pbch_encode_batch), scrambling with the cell identity advanced by (ssb_idx & 7) * 864, QPSK on the
 * 432 PBCH REs, the 144 PBCH DM-RS (c_init from ssb_idx / half frame / cell identity, +-1/sqrt(2)), PSS (127 REs, amplitude
 * 10^(beta_pss / 20)) and SSS, written to every listed port. ssb_first_symbol / ssb_first_subcarrier are the reference's
 * ssb_get_l_first() % 14 and ssb_get_k_first() (include/srsran/ran/ssb_mapping.h), host bookkeeping that stays with the caller. */
typedef struct {
  miphy_pbch_msg msg;             /* N_id = physical cell identity, ssb_idx, L_max, hrf, sfn, k_ssb, payload */
  uint32_t ssb_first_subcarrier;
  uint32_t ssb_first_symbol;      /* 0..10 */
  float    beta_pss_dB;
  uint16_t grid_nof_prb;
  uint8_t  nof_ports;             /* 1..4 */
  uint8_t  ports[4];
  uint8_t  pad;
  uint64_t grid_offset;           /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
} miphy_ssb_pdu;

int miphy_ssb_process_batch(miphy_ctx* ctx, const miphy_ssb_pdu* pdus /* host */, uint32_t n, float* grid /* device cf_t; only the SSB REs are written */,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * NZP-CSI-RS generator  --  replaces srsran::nzp_csi_rs_generator::map after the pattern look-up
 *   include/srsran/phy/upper/signal_processors/nzp_csi_rs_generator.h:37-91, lib/phy/upper/signal_processors/nzp_csi_rs_generator_impl.cpp:34-296
 * Per port and OFDM symbol of its pattern: Gold sequence with c_init = (2^10 (14 n_slot + l + 1)(2 n_id + 1) + n_id) mod 2^31, the
 * elements below the first occupied PRB skipped (:69-108), QPSK of amplitude `amplitude` / sqrt(2), the CDM weights w_t[l'] w_f[k']
 * of the port's index in its CDM group (:34-57, 223-296), written to the REs of the port's pattern inside [start_rb, start_rb + nof_rb).
 * The per-port patterns (rb_begin / rb_end / rb_stride, RE mask, symbol mask) are the output of the reference's get_csi_rs_pattern()
 * (TS 38.211 Table 7.4.1.5.3-1 bookkeeping, include/srsran/ran/csi_rs/csi_rs_pattern.h), which stays with the caller. */
typedef struct {
  uint32_t slot_in_frame;
  uint32_t scrambling_id;
  float    amplitude;
  uint16_t start_rb;
  uint16_t nof_rb;
  uint16_t rb_begin;       /* csi_rs_pattern */
  uint16_t rb_end;
  uint16_t rb_stride;
  uint16_t grid_nof_prb;
  uint8_t  mapping_row;    /* csi_rs_mapping_table_row (only row 2 changes the sequence offset) */
  uint8_t  cdm;            /* csi_rs_cdm_type: 0 none, 1 FD-CDM2, 2 CDM4-FD2-TD2, 3 CDM8-FD2-TD4 */
  uint8_t  freq_density;   /* csi_rs_freq_density_type: 0 0.5 even PRBs, 1 0.5 odd PRBs, 2 one, 3 three */
  uint8_t  nof_ports;      /* 1..16 */
  uint8_t  ports[16];      /* grid port of each CSI-RS port */
  uint16_t re_mask[16];    /* csi_rs_pattern_port::re_mask, bit k = subcarrier k of the PRB */
  uint16_t symbol_mask[16];
  uint64_t grid_offset;    /* cf_t offset of grid port 0: [port][14][grid_nof_prb*12] */
} miphy_csi_rs_job;

int miphy_csi_rs_map_batch(miphy_ctx* ctx, const miphy_csi_rs_job* jobs, int jobs_on_device, uint32_t n, float* grid /* device cf_t */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Polar successive-cancellation LIST decoder (list size 1, 2, 4 or 8), optionally CRC-aided  --  no counterpart in the
 * reference (its polar_decoder is the list-size-1 SSC decoder that miphy_polar_decode_batch reproduces bit for bit); this
 * is the SCL-8 path BASELINE.json's north_star / configs[3] ask for. Same rate-dematcher and LLR algebra as the reference;
 * path metric PM += |llr| whenever a decision disagrees with the hard decision; candidates ranked by (metric, 2*slot+flip).
 *   crc_mode 0: msg_out = K bits of the best-metric path in K-set order (the format of miphy_polar_decode_batch);
 *   crc_mode 1: PDCCH -- every surviving path is CRC de-interleaved (TS 38.212 5.3.1.1) and checked with CRC24C over 24
 *               leading ones + payload and the RNTI mask (pdcch_encoder_impl.cpp:33-59 inverted); the best-metric path that
 *               passes wins; msg_out = the K de-interleaved bits (payload then masked CRC), crc_ok_out = 1 on a pass;
 *   crc_mode 2: PBCH -- the same without leading ones / RNTI.
 * rnti may be NULL unless crc_mode == 1. Bit-exact against oracle/phy_oracle.c::orc_polar_scl_decode. */
int miphy_polar_decode_list_batch(miphy_ctx* ctx, const miphy_polar_code* code, uint32_t list_size, uint32_t crc_mode, uint32_t n,
                                  const int8_t* llr /* device, n x E */, const uint16_t* rnti /* device, n */,
                                  uint8_t* msg_out /* device, n x K */, uint8_t* crc_ok_out /* device, n */,
                                  int32_t* metric_out /* device, n; may be NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Open Fronthaul IQ (de)compression  --  replaces srsran::ofh::iq_decompressor::decompress and
 * srsran::ofh::iq_compressor::compress for the two methods the reference implements, compression_type::none (fixed point)
 * and compression_type::BFP (block floating point) (U-plane payloads to / from the resource grid in device memory)
 *   include/srsran/ofh/compression/iq_decompressor.h:35-52, iq_compressor.h:35-52, compressed_prb.h:36-80, compression_params.h:38-53,
 *   lib/ofh/compression/iq_compression_bfp_impl.cpp:28-143, iq_compression_bfp_avx2.cpp:31-132, iq_compression_none_impl.cpp:29-69,
 *   compressed_prb.cpp:31-79, quantizer.h:34-100, lib/srsvec/conversion.cpp:61-130
 * A job is one U-plane section: `nof_prb` consecutive PRB records as ofh_uplane_message_builder_impl.cpp:145-152 puts them on the
 * wire -- BFP: [udCompParam][24 x data_width bits, big endian] (1 + 3 * data_width bytes), none: the 3 * data_width bytes of
 * samples only -- and the nof_prb * 12 subcarriers of one (port, symbol) row of a resource grid they belong to.
 * Decompression: BFP sample = sign_extend(bits) * 2^(udCompParam & 15) / 32767; none sample = sign_extend(bits) / (2^(w-1) - 1).
 * `simd_arithmetic` != 0 reproduces the reference's production BFP classes ("avx2" / "avx512": data_width 9 multiplies by the
 * rounded reciprocal 1 / (32767 / 2^e)), 0 its generic class (a division for every width); both bit for bit. (For 9-bit samples
 * and exponents 0..7 the two forms give the same single-precision value, tests/test_oracle_golden.py checks that exhaustively;
 * the switch only matters for exponents a compliant RU does not send.)
 * Compression (data_width 8..16; the reference's packing asserts below that): quantisation through srsvec::convert_round exactly
 * (round to nearest even with saturation for the SIMD part of the converted span, round-half-away with a wrapping conversion for
 * its tail: BFP converts the whole job with scale 32767 * iq_scaling and 16-bit range, so the tail is the last 24 * nof_prb mod 16
 * values; none converts PRB by PRB with scale (2^(w-1) - 1) * iq_scaling, so the tail is the last 8 values of every PRB), then for
 * BFP the exponent from the largest magnitude of the PRB and an arithmetic shift, then packing of the low data_width bits. */
enum { MIPHY_OFH_COMPRESSION_NONE = 0, MIPHY_OFH_COMPRESSION_BFP = 1 }; /* values of srsran::ofh::compression_type */

typedef struct {
  uint64_t payload_offset; /* byte offset of the first PRB record */
  uint64_t grid_offset;    /* cf_t offset of the first subcarrier */
  uint32_t nof_prb;        /* 1..275 */
  uint16_t data_width;     /* 1..16 (compression: 8..16) */
  uint16_t compression;    /* MIPHY_OFH_COMPRESSION_*; other methods -> MIPHY_EUNSUPP (the reference aborts on them) */
} miphy_ofh_iq_job;

/* Bytes of one PRB record: 3 * data_width, plus the udCompParam byte for BFP. Host function. */
uint32_t miphy_ofh_iq_record_bytes(uint32_t compression, uint32_t data_width);

int miphy_ofh_iq_decompress_batch(miphy_ctx* ctx, const miphy_ofh_iq_job* jobs, int jobs_on_device, uint32_t n, const uint8_t* payload /* device */,
                                  float* grid /* device cf_t */, int simd_arithmetic, void* stream);
int miphy_ofh_iq_compress_batch(miphy_ctx* ctx, const miphy_ofh_iq_job* jobs, int jobs_on_device, uint32_t n, const float* grid /* device cf_t */,
                                float iq_scaling, uint8_t* payload /* device */, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Device-resident HARQ softbuffer pool  --  replaces srsran::rx_softbuffer_pool / rx_softbuffer
 *   include/srsran/phy/upper/rx_softbuffer_pool.h:31-96, include/srsran/phy/upper/rx_softbuffer.h:42-72,
 *   lib/phy/upper/rx_softbuffer_pool_impl.cpp:27-69, lib/phy/upper/rx_softbuffer_impl.h:33-258
 * The pool owns the three HARQ arrays miphy_pusch_decode_batch / miphy_pusch_process_batch work on (soft bits, decoded
 * messages, codeblock CRC flags, see above) and hands out softbuffers keyed by (rnti, harq process) with the reference's
 * reservation rules and state machine:
 *   reserve:  the first softbuffer whose last identifier equals (rnti, harq_id) -- in any state -- else the first available
 *             one; fails (buffer = -1, like an invalid unique_rx_softbuffer) when that softbuffer is locked or the pool-wide
 *             codeblock budget cannot cover nof_codeblocks. A reservation with the same number of codeblocks keeps the
 *             softbuffer (and its contents); a different number returns its codeblocks to the budget first.
 *   lock / unlock / release: reserved -> locked -> reserved | released; a released softbuffer can be reserved again and is
 *             freed by the next run_slot.
 *   run_slot: frees released softbuffers and reserved ones whose expiry slot (reservation slot + expire_timeout_slots,
 *             modulo nof_slots_wrap, compared like slot_point) is <= slot.
 * The pool never touches the contents. Every softbuffer owns a fixed extent of max_codeblocks_per_buffer codeblock slots
 * (first_cb = buffer * max_codeblocks_per_buffer: the `harq_cb_index` of the transport-block descriptors), so reservations
 * never fragment; max_nof_codeblocks is enforced as a budget exactly like the reference's codeblock pool. Device memory:
 * max_softbuffers * max_codeblocks_per_buffer * (66*384 + 1056 + 1) bytes. Thread safe (one mutex, like the reference).
 * ctx == NULL creates a bookkeeping-only pool without device arrays (miphy_harq_pool_arrays then fails). */
typedef struct miphy_harq_pool miphy_harq_pool;

typedef struct {
  uint32_t max_softbuffers;           /* rx_softbuffer_pool_config::max_softbuffers */
  uint32_t max_nof_codeblocks;        /* rx_softbuffer_pool_config::max_nof_codeblocks (budget over all softbuffers) */
  uint32_t expire_timeout_slots;      /* rx_softbuffer_pool_config::expire_timeout_slots */
  uint32_t nof_slots_wrap;            /* period of the slot counter: 10240 << numerology (slot_point.h:122) */
  uint32_t max_codeblocks_per_buffer; /* extent of one softbuffer; 0 = 52 (MAX_NOF_SEGMENTS, codeblock_metadata.h:88) */
} miphy_harq_pool_config;

enum { MIPHY_HARQ_AVAILABLE = 0, MIPHY_HARQ_RESERVED = 1, MIPHY_HARQ_LOCKED = 2, MIPHY_HARQ_RELEASED = 3 };

typedef struct {
  uint32_t state; /* MIPHY_HARQ_* */
  uint32_t rnti;
  uint32_t harq_id;
  uint32_t nof_codeblocks;
  uint32_t first_cb;
  uint32_t expire_slot;
} miphy_harq_buffer_info;

int  miphy_harq_pool_create(miphy_ctx* ctx, const miphy_harq_pool_config* cfg, miphy_harq_pool** out);
void miphy_harq_pool_destroy(miphy_harq_pool* pool);
/* *buffer = softbuffer index or -1 (no softbuffer: the caller drops the transmission, as the reference does). */
int miphy_harq_pool_reserve(miphy_harq_pool* pool, uint32_t slot, uint32_t rnti, uint32_t harq_id, uint32_t nof_codeblocks,
                            int32_t* buffer, uint32_t* first_cb);
int miphy_harq_pool_lock(miphy_harq_pool* pool, int32_t buffer);    /* MIPHY_EINVAL unless reserved (reference: assertion) */
int miphy_harq_pool_unlock(miphy_harq_pool* pool, int32_t buffer);  /* locked -> reserved, otherwise no effect */
int miphy_harq_pool_release(miphy_harq_pool* pool, int32_t buffer); /* MIPHY_EINVAL unless reserved or locked */
int miphy_harq_pool_run_slot(miphy_harq_pool* pool, uint32_t slot);
int miphy_harq_pool_info(miphy_harq_pool* pool, int32_t buffer, miphy_harq_buffer_info* out);
/* Remaining codeblock budget. */
int miphy_harq_pool_free_codeblocks(miphy_harq_pool* pool, uint32_t* out);
/* The device arrays to pass as harq_softbits / harq_msgs / harq_crc_ok. */
int miphy_harq_pool_arrays(miphy_harq_pool* pool, int8_t** softbits, uint8_t** msgs, uint8_t** crc_ok);

#ifdef __cplusplus
}
#endif
#endif /* MIPHY_H */
