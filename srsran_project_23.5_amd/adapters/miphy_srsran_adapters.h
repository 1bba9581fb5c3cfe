// Host-side adapters: implement srsRAN_Project 23.5's own abstract interfaces on top of the miphy C ABI, so that the
// reference's factories / processors can use the MI355X path as a drop-in.
//
// Each class derives from the reference interface it replaces and forwards ONE call as a batch of one: spans in, H2D copy,
// kernel(s), D2H copy, spans out -- same argument meaning, same results, `report_fatal_error` where the reference would
// assert. They are deliberately thin: throughput comes from the batched C ABI (include/miphy.h), which the slot-level
// callers should use directly; the adapters exist so that every existing call site keeps compiling and keeps its tests.
//
// This header needs the reference's include/ directory and <hip/hip_runtime_api.h>; it is header-only and is compiled by
// whoever integrates it (the reference's build, or oracle/build_ref.sh for the drop-in test).
#pragma once

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include "miphy.h"
#include "srsran/ofh/compression/iq_compressor.h"
#include "srsran/ofh/compression/iq_decompressor.h"
#include "srsran/phy/generic_functions/generic_functions_factories.h"
#include "srsran/phy/lower/modulation/modulation_factories.h"
#include "srsran/phy/support/resource_grid.h"
#include "srsran/phy/upper/channel_coding/channel_coding_factories.h"
#include "srsran/phy/upper/channel_estimation.h"
#include "srsran/phy/support/resource_grid_context.h"
#include "srsran/phy/upper/channel_processors/channel_processor_factories.h"
#include "srsran/phy/upper/downlink_processor.h"
#include "srsran/phy/upper/equalization/equalization_factories.h"
#include "srsran/phy/upper/precoding/precoding_factories.h"
#include "srsran/phy/upper/resource_grid_mapper.h"
#include "srsran/phy/upper/upper_phy_rg_gateway.h"
#include "srsran/ran/csi_rs/csi_rs_pattern.h"
#include "srsran/ran/pdcch/cce_to_prb_mapping.h"
#include "srsran/ran/pucch/pucch_info.h"
#include "srsran/ran/pusch/ulsch_info.h"
#include "srsran/ran/ssb_mapping.h"
#include "srsran/ran/prach/prach_preamble_information.h"
#include "srsran/ran/precoding/precoding_codebooks.h"
#include "srsran/phy/upper/rx_softbuffer.h"
#include "srsran/phy/upper/rx_softbuffer_pool.h"
#include "srsran/phy/upper/unique_rx_softbuffer.h"
#include "srsran/phy/upper/uplink_processor.h"
#include "srsran/phy/upper/upper_phy_rx_results_notifier.h"
#include "srsran/phy/upper/signal_processors/nzp_csi_rs_generator.h"
#include "srsran/phy/upper/signal_processors/port_channel_estimator.h"
#include "srsran/phy/upper/signal_processors/signal_processor_factories.h"
#include "srsran/support/error_handling.h"
#include "srsran/support/math_utils.h"
#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstring>
#include <hip/hip_runtime_api.h>
#include <memory>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace miphy {

/// Precondition that also holds in release builds (srsran_assert compiles out): report_fatal_error when it fails.
template <typename... Args>
inline void require(bool condition, const char* fmtstr, Args&&... args)
{
  if (!condition) {
    srsran::report_fatal_error(fmtstr, std::forward<Args>(args)...);
  }
}

// ---------------------------------------------------------------------------------------------------------------- context
/// Owns a miphy context, a stream and a growable pair of device buffers used as staging by the per-call adapters.
class context
{
public:
  explicit context(int device_ = 0) : device(device_)
  {
    check(miphy_create(device, &ctx), "miphy_create"); // makes `device` the calling thread's current device
    hip(hipStreamCreate(&stream), "hipStreamCreate");
  }
  /// Makes the context's device the current one of the calling thread. A new thread starts on device 0: every thread that
  /// drives this context (allocations in buf(), the library's workspaces, launches) has to call this first.
  void bind_thread() const { hip(hipSetDevice(device), "hipSetDevice"); }
  ~context()
  {
    for (auto& b : bufs) {
      (void)hipFree(b.p);
    }
    (void)hipStreamDestroy(stream);
    miphy_destroy(ctx);
  }
  context(const context&)            = delete;
  context& operator=(const context&) = delete;

  static void check(int rc, const char* what)
  {
    if (rc != MIPHY_OK) {
      srsran::report_fatal_error("{} failed ({}): {}", what, rc, miphy_last_error());
    }
  }
  static void hip(hipError_t e, const char* what)
  {
    if (e != hipSuccess) {
      srsran::report_fatal_error("{} failed: {}", what, hipGetErrorString(e));
    }
  }
  /// Device scratch buffer number \c i of at least \c bytes bytes.
  void* buf(unsigned i, size_t bytes)
  {
    if (bufs.size() <= i) {
      bufs.resize(i + 1);
    }
    if (bufs[i].n < bytes) {
      hip(hipStreamSynchronize(stream), "sync");
      (void)hipFree(bufs[i].p);
      bufs[i].n = bytes + bytes / 2 + 4096;
      hip(hipMalloc(&bufs[i].p, bufs[i].n), "hipMalloc");
    }
    return bufs[i].p;
  }
  void h2d(void* d, const void* h, size_t n) { hip(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream), "h2d"); }
  void d2h(void* h, const void* d, size_t n) { hip(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, stream), "d2h"); }
  void sync() { hip(hipStreamSynchronize(stream), "sync"); }

  miphy_ctx*  ctx    = nullptr;
  hipStream_t stream = nullptr;
  const int   device;

private:
  struct dbuf {
    void*  p = nullptr;
    size_t n = 0;
  };
  std::vector<dbuf> bufs;
};

inline uint8_t to_miphy_crc(srsran::crc_generator_poly p)
{
  switch (p) {
    case srsran::crc_generator_poly::CRC24A:
      return MIPHY_CRC24A;
    case srsran::crc_generator_poly::CRC24B:
      return MIPHY_CRC24B;
    case srsran::crc_generator_poly::CRC24C:
      return MIPHY_CRC24C;
    case srsran::crc_generator_poly::CRC16:
      return MIPHY_CRC16;
    case srsran::crc_generator_poly::CRC11:
      return MIPHY_CRC11;
    default:
      srsran::report_fatal_error("CRC polynomial not supported by the HIP path");
  }
}

inline uint8_t bg_id(srsran::ldpc_base_graph_type bg)
{
  return bg == srsran::ldpc_base_graph_type::BG1 ? 1 : 2;
}

// ---------------------------------------------------------------------------------------------------------------- LDPC
/// srsran::ldpc_decoder over miphy_ldpc_decode_batch (include/srsran/phy/upper/channel_coding/ldpc/ldpc_decoder.h:73-74).
class ldpc_decoder_hip : public srsran::ldpc_decoder
{
public:
  explicit ldpc_decoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  srsran::optional<unsigned> decode(srsran::bit_buffer&                              output,
                                    srsran::span<const srsran::log_likelihood_ratio> input,
                                    srsran::crc_calculator*                          crc,
                                    const configuration&                             cfg) override
  {
    miphy_ldpc_dec_desc d = {};
    d.bg                  = bg_id(cfg.block_conf.tb_common.base_graph);
    d.Z                   = static_cast<uint16_t>(cfg.block_conf.tb_common.lifting_size);
    d.crc_poly            = crc ? to_miphy_crc(crc->get_generator_poly()) : MIPHY_CRC_NONE;
    d.max_iter            = cfg.algorithm_conf.max_iterations;
    d.nof_filler_bits     = cfg.block_conf.cb_specific.nof_filler_bits;
    d.in_len              = input.size();
    size_t   nbytes       = (output.size() + 7) / 8;
    auto*    d_llr        = static_cast<int8_t*>(c->buf(0, input.size()));
    auto*    d_out        = static_cast<uint8_t*>(c->buf(1, nbytes + 16));
    int32_t* d_it         = reinterpret_cast<int32_t*>(d_out + ((nbytes + 7) / 8) * 8);
    c->h2d(d_llr, input.data(), input.size());
    c->h2d(d_out, output.get_buffer().data(), nbytes); // all-zero input with a CRC leaves the output untouched
    context::check(miphy_ldpc_decode_batch(c->ctx, &d, 0, 1, d_llr, d_out, d_it, nullptr, c->stream), "ldpc_decode");
    int32_t it = 0;
    c->d2h(output.get_buffer().data(), d_out, nbytes);
    c->d2h(&it, d_it, sizeof(it));
    c->sync();
    if (it > 0) {
      return static_cast<unsigned>(it);
    }
    return srsran::nullopt;
  }

private:
  std::shared_ptr<context> c;
};

/// srsran::ldpc_encoder over miphy_ldpc_encode_batch (ldpc_encoder.h:46-47).
class ldpc_encoder_hip : public srsran::ldpc_encoder
{
public:
  explicit ldpc_encoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void encode(srsran::span<uint8_t>                                 output,
              srsran::span<const uint8_t>                           input,
              const srsran::codeblock_metadata::tb_common_metadata& cfg) override
  {
    miphy_ldpc_enc_desc d = {};
    d.bg                  = bg_id(cfg.base_graph);
    d.Z                   = static_cast<uint16_t>(cfg.lifting_size);
    d.out_len             = output.size();
    auto* d_in            = static_cast<uint8_t*>(c->buf(0, input.size()));
    auto* d_out           = static_cast<uint8_t*>(c->buf(1, output.size()));
    c->h2d(d_in, input.data(), input.size());
    context::check(miphy_ldpc_encode_batch(c->ctx, &d, 0, 1, d_in, d_out, c->stream), "ldpc_encode");
    c->d2h(output.data(), d_out, output.size());
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

inline miphy_ldpc_rdm_desc make_rdm_desc(const srsran::codeblock_metadata& cfg, unsigned block_length, unsigned E, bool new_data)
{
  miphy_ldpc_rdm_desc d = {};
  // The reference infers the base graph from the block length (ldpc_rate_matcher_impl.cpp:68-80).
  d.bg = (block_length % 66 == 0) ? 1 : 2;
  d.Z  = static_cast<uint16_t>(block_length / (d.bg == 1 ? 66 : 50));
  d.rv = cfg.tb_common.rv;
  d.mod             = srsran::get_bits_per_symbol(cfg.tb_common.mod);
  d.new_data        = new_data;
  d.nof_filler_bits = cfg.cb_specific.nof_filler_bits;
  d.Nref            = cfg.tb_common.Nref;
  d.E               = E;
  return d;
}

/// srsran::ldpc_rate_matcher over miphy_ldpc_rate_match_batch (ldpc_rate_matcher.h:46).
class ldpc_rate_matcher_hip : public srsran::ldpc_rate_matcher
{
public:
  explicit ldpc_rate_matcher_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void rate_match(srsran::span<uint8_t> output, srsran::span<const uint8_t> input, const srsran::codeblock_metadata& cfg) override
  {
    miphy_ldpc_rdm_desc d = make_rdm_desc(cfg, input.size(), output.size(), true);
    auto* d_in  = static_cast<uint8_t*>(c->buf(0, input.size()));
    auto* d_out = static_cast<uint8_t*>(c->buf(1, output.size()));
    c->h2d(d_in, input.data(), input.size());
    context::check(miphy_ldpc_rate_match_batch(c->ctx, &d, 0, 1, d_in, d_out, c->stream), "ldpc_rate_match");
    c->d2h(output.data(), d_out, output.size());
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

/// srsran::ldpc_rate_dematcher over miphy_ldpc_rate_dematch_batch (ldpc_rate_dematcher.h:52-55).
class ldpc_rate_dematcher_hip : public srsran::ldpc_rate_dematcher
{
public:
  explicit ldpc_rate_dematcher_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void rate_dematch(srsran::span<srsran::log_likelihood_ratio>       output,
                    srsran::span<const srsran::log_likelihood_ratio> input,
                    bool                                             new_data,
                    const srsran::codeblock_metadata&                cfg) override
  {
    miphy_ldpc_rdm_desc d = make_rdm_desc(cfg, output.size(), input.size(), new_data);
    auto* d_in  = static_cast<int8_t*>(c->buf(0, input.size()));
    auto* d_out = static_cast<int8_t*>(c->buf(1, output.size()));
    c->h2d(d_in, input.data(), input.size());
    c->h2d(d_out, output.data(), output.size()); // in/out: the soft buffer content is combined or partially kept
    context::check(miphy_ldpc_rate_dematch_batch(c->ctx, &d, 0, 1, d_in, d_out, nullptr, c->stream), "ldpc_rate_dematch");
    c->d2h(output.data(), d_out, output.size());
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- SCH
/// srsran::pdsch_encoder over miphy_pdsch_encode_batch (pdsch_encoder.h:54).
class pdsch_encoder_hip : public srsran::pdsch_encoder
{
public:
  explicit pdsch_encoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void encode(srsran::span<uint8_t> codeword, srsran::span<const uint8_t> transport_block, const srsran::segmenter_config& cfg) override
  {
    miphy_pdsch_tb_desc d = {};
    d.bg                  = bg_id(cfg.base_graph);
    d.rv                  = cfg.rv;
    d.mod                 = srsran::get_bits_per_symbol(cfg.mod);
    d.nof_layers          = cfg.nof_layers;
    d.Nref                = cfg.Nref;
    d.nof_ch_symbols      = cfg.nof_ch_symbols;
    d.tb_bytes            = transport_block.size();
    auto* d_tb            = static_cast<uint8_t*>(c->buf(0, transport_block.size() + 16));
    auto* d_cw            = static_cast<uint8_t*>(c->buf(1, codeword.size()));
    c->h2d(d_tb, transport_block.data(), transport_block.size());
    context::check(miphy_pdsch_encode_batch(c->ctx, &d, 1, d_tb, d_cw, c->stream), "pdsch_encode");
    c->d2h(codeword.data(), d_cw, codeword.size());
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- HARQ softbuffer pool
/// A softbuffer of the device-resident pool (miphy_harq_pool). pusch_decoder_hip and pusch_processor_hip recognise it and work
/// on the device arrays in place: no HARQ state crosses PCIe. The host accessors of srsran::rx_softbuffer still work, so that
/// a CPU block can be handed the same softbuffer: they download the codeblock into a host mirror, and everything handed out
/// is written back to the device before the next device use and when the softbuffer is unlocked or released.
class rx_softbuffer_hip : public srsran::unique_rx_softbuffer::softbuffer
{
public:
  static constexpr size_t CBS = 66 * 384, MSG = 1056;

  rx_softbuffer_hip(std::shared_ptr<context> c, miphy_harq_pool* pool, int32_t index) : c(std::move(c)), pool(pool), index(index)
  {
    context::check(miphy_harq_pool_arrays(pool, &d_soft, &d_msgs, &d_crc), "harq_pool_arrays");
  }
  unsigned get_nof_codeblocks() const override { return info().nof_codeblocks; }
  void     reset_codeblocks_crc() override
  {
    const miphy_harq_buffer_info i = info();
    crc_out                        = false;
    context::hip(hipMemsetAsync(d_crc + i.first_cb, 0, i.nof_codeblocks, c->stream), "memset");
    c->sync();
  }
  srsran::span<bool> get_codeblocks_crc() override
  {
    const miphy_harq_buffer_info i = info();
    if (!crc_out) {
      crc_bytes.resize(i.nof_codeblocks);
      c->d2h(crc_bytes.data(), d_crc + i.first_cb, i.nof_codeblocks);
      c->sync();
      crc_mirror.reset(new bool[i.nof_codeblocks + 1]);
      for (unsigned k = 0; k != i.nof_codeblocks; ++k) {
        crc_mirror[k] = crc_bytes[k] != 0;
      }
      crc_out = true;
    }
    return srsran::span<bool>(crc_mirror.get(), i.nof_codeblocks);
  }
  srsran::span<srsran::log_likelihood_ratio> get_codeblock_soft_bits(unsigned codeblock_id, unsigned codeblock_size) override
  {
    const miphy_harq_buffer_info i = info();
    srsran_assert(codeblock_id < i.nof_codeblocks, "Codeblock index ({}) is out of range ({}).", codeblock_id, i.nof_codeblocks);
    srsran_assert(codeblock_size <= CBS, "Codeblock size {} exceeds maximum size {}.", codeblock_size, CBS);
    mirror& m = mirror_of(codeblock_id);
    if (!m.soft_out) {
      m.soft.resize(CBS);
      c->d2h(m.soft.data(), d_soft + (i.first_cb + codeblock_id) * CBS, CBS);
      c->sync();
      m.soft_out = true;
    }
    return srsran::span<srsran::log_likelihood_ratio>(m.soft).first(codeblock_size);
  }
  srsran::bit_buffer get_codeblock_data_bits(unsigned codeblock_id, unsigned data_size) override
  {
    const miphy_harq_buffer_info i = info();
    srsran_assert(codeblock_id < i.nof_codeblocks, "Codeblock index ({}) is out of range ({}).", codeblock_id, i.nof_codeblocks);
    srsran_assert(data_size <= MSG * 8, "Codeblock data size {} exceeds maximum size {}.", data_size, MSG * 8);
    mirror& m = mirror_of(codeblock_id);
    if (!m.msg_out) {
      m.msg.resize(MSG * 8);
      c->d2h(m.msg.get_buffer().data(), d_msgs + (i.first_cb + codeblock_id) * MSG, MSG);
      c->sync();
      m.msg_out = true;
    }
    return m.msg.first(data_size);
  }
  void lock() override { context::check(miphy_harq_pool_lock(pool, index), "harq_pool_lock"); }
  void unlock() override
  {
    flush();
    context::check(miphy_harq_pool_unlock(pool, index), "harq_pool_unlock");
  }
  void release() override
  {
    flush();
    context::check(miphy_harq_pool_release(pool, index), "harq_pool_release");
  }

  /// Writes back whatever the host accessors handed out since the last flush (a CPU block may have modified it).
  void flush()
  {
    const miphy_harq_buffer_info i    = info();
    bool                         any  = false;
    for (size_t k = 0; k != mirrors.size(); ++k) {
      if (!mirrors[k]) {
        continue;
      }
      mirror& m = *mirrors[k];
      if (m.soft_out && k < i.nof_codeblocks) {
        c->h2d(d_soft + (i.first_cb + k) * CBS, m.soft.data(), CBS);
        any = true;
      }
      if (m.msg_out && k < i.nof_codeblocks) {
        c->h2d(d_msgs + (i.first_cb + k) * MSG, m.msg.get_buffer().data(), MSG);
        any = true;
      }
      m.soft_out = m.msg_out = false;
    }
    if (crc_out) {
      for (size_t k = 0; k != crc_bytes.size(); ++k) {
        crc_bytes[k] = crc_mirror[k] ? 1 : 0;
      }
      c->h2d(d_crc + i.first_cb, crc_bytes.data(), std::min<size_t>(crc_bytes.size(), i.nof_codeblocks));
      any     = true;
      crc_out = false;
    }
    if (any) {
      c->sync();
    }
  }
  uint32_t first_cb() const { return info().first_cb; }
  int8_t*  softbits() const { return d_soft; }
  uint8_t* msgs() const { return d_msgs; }
  uint8_t* crc_ok() const { return d_crc; }

private:
  struct mirror {
    std::vector<srsran::log_likelihood_ratio> soft;
    srsran::dynamic_bit_buffer                msg;
    bool                                      soft_out = false, msg_out = false;
  };
  miphy_harq_buffer_info info() const
  {
    miphy_harq_buffer_info i;
    context::check(miphy_harq_pool_info(pool, index, &i), "harq_pool_info");
    return i;
  }
  // The views handed out must stay valid while other codeblocks are visited: every mirror is its own allocation.
  mirror& mirror_of(unsigned cb)
  {
    if (mirrors.size() <= cb) {
      mirrors.resize(cb + 1);
    }
    if (!mirrors[cb]) {
      mirrors[cb] = std::make_unique<mirror>();
    }
    return *mirrors[cb];
  }

  std::shared_ptr<context> c;
  miphy_harq_pool*         pool;
  int32_t                  index;
  int8_t*                  d_soft = nullptr;
  uint8_t *                d_msgs = nullptr, *d_crc = nullptr;
  std::vector<std::unique_ptr<mirror>> mirrors;
  std::vector<uint8_t>     crc_bytes;
  std::unique_ptr<bool[]>  crc_mirror;
  bool                     crc_out = false;
};

/// srsran::rx_softbuffer_pool over miphy_harq_pool (rx_softbuffer_pool.h:52-80): same reservation rules and life cycle as
/// create_rx_softbuffer_pool(config), with the codeblocks in device memory. max_codeblock_size is fixed by the device
/// layout (66 * 384 soft bits per codeblock). The slot period needs the numerology, which the reference's configuration does
/// not carry: it is taken from the first slot_point the pool sees unless given here.
class rx_softbuffer_pool_hip : public srsran::rx_softbuffer_pool
{
public:
  rx_softbuffer_pool_hip(std::shared_ptr<context> c, const srsran::rx_softbuffer_pool_config& config) : c(std::move(c)), config(config)
  {
    srsran_assert(config.max_codeblock_size <= rx_softbuffer_hip::CBS, "Codeblocks of the device pool hold {} soft bits.", rx_softbuffer_hip::CBS);
  }
  ~rx_softbuffer_pool_hip() override
  {
    buffers.clear();
    miphy_harq_pool_destroy(pool);
  }
  srsran::unique_rx_softbuffer
  reserve_softbuffer(const srsran::slot_point& slot, const srsran::rx_softbuffer_identifier& id, unsigned nof_codeblocks) override
  {
    std::lock_guard<std::mutex> lock(mutex);
    create(slot);
    int32_t  b     = -1;
    uint32_t first = 0;
    context::check(miphy_harq_pool_reserve(pool, slot.to_uint(), id.rnti, id.harq_ack_id, nof_codeblocks, &b, &first), "harq_pool_reserve");
    if (b < 0) {
      return srsran::unique_rx_softbuffer();
    }
    return srsran::unique_rx_softbuffer(*buffers[b]); // locks, like the reference
  }
  void run_slot(const srsran::slot_point& slot) override
  {
    std::lock_guard<std::mutex> lock(mutex);
    create(slot);
    context::check(miphy_harq_pool_run_slot(pool, slot.to_uint()), "harq_pool_run_slot");
  }

private:
  void create(const srsran::slot_point& slot)
  {
    if (pool != nullptr) {
      return;
    }
    miphy_harq_pool_config cfg = {};
    cfg.max_softbuffers = config.max_softbuffers, cfg.max_nof_codeblocks = config.max_nof_codeblocks;
    cfg.expire_timeout_slots = config.expire_timeout_slots, cfg.nof_slots_wrap = slot.nof_slots_per_system_frame();
    cfg.max_codeblocks_per_buffer = srsran::MAX_NOF_SEGMENTS;
    context::check(miphy_harq_pool_create(c->ctx, &cfg, &pool), "harq_pool_create");
    for (unsigned i = 0; i != config.max_softbuffers; ++i) {
      buffers.emplace_back(std::make_unique<rx_softbuffer_hip>(c, pool, static_cast<int32_t>(i)));
    }
  }

  std::shared_ptr<context>                        c;
  srsran::rx_softbuffer_pool_config               config;
  std::mutex                                      mutex;
  miphy_harq_pool*                                pool = nullptr;
  std::vector<std::unique_ptr<rx_softbuffer_hip>> buffers;
};

/// Replaces srsran::create_rx_softbuffer_pool(config).
inline std::unique_ptr<srsran::rx_softbuffer_pool> create_rx_softbuffer_pool_hip(std::shared_ptr<context> c, const srsran::rx_softbuffer_pool_config& config)
{
  return std::make_unique<rx_softbuffer_pool_hip>(std::move(c), config);
}

/// srsran::pusch_decoder over miphy_pusch_decode_batch (pusch_decoder.h:74-78). With a softbuffer of rx_softbuffer_pool_hip
/// the HARQ state is used in place in device memory; with any other rx_softbuffer (the reference's CPU pool) it is uploaded
/// before and downloaded after the call.
class pusch_decoder_hip : public srsran::pusch_decoder
{
public:
  explicit pusch_decoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void decode(srsran::span<uint8_t>                            transport_block,
              srsran::pusch_decoder_result&                    stats,
              srsran::rx_softbuffer*                           soft_codeword,
              srsran::span<const srsran::log_likelihood_ratio> llrs,
              const configuration&                             cfg) override
  {
    miphy_sch_segmentation sg;
    context::check(miphy_sch_segmentation_info(transport_block.size(), bg_id(cfg.segmenter_cfg.base_graph), &sg), "segmentation");
    srsran_assert(sg.nof_cbs == soft_codeword->get_nof_codeblocks(), "Wrong number of codeblocks.");
    const size_t CBS = 66 * 384, MSG = 1056;
    auto*        resident = dynamic_cast<rx_softbuffer_hip*>(soft_codeword);
    auto*        d_llr  = static_cast<int8_t*>(c->buf(0, llrs.size()));
    auto*        d_misc = static_cast<uint8_t*>(c->buf(3, 64 + sizeof(miphy_pusch_result) + transport_block.size() + 64));
    auto*        d_res  = reinterpret_cast<miphy_pusch_result*>(d_misc + 64);
    uint8_t*     d_tb   = d_misc + 64 + 64;
    int8_t*      d_soft = nullptr;
    uint8_t *    d_msg = nullptr, *d_crc = nullptr;
    std::vector<uint8_t> crc_h(sg.nof_cbs);
    if (resident != nullptr) {
      resident->flush();
      d_soft = resident->softbits(), d_msg = resident->msgs(), d_crc = resident->crc_ok();
    } else {
      d_soft = static_cast<int8_t*>(c->buf(1, sg.nof_cbs * CBS));
      d_msg  = static_cast<uint8_t*>(c->buf(2, sg.nof_cbs * MSG));
      d_crc  = d_misc;
      srsran::span<bool> crcs = soft_codeword->get_codeblocks_crc();
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        crc_h[i] = crcs[i] ? 1 : 0;
        auto sb  = soft_codeword->get_codeblock_soft_bits(i, sg.N);
        c->h2d(d_soft + i * CBS, sb.data(), sg.N);
        auto mb = soft_codeword->get_codeblock_data_bits(i, sg.K);
        c->h2d(d_msg + i * MSG, mb.get_buffer().data(), (sg.K + 7) / 8);
      }
      c->h2d(d_crc, crc_h.data(), sg.nof_cbs);
    }
    c->h2d(d_llr, llrs.data(), llrs.size());
    c->h2d(d_tb, transport_block.data(), transport_block.size());
    miphy_pusch_tb_desc d = {};
    d.bg                  = bg_id(cfg.segmenter_cfg.base_graph);
    d.rv                  = cfg.segmenter_cfg.rv;
    d.mod                 = srsran::get_bits_per_symbol(cfg.segmenter_cfg.mod);
    d.nof_layers          = cfg.segmenter_cfg.nof_layers;
    d.new_data            = cfg.new_data;
    d.use_early_stop      = cfg.use_early_stop;
    d.nof_ldpc_iterations = cfg.nof_ldpc_iterations;
    d.Nref                = cfg.segmenter_cfg.Nref;
    d.nof_ch_symbols      = cfg.segmenter_cfg.nof_ch_symbols;
    d.tb_bytes            = transport_block.size();
    d.harq_cb_index       = resident != nullptr ? resident->first_cb() : 0;
    context::check(miphy_pusch_decode_batch(c->ctx, &d, 1, d_llr, d_soft, d_msg, d_crc, d_tb, d_res, c->stream), "pusch_decode");
    miphy_pusch_result r;
    c->d2h(&r, d_res, sizeof(r));
    c->d2h(transport_block.data(), d_tb, transport_block.size());
    if (resident == nullptr) {
      c->d2h(crc_h.data(), d_crc, sg.nof_cbs);
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        auto sb = soft_codeword->get_codeblock_soft_bits(i, sg.N);
        c->d2h(sb.data(), d_soft + i * CBS, sg.N);
        auto mb = soft_codeword->get_codeblock_data_bits(i, sg.K);
        c->d2h(mb.get_buffer().data(), d_msg + i * MSG, (sg.K + 7) / 8);
      }
    }
    c->sync();
    if (resident == nullptr) {
      srsran::span<bool> crcs = soft_codeword->get_codeblocks_crc();
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        crcs[i] = crc_h[i] != 0;
      }
    }
    stats.tb_crc_ok            = r.tb_crc_ok != 0;
    stats.nof_codeblocks_total = r.nof_codeblocks_total;
    stats.ldpc_decoder_stats.reset();
    // min / max / count are reproduced exactly; the running mean is rebuilt from them and the device-side mean.
    if (r.nof_decoded > 0) {
      stats.ldpc_decoder_stats.update(r.iters_min);
      for (unsigned i = 1; i + 1 < r.nof_decoded; ++i) {
        stats.ldpc_decoder_stats.update(static_cast<unsigned>(r.iters_mean + 0.5F));
      }
      if (r.nof_decoded > 1) {
        stats.ldpc_decoder_stats.update(r.iters_max);
      }
    }
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- DFT
/// srsran::dft_processor over miphy_dft_batch (include/srsran/phy/generic_functions/dft_processor.h:34-73). Like the
/// reference implementations it owns its input and output buffers and hands out views.
class dft_processor_hip : public srsran::dft_processor
{
public:
  dft_processor_hip(std::shared_ptr<context> c, const configuration& cfg) : c(std::move(c)), dir(cfg.dir), in(cfg.size), out(cfg.size) {}
  direction                        get_direction() const override { return dir; }
  unsigned                         get_size() const override { return in.size(); }
  srsran::span<srsran::cf_t>       get_input() override { return in; }
  srsran::span<const srsran::cf_t> run() override
  {
    const size_t bytes = in.size() * sizeof(srsran::cf_t);
    auto*        d_in  = static_cast<float*>(c->buf(0, bytes));
    auto*        d_out = static_cast<float*>(c->buf(1, bytes));
    c->h2d(d_in, in.data(), bytes);
    context::check(miphy_dft_batch(c->ctx, in.size(), dir == direction::INVERSE, 1, d_in, d_out, c->stream), "dft");
    c->d2h(out.data(), d_out, bytes);
    c->sync();
    return out;
  }

private:
  std::shared_ptr<context>  c;
  direction                 dir;
  std::vector<srsran::cf_t> in, out;
};

class dft_processor_factory_hip : public srsran::dft_processor_factory
{
public:
  explicit dft_processor_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::dft_processor> create(const srsran::dft_processor::configuration& cfg) override
  {
    return std::make_unique<dft_processor_hip>(c, cfg);
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- OFDM
/// srsran::ofdm_slot_demodulator over miphy_ofdm_demodulate_slots (ofdm_demodulator.h:91-101).
class ofdm_slot_demodulator_hip : public srsran::ofdm_slot_demodulator
{
public:
  ofdm_slot_demodulator_hip(std::shared_ptr<context> c, const srsran::ofdm_demodulator_configuration& cfg_) : c(std::move(c))
  {
    cfg.numerology                = cfg_.numerology;
    cfg.bw_rb                     = cfg_.bw_rb;
    cfg.dft_size                  = cfg_.dft_size;
    cfg.nof_samples_window_offset = cfg_.nof_samples_window_offset;
    cfg.scale                     = cfg_.scale;
    cfg.center_freq_hz            = cfg_.center_freq_hz;
    srsran_assert(cfg_.cp == srsran::cyclic_prefix::NORMAL, "Only normal cyclic prefix is supported by the HIP path.");
  }
  unsigned get_slot_size(unsigned slot_index) const override { return miphy_ofdm_slot_size(&cfg, slot_index); }
  void demodulate(srsran::resource_grid_writer& grid, srsran::span<const srsran::cf_t> input, unsigned port_index, unsigned slot_index) override
  {
    const unsigned rg   = cfg.bw_rb * 12;
    auto*          d_in = static_cast<float*>(c->buf(0, input.size() * sizeof(srsran::cf_t)));
    auto*          d_g  = static_cast<float*>(c->buf(1, 14 * rg * sizeof(srsran::cf_t)));
    c->h2d(d_in, input.data(), input.size() * sizeof(srsran::cf_t));
    miphy_ofdm_job job = {0, 0, slot_index, 0};
    context::check(miphy_ofdm_demodulate_slots(c->ctx, &cfg, &job, 0, 1, d_in, d_g, c->stream), "ofdm_demodulate");
    host.resize(14 * rg);
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned l = 0; l != 14; ++l) {
      grid.put(port_index, l, 0, srsran::span<const srsran::cf_t>(host.data() + l * rg, rg));
    }
  }

private:
  std::shared_ptr<context>  c;
  miphy_ofdm_config         cfg = {};
  std::vector<srsran::cf_t> host;
};

/// srsran::ofdm_slot_modulator over miphy_ofdm_modulate_slots (ofdm_modulator.h:89-101).
class ofdm_slot_modulator_hip : public srsran::ofdm_slot_modulator
{
public:
  ofdm_slot_modulator_hip(std::shared_ptr<context> c, const srsran::ofdm_modulator_configuration& cfg_) : c(std::move(c))
  {
    cfg.numerology     = cfg_.numerology;
    cfg.bw_rb          = cfg_.bw_rb;
    cfg.dft_size       = cfg_.dft_size;
    cfg.scale          = cfg_.scale;
    cfg.center_freq_hz = cfg_.center_freq_hz;
    srsran_assert(cfg_.cp == srsran::cyclic_prefix::NORMAL, "Only normal cyclic prefix is supported by the HIP path.");
  }
  unsigned get_slot_size(unsigned slot_index) const override { return miphy_ofdm_slot_size(&cfg, slot_index); }
  void modulate(srsran::span<srsran::cf_t> output, const srsran::resource_grid_reader& grid, unsigned port_index, unsigned slot_index) override
  {
    const unsigned rg = cfg.bw_rb * 12;
    host.resize(14 * rg);
    miphy_ofdm_job job = {0, 0, slot_index, grid.is_empty(port_index) ? 1U : 0U};
    if (!job.grid_empty) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + l * rg, rg), port_index, l, 0);
      }
    }
    auto* d_g   = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto* d_out = static_cast<float*>(c->buf(1, output.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_ofdm_modulate_slots(c->ctx, &cfg, &job, 0, 1, d_g, d_out, c->stream), "ofdm_modulate");
    c->d2h(output.data(), d_out, output.size() * sizeof(srsran::cf_t));
    c->sync();
  }

private:
  std::shared_ptr<context>  c;
  miphy_ofdm_config         cfg = {};
  std::vector<srsran::cf_t> host;
};

/// srsran::ofdm_symbol_demodulator over miphy_ofdm_demodulate_symbols (ofdm_demodulator.h:55-74): what the lower PHY calls once per
/// received OFDM symbol and port (lib/phy/lower/processors/uplink/puxch/puxch_processor_impl.cpp:64-76). One symbol per call:
/// samples up, one transform, one row of subcarriers back into the grid before the call returns, as the interface requires.
class ofdm_symbol_demodulator_hip : public srsran::ofdm_symbol_demodulator
{
public:
  ofdm_symbol_demodulator_hip(std::shared_ptr<context> c, const srsran::ofdm_demodulator_configuration& cfg_) : c(std::move(c))
  {
    cfg.numerology                = cfg_.numerology;
    cfg.bw_rb                     = cfg_.bw_rb;
    cfg.dft_size                  = cfg_.dft_size;
    cfg.nof_samples_window_offset = cfg_.nof_samples_window_offset;
    cfg.scale                     = cfg_.scale;
    cfg.center_freq_hz            = cfg_.center_freq_hz;
    require(cfg_.cp == srsran::cyclic_prefix::NORMAL, "Only normal cyclic prefix is supported by the HIP path.");
  }
  unsigned get_symbol_size(unsigned symbol_index) const override { return miphy_ofdm_symbol_size(&cfg, symbol_index); }
  void demodulate(srsran::resource_grid_writer& grid, srsran::span<const srsran::cf_t> input, unsigned port_index, unsigned symbol_index) override
  {
    require(input.size() == get_symbol_size(symbol_index), "The input size is not consistent with the symbol size.");
    const unsigned rg   = cfg.bw_rb * 12;
    auto*          d_in = static_cast<float*>(c->buf(0, input.size() * sizeof(srsran::cf_t)));
    auto*          d_g  = static_cast<float*>(c->buf(1, rg * sizeof(srsran::cf_t)));
    c->h2d(d_in, input.data(), input.size() * sizeof(srsran::cf_t));
    miphy_ofdm_job job = {0, 0, symbol_index, 0};
    context::check(miphy_ofdm_demodulate_symbols(c->ctx, &cfg, &job, 0, 1, d_in, d_g, c->stream), "ofdm_demodulate_symbols");
    host.resize(rg);
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    grid.put(port_index, symbol_index % 14, 0, host); // the grid holds one slot (ofdm_demodulator_impl.cpp:133,137)
  }

private:
  std::shared_ptr<context>  c;
  miphy_ofdm_config         cfg = {};
  std::vector<srsran::cf_t> host;
};

/// srsran::ofdm_symbol_modulator over miphy_ofdm_modulate_symbols (ofdm_modulator.h:55-74; caller
/// lib/phy/lower/processors/downlink/pdxch/pdxch_processor_impl.cpp:76-82).
class ofdm_symbol_modulator_hip : public srsran::ofdm_symbol_modulator
{
public:
  ofdm_symbol_modulator_hip(std::shared_ptr<context> c, const srsran::ofdm_modulator_configuration& cfg_) : c(std::move(c))
  {
    cfg.numerology     = cfg_.numerology;
    cfg.bw_rb          = cfg_.bw_rb;
    cfg.dft_size       = cfg_.dft_size;
    cfg.scale          = cfg_.scale;
    cfg.center_freq_hz = cfg_.center_freq_hz;
    require(cfg_.cp == srsran::cyclic_prefix::NORMAL, "Only normal cyclic prefix is supported by the HIP path.");
  }
  unsigned get_symbol_size(unsigned symbol_index) const override { return miphy_ofdm_symbol_size(&cfg, symbol_index); }
  void modulate(srsran::span<srsran::cf_t> output, const srsran::resource_grid_reader& grid, unsigned port_index, unsigned symbol_index) override
  {
    require(output.size() == get_symbol_size(symbol_index), "The output size is not consistent with the symbol size.");
    const unsigned rg = cfg.bw_rb * 12;
    host.resize(rg);
    miphy_ofdm_job job = {0, 0, symbol_index, grid.is_empty(port_index) ? 1U : 0U};
    if (!job.grid_empty) {
      grid.get(host, port_index, symbol_index % 14, 0);
    }
    auto* d_g   = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto* d_out = static_cast<float*>(c->buf(1, output.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_ofdm_modulate_symbols(c->ctx, &cfg, &job, 0, 1, d_g, d_out, c->stream), "ofdm_modulate_symbols");
    c->d2h(output.data(), d_out, output.size() * sizeof(srsran::cf_t));
    c->sync();
  }

private:
  std::shared_ptr<context>  c;
  miphy_ofdm_config         cfg = {};
  std::vector<srsran::cf_t> host;
};

// ---------------------------------------------------------------------------------------------------------------- estimator
/// srsran::dmrs_pusch_estimator over miphy_dmrs_pusch_estimate_batch (dmrs_pusch_estimator.h:84). \c separate_layers: through
/// miphy_dmrs_pusch_estimate_layers_batch, which separates the layers that share a CDM group (beyond the reference, whose estimate of such a
/// layer holds the other one too); the default is the reference's arithmetic. \c compensate_cfo: through miphy_dmrs_pusch_estimate_cfo_batch,
/// which separates the layers too, estimates the carrier frequency offset from the DM-RS symbols and writes an estimate that differs from symbol to
/// symbol into the reference's channel_estimate; 23.5 has no field for the offset, so the last {cfo_hz, rho} are kept for last_cfo_hz() / last_cfo_rho().
/// \c time: what becomes of the DM-RS symbols of a slot. \c average (the default, the reference's rule) fits one channel to all of them;
/// \c interpolate and \c line go through miphy_dmrs_pusch_estimate_tv_batch, which compensates the offset too, keeps the fits of the DM-RS symbols
/// apart and blends them in time (a polygon through them, or one least-squares line) for a channel that changes within the slot; the share of the
/// DM-RS energy the average does not explain is kept for last_variation().
enum class time_strategy { average, interpolate, line };
class dmrs_pusch_estimator_hip : public srsran::dmrs_pusch_estimator
{
public:
  explicit dmrs_pusch_estimator_hip(std::shared_ptr<context> c, bool separate_layers = false, bool compensate_cfo = false,
                                    time_strategy time = time_strategy::average) :
    c(std::move(c)), separate_layers(separate_layers), compensate_cfo(compensate_cfo), time(time)
  {
  }
  /// The variation of (rx port, layer) of the last estimate() with a \c time strategy other than average (0 before the first one), and the largest
  /// of them: what a scheduler reads to tell a moving UE from a still one.
  float last_variation(unsigned port, unsigned layer) const { return port < 4 && layer < nof_var_layers ? variation[port * nof_var_layers + layer] : 0.F; }
  float last_variation() const
  {
    float v = 0.F;
    for (float x : variation)
      v = x > v ? x : v;
    return v;
  }
  /// The offset in Hz and the normalised correlation of the last estimate() with \c compensate_cfo (0 before the first one).
  float last_cfo_hz() const { return cfo[0]; }
  float last_cfo_rho() const { return cfo[1]; }
  void estimate(srsran::channel_estimate& estimate, const srsran::resource_grid_reader& grid, const configuration& config) override
  {
    srsran_assert(config.type == srsran::dmrs_type::TYPE1, "Only DM-RS type 1 is supported.");
    const unsigned nprb = config.rb_mask.size(), nsc = nprb * 12;
    const unsigned nports = config.rx_ports.size(), nl = config.nof_tx_layers, nsymb = config.first_symbol + config.nof_symbols;
    estimate.resize({nprb, nsymb, nports, nl});
    miphy_pusch_chest_job j = {};
    j.numerology            = config.slot.numerology();
    j.slot_in_frame         = config.slot.slot_index();
    j.scrambling_id         = config.scrambling_id;
    j.scaling               = config.scaling;
    j.n_scid                = config.n_scid;
    j.nof_tx_layers         = nl;
    j.nof_rx_ports          = nports;
    j.first_symbol          = config.first_symbol;
    j.nof_symbols           = config.nof_symbols;
    j.grid_nof_prb          = nprb;
    for (unsigned p = 0; p != nports; ++p) {
      j.rx_ports[p] = p; // the staging grid below is already ordered by rx_ports
    }
    for (unsigned l = 0; l != 14; ++l) {
      if (l < config.symbols_mask.size() && config.symbols_mask.test(l)) {
        j.symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    config.rb_mask.for_each(0, nprb, [&j](unsigned r) { j.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), config.rx_ports[p], l, 0);
      }
    }
    const size_t ce_n = static_cast<size_t>(nl) * nports * nsymb * nsc;
    auto*        d_g  = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto*        d_ce = static_cast<float*>(c->buf(1, ce_n * sizeof(srsran::cf_t)));
    auto*        d_sc = static_cast<float*>(c->buf(2, nports * nl * 5 * sizeof(float)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    ce_host.resize(ce_n);
    // Unallocated PRBs keep whatever the channel_estimate object holds (the reference only writes the allocation).
    for (unsigned ly = 0; ly != nl; ++ly) {
      for (unsigned p = 0; p != nports; ++p) {
        for (unsigned l = 0; l != nsymb; ++l) {
          auto v = estimate.get_symbol_ch_estimate(l, p, ly);
          std::memcpy(ce_host.data() + ((static_cast<size_t>(ly) * nports + p) * nsymb + l) * nsc, v.data(), nsc * sizeof(srsran::cf_t));
        }
      }
    }
    c->h2d(d_ce, ce_host.data(), ce_n * sizeof(srsran::cf_t));
    if (time != time_strategy::average) {
      miphy_pusch_chest_tv_job vj = {};
      vj.base.base                = j;
      vj.time_mode                = time == time_strategy::interpolate ? MIPHY_TIME_INTERPOLATE : MIPHY_TIME_LINE;
      auto* d_cfo                 = static_cast<float*>(c->buf(3, (2 + 16) * sizeof(float)));
      context::check(miphy_dmrs_pusch_estimate_tv_batch(c->ctx, &vj, 0, 1, d_g, d_ce, d_sc, d_cfo, d_cfo + 2, c->stream), "dmrs_pusch_estimate_tv");
      float out[2 + 16] = {};
      c->d2h(out, d_cfo, (2 + nports * nl) * sizeof(float));
      cfo[0] = out[0], cfo[1] = out[1];
      nof_var_layers = nl;
      for (unsigned k = 0; k != 16; ++k)
        variation[k] = k < nports * nl ? out[2 + k] : 0.F;
    } else if (compensate_cfo) {
      miphy_pusch_chest_cfo_job fj = {};
      fj.base                      = j;
      auto* d_cfo                  = static_cast<float*>(c->buf(3, 2 * sizeof(float)));
      context::check(miphy_dmrs_pusch_estimate_cfo_batch(c->ctx, &fj, 0, 1, d_g, d_ce, d_sc, d_cfo, c->stream), "dmrs_pusch_estimate_cfo");
      c->d2h(cfo, d_cfo, sizeof(cfo));
    } else {
      context::check((separate_layers ? miphy_dmrs_pusch_estimate_layers_batch : miphy_dmrs_pusch_estimate_batch)(c->ctx, &j, 0, 1, d_g, d_ce, d_sc, c->stream),
                     "dmrs_pusch_estimate");
    }
    std::vector<float> sc(nports * nl * 5);
    c->d2h(ce_host.data(), d_ce, ce_n * sizeof(srsran::cf_t));
    c->d2h(sc.data(), d_sc, sc.size() * sizeof(float));
    c->sync();
    for (unsigned ly = 0; ly != nl; ++ly) {
      for (unsigned p = 0; p != nports; ++p) {
        for (unsigned l = 0; l != nsymb; ++l) {
          auto v = estimate.get_symbol_ch_estimate(l, p, ly);
          std::memcpy(v.data(), ce_host.data() + ((static_cast<size_t>(ly) * nports + p) * nsymb + l) * nsc, nsc * sizeof(srsran::cf_t));
        }
        const float* s = sc.data() + 5 * (static_cast<size_t>(p) * nl + ly);
        estimate.set_rsrp(s[0], p, ly);
        estimate.set_epre(s[1], p, ly);
        estimate.set_noise_variance(s[2], p, ly);
        estimate.set_snr(s[3], p, ly);
        estimate.set_time_alignment(srsran::phy_time_unit::from_seconds(s[4]), p, ly);
      }
    }
  }

private:
  std::shared_ptr<context>  c;
  bool                      separate_layers, compensate_cfo;
  time_strategy             time;
  float                     cfo[2] = {0.F, 0.F}, variation[16] = {};
  unsigned                  nof_var_layers = 1;
  std::vector<srsran::cf_t> host, ce_host;
};

// ---------------------------------------------------------------------------------------------------------------- PUSCH demodulator
/// srsran::pusch_demodulator over miphy_pusch_demodulate_batch (pusch_demodulator.h:105-108): equaliser, soft demapper and
/// descrambler of pusch_demodulator_impl in one device pass. No UCI placeholders, no EVM report (status.evm stays empty). Two to four
/// transmit layers (which the reference's demodulator asserts against) go to miphy_pusch_demodulate_layers_batch.
class pusch_demodulator_hip : public srsran::pusch_demodulator
{
public:
  explicit pusch_demodulator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  demodulation_status demodulate(srsran::span<srsran::log_likelihood_ratio> codeword,
                                 const srsran::resource_grid_reader&        grid,
                                 const srsran::channel_estimate&            estimates,
                                 const configuration&                       config) override
  {
    const unsigned nl = config.nof_tx_layers;
    srsran_assert(nl >= 1 && nl <= 4 && nl <= config.rx_ports.size(), "One to four transmit layers on at least as many receive ports are supported.");
    bool has_placeholders = false;
    config.placeholders.for_each(config.modulation, config.nof_tx_layers, [&has_placeholders](unsigned, unsigned) { has_placeholders = true; });
    if (has_placeholders) {
      srsran::report_fatal_error("pusch_demodulator_hip: UCI placeholders are not supported.");
    }
    const unsigned nprb = config.rb_mask.size(), nsc = nprb * 12, nports = config.rx_ports.size();
    const unsigned nsymb = config.start_symbol_index + config.nof_symbols;
    miphy_pusch_demod_layers_job lj = {};
    lj.nof_tx_layers                = nl;
    miphy_pusch_demod_job& j        = lj.base;
    j.rnti                  = config.rnti;
    j.n_id                  = config.n_id;
    j.mod                   = srsran::get_bits_per_symbol(config.modulation);
    j.nof_rx_ports          = nports;
    j.start_symbol          = config.start_symbol_index;
    j.nof_symbols           = config.nof_symbols;
    j.dmrs_type             = (config.dmrs_config_type == srsran::dmrs_type::TYPE1) ? 1 : 2;
    j.nof_cdm_groups_without_data = config.nof_cdm_groups_without_data;
    j.ce_nof_symbols        = nsymb;
    j.grid_nof_prb          = nprb;
    for (unsigned p = 0; p != nports; ++p) {
      j.rx_ports[p] = p; // the staging grid below is already ordered by rx_ports
    }
    for (unsigned l = 0; l != 14; ++l) {
      if (config.dmrs_symb_pos[l]) {
        j.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    config.rb_mask.for_each(0, nprb, [&j](unsigned r) { j.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    j.nof_llr = codeword.size(); // validated against the allocation by the library, like pusch_demodulator_impl.cpp:76-80
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), config.rx_ports[p], l, 0);
      }
    }
    ce_host.resize(static_cast<size_t>(nl) * nports * nsymb * nsc); // [layer][rx port][symbol][subcarrier]
    for (unsigned ly = 0; ly != nl; ++ly) {
      for (unsigned p = 0; p != nports; ++p) {
        for (unsigned l = 0; l != nsymb; ++l) {
          auto v = estimates.get_symbol_ch_estimate(l, p, ly);
          std::memcpy(ce_host.data() + ((static_cast<size_t>(ly) * nports + p) * nsymb + l) * nsc, v.data(), nsc * sizeof(srsran::cf_t));
        }
      }
    }
    float sc[5] = {0, 0, estimates.get_noise_variance(0, 0), 0, 0};
    auto* d_g   = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto* d_ce  = static_cast<float*>(c->buf(1, ce_host.size() * sizeof(srsran::cf_t)));
    auto* d_sc  = static_cast<float*>(c->buf(2, sizeof(sc)));
    auto* d_llr = static_cast<int8_t*>(c->buf(3, codeword.size() + 16));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    c->h2d(d_ce, ce_host.data(), ce_host.size() * sizeof(srsran::cf_t));
    c->h2d(d_sc, sc, sizeof(sc));
    if (nl == 1) {
      context::check(miphy_pusch_demodulate_batch(c->ctx, &j, 0, 1, d_g, d_ce, d_sc, d_llr, c->stream), "pusch_demodulate");
    } else { // beyond the reference: L x P zero forcing and the layer demapping of TS 38.211 6.3.1.3
      context::check(miphy_pusch_demodulate_layers_batch(c->ctx, &lj, 0, 1, d_g, d_ce, d_sc, d_llr, c->stream), "pusch_demodulate_layers");
    }
    static_assert(sizeof(srsran::log_likelihood_ratio) == 1, "LLRs are int8");
    c->d2h(codeword.data(), d_llr, codeword.size());
    c->sync();
    return {};
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host, ce_host;
};

// ---------------------------------------------------------------------------------------------------------------- UCI decoder
/// srsran::short_block_detector over miphy_uci_decode_batch (short_block_detector.h:38-50), a batch of one: the soft bits go to the
/// device, the payload bits and the verdict come back. Invalid spans are fatal, as the reference's asserts are.
class short_block_detector_hip : public srsran::short_block_detector
{
public:
  explicit short_block_detector_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  bool detect(srsran::span<uint8_t> output, srsran::span<const srsran::log_likelihood_ratio> input, srsran::modulation_scheme mod) override
  {
    miphy_uci_field_job j = {};
    j.nof_bits = static_cast<uint8_t>(std::min<size_t>(output.size(), 255)), j.mod = static_cast<uint8_t>(srsran::get_bits_per_symbol(mod));
    j.nof_llr = static_cast<uint32_t>(input.size()), j.llr_offset = 0, j.payload_offset = 0;
    auto* d = static_cast<uint8_t*>(c->buf(5, 64 + input.size())); // [0,16) payload, [16] status, [64,..) soft bits
    c->h2d(d + 64, input.data(), input.size());
    context::check(miphy_uci_decode_batch(c->ctx, &j, 0, 1, reinterpret_cast<const int8_t*>(d + 64), d, d + 16, c->stream), "uci_decode");
    uint8_t h[17];
    c->d2h(h, d, sizeof(h));
    c->sync();
    std::copy(h, h + output.size(), output.begin());
    return h[16] == MIPHY_UCI_STATUS_VALID;
  }

private:
  std::shared_ptr<context> c;
};

/// srsran::uci_decoder on the device: fields of 1 to 11 bits are short blocks (uci_decoder_impl.cpp:41-50, all the reference decodes),
/// fields of 12 to 1706 bits are polar coded and go to miphy_uci_polar_decode_list_batch as one job per call (beyond the reference;
/// the verdict is the CRC of every segment). \c list_size 1 (the default) is the reference's SSC decoder, 2 / 4 / 8 decode the fields
/// of 20 bits and more with a CRC-aided list of that size. pusch_processor_hip recognises the decoder and decodes the UCI fields of a
/// PDU where the demultiplexer left them, in the same submission and at the decoder's list size.
class uci_decoder_hip : public srsran::uci_decoder
{
public:
  explicit uci_decoder_hip(std::shared_ptr<context> c_, unsigned list_size_ = 1) : c(c_), detector(std::move(c_)), list_size(list_size_)
  {
    require(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "The UCI list size must be 1, 2, 4 or 8.");
  }
  unsigned get_list_size() const { return list_size; }
  srsran::uci_status
  decode(srsran::span<uint8_t> message, srsran::span<const srsran::log_likelihood_ratio> llr, const configuration& config) override
  {
    require(message.size() <= MIPHY_UCI_POLAR_MAX_BITS, "UCI message lengths above 1706 bits are not supported.");
    if (message.size() <= 11) {
      return detector.detect(message, llr, config.modulation) ? srsran::uci_status::valid : srsran::uci_status::invalid;
    }
    miphy_uci_polar_job j = {};
    j.nof_bits = static_cast<uint16_t>(message.size()), j.nof_llr = static_cast<uint32_t>(llr.size()), j.llr_offset = 0, j.payload_offset = 0;
    auto* d = static_cast<uint8_t*>(c->buf(5, 2048 + llr.size())); // [0,1706) payload, [1728] status, [2048,..) soft bits
    c->h2d(d + 2048, llr.data(), llr.size());
    context::check(miphy_uci_polar_decode_list_batch(c->ctx, &j, 1, list_size, reinterpret_cast<const int8_t*>(d + 2048), d, d + 1728, c->stream),
                   "uci_polar_decode");
    uint8_t status = MIPHY_UCI_STATUS_UNKNOWN;
    c->d2h(message.data(), d, message.size());
    c->d2h(&status, d + 1728, 1);
    c->sync();
    return status == MIPHY_UCI_STATUS_VALID ? srsran::uci_status::valid : srsran::uci_status::invalid;
  }

private:
  std::shared_ptr<context> c;
  short_block_detector_hip detector;
  unsigned                 list_size;
};

// ---------------------------------------------------------------------------------------------------------------- PUCCH processor
/// srsran::pucch_processor over miphy_pucch_process_batch_ex (pucch_processor.h:160-193, pucch_processor_impl.cpp:28-189): formats 1 and 2
/// on the device, one PDU per call or a whole slot through process_batch(). A format-2 configuration above 11 bits, on which the
/// reference asserts, is decoded on the device as one polar-coded UCI field (\c list_size 1, the default, is the SSC decoder, 2 / 4 / 8
/// decode payloads of 20 bits and more with the CRC-aided list decoder) and fills the pucch_uci_message like a short payload does. A single PDU copies only its PRB window of the grid (all 14
/// symbols of its ports) into the device staging buffer; the batch copies the grid once. Formats 0, 3 and 4 go to the CPU processor
/// given at construction; without one they behave as the reference (format 0 asserts, formats 3 and 4 return an empty result).
/// Receive ports: the staging grid holds config.ports in order, so the device reads the listed ports. The reference's estimator reads
/// the listed ports too, but its format-1 detector and format-2 demodulator index the grid and the estimates by position
/// (pucch_detector_impl.cpp:264-303, pucch_demodulator_impl.cpp:93-125); the two agree only when ports[i] == i, so another list goes to
/// the CPU processor when there is one.
/// Formats 3 and 4 on the device: the reference's format3_configuration and format4_configuration hold nothing but the cyclic prefix and cannot
/// express a PDU, so those process() overrides stay as they are and process_f34_batch() takes pucch_f34_configuration records instead.
/// Format 0 on the device likewise: the reference's format0_configuration holds three fields, so process(grid, format0_configuration) stays as it is
/// and process_f0_batch() takes pucch_f0_configuration records.

/// One PUCCH format 3 or 4 PDU for pucch_processor_hip::process_f34_batch: the fields of pucch_processor::format2_configuration with their
/// meaning (\c n_id scrambles the data; there is no \c n_id_0, the DM-RS of these formats is a low-PAPR sequence) plus what the two formats add.
struct pucch_f34_configuration {
  srsran::optional<srsran::pucch_context>           context;
  srsran::slot_point                                slot;
  srsran::cyclic_prefix                             cp = srsran::cyclic_prefix::NORMAL;
  srsran::static_vector<uint8_t, srsran::MAX_PORTS> ports;
  unsigned                                          bwp_size_rb  = 0;
  unsigned                                          bwp_start_rb = 0;
  unsigned                                          starting_prb = 0;
  srsran::optional<unsigned>                        second_hop_prb;
  unsigned                                          nof_prb            = 1; ///< Format 3: 1, 3, 4, 5, 6, 8, 9, 10, 12, 15 or 16; format 4: 1.
  unsigned                                          start_symbol_index = 0;
  unsigned                                          nof_symbols        = 4; ///< 4 to 14.
  uint16_t                                          rnti               = 0;
  unsigned                                          n_id               = 0; ///< Data scrambling identity {0, ..., 1023}.
  unsigned                                          nof_harq_ack       = 0;
  unsigned                                          nof_sr             = 0;
  unsigned                                          nof_csi_part1      = 0;
  unsigned                                          nof_csi_part2      = 0; ///< Must be 0: CSI part 2 is not decoded on PUCCH.
  unsigned                                          format             = 3; ///< 3 or 4.
  bool                                              pi2_bpsk           = false;
  bool                                              additional_dmrs    = false;
  unsigned                                          occ_length         = 0; ///< Format 4: 2 or 4.
  unsigned                                          occ_index          = 0; ///< Format 4: below occ_length.
  unsigned                                          n_id_hopping       = 0; ///< Sequence group and cyclic-shift hopping identity {0, ..., 1023}.
};

/// One PUCCH format 0 PDU for pucch_processor_hip::process_f0_batch: the fields of pucch_processor::format1_configuration that apply, with their
/// meaning, plus the SR opportunity, the cyclic shifts other PDUs of the PRB may use and, optionally, a threshold and a noise variance of the caller's.
struct pucch_f0_configuration {
  srsran::optional<srsran::pucch_context>           context;
  srsran::slot_point                                slot;
  srsran::cyclic_prefix                             cp = srsran::cyclic_prefix::NORMAL;
  srsran::static_vector<uint8_t, srsran::MAX_PORTS> ports;
  unsigned                                          bwp_size_rb  = 0;
  unsigned                                          bwp_start_rb = 0;
  unsigned                                          starting_prb = 0;
  srsran::optional<unsigned>                        second_hop_prb;           ///< Two symbols only: the PRB of the second one.
  unsigned                                          start_symbol_index   = 0; ///< 0 to 13.
  unsigned                                          nof_symbols          = 1; ///< 1 or 2.
  unsigned                                          initial_cyclic_shift = 0; ///< 0 to 11.
  unsigned                                          n_id                 = 0; ///< Sequence group and cyclic-shift hopping identity {0, ..., 1023}.
  unsigned                                          nof_harq_ack         = 0; ///< 0 to 2.
  bool                                              sr_opportunity       = false;
  uint16_t                                          used_shifts_mask     = 0; ///< Bit k: some PDU of this PRB may use the cyclic shift k (before hopping).
  srsran::optional<float>                           threshold;                ///< On the metric; without it the 1 % false-alarm default.
  srsran::optional<float>                           noise_variance;           ///< Per RE; without it estimated from the free cyclic shifts.
};

class pucch_processor_hip : public srsran::pucch_processor
{
public:
  using format0_configuration = srsran::pucch_processor::format0_configuration;
  using format1_configuration = srsran::pucch_processor::format1_configuration;
  using format2_configuration = srsran::pucch_processor::format2_configuration;
  using format3_configuration = srsran::pucch_processor::format3_configuration;
  using format4_configuration = srsran::pucch_processor::format4_configuration;

  explicit pucch_processor_hip(std::shared_ptr<context> c, std::unique_ptr<srsran::pucch_processor> cpu_ = nullptr, unsigned list_size_ = 1) :
    c(std::move(c)), cpu(std::move(cpu_)), list_size(list_size_)
  {
    require(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "The UCI list size must be 1, 2, 4 or 8.");
  }
  unsigned get_list_size() const { return list_size; }

  srsran::pucch_processor_result process(const srsran::resource_grid_reader& grid, const format0_configuration& config) override
  {
    if (cpu) {
      return cpu->process(grid, config);
    }
    srsran::report_fatal_error("PUCCH Format 0 not implemented.");
  }
  srsran::pucch_processor_result process(const srsran::resource_grid_reader& grid, const format1_configuration& config) override
  {
    if (cpu && !identity_ports(config.ports)) {
      return cpu->process(grid, config);
    }
    srsran::pucch_processor_result r;
    run_one(grid, to_job(config), config.ports, r);
    return r;
  }
  srsran::pucch_processor_result process(const srsran::resource_grid_reader& grid, const format2_configuration& config) override
  {
    if (cpu && !identity_ports(config.ports)) {
      return cpu->process(grid, config);
    }
    srsran::pucch_processor_result r;
    run_one(grid, to_job(config), config.ports, r);
    return r;
  }
  srsran::pucch_processor_result process(const srsran::resource_grid_reader& grid, const format3_configuration& config) override
  {
    return cpu ? cpu->process(grid, config) : srsran::pucch_processor_result();
  }
  srsran::pucch_processor_result process(const srsran::resource_grid_reader& grid, const format4_configuration& config) override
  {
    return cpu ? cpu->process(grid, config) : srsran::pucch_processor_result();
  }

  /// A slot's PUCCH in one launch: the grid goes to the device once (the ports of the widest PDU, the PRBs up to the end of the
  /// widest BWP), every PDU is one job, results and payloads come back in one download. out1 / out2: one result per configuration.
  void process_batch(const srsran::resource_grid_reader&        grid,
                     srsran::span<const format1_configuration>  f1,
                     srsran::span<const format2_configuration>  f2,
                     srsran::span<srsran::pucch_processor_result> out1,
                     srsran::span<srsran::pucch_processor_result> out2)
  {
    require(out1.size() == f1.size() && out2.size() == f2.size(), "pucch_processor_hip::process_batch: one result per configuration.");
    const size_t n = f1.size() + f2.size();
    if (n == 0) {
      return;
    }
    std::vector<miphy_pucch_job> jobs;
    jobs.reserve(n);
    unsigned nports = 0, nprb = 0;
    auto add = [&](miphy_pucch_job j, const srsran::static_vector<uint8_t, srsran::MAX_PORTS>& ports) {
      require(identity_ports(ports), "pucch_processor_hip::process_batch: receive ports must be 0, 1, ... in order.");
      nports = std::max<unsigned>(nports, j.nof_ports), nprb = std::max<unsigned>(nprb, j.grid_nprb);
      jobs.push_back(j);
    };
    for (const auto& cfg : f1) {
      add(to_job(cfg), cfg.ports);
    }
    for (const auto& cfg : f2) {
      add(to_job(cfg), cfg.ports);
    }
    const unsigned nsc = 12 * nprb;
    for (auto& j : jobs) { // every PDU reads the first nof_ports ports of the one staged grid, whose rows are nprb PRBs wide
      j.grid_nprb = nprb;
    }
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), p, l, 0);
      }
    }
    auto* d_g = static_cast<float*>(c->buf(6, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    download(run(jobs, d_g), jobs, f1, f2, out1, out2);
  }

  /// A slot's PUCCH formats 3 and 4 in one launch of miphy_pucch_process_f34_batch (the list size of the processor decodes the payloads of 12 bits and
  /// more): the grid goes to the device once, as in process_batch(); every result gets its pucch_uci_message (HARQ-ACK, SR, CSI part 1) and the CSI
  /// exactly as process_batch() fills them for format 2. The library's rules (miphy_pucch_f34_info) are the validator: a PDU that breaks one fails the
  /// call with the rule as message before anything is enqueued.
  void process_f34_batch(const srsran::resource_grid_reader&          grid,
                         srsran::span<const pucch_f34_configuration>  configs,
                         srsran::span<srsran::pucch_processor_result> out)
  {
    require(out.size() == configs.size(), "pucch_processor_hip::process_f34_batch: one result per configuration.");
    const size_t n = configs.size();
    if (n == 0) {
      return;
    }
    std::vector<miphy_pucch_f34_job> jobs(n);
    unsigned                         nports = 0, nprb = 0;
    size_t                           pay_bytes = 0;
    for (size_t i = 0; i != n; ++i) {
      const pucch_f34_configuration& cfg = configs[i];
      require(cfg.cp == srsran::cyclic_prefix::NORMAL, "pucch_processor_hip: only the normal cyclic prefix is supported.");
      require(cfg.ports.size() >= 1 && cfg.ports.size() <= 4, "The number of receive ports must be 1 to 4.");
      require(identity_ports(cfg.ports), "pucch_processor_hip::process_f34_batch: receive ports must be 0, 1, ... in order.");
      miphy_pucch_f34_job& j = jobs[i];
      j                      = {};
      j.format = static_cast<uint8_t>(cfg.format), j.numerology = cfg.slot.numerology(), j.slot = cfg.slot.slot_index();
      j.nof_ports = static_cast<uint8_t>(cfg.ports.size()), j.start_symbol = static_cast<uint8_t>(cfg.start_symbol_index);
      j.nof_symbols = static_cast<uint8_t>(cfg.nof_symbols), j.intra_slot_hopping = cfg.second_hop_prb.has_value() ? 1 : 0;
      j.bwp_start_rb = static_cast<uint16_t>(cfg.bwp_start_rb), j.bwp_size_rb = static_cast<uint16_t>(cfg.bwp_size_rb);
      j.starting_prb   = static_cast<uint16_t>(cfg.starting_prb);
      j.second_hop_prb = static_cast<uint16_t>(cfg.second_hop_prb.has_value() ? cfg.second_hop_prb.value() : 0);
      j.nof_prb = static_cast<uint8_t>(cfg.nof_prb), j.pi2_bpsk = cfg.pi2_bpsk ? 1 : 0, j.additional_dmrs = cfg.additional_dmrs ? 1 : 0;
      j.occ_length = static_cast<uint8_t>(cfg.occ_length), j.occ_index = static_cast<uint8_t>(cfg.occ_index);
      j.nof_harq_ack = static_cast<uint16_t>(cfg.nof_harq_ack), j.nof_sr = static_cast<uint16_t>(cfg.nof_sr);
      j.nof_csi_part1 = static_cast<uint16_t>(cfg.nof_csi_part1), j.nof_csi_part2 = static_cast<uint16_t>(cfg.nof_csi_part2);
      j.n_id_hopping = static_cast<uint16_t>(cfg.n_id_hopping), j.n_id_scrambling = static_cast<uint16_t>(cfg.n_id), j.rnti = cfg.rnti;
      j.payload_offset = pay_bytes;
      pay_bytes += static_cast<size_t>(cfg.nof_harq_ack) + cfg.nof_sr + cfg.nof_csi_part1;
      nports = std::max<unsigned>(nports, j.nof_ports), nprb = std::max<unsigned>(nprb, cfg.bwp_start_rb + cfg.bwp_size_rb);
    }
    require(nprb >= 1 && nprb <= 275, "pucch_processor_hip::process_f34_batch: the BWPs must lie within 275 PRBs.");
    const unsigned nsc = 12 * nprb;
    for (auto& j : jobs) { // every PDU reads the first nof_ports ports of the one staged grid, whose rows are nprb PRBs wide
      j.grid_nprb = nprb;
    }
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), p, l, 0);
      }
    }
    auto* d_g = static_cast<float*>(c->buf(6, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    const size_t res_bytes = n * sizeof(miphy_pucch_result), bytes = res_bytes + pay_bytes;
    auto*        d         = static_cast<uint8_t*>(c->buf(7, bytes));
    context::check(miphy_pucch_process_f34_batch(c->ctx, jobs.data(), static_cast<uint32_t>(n), list_size, d_g, d + res_bytes,
                                                 reinterpret_cast<miphy_pucch_result*>(d), nullptr, nullptr, c->stream),
                   "pucch_process_f34");
    nof_run = n;
    down.resize(bytes);
    c->d2h(down.data(), d, bytes);
    c->sync();
    for (size_t i = 0; i != n; ++i) { // unpack() reads the counts and the payload offset of a format-2 job
      miphy_pucch_job j = {};
      j.format = 2, j.payload_offset = jobs[i].payload_offset;
      srsran::pucch_uci_message::configuration mc = {};
      mc.nof_harq_ack = jobs[i].nof_harq_ack, mc.nof_sr = jobs[i].nof_sr, mc.nof_csi_part1 = jobs[i].nof_csi_part1;
      unpack_message(down.data(), i, j, mc, out[i]);
    }
  }

  /// A slot's PUCCH format 0 in one launch of miphy_pucch_process_f0_batch: the grid goes to the device once, as in process_batch(); every result gets
  /// its pucch_uci_message (HARQ-ACK bits, then the SR bit of an SR opportunity), the detection metric and the CSI as process_batch() fills them for
  /// format 1. The library's rules (miphy_pucch_f0_info) are the validator: a PDU that breaks one fails the call with the rule as message before
  /// anything is enqueued.
  void process_f0_batch(const srsran::resource_grid_reader&          grid,
                        srsran::span<const pucch_f0_configuration>   configs,
                        srsran::span<srsran::pucch_processor_result> out)
  {
    require(out.size() == configs.size(), "pucch_processor_hip::process_f0_batch: one result per configuration.");
    const size_t n = configs.size();
    if (n == 0) {
      return;
    }
    std::vector<miphy_pucch_f0_job> jobs(n);
    unsigned                        nports = 0, nprb = 0;
    size_t                          pay_bytes = 0;
    for (size_t i = 0; i != n; ++i) {
      const pucch_f0_configuration& cfg = configs[i];
      require(cfg.cp == srsran::cyclic_prefix::NORMAL, "pucch_processor_hip: only the normal cyclic prefix is supported.");
      require(cfg.ports.size() >= 1 && cfg.ports.size() <= 4, "The number of receive ports must be 1 to 4.");
      require(identity_ports(cfg.ports), "pucch_processor_hip::process_f0_batch: receive ports must be 0, 1, ... in order.");
      miphy_pucch_f0_job& j = jobs[i];
      j                     = {};
      j.format = 0, j.numerology = cfg.slot.numerology(), j.slot = cfg.slot.slot_index();
      j.nof_ports = static_cast<uint8_t>(cfg.ports.size()), j.start_symbol = static_cast<uint8_t>(cfg.start_symbol_index);
      j.nof_symbols = static_cast<uint8_t>(cfg.nof_symbols), j.intra_slot_hopping = cfg.second_hop_prb.has_value() ? 1 : 0;
      j.bwp_start_rb = static_cast<uint16_t>(cfg.bwp_start_rb), j.bwp_size_rb = static_cast<uint16_t>(cfg.bwp_size_rb);
      j.starting_prb   = static_cast<uint16_t>(cfg.starting_prb);
      j.second_hop_prb = static_cast<uint16_t>(cfg.second_hop_prb.has_value() ? cfg.second_hop_prb.value() : 0);
      j.initial_cyclic_shift = static_cast<uint8_t>(cfg.initial_cyclic_shift), j.nof_harq_ack = static_cast<uint8_t>(cfg.nof_harq_ack);
      j.nof_sr = cfg.sr_opportunity ? 1 : 0, j.used_shifts_mask = cfg.used_shifts_mask, j.n_id = static_cast<uint16_t>(cfg.n_id);
      j.threshold = cfg.threshold.has_value() ? cfg.threshold.value() : 0.f;
      j.noise_var = cfg.noise_variance.has_value() ? cfg.noise_variance.value() : 0.f;
      j.payload_offset = pay_bytes;
      pay_bytes += static_cast<size_t>(cfg.nof_harq_ack) + j.nof_sr;
      nports = std::max<unsigned>(nports, j.nof_ports), nprb = std::max<unsigned>(nprb, cfg.bwp_start_rb + cfg.bwp_size_rb);
    }
    require(nprb >= 1 && nprb <= 275, "pucch_processor_hip::process_f0_batch: the BWPs must lie within 275 PRBs.");
    const unsigned nsc = 12 * nprb;
    for (auto& j : jobs) { // every PDU reads the first nof_ports ports of the one staged grid, whose rows are nprb PRBs wide
      j.grid_nprb = nprb;
    }
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), p, l, 0);
      }
    }
    auto* d_g = static_cast<float*>(c->buf(6, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    const size_t res_bytes = n * sizeof(miphy_pucch_result), bytes = res_bytes + pay_bytes;
    auto*        d         = static_cast<uint8_t*>(c->buf(7, bytes));
    context::check(miphy_pucch_process_f0_batch(c->ctx, jobs.data(), 0, static_cast<uint32_t>(n), d_g, d + res_bytes, reinterpret_cast<miphy_pucch_result*>(d),
                                                nullptr, c->stream),
                   "pucch_process_f0");
    nof_run = n;
    down.resize(bytes);
    c->d2h(down.data(), d, bytes);
    c->sync();
    for (size_t i = 0; i != n; ++i) { // unpack_message() reads the format (1: the result carries a detection metric) and the payload offset
      miphy_pucch_job j = {};
      j.format = 1, j.payload_offset = jobs[i].payload_offset;
      srsran::pucch_uci_message::configuration mc = {};
      mc.nof_harq_ack = jobs[i].nof_harq_ack, mc.nof_sr = jobs[i].nof_sr;
      unpack_message(down.data(), i, j, mc, out[i]);
    }
  }

private:
  static bool identity_ports(const srsran::static_vector<uint8_t, srsran::MAX_PORTS>& ports)
  {
    for (unsigned i = 0; i != ports.size(); ++i) {
      if (ports[i] != i) {
        return false;
      }
    }
    return true;
  }

  static miphy_pucch_job common(const srsran::slot_point& slot, srsran::cyclic_prefix cp, size_t nof_ports, unsigned start, unsigned nsym,
                                unsigned bwp_start, unsigned bwp_size)
  {
    require(cp == srsran::cyclic_prefix::NORMAL, "pucch_processor_hip: only the normal cyclic prefix is supported.");
    require(nof_ports >= 1 && nof_ports <= 4, "The number of receive ports must be 1 to 4.");
    miphy_pucch_job j = {};
    j.numerology = slot.numerology(), j.slot = slot.slot_index(), j.nof_ports = static_cast<uint8_t>(nof_ports);
    j.start_symbol = static_cast<uint8_t>(start), j.nof_symbols = static_cast<uint8_t>(nsym);
    j.bwp_start_rb = static_cast<uint16_t>(bwp_start), j.bwp_size_rb = static_cast<uint16_t>(bwp_size), j.grid_nprb = bwp_start + bwp_size;
    return j;
  }
  static miphy_pucch_job to_job(const format1_configuration& cfg)
  {
    miphy_pucch_job j = common(cfg.slot, cfg.cp, cfg.ports.size(), cfg.start_symbol_index, cfg.nof_symbols, cfg.bwp_start_rb, cfg.bwp_size_rb);
    j.format = 1, j.starting_prb = static_cast<uint16_t>(cfg.starting_prb);
    j.intra_slot_hopping = cfg.second_hop_prb.has_value() ? 1 : 0;
    j.second_hop_prb     = static_cast<uint16_t>(cfg.second_hop_prb.has_value() ? cfg.second_hop_prb.value() : 0);
    j.initial_cyclic_shift = static_cast<uint8_t>(cfg.initial_cyclic_shift), j.time_domain_occ = static_cast<uint8_t>(cfg.time_domain_occ);
    j.nof_harq_ack = static_cast<uint8_t>(cfg.nof_harq_ack), j.n_id = static_cast<uint16_t>(cfg.n_id);
    return j;
  }
  static miphy_pucch_job to_job(const format2_configuration& cfg)
  {
    miphy_pucch_job j = common(cfg.slot, cfg.cp, cfg.ports.size(), cfg.start_symbol_index, cfg.nof_symbols, cfg.bwp_start_rb, cfg.bwp_size_rb);
    j.format = 2, j.starting_prb = static_cast<uint16_t>(cfg.starting_prb), j.nof_prb = static_cast<uint8_t>(cfg.nof_prb);
    j.intra_slot_hopping = cfg.second_hop_prb.has_value() ? 1 : 0;
    j.nof_harq_ack = static_cast<uint8_t>(cfg.nof_harq_ack), j.nof_sr = static_cast<uint8_t>(cfg.nof_sr);
    j.nof_csi_part1 = static_cast<uint8_t>(cfg.nof_csi_part1), j.nof_csi_part2 = static_cast<uint8_t>(cfg.nof_csi_part2);
    j.n_id = static_cast<uint16_t>(cfg.n_id), j.n_id_0 = static_cast<uint16_t>(cfg.n_id_0), j.rnti = cfg.rnti;
    return j;
  }

  /// One PDU: only its PRB window [lo, hi) of every listed port is read from the grid and uploaded; the staged rows keep the PDU's
  /// absolute PRB numbering (the format-2 pilots depend on it), the columns outside the window are never read.
  void run_one(const srsran::resource_grid_reader& grid, miphy_pucch_job j, const srsran::static_vector<uint8_t, srsran::MAX_PORTS>& ports,
               srsran::pucch_processor_result& r)
  {
    unsigned lo = j.bwp_start_rb + j.starting_prb, hi = lo + (j.format == 2 ? j.nof_prb : 1);
    if (j.format == 1 && j.intra_slot_hopping) {
      const unsigned p2 = j.bwp_start_rb + j.second_hop_prb;
      lo = std::min(lo, p2), hi = std::max(hi, p2 + 1);
    }
    require(hi <= j.grid_nprb, "PRB allocation goes beyond the BWP.");
    const unsigned w = 12 * (hi - lo), nsc = 12 * j.grid_nprb, nports = ports.size();
    host.resize(static_cast<size_t>(nports) * 14 * w);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * w, w), ports[p], l, 12 * lo);
      }
    }
    auto* d_g = static_cast<srsran::cf_t*>(c->buf(6, static_cast<size_t>(nports) * 14 * nsc * sizeof(srsran::cf_t)));
    context::hip(hipMemcpy2DAsync(d_g + 12 * lo, nsc * sizeof(srsran::cf_t), host.data(), w * sizeof(srsran::cf_t), w * sizeof(srsran::cf_t),
                                  static_cast<size_t>(nports) * 14, hipMemcpyHostToDevice, c->stream),
                 "h2d window");
    std::vector<miphy_pucch_job> jobs{j};
    const uint8_t* h = run(jobs, reinterpret_cast<float*>(d_g));
    unpack(h, 0, jobs[0], r);
  }

  /// Launches the jobs on the staged grid and downloads results and payloads: returns the host copy, results first, then the payload
  /// bytes of the jobs one after the other from the payload_offset this function gives each job.
  const uint8_t* run(std::vector<miphy_pucch_job>& jobs, const float* d_g)
  {
    const size_t n = jobs.size(), res_bytes = n * sizeof(miphy_pucch_result);
    size_t       pay_bytes = 0;
    for (auto& j : jobs) {
      j.payload_offset = pay_bytes;
      pay_bytes += j.format == 2 ? static_cast<size_t>(j.nof_harq_ack) + j.nof_sr + j.nof_csi_part1 : j.nof_harq_ack;
    }
    const size_t bytes = res_bytes + pay_bytes;
    auto*        d     = static_cast<uint8_t*>(c->buf(7, bytes));
    context::check(miphy_pucch_process_batch_ex(c->ctx, jobs.data(), static_cast<uint32_t>(n), list_size, d_g, d + res_bytes,
                                                reinterpret_cast<miphy_pucch_result*>(d), nullptr, c->stream),
                   "pucch_process");
    nof_run = n;
    down.resize(bytes);
    c->d2h(down.data(), d, bytes);
    c->sync();
    return down.data();
  }

  void download(const uint8_t* h, const std::vector<miphy_pucch_job>& jobs, srsran::span<const format1_configuration> f1,
                srsran::span<const format2_configuration> f2, srsran::span<srsran::pucch_processor_result> out1,
                srsran::span<srsran::pucch_processor_result> out2)
  {
    for (size_t i = 0; i != jobs.size(); ++i) {
      unpack(h, i, jobs[i], i < f1.size() ? out1[i] : out2[i - f1.size()]);
    }
  }

  /// pucch_processor_result of job i (pucch_processor_impl.cpp:95-100 and 167-186).
  void unpack(const uint8_t* h, size_t i, const miphy_pucch_job& j, srsran::pucch_processor_result& r) const
  {
    srsran::pucch_uci_message::configuration mc = {};
    mc.nof_harq_ack = j.nof_harq_ack;
    if (j.format == 2) {
      mc.nof_sr = j.nof_sr, mc.nof_csi_part1 = j.nof_csi_part1, mc.nof_csi_part2 = j.nof_csi_part2;
    }
    unpack_message(h, i, j, mc, r);
  }
  /// The same for a message of the bit counts \c mc (formats 3 and 4 count in 16 bits): record i, the payload at j.payload_offset.
  void unpack_message(const uint8_t* h, size_t i, const miphy_pucch_job& j, const srsran::pucch_uci_message::configuration& mc,
                      srsran::pucch_processor_result& r) const
  {
    miphy_pucch_result res;
    std::memcpy(&res, h + i * sizeof(miphy_pucch_result), sizeof(res));
    r.message                   = srsran::pucch_uci_message(mc);
    srsran::span<uint8_t> bits  = r.message.get_full_payload();
    const uint8_t*        pay   = h + nof_run * sizeof(miphy_pucch_result) + j.payload_offset;
    std::copy(pay, pay + bits.size(), bits.begin());
    r.message.set_status(res.status == MIPHY_UCI_STATUS_VALID     ? srsran::uci_status::valid
                         : res.status == MIPHY_UCI_STATUS_INVALID ? srsran::uci_status::invalid
                                                                   : srsran::uci_status::unknown);
    r.csi.epre_dB        = res.epre_db;
    r.csi.rsrp_dB        = res.rsrp_db;
    r.csi.sinr_dB        = res.sinr_db;
    r.csi.time_alignment = srsran::phy_time_unit::from_seconds(res.time_alignment_s);
    if (j.format == 1) {
      r.detection_metric = res.detection_metric;
    } else {
      r.detection_metric.reset();
    }
  }

  std::shared_ptr<context>                 c;
  std::unique_ptr<srsran::pucch_processor> cpu;
  unsigned                                 list_size;
  size_t                                   nof_run = 0; // jobs of the last run(): the payloads follow that many result records
  std::vector<srsran::cf_t>                host;
  std::vector<uint8_t>                     down;
};

/// srsran::pucch_pdu_validator with the reference's rules (pucch_processor_impl.cpp:287-380) for the maximum channel-estimate
/// dimensions the processor is built for. Formats 0, 3 and 4 are accepted, as the reference does. \c long_payloads (off by default, the
/// reference's behaviour) lets format 2 above 11 bits through where pucch_processor_hip decodes it: no CSI part 2, the reference's
/// code-rate rule on the payload bits, and a payload the polar framing takes in the allocation's 16 nof_prb nof_symbols soft bits.
class pucch_pdu_validator_hip : public srsran::pucch_pdu_validator
{
public:
  explicit pucch_pdu_validator_hip(const srsran::channel_estimate::channel_estimate_dimensions& dims_, bool long_payloads_ = false) :
    dims(dims_), long_payloads(long_payloads_)
  {
  }
  bool is_valid(const srsran::pucch_processor::format0_configuration&) const override { return true; }
  bool is_valid(const srsran::pucch_processor::format1_configuration& config) const override
  {
    if (config.bwp_start_rb + config.bwp_size_rb > dims.nof_prb || config.starting_prb >= config.bwp_size_rb) {
      return false;
    }
    if (config.second_hop_prb.has_value() && config.second_hop_prb.value() >= config.bwp_size_rb) {
      return false;
    }
    return symbols_ok(config.cp, config.start_symbol_index, config.nof_symbols) && ports_ok(config.ports.size());
  }
  bool is_valid(const srsran::pucch_processor::format2_configuration& config) const override
  {
    const unsigned nof_uci_bits = config.nof_harq_ack + config.nof_sr + config.nof_csi_part1 + config.nof_csi_part2;
    if (config.bwp_start_rb + config.bwp_size_rb > dims.nof_prb || config.starting_prb + config.nof_prb > config.bwp_size_rb) {
      return false;
    }
    if (!symbols_ok(config.cp, config.start_symbol_index, config.nof_symbols) || !ports_ok(config.ports.size())) {
      return false;
    }
    if (config.nof_csi_part2 != 0 || config.second_hop_prb.has_value()) {
      return false;
    }
    if (srsran::pucch_format2_code_rate(config.nof_prb, config.nof_symbols, nof_uci_bits) > srsran::pucch_constants::MAX_CODE_RATE) {
      return false;
    }
    if (nof_uci_bits < srsran::pucch_constants::FORMAT2_MIN_UCI_NBITS) {
      return false;
    }
    if (nof_uci_bits <= 11) {
      return true;
    }
    miphy_uci_polar_info_t info;
    return long_payloads && miphy_uci_polar_info(nof_uci_bits, 16 * config.nof_prb * config.nof_symbols, &info) == MIPHY_OK;
  }
  bool is_valid(const srsran::pucch_processor::format3_configuration&) const override { return true; }
  bool is_valid(const srsran::pucch_processor::format4_configuration&) const override { return true; }

private:
  bool symbols_ok(srsran::cyclic_prefix cp, unsigned start, unsigned nsym) const
  {
    return start + nsym <= srsran::get_nsymb_per_slot(cp) && start + nsym <= dims.nof_symbols;
  }
  bool ports_ok(size_t nports) const { return nports != 0 && nports <= dims.nof_rx_ports; }

  srsran::channel_estimate::channel_estimate_dimensions dims;
  bool                                                  long_payloads;
};

/// srsran::pucch_processor_factory handing out pucch_processor_hip on one context; \c cpu_factory (may be null) provides the CPU
/// processor for formats 0, 3 and 4. \c list_size goes to the processors, \c long_payloads to the validators.
class pucch_processor_factory_hip : public srsran::pucch_processor_factory
{
public:
  pucch_processor_factory_hip(std::shared_ptr<context> c_, const srsran::channel_estimate::channel_estimate_dimensions& dims_,
                              std::shared_ptr<srsran::pucch_processor_factory> cpu_factory_ = nullptr, unsigned list_size_ = 1,
                              bool long_payloads_ = false) :
    c(std::move(c_)), dims(dims_), cpu_factory(std::move(cpu_factory_)), list_size(list_size_), long_payloads(long_payloads_)
  {
    require(list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8, "The UCI list size must be 1, 2, 4 or 8.");
  }
  std::unique_ptr<srsran::pucch_processor> create() override
  {
    return std::make_unique<pucch_processor_hip>(c, cpu_factory ? cpu_factory->create() : nullptr, list_size);
  }
  std::unique_ptr<srsran::pucch_pdu_validator> create_validator() override
  {
    return std::make_unique<pucch_pdu_validator_hip>(dims, long_payloads);
  }

private:
  std::shared_ptr<context>                         c;
  srsran::channel_estimate::channel_estimate_dimensions dims;
  std::shared_ptr<srsran::pucch_processor_factory> cpu_factory;
  unsigned                                         list_size;
  bool                                             long_payloads;
};

inline std::shared_ptr<srsran::pucch_processor_factory>
create_pucch_processor_factory_hip(std::shared_ptr<context> c, const srsran::channel_estimate::channel_estimate_dimensions& dims,
                                   std::shared_ptr<srsran::pucch_processor_factory> cpu_factory = nullptr, unsigned list_size = 1,
                                   bool long_payloads = false)
{
  return std::make_shared<pucch_processor_factory_hip>(std::move(c), dims, std::move(cpu_factory), list_size, long_payloads);
}

// ---------------------------------------------------------------------------------------------------------------- SRS estimator
/// The 23.5 reference has no SRS estimator, so there is no interface to derive from: srs_estimator_hip::estimate_batch() takes
/// srs_estimator_configuration records over miphy_srs_estimate_batch and returns one srs_estimator_result each.

/// One SRS resource at one frequency position in one slot (a frequency-hopping resource is one configuration per hop; the scheduler resolves the
/// position from C_SRS, B_SRS, n_shift and n_RRC).
struct srs_estimator_configuration {
  srsran::slot_point                                slot;
  srsran::cyclic_prefix                             cp = srsran::cyclic_prefix::NORMAL;
  srsran::static_vector<uint8_t, srsran::MAX_PORTS> ports;                  ///< Receive ports 0, 1, ... in order, 1 to 4.
  unsigned                                          nof_tx_ports       = 1; ///< 1, 2 or 4.
  unsigned                                          start_symbol_index = 13;
  unsigned                                          nof_symbols        = 1; ///< 1, 2 or 4.
  unsigned                                          start_prb          = 0; ///< First PRB of the allocation in the grid.
  unsigned                                          nof_prb            = 4; ///< A multiple of 4 up to 272.
  unsigned                                          comb_size          = 2; ///< 2 or 4.
  unsigned                                          comb_offset        = 0;
  unsigned                                          cyclic_shift       = 0; ///< Below 8 (comb 2) or 12 (comb 4).
  unsigned                                          n_id               = 0; ///< Sequence identity {0, ..., 1023}.
  bool                                              group_hopping      = false;
  bool                                              sequence_hopping   = false; ///< Not together with group hopping.
  unsigned                                          prg_size           = 4; ///< PRBs per channel matrix: 1, 2 or 4.
};

struct srs_estimator_result {
  unsigned                  nof_prg = 0, nof_rx_ports = 0, nof_tx_ports = 0;
  std::vector<srsran::cf_t> channel;  ///< [PRG][rx port][tx port]: the channel at the centre of each PRG, what per-PRG precoding weights are computed from.
  srsran::cf_t              wideband[4][4] = {}; ///< [rx port][tx port], delay compensated.
  float                     noise_variance = 0.f;
  float                     epre_dB        = 0.f;
  float                     rsrp_dB[4]     = {};
  float                     sinr_dB        = 0.f;
  srsran::phy_time_unit     time_alignment;
};

class srs_estimator_hip
{
public:
  explicit srs_estimator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}

  /// A slot's SRS in one launch of miphy_srs_estimate_batch: the grid goes to the device once (the ports of the widest configuration, the PRBs up to
  /// the end of the furthest allocation), estimates and records come back in one download. The library's rules (miphy_srs_info) are the validator:
  /// a configuration that breaks one fails the call with the rule as message before anything is enqueued.
  void estimate_batch(const srsran::resource_grid_reader&           grid,
                      srsran::span<const srs_estimator_configuration> configs,
                      srsran::span<srs_estimator_result>              out)
  {
    require(out.size() == configs.size(), "srs_estimator_hip::estimate_batch: one result per configuration.");
    const size_t n = configs.size();
    if (n == 0) {
      return;
    }
    std::vector<miphy_srs_job> jobs(n);
    unsigned                   nports = 0, nprb = 0;
    size_t                     nof_h = 0;
    for (size_t i = 0; i != n; ++i) {
      const srs_estimator_configuration& cfg = configs[i];
      require(cfg.cp == srsran::cyclic_prefix::NORMAL, "srs_estimator_hip: only the normal cyclic prefix is supported.");
      require(cfg.ports.size() >= 1 && cfg.ports.size() <= 4, "The number of receive ports must be 1 to 4.");
      for (unsigned p = 0; p != cfg.ports.size(); ++p) {
        require(cfg.ports[p] == p, "srs_estimator_hip::estimate_batch: receive ports must be 0, 1, ... in order.");
      }
      require(!(cfg.group_hopping && cfg.sequence_hopping), "srs_estimator_hip: group and sequence hopping exclude each other.");
      miphy_srs_job& j = jobs[i];
      j                = {};
      j.numerology = static_cast<uint8_t>(cfg.slot.numerology()), j.slot = static_cast<uint16_t>(cfg.slot.slot_index());
      j.nof_rx_ports = static_cast<uint8_t>(cfg.ports.size()), j.nof_tx_ports = static_cast<uint8_t>(cfg.nof_tx_ports);
      j.start_symbol = static_cast<uint8_t>(cfg.start_symbol_index), j.nof_symbols = static_cast<uint8_t>(cfg.nof_symbols);
      j.comb_size = static_cast<uint8_t>(cfg.comb_size), j.comb_offset = static_cast<uint8_t>(cfg.comb_offset);
      j.cyclic_shift = static_cast<uint8_t>(cfg.cyclic_shift), j.hopping = cfg.group_hopping ? 1 : (cfg.sequence_hopping ? 2 : 0);
      j.prg_size = static_cast<uint8_t>(cfg.prg_size), j.start_prb = static_cast<uint16_t>(cfg.start_prb), j.nof_prb = static_cast<uint16_t>(cfg.nof_prb);
      j.n_id = static_cast<uint16_t>(cfg.n_id), j.h_offset = nof_h;
      miphy_srs_info_t info = {};
      j.grid_nprb           = cfg.start_prb + cfg.nof_prb; // for the rules; every job then reads the one staged grid
      context::check(miphy_srs_info(&j, &info), "srs_info");
      nof_h += info.nof_h;
      nports = std::max<unsigned>(nports, j.nof_rx_ports), nprb = std::max<unsigned>(nprb, cfg.start_prb + cfg.nof_prb);
    }
    const unsigned nsc = 12 * nprb;
    for (auto& j : jobs) {
      j.grid_nprb = nprb;
    }
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), p, l, 0);
      }
    }
    auto* d_g = static_cast<float*>(c->buf(6, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    const size_t res_bytes = n * sizeof(miphy_srs_result), bytes = res_bytes + nof_h * sizeof(srsran::cf_t);
    auto*        d         = static_cast<uint8_t*>(c->buf(7, bytes));
    context::check(miphy_srs_estimate_batch(c->ctx, jobs.data(), 0, static_cast<uint32_t>(n), d_g, reinterpret_cast<float*>(d + res_bytes),
                                            reinterpret_cast<miphy_srs_result*>(d), c->stream),
                   "srs_estimate");
    down.resize(bytes);
    c->d2h(down.data(), d, bytes);
    c->sync();
    for (size_t i = 0; i != n; ++i) {
      miphy_srs_result res;
      std::memcpy(&res, down.data() + i * sizeof(miphy_srs_result), sizeof(res));
      srs_estimator_result& r = out[i];
      r.nof_rx_ports = jobs[i].nof_rx_ports, r.nof_tx_ports = jobs[i].nof_tx_ports, r.nof_prg = jobs[i].nof_prb / jobs[i].prg_size;
      r.channel.resize(static_cast<size_t>(r.nof_prg) * r.nof_rx_ports * r.nof_tx_ports);
      std::memcpy(r.channel.data(), down.data() + res_bytes + jobs[i].h_offset * sizeof(srsran::cf_t), r.channel.size() * sizeof(srsran::cf_t));
      for (unsigned rx = 0; rx != 4; ++rx) {
        for (unsigned tx = 0; tx != 4; ++tx) {
          r.wideband[rx][tx] = srsran::cf_t(res.h_wb[rx][tx][0], res.h_wb[rx][tx][1]);
        }
      }
      r.noise_variance = res.noise_var, r.epre_dB = res.epre_db, r.sinr_dB = res.sinr_db;
      std::copy(res.rsrp_db, res.rsrp_db + 4, r.rsrp_dB);
      r.time_alignment = srsran::phy_time_unit::from_seconds(res.time_alignment_s);
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host;
  std::vector<uint8_t>      down;
};

// ---------------------------------------------------------------------------------------------------------------- PRACH
static_assert(static_cast<unsigned>(srsran::prach_format_type::three) == MIPHY_PRACH_FORMAT_3 &&
                  static_cast<unsigned>(srsran::prach_format_type::A1) == MIPHY_PRACH_FORMAT_A1 &&
                  static_cast<unsigned>(srsran::prach_format_type::B4) == MIPHY_PRACH_FORMAT_B4 &&
                  static_cast<unsigned>(srsran::prach_format_type::A3_B3) == MIPHY_PRACH_FORMAT_A3_B3 &&
                  static_cast<unsigned>(srsran::prach_format_type::invalid) == MIPHY_PRACH_NOF_FORMATS,
              "MIPHY_PRACH_FORMAT_* follows srsran::prach_format_type");
static_assert(static_cast<unsigned>(srsran::prach_subcarrier_spacing::kHz120) == 3 && static_cast<unsigned>(srsran::restricted_set_config::UNRESTRICTED) == 0,
              "ra_scs and restricted_set of miphy_prach_job follow the reference's enums");

/// srsran::prach_generator over miphy_prach_generate_batch (prach_generator.h:36-58), a batch of one: the frequency-domain sequence
/// y_u,v comes back into a buffer the generator owns, valid until the next call. What the reference asserts is fatal.
class prach_generator_hip : public srsran::prach_generator
{
public:
  explicit prach_generator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  srsran::span<const srsran::cf_t> generate(const configuration& config) override
  {
    miphy_prach_gen_job j = {};
    j.format = static_cast<uint32_t>(config.format), j.root_sequence_index = config.root_sequence_index;
    j.zero_correlation_zone = config.zero_correlation_zone, j.restricted_set = static_cast<uint32_t>(config.restricted_set);
    j.preamble_index = config.preamble_index, j.out_offset = 0;
    const size_t L = srsran::is_long_preamble(config.format) ? srsran::prach_constants::LONG_SEQUENCE_LENGTH : srsran::prach_constants::SHORT_SEQUENCE_LENGTH;
    void*        d = c->buf(8, sequence.size() * sizeof(srsran::cf_t));
    context::check(miphy_prach_generate_batch(c->ctx, &j, 0, 1, static_cast<float*>(d), c->stream), "prach_generate");
    c->d2h(sequence.data(), d, L * sizeof(srsran::cf_t));
    c->sync();
    return srsran::span<const srsran::cf_t>(sequence.data(), L);
  }

private:
  std::shared_ptr<context>                                                  c;
  std::array<srsran::cf_t, srsran::prach_constants::LONG_SEQUENCE_LENGTH> sequence;
};

/// srsran::prach_detector over miphy_prach_detect_batch (prach_detector.h:37-72, prach_detector_simple_impl.cpp:35-169): one occasion
/// per call, or several buffers at once through detect_batch(). Only get_symbol(0, 0, 0, 0) of a buffer is uploaded -- the 23.5
/// detector reads nothing else. The records of every requested preamble come back and the result is assembled with the reference's
/// own phy_time_unit::from_seconds and convert_power_to_dB, detections in preamble-index order.
class prach_detector_hip : public srsran::prach_detector
{
public:
  /// \c idft_size plays the role of the reference factory's dft_size_detector (1536 in upper_phy_factories.cpp): 1536 or 3072.
  explicit prach_detector_hip(std::shared_ptr<context> c, unsigned idft_size_ = 1536) : c(std::move(c)), idft_size(idft_size_)
  {
    require(idft_size == 1536 || idft_size == 3072, "prach_detector_hip: IDFT size {} is not 1536 or 3072.", idft_size);
  }

  srsran::prach_detection_result detect(const srsran::prach_buffer& input, const configuration& config) override
  {
    const srsran::prach_buffer*    in = &input;
    srsran::prach_detection_result r;
    detect_batch(srsran::span<const srsran::prach_buffer* const>(&in, 1), srsran::span<const configuration>(&config, 1),
                 srsran::span<srsran::prach_detection_result>(&r, 1));
    return r;
  }

  /// Several occasions in one launch: one upload of their symbols, one job each, one download of the records.
  void detect_batch(srsran::span<const srsran::prach_buffer* const> inputs,
                    srsran::span<const configuration>               configs,
                    srsran::span<srsran::prach_detection_result>    out)
  {
    require(inputs.size() == configs.size() && out.size() == configs.size(), "prach_detector_hip::detect_batch: one buffer and one result per configuration.");
    const size_t n = configs.size();
    if (n == 0) {
      return;
    }
    jobs.resize(n), infos.resize(n);
    host_symbols.clear();
    uint32_t nof_records = 0;
    for (size_t i = 0; i != n; ++i) {
      const configuration& cfg = configs[i];
      require(cfg.start_preamble_index + cfg.nof_preamble_indices <= srsran::prach_constants::MAX_NUM_PREAMBLES,
              "The start preamble index {} and the number of preambles to detect {}, exceed the maximum of 64.", cfg.start_preamble_index,
              cfg.nof_preamble_indices);
      infos[i] = srsran::is_long_preamble(cfg.format) ? srsran::get_prach_preamble_long_info(cfg.format)
                                                       : srsran::get_prach_preamble_short_info(cfg.format, cfg.ra_scs, false);
      require(inputs[i]->get_sequence_length() == infos[i].sequence_length,
              "The input buffer sequence length {} is not equal to the expected preamble sequence length {}.", inputs[i]->get_sequence_length(),
              infos[i].sequence_length);
      srsran::span<const srsran::cf_t> symbol = inputs[i]->get_symbol(0, 0, 0, 0);
      miphy_prach_job&                 j      = jobs[i];
      j                                       = {};
      j.format = static_cast<uint32_t>(cfg.format), j.ra_scs = srsran::is_long_preamble(cfg.format) ? 0 : static_cast<uint32_t>(cfg.ra_scs);
      j.root_sequence_index = cfg.root_sequence_index, j.zero_correlation_zone = cfg.zero_correlation_zone;
      j.restricted_set = static_cast<uint32_t>(cfg.restricted_set), j.start_preamble_index = cfg.start_preamble_index;
      j.nof_preamble_indices = cfg.nof_preamble_indices, j.idft_size = idft_size;
      j.symbol_offset = static_cast<uint32_t>(host_symbols.size()), j.preamble_offset = nof_records;
      host_symbols.insert(host_symbols.end(), symbol.begin(), symbol.begin() + infos[i].sequence_length);
      nof_records += cfg.nof_preamble_indices;
    }
    // One device buffer: [symbols][results][preamble records], each part 16-byte aligned.
    const size_t sym_bytes = (host_symbols.size() * sizeof(srsran::cf_t) + 15) & ~size_t(15);
    const size_t res_bytes = n * sizeof(miphy_prach_result); // 16 bytes each
    const size_t rec_bytes = nof_records * sizeof(miphy_prach_preamble_result);
    auto*        d         = static_cast<uint8_t*>(c->buf(8, sym_bytes + res_bytes + rec_bytes + 16));
    c->h2d(d, host_symbols.data(), host_symbols.size() * sizeof(srsran::cf_t));
    context::check(miphy_prach_detect_batch(c->ctx, jobs.data(), 0, static_cast<uint32_t>(n), reinterpret_cast<const float*>(d),
                                            reinterpret_cast<miphy_prach_result*>(d + sym_bytes),
                                            reinterpret_cast<miphy_prach_preamble_result*>(d + sym_bytes + res_bytes), c->stream),
                   "prach_detect");
    host_out.resize(res_bytes + rec_bytes);
    c->d2h(host_out.data(), d + sym_bytes, host_out.size());
    c->sync();
    for (size_t i = 0; i != n; ++i) {
      miphy_prach_result res;
      std::memcpy(&res, host_out.data() + i * sizeof(res), sizeof(res));
      const double                    sampling_rate_Hz = static_cast<double>(srsran::ra_scs_to_Hz(infos[i].scs) * idft_size);
      srsran::prach_detection_result& r                = out[i];
      r.rssi_dB                                        = srsran::convert_power_to_dB(res.rssi);
      r.time_resolution                                = srsran::phy_time_unit::from_seconds(1.0 / sampling_rate_Hz);
      r.time_advance_max = res.n_cs_limited ? srsran::phy_time_unit::from_seconds(static_cast<double>(res.delay_n_maximum) / sampling_rate_Hz)
                                            : infos[i].cp_length;
      r.preambles.clear();
      for (unsigned k = 0; k != jobs[i].nof_preamble_indices; ++k) {
        miphy_prach_preamble_result rec;
        std::memcpy(&rec, host_out.data() + res_bytes + (jobs[i].preamble_offset + k) * sizeof(rec), sizeof(rec));
        if (!rec.detected) {
          continue;
        }
        srsran::prach_detection_result::preamble_indication& info = r.preambles.emplace_back();
        info.preamble_index                                       = jobs[i].start_preamble_index + k;
        info.time_advance = srsran::phy_time_unit::from_seconds(static_cast<double>(rec.delay_n) / sampling_rate_Hz);
        info.power_dB     = srsran::convert_power_to_dB(rec.peak_power);
        info.snr_dB       = 0.0F;
      }
    }
  }

private:
  std::shared_ptr<context>                        c;
  unsigned                                        idft_size;
  std::vector<miphy_prach_job>                    jobs;
  std::vector<srsran::prach_preamble_information> infos;
  std::vector<srsran::cf_t>                       host_symbols;
  std::vector<uint8_t>                            host_out;
};

/// srsran::prach_detector_validator for prach_detector_hip: what the reference's detector and generator assert (an unrestricted set, a
/// zone whose N_CS is not reserved, at most 64 preamble indices) and what get_prach_preamble_long_info / _short_info serve (a valid
/// format; a short format with a short RA subcarrier spacing).
class prach_detector_validator_hip : public srsran::prach_detector_validator
{
public:
  bool is_valid(const srsran::prach_detector::configuration& config) override
  {
    if (config.restricted_set != srsran::restricted_set_config::UNRESTRICTED || config.zero_correlation_zone > 15) {
      return false;
    }
    if (config.start_preamble_index + config.nof_preamble_indices > srsran::prach_constants::MAX_NUM_PREAMBLES) {
      return false;
    }
    if (srsran::is_long_preamble(config.format)) {
      return true;
    }
    return srsran::is_short_preamble(config.format) && srsran::is_short_preamble(config.ra_scs);
  }
};

/// srsran::prach_detector_factory / prach_generator_factory handing out the device blocks on one context.
class prach_detector_factory_hip : public srsran::prach_detector_factory
{
public:
  explicit prach_detector_factory_hip(std::shared_ptr<context> c_, unsigned idft_size_ = 1536) : c(std::move(c_)), idft_size(idft_size_) {}
  std::unique_ptr<srsran::prach_detector>           create() override { return std::make_unique<prach_detector_hip>(c, idft_size); }
  std::unique_ptr<srsran::prach_detector_validator> create_validator() override { return std::make_unique<prach_detector_validator_hip>(); }

private:
  std::shared_ptr<context> c;
  unsigned                 idft_size;
};

class prach_generator_factory_hip : public srsran::prach_generator_factory
{
public:
  explicit prach_generator_factory_hip(std::shared_ptr<context> c_) : c(std::move(c_)) {}
  std::unique_ptr<srsran::prach_generator> create() override { return std::make_unique<prach_generator_hip>(c); }

private:
  std::shared_ptr<context> c;
};

inline std::shared_ptr<srsran::prach_detector_factory> create_prach_detector_factory_hip(std::shared_ptr<context> c, unsigned idft_size = 1536)
{
  return std::make_shared<prach_detector_factory_hip>(std::move(c), idft_size);
}

inline std::shared_ptr<srsran::prach_generator_factory> create_prach_generator_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<prach_generator_factory_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- PRACH demodulator
static_assert(static_cast<unsigned>(srsran::subcarrier_spacing::kHz15) == 0 && static_cast<unsigned>(srsran::subcarrier_spacing::kHz120) == 3,
              "pusch_scs of miphy_prach_demod_job follows srsran::subcarrier_spacing");

/// srsran::ofdm_prach_demodulator over miphy_prach_demodulate_batch (ofdm_prach_demodulator.h:36-79,
/// ofdm_prach_demodulator_impl.cpp:31-199), a batch of one window: only the spans the transforms read (the symbols of every
/// time-domain occasion, not their cyclic prefixes nor what lies between occasions) are uploaded, one call demodulates, and the rows
/// come back into buffer.get_symbol(0, td, fd, symbol). What the reference asserts is fatal.
class ofdm_prach_demodulator_hip : public srsran::ofdm_prach_demodulator
{
public:
  ofdm_prach_demodulator_hip(std::shared_ptr<context> c, srsran::sampling_rate srate_) : c(std::move(c)), srate(srate_) {}

  void demodulate(srsran::prach_buffer& buffer, srsran::span<const srsran::cf_t> input, const configuration& config) override
  {
    miphy_prach_demod_job j = {};
    j.format = static_cast<uint32_t>(config.format), j.pusch_scs = static_cast<uint32_t>(config.pusch_scs);
    j.nof_td_occasions = config.nof_td_occasions, j.nof_fd_occasions = config.nof_fd_occasions, j.start_symbol = config.start_symbol;
    j.rb_offset = config.rb_offset, j.nof_prb_ul_grid = config.nof_prb_ul_grid, j.nof_samples = static_cast<uint32_t>(input.size());
    require(config.nof_td_occasions <= buffer.get_max_nof_td_occasions() && config.nof_fd_occasions <= buffer.get_max_nof_fd_occasions(),
            "The number of occasions ({} x {}) exceeds the buffer maximum ({} x {}).", config.nof_td_occasions, config.nof_fd_occasions,
            buffer.get_max_nof_td_occasions(), buffer.get_max_nof_fd_occasions());
    // The device copy is compact: [td][fd][symbol][L] with exactly the occasions and symbols of the configuration.
    j.max_nof_fd_occasions = config.nof_fd_occasions, j.max_nof_symbols = buffer.get_max_nof_symbols();
    miphy_prach_demod_info_t g;
    context::check(miphy_prach_demod_info(srate.to_Hz(), &j, &g), "prach_demod_info");
    require(buffer.get_sequence_length() == g.L, "The buffer sequence length {} is not the preamble's {}.", buffer.get_sequence_length(), g.L);
    j.max_nof_symbols = g.nof_symbols;
    const size_t read = static_cast<size_t>(g.nof_symbols) * g.dft_size; // samples an occasion's transforms read, behind its cyclic prefix
    size_t       last = 0;
    for (unsigned td = 0; td != config.nof_td_occasions; ++td) {
      last = std::max(last, static_cast<size_t>(g.td_sample_offset[td]) + g.td_cp_samples[td] + read);
    }
    const size_t in_bytes = (last * sizeof(srsran::cf_t) + 15) & ~size_t(15);
    const size_t rows     = static_cast<size_t>(config.nof_td_occasions) * config.nof_fd_occasions * g.nof_symbols;
    auto*        d        = static_cast<uint8_t*>(c->buf(9, in_bytes + rows * g.L * sizeof(srsran::cf_t)));
    for (unsigned td = 0; td != config.nof_td_occasions; ++td) {
      const size_t first = static_cast<size_t>(g.td_sample_offset[td]) + g.td_cp_samples[td];
      c->h2d(d + first * sizeof(srsran::cf_t), input.data() + first, read * sizeof(srsran::cf_t));
    }
    context::check(miphy_prach_demodulate_batch(c->ctx, srate.to_Hz(), &j, 1, reinterpret_cast<const float*>(d), reinterpret_cast<float*>(d + in_bytes),
                                                c->stream),
                   "prach_demodulate");
    host_out.resize(rows * g.L);
    c->d2h(host_out.data(), d + in_bytes, host_out.size() * sizeof(srsran::cf_t));
    c->sync();
    size_t row = 0;
    for (unsigned td = 0; td != config.nof_td_occasions; ++td) {
      for (unsigned fd = 0; fd != config.nof_fd_occasions; ++fd) {
        for (unsigned symbol = 0; symbol != g.nof_symbols; ++symbol, ++row) {
          srsran::span<srsran::cf_t> dst = buffer.get_symbol(0, td, fd, symbol);
          std::copy_n(host_out.data() + row * g.L, g.L, dst.begin());
        }
      }
    }
  }

private:
  std::shared_ptr<context>  c;
  srsran::sampling_rate     srate;
  std::vector<srsran::cf_t> host_out;
};

class ofdm_prach_demodulator_factory_hip : public srsran::ofdm_prach_demodulator_factory
{
public:
  ofdm_prach_demodulator_factory_hip(std::shared_ptr<context> c_, srsran::sampling_rate srate_) : c(std::move(c_)), srate(srate_) {}
  std::unique_ptr<srsran::ofdm_prach_demodulator> create() override { return std::make_unique<ofdm_prach_demodulator_hip>(c, srate); }

private:
  std::shared_ptr<context> c;
  srsran::sampling_rate    srate;
};

inline std::shared_ptr<srsran::ofdm_prach_demodulator_factory> create_ofdm_prach_demodulator_factory_hip(std::shared_ptr<context> c,
                                                                                                        srsran::sampling_rate    srate)
{
  return std::make_shared<ofdm_prach_demodulator_factory_hip>(std::move(c), srate);
}

// ---------------------------------------------------------------------------------------------------------------- PUSCH processor
/// srsran::pusch_processor over miphy_pusch_process_batch (pusch_processor.h:158-162): estimation, demodulation and decoding in one
/// device pass, with the UCI multiplexed on the PUSCH demultiplexed and decoded behind it; the resource grid goes to the device once, the
/// transport block, the HARQ buffer of the rx_softbuffer, the UCI fields and the channel state information come back.
class pusch_processor_hip : public srsran::pusch_processor
{
public:
  /// \c uci_dec: uci_decoder_hip (the fields are decoded on the device behind the demultiplexer) or the reference's CPU UCI decoder
  /// (the soft bits come back and are decoded on the host); without it PDUs with multiplexed UCI are refused. \c enable_evm as in create_pusch_demodulator_factory_sw.
  /// \c max_layers: 1 (the reference's limit) to 4; a PDU on two to four layers goes through miphy_pusch_process_layers_batch_ex, with UCI
  /// and EVM as on one layer.
  pusch_processor_hip(std::shared_ptr<context> c, unsigned nof_iterations, bool early_stop, std::unique_ptr<srsran::uci_decoder> uci_dec_ = nullptr,
                      bool enable_evm_ = false, unsigned max_layers_ = 1) :
    c(std::move(c)), dec_nof_iterations(nof_iterations), dec_enable_early_stop(early_stop), uci_dec(std::move(uci_dec_)), enable_evm(enable_evm_),
    max_layers(max_layers_)
  {
  }
  void process(srsran::span<uint8_t>                    data,
               srsran::rx_softbuffer&                   softbuffer,
               srsran::pusch_processor_result_notifier& notifier,
               const srsran::resource_grid_reader&      grid,
               const pdu_t&                             pdu) override
  {
    const bool has_uci = pdu.uci.nof_harq_ack != 0 || pdu.uci.nof_csi_part1 != 0 || pdu.uci.nof_csi_part2 != 0;
    require(!has_uci || uci_dec != nullptr, "pusch_processor_hip: a PDU with multiplexed UCI needs the UCI decoder (see the factory).");
    require(has_uci || pdu.codeword.has_value(), "pusch_processor_hip: the PDU carries neither a codeword nor UCI.");
    const unsigned nl = pdu.nof_tx_layers;
    require(pdu.dmrs == srsran::dmrs_type::TYPE1 && pdu.nof_cdm_groups_without_data == 2 && nl >= 1 && nl <= max_layers,
            "Only DM-RS type 1, two CDM groups without data and one layer (up to max_layers with the layered path) are supported.");
    require(nl <= pdu.rx_ports.size(), "pusch_processor_hip: the layers need at least as many receive ports.");
    const srsran::bounded_bitset<srsran::MAX_RB> rb_mask = pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb);
    const unsigned nprb = rb_mask.size(), nsc = nprb * 12, nports = pdu.rx_ports.size();
    miphy_pusch_layers_pdu lp = {};
    miphy_pusch_pdu&       p  = lp.base;
    lp.nof_tx_layers          = static_cast<uint8_t>(nl);
    p.numerology = pdu.slot.numerology(), p.slot_in_frame = pdu.slot.slot_index(), p.rnti = pdu.rnti, p.n_id = pdu.n_id;
    p.dmrs_scrambling_id = pdu.scrambling_id, p.Nref = pdu.tbs_lbrm_bytes * 8, p.tb_bytes = data.size(), p.harq_cb_index = 0;
    p.n_scid = pdu.n_scid, p.mod = srsran::get_bits_per_symbol(pdu.mcs_descr.modulation), p.nof_rx_ports = nports;
    p.start_symbol = pdu.start_symbol_index, p.nof_symbols = pdu.nof_symbols;
    if (pdu.codeword.has_value()) {
      p.bg = bg_id(pdu.codeword.value().ldpc_base_graph), p.rv = pdu.codeword.value().rv, p.new_data = pdu.codeword.value().new_data;
    } else {
      p.bg = 1, p.tb_bytes = 1; // unused: no transport block is decoded
    }
    p.use_early_stop = dec_enable_early_stop, p.nof_ldpc_iterations = dec_nof_iterations, p.grid_nof_prb = nprb;
    for (unsigned i = 0; i != nports; ++i) {
      p.rx_ports[i] = i; // the staging grid is ordered by rx_ports
    }
    for (unsigned l = 0; l != 14 && l != pdu.dmrs_symbol_mask.size(); ++l) {
      if (pdu.dmrs_symbol_mask.test(l)) {
        p.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    rb_mask.for_each(0, nprb, [&p](unsigned r) { p.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    // UCI lengths through the reference's own get_ulsch_information (pusch_processor_impl.cpp:152-170)
    miphy_pusch_uci u = {};
    u.has_codeword    = pdu.codeword.has_value() ? 1U : 0U;
    if (has_uci) {
      srsran::ulsch_configuration uc;
      uc.tbs = srsran::units::bytes(data.size()).to_bits(), uc.mcs_descr = pdu.mcs_descr;
      uc.nof_harq_ack_bits = srsran::units::bits(pdu.uci.nof_harq_ack), uc.nof_csi_part1_bits = srsran::units::bits(pdu.uci.nof_csi_part1);
      uc.nof_csi_part2_bits = srsran::units::bits(pdu.uci.nof_csi_part2), uc.alpha_scaling = pdu.uci.alpha_scaling;
      uc.beta_offset_harq_ack = pdu.uci.beta_offset_harq_ack, uc.beta_offset_csi_part1 = pdu.uci.beta_offset_csi_part1;
      uc.beta_offset_csi_part2 = pdu.uci.beta_offset_csi_part2, uc.nof_rb = pdu.freq_alloc.get_nof_rb();
      uc.start_symbol_index = pdu.start_symbol_index, uc.nof_symbols = pdu.nof_symbols, uc.dmrs_type = srsran::dmrs_config_type::type1;
      uc.dmrs_symbol_mask = pdu.dmrs_symbol_mask, uc.nof_cdm_groups_without_data = pdu.nof_cdm_groups_without_data, uc.nof_layers = pdu.nof_tx_layers;
      const srsran::ulsch_information info = srsran::get_ulsch_information(uc);
      u.nof_harq_ack_bits = pdu.uci.nof_harq_ack, u.nof_csi_part1_bits = pdu.uci.nof_csi_part1, u.nof_csi_part2_bits = pdu.uci.nof_csi_part2;
      u.nof_enc_harq_ack_bits = info.nof_harq_ack_bits.value(), u.nof_enc_csi_part1_bits = info.nof_csi_part1_bits.value();
      u.nof_enc_csi_part2_bits = info.nof_csi_part2_bits.value(), u.nof_harq_ack_rvd = info.nof_harq_ack_rvd.value();
      u.harq_ack_offset = 0, u.csi_part1_offset = u.nof_enc_harq_ack_bits, u.csi_part2_offset = u.csi_part1_offset + u.nof_enc_csi_part1_bits;
    }
    const size_t nof_uci_llr = static_cast<size_t>(u.nof_enc_harq_ack_bits) + u.nof_enc_csi_part1_bits + u.nof_enc_csi_part2_bits;
    miphy_sch_segmentation sg = {};
    if (pdu.codeword.has_value()) {
      context::check(miphy_sch_segmentation_info(data.size(), p.bg, &sg), "segmentation");
      require(sg.nof_cbs == softbuffer.get_nof_codeblocks(), "Wrong number of codeblocks.");
    }
    const size_t CBS = 66 * 384, MSG = 1056;
    host.resize(static_cast<size_t>(nports) * 14 * nsc);
    for (unsigned i = 0; i != nports; ++i) {
      for (unsigned l = 0; l != 14; ++l) {
        grid.get(srsran::span<srsran::cf_t>(host.data() + (static_cast<size_t>(i) * 14 + l) * nsc, nsc), pdu.rx_ports[i], l, 0);
      }
    }
    auto*    resident = dynamic_cast<rx_softbuffer_hip*>(&softbuffer);
    auto*    d_g    = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto*    d_misc = static_cast<uint8_t*>(c->buf(3, 64 + 64 + 384 + data.size() + 64));
    auto*    d_uci  = static_cast<int8_t*>(c->buf(4, nof_uci_llr + 64));
    auto*    d_evm  = reinterpret_cast<float*>(d_misc + 56); // [0,52) codeblock CRC flags of a host softbuffer, [56,60) EVM, [64,..) result
    auto*    d_res  = reinterpret_cast<miphy_pusch_result*>(d_misc + 64);
    auto*    d_sc   = reinterpret_cast<float*>(d_misc + 128);
    uint8_t* d_tb   = d_misc + 512; // (80 scalars of a PDU on four layers in front of it)
    int8_t*  d_soft = nullptr;
    uint8_t *d_msg = nullptr, *d_crc = nullptr;
    std::vector<uint8_t> crc_h(sg.nof_cbs);
    if (resident != nullptr) { // softbuffer of rx_softbuffer_pool_hip: the HARQ state is used in place
      resident->flush();
      d_soft = resident->softbits(), d_msg = resident->msgs(), d_crc = resident->crc_ok();
      p.harq_cb_index = resident->first_cb();
    } else {
      d_soft = static_cast<int8_t*>(c->buf(1, sg.nof_cbs * CBS));
      d_msg  = static_cast<uint8_t*>(c->buf(2, sg.nof_cbs * MSG));
      d_crc  = d_misc;
      srsran::span<bool> crcs = softbuffer.get_codeblocks_crc();
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        crc_h[i] = crcs[i] ? 1 : 0;
        auto sb  = softbuffer.get_codeblock_soft_bits(i, sg.N);
        c->h2d(d_soft + i * CBS, sb.data(), sg.N);
        auto mb = softbuffer.get_codeblock_data_bits(i, sg.K);
        c->h2d(d_msg + i * MSG, mb.get_buffer().data(), (sg.K + 7) / 8);
      }
      c->h2d(d_crc, crc_h.data(), sg.nof_cbs);
    }
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    c->h2d(d_tb, data.data(), data.size());
    if (nl > 1) {
      context::check(miphy_pusch_process_layers_batch_ex(
                         c->ctx, &lp, &u, 1, d_g, d_soft, d_msg, d_crc, d_tb, d_res, d_sc, d_uci, enable_evm ? d_evm : nullptr, c->stream),
                     "pusch_process_layers");
    } else {
      context::check(
          miphy_pusch_process_batch_ex(c->ctx, &p, &u, 1, d_g, d_soft, d_msg, d_crc, d_tb, d_res, d_sc, d_uci, enable_evm ? d_evm : nullptr, c->stream),
          "pusch_process");
    }
    // With the device UCI decoder the fields are decoded behind _ex on the same stream: only payload bits and verdicts come back.
    const auto*          uci_dec_hip   = dynamic_cast<const uci_decoder_hip*>(uci_dec.get());
    const bool           uci_on_device = has_uci && uci_dec_hip != nullptr;
    // Fields of 1 to 11 bits go to the short-block detector, longer ones to the polar decoder; both write one payload area.
    miphy_uci_field_job  uci_short[3];
    miphy_uci_polar_job  uci_polar[3];
    uint32_t             short_field[3] = {}, polar_field[3] = {}, nof_short = 0, nof_polar = 0;
    constexpr size_t     UCI_PAYLOAD = 8; // [0, 3) short-block verdicts, [3, 6) polar verdicts, [8, ..) the payloads packed in field order
    size_t               nof_uci_out = 0;
    if (uci_on_device) {
      context::check(miphy_pusch_uci_jobs(&p, &u, 1, uci_short, short_field, &nof_short, uci_polar, polar_field, &nof_polar), "pusch_uci_jobs");
      for (uint32_t j = 0; j != nof_short; ++j) {
        uci_short[j].payload_offset += UCI_PAYLOAD;
      }
      for (uint32_t j = 0; j != nof_polar; ++j) {
        uci_polar[j].payload_offset += UCI_PAYLOAD;
      }
      nof_uci_out = UCI_PAYLOAD + pdu.uci.nof_harq_ack + pdu.uci.nof_csi_part1 + pdu.uci.nof_csi_part2;
      uci_out.resize(nof_uci_out);
      auto* d_uci_out = static_cast<uint8_t*>(c->buf(5, nof_uci_out));
      if (nof_short != 0) {
        context::check(miphy_uci_decode_batch(c->ctx, uci_short, 0, nof_short, d_uci, d_uci_out, d_uci_out, c->stream), "uci_decode");
      }
      if (nof_polar != 0) {
        context::check(miphy_uci_polar_decode_list_batch(
                           c->ctx, uci_polar, nof_polar, uci_dec_hip->get_list_size(), d_uci, d_uci_out, d_uci_out + 3, c->stream),
                       "uci_polar_decode");
      }
      c->d2h(uci_out.data(), d_uci_out, nof_uci_out); // (verdict slots without a job are not read)
    }
    miphy_pusch_result r;
    float              sc[80], evm = 0.F; // [rx port][layer][5]; layer 0 is what the channel state information averages
    uci_llr.resize(uci_on_device ? 0 : nof_uci_llr);
    if (nof_uci_llr && !uci_on_device) {
      c->d2h(uci_llr.data(), d_uci, nof_uci_llr);
    }
    if (enable_evm) {
      c->d2h(&evm, d_evm, sizeof(evm));
    }
    c->d2h(&r, d_res, sizeof(r));
    c->d2h(sc, d_sc, (nl > 1 ? 80 : 20) * sizeof(float));
    c->d2h(data.data(), d_tb, data.size());
    if (resident == nullptr) {
      c->d2h(crc_h.data(), d_crc, sg.nof_cbs);
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        auto sb = softbuffer.get_codeblock_soft_bits(i, sg.N);
        c->d2h(sb.data(), d_soft + i * CBS, sg.N);
        auto mb = softbuffer.get_codeblock_data_bits(i, sg.K);
        c->d2h(mb.get_buffer().data(), d_msg + i * MSG, (sg.K + 7) / 8);
      }
    }
    c->sync();
    if (resident == nullptr) {
      srsran::span<bool> crcs = softbuffer.get_codeblocks_crc();
      for (unsigned i = 0; i != sg.nof_cbs; ++i) {
        crcs[i] = crc_h[i] != 0;
      }
    }
    // channel_estimate::get_channel_state_information (channel_estimation.h:211-232): linear averages over the receive ports, then dB
    srsran::channel_state_information csi = {};
    float                             epre = 0, rsrp = 0, snr = 0;
    double                            ta   = 0;
    for (unsigned i = 0; i != nports; ++i) {
      const float* s = sc + 5 * i * nl;
      rsrp += s[0], epre += s[1], snr += s[3], ta += s[4];
    }
    csi.epre_dB        = srsran::convert_power_to_dB(epre / static_cast<float>(nports));
    csi.rsrp_dB        = srsran::convert_power_to_dB(rsrp / static_cast<float>(nports));
    csi.sinr_dB        = srsran::convert_power_to_dB(snr / static_cast<float>(nports));
    csi.time_alignment = srsran::phy_time_unit::from_seconds(ta / nports);
    if (enable_evm) {
      csi.sinr_dB = -20 * log10f(evm) - 3.7F; // pusch_processor_impl.cpp:237-241
    }
    notifier.on_csi(csi);
    if (has_uci) { // pusch_processor_impl.cpp:264-286: the three fields through the reference's UCI decoder
      srsran::uci_decoder::configuration ucfg;
      ucfg.modulation = pdu.mcs_descr.modulation;
      srsran::pusch_processor_result_control ru;
      if (enable_evm) {
        ru.evm.emplace(evm);
      }
      auto field = [&](unsigned k, size_t off, unsigned G, unsigned nof_bits) {
        srsran::pusch_uci_field f;
        if (nof_bits == 0) {
          f.payload.clear();
          f.status = srsran::uci_status::unknown;
          return f;
        }
        f.payload.resize(nof_bits);
        if (uci_on_device) {
          const uint32_t js = static_cast<uint32_t>(std::find(short_field, short_field + nof_short, k) - short_field);
          const uint32_t jp = static_cast<uint32_t>(std::find(polar_field, polar_field + nof_polar, k) - polar_field);
          const size_t   at = js != nof_short ? uci_short[js].payload_offset : uci_polar[jp].payload_offset;
          const uint8_t  st = js != nof_short ? uci_out[js] : uci_out[3 + jp];
          std::copy(uci_out.begin() + at, uci_out.begin() + at + nof_bits, f.payload.begin());
          f.status = st == MIPHY_UCI_STATUS_VALID ? srsran::uci_status::valid : srsran::uci_status::invalid;
          return f;
        }
        f.status = uci_dec->decode(f.payload, srsran::span<const srsran::log_likelihood_ratio>(uci_llr.data() + off, G), ucfg);
        return f;
      };
      ru.harq_ack  = field(0, u.harq_ack_offset, u.nof_enc_harq_ack_bits, pdu.uci.nof_harq_ack);
      ru.csi_part1 = field(1, u.csi_part1_offset, u.nof_enc_csi_part1_bits, pdu.uci.nof_csi_part1);
      ru.csi_part2 = field(2, u.csi_part2_offset, u.nof_enc_csi_part2_bits, pdu.uci.nof_csi_part2);
      notifier.on_uci(ru);
    }
    if (!pdu.codeword.has_value()) {
      return;
    }
    srsran::pusch_processor_result_data result;
    if (enable_evm) {
      result.evm.emplace(evm);
    }
    result.data.tb_crc_ok            = r.tb_crc_ok != 0;
    result.data.nof_codeblocks_total = r.nof_codeblocks_total;
    result.data.ldpc_decoder_stats.reset();
    if (r.nof_decoded > 0) {
      result.data.ldpc_decoder_stats.update(r.iters_min);
      for (unsigned i = 1; i + 1 < r.nof_decoded; ++i) {
        result.data.ldpc_decoder_stats.update(static_cast<unsigned>(r.iters_mean + 0.5F));
      }
      if (r.nof_decoded > 1) {
        result.data.ldpc_decoder_stats.update(r.iters_max);
      }
    }
    notifier.on_sch(result);
  }

private:
  std::shared_ptr<context>  c;
  unsigned                  dec_nof_iterations;
  bool                      dec_enable_early_stop;
  std::unique_ptr<srsran::uci_decoder>      uci_dec;
  bool                                      enable_evm;
  unsigned                                  max_layers;
  std::vector<srsran::cf_t>                 host;
  std::vector<srsran::log_likelihood_ratio> uci_llr;
  std::vector<uint8_t>                      uci_out;
};

/// Replaces create_pusch_processor_factory_sw(config) (channel_processor_factories.h): only the decoder settings of the
/// configuration are needed, the sub-block factories are not.
class pusch_processor_factory_hip : public srsran::pusch_processor_factory
{
public:
  /// \c uci_dec_factory: the reference's create_uci_decoder_factory_sw(...) for PDUs with multiplexed UCI (nullptr: such PDUs are
  /// rejected by the validator); \c enable_evm as in create_pusch_demodulator_factory_sw; \c max_layers: 1 to 4, for the processor and
  /// its validator (above one layer: miphy_pusch_process_layers_batch, beyond the reference).
  pusch_processor_factory_hip(std::shared_ptr<context>                     c,
                              unsigned                                     nof_iterations,
                              bool                                         early_stop,
                              std::shared_ptr<srsran::uci_decoder_factory> uci_dec_factory = nullptr,
                              bool                                         enable_evm      = false,
                              unsigned                                     max_layers      = 1) :
    c(std::move(c)), nof_iterations(nof_iterations), early_stop(early_stop), uci_dec_factory(std::move(uci_dec_factory)), enable_evm(enable_evm),
    max_layers(max_layers)
  {
  }
  std::unique_ptr<srsran::pusch_processor> create() override
  {
    return std::make_unique<pusch_processor_hip>(c, nof_iterations, early_stop, uci_dec_factory ? uci_dec_factory->create() : nullptr, enable_evm,
                                                 max_layers);
  }
  std::unique_ptr<srsran::pusch_pdu_validator> create_validator() override; // defined at the end of this header

private:
  std::shared_ptr<context>                     c;
  unsigned                                     nof_iterations;
  bool                                         early_stop;
  std::shared_ptr<srsran::uci_decoder_factory> uci_dec_factory;
  bool                                         enable_evm;
  unsigned                                     max_layers;
};

// ---------------------------------------------------------------------------------------------------------------- uplink processor
/// srsran::uplink_processor (uplink_processor.h:52-98, lib/phy/upper/uplink_processor_impl.cpp:143-214) that batches the PUSCH
/// PDUs of a slot into one device submission: process_pusch() only queues the PDU, flush() uploads the resource grid once,
/// runs miphy_pusch_process_batch over all queued PDUs and then notifies the results in the order the PDUs were queued, with
/// the notifications of uplink_processor_impl (channel state information, decoder result, payload view only when the CRC
/// passed, softbuffer released when the CRC passed). PRACH detection and PUCCH processing are delegated to the CPU blocks given
/// at construction. The softbuffers must come from rx_softbuffer_pool_hip (HARQ state resident on the device); a PDU with any
/// other softbuffer is processed at once through the per-PDU path.
///
/// The interface has no end-of-slot call: the caller invokes flush() after its loop over the PDUs of the slot
/// (upper_phy_rx_symbol_handler_impl.cpp:97-107); a PDU of another slot, a full queue and the destructor flush as well.
class uplink_processor_hip : public srsran::uplink_processor
{
public:
  /// \c linger_us > 0 (default): asynchronous delivery. process_pusch() returns at once; a delivery thread submits the PDUs of a slot
  /// as one device batch as soon as no further PDU has arrived for \c linger_us microseconds (or the batch is full / a PDU of another
  /// slot arrives) and calls the notifier from that thread -- the reference notifies from its executor threads as well. No end-of-slot
  /// call is needed, so the unmodified caller (upper_phy_rx_symbol_handler_impl.cpp:92-105) works. \c linger_us == 0: synchronous
  /// mode, results are delivered by flush() (or by the next PDU of another slot / the destructor).
  /// \c uci_dec_factory / \c enable_evm: for PDUs with multiplexed UCI, which take the per-PDU path (pusch_processor_hip).
  uplink_processor_hip(std::shared_ptr<context>                     c,
                       std::unique_ptr<srsran::prach_detector>      prach,
                       std::unique_ptr<srsran::pucch_processor>     pucch,
                       unsigned                                     grid_nof_ports,
                       unsigned                                     grid_nof_prb,
                       unsigned                                     dec_nof_iterations,
                       bool                                         dec_enable_early_stop,
                       unsigned                                     max_batch       = 64,
                       unsigned                                     linger_us       = 100,
                       std::shared_ptr<srsran::uci_decoder_factory> uci_dec_factory = nullptr,
                       bool                                         enable_evm      = false) :
    c(std::move(c)),
    prach(std::move(prach)),
    pucch(std::move(pucch)),
    single(this->c, dec_nof_iterations, dec_enable_early_stop, uci_dec_factory ? uci_dec_factory->create() : nullptr, enable_evm),
    nports(grid_nof_ports),
    nprb(grid_nof_prb),
    nof_iterations(dec_nof_iterations),
    early_stop(dec_enable_early_stop),
    max_batch(max_batch),
    linger(std::chrono::microseconds(linger_us))
  {
    if (linger_us != 0) {
      wc     = std::make_shared<context>(this->c->device); // the delivery thread drives the caller's device through its own context
      this->c->bind_thread();                              // (creating it left wc's device current, which is the same one)
      worker = std::thread([this]() { deliver_loop(); });
    }
  }
  ~uplink_processor_hip() override
  {
    flush();
    if (worker.joinable()) {
      {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
      }
      cv.notify_all();
      worker.join();
    }
  }

  void process_prach(srsran::upper_phy_rx_results_notifier& notifier, const srsran::prach_buffer& buffer, const srsran::prach_buffer_context& context) override
  {
    srsran_assert(prach, "A PRACH detector is required.");
    srsran::ul_prach_results r;
    r.context = context;
    srsran::prach_detector::configuration cfg;
    cfg.root_sequence_index = context.root_sequence_index, cfg.format = context.format, cfg.restricted_set = context.restricted_set;
    cfg.zero_correlation_zone = context.zero_correlation_zone, cfg.start_preamble_index = context.start_preamble_index;
    cfg.nof_preamble_indices = context.nof_preamble_indices, cfg.ra_scs = srsran::to_ra_subcarrier_spacing(context.pusch_scs);
    r.result = prach->detect(buffer, cfg);
    notifier.on_new_prach_results(r);
  }

  void process_pucch(srsran::upper_phy_rx_results_notifier& notifier, const srsran::resource_grid_reader& grid, const pucch_pdu& pdu) override
  {
    srsran_assert(pucch, "A PUCCH processor is required.");
    srsran::ul_pucch_results r;
    r.context = pdu.context;
    switch (pdu.context.format) {
      case srsran::pucch_format::FORMAT_0:
        r.processor_result = pucch->process(grid, pdu.format0);
        break;
      case srsran::pucch_format::FORMAT_1:
        r.processor_result = pucch->process(grid, pdu.format1);
        break;
      case srsran::pucch_format::FORMAT_2:
        r.processor_result = pucch->process(grid, pdu.format2);
        break;
      case srsran::pucch_format::FORMAT_3:
        r.processor_result = pucch->process(grid, pdu.format3);
        break;
      default:
        r.processor_result = pucch->process(grid, pdu.format4);
        break;
    }
    notifier.on_new_pucch_results(r);
  }

  void process_pusch(srsran::span<uint8_t>                  data,
                     srsran::unique_rx_softbuffer           softbuffer,
                     srsran::upper_phy_rx_results_notifier& notifier,
                     const srsran::resource_grid_reader&    grid,
                     const pusch_pdu&                       pdu) override
  {
    auto*      resident = dynamic_cast<rx_softbuffer_hip*>(&softbuffer.get());
    const bool has_uci  = pdu.pdu.uci.nof_harq_ack != 0 || pdu.pdu.uci.nof_csi_part1 != 0 || pdu.pdu.uci.nof_csi_part2 != 0;
    if (resident == nullptr || has_uci || !pdu.pdu.codeword.has_value()) {
      // not a device softbuffer, or UCI to decode on the host: per-PDU path at once, like uplink_processor_impl::process_pusch
      notifier_adaptor n(notifier, pdu, data);
      single.process(data, softbuffer.get(), n, grid, pdu.pdu);
      if (n.tb_crc_ok) {
        softbuffer.release();
      }
      return;
    }
    std::unique_lock<std::mutex> lk(mu);
    if (!open.entries.empty() && (open.entries.front().pdu.pdu.slot != pdu.pdu.slot || open.grid != &grid || open.entries.size() >= max_batch)) {
      close_open_batch(lk);
    }
    if (open.entries.empty()) {
      // The samples of the slot are copied NOW: the resource-grid pool may hand the grid to another slot before the batch is
      // submitted, and a late submission must be slow rather than wrong.
      const unsigned nsc = nprb * 12;
      open.grid          = &grid;
      open.samples.resize(static_cast<size_t>(nports) * 14 * nsc);
      for (unsigned p = 0; p != nports; ++p) {
        for (unsigned l = 0; l != 14; ++l) {
          grid.get(srsran::span<srsran::cf_t>(open.samples.data() + (static_cast<size_t>(p) * 14 + l) * nsc, nsc), p, l, 0);
        }
      }
    }
    open.entries.emplace_back(entry{data, std::move(softbuffer), resident, &notifier, pdu});
    last_push = std::chrono::steady_clock::now();
    lk.unlock();
    cv.notify_all();
  }

  /// Submits what is queued and returns when every result has been delivered (asynchronous mode: waits for the delivery thread).
  void flush()
  {
    std::unique_lock<std::mutex> lk(mu);
    if (!open.entries.empty()) {
      close_open_batch(lk);
    }
    if (worker.joinable()) {
      cv.notify_all();
      cv_done.wait(lk, [this]() { return ready.empty() && !busy; });
    }
  }

private:
  struct entry;
  struct batch;
  // Moves the open batch to the ready list (asynchronous mode) or runs it in place (synchronous mode). Called with the lock held.
  void close_open_batch(std::unique_lock<std::mutex>& lk)
  {
    batch b = std::move(open);
    open    = batch{};
    if (worker.joinable()) {
      ready.emplace_back(std::move(b));
      return;
    }
    lk.unlock();
    run_batch(b, *c);
    lk.lock();
  }
  void deliver_loop()
  {
    wc->bind_thread(); // a new thread starts on device 0
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      if (ready.empty() && !open.entries.empty()) {
        // wait for the linger time of the open batch, then close it
        if (!cv.wait_until(lk, last_push + linger, [this]() { return stop || !ready.empty() || std::chrono::steady_clock::now() >= last_push + linger; })) {
          continue;
        }
        if (ready.empty() && !open.entries.empty() && std::chrono::steady_clock::now() >= last_push + linger) {
          ready.emplace_back(std::move(open));
          open = batch{};
        }
      } else if (ready.empty()) {
        if (stop) {
          return;
        }
        cv.wait(lk, [this]() { return stop || !ready.empty() || !open.entries.empty(); });
        continue;
      }
      while (!ready.empty()) {
        batch b = std::move(ready.front());
        ready.pop_front();
        busy = true;
        lk.unlock();
        run_batch(b, *wc);
        lk.lock();
        busy = false;
      }
      cv_done.notify_all();
    }
  }
  void run_batch(batch& bt, context& dc)
  {
    std::vector<entry>& queue = bt.entries;
    if (queue.empty()) {
      return;
    }
    const unsigned n = queue.size();
    std::vector<srsran::cf_t>& host = bt.samples;
    std::vector<miphy_pusch_pdu> pdus(n);
    size_t                       tb_bytes = 0;
    int8_t*                      d_soft   = queue.front().resident->softbits();
    uint8_t *                    d_msg = queue.front().resident->msgs(), *d_crc = queue.front().resident->crc_ok();
    for (unsigned i = 0; i != n; ++i) {
      entry&                                  e   = queue[i];
      const srsran::pusch_processor::pdu_t&   pdu = e.pdu.pdu;
      require(e.resident->softbits() == d_soft, "All softbuffers of a batch must belong to the same device pool.");
      require(pdu.dmrs == srsran::dmrs_type::TYPE1 && pdu.nof_cdm_groups_without_data == 2 && pdu.nof_tx_layers == 1,
              "Only DM-RS type 1, two CDM groups without data and one layer are supported.");
      const srsran::bounded_bitset<srsran::MAX_RB> rb_mask = pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb);
      require(rb_mask.size() <= nprb, "The allocation exceeds the resource grid.");
      e.resident->flush();
      miphy_pusch_pdu& p = pdus[i];
      p                  = {};
      p.numerology = pdu.slot.numerology(), p.slot_in_frame = pdu.slot.slot_index(), p.rnti = pdu.rnti, p.n_id = pdu.n_id;
      p.dmrs_scrambling_id = pdu.scrambling_id, p.Nref = pdu.tbs_lbrm_bytes * 8, p.tb_bytes = e.data.size();
      p.harq_cb_index = e.resident->first_cb();
      p.n_scid = pdu.n_scid, p.mod = srsran::get_bits_per_symbol(pdu.mcs_descr.modulation), p.nof_rx_ports = pdu.rx_ports.size();
      p.start_symbol = pdu.start_symbol_index, p.nof_symbols = pdu.nof_symbols;
      p.bg = bg_id(pdu.codeword.value().ldpc_base_graph), p.rv = pdu.codeword.value().rv, p.new_data = pdu.codeword.value().new_data;
      p.use_early_stop = early_stop, p.nof_ldpc_iterations = nof_iterations, p.grid_nof_prb = nprb;
      for (unsigned k = 0; k != pdu.rx_ports.size(); ++k) {
        require(pdu.rx_ports[k] < nports, "Receive port outside the resource grid.");
        p.rx_ports[k] = pdu.rx_ports[k];
      }
      for (unsigned l = 0; l != 14 && l != pdu.dmrs_symbol_mask.size(); ++l) {
        if (pdu.dmrs_symbol_mask.test(l)) {
          p.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
        }
      }
      rb_mask.for_each(0, rb_mask.size(), [&p](unsigned r) { p.rb_mask[r >> 6] |= 1ULL << (r & 63); });
      p.grid_offset = 0, p.tb_offset = tb_bytes;
      tb_bytes += (e.data.size() + 15) & ~static_cast<size_t>(15);
    }
    auto*    d_g    = static_cast<float*>(dc.buf(0, host.size() * sizeof(srsran::cf_t)));
    auto*    d_tb   = static_cast<uint8_t*>(dc.buf(1, tb_bytes + 16));
    auto*    d_misc = static_cast<uint8_t*>(dc.buf(2, static_cast<size_t>(n) * (sizeof(miphy_pusch_result) + 80) + 64));
    auto*    d_res  = reinterpret_cast<miphy_pusch_result*>(d_misc);
    auto*    d_sc   = reinterpret_cast<float*>(d_misc + ((static_cast<size_t>(n) * sizeof(miphy_pusch_result) + 63) & ~static_cast<size_t>(63)));
    dc.h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_pusch_process_batch(dc.ctx, pdus.data(), n, d_g, d_soft, d_msg, d_crc, d_tb, d_res, d_sc, dc.stream), "pusch_process");
    std::vector<miphy_pusch_result> res(n);
    std::vector<float>              sc(static_cast<size_t>(n) * 20);
    std::vector<uint8_t>            tbs(tb_bytes);
    dc.d2h(res.data(), d_res, n * sizeof(miphy_pusch_result));
    dc.d2h(sc.data(), d_sc, sc.size() * sizeof(float));
    dc.d2h(tbs.data(), d_tb, tb_bytes);
    dc.sync();
    for (unsigned i = 0; i != n; ++i) {
      entry&                      e = queue[i];
      const miphy_pusch_result&   r = res[i];
      srsran::ul_pusch_results_data out;
      out.rnti = srsran::to_rnti(e.pdu.pdu.rnti), out.slot = e.pdu.pdu.slot, out.harq_id = e.pdu.harq_id;
      out.csi = csi_of(&sc[static_cast<size_t>(i) * 20], e.pdu.pdu.rx_ports.size());
      fill_decoder_result(out.decoder_result, r);
      if (r.tb_crc_ok != 0) {
        std::memcpy(e.data.data(), &tbs[pdus[i].tb_offset], e.data.size());
        out.payload = e.data;
      }
      e.notifier->on_new_pusch_results_data(out);
      if (r.tb_crc_ok != 0) {
        e.softbuffer.release();
      }
    }
    queue.clear(); // the remaining unique_rx_softbuffers unlock here
  }

  /// channel_estimate::get_channel_state_information (channel_estimation.h:211-232) from the estimator scalars of a PDU.
  static srsran::channel_state_information csi_of(const float* sc, unsigned nof_ports)
  {
    srsran::channel_state_information csi = {};
    float                             epre = 0, rsrp = 0, snr = 0;
    double                            ta   = 0;
    for (unsigned i = 0; i != nof_ports; ++i) {
      rsrp += sc[5 * i + 0], epre += sc[5 * i + 1], snr += sc[5 * i + 3], ta += sc[5 * i + 4];
    }
    csi.epre_dB        = srsran::convert_power_to_dB(epre / static_cast<float>(nof_ports));
    csi.rsrp_dB        = srsran::convert_power_to_dB(rsrp / static_cast<float>(nof_ports));
    csi.sinr_dB        = srsran::convert_power_to_dB(snr / static_cast<float>(nof_ports));
    csi.time_alignment = srsran::phy_time_unit::from_seconds(ta / nof_ports);
    return csi;
  }
  static void fill_decoder_result(srsran::pusch_decoder_result& out, const miphy_pusch_result& r)
  {
    out.tb_crc_ok            = r.tb_crc_ok != 0;
    out.nof_codeblocks_total = r.nof_codeblocks_total;
    out.ldpc_decoder_stats.reset();
    if (r.nof_decoded > 0) {
      out.ldpc_decoder_stats.update(r.iters_min);
      for (unsigned i = 1; i + 1 < r.nof_decoded; ++i) {
        out.ldpc_decoder_stats.update(static_cast<unsigned>(r.iters_mean + 0.5F));
      }
      if (r.nof_decoded > 1) {
        out.ldpc_decoder_stats.update(r.iters_max);
      }
    }
  }

private:
  /// pusch_processor_result_notifier_adaptor of uplink_processor_impl.cpp:41-105 for the per-PDU path.
  class notifier_adaptor : public srsran::pusch_processor_result_notifier
  {
  public:
    notifier_adaptor(srsran::upper_phy_rx_results_notifier& n, const pusch_pdu& pdu, srsran::span<const uint8_t> payload) : n(n), pdu(pdu), payload(payload) {}
    void on_csi(const srsran::channel_state_information& v) override { csi = v; }
    void on_uci(const srsran::pusch_processor_result_control& /**/) override {}
    void on_sch(const srsran::pusch_processor_result_data& sch) override
    {
      srsran::ul_pusch_results_data out;
      out.rnti = srsran::to_rnti(pdu.pdu.rnti), out.slot = pdu.pdu.slot, out.csi = csi, out.harq_id = pdu.harq_id;
      out.decoder_result = sch.data;
      out.payload        = sch.data.tb_crc_ok ? payload : srsran::span<const uint8_t>();
      n.on_new_pusch_results_data(out);
      tb_crc_ok = sch.data.tb_crc_ok;
    }
    bool tb_crc_ok = false;

  private:
    srsran::upper_phy_rx_results_notifier& n;
    const pusch_pdu&                       pdu;
    srsran::span<const uint8_t>            payload;
    srsran::channel_state_information      csi = {};
  };
  struct entry {
    srsran::span<uint8_t>                  data;
    srsran::unique_rx_softbuffer           softbuffer;
    rx_softbuffer_hip*                     resident;
    srsran::upper_phy_rx_results_notifier* notifier;
    pusch_pdu                              pdu;
  };

  struct batch {
    std::vector<entry>                  entries;
    const srsran::resource_grid_reader* grid = nullptr;
    std::vector<srsran::cf_t>           samples; // the slot's resource grid, copied when the batch was opened
  };

  std::shared_ptr<context>                 c, wc;
  std::unique_ptr<srsran::prach_detector>  prach;
  std::unique_ptr<srsran::pucch_processor> pucch;
  pusch_processor_hip                      single;
  unsigned                                 nports, nprb, nof_iterations;
  bool                                     early_stop;
  unsigned                                 max_batch;
  std::chrono::microseconds                linger;
  std::mutex                               mu;
  std::condition_variable                  cv, cv_done;
  std::thread                              worker;
  batch                                    open;
  std::deque<batch>                        ready;
  std::chrono::steady_clock::time_point    last_push;
  bool                                     stop = false, busy = false;
};

// ---------------------------------------------------------------------------------------------------------------- PDSCH modulator / DM-RS
/// The reserved-RE list only exposes per-symbol masks (re_pattern_list::get_exclusion_mask): turn them back into at most four
/// (PRB set, RE mask, symbol set) rectangles for the C ABI. Returns their number.
inline uint8_t reserved_rectangles(const srsran::re_pattern_list& reserved, unsigned nprb, miphy_re_pattern* out)
{
  if (reserved.get_nof_entries() == 0) {
    return 0;
  }
  const unsigned nsc = nprb * 12;
  struct rect {
    uint16_t                re;
    std::array<uint64_t, 5> prbs;
    uint16_t                symbols;
  };
  std::vector<rect> rects;
  for (unsigned l = 0; l != 14; ++l) {
    srsran::bounded_bitset<srsran::MAX_RB * srsran::NRE> msk(nsc);
    msk.fill(0, nsc, true);
    reserved.get_exclusion_mask(msk, l);
    std::vector<rect> here;
    for (unsigned r = 0; r != nprb; ++r) {
      uint16_t v = 0;
      for (unsigned k = 0; k != 12; ++k) {
        v |= static_cast<uint16_t>(msk.test(r * 12 + k) ? 0U : (1U << k));
      }
      if (v == 0) {
        continue;
      }
      auto it = std::find_if(here.begin(), here.end(), [v](const rect& x) { return x.re == v; });
      if (it == here.end()) {
        here.push_back(rect{v, {}, static_cast<uint16_t>(1U << l)});
        it = here.end() - 1;
      }
      it->prbs[r >> 6] |= 1ULL << (r & 63);
    }
    for (const rect& h : here) {
      auto it = std::find_if(rects.begin(), rects.end(), [&h](const rect& x) { return x.re == h.re && x.prbs == h.prbs; });
      if (it == rects.end()) {
        rects.push_back(h);
      } else {
        it->symbols |= h.symbols;
      }
    }
  }
  if (rects.size() > 4) {
    srsran::report_fatal_error("The reserved RE patterns need {} rectangles, at most 4 are supported by the HIP path.", rects.size());
  }
  uint8_t n = 0;
  for (const rect& x : rects) {
    miphy_re_pattern& o = out[n++];
    std::copy(x.prbs.begin(), x.prbs.end(), o.prb_mask);
    o.re_mask = x.re, o.symbols = x.symbols;
  }
  return n;
}

/// Writes the REs a kernel produced into a resource grid: `host` is one port of a staging grid [14][nsc] that was filled with
/// NaN before the kernel ran, so that everything that is not NaN was written.
inline void put_written_res(srsran::resource_grid_writer& grid, unsigned port, unsigned nsc, const srsran::cf_t* host)
{
  std::unique_ptr<bool[]>   mask(new bool[nsc]);
  std::vector<srsran::cf_t> vals;
  for (unsigned l = 0; l != 14; ++l) {
    vals.clear();
    for (unsigned k = 0; k != nsc; ++k) {
      const srsran::cf_t v = host[static_cast<size_t>(l) * nsc + k];
      mask[k]              = !std::isnan(v.real());
      if (mask[k]) {
        vals.push_back(v);
      }
    }
    if (!vals.empty()) {
      grid.put(port, l, 0, srsran::span<const bool>(mask.get(), nsc), vals);
    }
  }
}

/// The list rule of miphy_pdsch_modulate_mapped_batch on a PRB list in mapping order (rb_allocation::get_prb_indices) and the PRB mask of the
/// same allocation (rb_allocation::get_prb_mask): every entry inside the mask and set in it, none twice, as many entries as set bits.
inline bool prb_list_obeys_list_rule(const srsran::static_vector<uint16_t, srsran::MAX_RB>& list, const srsran::bounded_bitset<srsran::MAX_RB>& mask)
{
  srsran::bounded_bitset<srsran::MAX_RB> seen(mask.size());
  for (uint16_t rb : list) {
    if (rb >= mask.size() || !mask.test(rb) || seen.test(rb)) {
      return false;
    }
    seen.set(rb);
  }
  return list.size() == mask.count();
}

/// A precoding_configuration as the C ABI takes it: the miphy_precoding record (antenna port a on grid port a, weights_offset 0) and, in `weights`, the
/// coefficients in the order W[prg][port][layer] -- the memory order of the configuration's own tensor (layer fastest, then port, then PRG).
inline miphy_precoding precoding_of(const srsran::precoding_configuration& config, std::vector<srsran::cf_t>& weights)
{
  const unsigned  nlayers = config.get_nof_layers(), nports = config.get_nof_ports(), nprg = config.get_nof_prg();
  miphy_precoding p       = {};
  p.nof_layers = nlayers, p.nof_ports = nports, p.prg_size = config.get_prg_size(), p.nof_prg = nprg, p.weights_offset = 0;
  for (unsigned a = 0; a != 16; ++a) {
    p.ports[a] = a;
  }
  weights.resize(static_cast<size_t>(nprg) * nports * nlayers);
  for (unsigned g = 0; g != nprg; ++g) {
    for (unsigned a = 0; a != nports; ++a) {
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        weights[(static_cast<size_t>(g) * nports + a) * nlayers + ly] = config.get_coefficient(ly, a, g);
      }
    }
  }
  return p;
}

/// srsran::channel_precoder over miphy_channel_precode_batch (channel_precoder.h): the layers go up, the antenna ports come back.
class channel_precoder_hip : public srsran::channel_precoder
{
public:
  explicit channel_precoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void apply_precoding(srsran::re_buffer_writer& output, const srsran::re_buffer_reader& input, const srsran::precoding_weight_matrix& precoding) override
  {
    const unsigned nre = input.get_nof_re(), nlayers = precoding.get_nof_layers(), nports = precoding.get_nof_ports();
    srsran_assert(input.get_nof_slices() == nlayers && output.get_nof_slices() == nports && output.get_nof_re() == nre,
                  "The input, the output and the weights do not agree on {} layers, {} ports and {} REs.", nlayers, nports, nre);
    if (nre == 0) {
      return;
    }
    miphy_precode_job j = {};
    j.nof_re = nre, j.nof_layers = nlayers, j.nof_ports = nports, j.in_stride = nre, j.out_stride = nre;
    host.resize(static_cast<size_t>(nlayers) * nre);
    weights.resize(static_cast<size_t>(nports) * nlayers);
    for (unsigned ly = 0; ly != nlayers; ++ly) {
      const srsran::span<const srsran::cf_t> x = input.get_slice(ly);
      std::copy(x.begin(), x.end(), host.begin() + static_cast<size_t>(ly) * nre);
    }
    for (unsigned a = 0; a != nports; ++a) {
      const srsran::span<const srsran::cf_t> w = precoding.get_port_coefficients(a);
      std::copy(w.begin(), w.end(), weights.begin() + static_cast<size_t>(a) * nlayers);
    }
    auto* d_in  = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto* d_out = static_cast<float*>(c->buf(1, static_cast<size_t>(nports) * nre * sizeof(srsran::cf_t)));
    c->h2d(d_in, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_channel_precode_batch(c->ctx, &j, 0, 1, reinterpret_cast<const float*>(weights.data()), weights.size(), d_in, d_out, c->stream),
                   "channel_precode");
    host.resize(static_cast<size_t>(nports) * nre);
    c->d2h(host.data(), d_out, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned a = 0; a != nports; ++a) {
      const srsran::span<srsran::cf_t> y = output.get_slice(a);
      std::copy(host.begin() + static_cast<size_t>(a) * nre, host.begin() + static_cast<size_t>(a + 1) * nre, y.begin());
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host, weights;
};

/// Replaces create_channel_precoder_factory("generic" / "auto") (precoding_factories.h).
class channel_precoder_factory_hip : public srsran::channel_precoder_factory
{
public:
  explicit channel_precoder_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::channel_precoder> create() override { return std::make_unique<channel_precoder_hip>(c); }

private:
  std::shared_ptr<context> c;
};

inline std::shared_ptr<srsran::channel_precoder_factory> create_channel_precoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<channel_precoder_factory_hip>(std::move(c));
}

/// srsran::pdsch_modulator over miphy_pdsch_modulate_batch (pdsch_modulator.h:98). One codeword on one layer, contiguous
/// allocation -- the configurations the 23.5 software modulator handles correctly -- and, beyond it, one codeword on two to four
/// layers (config.ports.size() layers, layer ly on port config.ports[ly]) over miphy_pdsch_modulate_layers_batch. An allocation that is
/// not contiguous or is interleaved goes over miphy_pdsch_modulate_mapped_batch with rb_allocation::get_prb_indices as the list in
/// mapping order (where the reference's vrb_to_prb_mapper deviates from TS 38.211 7.3.1.6). Two codewords on five to eight
/// layers (TS 38.211 Table 7.3.1.3-1) go over miphy_pdsch_modulate_codewords_batch, with the list where the allocation is not contiguous.
class pdsch_modulator_hip : public srsran::pdsch_modulator
{
public:
  explicit pdsch_modulator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void modulate(srsran::resource_grid_writer& grid, srsran::span<const srsran::bit_buffer> codewords, const config_t& config) override
  {
    const unsigned nlayers = config.ports.size();
    srsran_assert((nlayers >= 1 && nlayers <= 4 && codewords.size() == 1) || (nlayers >= 5 && nlayers <= 8 && codewords.size() == 2),
                  "Only one codeword on one to four layers or two codewords on five to eight layers are supported.");
    const srsran::bounded_bitset<srsran::MAX_RB> prb = config.freq_allocation.get_prb_mask(config.bwp_start_rb, config.bwp_size_rb);
    const unsigned                               nprb = prb.size(), nsc = nprb * 12;
    const miphy_pdsch_mod_job                    j    = job_of(config, codewords[0], prb);
    const size_t                                 cw1_offset = (bits.size() + 15) & ~static_cast<size_t>(15);
    if (codewords.size() == 2) { // the bits of codeword 1 behind those of codeword 0
      bits.resize(cw1_offset + codewords[1].size());
      for (unsigned i = 0; i != codewords[1].size(); ++i) {
        bits[cw1_offset + i] = codewords[1].extract<uint8_t>(i, 1);
      }
    }
    host.assign(static_cast<size_t>(nlayers) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernel"
    auto* d_cw = static_cast<uint8_t*>(c->buf(0, bits.size() + 16));
    auto* d_g  = static_cast<float*>(c->buf(1, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_cw, bits.data(), bits.size());
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    if (codewords.size() == 2) {
      srsran::static_vector<uint16_t, srsran::MAX_RB> list;
      miphy_pdsch_mod_codewords_job                   cj = {};
      if (!config.freq_allocation.is_contiguous()) {
        list              = config.freq_allocation.get_prb_indices(config.bwp_start_rb, config.bwp_size_rb);
        cj.mapped.nof_prb = list.size();
      }
      cj.mapped.layers.base = j, cj.nof_layers = nlayers, cj.mod1 = srsran::get_bits_per_symbol(config.modulation2);
      cj.nof_bits1 = codewords[1].size(), cj.cw1_offset = cw1_offset;
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        cj.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_modulate_codewords_batch(c->ctx, &cj, 0, 1, list.data(), list.size(), d_cw, d_g, c->stream), "pdsch_modulate_codewords");
    } else if (!config.freq_allocation.is_contiguous()) {
      const srsran::static_vector<uint16_t, srsran::MAX_RB> list = config.freq_allocation.get_prb_indices(config.bwp_start_rb, config.bwp_size_rb);
      miphy_pdsch_mod_mapped_job                            mj   = {};
      mj.layers.base = j, mj.layers.nof_layers = nlayers, mj.prb_list_offset = 0, mj.nof_prb = list.size();
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        mj.layers.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_modulate_mapped_batch(c->ctx, &mj, 0, 1, list.data(), list.size(), d_cw, d_g, c->stream), "pdsch_modulate_mapped");
    } else if (nlayers == 1) {
      context::check(miphy_pdsch_modulate_batch(c->ctx, &j, 0, 1, d_cw, d_g, c->stream), "pdsch_modulate");
    } else {
      miphy_pdsch_mod_layers_job lj = {};
      lj.base = j, lj.nof_layers = nlayers;
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        lj.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_modulate_layers_batch(c->ctx, &lj, 0, 1, d_cw, d_g, c->stream), "pdsch_modulate_layers");
    }
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned ly = 0; ly != nlayers; ++ly) {
      put_written_res(grid, config.ports[ly], nsc, host.data() + static_cast<size_t>(ly) * 14 * nsc);
    }
  }

  /// The same with precoding (not part of srsran::pdsch_modulator, whose 23.5 form carries none): config.ports.size() stays the number of layers, the
  /// layers go through the per-PRG matrices of `precoding` (PRG 0 starts at CRB 0) onto its antenna ports, antenna port a being grid port a, over
  /// miphy_pdsch_modulate_precoded_batch -- with the allocation's PRB list in mapping order where it is not contiguous.
  void modulate(srsran::resource_grid_writer& grid, srsran::span<const srsran::bit_buffer> codewords, const config_t& config,
                const srsran::precoding_configuration& precoding)
  {
    const unsigned nlayers = config.ports.size();
    srsran_assert(nlayers >= 1 && nlayers <= 4 && codewords.size() == 1, "Only one codeword on one to four layers is supported.");
    srsran_assert(precoding.get_nof_layers() == nlayers, "The precoding is for {} layers, the transmission has {}.", precoding.get_nof_layers(), nlayers);
    const srsran::bounded_bitset<srsran::MAX_RB> prb = config.freq_allocation.get_prb_mask(config.bwp_start_rb, config.bwp_size_rb);
    const unsigned                               nprb = prb.size(), nsc = nprb * 12, nports = precoding.get_nof_ports();
    miphy_pdsch_mod_precoded_job                 pj   = {};
    pj.mapped.layers.base = job_of(config, codewords[0], prb), pj.mapped.layers.nof_layers = nlayers;
    srsran::static_vector<uint16_t, srsran::MAX_RB> list;
    if (!config.freq_allocation.is_contiguous()) {
      list              = config.freq_allocation.get_prb_indices(config.bwp_start_rb, config.bwp_size_rb);
      pj.mapped.nof_prb = list.size();
    }
    pj.precoding = precoding_of(precoding, weights);
    host.assign(static_cast<size_t>(nports) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernel"
    auto* d_cw = static_cast<uint8_t*>(c->buf(0, bits.size() + 16));
    auto* d_g  = static_cast<float*>(c->buf(1, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_cw, bits.data(), bits.size());
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_pdsch_modulate_precoded_batch(c->ctx, &pj, 0, 1, list.data(), list.size(), reinterpret_cast<const float*>(weights.data()), weights.size(),
                                                       d_cw, d_g, c->stream),
                   "pdsch_modulate_precoded");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned a = 0; a != nports; ++a) {
      put_written_res(grid, a, nsc, host.data() + static_cast<size_t>(a) * 14 * nsc);
    }
  }

private:
  /// The modulator job of a configuration on a staging grid of `prb.size()` PRBs; the codeword's bits go to `bits`, one per byte.
  miphy_pdsch_mod_job job_of(const config_t& config, const srsran::bit_buffer& cw, const srsran::bounded_bitset<srsran::MAX_RB>& prb)
  {
    const unsigned      nprb = prb.size();
    miphy_pdsch_mod_job j    = {};
    j.rnti = config.rnti, j.n_id = config.n_id, j.scaling = config.scaling;
    j.mod  = srsran::get_bits_per_symbol(config.modulation1);
    j.port = 0; // the staging grid has a single port
    j.start_symbol = config.start_symbol_index, j.nof_symbols = config.nof_symbols;
    j.dmrs_type    = (config.dmrs_config_type == srsran::dmrs_type::TYPE1) ? 1 : 2;
    j.nof_cdm_groups_without_data = config.nof_cdm_groups_without_data;
    j.grid_nof_prb = nprb, j.bwp_start_rb = config.bwp_start_rb, j.bwp_size_rb = config.bwp_size_rb;
    for (unsigned l = 0; l != 14 && l != config.dmrs_symb_pos.size(); ++l) {
      if (config.dmrs_symb_pos.test(l)) {
        j.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    prb.for_each(0, nprb, [&j](unsigned r) { j.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    j.nof_reserved = reserved_rectangles(config.reserved, nprb, j.reserved);
    j.nof_bits     = cw.size();
    bits.resize(cw.size());
    for (unsigned i = 0; i != cw.size(); ++i) {
      bits[i] = cw.extract<uint8_t>(i, 1);
    }
    return j;
  }

  std::shared_ptr<context>  c;
  std::vector<uint8_t>      bits;
  std::vector<srsran::cf_t> host, weights;
};

/// srsran::dmrs_pdsch_processor over miphy_dmrs_pdsch_map_batch (dmrs_pdsch_processor.h:65).
class dmrs_pdsch_processor_hip : public srsran::dmrs_pdsch_processor
{
public:
  explicit dmrs_pdsch_processor_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void map(srsran::resource_grid_writer& grid, const config_t& config) override
  {
    const unsigned nprb = config.rb_mask.size(), nsc = nprb * 12, nports = config.ports.size();
    miphy_dmrs_pdsch_job j = {};
    j.slot_in_frame = config.slot.slot_index(), j.reference_point_k_rb = config.reference_point_k_rb, j.scrambling_id = config.scrambling_id;
    j.amplitude = config.amplitude, j.dmrs_type = (config.type == srsran::dmrs_type::TYPE1) ? 1 : 2, j.n_scid = config.n_scid;
    j.nof_ports = nports, j.grid_nof_prb = nprb;
    for (unsigned p = 0; p != nports; ++p) {
      j.ports[p] = p; // staging grid indexed by DM-RS port
    }
    for (unsigned l = 0; l != 14 && l != config.symbols_mask.size(); ++l) {
      if (config.symbols_mask.test(l)) {
        j.symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    config.rb_mask.for_each(0, nprb, [&j](unsigned r) { j.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    host.assign(static_cast<size_t>(nports) * 14 * nsc, srsran::cf_t(NAN, NAN));
    auto* d_g = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_dmrs_pdsch_map_batch(c->ctx, &j, 0, 1, d_g, c->stream), "dmrs_pdsch_map");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    std::unique_ptr<bool[]>   m(new bool[nsc]);
    std::vector<srsran::cf_t> vals;
    for (unsigned p = 0; p != nports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        vals.clear();
        for (unsigned k = 0; k != nsc; ++k) {
          const srsran::cf_t v = host[(static_cast<size_t>(p) * 14 + l) * nsc + k];
          m[k]                 = !std::isnan(v.real());
          if (m[k]) {
            vals.push_back(v);
          }
        }
        if (!vals.empty()) {
          grid.put(config.ports[p], l, 0, srsran::span<const bool>(m.get(), nsc), vals);
        }
      }
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host;
};

// ---------------------------------------------------------------------------------------------------------------- PDSCH processor
/// srsran::pdsch_processor over miphy_pdsch_process_batch (pdsch_processor.h:164-166): encoding, modulation and DM-RS generation
/// in one device pass; the transport block goes up, the written resource elements come back. A PDU of one codeword on two to four
/// layers (pdu.ports.size() layers, layer ly and DM-RS port 1000 + ly on port pdu.ports[ly]) goes to miphy_pdsch_process_layers_batch, a
/// PDU of two codewords on five to eight layers to miphy_pdsch_process_codewords_batch (data[q] is transport block q), a
/// PDU whose allocation is not contiguous or is interleaved to miphy_pdsch_process_mapped_batch with rb_allocation::get_prb_indices as
/// its list in mapping order.
class pdsch_processor_hip : public srsran::pdsch_processor
{
public:
  explicit pdsch_processor_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void process(srsran::resource_grid_writer&                                                        grid,
               srsran::static_vector<srsran::span<const uint8_t>, srsran::pdsch_processor::MAX_NOF_TRANSPORT_BLOCKS> data,
               const pdu_t&                                                                         pdu) override
  {
    const unsigned nlayers = pdu.ports.size();
    const bool     two     = pdu.codewords.size() == 2;
    srsran_assert((nlayers >= 1 && nlayers <= 4 && pdu.codewords.size() == 1 && data.size() == 1) || (nlayers >= 5 && nlayers <= 8 && two && data.size() == 2),
                  "Only one codeword on one to four layers or two codewords on five to eight layers are supported.");
    srsran_assert(pdu.dmrs == srsran::dmrs_type::TYPE1, "Only DM-RS Type 1 is currently supported.");
    const srsran::bounded_bitset<srsran::MAX_RB> prb  = pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb);
    const unsigned                               nprb = prb.size(), nsc = nprb * 12;
    const miphy_pdsch_pdu                        p    = pdu_of(pdu, data[0].size(), prb);
    const size_t                                 tb1_offset = (data[0].size() + 15) & ~static_cast<size_t>(15); // transport block 1 behind block 0
    host.assign(static_cast<size_t>(nlayers) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernels"
    auto* d_tb = static_cast<uint8_t*>(c->buf(0, tb1_offset + (two ? data[1].size() : 0) + 16));
    auto* d_g  = static_cast<float*>(c->buf(1, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_tb, data[0].data(), data[0].size());
    if (two) {
      c->h2d(d_tb + tb1_offset, data[1].data(), data[1].size());
    }
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    if (two) {
      srsran::static_vector<uint16_t, srsran::MAX_RB> list;
      miphy_pdsch_codewords_pdu                       cp = {};
      if (!pdu.freq_alloc.is_contiguous()) {
        list              = pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb);
        cp.mapped.nof_prb = list.size();
      }
      cp.mapped.layers.base = p, cp.nof_layers = nlayers;
      second_block_of(pdu, data[1].size(), tb1_offset, cp);
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        cp.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_process_codewords_batch(c->ctx, &cp, 1, list.data(), list.size(), d_tb, d_g, c->stream), "pdsch_process_codewords");
    } else if (!pdu.freq_alloc.is_contiguous()) {
      const srsran::static_vector<uint16_t, srsran::MAX_RB> list = pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb);
      miphy_pdsch_mapped_pdu                                mp   = {};
      mp.layers.base = p, mp.layers.nof_layers = nlayers, mp.prb_list_offset = 0, mp.nof_prb = list.size();
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        mp.layers.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_process_mapped_batch(c->ctx, &mp, 1, list.data(), list.size(), d_tb, d_g, c->stream), "pdsch_process_mapped");
    } else if (nlayers == 1) {
      context::check(miphy_pdsch_process_batch(c->ctx, &p, 1, d_tb, d_g, c->stream), "pdsch_process");
    } else {
      miphy_pdsch_layers_pdu lp = {};
      lp.base = p, lp.nof_layers = nlayers;
      for (unsigned ly = 0; ly != nlayers; ++ly) {
        lp.ports[ly] = ly; // the staging grid has one port per layer
      }
      context::check(miphy_pdsch_process_layers_batch(c->ctx, &lp, 1, d_tb, d_g, c->stream), "pdsch_process_layers");
    }
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned ly = 0; ly != nlayers; ++ly) {
      put_written_res(grid, pdu.ports[ly], nsc, host.data() + static_cast<size_t>(ly) * 14 * nsc);
    }
  }

  /// The same with precoding (not part of srsran::pdsch_processor: the 23.5 pdu_t carries none): pdu.ports.size() stays the number of layers, the data
  /// and its DM-RS go through the per-PRG matrices of `precoding` onto its antenna ports, antenna port a being grid port a, over
  /// miphy_pdsch_process_precoded_batch.
  void process(srsran::resource_grid_writer&                                                        grid,
               srsran::static_vector<srsran::span<const uint8_t>, srsran::pdsch_processor::MAX_NOF_TRANSPORT_BLOCKS> data,
               const pdu_t&                                                                         pdu,
               const srsran::precoding_configuration&                                               precoding)
  {
    const unsigned nlayers = pdu.ports.size();
    srsran_assert(nlayers >= 1 && nlayers <= 4 && pdu.codewords.size() == 1 && data.size() == 1, "Only one codeword on one to four layers is supported.");
    srsran_assert(pdu.dmrs == srsran::dmrs_type::TYPE1, "Only DM-RS Type 1 is currently supported.");
    srsran_assert(precoding.get_nof_layers() == nlayers, "The precoding is for {} layers, the transmission has {}.", precoding.get_nof_layers(), nlayers);
    const srsran::bounded_bitset<srsran::MAX_RB> prb  = pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb);
    const unsigned                               nprb = prb.size(), nsc = nprb * 12, nports = precoding.get_nof_ports();
    miphy_pdsch_precoded_pdu                     pp   = {};
    pp.mapped.layers.base = pdu_of(pdu, data[0].size(), prb), pp.mapped.layers.nof_layers = nlayers;
    srsran::static_vector<uint16_t, srsran::MAX_RB> list;
    if (!pdu.freq_alloc.is_contiguous()) {
      list              = pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb);
      pp.mapped.nof_prb = list.size();
    }
    pp.precoding = precoding_of(precoding, weights);
    host.assign(static_cast<size_t>(nports) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernels"
    auto* d_tb = static_cast<uint8_t*>(c->buf(0, data[0].size() + 16));
    auto* d_g  = static_cast<float*>(c->buf(1, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_tb, data[0].data(), data[0].size());
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_pdsch_process_precoded_batch(c->ctx, &pp, 1, list.data(), list.size(), reinterpret_cast<const float*>(weights.data()), weights.size(), d_tb,
                                                      d_g, c->stream),
                   "pdsch_process_precoded");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned a = 0; a != nports; ++a) {
      put_written_res(grid, a, nsc, host.data() + static_cast<size_t>(a) * 14 * nsc);
    }
  }

  /// Transport block 1 of a two-codeword PDU (tb_bytes at tb_offset of the call's transport blocks) into its record; the base graph is the PDU's.
  static void second_block_of(const pdu_t& pdu, size_t tb_bytes, size_t tb_offset, miphy_pdsch_codewords_pdu& cp)
  {
    cp.bg1 = bg_id(pdu.ldpc_base_graph), cp.rv1 = pdu.codewords[1].rv, cp.mod1 = srsran::get_bits_per_symbol(pdu.codewords[1].modulation);
    cp.tb_bytes1 = tb_bytes, cp.tb_offset1 = tb_offset;
  }

private:
  /// The processor's record of a PDU with a transport block of tb_bytes on a staging grid of `prb.size()` PRBs.
  static miphy_pdsch_pdu pdu_of(const pdu_t& pdu, size_t tb_bytes, const srsran::bounded_bitset<srsran::MAX_RB>& prb)
  {
    const unsigned  nprb = prb.size();
    miphy_pdsch_pdu p    = {};
    p.slot_in_frame = pdu.slot.slot_index(), p.rnti = pdu.rnti, p.n_id = pdu.n_id, p.dmrs_scrambling_id = pdu.scrambling_id;
    p.tbs_lbrm_bytes = pdu.tbs_lbrm_bytes, p.tb_bytes = tb_bytes;
    p.ratio_pdsch_dmrs_to_sss_dB = pdu.ratio_pdsch_dmrs_to_sss_dB, p.ratio_pdsch_data_to_sss_dB = pdu.ratio_pdsch_data_to_sss_dB;
    p.bg = bg_id(pdu.ldpc_base_graph), p.rv = pdu.codewords[0].rv, p.mod = srsran::get_bits_per_symbol(pdu.codewords[0].modulation);
    p.port = 0; // the staging grid has a single port
    p.start_symbol = pdu.start_symbol_index, p.nof_symbols = pdu.nof_symbols, p.nof_cdm_groups_without_data = pdu.nof_cdm_groups_without_data;
    p.n_scid = pdu.n_scid ? 1 : 0, p.ref_point_prb0 = (pdu.ref_point == pdu_t::PRB0) ? 1 : 0;
    p.grid_nof_prb = nprb, p.bwp_start_rb = pdu.bwp_start_rb, p.bwp_size_rb = pdu.bwp_size_rb;
    for (unsigned l = 0; l != 14 && l != pdu.dmrs_symbol_mask.size(); ++l) {
      if (pdu.dmrs_symbol_mask.test(l)) {
        p.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
      }
    }
    prb.for_each(0, nprb, [&p](unsigned r) { p.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    p.nof_reserved = reserved_rectangles(pdu.reserved, nprb, p.reserved);
    return p;
  }

  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host, weights;
};

/// Replaces create_pdsch_processor_factory_sw(encoder, modulator, dmrs) (channel_processor_factories.h:153-156).
class pdsch_processor_factory_hip : public srsran::pdsch_processor_factory
{
public:
  explicit pdsch_processor_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::pdsch_processor>     create() override { return std::make_unique<pdsch_processor_hip>(c); }
  std::unique_ptr<srsran::pdsch_pdu_validator> create_validator() override; // defined at the end of this header

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- PDCCH processor
/// srsran::pdcch_processor over miphy_pdcch_process_batch (pdcch_processor.h:151): the CCE-to-PRB mapping is the reference's own host
/// function (pdcch_processor_impl::compute_rb_mask, lib/ran/pdcch/cce_to_prb_mapping.cpp), everything after it -- encoding, scrambling,
/// modulation, mapping and DM-RS -- runs on the device; the written REs come back through the resource_grid_mapper's grid.
class pdcch_processor_hip : public srsran::pdcch_processor
{
public:
  explicit pdcch_processor_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void process(srsran::resource_grid_mapper& mapper, const pdu_t& pdu) override
  {
    const coreset_description& coreset = pdu.coreset;
    const dci_description&     dci     = pdu.dci;
    srsran_assert(coreset.duration > 0 && coreset.duration <= srsran::pdcch_constants::MAX_CORESET_DURATION, "Invalid CORESET duration ({})", coreset.duration);
    srsran::prb_index_list prbs;
    switch (coreset.cce_to_reg_mapping) {
      case cce_to_reg_mapping_type::CORESET0:
        prbs = srsran::cce_to_prb_mapping_coreset0(coreset.bwp_start_rb, coreset.bwp_size_rb, coreset.duration, coreset.shift_index, dci.aggregation_level, dci.cce_index);
        break;
      case cce_to_reg_mapping_type::NON_INTERLEAVED:
        prbs = srsran::cce_to_prb_mapping_non_interleaved(coreset.bwp_start_rb, coreset.frequency_resources, coreset.duration, dci.aggregation_level, dci.cce_index);
        break;
      default:
        prbs = srsran::cce_to_prb_mapping_interleaved(coreset.bwp_start_rb, coreset.frequency_resources, coreset.duration, coreset.reg_bundle_size, coreset.interleaver_size,
                                                      coreset.shift_index, dci.aggregation_level, dci.cce_index);
        break;
    }
    const unsigned  nprb = coreset.bwp_start_rb + coreset.bwp_size_rb, nsc = nprb * 12;
    miphy_pdcch_pdu p    = {};
    p.slot_in_frame = pdu.slot.slot_index(), p.rnti = dci.rnti, p.n_id_pdcch_data = dci.n_id_pdcch_data, p.n_rnti = dci.n_rnti;
    p.n_id_pdcch_dmrs = dci.n_id_pdcch_dmrs;
    p.reference_point_k_rb = coreset.cce_to_reg_mapping == cce_to_reg_mapping_type::CORESET0 ? coreset.bwp_start_rb : 0;
    p.data_power_offset_dB = dci.data_power_offset_dB, p.dmrs_power_offset_dB = dci.dmrs_power_offset_dB;
    p.payload_size = dci.payload.size(), p.aggregation_level = dci.aggregation_level, p.start_symbol = coreset.start_symbol_index;
    p.duration = coreset.duration, p.port = 0, p.grid_nof_prb = nprb;
    for (uint16_t r : prbs) {
      p.rb_mask[r >> 6] |= 1ULL << (r & 63);
    }
    host.assign(static_cast<size_t>(14) * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernels"
    auto* d_pl = static_cast<uint8_t*>(c->buf(0, dci.payload.size() + 16));
    auto* d_g  = static_cast<float*>(c->buf(1, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_pl, dci.payload.data(), dci.payload.size());
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_pdcch_process_batch(c->ctx, &p, 1, d_pl, d_g, c->stream), "pdcch_process");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    // Data REs {0,2,3,4,6,7,8,10,11} and DM-RS REs {1,5,9}: every RE of the allocated PRBs over the CORESET symbols was written, so
    // one pattern (all twelve REs) hands them to the mapper in its own order: symbol by symbol, ascending subcarrier.
    srsran::re_pattern pattern;
    pattern.prb_mask = srsran::bounded_bitset<srsran::MAX_RB>(nprb);
    for (uint16_t r : prbs) {
      pattern.prb_mask.set(r, true);
    }
    pattern.symbols.fill(coreset.start_symbol_index, coreset.start_symbol_index + coreset.duration);
    pattern.re_mask = ~srsran::re_prb_mask();
    srsran::dynamic_re_buffer res(1, prbs.size() * 12 * coreset.duration);
    srsran::span<srsran::cf_t> out = res.get_slice(0);
    unsigned                   n   = 0;
    for (unsigned l = coreset.start_symbol_index; l != coreset.start_symbol_index + coreset.duration; ++l) {
      for (unsigned r = 0; r != nprb; ++r) {
        if (pattern.prb_mask.test(r)) {
          for (unsigned k = 0; k != 12; ++k) {
            out[n++] = host[static_cast<size_t>(l) * nsc + r * 12 + k];
          }
        }
      }
    }
    srsran::re_pattern_list patterns;
    patterns.merge(pattern);
    mapper.map(res, patterns, srsran::make_single_port());
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host;
};

/// Replaces create_pdcch_processor_factory_sw(encoder, modulator, dmrs) (channel_processor_factories.h:113-116).
class pdcch_processor_factory_hip : public srsran::pdcch_processor_factory
{
public:
  explicit pdcch_processor_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::pdcch_processor>     create() override { return std::make_unique<pdcch_processor_hip>(c); }
  std::unique_ptr<srsran::pdcch_pdu_validator> create_validator() override; // defined at the end of this header

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- SS/PBCH block processor
/// srsran::ssb_processor over miphy_ssb_process_batch (ssb_processor.h:80): the block position is the reference's own look-up
/// (ssb_get_l_first / ssb_get_k_first, ssb_mapping.h), everything else -- PBCH encoding and modulation, its DM-RS, PSS and SSS -- is one
/// device pass; the 4 x 240 REs of the block come back and are put on every port of the PDU.
class ssb_processor_hip : public srsran::ssb_processor
{
public:
  explicit ssb_processor_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void process(srsran::resource_grid_writer& grid, const pdu_t& pdu) override
  {
    const unsigned l_in_burst = srsran::ssb_get_l_first(pdu.pattern_case, pdu.ssb_idx);
    const unsigned l_start    = l_in_burst % srsran::get_nsymb_per_slot(srsran::cyclic_prefix::NORMAL);
    const unsigned k_start    = srsran::ssb_get_k_first(srsran::to_frequency_range(pdu.pattern_case), srsran::to_subcarrier_spacing(pdu.pattern_case), pdu.common_scs,
                                                     pdu.offset_to_pointA, pdu.subcarrier_offset);
    srsran_assert((l_in_burst / srsran::get_nsymb_per_slot(srsran::cyclic_prefix::NORMAL)) == pdu.slot.hrf_slot_index(), "Invalid slot index ({}) for SSB index {}",
                  pdu.slot.hrf_slot_index(), l_in_burst);
    // staging grid: one port, just wide enough for the block
    const unsigned nprb = (k_start + 240 + 11) / 12, nsc = nprb * 12;
    miphy_ssb_pdu  p    = {};
    p.msg.N_id = pdu.phys_cell_id, p.msg.ssb_idx = pdu.ssb_idx, p.msg.L_max = pdu.L_max, p.msg.hrf = pdu.slot.is_odd_hrf() ? 1 : 0, p.msg.sfn = pdu.slot.sfn();
    p.msg.k_ssb = pdu.subcarrier_offset.to_uint();
    for (unsigned i = 0; i != 32 && i != pdu.bch_payload.size(); ++i) {
      p.msg.payload[i] = pdu.bch_payload[i];
    }
    p.ssb_first_subcarrier = k_start, p.ssb_first_symbol = l_start, p.beta_pss_dB = pdu.beta_pss, p.grid_nof_prb = nprb < 20 ? 20 : nprb;
    p.nof_ports = 1, p.ports[0] = 0;
    const unsigned nsc_g = p.grid_nof_prb * 12;
    (void)nsc;
    host.assign(static_cast<size_t>(14) * nsc_g, srsran::cf_t(NAN, NAN));
    auto* d_g = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_ssb_process_batch(c->ctx, &p, 1, d_g, c->stream), "ssb_process");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned port : pdu.ports) {
      put_written_res(grid, port, nsc_g, host.data());
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host;
};

/// Replaces create_ssb_processor_factory_sw(config) (channel_processor_factories.h:293-301).
class ssb_processor_factory_hip : public srsran::ssb_processor_factory
{
public:
  explicit ssb_processor_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::ssb_processor>     create() override { return std::make_unique<ssb_processor_hip>(c); }
  std::unique_ptr<srsran::ssb_pdu_validator> create_validator() override; // defined at the end of this header

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- NZP-CSI-RS generator
/// srsran::nzp_csi_rs_generator over miphy_csi_rs_map_batch (nzp_csi_rs_generator.h:91): the per-port patterns are the reference's own
/// get_csi_rs_pattern() (TS 38.211 Table 7.4.1.5.3-1 bookkeeping), sequence generation, CDM weights and RE mapping run on the device.
class nzp_csi_rs_generator_hip : public srsran::nzp_csi_rs_generator
{
public:
  explicit nzp_csi_rs_generator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void map(srsran::resource_grid_writer& grid, const config_t& config) override
  {
    const unsigned nof_ports = config.ports.size();
    srsran_assert(config.pmi == 0, "Precoding is not currently supported");
    srsran_assert(nof_ports >= 1 && nof_ports <= 16, "Invalid number of ports.");
    srsran::csi_rs_pattern_configuration pc;
    pc.start_rb = config.start_rb, pc.nof_rb = config.nof_rb, pc.csi_rs_mapping_table_row = config.csi_rs_mapping_table_row;
    pc.freq_allocation_ref_idx = config.freq_allocation_ref_idx, pc.symbol_l0 = config.symbol_l0, pc.symbol_l1 = config.symbol_l1;
    pc.cdm = config.cdm, pc.freq_density = config.freq_density, pc.nof_ports = nof_ports;
    const srsran::csi_rs_pattern pat = srsran::get_csi_rs_pattern(pc);
    const unsigned               nprb = config.start_rb + config.nof_rb, nsc = nprb * 12;
    miphy_csi_rs_job             j    = {};
    j.slot_in_frame = config.slot.slot_index(), j.scrambling_id = config.scrambling_id, j.amplitude = config.amplitude;
    j.start_rb = config.start_rb, j.nof_rb = config.nof_rb, j.rb_begin = pat.rb_begin, j.rb_end = std::min<unsigned>(pat.rb_end, nprb), j.rb_stride = pat.rb_stride;
    j.grid_nof_prb = nprb, j.mapping_row = config.csi_rs_mapping_table_row, j.cdm = static_cast<uint8_t>(config.cdm);
    j.freq_density = static_cast<uint8_t>(config.freq_density), j.nof_ports = nof_ports;
    for (unsigned p = 0; p != nof_ports; ++p) {
      j.ports[p] = p; // staging grid indexed by CSI-RS port
      for (unsigned k = 0; k != 12; ++k) {
        j.re_mask[p] |= static_cast<uint16_t>(pat.prb_patterns[p].re_mask.test(k) ? (1U << k) : 0U);
      }
      for (unsigned l = 0; l != 14; ++l) {
        j.symbol_mask[p] |= static_cast<uint16_t>(pat.prb_patterns[p].symbol_mask.test(l) ? (1U << l) : 0U);
      }
    }
    host.assign(static_cast<size_t>(nof_ports) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernel"
    auto* d_g = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    context::check(miphy_csi_rs_map_batch(c->ctx, &j, 0, 1, d_g, c->stream), "csi_rs_map");
    c->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    c->sync();
    for (unsigned p = 0; p != nof_ports; ++p) {
      put_written_res(grid, config.ports[p], nsc, host.data() + static_cast<size_t>(p) * 14 * nsc);
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host;
};

/// Replaces create_nzp_csi_rs_generator_factory_sw(prg) (signal_processor_factories.h:81-82).
class nzp_csi_rs_generator_factory_hip : public srsran::nzp_csi_rs_generator_factory
{
public:
  explicit nzp_csi_rs_generator_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::nzp_csi_rs_generator>               create() override { return std::make_unique<nzp_csi_rs_generator_hip>(c); }
  std::unique_ptr<srsran::nzp_csi_rs_configuration_validator> create_validator() override; // defined at the end of this header

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- downlink processor
/// srsran::downlink_processor (downlink_processor.h:45-111, lib/phy/upper/downlink_processor_single_executor_impl.cpp:54-199) that
/// batches the PDSCH PDUs of a slot: process_pdsch() queues, finish_processing_pdus() -- the reference's own end-of-slot call --
/// runs miphy_pdsch_process_batch over the one-layer PDUs, miphy_pdsch_process_layers_batch over those of two to four layers and, behind
/// the mapped ones, miphy_pdsch_process_codewords_batch over those of two codewords on five to eight layers, on
/// the same device grid (transport blocks up once, written REs down once), puts the REs into the grid
/// and sends it through the gateway. PDCCH, SSB and CSI-RS go to the CPU processors given at construction, at once. Same
/// observable behaviour as the reference processor with its executor: nothing happens without a configured grid, the grid is zeroed
/// on configuration and sent exactly once, after finish_processing_pdus(). Like the reference (downlink_processor_single_executor_impl
/// hands every PDU to an executor and sends the grid from there when the last one is done) the call returns at once: a completion
/// thread owned by the processor runs the batch, writes the resource elements and calls the gateway; is_reserved() stays true until
/// the grid has been sent, which is what the processor pool looks at before it hands the processor out again.
class downlink_processor_hip : public srsran::downlink_processor
{
public:
  downlink_processor_hip(std::shared_ptr<context>                      c,
                         srsran::upper_phy_rg_gateway&                 gateway,
                         std::unique_ptr<srsran::pdcch_processor>      pdcch,
                         std::unique_ptr<srsran::ssb_processor>        ssb,
                         std::unique_ptr<srsran::nzp_csi_rs_generator> csi_rs,
                         unsigned                                      grid_nof_ports,
                         unsigned                                      grid_nof_prb) :
    c(std::move(c)), gateway(gateway), pdcch(std::move(pdcch)), ssb(std::move(ssb)), csi_rs(std::move(csi_rs)), nports(grid_nof_ports), nprb(grid_nof_prb)
  {
    wc     = std::make_shared<context>(this->c->device); // the completion thread drives the caller's device through its own context and stream
    worker = std::thread([this] { completion_loop(); });
  }

  void process_pdcch(const srsran::pdcch_processor::pdu_t& pdu) override
  {
    if (grid == nullptr) {
      return;
    }
    srsran_assert(pdcch, "A PDCCH processor is required.");
    srsran::resource_grid_mapper mapper(*grid);
    pdcch->process(mapper, pdu);
  }
  void process_ssb(const srsran::ssb_processor::pdu_t& pdu) override
  {
    if (grid == nullptr) {
      return;
    }
    srsran_assert(ssb, "An SSB processor is required.");
    ssb->process(*grid, pdu);
  }
  void process_nzp_csi_rs(const srsran::nzp_csi_rs_generator::config_t& config) override
  {
    if (grid == nullptr) {
      return;
    }
    srsran_assert(csi_rs, "A CSI-RS generator is required.");
    csi_rs->map(*grid, config);
  }
  void process_pdsch(const srsran::static_vector<srsran::span<const uint8_t>, srsran::pdsch_processor::MAX_NOF_TRANSPORT_BLOCKS>& data,
                     const srsran::pdsch_processor::pdu_t&                                                                        pdu) override
  {
    if (grid == nullptr) {
      return;
    }
    // The PDU validator of the factory rejects these up front (pdsch_pdu_validator_hip); a caller that skips it fails loudly here
    // also in release builds.
    require((pdu.ports.size() >= 1 && pdu.ports.size() <= 4 && pdu.codewords.size() == 1 && data.size() == 1) ||
                (pdu.ports.size() >= 5 && pdu.ports.size() <= 8 && pdu.codewords.size() == 2 && data.size() == 2),
            "Only one codeword on one to four layers or two codewords on five to eight layers are supported.");
    require(pdu.dmrs == srsran::dmrs_type::TYPE1, "Only DM-RS Type 1 is currently supported.");
    require(pdu.freq_alloc.is_contiguous() || prb_list_obeys_list_rule(pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb),
                                                                       pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb)),
            "The PRB list of the allocation names a PRB twice or one outside its mask.");
    for (uint8_t port : pdu.ports) {
      require(port < nports, "Transmit port outside the resource grid.");
    }
    queue.push_back(entry{data[0], pdu, data.size() == 2 ? data[1] : srsran::span<const uint8_t>()});
  }
  void configure_resource_grid(const srsran::resource_grid_context& context, srsran::resource_grid& grid_) override
  {
    require(!reserved.load(std::memory_order_acquire) && queue.empty(), "Reusing downlink processor that it is still processing PDUs.");
    rg_context = context;
    grid       = &grid_;
    grid->set_all_zero();
    reserved.store(true, std::memory_order_release);
  }
  void finish_processing_pdus() override
  {
    if (grid == nullptr) {
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mtx);
      pending = true; // the completion thread takes the queue, the grid and the context from here
    }
    cv.notify_all();
  }
  /// True from configure_resource_grid() until the completion thread has sent the grid.
  bool is_reserved() const override { return reserved.load(std::memory_order_acquire); }
  /// Blocks until the grid of the last finish_processing_pdus() has been sent (tests, shutdown).
  void wait_sent()
  {
    std::unique_lock<std::mutex> lk(mtx);
    cv.wait(lk, [this] { return !pending; });
  }
  ~downlink_processor_hip() override
  {
    {
      std::lock_guard<std::mutex> lk(mtx);
      stop = true;
    }
    cv.notify_all();
    if (worker.joinable()) {
      worker.join();
    }
  }

private:
  void completion_loop()
  {
    wc->bind_thread(); // a new thread starts on device 0
    std::unique_lock<std::mutex> lk(mtx);
    for (;;) {
      cv.wait(lk, [this] { return pending || stop; });
      if (pending) {
        lk.unlock();
        run_pdsch_batch();
        gateway.send(rg_context, *grid);
        lk.lock();
        // Everything of this slot is cleared BEFORE the reservation is released: once is_reserved() reads false the pool may hand the
        // processor out again, and the next slot's configure_resource_grid() / finish_processing_pdus() set `grid` and `pending` anew --
        // nothing written here may come after that.
        grid    = nullptr;
        pending = false;
        reserved.store(false, std::memory_order_release);
        cv.notify_all();
        continue;
      }
      if (stop) {
        return;
      }
    }
  }
  void run_pdsch_batch()
  {
    if (queue.empty()) {
      return;
    }
    const unsigned                      n = queue.size(), nsc = nprb * 12;
    std::vector<miphy_pdsch_pdu>        pdus;  // one layer
    std::vector<miphy_pdsch_layers_pdu> lpdus; // two to four layers
    std::vector<miphy_pdsch_mapped_pdu> mpdus; // an allocation that is not contiguous or is interleaved, one to four layers ...
    std::vector<uint16_t>               lists; // ... and their PRBs in mapping order (rb_allocation::get_prb_indices)
    std::vector<miphy_pdsch_codewords_pdu> cpdus; // two codewords on five to eight layers, with a list of their own array where not contiguous
    std::vector<uint16_t>                  clists;
    std::vector<size_t>                 tb_offset(n), tb1_offset(n);
    size_t                              tb_bytes = 0;
    pdus.reserve(n), lpdus.reserve(n), mpdus.reserve(n), cpdus.reserve(n);
    for (unsigned i = 0; i != n; ++i) {
      const srsran::pdsch_processor::pdu_t&        pdu = queue[i].pdu;
      const srsran::bounded_bitset<srsran::MAX_RB> prb = pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb);
      srsran_assert(prb.size() <= nprb, "The allocation exceeds the resource grid.");
      const unsigned nlayers = pdu.ports.size();
      const bool     two     = pdu.codewords.size() == 2;
      const bool     mapped  = !two && !pdu.freq_alloc.is_contiguous();
      if (two) {
        miphy_pdsch_codewords_pdu cp = {};
        cp.nof_layers                = nlayers;
        std::copy(pdu.ports.begin(), pdu.ports.end(), cp.ports);
        if (!pdu.freq_alloc.is_contiguous()) {
          const srsran::static_vector<uint16_t, srsran::MAX_RB> list = pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb);
          cp.mapped.prb_list_offset = clists.size(), cp.mapped.nof_prb = list.size();
          clists.insert(clists.end(), list.begin(), list.end());
        }
        cpdus.push_back(cp);
      } else if (mapped) {
        const srsran::static_vector<uint16_t, srsran::MAX_RB> list = pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb);
        miphy_pdsch_mapped_pdu                                mp   = {};
        mp.layers.nof_layers = nlayers, mp.prb_list_offset = lists.size(), mp.nof_prb = list.size();
        std::copy(pdu.ports.begin(), pdu.ports.end(), mp.layers.ports);
        lists.insert(lists.end(), list.begin(), list.end());
        mpdus.push_back(mp);
      } else if (nlayers == 1) {
        pdus.push_back(miphy_pdsch_pdu{});
      } else {
        miphy_pdsch_layers_pdu lp = {};
        lp.nof_layers             = nlayers;
        std::copy(pdu.ports.begin(), pdu.ports.end(), lp.ports);
        lpdus.push_back(lp);
      }
      miphy_pdsch_pdu& p = two ? cpdus.back().mapped.layers.base : mapped ? mpdus.back().layers.base : (nlayers == 1 ? pdus.back() : lpdus.back().base);
      p.slot_in_frame = pdu.slot.slot_index(), p.rnti = pdu.rnti, p.n_id = pdu.n_id, p.dmrs_scrambling_id = pdu.scrambling_id;
      p.tbs_lbrm_bytes = pdu.tbs_lbrm_bytes, p.tb_bytes = queue[i].data.size();
      p.ratio_pdsch_dmrs_to_sss_dB = pdu.ratio_pdsch_dmrs_to_sss_dB, p.ratio_pdsch_data_to_sss_dB = pdu.ratio_pdsch_data_to_sss_dB;
      p.bg = bg_id(pdu.ldpc_base_graph), p.rv = pdu.codewords[0].rv, p.mod = srsran::get_bits_per_symbol(pdu.codewords[0].modulation);
      p.port = pdu.ports[0];
      p.start_symbol = pdu.start_symbol_index, p.nof_symbols = pdu.nof_symbols, p.nof_cdm_groups_without_data = pdu.nof_cdm_groups_without_data;
      p.n_scid = pdu.n_scid ? 1 : 0, p.ref_point_prb0 = (pdu.ref_point == srsran::pdsch_processor::pdu_t::PRB0) ? 1 : 0;
      p.grid_nof_prb = nprb, p.bwp_start_rb = pdu.bwp_start_rb, p.bwp_size_rb = pdu.bwp_size_rb;
      for (unsigned l = 0; l != 14 && l != pdu.dmrs_symbol_mask.size(); ++l) {
        if (pdu.dmrs_symbol_mask.test(l)) {
          p.dmrs_symbols_mask |= static_cast<uint16_t>(1U << l);
        }
      }
      prb.for_each(0, prb.size(), [&p](unsigned r) { p.rb_mask[r >> 6] |= 1ULL << (r & 63); });
      p.nof_reserved = reserved_rectangles(pdu.reserved, prb.size(), p.reserved);
      p.tb_offset = tb_bytes, p.grid_offset = 0;
      tb_offset[i] = tb_bytes;
      tb_bytes += (queue[i].data.size() + 15) & ~static_cast<size_t>(15);
      if (two) { // transport block 1 behind block 0
        pdsch_processor_hip::second_block_of(pdu, queue[i].data1.size(), tb_bytes, cpdus.back());
        tb1_offset[i] = tb_bytes;
        tb_bytes += (queue[i].data1.size() + 15) & ~static_cast<size_t>(15);
      }
    }
    tbs.assign(tb_bytes + 16, 0);
    for (unsigned i = 0; i != n; ++i) {
      std::memcpy(&tbs[tb_offset[i]], queue[i].data.data(), queue[i].data.size());
      if (!queue[i].data1.empty()) {
        std::memcpy(&tbs[tb1_offset[i]], queue[i].data1.data(), queue[i].data1.size());
      }
    }
    host.assign(static_cast<size_t>(nports) * 14 * nsc, srsran::cf_t(NAN, NAN)); // NaN marks "not written by the kernels"
    auto* d_tb = static_cast<uint8_t*>(wc->buf(0, tbs.size()));
    auto* d_g  = static_cast<float*>(wc->buf(1, host.size() * sizeof(srsran::cf_t)));
    wc->h2d(d_tb, tbs.data(), tbs.size());
    wc->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    if (!pdus.empty()) {
      context::check(miphy_pdsch_process_batch(wc->ctx, pdus.data(), pdus.size(), d_tb, d_g, wc->stream), "pdsch_process");
    }
    if (!lpdus.empty()) {
      context::check(miphy_pdsch_process_layers_batch(wc->ctx, lpdus.data(), lpdus.size(), d_tb, d_g, wc->stream), "pdsch_process_layers");
    }
    if (!mpdus.empty()) {
      context::check(miphy_pdsch_process_mapped_batch(wc->ctx, mpdus.data(), mpdus.size(), lists.data(), lists.size(), d_tb, d_g, wc->stream),
                     "pdsch_process_mapped");
    }
    if (!cpdus.empty()) { // one more batch behind the others, on the same grid and stream
      context::check(miphy_pdsch_process_codewords_batch(wc->ctx, cpdus.data(), cpdus.size(), clists.data(), clists.size(), d_tb, d_g, wc->stream),
                     "pdsch_process_codewords");
    }
    wc->d2h(host.data(), d_g, host.size() * sizeof(srsran::cf_t));
    wc->sync();
    for (unsigned p = 0; p != nports; ++p) {
      put_written_res(*grid, p, nsc, host.data() + static_cast<size_t>(p) * 14 * nsc);
    }
    queue.clear();
  }

  struct entry {
    srsran::span<const uint8_t>    data;
    srsran::pdsch_processor::pdu_t pdu;
    srsran::span<const uint8_t>    data1; // transport block 1 of a two-codeword PDU, empty otherwise
  };
  std::shared_ptr<context>                      c;
  srsran::upper_phy_rg_gateway&                 gateway;
  std::unique_ptr<srsran::pdcch_processor>      pdcch;
  std::unique_ptr<srsran::ssb_processor>        ssb;
  std::unique_ptr<srsran::nzp_csi_rs_generator> csi_rs;
  unsigned                                      nports, nprb;
  srsran::resource_grid_context                 rg_context = {};
  srsran::resource_grid*                        grid       = nullptr;
  std::vector<entry>                            queue;
  std::vector<uint8_t>                          tbs;
  std::vector<srsran::cf_t>                     host;
  std::atomic<bool>                             reserved{false};
  std::mutex                                    mtx;
  std::condition_variable                       cv;
  bool                                          pending = false, stop = false;
  std::shared_ptr<context>                      wc;
  std::thread                                   worker; // started at the end of the constructor
};

/// A downlink processor whose four PDU types all run on the device: PDSCH batched per slot, PDCCH / SSB / CSI-RS through the
/// device processors above (replaces the pool entry downlink_processor_single_executor_factory::create builds, upper_phy_factories.cpp:269-300).
inline std::unique_ptr<srsran::downlink_processor>
create_downlink_processor_hip(std::shared_ptr<context> c, srsran::upper_phy_rg_gateway& gateway, unsigned grid_nof_ports, unsigned grid_nof_prb)
{
  return std::make_unique<downlink_processor_hip>(c, gateway, std::make_unique<pdcch_processor_hip>(c), std::make_unique<ssb_processor_hip>(c),
                                                  std::make_unique<nzp_csi_rs_generator_hip>(c), grid_nof_ports, grid_nof_prb);
}

// ---------------------------------------------------------------------------------------------------------------- Open Fronthaul IQ compression
/// srsran::ofh::iq_decompressor / iq_compressor for compression_type::BFP and compression_type::none over miphy_ofh_iq_*_batch
/// (iq_decompressor.h:49-50, iq_compressor.h:49-50): what iq_{de}compressor_selector dispatches to for the two methods the reference
/// implements. The compressed_prb objects are laid out as the U-plane section payload ([udCompParam][packed IQ] per PRB for BFP,
/// the packed IQ alone for the uncompressed format) on the way to and from the device.
class iq_compression_hip : public srsran::ofh::iq_compressor, public srsran::ofh::iq_decompressor
{
public:
  explicit iq_compression_hip(std::shared_ptr<context> c, float iq_scaling = 1.0F) : c(std::move(c)), iq_scaling(iq_scaling) {}
  void compress(srsran::span<srsran::ofh::compressed_prb> output, srsran::span<const srsran::cf_t> input, const srsran::ofh::ru_compression_params& params) override
  {
    srsran_assert(input.size() == output.size() * 12, "Wrong number of input samples.");
    const uint16_t comp = method(params);
    const unsigned w = params.data_width, hdr = comp == MIPHY_OFH_COMPRESSION_BFP ? 1 : 0, rec = hdr + 3 * w, nprb = output.size();
    if (nprb == 0) {
      return;
    }
    auto* d_x = static_cast<float*>(c->buf(0, input.size() * sizeof(srsran::cf_t)));
    auto* d_p = static_cast<uint8_t*>(c->buf(1, static_cast<size_t>(nprb) * rec));
    bytes.resize(static_cast<size_t>(nprb) * rec);
    c->h2d(d_x, input.data(), input.size() * sizeof(srsran::cf_t));
    srsran_assert(nprb <= 275, "At most 275 PRBs per call.");
    miphy_ofh_iq_job job{0, 0, nprb, static_cast<uint16_t>(w), comp};
    context::check(miphy_ofh_iq_compress_batch(c->ctx, &job, 0, 1, d_x, iq_scaling, d_p, c->stream), "ofh_iq_compress");
    c->d2h(bytes.data(), d_p, bytes.size());
    c->sync();
    for (unsigned p = 0; p != nprb; ++p) {
      if (hdr != 0) {
        output[p].set_compression_param(bytes[static_cast<size_t>(p) * rec]);
      }
      std::memcpy(output[p].get_buffer().data(), &bytes[static_cast<size_t>(p) * rec + hdr], 3 * w);
      output[p].set_stored_size(3 * w);
    }
  }
  void decompress(srsran::span<srsran::cf_t> output, srsran::span<const srsran::ofh::compressed_prb> input, const srsran::ofh::ru_compression_params& params) override
  {
    srsran_assert(output.size() == input.size() * 12, "Wrong number of output samples.");
    const uint16_t comp = method(params);
    const unsigned w = params.data_width, hdr = comp == MIPHY_OFH_COMPRESSION_BFP ? 1 : 0, rec = hdr + 3 * w, nprb = input.size();
    if (nprb == 0) {
      return;
    }
    srsran_assert(nprb <= 275, "At most 275 PRBs per call.");
    bytes.resize(static_cast<size_t>(nprb) * rec);
    for (unsigned p = 0; p != nprb; ++p) {
      if (hdr != 0) {
        bytes[static_cast<size_t>(p) * rec] = input[p].get_compression_param();
      }
      // get_packed_data() depends on set_stored_size(), which the U-plane decoder does not call: take the bytes themselves
      std::memcpy(&bytes[static_cast<size_t>(p) * rec + hdr], const_cast<srsran::ofh::compressed_prb&>(input[p]).get_buffer().data(), 3 * w);
    }
    auto* d_p = static_cast<uint8_t*>(c->buf(0, bytes.size()));
    auto* d_x = static_cast<float*>(c->buf(1, output.size() * sizeof(srsran::cf_t)));
    c->h2d(d_p, bytes.data(), bytes.size());
    miphy_ofh_iq_job job{0, 0, nprb, static_cast<uint16_t>(w), comp};
    context::check(miphy_ofh_iq_decompress_batch(c->ctx, &job, 0, 1, d_p, d_x, 1, c->stream), "ofh_iq_decompress");
    c->d2h(output.data(), d_x, output.size() * sizeof(srsran::cf_t));
    c->sync();
  }

private:
  static uint16_t method(const srsran::ofh::ru_compression_params& params)
  {
    if (params.type == srsran::ofh::compression_type::BFP) {
      return MIPHY_OFH_COMPRESSION_BFP;
    }
    if (params.type == srsran::ofh::compression_type::none) {
      return MIPHY_OFH_COMPRESSION_NONE;
    }
    srsran::report_fatal_error("Compression of {} type is not implemented", srsran::ofh::to_string(params.type));
  }

  std::shared_ptr<context> c;
  float                    iq_scaling;
  std::vector<uint8_t>     bytes;
};

/// Replace create_iq_compressor(type, iq_scaling, impl) and create_iq_decompressor(type, impl) for type = none | BFP, or the
/// selectors built from them (compression_factory.h:36-50).
inline std::unique_ptr<srsran::ofh::iq_compressor> create_iq_compressor_hip(std::shared_ptr<context> c, float iq_scaling = 1.0F)
{
  return std::make_unique<iq_compression_hip>(std::move(c), iq_scaling);
}
inline std::unique_ptr<srsran::ofh::iq_decompressor> create_iq_decompressor_hip(std::shared_ptr<context> c)
{
  return std::make_unique<iq_compression_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- PDCCH
/// srsran::pdcch_encoder over miphy_pdcch_encode_batch (pdcch_encoder.h:53).
class pdcch_encoder_hip : public srsran::pdcch_encoder
{
public:
  explicit pdcch_encoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void encode(srsran::span<uint8_t> encoded, srsran::span<const uint8_t> data, const config_t& config) override
  {
    srsran_assert(encoded.size() >= config.E, "Output data vector is too small to store encoded bits");
    auto*    d_in  = static_cast<uint8_t*>(c->buf(0, data.size() + 16));
    auto*    d_out = static_cast<uint8_t*>(c->buf(1, config.E));
    uint16_t rnti  = static_cast<uint16_t>(config.rnti);
    auto*    d_rn  = reinterpret_cast<uint16_t*>(d_in + ((data.size() + 7) / 8) * 8);
    c->h2d(d_in, data.data(), data.size());
    c->h2d(d_rn, &rnti, sizeof(rnti));
    context::check(miphy_pdcch_encode_batch(c->ctx, data.size(), config.E, 1, d_in, d_rn, d_out, c->stream), "pdcch_encode");
    c->d2h(encoded.data(), d_out, config.E);
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- factories
#define MIPHY_SIMPLE_FACTORY(NAME, BASE, PRODUCT, IMPL)                                        \
  class NAME : public srsran::BASE                                                             \
  {                                                                                            \
  public:                                                                                      \
    explicit NAME(std::shared_ptr<context> c) : c(std::move(c)) {}                             \
    std::unique_ptr<srsran::PRODUCT> create() override { return std::make_unique<IMPL>(c); }   \
                                                                                               \
  private:                                                                                     \
    std::shared_ptr<context> c;                                                                \
  };

MIPHY_SIMPLE_FACTORY(ldpc_decoder_factory_hip, ldpc_decoder_factory, ldpc_decoder, ldpc_decoder_hip)
MIPHY_SIMPLE_FACTORY(ldpc_encoder_factory_hip, ldpc_encoder_factory, ldpc_encoder, ldpc_encoder_hip)
MIPHY_SIMPLE_FACTORY(ldpc_rate_matcher_factory_hip, ldpc_rate_matcher_factory, ldpc_rate_matcher, ldpc_rate_matcher_hip)
MIPHY_SIMPLE_FACTORY(ldpc_rate_dematcher_factory_hip, ldpc_rate_dematcher_factory, ldpc_rate_dematcher, ldpc_rate_dematcher_hip)
MIPHY_SIMPLE_FACTORY(pdsch_encoder_factory_hip, pdsch_encoder_factory, pdsch_encoder, pdsch_encoder_hip)
MIPHY_SIMPLE_FACTORY(pusch_decoder_factory_hip, pusch_decoder_factory, pusch_decoder, pusch_decoder_hip)
/// \c separate_layers, \c compensate_cfo and \c time as in dmrs_pusch_estimator_hip.
class dmrs_pusch_estimator_factory_hip : public srsran::dmrs_pusch_estimator_factory
{
public:
  explicit dmrs_pusch_estimator_factory_hip(std::shared_ptr<context> c, bool separate_layers = false, bool compensate_cfo = false,
                                            time_strategy time = time_strategy::average) :
    c(std::move(c)), separate_layers(separate_layers), compensate_cfo(compensate_cfo), time(time)
  {
  }
  std::unique_ptr<srsran::dmrs_pusch_estimator> create() override
  {
    return std::make_unique<dmrs_pusch_estimator_hip>(c, separate_layers, compensate_cfo, time);
  }

private:
  std::shared_ptr<context> c;
  bool                     separate_layers, compensate_cfo;
  time_strategy            time;
};
MIPHY_SIMPLE_FACTORY(pdcch_encoder_factory_hip, pdcch_encoder_factory, pdcch_encoder, pdcch_encoder_hip)
MIPHY_SIMPLE_FACTORY(pusch_demodulator_factory_hip, pusch_demodulator_factory, pusch_demodulator, pusch_demodulator_hip)
MIPHY_SIMPLE_FACTORY(pdsch_modulator_factory_hip, pdsch_modulator_factory, pdsch_modulator, pdsch_modulator_hip)
MIPHY_SIMPLE_FACTORY(dmrs_pdsch_processor_factory_hip, dmrs_pdsch_processor_factory, dmrs_pdsch_processor, dmrs_pdsch_processor_hip)
MIPHY_SIMPLE_FACTORY(short_block_detector_factory_hip, short_block_detector_factory, short_block_detector, short_block_detector_hip)
#undef MIPHY_SIMPLE_FACTORY

/// The UCI decoders of one factory share the list size of their polar decoder (see uci_decoder_hip).
class uci_decoder_factory_hip : public srsran::uci_decoder_factory
{
public:
  explicit uci_decoder_factory_hip(std::shared_ptr<context> c, unsigned list_size = 1) : c(std::move(c)), list_size(list_size) {}
  std::unique_ptr<srsran::uci_decoder> create() override { return std::make_unique<uci_decoder_hip>(c, list_size); }

private:
  std::shared_ptr<context> c;
  unsigned                 list_size;
};

/// The string-selected factory functions of the reference (channel_coding_factories.cpp:86-180) gain a "hip" case that
/// returns these.
inline std::shared_ptr<srsran::ldpc_decoder_factory> create_ldpc_decoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<ldpc_decoder_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::ldpc_encoder_factory> create_ldpc_encoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<ldpc_encoder_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::ldpc_rate_matcher_factory> create_ldpc_rate_matcher_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<ldpc_rate_matcher_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::ldpc_rate_dematcher_factory> create_ldpc_rate_dematcher_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<ldpc_rate_dematcher_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::pdsch_encoder_factory> create_pdsch_encoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<pdsch_encoder_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::pusch_decoder_factory> create_pusch_decoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<pusch_decoder_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::dmrs_pusch_estimator_factory> create_dmrs_pusch_estimator_factory_hip(std::shared_ptr<context> c, bool separate_layers = false,
                                                                                                     bool compensate_cfo = false,
                                                                                                     time_strategy time = time_strategy::average)
{
  return std::make_shared<dmrs_pusch_estimator_factory_hip>(std::move(c), separate_layers, compensate_cfo, time);
}
inline std::shared_ptr<srsran::pdcch_encoder_factory> create_pdcch_encoder_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<pdcch_encoder_factory_hip>(std::move(c));
}
/// Replace create_pdsch_modulator_factory_sw(modulation, prg) (channel_processor_factories.h:140-142) and
/// create_dmrs_pdsch_processor_factory_sw(prg) (signal_processor_factories.h:46-47).
inline std::shared_ptr<srsran::pdsch_modulator_factory> create_pdsch_modulator_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<pdsch_modulator_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::dmrs_pdsch_processor_factory> create_dmrs_pdsch_processor_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<dmrs_pdsch_processor_factory_hip>(std::move(c));
}
/// Replaces create_pusch_demodulator_factory_sw(equalizer, demodulation, prg) (channel_processor_factories.h:256-259).
inline std::shared_ptr<srsran::pusch_demodulator_factory> create_pusch_demodulator_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<pusch_demodulator_factory_hip>(std::move(c));
}
/// Replace create_short_block_detector_factory_sw() and create_uci_decoder_factory_sw(config) (channel_coding_factories.h:123-130,
/// channel_processor_factories.h:303-314); pass the UCI decoder factory to pusch_processor_factory_hip / uplink_processor_hip.
inline std::shared_ptr<srsran::short_block_detector_factory> create_short_block_detector_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<short_block_detector_factory_hip>(std::move(c));
}
inline std::shared_ptr<srsran::uci_decoder_factory> create_uci_decoder_factory_hip(std::shared_ptr<context> c, unsigned list_size = 1)
{
  return std::make_shared<uci_decoder_factory_hip>(std::move(c), list_size);
}

/// OFDM factories take a configuration per product (modulation_factories.h:34-76).
class ofdm_demodulator_factory_hip : public srsran::ofdm_demodulator_factory
{
public:
  explicit ofdm_demodulator_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::ofdm_symbol_demodulator> create_ofdm_symbol_demodulator(const srsran::ofdm_demodulator_configuration& cfg) override
  {
    return std::make_unique<ofdm_symbol_demodulator_hip>(c, cfg);
  }
  std::unique_ptr<srsran::ofdm_slot_demodulator> create_ofdm_slot_demodulator(const srsran::ofdm_demodulator_configuration& cfg) override
  {
    return std::make_unique<ofdm_slot_demodulator_hip>(c, cfg);
  }

private:
  std::shared_ptr<context> c;
};

class ofdm_modulator_factory_hip : public srsran::ofdm_modulator_factory
{
public:
  explicit ofdm_modulator_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::ofdm_symbol_modulator> create_ofdm_symbol_modulator(const srsran::ofdm_modulator_configuration& cfg) override
  {
    return std::make_unique<ofdm_symbol_modulator_hip>(c, cfg);
  }
  std::unique_ptr<srsran::ofdm_slot_modulator>   create_ofdm_slot_modulator(const srsran::ofdm_modulator_configuration& cfg) override
  {
    return std::make_unique<ofdm_slot_modulator_hip>(c, cfg);
  }

private:
  std::shared_ptr<context> c;
};

// ---------------------------------------------------------------------------------------------------------------- polar blocks
/// The block-level polar interfaces over miphy_polar_block_batch (include/srsran/phy/upper/channel_coding/polar/*.h), a batch of one
/// per call, so that the reference's own chains (pdcch_encoder_impl, pbch_encoder_impl, uci decoders, polar_chain_test.cpp:156-210)
/// run on the device block by block. polar_code stays the reference's host class (bookkeeping of sets and tables).
namespace detail {
inline miphy_polar_code to_miphy_code(const srsran::polar_code& code)
{
  miphy_polar_code mc = {code.get_K(), code.get_E(), 10, code.get_ibil() == srsran::polar_code_ibil::present ? 1U : 0U};
  // nMax is not kept by polar_code: it is 10 unless that would give a larger mother code than the one the code object holds
  uint32_t n = 0, N = 0, npc = 0;
  if (miphy_polar_code_info(&mc, &n, &N, &npc) != MIPHY_OK || n != code.get_n()) {
    mc.nMax = 9;
    context::check(miphy_polar_code_info(&mc, &n, &N, &npc), "polar_code_info");
    require(n == code.get_n(), "The polar code object is not a TS 38.212 code (n = {}).", code.get_n());
  }
  return mc;
}
inline void polar_block(context& c, const miphy_polar_code* code, uint32_t op, uint32_t param, void* out, size_t out_bytes, const void* in, size_t in_bytes)
{
  void* d_in  = c.buf(0, in_bytes);
  void* d_out = c.buf(1, out_bytes);
  c.h2d(d_in, in, in_bytes);
  context::check(miphy_polar_block_batch(c.ctx, code, op, param, 1, d_in, d_out, c.stream), "polar_block");
  c.d2h(out, d_out, out_bytes);
  c.sync();
}
} // namespace detail

class polar_allocator_hip : public srsran::polar_allocator
{
public:
  explicit polar_allocator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void allocate(srsran::span<uint8_t> input_encoder, srsran::span<const uint8_t> message, const srsran::polar_code& code) override
  {
    require(input_encoder.size() == code.get_N() && message.size() == code.get_K(), "polar_allocator: wrong sizes");
    const miphy_polar_code mc = detail::to_miphy_code(code);
    detail::polar_block(*c, &mc, MIPHY_POLAR_OP_ALLOCATE, 0, input_encoder.data(), input_encoder.size(), message.data(), message.size());
  }

private:
  std::shared_ptr<context> c;
};

class polar_deallocator_hip : public srsran::polar_deallocator
{
public:
  explicit polar_deallocator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void deallocate(srsran::span<uint8_t> message, srsran::span<const uint8_t> output_decoder, const srsran::polar_code& code) override
  {
    require(output_decoder.size() == code.get_N() && message.size() == code.get_K(), "polar_deallocator: wrong sizes");
    const miphy_polar_code mc = detail::to_miphy_code(code);
    detail::polar_block(*c, &mc, MIPHY_POLAR_OP_DEALLOCATE, 0, message.data(), message.size(), output_decoder.data(), output_decoder.size());
  }

private:
  std::shared_ptr<context> c;
};

class polar_encoder_hip : public srsran::polar_encoder
{
public:
  explicit polar_encoder_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void encode(srsran::span<uint8_t> output, srsran::span<const uint8_t> input, unsigned code_size_log) override
  {
    require(output.size() == (1U << code_size_log) && input.size() == output.size(), "polar_encoder: wrong sizes");
    detail::polar_block(*c, nullptr, MIPHY_POLAR_OP_ENCODE, code_size_log, output.data(), output.size(), input.data(), input.size());
  }

private:
  std::shared_ptr<context> c;
};

class polar_decoder_hip : public srsran::polar_decoder
{
public:
  polar_decoder_hip(std::shared_ptr<context> c, unsigned nMax) : c(std::move(c)), nMax(nMax) {}
  void decode(srsran::span<uint8_t> data_decoded, srsran::span<const srsran::log_likelihood_ratio> input_llr, const srsran::polar_code& code) override
  {
    require(code.get_n() <= nMax, "polar_decoder: code size 2^{} exceeds the decoder's 2^{}", code.get_n(), nMax);
    require(data_decoded.size() == code.get_N() && input_llr.size() == code.get_N(), "polar_decoder: wrong sizes");
    const miphy_polar_code mc = detail::to_miphy_code(code);
    detail::polar_block(*c, &mc, MIPHY_POLAR_OP_DECODE, 0, data_decoded.data(), data_decoded.size(), input_llr.data(), input_llr.size());
  }

private:
  std::shared_ptr<context> c;
  unsigned                 nMax;
};

class polar_rate_matcher_hip : public srsran::polar_rate_matcher
{
public:
  explicit polar_rate_matcher_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void rate_match(srsran::span<uint8_t> output, srsran::span<const uint8_t> input, const srsran::polar_code& code) override
  {
    require(output.size() == code.get_E() && input.size() == code.get_N(), "polar_rate_matcher: wrong sizes");
    const miphy_polar_code mc = detail::to_miphy_code(code);
    detail::polar_block(*c, &mc, MIPHY_POLAR_OP_RATE_MATCH, 0, output.data(), output.size(), input.data(), input.size());
  }

private:
  std::shared_ptr<context> c;
};

class polar_rate_dematcher_hip : public srsran::polar_rate_dematcher
{
public:
  explicit polar_rate_dematcher_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void rate_dematch(srsran::span<srsran::log_likelihood_ratio>       output,
                    srsran::span<const srsran::log_likelihood_ratio> input,
                    const srsran::polar_code&                        code) override
  {
    require(input.size() == code.get_E() && output.size() == code.get_N(), "polar_rate_dematcher: wrong sizes");
    const miphy_polar_code mc = detail::to_miphy_code(code);
    detail::polar_block(*c, &mc, MIPHY_POLAR_OP_RATE_DEMATCH, 0, output.data(), output.size(), input.data(), input.size());
  }

private:
  std::shared_ptr<context> c;
};

class polar_interleaver_hip : public srsran::polar_interleaver
{
public:
  explicit polar_interleaver_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void interleave(srsran::span<uint8_t> out, srsran::span<const uint8_t> in, srsran::polar_interleaver_direction direction) override
  {
    require(in.size() == out.size() && in.size() >= 1 && in.size() <= 164, "polar_interleaver: wrong sizes");
    detail::polar_block(*c, nullptr, direction == srsran::polar_interleaver_direction::tx ? MIPHY_POLAR_OP_INTERLEAVE_TX : MIPHY_POLAR_OP_INTERLEAVE_RX,
                        static_cast<uint32_t>(in.size()), out.data(), out.size(), in.data(), in.size());
  }

private:
  std::shared_ptr<context> c;
};

/// Replaces create_polar_factory_sw() (channel_coding_factories.h:107-121).
class polar_factory_hip : public srsran::polar_factory
{
public:
  explicit polar_factory_hip(std::shared_ptr<context> c) : c(std::move(c)), host(srsran::create_polar_factory_sw()) {}
  std::unique_ptr<srsran::polar_allocator>      create_allocator() override { return std::make_unique<polar_allocator_hip>(c); }
  std::unique_ptr<srsran::polar_code>           create_code() override { return host->create_code(); }
  std::unique_ptr<srsran::polar_deallocator>    create_deallocator() override { return std::make_unique<polar_deallocator_hip>(c); }
  std::unique_ptr<srsran::polar_decoder>        create_decoder(unsigned code_size_log) override { return std::make_unique<polar_decoder_hip>(c, code_size_log); }
  std::unique_ptr<srsran::polar_encoder>        create_encoder() override { return std::make_unique<polar_encoder_hip>(c); }
  std::unique_ptr<srsran::polar_interleaver>    create_interleaver() override { return std::make_unique<polar_interleaver_hip>(c); }
  std::unique_ptr<srsran::polar_rate_dematcher> create_rate_dematcher() override { return std::make_unique<polar_rate_dematcher_hip>(c); }
  std::unique_ptr<srsran::polar_rate_matcher>   create_rate_matcher() override { return std::make_unique<polar_rate_matcher_hip>(c); }

private:
  std::shared_ptr<context>               c;
  std::shared_ptr<srsran::polar_factory> host;
};
inline std::shared_ptr<srsran::polar_factory> create_polar_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<polar_factory_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- CRC calculator
/// srsran::crc_calculator over miphy_crc_batch (crc_calculator.h:45-67); with its factory it fills the hardware seam
/// downlink_processor_factory_hw_config::crc_calc_factory (upper_phy_factories.h:151-161).
class crc_calculator_hip : public srsran::crc_calculator
{
public:
  crc_calculator_hip(std::shared_ptr<context> c, srsran::crc_generator_poly poly) : c(std::move(c)), poly(poly) {}
  srsran::crc_calculator_checksum_t calculate_byte(srsran::span<const uint8_t> data) override { return run(data.data(), data.size(), data.size() * 8); }
  srsran::crc_calculator_checksum_t calculate_bit(srsran::span<const uint8_t> data) override
  {
    packed.assign((data.size() + 7) / 8, 0);
    for (size_t i = 0; i != data.size(); ++i) {
      packed[i >> 3] |= static_cast<uint8_t>((data[i] & 1U) << (7 - (i & 7)));
    }
    return run(packed.data(), packed.size(), data.size());
  }
  srsran::crc_calculator_checksum_t calculate(const srsran::bit_buffer& data) override
  {
    const srsran::span<const uint8_t> bytes = data.get_buffer();
    return run(bytes.data(), bytes.size(), data.size());
  }
  srsran::crc_generator_poly get_generator_poly() const override { return poly; }

private:
  srsran::crc_calculator_checksum_t run(const uint8_t* bytes, size_t nbytes, size_t nbits)
  {
    if (nbits == 0) {
      return 0;
    }
    auto* d_in  = static_cast<uint8_t*>(c->buf(0, nbytes + 8)); // the device CRC reads whole words: keep a zero pad behind the message
    auto* d_out = static_cast<uint32_t*>(c->buf(1, 16));
    context::hip(hipMemsetAsync(d_in + nbytes, 0, 8, c->stream), "memset");
    c->h2d(d_in, bytes, nbytes);
    miphy_crc_desc d = {0, static_cast<uint32_t>(nbits), to_miphy_crc(poly)};
    context::check(miphy_crc_batch(c->ctx, &d, 0, 1, d_in, d_out, c->stream), "crc");
    uint32_t v = 0;
    c->d2h(&v, d_out, sizeof(v));
    c->sync();
    return v;
  }
  std::shared_ptr<context>   c;
  srsran::crc_generator_poly poly;
  std::vector<uint8_t>       packed;
};

class crc_calculator_factory_hip : public srsran::crc_calculator_factory
{
public:
  explicit crc_calculator_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::crc_calculator> create(srsran::crc_generator_poly poly) override
  {
    if (poly == srsran::crc_generator_poly::CRC6) {
      return nullptr; // UCI-only polynomial, not on this path (factories return nullptr for what they do not support)
    }
    return std::make_unique<crc_calculator_hip>(c, poly);
  }

private:
  std::shared_ptr<context> c;
};
inline std::shared_ptr<srsran::crc_calculator_factory> create_crc_calculator_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<crc_calculator_factory_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- port channel estimator
/// srsran::port_channel_estimator over miphy_port_channel_estimate_batch (port_channel_estimator.h:102-106): the pilots come from the
/// caller (PUSCH and PUCCH estimators build them), one receive port per call, all layers, intra-slot frequency hopping included
/// (port_channel_estimator_average_impl.cpp:97-224). DM-RS on every second subcarrier (type 1 / PUCCH formats 1-4 comb); the layers
/// share symbols, PRBs and hop, as in every caller of the reference.
class port_channel_estimator_hip : public srsran::port_channel_estimator
{
public:
  explicit port_channel_estimator_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void compute(srsran::channel_estimate&           estimate,
               const srsran::resource_grid_reader& grid,
               unsigned                            port,
               const srsran::dmrs_symbol_list&     pilots,
               const configuration&                cfg) override
  {
    const unsigned nl = cfg.dmrs_pattern.size();
    require(nl >= 1 && nl <= 4, "port_channel_estimator_hip: 1 to 4 layers.");
    const layer_dmrs_pattern& pt   = cfg.dmrs_pattern[0];
    const unsigned            nprb = pt.rb_mask.size(), nsc = nprb * 12;
    miphy_pusch_chest_job     j    = {};
    j.numerology = srsran::to_numerology_value(cfg.scs), j.scaling = cfg.scaling, j.nof_tx_layers = nl, j.nof_rx_ports = 1;
    j.first_symbol = cfg.first_symbol, j.nof_symbols = cfg.nof_symbols, j.grid_nof_prb = nprb;
    for (unsigned ly = 0; ly != nl; ++ly) {
      const layer_dmrs_pattern& q = cfg.dmrs_pattern[ly];
      require(q.symbols == pt.symbols && q.rb_mask == pt.rb_mask && q.rb_mask2 == pt.rb_mask2 && q.hopping_symbol_index == pt.hopping_symbol_index,
              "port_channel_estimator_hip: the layers must share symbols, PRBs and hop.");
      uint16_t re = 0;
      for (unsigned k = 0; k != 12; ++k) {
        re |= static_cast<uint16_t>(q.re_pattern.test(k) ? (1U << k) : 0U);
      }
      require(re == 0x555 || re == 0xaaa, "port_channel_estimator_hip: DM-RS on every second subcarrier only.");
      j.re_odd_mask |= static_cast<uint8_t>((re == 0xaaa) ? (1U << ly) : 0U);
    }
    for (unsigned l = 0; l != 14 && l != pt.symbols.size(); ++l) {
      j.symbols_mask |= static_cast<uint16_t>(pt.symbols.test(l) ? (1U << l) : 0U);
    }
    pt.rb_mask.for_each(0, nprb, [&j](unsigned r) { j.rb_mask[r >> 6] |= 1ULL << (r & 63); });
    if (pt.hopping_symbol_index.has_value()) {
      j.hop_symbol = pt.hopping_symbol_index.value();
      pt.rb_mask2.for_each(0, pt.rb_mask2.size(), [&j](unsigned r) { j.rb_mask2[r >> 6] |= 1ULL << (r & 63); });
    }
    const unsigned nsymb = cfg.first_symbol + cfg.nof_symbols;
    host.resize(static_cast<size_t>(14) * nsc);
    for (unsigned l = 0; l != 14; ++l) {
      grid.get(srsran::span<srsran::cf_t>(host.data() + static_cast<size_t>(l) * nsc, nsc), port, l, 0);
    }
    const srsran::re_measurement_dimensions pd = pilots.size();
    pil.resize(static_cast<size_t>(nl) * pd.nof_symbols * pd.nof_subc);
    for (unsigned ly = 0; ly != nl; ++ly) {
      for (unsigned d = 0; d != pd.nof_symbols; ++d) {
        srsran::span<const srsran::cf_t> v = pilots.get_symbol(d, ly);
        std::copy(v.begin(), v.end(), pil.begin() + (static_cast<size_t>(ly) * pd.nof_symbols + d) * pd.nof_subc);
      }
    }
    auto* d_g  = static_cast<float*>(c->buf(0, host.size() * sizeof(srsran::cf_t)));
    auto* d_p  = static_cast<float*>(c->buf(1, pil.size() * sizeof(srsran::cf_t)));
    auto* d_ce = static_cast<float*>(c->buf(2, static_cast<size_t>(nl) * nsymb * nsc * sizeof(srsran::cf_t)));
    auto* d_sc = static_cast<float*>(c->buf(3, 5 * 4 * sizeof(float) + 64));
    c->h2d(d_g, host.data(), host.size() * sizeof(srsran::cf_t));
    c->h2d(d_p, pil.data(), pil.size() * sizeof(srsran::cf_t));
    context::check(miphy_port_channel_estimate_batch(c->ctx, &j, 0, 1, d_g, d_p, d_ce, d_sc, c->stream), "port_channel_estimate");
    ce.resize(static_cast<size_t>(nl) * nsymb * nsc);
    float sc[20];
    c->d2h(ce.data(), d_ce, ce.size() * sizeof(srsran::cf_t));
    c->d2h(sc, d_sc, sizeof(float) * 5 * nl);
    c->sync();
    for (unsigned ly = 0; ly != nl; ++ly) {
      for (unsigned l = cfg.first_symbol; l != nsymb; ++l) {
        // only the PRBs of the hop the symbol belongs to carry an estimate (port_channel_estimator_average_impl.cpp:216-224)
        const srsran::bounded_bitset<srsran::MAX_RB>& m = (pt.hopping_symbol_index.has_value() && l >= pt.hopping_symbol_index.value()) ? pt.rb_mask2 : pt.rb_mask;
        srsran::span<srsran::cf_t>                    o = estimate.get_symbol_ch_estimate(l, port, ly);
        const srsran::cf_t*                           v = ce.data() + (static_cast<size_t>(ly) * nsymb + l) * nsc;
        m.for_each(0, m.size(), [&](unsigned r) { std::copy(v + r * 12, v + r * 12 + 12, o.begin() + r * 12); });
      }
      estimate.set_rsrp(sc[5 * ly + 0], port, ly);
      estimate.set_epre(sc[5 * ly + 1], port, ly);
      estimate.set_noise_variance(sc[5 * ly + 2], port, ly);
      estimate.set_snr(sc[5 * ly + 3], port, ly);
      estimate.set_time_alignment(srsran::phy_time_unit::from_seconds(sc[5 * ly + 4]), port, ly);
    }
  }

private:
  std::shared_ptr<context>  c;
  std::vector<srsran::cf_t> host, pil, ce;
};

class port_channel_estimator_factory_hip : public srsran::port_channel_estimator_factory
{
public:
  explicit port_channel_estimator_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::port_channel_estimator> create() override { return std::make_unique<port_channel_estimator_hip>(c); }

private:
  std::shared_ptr<context> c;
};
inline std::shared_ptr<srsran::port_channel_estimator_factory> create_port_channel_estimator_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<port_channel_estimator_factory_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- channel equalizer
/// srsran::channel_equalizer over miphy_channel_equalize_batch (channel_equalizer.h:93-100, channel_equalizer_zf_impl.cpp:123-162):
/// one transmit layer on up to four ports or two layers on two ports; the topologies beyond the reference (up to four layers on at least
/// as many ports, at most four) go to miphy_channel_equalize_layers_batch. Inside pusch_processor_hip the one-layer case runs fused with
/// the soft demapper; this class is the block for whoever builds a demodulator of their own around the reference interfaces.
class channel_equalizer_hip : public srsran::channel_equalizer
{
public:
  explicit channel_equalizer_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  void equalize(re_list&                 eq_symbols,
                noise_var_list&          eq_noise_vars,
                const re_list&           ch_symbols,
                const ch_est_list&       ch_estimates,
                srsran::span<const float> noise_var_estimates,
                float                    tx_scaling) override
  {
    const unsigned nre = ch_symbols.get_dimension_size(re_list::dims::re);
    const unsigned npt = ch_estimates.get_dimension_size(ch_est_list::dims::rx_port);
    const unsigned nl  = ch_estimates.get_dimension_size(ch_est_list::dims::tx_layer);
    // the checks of channel_equalizer_zf_impl.cpp:27-90
    require(ch_symbols.get_dimension_size(re_list::dims::slice) == npt, "Number of Rx ports does not match: ch_symbols vs ch_estimates.");
    require(ch_estimates.get_dimension_size(ch_est_list::dims::re) == nre, "Number of channel estimates does not match the number of Rx symbols.");
    require(eq_symbols.get_dimension_size(re_list::dims::re) == nre && eq_symbols.get_dimension_size(re_list::dims::slice) == nl,
            "Equalized symbols do not match the channel dimensions.");
    require(eq_noise_vars.get_dimension_size(re_list::dims::re) == nre && eq_noise_vars.get_dimension_size(re_list::dims::slice) == nl,
            "Post-equalization noise variances do not match the channel dimensions.");
    require(noise_var_estimates.size() == npt, "Number of noise variance estimates does not match the number of Rx ports.");
    require(tx_scaling > 0, "Tx scaling factor must be positive.");
    const bool reference_topology = (nl == 1 && npt >= 1 && npt <= 4) || (nl == 2 && npt == 2);
    require(reference_topology || (nl >= 1 && nl <= 4 && npt >= nl && npt <= 4), "Invalid channel spatial topology.");
    if (nre == 0) {
      return;
    }
    miphy_equalizer_job j = {};
    j.nof_re = nre, j.nof_rx_ports = static_cast<uint8_t>(npt), j.nof_tx_layers = static_cast<uint8_t>(nl);
    j.noise_var = noise_var_estimates[0], j.tx_scaling = tx_scaling;
    const size_t ny = static_cast<size_t>(npt) * nre, nh = ny * nl, nz = static_cast<size_t>(nl) * nre;
    auto*        d_y = static_cast<float*>(c->buf(0, ny * sizeof(srsran::cf_t)));
    auto*        d_h = static_cast<float*>(c->buf(1, nh * sizeof(srsran::cf_t)));
    auto*        d_z = static_cast<float*>(c->buf(2, nz * sizeof(srsran::cf_t)));
    auto*        d_v = static_cast<float*>(c->buf(3, nz * sizeof(float)));
    c->h2d(d_y, ch_symbols.get_view<2>({}).data(), ny * sizeof(srsran::cf_t));
    c->h2d(d_h, ch_estimates.get_view<3>({}).data(), nh * sizeof(srsran::cf_t));
    if (reference_topology) {
      context::check(miphy_channel_equalize_batch(c->ctx, &j, 0, 1, d_y, d_h, d_z, d_v, c->stream), "channel_equalize");
    } else { // beyond the reference: 2..4 layers on at least as many ports
      context::check(miphy_channel_equalize_layers_batch(c->ctx, &j, 0, 1, d_y, d_h, d_z, d_v, c->stream), "channel_equalize_layers");
    }
    c->d2h(eq_symbols.get_view<2>({}).data(), d_z, nz * sizeof(srsran::cf_t));
    c->d2h(eq_noise_vars.get_view<2>({}).data(), d_v, nz * sizeof(float));
    c->sync();
  }

private:
  std::shared_ptr<context> c;
};

class channel_equalizer_factory_hip : public srsran::channel_equalizer_factory
{
public:
  explicit channel_equalizer_factory_hip(std::shared_ptr<context> c) : c(std::move(c)) {}
  std::unique_ptr<srsran::channel_equalizer> create() override { return std::make_unique<channel_equalizer_hip>(c); }

private:
  std::shared_ptr<context> c;
};
inline std::shared_ptr<srsran::channel_equalizer_factory> create_channel_equalizer_factory_hip(std::shared_ptr<context> c)
{
  return std::make_shared<channel_equalizer_factory_hip>(std::move(c));
}

// ---------------------------------------------------------------------------------------------------------------- PDU validators
/// The validators the upper PHY asks the processor factories for (upper_phy_factories.cpp:96-99,329-334) and calls per PDU
/// (upper_phy_pdu_validators.h:71-74): the reference's own checks (its validator, built from the reference factory over the HIP
/// blocks) AND the restrictions of the device path, so that the MAC gets a clean rejection instead of an assertion.
class pusch_pdu_validator_hip : public srsran::pusch_pdu_validator
{
public:
  /// \c max_layers: 1 (the reference's limit, the default) to 4 with pusch_processor_hip's layered path behind it.
  pusch_pdu_validator_hip(std::unique_ptr<srsran::pusch_pdu_validator> ref, bool uci_supported, unsigned max_layers = 1) :
    ref(std::move(ref)), uci_supported(uci_supported), max_layers(max_layers)
  {
  }
  bool is_valid(const srsran::pusch_processor::pdu_t& pdu) const override
  {
    if (pdu.nof_tx_layers > 1) {
      // Beyond the reference, whose validator stops at one layer (pusch_processor_impl.cpp:40-42): its other rules (DM-RS type 1, two CDM groups
      // without data among them, a codeword or UCI, UCI only with a UCI decoder behind the processor, the long fields) on a copy on one layer; at
      // most max_layers layers, on at least as many ports.
      srsran::pusch_processor::pdu_t one = pdu;
      one.nof_tx_layers                  = 1;
      return pdu.nof_tx_layers <= max_layers && pdu.nof_tx_layers <= 4 && pdu.nof_tx_layers <= pdu.rx_ports.size() && is_valid(one);
    }
    // The reference's validator (pusch_processor_impl.cpp:54-58) refuses HARQ-ACK and CSI part 1 above 11 bits because its UCI decoder
    // does. With the device UCI decoder behind the processor those fields may have up to 1706 bits (polar coded): the reference's
    // remaining rules are applied to a copy of the PDU whose long fields are shortened to 11 bits, which none of them looks at
    // otherwise. CSI part 2 stays refused, as the reference refuses it (:60-63). The rate bounds of miphy_uci_polar_info (K_r + nPC < E_r,
    // E_r <= 8192) depend on the rate-matched lengths, which follow from the transport block size the validator is not given: the
    // processor checks them (miphy_pusch_uci_jobs) when the PDU arrives.
    const bool long_ack = pdu.uci.nof_harq_ack >= MIPHY_UCI_POLAR_MIN_BITS, long_csi1 = pdu.uci.nof_csi_part1 >= MIPHY_UCI_POLAR_MIN_BITS;
    if (long_ack || long_csi1) {
      if (!uci_supported || pdu.uci.nof_harq_ack > MIPHY_UCI_POLAR_MAX_BITS || pdu.uci.nof_csi_part1 > MIPHY_UCI_POLAR_MAX_BITS) {
        return false;
      }
      srsran::pusch_processor::pdu_t shortened = pdu;
      shortened.uci.nof_harq_ack               = long_ack ? 11 : pdu.uci.nof_harq_ack;
      shortened.uci.nof_csi_part1              = long_csi1 ? 11 : pdu.uci.nof_csi_part1;
      if (!ref->is_valid(shortened)) {
        return false;
      }
    } else if (!ref->is_valid(pdu)) {
      return false;
    }
    const bool has_uci = pdu.uci.nof_harq_ack != 0 || pdu.uci.nof_csi_part1 != 0 || pdu.uci.nof_csi_part2 != 0;
    // device path: multiplexed UCI only with a UCI decoder behind it, a codeword or UCI present, one layer, at most four receive
    // ports, normal cyclic prefix
    return (pdu.codeword.has_value() || has_uci) && (!has_uci || uci_supported) && pdu.nof_tx_layers == 1 && pdu.rx_ports.size() >= 1 &&
           pdu.rx_ports.size() <= 4 && pdu.cp == srsran::cyclic_prefix::NORMAL && pdu.mcs_descr.modulation != srsran::modulation_scheme::BPSK;
  }

private:
  std::unique_ptr<srsran::pusch_pdu_validator> ref;
  bool                                         uci_supported;
  unsigned                                     max_layers;
};

class pdsch_pdu_validator_hip : public srsran::pdsch_pdu_validator
{
public:
  explicit pdsch_pdu_validator_hip(std::unique_ptr<srsran::pdsch_pdu_validator> ref) : ref(std::move(ref)) {}
  bool is_valid(const srsran::pdsch_processor::pdu_t& pdu) const override
  {
    // device path: one codeword on one to four layers or two codewords on five to eight (TS 38.211 Table 7.3.1.3-1; the number of ports is
    // the number of layers) on distinct ports, DM-RS type 1, at most four reserved patterns, and an allocation that is contiguous and not
    // interleaved or whose PRB list in mapping order (rb_allocation::get_prb_indices) passes the list rule of
    // miphy_pdsch_process_mapped_batch. Two codewords on four or fewer ports (which the standard does not have) and one codeword on five or
    // more stay refused. The reference validator stops at one layer and one codeword: it judges everything else on a copy of the PDU that
    // keeps the first port and the first codeword.
    const unsigned nlayers = pdu.ports.size(), ncw = pdu.codewords.size();
    if (!((nlayers >= 1 && nlayers <= 4 && ncw == 1) || (nlayers >= 5 && nlayers <= 8 && ncw == 2))) {
      return false;
    }
    if (ncw == 2) {
      // DM-RS ports 1004 .. 1007 of type 1 exist only on a double-symbol DM-RS with two CDM groups (miphy_pdsch_process_codewords_batch):
      // every DM-RS symbol in a run of exactly two
      if (pdu.nof_cdm_groups_without_data != 2) {
        return false;
      }
      for (unsigned l = 0, run = 0; l <= pdu.dmrs_symbol_mask.size(); ++l) {
        if (l != pdu.dmrs_symbol_mask.size() && pdu.dmrs_symbol_mask.test(l)) {
          ++run;
        } else if (run != 0 && run != 2) {
          return false;
        } else {
          run = 0;
        }
      }
    }
    for (unsigned a = 0; a != nlayers; ++a) {
      for (unsigned b = 0; b != a; ++b) {
        if (pdu.ports[a] == pdu.ports[b]) {
          return false;
        }
      }
    }
    srsran::pdsch_processor::pdu_t one = pdu;
    one.ports.resize(1);
    one.codewords.resize(1);
    if (!pdu.freq_alloc.is_contiguous()) {
      // The reference validator refuses these outright: the allocation is judged here (its own BWP check, then the list rule) and the
      // rest of the PDU on a copy with one PRB in its place.
      if (!pdu.freq_alloc.is_bwp_valid(pdu.bwp_start_rb, pdu.bwp_size_rb) ||
          !prb_list_obeys_list_rule(pdu.freq_alloc.get_prb_indices(pdu.bwp_start_rb, pdu.bwp_size_rb),
                                    pdu.freq_alloc.get_prb_mask(pdu.bwp_start_rb, pdu.bwp_size_rb))) {
        return false;
      }
      one.freq_alloc = srsran::rb_allocation::make_type1(0, 1);
    }
    if (!ref->is_valid(one)) {
      return false;
    }
    return pdu.dmrs == srsran::dmrs_type::TYPE1 && pdu.cp == srsran::cyclic_prefix::NORMAL && pdu.reserved.get_nof_entries() <= 4;
  }

private:
  std::unique_ptr<srsran::pdsch_pdu_validator> ref;
};

inline std::unique_ptr<srsran::pusch_pdu_validator> pusch_processor_factory_hip::create_validator()
{
  srsran::uci_decoder_factory_sw_configuration uc;
  uc.decoder_factory = srsran::create_short_block_detector_factory_sw();
  srsran::pusch_processor_factory_sw_configuration pc;
  pc.estimator_factory                    = std::make_shared<dmrs_pusch_estimator_factory_hip>(c);
  pc.demodulator_factory                  = std::make_shared<pusch_demodulator_factory_hip>(c);
  pc.demux_factory                        = srsran::create_ulsch_demultiplex_factory_sw();
  pc.decoder_factory                      = std::make_shared<pusch_decoder_factory_hip>(c);
  pc.uci_dec_factory                      = srsran::create_uci_decoder_factory_sw(uc);
  pc.ch_estimate_dimensions.nof_prb       = srsran::MAX_RB;
  pc.ch_estimate_dimensions.nof_symbols   = srsran::MAX_NSYMB_PER_SLOT;
  pc.ch_estimate_dimensions.nof_rx_ports  = 4;
  pc.ch_estimate_dimensions.nof_tx_layers = 1;
  pc.dec_nof_iterations                   = nof_iterations;
  pc.dec_enable_early_stop                = early_stop;
  return std::make_unique<pusch_pdu_validator_hip>(srsran::create_pusch_processor_factory_sw(pc)->create_validator(), uci_dec_factory != nullptr, max_layers);
}

inline std::unique_ptr<srsran::pdsch_pdu_validator> pdsch_processor_factory_hip::create_validator()
{
  auto ref = srsran::create_pdsch_processor_factory_sw(std::make_shared<pdsch_encoder_factory_hip>(c), std::make_shared<pdsch_modulator_factory_hip>(c),
                                                       std::make_shared<dmrs_pdsch_processor_factory_hip>(c));
  return std::make_unique<pdsch_pdu_validator_hip>(ref->create_validator());
}

// The PDCCH / SSB / CSI-RS device paths take everything the reference processors take: the reference's validators apply unchanged.
inline std::unique_ptr<srsran::pdcch_pdu_validator> pdcch_processor_factory_hip::create_validator()
{
  auto prg = srsran::create_pseudo_random_generator_sw_factory();
  auto ref = srsran::create_pdcch_processor_factory_sw(std::make_shared<pdcch_encoder_factory_hip>(c),
                                                       srsran::create_pdcch_modulator_factory_sw(srsran::create_channel_modulation_sw_factory(), prg),
                                                       srsran::create_dmrs_pdcch_processor_factory_sw(prg));
  return ref->create_validator();
}

inline std::unique_ptr<srsran::ssb_pdu_validator> ssb_processor_factory_hip::create_validator()
{
  auto                                       prg = srsran::create_pseudo_random_generator_sw_factory();
  srsran::ssb_processor_factory_sw_configuration sc;
  sc.encoder_factory   = srsran::create_pbch_encoder_factory_sw(srsran::create_crc_calculator_factory_sw("auto"), prg, srsran::create_polar_factory_sw());
  sc.modulator_factory = srsran::create_pbch_modulator_factory_sw(srsran::create_channel_modulation_sw_factory(), prg);
  sc.dmrs_factory      = srsran::create_dmrs_pbch_processor_factory_sw(prg);
  sc.pss_factory       = srsran::create_pss_processor_factory_sw();
  sc.sss_factory       = srsran::create_sss_processor_factory_sw();
  return srsran::create_ssb_processor_factory_sw(sc)->create_validator();
}

inline std::unique_ptr<srsran::nzp_csi_rs_configuration_validator> nzp_csi_rs_generator_factory_hip::create_validator()
{
  return srsran::create_nzp_csi_rs_generator_factory_sw(srsran::create_pseudo_random_generator_sw_factory())->create_validator();
}

// --------------------------------------------------------------------------------------------------- multi-GPU placement
/// Device placement of a node with several GPUs: the path shards by cell / transport block with no cross-unit
/// dependency, exactly like the reference runs one processor instance per worker (lib/phy/upper/uplink_processor_concurrent.h:41-54).
/// One context per device; a CELL is pinned to one device -- `cell % devices` -- so that everything stateful of its UEs (the HARQ
/// soft buffers of rx_softbuffer_pool_hip, which a retransmission must find where the first transmission left them) lives on
/// that device and no PHY data ever crosses xGMI. One HARQ pool per device, created on first use with the configuration given here.
/// A thread that drives a cell calls bind_thread(cell) once (a new thread starts on device 0).
class device_placement
{
public:
  /// \param nof_devices Devices to use, -1 = all visible ones.
  explicit device_placement(const srsran::rx_softbuffer_pool_config& pool_config_, int nof_devices = -1) : pool_config(pool_config_)
  {
    int n = 0;
    context::hip(hipGetDeviceCount(&n), "hipGetDeviceCount");
    if (nof_devices > 0 && nof_devices < n) {
      n = nof_devices;
    }
    require(n > 0, "No GPU visible.");
    for (int d = 0; d != n; ++d) {
      contexts.emplace_back(std::make_shared<context>(d));
    }
    pools.resize(contexts.size());
  }
  unsigned nof_devices() const { return contexts.size(); }
  /// Device index a cell is pinned to.
  unsigned device_of_cell(unsigned cell_index) const { return cell_index % contexts.size(); }
  /// The context every block of that cell is created with (create_*_factory_hip(placement.context_of_cell(cell))).
  std::shared_ptr<context> context_of_cell(unsigned cell_index) const { return contexts[device_of_cell(cell_index)]; }
  /// The HARQ pool of the cell's device (shared by the cells pinned to it).
  srsran::rx_softbuffer_pool& softbuffer_pool_of_cell(unsigned cell_index)
  {
    const unsigned              d = device_of_cell(cell_index);
    std::lock_guard<std::mutex> lk(mutex);
    if (!pools[d]) {
      contexts[d]->bind_thread();
      pools[d] = create_rx_softbuffer_pool_hip(contexts[d], pool_config);
    }
    return *pools[d];
  }
  /// Makes the cell's device the current one of the calling thread.
  void bind_thread(unsigned cell_index) const { contexts[device_of_cell(cell_index)]->bind_thread(); }

private:
  srsran::rx_softbuffer_pool_config                         pool_config;
  std::vector<std::shared_ptr<context>>                     contexts;
  std::vector<std::unique_ptr<srsran::rx_softbuffer_pool>>  pools;
  std::mutex                                                mutex;
};

} // namespace miphy
