"""CPU: the srsRAN adapter header compiles with the route to miphy_pusch_process_layers_batch_ex -- pusch_processor_hip with a UCI decoder and the
EVM on four layers -- and the layered validator, with a UCI decoder factory behind it, accepts UCI above one layer (short and polar-coded HARQ-ACK,
UCI only), keeps the limits of one layer (1706 bits, a codeword or UCI) and, without a UCI decoder, keeps refusing UCI. A small program is
compiled against the reference's headers, linked with the reference archive of oracle/_ref and the library, and run here; the device path is only
compiled, its behaviour on the GPU is covered through the C ABI it calls (tests/test_pusch_process_layers_uci_gpu.py). Skipped where the reference
tree or its build is absent."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libsrsran_ref.a")
PKG = os.path.join(ROOT, "srsran_project_23.5_amd")

TU = r"""
#include "miphy_srsran_adapters.h"
#include <cstdio>

using namespace srsran;

// Compiled, never called: UCI and EVM on four layers through the processor.
void instantiate(std::shared_ptr<miphy::context> c, const resource_grid_reader& grid, rx_softbuffer& softbuffer, pusch_processor_result_notifier& notifier,
                 pusch_processor::pdu_t pdu)
{
  pdu.nof_tx_layers    = 4;
  pdu.uci.nof_harq_ack = 20, pdu.uci.nof_csi_part1 = 4;
  miphy::pusch_processor_hip p(c, 6, true, std::make_unique<miphy::uci_decoder_hip>(c), true, 4);
  std::vector<uint8_t>       data(100);
  p.process(data, softbuffer, notifier, grid, pdu);
  auto q = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true, miphy::create_uci_decoder_factory_hip(c), true, 4)->create();
  q->process(data, softbuffer, notifier, grid, pdu);
  int (*ex)(miphy_ctx*, const miphy_pusch_layers_pdu*, const miphy_pusch_uci*, uint32_t, const float*, int8_t*, uint8_t*, uint8_t*, uint8_t*,
            miphy_pusch_result*, float*, int8_t*, float*, void*) = &miphy_pusch_process_layers_batch_ex;
  int (*demod)(miphy_ctx*, const miphy_pusch_demod_layers_job*, int, uint32_t, const float*, const float*, const float*, int8_t*, const uint16_t*, float*,
               void*) = &miphy_pusch_demodulate_layers_batch_ex;
  (void)ex, (void)demod;
}

int main()
{
  int failed = 0;
  std::shared_ptr<miphy::context> c; // the validators never touch the device
  auto with_uci = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true, miphy::create_uci_decoder_factory_hip(c), false, 4)->create_validator();
  auto without  = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true, nullptr, false, 4)->create_validator();
  symbol_slot_mask dm(14);
  dm.set(2);
  pusch_processor::pdu_t pdu;
  pdu.slot = slot_point(1, 7), pdu.rnti = 0x4601, pdu.bwp_size_rb = 273, pdu.bwp_start_rb = 0, pdu.cp = cyclic_prefix::NORMAL;
  pdu.mcs_descr.modulation = modulation_scheme::QAM256, pdu.mcs_descr.target_code_rate = 0.9F;
  pdu.codeword.emplace();
  pdu.codeword.value().rv = 0, pdu.codeword.value().ldpc_base_graph = ldpc_base_graph_type::BG1, pdu.codeword.value().new_data = true;
  pdu.uci = {};
  pdu.n_id = 935, pdu.nof_tx_layers = 4;
  for (unsigned p = 0; p != 4; ++p)
    pdu.rx_ports.push_back(p);
  pdu.dmrs_symbol_mask = dm, pdu.dmrs = dmrs_type::TYPE1, pdu.scrambling_id = 42, pdu.n_scid = false, pdu.nof_cdm_groups_without_data = 2;
  pdu.freq_alloc         = rb_allocation::make_type1(0, 273);
  pdu.start_symbol_index = 0, pdu.nof_symbols = 14, pdu.tbs_lbrm_bytes = ldpc::MAX_CODEBLOCK_SIZE / 8;
  failed += !with_uci->is_valid(pdu) || !without->is_valid(pdu); // four layers, no UCI
  auto q = pdu;
  q.uci.nof_harq_ack = 2;
  failed += 2 * (!with_uci->is_valid(q) || without->is_valid(q)); // a two-bit HARQ-ACK: only with a UCI decoder
  q = pdu, q.uci.nof_harq_ack = 20;
  failed += 4 * (!with_uci->is_valid(q) || without->is_valid(q)); // polar coded
  q = pdu, q.uci.nof_harq_ack = 2, q.codeword.reset();
  failed += 8 * (!with_uci->is_valid(q) || without->is_valid(q)); // UCI only
  q = pdu, q.uci.nof_harq_ack = 1707;
  failed += 16 * with_uci->is_valid(q); // above the polar decoder's limit
  q = pdu, q.codeword.reset();
  failed += 32 * (with_uci->is_valid(q) || without->is_valid(q)); // neither codeword nor UCI
  q = pdu, q.uci.nof_harq_ack = 2, q.rx_ports.pop_back();
  failed += 64 * with_uci->is_valid(q); // more layers than ports
  std::printf(failed ? "FAILED %d\n" : "OK\n", failed);
  return failed != 0;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_uci_and_evm_above_one_layer():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pusch_process_layers_uci.cpp"), os.path.join(tmp, "pusch_process_layers_uci")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
