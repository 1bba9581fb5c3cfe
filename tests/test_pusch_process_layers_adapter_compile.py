"""CPU: the srsRAN adapter header compiles with the routes to miphy_dmrs_pusch_estimate_layers_batch and miphy_pusch_process_layers_batch --
dmrs_pusch_estimator_hip(separate_layers), pusch_processor_hip / pusch_processor_factory_hip(max_layers) and the validator behind them -- the
record the processor fills has the layout the library expects, the layered validator accepts four layers on four ports and a default one still
refuses two. A small program is compiled against the reference's headers, linked with the reference archive of oracle/_ref and the library, and
run here; the device paths are only compiled, their behaviour on the GPU is covered through the C ABI they call
(tests/test_chest_layers_gpu.py, tests/test_pusch_process_layers_gpu.py). Skipped where the reference tree or its build is absent."""
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
#include <cstddef>
#include <cstdio>

using namespace srsran;

// Compiled, never called: the layered estimator and processor routes.
void instantiate(std::shared_ptr<miphy::context> c, const resource_grid_reader& grid, rx_softbuffer& softbuffer, pusch_processor_result_notifier& notifier,
                 const pusch_processor::pdu_t& pdu)
{
  miphy::dmrs_pusch_estimator_hip     e(c, true);
  dmrs_pusch_estimator::configuration ecfg = {};
  ecfg.nof_tx_layers                       = 4;
  channel_estimate ce;
  e.estimate(ce, grid, ecfg);
  auto est = miphy::create_dmrs_pusch_estimator_factory_hip(c, true)->create();
  est->estimate(ce, grid, ecfg);
  miphy::pusch_processor_hip p(c, 6, true, nullptr, false, 4);
  std::vector<uint8_t>       data(100);
  p.process(data, softbuffer, notifier, grid, pdu);
  auto q = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true, nullptr, false, 4)->create();
  q->process(data, softbuffer, notifier, grid, pdu);
}

int main()
{
  int failed = 0;
  failed += sizeof(miphy_pusch_layers_pdu) != sizeof(miphy_pusch_pdu) + 8 || offsetof(miphy_pusch_layers_pdu, nof_tx_layers) != sizeof(miphy_pusch_pdu);
  failed += sizeof(miphy_pusch_pdu) != 112 || offsetof(miphy_pusch_layers_pdu, base) != 0;
  std::shared_ptr<miphy::context> c; // the validators never touch the device
  auto layered = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true, nullptr, false, 4)->create_validator();
  auto plain   = std::make_shared<miphy::pusch_processor_factory_hip>(c, 6, true)->create_validator();
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
  failed += !layered->is_valid(pdu); // four layers on four ports
  auto q          = pdu;
  q.nof_tx_layers = 1;
  failed += !layered->is_valid(q) || !plain->is_valid(q);
  q.nof_tx_layers = 2;
  failed += !layered->is_valid(q) || plain->is_valid(q); // a default validator still refuses two layers
  q = pdu, q.rx_ports.pop_back();
  failed += layered->is_valid(q); // more layers than ports
  q = pdu, q.dmrs = dmrs_type::TYPE2;
  failed += layered->is_valid(q);
  q = pdu, q.nof_cdm_groups_without_data = 1;
  failed += layered->is_valid(q);
  q = pdu, q.uci.nof_harq_ack = 2;
  failed += layered->is_valid(q); // no UCI above one layer
  q = pdu, q.codeword.reset();
  failed += layered->is_valid(q);
  std::printf(failed ? "FAILED %d\n" : "OK\n", failed);
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_layered_estimator_and_processor():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pusch_process_layers.cpp"), os.path.join(tmp, "pusch_process_layers")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
