"""CPU: the srsRAN adapter header compiles with the list size and the long-payload flag of the device PUCCH processor
(pucch_processor_hip, pucch_pdu_validator_hip, the factory and create_pucch_processor_factory_hip), and the validator's host logic for
format 2 above 11 bits is run: a small program is compiled against the reference's headers, linked with the reference archive of
oracle/_ref and the library, and run here. The cases follow the reference's pucch_format2_code_rate (payload bits over 16 nof_prb
nof_symbols channel bits, at most 0.8) and miphy_uci_polar_info. The processor is only compiled; its behaviour on the GPU is covered
through the C ABI it calls (tests/test_pucch_long_gpu.py). Skipped where the reference tree or its build is absent."""
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

// Compiled, never called: the new constructor arguments.
void instantiate(std::shared_ptr<miphy::context> c, std::shared_ptr<srsran::pucch_processor_factory> cpu_factory,
                 const srsran::resource_grid_reader& grid)
{
  srsran::channel_estimate::channel_estimate_dimensions dims;
  dims.nof_prb = 273, dims.nof_symbols = 14, dims.nof_rx_ports = 4, dims.nof_tx_layers = 1;
  std::shared_ptr<srsran::pucch_processor_factory> f  = miphy::create_pucch_processor_factory_hip(c, dims, cpu_factory, 8, true);
  std::shared_ptr<srsran::pucch_processor_factory> f0 = miphy::create_pucch_processor_factory_hip(c, dims);
  miphy::pucch_processor_factory_hip               f1(c, dims, nullptr, 4, true);
  std::unique_ptr<srsran::pucch_processor>         p  = f->create();
  std::unique_ptr<srsran::pucch_pdu_validator>     v  = f->create_validator();
  miphy::pucch_processor_hip                       gpu_only(c, nullptr, 2);
  srsran::pucch_processor::format1_configuration   c1;
  srsran::pucch_processor::format2_configuration   c2;
  c2.nof_csi_part1 = 40, c2.nof_prb = 9, c2.nof_symbols = 1;
  srsran::pucch_processor_result r1 = p->process(grid, c1), r2 = gpu_only.process(grid, c2);
  std::vector<srsran::pucch_processor::format1_configuration> b1(3);
  std::vector<srsran::pucch_processor::format2_configuration> b2(2);
  std::vector<srsran::pucch_processor_result>                 o1(3), o2(2);
  gpu_only.process_batch(grid, b1, b2, o1, o2);
  bool ok = v->is_valid(c1) && v->is_valid(c2) && gpu_only.get_list_size() == 2;
  (void)r1, (void)r2, (void)ok, (void)f0;
}

int main()
{
  srsran::channel_estimate::channel_estimate_dimensions dims;
  dims.nof_prb = 273, dims.nof_symbols = 14, dims.nof_rx_ports = 4, dims.nof_tx_layers = 1;
  int  failed = 0;
  auto check  = [&](bool flag, unsigned ack, unsigned sr, unsigned csi1, unsigned csi2, unsigned nof_prb, unsigned nof_symbols, bool want) {
    miphy::pucch_pdu_validator_hip                 v(dims, flag);
    srsran::pucch_processor::format2_configuration cfg = {};
    cfg.cp = srsran::cyclic_prefix::NORMAL, cfg.bwp_size_rb = 52, cfg.bwp_start_rb = 0, cfg.starting_prb = 3, cfg.nof_prb = nof_prb;
    cfg.start_symbol_index = 5, cfg.nof_symbols = nof_symbols, cfg.ports.push_back(0);
    cfg.nof_harq_ack = ack, cfg.nof_sr = sr, cfg.nof_csi_part1 = csi1, cfg.nof_csi_part2 = csi2;
    const bool got = v.is_valid(cfg);
    if (got != want) {
      std::printf("FAIL flag=%d bits=%u+%u+%u+%u on %u PRB x %u: got %d want %d\n", flag, ack, sr, csi1, csi2, nof_prb, nof_symbols, got, want);
      ++failed;
    }
  };
  for (int flag = 0; flag != 2; ++flag) {
    const bool on = flag != 0;
    check(on, 2, 1, 4, 0, 1, 1, true);       // 7 bits: as before, whatever the flag
    check(on, 2, 0, 0, 0, 1, 1, false);      // 2 bits
    check(on, 5, 1, 6, 0, 1, 1, false);      // 12 bits on 16: rate 0.75 passes, the polar framing needs K_r + nPC = 21 < 16
    check(on, 5, 1, 6, 0, 2, 1, on);         // 12 bits on 32: rate 0.375, framing 21 < 32
    check(on, 0, 0, 12, 0, 2, 1, on);
    check(on, 5, 1, 34, 0, 9, 1, on);        // 40 bits on 144
    check(on, 5, 1, 94, 0, 8, 1, on);        // 100 bits on 128: rate 0.78
    check(on, 5, 1, 98, 0, 8, 1, false);     // 104 bits on 128: rate 0.8125 > 0.8 although the framing (115 < 128) would take it
    check(on, 5, 1, 34, 1, 9, 1, false);     // CSI part 2
    check(on, 5, 1, 15, 0, 2, 1, false);     // 21 bits on 32: rate 0.66 passes, framing 32 < 32 does not
    check(on, 100, 100, 209, 0, 16, 2, on);  // 409 bits on 512: rate 0.799
    check(on, 100, 100, 210, 0, 16, 2, false);
  }
  {
    miphy::pucch_pdu_validator_hip                 v(dims); // the default is the flag off
    srsran::pucch_processor::format2_configuration cfg = {};
    cfg.cp = srsran::cyclic_prefix::NORMAL, cfg.bwp_size_rb = 52, cfg.nof_prb = 9, cfg.nof_symbols = 1, cfg.ports.push_back(0), cfg.nof_csi_part1 = 40;
    if (v.is_valid(cfg)) {
      std::printf("FAIL default validator accepts 40 bits\n");
      ++failed;
    }
  }
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_and_the_validator_takes_long_format2_payloads_behind_its_flag():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pucch_long.cpp"), os.path.join(tmp, "pucch_long")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
