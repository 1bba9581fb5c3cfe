"""CPU: the srsRAN adapter header compiles with the PUCCH format 0 additions (pucch_f0_configuration and pucch_processor_hip::process_f0_batch
next to the unchanged process() overrides), and the host part of the new C ABI is run from C++: a small program is compiled against the
reference's headers, linked with the reference archive of oracle/_ref and the library, and asks miphy_pucch_f0_info for the hypotheses, the free
shifts and the refusals a scheduler would meet. The processor is only compiled; its behaviour on the GPU is covered through the C ABI it calls
(tests/test_pucch_f0_gpu.py). Skipped where the reference tree or its build is absent."""
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
#include <cmath>
#include <cstdio>
#include <cstring>

// Compiled, never called: a slot's format 0 PDUs through the device processor.
void instantiate(std::shared_ptr<miphy::context> c, const srsran::resource_grid_reader& grid)
{
  miphy::pucch_processor_hip                 gpu(c, nullptr, 1);
  std::vector<miphy::pucch_f0_configuration> cfgs(2);
  cfgs[0].slot = srsran::slot_point(1, 3), cfgs[0].ports.push_back(0), cfgs[0].bwp_size_rb = 52, cfgs[0].starting_prb = 4, cfgs[0].start_symbol_index = 13;
  cfgs[0].initial_cyclic_shift = 2, cfgs[0].n_id = 7, cfgs[0].nof_harq_ack = 1, cfgs[0].used_shifts_mask = 0x104;
  cfgs[1] = cfgs[0];
  cfgs[1].start_symbol_index = 12, cfgs[1].nof_symbols = 2, cfgs[1].second_hop_prb = 40, cfgs[1].nof_harq_ack = 2, cfgs[1].sr_opportunity = true;
  cfgs[1].threshold = 6.0f, cfgs[1].noise_variance = 0.01f;
  std::vector<srsran::pucch_processor_result> out(2);
  gpu.process_f0_batch(grid, cfgs, out);
  srsran::pucch_processor::format0_configuration c0;
  srsran::pucch_processor::format1_configuration c1;
  srsran::pucch_processor_result r0 = gpu.process(grid, c0), r1 = gpu.process(grid, c1); // as before
  (void)r0, (void)r1;
}

int main()
{
  int  failed = 0;
  auto job    = [](unsigned nports, unsigned nsym, unsigned ics, unsigned nharq, unsigned nsr, unsigned mask, float noise_var) {
    miphy_pucch_f0_job j = {};
    j.numerology = 1, j.slot = 3, j.nof_ports = nports, j.start_symbol = 14 - nsym, j.nof_symbols = nsym, j.bwp_size_rb = 52, j.starting_prb = 4;
    j.initial_cyclic_shift = ics, j.nof_harq_ack = nharq, j.nof_sr = nsr, j.used_shifts_mask = mask, j.n_id = 5, j.noise_var = noise_var, j.grid_nprb = 52;
    return j;
  };
  auto expect = [&](const miphy_pucch_f0_job& j, int rc, unsigned H, unsigned last_shift, unsigned F, double threshold, const char* text) {
    miphy_pucch_f0_info_t info = {};
    const int             got  = miphy_pucch_f0_info(&j, &info);
    const bool            ok   = got == rc && (rc != MIPHY_OK ? std::strstr(miphy_last_error(), text) != nullptr
                                                             : info.nof_hypotheses == H && info.shifts[H - 1] == last_shift && info.F == F &&
                                                      info.D == unsigned(j.nof_ports) * j.nof_symbols && (threshold == 0 || std::fabs(info.threshold - threshold) <= 5e-3 * threshold));
    if (!ok) {
      std::printf("FAIL: rc %d (want %d), H %u, F %u, threshold %g (want %g), '%s'\n", got, rc, info.nof_hypotheses, info.F, info.threshold, threshold,
                  rc ? miphy_last_error() : "");
      ++failed;
    }
  };
  // the thresholds are the closed forms at (D, F, H): (1, 11, 1) and (2, 8, 4) with estimated noise; e^-t = 0.01 with known noise
  expect(job(1, 1, 0, 0, 1, 0, 0.f), MIPHY_OK, 1, 0, 11, 5.72, "");
  expect(job(1, 2, 11, 2, 0, 0, 0.f), MIPHY_OK, 4, 8, 8, 5.17, "");
  expect(job(2, 2, 3, 2, 1, 0x005, 0.f), MIPHY_OK, 8, 1, 3, 0, ""); // shifts 5, 8 and 11 stay free
  expect(job(1, 1, 0, 0, 1, 0xfff, 0.5f), MIPHY_OK, 1, 0, 0, 4.605, "");
  expect(job(1, 1, 0, 1, 0, 0xfff, 0.f), MIPHY_EINVAL, 0, 0, 0, 0, "no free cyclic shift to estimate the noise from");
  expect(job(1, 3, 0, 1, 0, 0, 0.f), MIPHY_EINVAL, 0, 0, 0, 0, "invalid symbol range");
  expect(job(5, 1, 0, 1, 0, 0, 0.f), MIPHY_EINVAL, 0, 0, 0, 0, "invalid number of receive ports");
  expect(job(1, 1, 12, 1, 0, 0, 0.f), MIPHY_EINVAL, 0, 0, 0, 0, "initial_cyclic_shift");
  expect(job(1, 1, 0, 0, 0, 0, 0.f), MIPHY_EINVAL, 0, 0, 0, 0, "no UCI bits");
  expect(job(1, 1, 0, 1, 0, 0, -1.f), MIPHY_EINVAL, 0, 0, 0, 0, "finite and not negative");
  static_assert(sizeof(miphy_pucch_f0_job) == 64 && sizeof(miphy_pucch_f0_info_t) == 28 && sizeof(miphy_pucch_result) == 24, "record sizes");
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_format_0_batch_and_the_info_call_answers_from_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pucch_f0.cpp"), os.path.join(tmp, "pucch_f0")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
