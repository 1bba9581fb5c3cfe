"""CPU: the srsRAN adapter header compiles with the PUCCH format 3 / 4 additions (pucch_f34_configuration and
pucch_processor_hip::process_f34_batch next to the unchanged process() overrides of formats 3 and 4), and the host part of the new C ABI
is run from C++: a small program is compiled against the reference's headers, linked with the reference archive of oracle/_ref and the
library, and asks miphy_pucch_f34_info for the layouts and the refusals a scheduler would meet. The processor is only compiled; its
behaviour on the GPU is covered through the C ABI it calls (tests/test_pucch_f34_gpu.py). Skipped where the reference tree or its build is
absent."""
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
#include <cstring>

// Compiled, never called: a slot's format 3 and 4 PDUs through the device processor.
void instantiate(std::shared_ptr<miphy::context> c, const srsran::resource_grid_reader& grid)
{
  miphy::pucch_processor_hip                  gpu(c, nullptr, 8);
  std::vector<miphy::pucch_f34_configuration> cfgs(2);
  cfgs[0].slot = srsran::slot_point(1, 3), cfgs[0].ports.push_back(0), cfgs[0].bwp_size_rb = 52, cfgs[0].starting_prb = 4, cfgs[0].nof_prb = 4;
  cfgs[0].nof_symbols = 14, cfgs[0].rnti = 0x4601, cfgs[0].n_id = 5, cfgs[0].n_id_hopping = 7, cfgs[0].nof_harq_ack = 8, cfgs[0].nof_csi_part1 = 40;
  cfgs[1] = cfgs[0];
  cfgs[1].format = 4, cfgs[1].nof_prb = 1, cfgs[1].occ_length = 4, cfgs[1].occ_index = 3, cfgs[1].pi2_bpsk = true, cfgs[1].second_hop_prb = 40;
  std::vector<srsran::pucch_processor_result> out(2);
  gpu.process_f34_batch(grid, cfgs, out);
  srsran::pucch_processor::format3_configuration c3;
  srsran::pucch_processor::format4_configuration c4;
  srsran::pucch_processor_result r3 = gpu.process(grid, c3), r4 = gpu.process(grid, c4); // as before: the CPU processor, or an empty result
  (void)r3, (void)r4;
}

int main()
{
  int  failed = 0;
  auto job    = [](unsigned format, unsigned nof_prb, unsigned nsym, bool hop, bool add, bool pi2, unsigned occ_length, unsigned occ_index, unsigned K) {
    miphy_pucch_f34_job j = {};
    j.format = format, j.numerology = 1, j.slot = 3, j.nof_ports = 2, j.start_symbol = 14 - nsym, j.nof_symbols = nsym, j.intra_slot_hopping = hop;
    j.bwp_size_rb = 52, j.starting_prb = 4, j.second_hop_prb = 30, j.nof_prb = nof_prb, j.pi2_bpsk = pi2, j.additional_dmrs = add;
    j.occ_length = occ_length, j.occ_index = occ_index, j.nof_harq_ack = K > 8 ? 8 : K, j.nof_csi_part1 = K > 8 ? K - 8 : 0, j.grid_nprb = 52;
    return j;
  };
  auto expect = [&](const miphy_pucch_f34_job& j, int rc, unsigned E, unsigned polar, const char* text) {
    miphy_pucch_f34_info_t info = {};
    const int              got  = miphy_pucch_f34_info(&j, &info);
    if (got != rc || (rc == MIPHY_OK && (info.E != E || info.polar != polar || info.M != 12u * j.nof_prb)) ||
        (rc != MIPHY_OK && !std::strstr(miphy_last_error(), text))) {
      std::printf("FAIL format %u, %u PRB: rc %d (want %d), E %u (want %u), polar %u, '%s'\n", j.format, j.nof_prb, got, rc, info.E, E, info.polar,
                  rc ? miphy_last_error() : "");
      ++failed;
    }
  };
  expect(job(3, 4, 14, false, false, false, 0, 0, 48), MIPHY_OK, 2 * 48 * 12, 1, "");
  expect(job(3, 16, 14, true, true, true, 0, 0, 11), MIPHY_OK, 192 * 10, 0, "");
  expect(job(4, 1, 4, true, false, true, 4, 3, 3), MIPHY_OK, 6, 0, "");
  expect(job(4, 1, 14, false, true, false, 2, 1, 20), MIPHY_OK, 2 * 6 * 10, 1, "");
  expect(job(3, 2, 14, false, false, false, 0, 0, 20), MIPHY_EUNSUPP, 0, 0, "length-24");
  expect(job(3, 7, 14, false, false, false, 0, 0, 20), MIPHY_EINVAL, 0, 0, "format 3 on 7 PRBs");
  expect(job(4, 1, 14, false, false, false, 4, 4, 20), MIPHY_EINVAL, 0, 0, "occ_index 4");
  expect(job(3, 1, 4, true, false, true, 0, 0, 19), MIPHY_EINVAL, 0, 0, "K_r + nPC < E_r");
  static_assert(sizeof(miphy_pucch_f34_job) == 80 && sizeof(miphy_pucch_f34_info_t) == 32, "record sizes");
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_format_3_and_4_batch_and_the_info_call_answers_from_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pucch_f34.cpp"), os.path.join(tmp, "pucch_f34")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
