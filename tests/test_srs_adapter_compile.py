"""CPU: the srsRAN adapter header compiles with the SRS additions (srs_estimator_configuration, srs_estimator_result and
srs_estimator_hip::estimate_batch), and the host part of the new C ABI is run from C++: a small program is compiled against the reference's headers,
linked with the reference archive of oracle/_ref and the library, and asks miphy_srs_info for what a scheduler would need and for the refusals it would
meet. The estimator is only compiled; its behaviour on the GPU is covered through the C ABI it calls (tests/test_srs_gpu.py). Skipped where the
reference tree or its build is absent."""
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

// Compiled, never called: a slot's SRS through the device estimator.
void instantiate(std::shared_ptr<miphy::context> c, const srsran::resource_grid_reader& grid)
{
  miphy::srs_estimator_hip                        gpu(c);
  std::vector<miphy::srs_estimator_configuration> cfgs(2);
  cfgs[0].slot = srsran::slot_point(1, 3), cfgs[0].ports.push_back(0), cfgs[0].ports.push_back(1), cfgs[0].nof_tx_ports = 2, cfgs[0].nof_prb = 48;
  cfgs[0].start_symbol_index = 12, cfgs[0].nof_symbols = 2, cfgs[0].cyclic_shift = 3, cfgs[0].n_id = 7, cfgs[0].prg_size = 2;
  cfgs[1] = cfgs[0];
  cfgs[1].comb_size = 4, cfgs[1].comb_offset = 3, cfgs[1].nof_tx_ports = 4, cfgs[1].cyclic_shift = 9, cfgs[1].group_hopping = true, cfgs[1].start_prb = 48;
  std::vector<miphy::srs_estimator_result> out(2);
  gpu.estimate_batch(grid, cfgs, out);
  const srsran::cf_t h = out[0].channel[(0 * out[0].nof_rx_ports + 1) * out[0].nof_tx_ports + 0] + out[1].wideband[0][3];
  (void)h, (void)out[0].time_alignment.to_seconds();
}

int main()
{
  int  failed = 0;
  auto job    = [](unsigned nprb, unsigned K, unsigned nap, unsigned ncs, unsigned prg, unsigned nsym) {
    miphy_srs_job j = {};
    j.numerology = 1, j.slot = 3, j.nof_rx_ports = 2, j.nof_tx_ports = nap, j.start_symbol = 14 - nsym, j.nof_symbols = nsym, j.comb_size = K, j.cyclic_shift = ncs;
    j.prg_size = prg, j.start_prb = 1, j.nof_prb = nprb, j.n_id = 5, j.grid_nprb = 275;
    return j;
  };
  auto expect = [&](const miphy_srs_job& j, int rc, unsigned M, unsigned Q, unsigned P, unsigned G, unsigned combs, double range, const char* text) {
    miphy_srs_info_t info = {};
    const int        got  = miphy_srs_info(&j, &info);
    const bool       ok   = got == rc && (rc != MIPHY_OK ? std::strstr(miphy_last_error(), text) != nullptr
                                                          : info.M == M && info.Q == Q && info.P == P && info.G == G && info.nof_combs == combs &&
                                                         info.nof_h == G * 2 * j.nof_tx_ports && std::fabs(info.max_delay_s - range) <= 1e-6 * range);
    if (!ok) {
      std::printf("FAIL: rc %d (want %d), M %u Q %u P %u G %u combs %u range %g, '%s'\n", got, rc, info.M, info.Q, info.P, info.G, info.nof_combs,
                  info.max_delay_s, rc ? miphy_last_error() : "");
      ++failed;
    }
  };
  expect(job(48, 2, 2, 3, 2, 2), MIPHY_OK, 288, 12, 2, 24, 1, 1.0 / (2 * 30e3 * 2 * 2), "");
  expect(job(272, 2, 1, 0, 1, 1), MIPHY_OK, 1632, 6, 1, 272, 1, 1.0 / (2 * 30e3 * 2), "");
  expect(job(48, 4, 4, 9, 2, 4), MIPHY_OK, 144, 6, 2, 24, 2, 1.0 / (2 * 30e3 * 4 * 2), "");
  expect(job(48, 4, 4, 2, 4, 4), MIPHY_OK, 144, 12, 4, 12, 1, 1.0 / (2 * 30e3 * 4 * 4), "");
  expect(job(4, 2, 1, 0, 1, 1), MIPHY_EUNSUPP, 0, 0, 0, 0, 0, 0, "Table 5.2.2.2-4");
  expect(job(8, 4, 1, 0, 1, 1), MIPHY_EUNSUPP, 0, 0, 0, 0, 0, 0, "Table 5.2.2.2-4");
  expect(job(48, 2, 4, 0, 1, 1), MIPHY_EINVAL, 0, 0, 0, 0, 0, 0, "not a multiple of the ports that share the comb");
  expect(job(50, 2, 1, 0, 1, 1), MIPHY_EINVAL, 0, 0, 0, 0, 0, 0, "nof_prb is a multiple of 4");
  expect(job(48, 2, 1, 8, 1, 1), MIPHY_EINVAL, 0, 0, 0, 0, 0, 0, "cyclic_shift is below 8");
  expect(job(48, 2, 1, 0, 1, 3), MIPHY_EINVAL, 0, 0, 0, 0, 0, 0, "invalid symbol range");
  expect(job(48, 2, 3, 0, 1, 1), MIPHY_EINVAL, 0, 0, 0, 0, 0, 0, "invalid number of transmit ports");
  static_assert(sizeof(miphy_srs_job) == 48 && sizeof(miphy_srs_info_t) == 36 && sizeof(miphy_srs_result) == 168, "record sizes");
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_srs_estimator_and_the_info_call_answers_from_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "srs.cpp"), os.path.join(tmp, "srs")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
