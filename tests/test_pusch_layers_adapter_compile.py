"""CPU: the srsRAN adapter header compiles with the layered PUSCH paths -- channel_equalizer_hip sending topologies beyond 1 x N / 2 x 2 to
miphy_channel_equalize_layers_batch, pusch_demodulator_hip taking config.nof_tx_layers 1..4 through miphy_pusch_demodulate_layers_batch -- and
the job type the adapter fills has the layout the library expects. A small program is compiled against the reference's headers, linked with the
reference archive of oracle/_ref and the library, and run here; the device paths are only compiled, their behaviour on the GPU is covered through
the C ABI they call (tests/test_equalizer_layers_gpu.py, tests/test_pusch_demod_layers_gpu.py). Skipped where the reference tree or its build is
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
#include <cstddef>
#include <cstdio>

// Compiled, never called: four layers on four ports through both adapters.
void instantiate(std::shared_ptr<miphy::context> c, const srsran::resource_grid_reader& grid, const srsran::channel_estimate& estimates)
{
  using eq = srsran::channel_equalizer;
  srsran::dynamic_tensor<2, srsran::cf_t, eq::re_list::dims>     y({100, 4}), z({100, 4});
  srsran::dynamic_tensor<2, float, eq::re_list::dims>            v({100, 4});
  srsran::dynamic_tensor<3, srsran::cf_t, eq::ch_est_list::dims> h({100, 4, 4});
  std::vector<float>                                              nvars(4, 0.1F);
  miphy::channel_equalizer_hip                                    q(c);
  q.equalize(z, v, y, h, nvars, 1.0F);
  miphy::pusch_demodulator_hip               d(c);
  srsran::pusch_demodulator::configuration   cfg = {};
  cfg.nof_tx_layers                                = 4;
  cfg.rx_ports                                     = {0, 1, 2, 3};
  std::vector<srsran::log_likelihood_ratio> cw(64);
  d.demodulate(cw, grid, estimates, cfg);
}

int main()
{
  int failed = 0;
  miphy_pusch_demod_layers_job j = {};
  j.nof_tx_layers               = 3;
  j.base.nof_rx_ports           = 2;
  failed += sizeof(miphy_pusch_demod_layers_job) != 128 || offsetof(miphy_pusch_demod_layers_job, nof_tx_layers) != 120;
  failed += miphy_pusch_demod_layers_nof_llr(&j) != 0; // more layers than ports
  j.base.nof_rx_ports = 4, j.base.mod = 4, j.base.nof_symbols = 14, j.base.dmrs_type = 1, j.base.nof_cdm_groups_without_data = 2;
  j.base.dmrs_symbols_mask = 1u << 2, j.base.grid_nof_prb = 24, j.base.rb_mask[0] = 0xff;
  failed += miphy_pusch_demod_layers_nof_llr(&j) != 8u * 12u * 13u * 3u * 4u;
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_layered_pusch_paths():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pusch_layers.cpp"), os.path.join(tmp, "pusch_layers")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
