"""CPU: the srsRAN adapter header compiles with the route to miphy_dmrs_pusch_estimate_tv_batch -- dmrs_pusch_estimator_hip(separate_layers,
compensate_cfo, time) and its factory -- the default strategy is still the average (the reference's rule), last_variation() starts at zero and the
job record has the layout the library expects. A small program is compiled against the reference's headers, linked with the reference archive of
oracle/_ref and the library, and run here; the device path is only compiled, its behaviour on the GPU is covered through the C ABI it calls
(tests/test_chest_tv_gpu.py). The processor adapter and the uplink processor's slot batch have no such option. Skipped where the reference tree or its
build is absent."""
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

// Compiled, never called: the estimator with a time strategy, made directly and through both factories.
float instantiate(std::shared_ptr<miphy::context> c, const resource_grid_reader& grid)
{
  miphy::dmrs_pusch_estimator_hip     e(c, true, true, miphy::time_strategy::interpolate);
  dmrs_pusch_estimator::configuration ecfg = {};
  ecfg.nof_tx_layers                       = 4;
  channel_estimate ce;
  e.estimate(ce, grid, ecfg);
  auto est = miphy::create_dmrs_pusch_estimator_factory_hip(c, true, true, miphy::time_strategy::line)->create();
  est->estimate(ce, grid, ecfg);
  auto est2 = std::make_shared<miphy::dmrs_pusch_estimator_factory_hip>(c, false, false, miphy::time_strategy::interpolate)->create();
  est2->estimate(ce, grid, ecfg);
  return e.last_cfo_hz() + e.last_cfo_rho() + e.last_variation() + e.last_variation(3, 3);
}

int main()
{
  int failed = 0;
  failed += sizeof(miphy_pusch_chest_tv_job) != 176 || offsetof(miphy_pusch_chest_tv_job, base) != 0 || sizeof(miphy_pusch_chest_cfo_job) != 160;
  failed += offsetof(miphy_pusch_chest_tv_job, var_offset) != 160 || offsetof(miphy_pusch_chest_tv_job, time_mode) != 168 ||
            offsetof(miphy_pusch_chest_tv_job, reserved) != 169;
  failed += MIPHY_TIME_INTERPOLATE != 1 || MIPHY_TIME_LINE != 2;
  std::shared_ptr<miphy::context> c; // construction never touches the device
  miphy::dmrs_pusch_estimator_hip plain(c), cfo(c, true, true), tv(c, true, true, miphy::time_strategy::line);
  failed += tv.last_variation() != 0.F || tv.last_variation(0, 0) != 0.F || tv.last_cfo_hz() != 0.F || plain.last_variation() != 0.F;
  failed += static_cast<int>(miphy::time_strategy::average) != 0; // the default of every constructor and factory
  failed += !miphy::create_dmrs_pusch_estimator_factory_hip(c)->create() || !miphy::create_dmrs_pusch_estimator_factory_hip(c, true, true)->create();
  failed += !miphy::create_dmrs_pusch_estimator_factory_hip(c, true, true, miphy::time_strategy::interpolate)->create();
  std::printf(failed ? "FAILED %d\n" : "OK\n", failed);
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_with_the_time_strategies():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pusch_tv.cpp"), os.path.join(tmp, "pusch_tv")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
