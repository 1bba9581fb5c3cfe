"""CPU: the srsRAN adapter header compiles with the device PRACH blocks (prach_generator_hip, prach_detector_hip with its batched method,
prach_detector_validator_hip and the two factories, the detector handed to uplink_processor_hip's constructor argument type) against the
reference's headers. Skipped where the reference tree is absent; the adapters' behaviour on the GPU is covered through the C ABI they
call (tests/test_prach_gpu.py)."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

TU = r"""
#include "miphy_srsran_adapters.h"

void instantiate(std::shared_ptr<miphy::context> c, const srsran::prach_buffer& buffer, const srsran::prach_buffer& other)
{
  std::shared_ptr<srsran::prach_detector_factory>   df = miphy::create_prach_detector_factory_hip(c);
  std::shared_ptr<srsran::prach_detector_factory>   d2 = miphy::create_prach_detector_factory_hip(c, 3072);
  std::shared_ptr<srsran::prach_generator_factory>  gf = miphy::create_prach_generator_factory_hip(c);
  std::unique_ptr<srsran::prach_detector>           d  = df->create();
  std::unique_ptr<srsran::prach_detector_validator> v  = df->create_validator();
  std::unique_ptr<srsran::prach_generator>          g  = gf->create();
  srsran::prach_detector::configuration             dc = {};
  srsran::prach_generator::configuration            gc = {};
  srsran::prach_detection_result                    r  = d->detect(buffer, dc);
  srsran::span<const srsran::cf_t>                  y  = g->generate(gc);
  miphy::prach_detector_hip                         batched(c, 1536);
  const srsran::prach_buffer*                       bufs[2] = {&buffer, &other};
  std::vector<srsran::prach_detector::configuration> cfgs(2);
  std::vector<srsran::prach_detection_result>        outs(2);
  batched.detect_batch(bufs, cfgs, outs);
  bool ok = v->is_valid(dc);
  (void)r, (void)y, (void)ok, (void)d2;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "srsran")), reason="reference headers not present")
def test_adapter_header_compiles_with_device_prach_blocks():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "prach_adapters.cpp")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "srsran_project_23.5_amd", "adapters"), "-I", os.path.join(REF, "include"),
               "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
