"""CPU: the srsRAN adapter header compiles with the device UCI decoder (short_block_detector_hip, uci_decoder_hip, their factories, and a
uci_decoder_hip handed to pusch_processor_hip) against the reference's headers. Skipped where the reference tree is absent; the
adapters' behaviour on the GPU is covered through the C ABI they call (tests/test_uci_decode_gpu.py)."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

TU = r"""
#include "miphy_srsran_adapters.h"

void instantiate(std::shared_ptr<miphy::context> c)
{
  std::shared_ptr<srsran::short_block_detector_factory> sbd = miphy::create_short_block_detector_factory_hip(c);
  std::unique_ptr<srsran::short_block_detector>         det = sbd->create();
  std::shared_ptr<srsran::uci_decoder_factory>          ucf = miphy::create_uci_decoder_factory_hip(c);
  std::unique_ptr<srsran::uci_decoder>                  dec = ucf->create();
  miphy::pusch_processor_hip proc(c, 6, true, std::make_unique<miphy::uci_decoder_hip>(c));
  miphy::pusch_processor_factory_hip factory(c, 6, true, ucf);
  std::unique_ptr<srsran::pusch_processor> p = factory.create();
  (void)det, (void)dec, (void)proc, (void)p;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "srsran")), reason="reference headers not present")
def test_adapter_header_compiles_with_device_uci_decoder():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "uci_adapters.cpp")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "srsran_project_23.5_amd", "adapters"), "-I", os.path.join(REF, "include"),
               "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
