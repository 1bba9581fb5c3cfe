"""CPU: the srsRAN adapter header compiles with the device PUCCH processor (pucch_processor_hip with and without a CPU processor for
formats 0, 3 and 4, its batched method, pucch_pdu_validator_hip and the factory, handed to uplink_processor_hip's factory argument type)
against the reference's headers. Skipped where the reference tree is absent; the adapters' behaviour on the GPU is covered through the C
ABI they call (tests/test_pucch_proc_gpu.py)."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

TU = r"""
#include "miphy_srsran_adapters.h"

void instantiate(std::shared_ptr<miphy::context> c, std::shared_ptr<srsran::pucch_processor_factory> cpu_factory,
                 const srsran::resource_grid_reader& grid)
{
  srsran::channel_estimate::channel_estimate_dimensions dims;
  dims.nof_prb = 273, dims.nof_symbols = 14, dims.nof_rx_ports = 4, dims.nof_tx_layers = 1;
  std::shared_ptr<srsran::pucch_processor_factory> f  = miphy::create_pucch_processor_factory_hip(c, dims, cpu_factory);
  std::unique_ptr<srsran::pucch_processor>         p  = f->create();
  std::unique_ptr<srsran::pucch_pdu_validator>     v  = f->create_validator();
  miphy::pucch_processor_hip                       gpu_only(c);
  srsran::pucch_processor::format1_configuration   c1;
  srsran::pucch_processor::format2_configuration   c2;
  srsran::pucch_processor_result                   r1 = p->process(grid, c1), r2 = gpu_only.process(grid, c2);
  std::vector<srsran::pucch_processor::format1_configuration> b1(3);
  std::vector<srsran::pucch_processor::format2_configuration> b2(2);
  std::vector<srsran::pucch_processor_result>                 o1(3), o2(2);
  gpu_only.process_batch(grid, b1, b2, o1, o2);
  bool ok = v->is_valid(c1) && v->is_valid(c2);
  (void)r1, (void)r2, (void)ok;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "srsran")), reason="reference headers not present")
def test_adapter_header_compiles_with_device_pucch_processor():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "pucch_adapters.cpp")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "srsran_project_23.5_amd", "adapters"), "-I", os.path.join(REF, "include"),
               "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
