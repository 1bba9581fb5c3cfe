"""CPU: the srsRAN adapter header compiles with the device UCI decoder taking polar-coded fields (uci_decoder_hip::decode on a message
of 12 to 1706 bits, pusch_processor_hip over miphy_pusch_uci_jobs with both decoders behind it) against the reference's headers, and
the C ABI of these entry points is the one the header declares. Skipped where the reference tree is absent; the adapters' behaviour
on the GPU is covered through the C ABI they call (tests/test_uci_polar_gpu.py)."""
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
  // a 20-bit CSI report in 120 soft bits and a 1706-bit field: the polar path of uci_decoder_hip
  std::vector<uint8_t>                      msg(20), big(1706);
  std::vector<srsran::log_likelihood_ratio> llr(120), many(3500);
  srsran::uci_decoder::configuration        cfg;
  cfg.modulation       = srsran::modulation_scheme::QPSK;
  srsran::uci_status s = dec->decode(msg, llr, cfg);
  s                    = dec->decode(big, many, cfg);
  // the validator the factory hands to the upper PHY, on a PDU with a 20-bit CSI part 1
  std::unique_ptr<srsran::pusch_pdu_validator> val = factory.create_validator();
  srsran::pusch_processor::pdu_t               pdu = {};
  pdu.uci.nof_csi_part1                            = 20;
  bool valid                                       = val->is_valid(pdu);
  (void)valid;
  // the C ABI the adapters call
  int (*info)(uint32_t, uint32_t, miphy_uci_polar_info_t*) = &miphy_uci_polar_info;
  int (*run)(miphy_ctx*, const miphy_uci_polar_job*, uint32_t, const int8_t*, uint8_t*, uint8_t*, void*) = &miphy_uci_polar_decode_batch;
  int (*jobs)(const miphy_pusch_pdu*, const miphy_pusch_uci*, uint32_t, miphy_uci_field_job*, uint32_t*, uint32_t*, miphy_uci_polar_job*, uint32_t*,
              uint32_t*)                                   = &miphy_pusch_uci_jobs;
  static_assert(sizeof(miphy_uci_polar_job) == 24 && sizeof(miphy_uci_polar_info_t) == 24, "records of the polar-coded UCI decoder");
  (void)det, (void)dec, (void)proc, (void)p, (void)s, (void)info, (void)run, (void)jobs;
}
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "srsran")), reason="reference headers not present")
def test_adapter_header_compiles_with_polar_coded_uci_fields():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "uci_polar_adapters.cpp")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-fsyntax-only", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(ROOT, "srsran_project_23.5_amd", "adapters"), "-I", os.path.join(REF, "include"),
               "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
