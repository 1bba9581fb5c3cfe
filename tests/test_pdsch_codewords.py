"""CPU: PDSCH on two codewords and 5..8 layers -- the host side of miphy_pdsch_modulate_codewords_batch / miphy_pdsch_process_codewords_batch (record
layouts through the binding, the two host size functions against a count in numpy), the fixture's own condition checked with the oracle alone -- for
every case, o_pdsch_modulate with two codeword arguments equals the numpy statement of TS 38.211 7.3.1.1-7.3.1.3 and Table 7.3.1.3-1 -- and the srsRAN
adapters compiled against the reference's headers with the validator's verdicts on two-codeword PDUs."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O
import pdsch_codewords_cases as CC
import pdsch_layers_cases as PC
from test_pdsch_layers import PKG, REF, REF_LIB, ROCM, ROOT
from test_pdsch_mapped import mod_mapped_job

CASES = CC.cases()
IDS = [c["name"] for c in CASES]
GARBAGE = dict(mod1=3, nof_bits1=12345, cw1_offset=1 << 40)  # what codeword 1 holds in a job of one codeword: ignored


def mod_codewords_job(miphy, c, list_off=None, cw_offs=(0, 0), grid_off=0):
    """The PdschModCodewordsJob record of a case of pdsch_codewords_cases, or of one of pdsch_layers_cases (one codeword: the fields of codeword 1 hold
    garbage); its list sits at list_off of the batch's list array (None: no list). The layers and ports inside the mapped job, and the ports behind
    the last layer, hold values no rule allows: they are ignored. Shared with the GPU tests."""
    j = np.zeros(1, dtype=miphy.PdschModCodewordsJob)[0]
    two = "mods" in c
    j["mapped"] = mod_mapped_job(miphy, CC.codeword_case(c, 0) if two else c, list_off, cw_off=cw_offs[0], grid_off=grid_off)
    j["mapped"]["layers"]["base"]["n_id"] = c["n_id"]
    j["mapped"]["layers"]["nof_layers"], j["mapped"]["layers"]["ports"] = 77, [99, 99, 98, 97]
    j["nof_layers"], j["ports"] = c["L"], 200
    j["ports"][:c["L"]] = c["ports8"][:c["L"]] if two else c["ports"]
    if two:
        L0, L1 = CC.split(c["L"])
        j["mod1"], j["nof_bits1"], j["cw1_offset"] = c["mods"][1], PC.nof_re(c) * L1 * c["mods"][1], cw_offs[1]
    else:
        j["mod1"], j["nof_bits1"], j["cw1_offset"] = GARBAGE["mod1"], GARBAGE["nof_bits1"], GARBAGE["cw1_offset"]
    return j


def test_record_layouts():
    """sizeof and the offsets of the new fields: the header's, through a small C program, against the binding's."""
    import miphy
    src = r"""
#include "miphy.h"
#include <stddef.h>
#include <stdio.h>
#define J miphy_pdsch_mod_codewords_job
#define P miphy_pdsch_codewords_pdu
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(J), offsetof(J, nof_layers), offsetof(J, mod1), offsetof(J, ports), offsetof(J, nof_bits1), offsetof(J, cw1_offset));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(P), offsetof(P, nof_layers), offsetof(P, ports), offsetof(P, bg1), offsetof(P, rv1), offsetof(P, mod1),
         offsetof(P, tb_bytes1), offsetof(P, tb_offset1));
  printf("%zu %zu\n", sizeof(miphy_pdsch_mod_mapped_job), sizeof(miphy_pdsch_mapped_pdu));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        cfile, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(cfile, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    m, p = miphy.PdschModCodewordsJob, miphy.PdschCodewordsPdu
    assert got[:6] == [m.itemsize] + [m.fields[f][1] for f in ("nof_layers", "mod1", "ports", "nof_bits1", "cw1_offset")] == [320, 296, 297, 298, 308, 312]
    assert got[6:14] == [p.itemsize] + [p.fields[f][1] for f in ("nof_layers", "ports", "bg1", "rv1", "mod1", "tb_bytes1", "tb_offset1")]
    assert got[6:14] == [344, 320, 321, 329, 330, 331, 332, 336]
    assert m.itemsize % 8 == 0 and p.itemsize % 8 == 0
    # the mapped records are the first member, unchanged
    assert got[14:] == [miphy.PdschModMappedJob.itemsize, miphy.PdschMappedPdu.itemsize] == [296, 320]
    assert m.fields["mapped"][1] == 0 and p.fields["mapped"][1] == 0 and m.fields["ports"][0].shape == (8,) and p.fields["ports"][0].shape == (8,)


def test_cases_cover_the_paths():
    assert {c["L"] for c in CASES} == {5, 6, 7, 8} and {c["type2"] for c in CASES} == {0, 1}
    assert {m for c in CASES for m in c["mods"]} == {1, 2, 4, 6, 8}
    assert any(c["reserved"] for c in CASES) and any(c["bwp"] != (0, c["nprb_grid"]) for c in CASES)
    assert any(c["cw_pads"][0] % 4 and not c["cw_pads"][1] for c in CASES) and any(c["cw_pads"][1] % 4 and not c["cw_pads"][0] for c in CASES)
    assert any(list(c["prbs"]) != sorted(c["prbs"]) for c in CASES) and any(max(c["ports8"]) == 15 for c in CASES)
    # a sequence of several pieces of 185 344 bits in each codeword
    assert any(PC.nof_re(c) * min(CC.split(c["L"])) * min(c["mods"]) > 2 * 185344 for c in CASES)


def test_interleaved_cases_hold_the_list_of_the_library():
    import miphy
    listed = [c for c in CASES if "vmap" in c]
    assert {c["L"] for c in listed} == {5, 8}
    for c in listed:
        got, pm = miphy.vrb_to_prb_list(*c["vmap"], vrbs=c["vrbs"])
        assert c["vmap"][0] == 2 and np.array_equal(got, c["prbs"]) and list(got) != sorted(got), c["name"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_grid_is_the_two_codewords_of_38211(c):
    """The fixture's own condition, with the oracle alone: the oracle grid equals, bit for bit, the background with codeword q put through
    PC.layer_symbols on its own layer count with c_init + q 2^14 onto ports[first_q ..], the data REs taken in list order."""
    bg = CC.background(c)
    g = bg.copy()
    rc = CC.oracle_modulate(c, g)
    want = CC.grid_from_38211(c, bg)
    diff = int((D.bits(g) != D.bits(want)).sum())
    print("%s: oracle returns %d for %d REs per layer, %d words differ" % (c["name"], rc, PC.nof_re(c), diff))
    assert rc == PC.nof_re(c) > 0
    assert diff == 0
    assert not np.array_equal(D.bits(g), D.bits(bg))


def test_oracle_refuses_one_codeword_argument_on_five_layers():
    c = CASES[0]
    assert c["L"] == 5
    rc = O.o_pdsch_modulate(c["rnti"], c["n_id"], c["scaling"], 5, [c["mods"][0]], [CC.codewords(c)[0] & 1], c["start"], c["nof"], PC.dmrs_mask(c), c["type2"], c["cdm"],
                            c["bwp"][0], c["bwp"][1], c["prbs"], c["reserved"], list(c["ports8"][:5]), c["nprb_grid"], CC.background(c))
    assert rc == -1


def test_oracle_dmrs_on_eight_ports_of_a_symbol_pair():
    """o_dmrs_pdsch_map on DM-RS ports 1000 .. 1007 of type 1 over the symbol pair (2, 3): 0, and 36 pilots on each of the eight grid ports."""
    rb = np.zeros(6, np.uint8)
    rb[[1, 2, 4]] = 1
    dm = np.zeros(14, np.uint8)
    dm[[2, 3]] = 1
    bg = D.background((8, 14, 72), np.random.default_rng(5))
    g = bg.copy()
    assert O.o_dmrs_pdsch_map(3, 0, 0, 77, 1, 1.0, dm, rb, list(range(8)), g) == 0
    assert [int((D.bits(g[p]) != D.bits(bg[p])).reshape(14, 72, 2).any(axis=-1).sum()) for p in range(8)] == [36] * 8
    assert not (D.bits(g[:, [0, 1] + list(range(4, 14))]) != D.bits(bg[:, [0, 1] + list(range(4, 14))])).any()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_size_functions_count_like_numpy(c):
    """miphy_pdsch_mod_codewords_nof_re and miphy_pdsch_codewords_pdu_nof_re against O.pdsch_nof_re (per layer: the count of the allocation), and 0 for
    L = 0 and L = 9."""
    import miphy
    j = mod_codewords_job(miphy, c, 0 if "vmap" in c else None)
    assert miphy.pdsch_mod_codewords_nof_re(j) == PC.nof_re(c) == int(PC.data_mask(c).sum()) > 0
    p = np.zeros(1, dtype=miphy.PdschCodewordsPdu)[0]
    b, m = p["mapped"]["layers"]["base"], j["mapped"]["layers"]["base"]
    for f in ("mod", "start_symbol", "nof_symbols", "nof_cdm_groups_without_data", "nof_reserved", "dmrs_symbols_mask", "grid_nof_prb", "bwp_start_rb", "bwp_size_rb",
              "rb_mask", "reserved"):
        b[f] = m[f]
    p["nof_layers"], p["ports"] = c["L"], j["ports"]
    if not c["type2"]:  # (the processor's DM-RS is of type 1)
        assert miphy.pdsch_codewords_pdu_nof_re(p) == PC.nof_re(c)
    for L in range(1, 9):
        j["nof_layers"] = p["nof_layers"] = L
        assert miphy.pdsch_mod_codewords_nof_re(j) == PC.nof_re(c) and (c["type2"] or miphy.pdsch_codewords_pdu_nof_re(p) == PC.nof_re(c))
    for bad in (0, 9, 255):
        j["nof_layers"] = p["nof_layers"] = bad
        assert miphy.pdsch_mod_codewords_nof_re(j) == 0 and miphy.pdsch_codewords_pdu_nof_re(p) == 0


TU = r"""
#include "miphy_srsran_adapters.h"
#include <cstdio>

// Compiled, never called: a modulator configuration and a PDU of two codewords on six layers through the adapters.
void instantiate(std::shared_ptr<miphy::context> c, srsran::resource_grid_writer& grid, srsran::upper_phy_rg_gateway& gateway)
{
  miphy::pdsch_modulator_hip          m(c);
  srsran::pdsch_modulator::config_t   cfg = {};
  cfg.ports = {0, 1, 2, 3, 4, 5};
  cfg.modulation1 = srsran::modulation_scheme::QAM256, cfg.modulation2 = srsran::modulation_scheme::QPSK;
  srsran::dynamic_bit_buffer            bits0(96), bits1(48);
  std::vector<srsran::bit_buffer>      cws;
  cws.emplace_back(bits0);
  cws.emplace_back(bits1);
  m.modulate(grid, cws, cfg);
  miphy::pdsch_processor_hip          p(c);
  srsran::pdsch_processor::pdu_t      pdu = {};
  pdu.ports = {5, 0, 1, 4, 2, 3};
  pdu.codewords.push_back(srsran::pdsch_processor::codeword_description{srsran::modulation_scheme::QAM64, 0});
  pdu.codewords.push_back(srsran::pdsch_processor::codeword_description{srsran::modulation_scheme::QAM16, 2});
  std::vector<uint8_t> tb0(100), tb1(60);
  srsran::static_vector<srsran::span<const uint8_t>, srsran::pdsch_processor::MAX_NOF_TRANSPORT_BLOCKS> data;
  data.emplace_back(tb0);
  data.emplace_back(tb1);
  p.process(grid, data, pdu);
  std::unique_ptr<srsran::downlink_processor> dl = miphy::create_downlink_processor_hip(c, gateway, 8, 106);
  dl->process_pdsch(data, pdu);
  dl->finish_processing_pdus();
}

int main()
{
  using namespace srsran;
  int  failed = 0;
  auto v      = std::make_shared<miphy::pdsch_processor_factory_hip>(nullptr)->create_validator();
  symbol_slot_mask dm(14);
  dm.set(2);
  dm.set(3);
  pdsch_processor::pdu_t pdu;
  pdu.slot = slot_point(1, 7), pdu.rnti = 0x4601, pdu.bwp_size_rb = 106, pdu.bwp_start_rb = 0, pdu.cp = cyclic_prefix::NORMAL;
  pdu.n_id = 321, pdu.ref_point = pdsch_processor::pdu_t::CRB0, pdu.dmrs_symbol_mask = dm, pdu.dmrs = dmrs_type::TYPE1, pdu.scrambling_id = 5, pdu.n_scid = false;
  pdu.nof_cdm_groups_without_data = 2, pdu.freq_alloc = rb_allocation::make_type1(4, 50), pdu.start_symbol_index = 0, pdu.nof_symbols = 14;
  pdu.ldpc_base_graph = ldpc_base_graph_type::BG1, pdu.tbs_lbrm_bytes = ldpc::MAX_CODEBLOCK_SIZE / 8;
  pdu.ratio_pdsch_dmrs_to_sss_dB = 0.0F, pdu.ratio_pdsch_data_to_sss_dB = 0.0F;
  auto check = [&](const char* what, unsigned nof_ports, unsigned nof_codewords, bool want, void (*edit)(pdsch_processor::pdu_t&) = nullptr) {
    pdsch_processor::pdu_t q = pdu;
    q.ports.clear();
    for (unsigned x = 0; x != nof_ports; ++x)
      q.ports.push_back(nof_ports - 1 - x); // distinct, descending
    for (unsigned k = 0; k != nof_codewords; ++k)
      q.codewords.push_back(pdsch_processor::codeword_description{k ? modulation_scheme::QAM16 : modulation_scheme::QAM256, k ? 2U : 0U});
    if (edit)
      edit(q);
    const bool got = v->is_valid(q);
    if (got != want) {
      std::printf("FAIL %s: got %d want %d\n", what, got, want);
      ++failed;
    }
  };
  check("two codewords on five ports", 5, 2, true);
  check("two codewords on six ports", 6, 2, true);
  check("two codewords on seven ports", 7, 2, true);
  check("two codewords on eight ports", 8, 2, true);
  check("two codewords on four ports", 4, 2, false);
  check("two codewords on two ports", 2, 2, false);
  check("one codeword on five ports", 5, 1, false);
  check("one codeword on eight ports", 8, 1, false);
  check("one codeword on four ports", 4, 1, true);
  check("two codewords on nine ports", 9, 2, false);
  check("three codewords on eight ports", 8, 3, false);
  check("two codewords, a port named twice", 6, 2, false, [](pdsch_processor::pdu_t& q) { q.ports[5] = q.ports[0]; });
  check("two codewords, DM-RS type 2", 6, 2, false, [](pdsch_processor::pdu_t& q) { q.dmrs = dmrs_type::TYPE2; });
  check("two codewords, one CDM group without data", 6, 2, false, [](pdsch_processor::pdu_t& q) { q.nof_cdm_groups_without_data = 1; });
  check("two codewords, a lone DM-RS symbol", 6, 2, false, [](pdsch_processor::pdu_t& q) {
    symbol_slot_mask one(14);
    one.set(2);
    q.dmrs_symbol_mask = one;
  });
  std::printf(failed ? "FAILED\n" : "OK\n");
  return failed;
}
"""


@pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "include", "srsran")) and os.path.exists(REF_LIB) and os.path.exists(os.path.join(PKG, "libmiphy.so"))),
                    reason="reference headers, oracle/_ref/libsrsran_ref.a or libmiphy.so not present")
def test_adapters_compile_and_the_validator_takes_two_codewords_on_five_to_eight_ports():
    """As tests/test_pdsch_layers.py does for layered PDUs: the header compiles against the reference's headers with a two-codeword modulator
    configuration, PDU and slot batch (compiled, not run: they need the device), and the validator's host logic is run."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pdsch_codewords.cpp"), os.path.join(tmp, "pdsch_codewords")
        open(src, "w").write(TU)
        cmd = ["g++", "-std=c++14", "-w", "-mavx2", "-mfma", "-DHAVE_AVX2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "adapters"),
               "-I", os.path.join(REF, "include"), "-I", os.path.join(REF, "external", "fmt", "include"), "-I", os.path.join(REF, "external"), "-I", REF,
               "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", src, REF_LIB, "-L", PKG, "-lmiphy", "-L", os.path.join(ROCM, "lib"),
               "-lamdhip64", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
