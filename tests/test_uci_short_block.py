"""CPU: the numpy restatement of the UCI short-block detector (tests/uci_short_block.py) against the reference's own detector
(tests/golden/short_block_detector.npz, recorded by tools/gen_short_block_golden.py through create_short_block_detector_factory_sw),
the TS 38.212 encoder round trip, and the host side of the device UCI decoder (record layout, PUSCH field jobs)."""
import os
import subprocess

import numpy as np
import pytest

import uci_short_block as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "short_block_detector.npz")


def _golden():
    return np.load(GOLDEN)


def test_restatement_equals_reference_fixture():
    d = _golden()
    n = d["K"].size
    for i in range(0, n, 7):  # the scalar form on a sample, the batch form (same arithmetic, vectorised fold) on every field
        K, mod, E, off, po = int(d["K"][i]), int(d["mod"][i]), int(d["E"][i]), int(d["llr_offset"][i]), int(d["payload_offset"][i])
        bits, st = U.detect(d["llr"][off:off + E], K, mod)
        assert np.array_equal(bits, d["payload"][po:po + K]), (i, K, mod, E)
        assert st == d["status"][i], (i, K, mod, E)
    bits, st = U.detect_batch(d["llr"], d["K"], d["mod"], d["E"], d["llr_offset"])
    assert np.array_equal(st, d["status"])
    assert np.array_equal(np.concatenate(bits), d["payload"])


def test_fixture_covers_the_space():
    d = _golden()
    K, mod, E, st = d["K"], d["mod"], d["E"], d["status"]
    for k in range(1, 12):
        for m in (1, 2, 4, 6, 8):
            sel = (K == k) & (mod == m)
            assert sel.any(), (k, m)
            assert E[sel].max() >= 2000 and (E[sel] % 2 == 1).any() and (E[sel] % 32 != 0).any()
            Emin = m if k == 1 else (3 * m if k == 2 else k + 1)
            assert E[sel].min() == Emin
        if k >= 3:  # both GLRT verdicts occur for every length the threshold applies to
            assert (st[K == k] == U.STATUS_VALID).any() and (st[K == k] == U.STATUS_INVALID).any(), k
    llr = d["llr"].astype(int)
    assert (llr == 127).any() and (llr == -127).any()
    assert any(not d["llr"][int(o):int(o) + int(e)].any() for o, e in zip(d["llr_offset"], d["E"]))  # an all-zero field


def test_saturating_sum():
    assert U.llr_add(127, -127) == 0 and U.llr_add(-127, 127) == 0
    assert U.llr_add(127, -5) == 127 and U.llr_add(-5, -127) == -127
    assert U.llr_add(100, 100) == 120 and U.llr_add(-100, -100) == -120 and U.llr_add(120, -100) == 20
    assert list(U.rate_dematch([100, 100, -100], 1)) == [20]  # not associative: 100 + (100 - 100) would be 100


def test_encoder_round_trip_clean_channel():
    rng = np.random.default_rng(5)
    for K in range(3, 12):
        msgs = ((np.arange(1 << K)[:, None] >> np.arange(K)[None, :]) & 1).astype(np.uint8)
        mods, Es, llr, offs = [], [], [], []
        o = 0
        for msg in msgs:
            mod = int(rng.choice([1, 2, 4, 6, 8]))
            E = int(rng.integers(32, 200))  # the whole codeword at least once
            x = (1 - 2 * U.rate_match(U.encode(msg, mod), E).astype(np.int64)) * int(rng.integers(1, 121))
            mods.append(mod), Es.append(E), llr.append(x), offs.append(o)
            o += E
        bits, st = U.detect_batch(np.concatenate(llr), np.full(len(msgs), K), mods, Es, offs)
        assert np.array_equal(np.array(bits), msgs), K
        assert (st == U.STATUS_VALID).all()  # a clean codeword: metric +inf
    for K in (1, 2):
        for mod in (1, 2, 4, 6, 8):
            for v in range(1 << K):
                msg = np.array([(v >> k) & 1 for k in range(K)], np.uint8)
                cw = U.encode(msg, mod)
                bits, _ = U.detect((1 - 2 * U.rate_match(cw, 3 * len(cw)).astype(np.int64)) * 7, K, mod)
                assert np.array_equal(bits, msg), (K, mod, v)


def test_uci_field_job_layout_matches_header():
    import miphy
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "miphy.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(miphy_uci_field_job), offsetof(miphy_uci_field_job, mod), offsetof(miphy_uci_field_job, nof_llr),
         offsetof(miphy_uci_field_job, llr_offset), offsetof(miphy_uci_field_job, payload_offset), sizeof(miphy_pusch_uci),
         MIPHY_UCI_STATUS_UNKNOWN, MIPHY_UCI_STATUS_VALID, MIPHY_UCI_STATUS_INVALID);
  return 0;
}
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "layout")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    J = miphy.UciFieldJob
    assert vals[:5] == [J.itemsize, J.fields["mod"][1], J.fields["nof_llr"][1], J.fields["llr_offset"][1], J.fields["payload_offset"][1]]
    assert vals[5] == miphy.PuschUci.itemsize
    assert vals[6:] == [miphy.UCI_STATUS_UNKNOWN, miphy.UCI_STATUS_VALID, miphy.UCI_STATUS_INVALID]


def _pdus_uci(rows):
    import miphy
    pdus = np.zeros(len(rows), miphy.PuschPdu)
    uci = np.zeros(len(rows), miphy.PuschUci)
    for i, (mod, O, G, off) in enumerate(rows):
        pdus[i]["mod"] = mod
        u = uci[i]
        u["nof_harq_ack_bits"], u["nof_csi_part1_bits"], u["nof_csi_part2_bits"] = O
        u["nof_enc_harq_ack_bits"], u["nof_enc_csi_part1_bits"], u["nof_enc_csi_part2_bits"] = G
        u["harq_ack_offset"], u["csi_part1_offset"], u["csi_part2_offset"] = off
    return pdus, uci


def test_pusch_uci_field_jobs_host_helper():
    import miphy
    pdus, uci = _pdus_uci([(4, (1, 0, 7), (20, 0, 96), (0, 20, 20)),
                           (2, (0, 0, 0), (0, 0, 0), (116, 116, 116)),
                           (6, (2, 11, 3), (18, 120, 42), (116, 134, 254))])
    jobs, field = miphy.pusch_uci_field_jobs(pdus, uci)
    assert list(field) == [0, 2, 6, 7, 8]
    assert list(jobs["nof_bits"]) == [1, 7, 2, 11, 3]
    assert list(jobs["mod"]) == [4, 4, 6, 6, 6]
    assert list(jobs["nof_llr"]) == [20, 96, 18, 120, 42]
    assert list(jobs["llr_offset"]) == [0, 20, 116, 134, 254]
    assert list(jobs["payload_offset"]) == [0, 1, 8, 10, 21]
    # a polar-coded field (more than 11 bits) and a field the detector refuses are errors
    for bad in ([(4, (12, 0, 0), (40, 0, 0), (0, 0, 0))], [(4, (5, 0, 0), (5, 0, 0), (0, 0, 0))], [(4, (2, 0, 0), (8, 0, 0), (0, 0, 0))]):
        with pytest.raises(RuntimeError, match="miphy error -1"):
            miphy.pusch_uci_field_jobs(*_pdus_uci(bad))
