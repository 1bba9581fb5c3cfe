"""CPU: the framing of polar-coded UCI fields. The library's host functions (miphy_uci_polar_info, miphy_pusch_uci_jobs) against the
restatement of tests/uci_polar.py, and the restatement's own round trip through the oracle's polar chains."""
import re

import numpy as np
import pytest

import miphy
import uci_polar as U

ALL_A = range(U.MIN_BITS, U.MAX_BITS + 1)
KEYS = ("C", "L", "K_r", "E_r", "n", "nPC")


def lib_info(A, E):
    """(dict, "") where the library accepts the field, (None, message) where it answers MIPHY_EINVAL."""
    try:
        o = miphy.uci_polar_info(A, E)
    except RuntimeError as e:
        m = re.match(r"miphy error (-?\d+): (.*)", str(e), re.S)
        assert int(m.group(1)) == -1, str(e)
        return None, m.group(2)
    return {k: int(o[k]) for k in KEYS}, ""


def test_info_equals_the_restatement_for_every_length():
    accepted = rejected = 0
    for A in ALL_A:
        for E in (U.min_E(A), 1087, 1088, 2 * A + 301, 8192, 8193, 16384, 16385):  # 2 A + 301 is odd
            want = U.info(A, E)
            got, msg = lib_info(A, E)
            if want is None:
                assert got is None and msg, (A, E, got)
                rejected += 1
            else:
                assert got == {k: want[k] for k in KEYS}, (A, E, got, want)
                accepted += 1
    assert accepted > 8000 and rejected > 1000, (accepted, rejected)


def test_the_shapes_checked_with_the_oracle():
    for A, E in ((12, 19), (19, 28)):
        assert U.info(A, E) is None and lib_info(A, E)[0] is None, (A, E)
    for A, E in ((12, 32), (19, 216), (20, 8192), (1012, 1087), (1706, 1760)):
        assert U.info(A, E) is not None and lib_info(A, E)[0] is not None, (A, E)
    assert U.info(1012, 1087)["K_r"] == 1023 and U.info(1012, 1088)["C"] == 2
    assert U.info(361, 1089)["pad"] == 1 and U.info(19, 215)["nPC"] == 3


@pytest.mark.parametrize("A,E,rule", [
    (11, 64, "12 to 1706"), (1707, 4000, "12 to 1706"), (0, 64, "12 to 1706"),
    (12, 21, "K_r + nPC < E_r"), (19, 28, "K_r + nPC < E_r"), (20, 31, "K_r + nPC < E_r"), (1706, 1729, "K_r + nPC < E_r"),
    (20, 8193, "exceeds 8192"), (359, 8193, "exceeds 8192"), (1706, 16386, "exceeds 8192"), (360, 16386, "exceeds 8192"),
])
def test_info_rejects_with_the_rule(A, E, rule):
    got, msg = lib_info(A, E)
    assert got is None and rule in msg, (A, E, msg)
    assert U.info(A, E) is None


def test_the_last_accepted_and_first_rejected_lengths():
    for A in (12, 19, 20, 359, 360, 1012, 1013, 1706):
        E = U.min_E(A)
        assert lib_info(A, E)[0] is not None and lib_info(A, E - 1)[0] is None, (A, E)
        f = U.info(A, E)
        assert f["K_r"] + f["nPC"] + 1 == f["E_r"], (A, E, f)
    assert lib_info(20, 8192)[0] is not None and lib_info(1706, 16385)[0] is not None and lib_info(1706, 16384)[0]["E_r"] == 8192


def test_crc_length_is_the_one_the_reference_sizes_fields_with():
    # get_crc_size_uci (lib/ran/pusch/ulsch_info.cpp:29-42): 0 below 12 bits, 6 from 12 to 19 bits, 11 from 20 bits
    for A in ALL_A:
        assert U.info(A, 16000 if A >= 1013 else 8000)["L"] == (6 if A < 20 else 11), A
        assert lib_info(A, 16000 if A >= 1013 else 8000)[0]["L"] == (6 if A < 20 else 11), A


def test_restatement_round_trip_for_every_length():
    rng = np.random.default_rng(20241)
    two = 0
    for A in ALL_A:
        for E in (U.min_E(A), max(1089, 3 * A + 1) if A >= 360 else 3 * A + 1):
            f = U.info(A, E)
            assert f is not None, (A, E)
            two += f["C"] == 2
            x = rng.integers(0, 2, A).astype(np.uint8)
            tx = U.encode(A, E, x)
            assert tx.size == E
            got, valid = U.decode(A, E, (100 * (1 - 2 * tx.astype(np.int32))).astype(np.int8))
            assert valid and np.array_equal(got, x), (A, E)
    assert two > 1300


def _pdus_uci(rows):
    """rows: (mod, (O_ack, G_ack), (O_csi1, G_csi1), (O_csi2, G_csi2)) per PDU; the three streams of a PDU lie one after the other."""
    pdus, uci = np.zeros(len(rows), miphy.PuschPdu), np.zeros(len(rows), miphy.PuschUci)
    pos = 0
    for i, (mod, ack, c1, c2) in enumerate(rows):
        pdus[i]["mod"] = mod
        for name, enc, off, (O, G) in (("nof_harq_ack_bits", "nof_enc_harq_ack_bits", "harq_ack_offset", ack),
                                       ("nof_csi_part1_bits", "nof_enc_csi_part1_bits", "csi_part1_offset", c1),
                                       ("nof_csi_part2_bits", "nof_enc_csi_part2_bits", "csi_part2_offset", c2)):
            uci[i][name], uci[i][enc], uci[i][off] = O, G, pos
            pos += G
    return pdus, uci


def test_pusch_uci_jobs_splits_and_packs():
    rows = [(2, (2, 60), (20, 200), (0, 0)), (4, (12, 96), (0, 0), (0, 0)), (6, (0, 0), (7, 90), (400, 1200)), (2, (1706, 3500), (11, 64), (12, 40))]
    pdus, uci = _pdus_uci(rows)
    sj, sf, pj, pf = miphy.pusch_uci_jobs(pdus, uci)
    assert list(sf) == [0, 7, 10] and list(pf) == [1, 3, 8, 9, 11]
    # one payload buffer in (PDU, field) order
    order, pos = {}, 0
    for i, row in enumerate(rows):
        for k, (O, G) in enumerate(row[1:]):
            if O:
                order[3 * i + k] = (O, G, pos, int(uci[i][("harq_ack_offset", "csi_part1_offset", "csi_part2_offset")[k]]), row[0])
                pos += O
    for j, fld in zip(sj, sf):
        O, G, p, off, mod = order[int(fld)]
        assert (int(j["nof_bits"]), int(j["nof_llr"]), int(j["payload_offset"]), int(j["llr_offset"]), int(j["mod"])) == (O, G, p, off, mod)
    for j, fld in zip(pj, pf):
        O, G, p, off, _ = order[int(fld)]
        assert (int(j["nof_bits"]), int(j["nof_llr"]), int(j["payload_offset"]), int(j["llr_offset"]), int(j["reserved"])) == (O, G, p, off, 0)


def test_pusch_uci_jobs_equals_field_jobs_without_long_fields():
    pdus, uci = _pdus_uci([(2, (2, 60), (11, 200), (0, 0)), (4, (1, 96), (5, 40), (3, 33)), (8, (0, 0), (0, 0), (0, 0))])
    jobs, field = miphy.pusch_uci_field_jobs(pdus, uci)
    sj, sf, pj, pf = miphy.pusch_uci_jobs(pdus, uci)
    assert pj.size == 0 and pf.size == 0 and sj.tobytes() == jobs.tobytes() and np.array_equal(sf, field)


@pytest.mark.parametrize("row,rule", [((2, (12, 19), (0, 0), (0, 0)), "K_r + nPC < E_r"), ((2, (0, 0), (1707, 5000), (0, 0)), "12 to 1706"),
                                      ((2, (0, 0), (0, 0), (20, 8193)), "exceeds 8192"), ((3, (2, 60), (0, 0), (0, 0)), "invalid field")])
def test_pusch_uci_jobs_rejects(row, rule):
    pdus, uci = _pdus_uci([(2, (2, 60), (20, 200), (0, 0)), row])
    with pytest.raises(RuntimeError, match=r"miphy error -1: .*" + re.escape(rule)):
        miphy.pusch_uci_jobs(pdus, uci)


def test_field_jobs_keep_rejecting_a_long_field():
    pdus, uci = _pdus_uci([(2, (12, 96), (0, 0), (0, 0))])
    with pytest.raises(RuntimeError, match="miphy error -1"):
        miphy.pusch_uci_field_jobs(pdus, uci)
