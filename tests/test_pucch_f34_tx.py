"""CPU: the numpy transmitter of PUCCH formats 3 and 4 (tests/pucch_f34_tx.py) against itself and against the float64 receiver
(tests/pucch_f34_ref.py): the orthogonal sequences, the cancellation of the co-scheduled DM-RS under the block average, the soft-bit count E
of every length, and a round trip of every payload class at 30 dB. The cases of the GPU test (tests/test_pucch_f34_gpu.py) that depend on
what a noisy channel does to the decoders (tests/pucch_f34_cases.py) are checked here with the float64 receiver first."""
import itertools

import numpy as np
import pytest

import pucch_f34_ref as R
import pucch_f34_tx as X

# data symbols of every length (without additional DM-RS, with it), from the DM-RS tables of the issue
DATA_SYMBOLS = {4: (3, 3), 5: (3, 3), 6: (4, 4), 7: (5, 5), 8: (6, 6), 9: (7, 7), 10: (8, 6), 11: (9, 7), 12: (10, 8), 13: (11, 9), 14: (12, 10)}


@pytest.mark.parametrize("nsf", [2, 4])
def test_orthogonal_sequences(nsf):
    w = np.array([X.occ_w(nsf, n) for n in range(nsf)])
    assert np.allclose(np.abs(w), 1)
    per = 12 // nsf
    for j in range(per):  # over every group {j + q 12 / N_SF} the rows are orthogonal
        g = w[:, j::per]
        assert g.shape == (nsf, nsf) and np.allclose(g @ g.conj().T, nsf * np.eye(nsf))
    for n in range(nsf):  # constant over each run of 12 / N_SF elements
        assert all(len(set(np.round(w[n, q * per:(q + 1) * per], 12))) == 1 for q in range(nsf))


@pytest.mark.parametrize("nsf", [2, 4])
def test_dmrs_of_the_other_sequences_cancel_under_the_block_average(nsf):
    pdus = [X.pdu(4, 14, occ_len=nsf, occ_idx=n, nid_hop=77, slot=5) for n in range(nsf)]
    for l in (3, 10):
        r = [X.dmrs_sequence(p, l) for p in pdus]
        for a, b in itertools.permutations(range(nsf), 2):
            blocks = (r[b] * r[a].conj()).reshape(-1, nsf).mean(axis=1)
            assert np.abs(blocks).max() < 1e-12, (a, b)
        assert np.allclose((r[0] * r[0].conj()).reshape(-1, nsf).mean(axis=1), 1)


def test_soft_bit_counts():
    n = 0
    for nsym, hop, add in itertools.product(range(4, 15), (0, 1), (0, 1)):
        dmrs, data = X.layout(nsym, hop, add)
        nd = DATA_SYMBOLS[nsym][add] - (1 if nsym == 4 and hop else 0)
        assert len(data[0]) + len(data[1]) == nd and len(dmrs[0]) + len(dmrs[1]) == nsym - nd
        assert sorted(dmrs[0] + dmrs[1] + data[0] + data[1]) == list(range(nsym))
        if hop:
            assert len(dmrs[0]) == len(dmrs[1]) >= 1 and max(dmrs[0] + data[0]) == nsym // 2 - 1
        for nprb, pi2 in itertools.product(X.F3_NPRB, (0, 1)):
            assert X.nof_soft_bits(X.pdu(3, nsym, nprb, hop, add, pi2)) == (1 if pi2 else 2) * 12 * nprb * nd
        for nsf, pi2 in itertools.product((2, 4), (0, 1)):
            assert X.nof_soft_bits(X.pdu(4, nsym, 1, hop, add, pi2, nsf, 1)) == (1 if pi2 else 2) * (12 // nsf) * nd
        n += 1
    assert n == 44
    assert X.nof_soft_bits(X.pdu(4, 4, 1, 1, 0, 1, 4, 0)) == 6  # the smallest there is


ROUND_TRIPS = [  # (format, nsym, nprb, hop, add, pi2, occ_len, occ_idx, ports, K)
    (3, 4, 1, 0, 0, 0, 0, 0, 1, 3), (3, 4, 1, 1, 0, 1, 0, 0, 2, 11), (3, 5, 3, 0, 0, 0, 0, 0, 1, 12), (3, 9, 5, 1, 0, 1, 0, 0, 4, 19),
    (3, 10, 15, 0, 1, 0, 0, 0, 2, 20), (3, 14, 16, 1, 1, 0, 0, 0, 1, 400), (3, 14, 4, 0, 0, 1, 0, 0, 1, 100), (4, 4, 1, 1, 0, 1, 4, 3, 1, 3),
    (4, 14, 1, 0, 1, 0, 2, 1, 2, 12), (4, 14, 1, 1, 0, 0, 4, 2, 1, 20), (4, 7, 1, 0, 0, 1, 2, 0, 4, 8)]


@pytest.mark.parametrize("case", ROUND_TRIPS, ids=lambda c: "f%d-%dsym-%dprb-K%d" % (c[0], c[1], c[2], c[9]))
def test_the_float64_receiver_recovers_the_payload_at_30_db(case):
    fmt, nsym, nprb, hop, add, pi2, nsf, idx, ports, K = case
    rng = np.random.default_rng(sum(case))
    p = X.pdu(fmt, nsym, nprb, hop, add, pi2, nsf, idx, nports=ports, prb=2, prb2=30, grid_nprb=52, nid_hop=int(rng.integers(0, 1024)),
              nid_scr=int(rng.integers(0, 1024)), rnti=int(rng.integers(1, 65520)), slot=int(rng.integers(0, 20)))
    bits = rng.integers(0, 2, K).astype(np.uint8)
    grid = X.build_grid(7 + K, ports, 52, 10 ** (-30 / 20), [p], [bits])
    out = R.receive(p, grid, K)
    assert np.array_equal(out["bits"], bits)
    # (six soft bits, the smallest E there is, cannot reach the short-block detector's threshold: the bits are right, the verdict is INVALID)
    assert out["status"] == (2 if X.nof_soft_bits(p) == 6 else 1)
    assert out["llr"].size == X.nof_soft_bits(p)
    assert abs(out["csi"]["epre_db"] - out["csi"]["rsrp_db"]) < 0.5


def test_the_multiplexed_format4_pdus_of_the_gpu_test_decode_at_20_db():
    import pucch_f34_cases as G
    for nsf in (2, 4):
        pdus, bits, grid = G.multiplexed(nsf)
        for p, b in zip(pdus, bits):
            out = R.receive(p, grid, len(b))
            assert out["status"] == 1 and np.array_equal(out["bits"], b), (nsf, p["occ_idx"])


def test_the_noisy_set_of_the_gpu_test_has_both_verdicts_in_each_class():
    import pucch_f34_cases as G
    seen = {"short": set(), "crc6": set(), "crc11": set()}
    for d in G.noisy_set():
        out = R.receive(d["pdu"], d["grid"], d["K"])
        seen[G.klass(d["K"])].add(out["status"])
    assert all(v == {1, 2} for v in seen.values()), seen


def test_the_clean_sets_of_the_gpu_test_decode_with_the_float64_receiver():
    import pucch_f34_cases as G
    items = [d for nports in G.PORTS for d in G.f3_set(nports)] + G.f4_set() + G.mixed_items()
    assert len(items) == 3 * 71 + 24 + 8
    for d in items:
        out = R.receive(d["pdu"], d["grid"], d["K"])
        assert np.array_equal(out["bits"], d["bits"]), (d["pdu"], d["K"])
        if d["K"] > 11 or out["llr"].size >= 32:  # (a short-block codeword cut below its 32 bits may stay under the detector's threshold)
            assert out["status"] == 1, (d["pdu"], d["K"])
