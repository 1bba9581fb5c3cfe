"""CPU: what the float64 receiver of tests/pucch_f0_ref.py makes of the PDU sets of tests/pucch_f0_cases.py, and the closed-form thresholds against
direct draws of the statistic. The GPU tests (tests/test_pucch_f0_gpu.py) compare the device with this receiver and rely on what is recorded
here: in the deterministic sets no decision is close enough to flip in single precision, in the noise set at most 1 % of the PDUs are."""
import numpy as np
import pytest

import pucch_f0_cases as G
import pucch_f0_ref as R
import pucch_f0_tx as X


@pytest.mark.parametrize("name", G.DETERMINISTIC)
def test_every_pdu_sent_at_20_db_decodes_its_own_bits_and_is_valid(name):
    items, refs = G.SETS[name](), G.reference(name)
    sent = 0
    for i, (d, r) in enumerate(zip(items, refs)):
        if d["hyp"] is None:
            continue
        p = d["pdu"]
        assert r["status"] == R.VALID, (name, i, r["metric"], r["threshold"])
        assert list(r["bits"]) == X.hypothesis_bits(p["nharq"], p["nsr"], d["hyp"]), (name, i)
        sent += 1
    assert sent >= 2


def test_the_shapes_set_covers_what_the_gpu_test_says_it_does():
    items = G.shapes_set()
    pd = [d["pdu"] for d in items]
    assert {p["nports"] for p in pd} == {1, 2, 3, 4} and {(p["nsym"], p["hop"]) for p in pd} == set(G.SHAPES)
    seen = {(p["nharq"], p["nsr"], d["hyp"]) for p, d in zip(pd, items)}
    assert seen == {(a, s, h) for a, s in G.UCI for h in list(range(len(X.hypotheses_mcs(a, s)))) + [None]}
    assert {p["ics"] for p in pd} == set(range(12)) and {p["start"] for p in pd} >= {13, 12, 0}
    assert {p["numerology"] for p in pd} == {0, 1} and min(p["slot"] for p in pd) == 0 < max(p["slot"] for p in pd)
    assert any(p["noise_var"] > 0 for p in pd) and any(p["threshold"] > 0 for p in pd) and any(p["mask"] for p in pd)
    assert 200 <= len(items) <= 400


def test_the_noise_only_set_has_at_most_64_valid_verdicts():
    """4096 PDUs at a false-alarm probability of at most 1 % each: the expectation is at most 41, and 64 is a little over three and a half binomial
    standard deviations above it."""
    items, refs = G.noise_set(), G.reference("noise")
    assert len(items) == G.NOISE_PDUS
    dfh = {(d["pdu"]["nports"] * d["pdu"]["nsym"], bin(R.free_mask(d["pdu"])).count("1"), len(R.hypotheses(d["pdu"])), d["pdu"]["noise_var"] > 0) for d in items}
    assert {x[0] for x in dfh} == {1, 2, 3, 4, 6, 8} and {x[2] for x in dfh} == {1, 2, 4, 8} and {x[1] for x in dfh if not x[3]} >= set(range(1, 11))
    assert any(x[3] and x[1] == 0 for x in dfh)
    nvalid = sum(r["status"] == R.VALID for r in refs)
    print("VALID verdicts on noise alone: %d of %d" % (nvalid, len(refs)))
    assert nvalid <= 64


# (D, F, H, known noise)
DRAWS = [(1, 11, 1, False), (1, 10, 2, False), (2, 8, 4, False), (4, 4, 8, False), (8, 1, 4, False), (2, 4, 8, False), (1, 0, 1, True), (4, 6, 4, True),
         (8, 0, 8, True)]


@pytest.mark.parametrize("D,F,H,known", DRAWS)
def test_the_closed_form_thresholds_hold_the_false_alarm_rate(D, F, H, known):
    """200 000 direct draws of the statistic on noise alone: every shift energy is Gamma(D) in units of the noise energy of one shift and pair. The
    union bound is conservative, never optimistic: between half the target and 1.15 %."""
    rng = np.random.default_rng(1000 * D + 10 * F + H)
    thr = R.default_threshold(D, F, H, known)
    best = rng.gamma(D, size=(200000, H)).max(axis=1)
    metric = best / D if known else F * best / rng.gamma(F * D, size=200000)
    rate = float((metric >= thr).mean())
    print("D %d F %d H %d known %d: threshold %.4g, false-alarm rate %.4f" % (D, F, H, known, thr, rate))
    assert 0.5 * (R.P_FALSE_ALARM / H) * H <= rate <= 0.0115


def test_the_thresholds_of_the_issue():
    got = [R.default_threshold(*x, False) for x in ((1, 11, 1), (1, 10, 2), (2, 8, 4), (4, 4, 8), (8, 1, 4), (8, 8, 4), (1, 1, 1), (2, 4, 8))]
    assert np.allclose(got, [5.72, 6.99, 5.17, 4.35, 4.42, 2.49, 99.0, 7.60], rtol=2e-3), got


@pytest.mark.parametrize("name", G.DETERMINISTIC)
def test_no_decision_of_the_deterministic_sets_is_close(name):
    """Best and second-best hypothesis energies more than 1e-3 apart (relative), no metric within 1e-3 of its threshold."""
    refs = G.reference(name)
    close = [(i, r["gap"], r["edge"]) for i, r in enumerate(refs) if R.near(r)]
    assert not close, (name, close)


def test_at_most_one_percent_of_the_noise_set_is_close():
    refs = G.reference("noise")
    close = sum(R.near(r) for r in refs)
    print("noise-only PDUs near a tie or a threshold: %d of %d" % (close, len(refs)))
    assert close <= len(refs) // 100
