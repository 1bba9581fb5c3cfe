"""CPU: the numpy SRS transmitter (tests/srs_tx.py) against the float64 receiver (tests/srs_ref.py), which restates the arithmetic of csrc/srs.hip, and
the cases of tests/srs_cases.py that the GPU tests run. No device. What is shown here is that the arithmetic itself is right: it recovers the channel,
the delay and the noise level it is given, and UEs multiplexed by comb offset or cyclic shift do not reach each other's estimates."""
import itertools

import numpy as np
import pytest

import miphy
import srs_cases as G
import srs_ref as R
import srs_tx as X


def smallest_prg(K, P):
    return next(prg for prg in (1, 2, 4) if (12 * prg // K) % P == 0)


def classes():
    """Every (K, N_ap, n_cs): M = 48 at comb 2 (8 PRB) and 36 at comb 4 (12 PRB), the smallest PRG the rule allows."""
    for K, nap in itertools.product((2, 4), (1, 2, 4)):
        for ncs in range(8 if K == 2 else 12):
            p = X.ue(R=2, nap=nap, start=10, nsym=2, K=K, kbar=K - 1, ncs=ncs, nid=17 * ncs + nap, prg=1, prb=1, nprb=8 if K == 2 else 12, slot=5, numerology=1)
            p["prg"] = smallest_prg(K, X.derive(p)["P"])
            yield p


def test_a_flat_channel_per_prg_without_delay_is_recovered_exactly():
    seen = set()
    for n, p in enumerate(classes()):
        d = X.derive(p)
        seen.add((p["K"], p["nap"], len(d["combs"])))
        Hg = X.prg_channel(np.random.default_rng(n), p)
        ref = R.receive(p, X.build_grid(0, p["R"], p["grid_nprb"], 0.0, [(p, Hg, 0.0)], dtype=np.complex128))
        assert np.abs(ref["H"] - Hg).max() <= 1e-12, (p, np.abs(ref["H"] - Hg).max())
        assert np.abs(ref["h_wb"][:p["R"], :p["nap"]] - Hg.mean(axis=0)).max() <= 1e-12
        assert abs(ref["phi"]) <= 1e-12 and ref["noise_var"] <= 1e-24
        assert np.abs(ref["rsrp"] - (np.abs(Hg) ** 2).mean(axis=(0, 1))).max() <= 1e-12
    assert seen == {(2, 1, 1), (2, 2, 1), (2, 4, 1), (2, 4, 2), (4, 1, 1), (4, 2, 1), (4, 4, 1), (4, 4, 2)}


@pytest.mark.parametrize("frac", [0.25, -0.25, 0.75, -0.75])
def test_delays_within_the_reported_range_are_recovered(frac):
    for n, p in enumerate(classes()):
        if p["ncs"] % 5:
            continue  # cyclic shifts 0, 5 and 10: every class once or twice
        tau = frac * R.max_delay(p)
        assert abs(float(miphy.srs_info(X.job_of(p))["max_delay_s"]) - R.max_delay(p)) <= 1e-6 * R.max_delay(p)
        Hg, theta = X.prg_channel(np.random.default_rng(n), p), X.theta_of_delay(p, tau)
        ref = R.receive(p, X.build_grid(0, p["R"], p["grid_nprb"], 0.0, [(p, Hg, theta)], dtype=np.complex128))
        assert abs(ref["time_alignment_s"] - tau) <= 1e-9 * abs(tau), (p, ref["time_alignment_s"], tau)
        assert abs(abs(ref["phi"]) - abs(frac) * np.pi) <= 1e-9
        want = X.centre_channel(p, Hg, theta)
        assert np.abs(ref["H"] - want).max() <= 1e-9 * np.abs(want).max(), (p, np.abs(ref["H"] - want).max())
        assert ref["noise_var"] <= 1e-18


def test_ues_on_the_two_offsets_of_comb_2_do_not_disturb_each_other():
    kw = dict(R=2, start=12, nsym=2, K=2, prg=2, prb=0, nprb=8, slot=1, numerology=1)
    a, b = X.ue(nap=2, kbar=0, ncs=3, nid=10, **kw), X.ue(nap=4, kbar=1, ncs=1, nid=11, **kw)
    rng = np.random.default_rng(3)
    Ha, Hb = X.prg_channel(rng, a), X.prg_channel(rng, b)
    for gain in (0.0, 1.0, 30.0):  # the other UE absent, alike, and 30 dB stronger
        grid = X.build_grid(0, 2, 8, 0.0, [(a, Ha, 0.0), (b, gain * Hb, 0.0)], dtype=np.complex128)
        assert np.abs(R.receive(a, grid)["H"] - Ha).max() <= 1e-12
        if gain:
            assert np.abs(R.receive(b, grid)["H"] - gain * Hb).max() <= 1e-12 * gain


def test_ues_on_one_comb_half_the_cyclic_shifts_apart_do_not_disturb_each_other():
    """Two one-port UEs n_cs_max / 2 apart are the two ports of a two-port job (P = 2): each job's port 0 is its own UE, whatever the other sends."""
    for K in (2, 4):
        nmax = 8 if K == 2 else 12
        kw = dict(R=2, nap=1, start=13, nsym=1, K=K, kbar=1, nid=99, prg=2, prb=2, nprb=12, slot=0, numerology=0, grid_nprb=14)
        a, b = X.ue(ncs=1, **kw), X.ue(ncs=1 + nmax // 2, **kw)
        rng = np.random.default_rng(K)
        Ha, Hb = X.prg_channel(rng, a), X.prg_channel(rng, b)
        for gain in (0.0, 1.0, 30.0):
            grid = X.build_grid(0, 2, 14, 0.0, [(a, Ha, 0.0), (b, gain * Hb, 0.0)], dtype=np.complex128)
            ra, rb = R.receive(dict(a, nap=2), grid), R.receive(dict(b, nap=2), grid)
            assert np.abs(ra["H"][:, :, 0] - Ha[:, :, 0]).max() <= 1e-12 and np.abs(ra["H"][:, :, 1] - gain * Hb[:, :, 0]).max() <= 1e-12 * max(gain, 1)
            assert np.abs(rb["H"][:, :, 0] - gain * Hb[:, :, 0]).max() <= 1e-12 * max(gain, 1) and np.abs(rb["H"][:, :, 1] - Ha[:, :, 0]).max() <= 1e-12
            assert ra["noise_var"] <= 1e-20 and abs(ra["phi"]) <= 1e-12


def test_the_noise_variance_is_unbiased():
    """2000 draws at 10 dB: the mean of noise_var within 3 standard errors of sigma^2. The delay is estimated from the noisy draw like everything
    else; its error leaves a residual of the order sigma^4 Q^2 / (|h|^2 P^2 R L M), three orders below sigma^2 here (Q = 3, M = 48)."""
    p = X.ue(R=2, nap=1, start=12, nsym=2, K=4, kbar=1, ncs=4, nid=3, prg=1, prb=0, nprb=16, slot=0, numerology=1)
    rng = np.random.default_rng(11)
    Hg = np.ones((16, 2, 1), np.complex128) * np.exp(1j * np.array([0.3, -1.1]))[None, :, None]  # |h| = 1 on every PRG and port
    clean = X.build_grid(0, 2, 16, 0.0, [(p, Hg, 0.0)], dtype=np.complex128)
    sigma2 = 0.1
    draws = np.empty(2000)
    for k in range(draws.size):
        noise = np.sqrt(sigma2 / 2) * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape))
        draws[k] = R.receive(p, clean + noise)["noise_var"]
    se = draws.std(ddof=1) / np.sqrt(draws.size)
    print("mean noise_var %.6f, sigma^2 %.6f, standard error %.2e" % (draws.mean(), sigma2, se))
    assert abs(draws.mean() - sigma2) <= 3 * se


def test_the_base_sequences_equal_the_library_host_function():
    worst = 0.0
    for nprb, K, hopping, nid in ((4, 4, 0, 7), (12, 4, 0, 29), (8, 2, 1, 512), (12, 2, 2, 5), (24, 4, 2, 1000), (268, 2, 2, 31), (180, 4, 1, 640)):
        p = X.ue(nap=1, start=2, nsym=4, K=K, ncs=0, nid=nid, hopping=hopping, prg=4, prb=0, nprb=nprb, slot=19, numerology=1)
        M = X.derive(p)["M"]
        for l in range(4):
            u, v = X.uv(p, 2 + l)
            worst = max(worst, np.abs(X.port_sequence(p, l, 0) - miphy.low_papr_sequence(u, v, M)).max())
    assert worst <= 2e-7, worst
    # M = 1632 is beyond that function (its limit of 1620 stays); the sequence is still Zadoff-Chu of N_ZC = 1627, of unit modulus
    with pytest.raises(Exception, match="invalid length"):
        miphy.low_papr_sequence(0, 0, 1632)
    p = X.ue(nap=1, K=2, nprb=272, nid=9)
    s = X.port_sequence(p, 0, 0)
    assert s.size == 1632 and np.abs(np.abs(s) - 1).max() <= 1e-12 and np.abs(s[1627:] - s[:5]).max() <= 1e-9


def test_the_cases_of_the_gpu_tests():
    """Every case keeps |phi| <= 2.5 rad, the float64 receiver finds what was sent, and the set covers what its docstring says."""
    items = G.shapes_set()
    cover = dict(M=set(), nap=set(), L=set(), R=set(), prg=set(), hop=set(), slot=set(), split=set(), v=set(), high=set())
    for it in items + G.multiplexed_set():
        p, ref, d = it["p"], it["ref"], X.derive(it["p"])
        assert abs(ref["phi"]) <= 2.5, (p, ref["phi"])
        assert int(miphy.srs_info(X.job_of(p))["nof_h"]) == ref["H"].size
    for it in items:
        p, ref, d = it["p"], it["ref"], X.derive(it["p"])
        for k, v in (("M", d["M"]), ("nap", p["nap"]), ("L", p["nsym"]), ("R", p["R"]), ("prg", p["prg"]), ("hop", p["hopping"]), ("slot", p["slot"]),
                     ("split", (p["K"], len(d["combs"]))), ("high", (p["nap"], p["ncs"] >= d["ncs_max"] // 2))):
            cover[k].add(v)
        cover["v"] |= {(d["M"] >= 72, X.uv(p, p["start"] + l)[1]) for l in range(p["nsym"])}
        want = X.centre_channel(p, it["Hg"], it["theta"])
        tol = 1e-5 if it["snr_db"] is None else 6 * 10 ** (-it["snr_db"] / 20)  # complex64 grid; with noise, far inside six sigma of one element
        assert np.abs(ref["H"] - want).max() <= tol * np.abs(want).max() + tol, (p, np.abs(ref["H"] - want).max())
        tau = it["frac"] * R.max_delay(p)
        assert abs(ref["time_alignment_s"] - tau) <= (1e-5 if it["snr_db"] is None else 0.05) * R.max_delay(p)
        if it["snr_db"] is None:
            assert ref["noise_var"] <= 1e-12 * ref["epre"]
        elif ref["H"].size * 8 <= d["M"] * p["nsym"] * p["R"]:  # enough residuals per estimate for a tight figure
            assert abs(ref["noise_var"] / 10 ** (-it["snr_db"] / 10) - 1) <= 0.2
    assert cover["M"] == {12, 36, 48, 72, 1632} and cover["nap"] == {1, 2, 4} and cover["L"] == {1, 2, 4} and cover["R"] == {1, 4}
    assert cover["prg"] == {1, 2, 4} and cover["hop"] == {0, 1, 2} and {0, 19} <= cover["slot"]
    assert cover["split"] == {(2, 1), (2, 2), (4, 1), (4, 2)} and {(n, h) for n in (1, 2, 4) for h in (False, True)} <= cover["high"]
    assert {(True, 0), (True, 1), (False, 0)} == cover["v"]
