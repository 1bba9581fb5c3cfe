"""CPU: tests/golden/prach_detector.npz (recorded from the reference's PRACH detector and generator) against the numpy restatement
of tests/prach_ref.py and the tables the kernel compiles in (csrc/tables/nr_prach_tables.h).

Tolerances, from the project's own DFT bound: tests/test_ofdm_gpu.py bounds the device transform at 4e-6 rms and the reference's own
sits at about 1.1e-6 rms; the peak is at least the rms, so |c|^2 agrees between two float32 implementations within
2 (4e-6 + 1.1e-6) ~ 1e-5 relative, and the float32 product, preamble phase and summations add a few 1e-7 each: TOL_P = 2e-5 on the peak
power, TOL_M = 4e-5 on the metric (two more float32 sums in the divisor), 1e-5 on the RSSI. Here the reference's recorded values must
lie within them of the float64 restatement, so they cannot hide a defect the reference does not have."""
import os

import numpy as np
import pytest

import prach_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
FX = os.path.join(HERE, "golden", "prach_detector.npz")
TOL_P, TOL_M, TOL_RSSI = 2e-5, 4e-5, 1e-5
BAND_CAP = 0.005  # share of (occasion, preamble) pairs whose metric may sit within TOL_M of the threshold


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FX))


@pytest.fixture(scope="module")
def symbols(fx):
    return P.fixture_symbols(fx)


def in_band(metric):
    return np.abs(metric.astype(np.float64) - float(P.THRESHOLD)) <= TOL_M * float(P.THRESHOLD)


def test_fixture_coverage(fx):
    cfg = fx["cfg"]
    assert 240 <= len(cfg) <= 260
    assert set(cfg[:, P.C_FMT]) == set(range(14)) and set(cfg[:, P.C_ZCZ]) == set(range(16))
    short = cfg[cfg[:, P.C_FMT] >= 4]
    assert {(f, s) for f, s in short[:, [P.C_FMT, P.C_SCS]]} == {(f, s) for f in range(4, 14) for s in (0, 1)}
    # a preamble range that runs past the last logical root
    wraps = 0
    for c in cfg:
        d = P.derive(c[P.C_FMT], c[P.C_SCS], c[P.C_ZCZ])
        last = c[P.C_START] + c[P.C_NOF] - 1
        last_root = c[P.C_ROOT] + (last // (d["L"] // d["n_cs"]) if d["n_cs"] else last)
        wraps += c[P.C_NOF] > 0 and last_root >= d["L"] - 1
    assert wraps >= 5
    assert ((cfg[:, P.C_START] == 0) & (cfg[:, P.C_NOF] == 64)).sum() >= 100 and (cfg[:, P.C_NOF] == 0).sum() >= 5
    assert ((cfg[:, P.C_NOF] > 0) & (cfg[:, P.C_NOF] < 64)).sum() >= 30
    assert set(fx["tx_n"]) == set(range(5))
    assert ((fx["tx_n"] == 0) & (fx["noise"] == 0)).sum() >= 2, "all-zero symbols"
    assert ((fx["tx_n"] == 0) & (fx["noise"] > 0)).sum() >= 10, "noise only"
    assert ((fx["tx_n"] > 0) & (fx["noise"] == 0)).sum() >= 10, "noise-free"
    # two transmitted preambles on one root with different cyclic shifts
    shared = 0
    for c, k, idx in zip(cfg, fx["tx_n"], fx["tx_idx"]):
        rs = [P.root_and_shift(int(c[P.C_FMT]), int(c[P.C_ROOT]), int(c[P.C_ZCZ]), int(i), P.header_tables())[1:] for i in idx[:k]]
        shared += any(a[0] == b[0] and a[1] != b[1] for n, a in enumerate(rs) for b in rs[n + 1:])
    assert shared >= 20
    frac = np.abs(fx["tx_delay"] - np.round(fx["tx_delay"])) > 1e-9
    assert frac.any() and (fx["tx_delay"] < 0).any()
    # detections with a negative time advance, and peaks above the threshold that the delay window drops
    assert (fx["det_time_advance_tc"] < 0).sum() >= 5
    dropped = 0
    for i, c in enumerate(cfg):
        d = P.derive(c[P.C_FMT], c[P.C_SCS], c[P.C_ZCZ])
        lo, hi = fx["peak_offset"][i], fx["peak_offset"][i + 1]
        over = ~(fx["peak_metric"][lo:hi] < P.THRESHOLD)
        dropped += (over & (np.abs(P.delay_of(fx["peak_index"][lo:hi])) >= d["delay_n_maximum"])).sum()
    assert dropped >= 5
    assert in_band(fx["peak_metric"]).mean() <= BAND_CAP


def test_symbols_rebuild_bit_exact(fx, symbols):
    bad = [i for i, s in enumerate(symbols) if P.symbol_hash(s) != str(fx["sha256"][i])]
    assert not bad, "symbols of cases %s differ from the ones the reference saw" % bad[:10]


@pytest.mark.parametrize("which", ["header", "restated"])
def test_sequences_match_reference(fx, which):
    """The recorded generator output against the closed form with the tables of nr_prach_tables.h and with the ones computed here;
    the angle of each table entry rounded as in the reference's single-precision table (see prach_ref)."""
    t = P.header_tables() if which == "header" else P.restated_tables()
    for L, tag, fmt in ((839, "long", 0), (139, "short", 4)):
        pos, rec = fx["gen_positions_" + tag], fx["gen_roots_" + tag]
        assert rec.shape == (L - 1, 8)
        mine = np.stack([P.preamble(fmt, r, 0, 0, t, ref_table=True)[pos] for r in range(L - 1)])
        assert np.abs(mine - rec).max() < 1e-5
        full_cfg, full = fx["gen_full_%s_cfg" % tag], fx["gen_full_" + tag]
        assert full.shape == (8, L)
        for c, y in zip(full_cfg, full):
            _, _, cv = P.root_and_shift(int(c[0]), int(c[1]), int(c[2]), int(c[3]), t)
            assert cv != 0
            mine = P.preamble(int(c[0]), int(c[1]), int(c[2]), int(c[3]), t, ref_table=True)
            assert np.abs(mine - y).max() < 1e-5
            assert np.abs(np.abs(y) - np.sqrt(L)).max() < 1e-5
            # and the exact angles stay within the rounding of the reference's table: 4 L entries, angle error up to about 1e-6 rad
            assert np.abs(P.preamble(int(c[0]), int(c[1]), int(c[2]), int(c[3]), t) - y).max() < 5e-5


def test_header_tables_are_consistent():
    t, r = P.header_tables(), P.restated_tables()
    for L in (839, 139):
        assert sorted(t.order[L]) == list(range(1, L))
        assert (t.inv[L] == r.inv[L]).all() and (t.off[L] == r.off[L]).all()
        assert ((np.arange(1, L) * t.inv[L][1:]) % L == 1).all()
    assert (t.order[139] == P.short_root_order()).all()


def test_restatement_matches_recorded_replay(fx, symbols):
    t = P.header_tables()
    cfg = fx["cfg"]
    npairs = nband = 0
    for i, c in enumerate(cfg):
        d = P.derive(c[P.C_FMT], c[P.C_SCS], c[P.C_ZCZ])
        rssi = P.rssi(symbols[i])
        assert abs(fx["rssi"][i] - rssi) <= TOL_RSSI * rssi
        lo, hi = fx["peak_offset"][i], fx["peak_offset"][i + 1]
        assert hi - lo == c[P.C_NOF]
        det = set(fx["det_index"][fx["det_offset"][i]:fx["det_offset"][i + 1]])
        if not rssi > 0:
            assert not det and not fx["peak_power"][lo:hi].any()
            continue
        assert abs(fx["rssi_db"][i] - 10 * np.log10(rssi)) < 1e-4
        if hi == lo:
            assert not det
            continue
        pw = P.correlation_power(symbols[i], c, t)
        peak = pw.max(axis=1)
        ref_idx, ref_pow, ref_met = fx["peak_index"][lo:hi], fx["peak_power"][lo:hi].astype(np.float64), fx["peak_metric"][lo:hi]
        assert (pw[np.arange(hi - lo), ref_idx] >= (1 - 2 * TOL_P) * peak).all(), "case %d: the reference's peak bin" % i
        assert (np.abs(ref_pow - peak) <= TOL_P * peak).all(), "case %d: peak power" % i
        metric = peak / (rssi * d["L"] ** 3)
        assert (np.abs(ref_met - metric) <= TOL_M * metric).all(), "case %d: metric" % i
        mine = ~(metric < float(P.THRESHOLD)) & (np.abs(P.delay_of(pw.argmax(axis=1))) < d["delay_n_maximum"])
        ref = np.array([c[P.C_START] + k in det for k in range(hi - lo)])
        band = in_band(ref_met)
        assert (mine == ref)[~band].all(), "case %d: detected" % i
        npairs += hi - lo
        nband += band.sum()
    assert nband <= BAND_CAP * npairs


def test_time_units(fx):
    """time_resolution, time_advance_max and every detection's time advance in T_c units from delay_n (phy_time_unit::from_seconds)."""
    for i, c in enumerate(fx["cfg"]):
        d = P.derive(c[P.C_FMT], c[P.C_SCS], c[P.C_ZCZ])
        assert fx["time_resolution_tc"][i] == d["time_resolution_tc"]
        assert fx["time_advance_max_tc"][i] == d["time_advance_max_tc"]
        lo = fx["peak_offset"][i]
        for k in range(fx["det_offset"][i], fx["det_offset"][i + 1]):
            rec = lo + fx["det_index"][k] - c[P.C_START]
            delay = int(P.delay_of(fx["peak_index"][rec]))
            assert fx["det_time_advance_tc"][k] == P.time_advance_tc(delay, d["fs"])
            assert abs(fx["det_power_db"][k] - 10 * np.log10(fx["peak_power"][rec])) < 1e-4


def test_binding_layout_matches_header(tmp_path):
    """Every field offset of the PRACH dtypes against include/miphy.h, compiled with gcc."""
    import subprocess

    import miphy
    fields = [("miphy_prach_job", miphy.PrachJob), ("miphy_prach_result", miphy.PrachResult),
              ("miphy_prach_preamble_result", miphy.PrachPreambleResult), ("miphy_prach_gen_job", miphy.PrachGenJob)]
    body = "".join('  printf("%%zu\\n", sizeof(%s));\n' % t + "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (t, f) for f in dt.names)
                   for t, dt in fields)
    src = tmp_path / "l.c"
    src.write_text('#include "miphy.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-I", os.path.join(HERE, "..", "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, dt in fields:
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert got == want
