"""CPU: the crafted demapper inputs of tests/demod_edges.py -- what the generator guarantees, that the edges really arrive at the demapper through
the equaliser, and the oracle's demapper against the reference's on them (tests/golden/demod_edges.npz, recorded by oracle/gen_golden.py from both
code paths of the reference)."""
import os

import numpy as np
import pytest

import demod_edges as DE
import oracle_lib as O

GOLD = os.path.join(os.path.dirname(__file__), "golden", "demod_edges.npz")
F = np.float32


def _class_counts(mod):
    el, names = DE.elements(mod)
    cnt = np.bincount(np.concatenate([el["cre"], el["cim"]]), minlength=len(names))
    return el, {n: int(c) for n, c in zip(names, cnt)}


@pytest.mark.parametrize("mod", DE.MODS)
def test_class_census(mod):
    """Floors per class: a tie at an even and at an odd n for every (soft-bit function, sign); the clip targets 119.5, 120 and 120.5 of either sign
    for every function that reaches them (the floats next to 120: exactly, or the nearest value on that side that +-64 ulps of x reach); every
    interior boundary of every interval grid five times; the threshold, zero, tiny, beyond, non-finite and noise classes."""
    el, cnt = _class_counts(mod)
    for fn in DE.FUNCS[mod]:
        for sign in "+-":
            for par in ("even", "odd"):
                assert cnt.get("tie:%s:%s:%s" % (fn, sign, par), 0) >= 1, (fn, sign, par)
            reach_plus = not (mod >= 6 and fn != "B0")  # the inner tables are bounded above: checked below where they still reach the clip
            for t in ("119.5", "120", "120.5")[:2 if mod == 1 else 3]:
                if sign == "-" or reach_plus:
                    assert cnt.get("clip:%s:%s%s" % (fn, sign, t), 0) >= 1, (fn, sign, t)
            for t in ("119.999992", "120.000008", "120.5"):
                assert cnt.get("clip:%s:%s%s" % (fn, sign, t), 0) + cnt.get("clip:%s:%snear%s" % (fn, sign, t), 0) >= 1, (fn, sign, t)
    assert any(n.startswith("clip") and n.endswith("1000000") and c for n, c in cnt.items())
    for name, count in DE.GRIDS.get(mod, ()):
        for k in range(-(count // 2 - 1), count // 2):
            if k:
                assert cnt["boundary:%s:%d" % (name, k)] >= 10, (name, k)  # five values, each once in re and once in im
        assert cnt["beyond:%s" % name] >= 2
    if mod == 4:
        assert cnt["threshold"] >= 10
    assert cnt["zero"] >= 5 and cnt["tiny"] >= 6 and cnt["beyond"] >= 4
    for name, _, _, _ in DE.NOISE_CLASSES:
        assert cnt[name] == 2 * len(DE.NOISE_SYMBOLS)
    # non-finite: each of +-Inf, NaN in re only, in im only, in both; +-FLT_MAX
    for v in DE.NONFINITE:
        same = (lambda a: np.isnan(a)) if np.isnan(v) else (lambda a: a == v)
        assert np.any(same(el["re"]) & np.isfinite(el["im"])) and np.any(np.isfinite(el["re"]) & same(el["im"])) and np.any(same(el["re"]) & same(el["im"]))
    assert np.any(el["re"] == DE.FLT_MAX) and np.any(el["im"] == -DE.FLT_MAX)
    # the ties are ties: recomputed here from the element, its variance and its class
    names = list(cnt)
    ties = 0
    for part, cls in (("re", "cre"), ("im", "cim")):
        for e in el:
            n = names[e[cls]]
            if n.startswith("tie:") and np.isfinite(e["re"]) and np.isfinite(e["im"]):
                s = float(DE.scaled(mod, n.split(":")[1], e[part], DE.nv_of(e["base"], e["k"])))
                assert s - np.floor(s) == 0.5 and (s > 0) == (n.split(":")[2] == "+") and (int(np.floor(abs(s))) & 1) == (n.split(":")[3] == "odd"), (n, s)
                ties += 1
    assert ties >= 4 * len(DE.FUNCS[mod])


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("mod", DE.MODS)
def test_crafted_equals_delivered(mod, compact):
    """The guard that the edges arrive: for every finite crafted element on a normal power-of-two estimate the oracle's own equalised symbol and
    variance (the eq and nv results of o_pusch_demodulate) are the crafted ones bit for bit. One exception, stated in demod_edges: a -0 component
    arrives as +0."""
    checked = 0
    for base, el in DE.bases(mod, with_noise_classes=not compact):
        lay = DE.lay(mod, el, base, compact, ports=2 if compact else 1)
        _, eq, nv = O.o_pusch_demodulate(*lay["args"])
        assert eq.size == lay["n_re"] and np.all(lay["slot"] >= 0) and np.unique(lay["slot"]).size == el.size
        ok = DE.delivered_exactly(el)
        s = lay["slot"][ok]
        for got, want in ((eq.real[s], el["re"][ok]), (eq.imag[s], el["im"][ok])):
            assert np.array_equal(got.view(np.uint32), (want + F(0)).view(np.uint32))  # (+ 0: -0 -> +0, every other value unchanged)
        want_nv = np.array([DE.nv_of(b, k) for b, k in zip(el["base"][ok], el["k"][ok])], F)
        assert np.array_equal(nv[s].view(np.uint32), want_nv.view(np.uint32))
        checked += int(ok.sum())
    el_all, _ = DE.elements(mod)
    assert checked == int((DE.delivered_exactly(el_all) & ~(compact & DE.is_noise_class(el_all))).sum()) and checked > 50


@pytest.mark.parametrize("mod", DE.MODS)
def test_oracle_matches_reference_fixture(mod):
    """The oracle's demapper within one step of the reference's on every crafted element, against both recorded code paths of the reference: the
    whole set in one call (a multiple of 32 symbols: its vector body) and slices of 7 symbols, a call each (its scalar code). Left out: the one class
    demod_edges.reference_comparable names (positive variances below 2^-100).
    Measured exact-match share of the compared LLRs, vector body / scalar code: modulation order 1: 1.0000 / 1.0000, 2: 1.0000 / 0.9746,
    4: 1.0000 / 0.9662, 6: 0.9888 / 0.9722, 8: 0.9877 / 0.9809 (the scalar code divides by the variance and by the interval width where the vector
    body and the oracle multiply by reciprocals; ties and boundaries are where that shows). No element is beyond one step on either path."""
    d = np.load(GOLD)
    sym, nv = d["sym_%d" % mod], d["nv_%d" % mod]
    want_sym, want_nv = DE.fixture_inputs(mod)  # the fixture is the generator's set of today
    assert np.array_equal(sym.view(np.uint32), want_sym.view(np.uint32)) and np.array_equal(nv.view(np.uint32), want_nv.view(np.uint32))
    assert sym.size % 32 == 0 and DE.reference_comparable(nv, mod).mean() > 0.8
    vec = O.o_demodulate_soft(mod, sym, nv)
    sc = np.concatenate([O.o_demodulate_soft(mod, sym[i:i + 7], nv[i:i + 7]) for i in range(0, sym.size, 7)])
    for name, o, r in (("vector body", vec, d["llr_vec_%d" % mod]), ("scalar code", sc, d["llr_sc_%d" % mod])):
        worst, exact = DE.compare_with_reference(mod, nv, o, r)
        print("modulation order %d, %s: max |oracle - reference| = %d, exact share %.4f" % (mod, name, worst, exact))
        assert worst <= 1, (name, worst)
