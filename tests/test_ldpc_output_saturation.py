"""Saturated rows detected from what a visit WRITES (csrc/ldpc_pk_device.h, update_rows_pk<..., DETECT>), on the CPU:
the per-visit model of tests/ldpc_visit_model.py against the oracle, the closed form of "every written soft bit is infinite" against the
written values, and simulated decodes that leave visits out under the rule against the oracle's hard bits -- with a rule that forgets the
parity term as the counter-example that must fail.
Inputs: SHAPES, transport_block and codeblock_inputs of tests/test_ldpc_saturated_rows.py; the flip cases are codewords received at
+-120 without noise with wrong-sign bits in columns 22 and 23 of codeblock 0 (parity columns with several checks each, behind the
fillers): every row has min + scaled min >= 121, and the rows on a flipped bit have odd parity."""
import functools
import itertools

import numpy as np
import pytest

from oracle_lib import o_ldpc_decode
from ldpc_visit_model import LLR_MAX, Visit, decode, layers_decoded, scaled, visits_left_out, visits_of
from test_ldpc_saturated_rows import BG, CASES, SHAPES, SIGMA, codeblock_inputs

SEED = 100
NOISE = [("z128", 0.10), ("z352", 0.10), ("z384", 0.10), ("z128", 0.35), ("z352", 0.35), ("z384", 0.35)]
FLIPS = {
    "z128": tuple(22 * 128 + r for r in range(0, 128, 9)) + tuple(23 * 128 + r for r in range(3, 128, 13)),
    "z384": tuple(22 * 384 + r for r in range(0, 384, 7)) + tuple(23 * 384 + r for r in range(3, 384, 11)),
}
FLIP_CASES = [("z128", None, FLIPS["z128"], 6), ("z384", None, FLIPS["z384"], 6)]


@functools.lru_cache(maxsize=None)
def traced(shape, sigma, flip_cb, max_iter):
    """Per codeblock of a decode that runs every visit: (soft bits behind every iteration, [(iteration, layer, rows, Visit)])."""
    Z, lay = SHAPES[shape][2], SHAPES[shape][4]
    out = []
    for image, _, _, _ in codeblock_inputs(shape, sigma, SEED, flip_cb):
        assert layers_decoded(Z, image) == lay
        snaps, visits = [], []
        decode(Z, image, lay, max_iter, None, lambda it, m, rows, v: visits.append((it, m, rows, v)), lambda it, soft: snaps.append(soft))
        out.append((snaps, visits))
    return out


def all_visits():
    for shape, sigma in NOISE:
        for _, visits in traced(shape, sigma, -1, 8):
            yield from visits
    for shape, sigma, flips, k in FLIP_CASES:
        yield from traced(shape, sigma, flips, k)[0][1]


@pytest.mark.parametrize("shape,sigma", NOISE)
def test_model_equals_the_oracle_at_every_iteration_boundary(shape, sigma):
    Z = SHAPES[shape][2]
    for (image, nf, _, _), (snaps, _) in zip(codeblock_inputs(shape, sigma, SEED, -1), traced(shape, sigma, -1, 8)):
        for k in range(1, 9):
            _, hard, soft = o_ldpc_decode(BG, Z, image, nf, -1, k, want_soft=True)
            assert np.array_equal(snaps[k - 1], soft), (shape, sigma, k, int(np.sum(snaps[k - 1] != soft)))
            assert np.array_equal(np.packbits(snaps[k - 1][:22 * Z] <= 0), hard)


def agree(v, what):
    written, closed, device = v.writes_infinite(), v.closed_form(), v.device_form()
    assert np.array_equal(closed, written), (what, int(np.sum(closed != written)))
    assert np.array_equal(device, written), (what, int(np.sum(device != written)))
    return written


def test_closed_form_on_every_row_of_every_visit():
    seen = {(False, False): 0, (True, False): 0, (True, True): 0}  # (written infinite, read infinite)
    for it, m, _, v in all_visits():
        written, read = agree(v, (it, m)), v.reads_infinite()
        assert not (read & ~written).any()  # a row that reads only infinite soft bits writes only infinite ones
        for key in seen:
            seen[key] += int(np.sum((written == key[0]) & (read == key[1])))
    assert min(seen.values()) > 1000, seen  # live rows, rows the output rule catches a visit early, frozen rows


def test_closed_form_on_a_grid_of_degree_three_rows():
    mags = [0, 1, 53, 54, 66, 67, 68, 96, 119, 120, 121, 126, 127]
    softs = sorted({s * m for m in mags for s in (1, -1)})
    msgs = [0, 1, -1, 96, -96]
    soft = np.array(list(itertools.product(softs, repeat=3)), np.int8)
    hit = 0
    for c in itertools.product(msgs, repeat=3):
        hit += int(agree(Visit(soft, np.array(c, np.int32)[None, :], False), c).sum())
    hit += int(agree(Visit(soft, None, True), "first visit").sum())
    assert 0 < hit < soft.shape[0] * (len(msgs) ** 3 + 1)
    # the boundary: 67 + scaled(67) = 120 stays finite, 68 + scaled(68) = 122 does not; odd parity never passes with a finite input
    assert (scaled(67), scaled(68), scaled(LLR_MAX)) == (53, 54, 95)
    for mag, sign, want in ((67, 1, False), (68, 1, True), (68, -1, False), (120, -1, False), (127, -1, True)):
        v = Visit(np.array([[mag, mag, sign * mag]], np.int8), None, True)
        assert bool(v.closed_form()[0]) == bool(v.device_form()[0]) == bool(v.writes_infinite()[0]) == want, (mag, sign)


def test_closed_form_on_random_rows_of_degree_nineteen():
    rng = np.random.default_rng(5)
    n, hit = 20000, 0
    for lo, p_inf in ((0, 0.0), (60, 0.3), (100, 0.9), (60, 1.0)):  # magnitudes from lo to 120, a share of them infinite
        s = rng.integers(lo, LLR_MAX + 1, (n, 19)) * rng.choice([-1, 1], (n, 19))
        s = np.where(rng.random((n, 19)) < p_inf, 127 * np.sign(s + 0.5), s).astype(np.int8)
        c = rng.integers(-96, 97, (n, 19)).astype(np.int32)
        for first in (False, True):
            w = agree(Visit(s, c, first), (lo, p_inf, first))
            hit += int(w.sum())
            assert 0 < w.sum() < n or p_inf in (0.0, 1.0) or lo == 0
    assert hit > n


def test_a_row_that_wrote_infinite_values_reads_infinite_values_at_its_next_visit():
    seen = 0
    cases = [traced(shape, sigma, -1, 8) for shape, sigma in NOISE] + [traced(shape, sigma, flips, k)[:1] for shape, sigma, flips, k in FLIP_CASES]
    for per_cb in cases:
        for _, visits in per_cb:
            wrote = {}
            for it, m, rows, v in visits:
                before = wrote.get((m, int(rows[0])))  # the same rows' visit of this layer one iteration earlier
                if before is not None:
                    assert v.reads_infinite()[before].all(), (it, m)
                    seen += int(before.sum())
                wrote[(m, int(rows[0]))] = v.writes_infinite()
    assert seen > 1000


def oracle_hard(shape, sigma, flip_cb, max_iter):
    Z = SHAPES[shape][2]
    return [o_ldpc_decode(BG, Z, image, nf, -1, max_iter)[1] for image, nf, _, _ in codeblock_inputs(shape, sigma, SEED, flip_cb)]


@pytest.mark.parametrize("shape,sigma,flip_cb,max_iter", [(s, SIGMA, f, 8) for s, f in CASES] + FLIP_CASES)
def test_skipping_under_the_rule_gives_the_oracle_hard_bits(shape, sigma, flip_cb, max_iter):
    Z, lay = SHAPES[shape][2], SHAPES[shape][4]
    for (image, _, _, _), want in zip(codeblock_inputs(shape, sigma, SEED, flip_cb), oracle_hard(shape, sigma, flip_cb, max_iter)):
        ran = {}
        for rule in ("input", "output", "device"):
            hard, ran[rule] = decode(Z, image, lay, max_iter, rule)
            assert np.array_equal(hard, want), (shape, rule)
        assert np.array_equal(ran["output"], ran["device"]) and (ran["output"] <= ran["input"]).all() and (ran["input"] <= visits_of(lay, max_iter)).all()


@pytest.mark.parametrize("shape,sigma,flip_cb,max_iter", FLIP_CASES)
def test_a_rule_without_the_parity_term_gives_wrong_hard_bits(shape, sigma, flip_cb, max_iter):
    """(62 wrong bits at z128, 142 at z384.)"""
    Z, lay = SHAPES[shape][2], SHAPES[shape][4]
    image = codeblock_inputs(shape, sigma, SEED, flip_cb)[0][0]
    want = oracle_hard(shape, sigma, flip_cb, max_iter)[0]
    hard, ran = decode(Z, image, lay, max_iter, "no_parity")
    wrong = int(np.unpackbits(hard ^ want).sum())
    print(shape, "wrong hard bits without the parity term:", wrong, "visits run", ran.tolist())
    assert wrong > 0
    # the right rule keeps a wavefront with rows on a flipped bit alive: it leaves out fewer visits than the wrong one
    out = {rule: int(visits_left_out(Z, image, lay, max_iter, rule).sum()) for rule in ("input", "output", "no_parity")}
    assert out["input"] <= out["output"] < out["no_parity"], out
