"""GPU: the packed LDPC decoder whose wavefronts leave out the visits of a layer once every soft bit their rows WRITE there is infinite
(csrc/ldpc_pk_device.h, update_rows_pk<..., DETECT>; DESIGN.md section 4, "saturated rows") against the CPU oracle chain, four ways
each -- skip on / off, soft-bit addresses from the table / computed (check_four_ways, tests/test_ldpc_saturated_rows_gpu.py): hard bits,
codeblock CRC flags, iteration counts, result records, transport blocks and HARQ soft images.
Every case asserts with the per-visit model (tests/ldpc_visit_model.py) what it is there for: that the output rule leaves out more visits
than the input rule did. z128 is one full wavefront, z352 has a partial last wavefront (H = 176), z384 is three codeblocks.
  clean: received at sigma 0.10;
  noisy: sigma 0.40 / 0.35, every codeblock still decodes: rows saturate late, one after another;
  full-magnitude flips: the codeword at +-120 without noise, wrong signs in columns 22 and 23 of codeblock 0 (FLIPS,
    tests/test_ldpc_output_saturation.py): every row has min + scaled min >= 121 and the rows on a flipped bit have odd parity -- a kernel
    that forgets the parity freezes them at their first visit and returns the wrong word (the CPU test shows that the model then does).
What these cannot see is a wrong freeze of rows whose checks hold (a threshold of 120, say): it leaves the hard bits alone. The CPU test
pins the formula for that."""
import numpy as np
import pytest

from ldpc_visit_model import visits_left_out, visits_of
from test_ldpc_output_saturation import FLIPS, SEED
from test_ldpc_saturated_rows import SHAPES, codeblock_inputs
from test_ldpc_saturated_rows_gpu import check_four_ways

pytestmark = pytest.mark.gpu


def left_out_by_rule(t, max_iter):
    """Per codeblock (visits left out under the input rule, under the output rule), summed over its wavefronts."""
    Z, lay = SHAPES[t[0]][2], SHAPES[t[0]][4]
    out = []
    for image, _, _, _ in codeblock_inputs(*t):
        a, b = (visits_left_out(Z, image, lay, max_iter, rule) for rule in ("input", "output"))
        assert (a <= b).all() and (b <= visits_of(lay, max_iter)).all()
        out.append((int(a.sum()), int(b.sum())))
    return out


@pytest.mark.parametrize("max_iter", [6, 8])
@pytest.mark.parametrize("shape", ["z128", "z352", "z384"])
def test_clean(ctx, shape, max_iter):
    """(z128 with 6 iterations: 6 -> 9 visits left out; z384 with 8: 32-33 -> 40 per codeblock.)"""
    t = (shape, 0.10, SEED, -1)
    per_cb = left_out_by_rule(t, max_iter)
    print(shape, max_iter, "visits left out per codeblock (input rule, output rule):", per_cb)
    assert all(b > a for a, b in per_cb), per_cb
    got, _ = check_four_ways(ctx, (t,), max_iter, False, True)
    assert got[0][0]["tb_crc_ok"] and got[0][2].all()
    assert (int(got[0][0]["iters_min"]), int(got[0][0]["iters_max"])) == (max_iter, max_iter)


@pytest.mark.parametrize("shape,sigma", [("z128", 0.40), ("z384", 0.35)])
def test_noisy(ctx, shape, sigma):
    """(Visits left out: z128 2 -> 5, z384 3-4 -> 7-11 per codeblock.)"""
    t = (shape, sigma, SEED, -1)
    per_cb = left_out_by_rule(t, 8)
    print(shape, sigma, "visits left out per codeblock (input rule, output rule):", per_cb)
    assert all(b > a for a, b in per_cb), per_cb
    got, _ = check_four_ways(ctx, (t,), 8, False, True)
    assert got[0][0]["tb_crc_ok"] and got[0][2].all()


@pytest.mark.parametrize("shape", ["z128", "z384"])
def test_full_magnitude_flips(ctx, shape):
    t = (shape, None, SEED, FLIPS[shape])
    Z, lay = SHAPES[shape][2], SHAPES[shape][4]
    image = codeblock_inputs(*t)[0][0]
    # a rule without the parity term would freeze more than the rule does: the rows on a flipped bit are what the case is about
    right, wrong = (int(visits_left_out(Z, image, lay, 6, rule).sum()) for rule in ("output", "no_parity"))
    print(shape, "visits left out in codeblock 0 (output rule, without the parity term):", right, wrong)
    assert wrong > right
    check_four_ways(ctx, (t,), 6, False, True)
