"""Saturated rows of the LDPC decoder against the CPU oracle (no GPU): the packed kernel leaves out the layer visits of a wavefront whose
rows read infinite soft bits only (csrc/ldpc_decode_pk.hip, "saturated rows"; the argument is DESIGN.md section 4). What that rests on
is checked here on the oracle's soft bits after k and k + 1 iterations (o_ldpc_decode, want_soft):
  - a soft bit that is +-127 after k iterations is +-127 with the same sign after k + 1;
  - once every soft bit of the columns a codeblock reaches is +-127, hard bits and CRC verdict are the same for every larger k.
Inputs are first transmissions as the demapper and the dematcher leave them: LLRs within +-120, fillers at +127, 256QAM, BG1, at the
shapes of tests/test_ldpc_address_table_gpu.py. The helpers below also serve tests/test_ldpc_saturated_rows_gpu.py and
tools/ldpc_saturation_profile.py."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import OraclePuschDecoder, o_ldpc_decode, o_pdsch_encode, o_segmentation
from ldpc_saturation_model import dead_below_live, infinite, left_out, saturated_from

BG, MOD = 1, 8
# name: TB bits, channel symbols, lifting size, codeblocks, layers reached
SHAPES = {
    "z384": (25224, 3420, 384, 3, 4),
    "z352": (15416, 2112, 352, 2, 4),
    "z128": (2800, 384, 128, 1, 4),
    "z256": (5608, 768, 256, 1, 4),
    "z384_six_layers": (25248, 3744, 384, 3, 6),
    "z384_rate_one_third": (8424, 3168, 384, 1, 46),  # the whole circular buffer: every layer of the base graph
}
SIGMA = 0.10
NOF_FLIPS = 60  # "live throughout": sign-flipped LLRs of full magnitude in one codeblock


def layers_reached(seg, c):
    cols = -(-(seg.E[c] + seg.nof_filler_bits) // seg.Z)
    return max(4, min(max(cols, 24), seg.N // seg.Z) + 2 - 22)


@functools.lru_cache(maxsize=None)
def transport_block(shape, sigma, seed, flip_cb=-1):
    """(TB bytes, LLRs) of one codeword received at noise `sigma`; NOF_FLIPS LLRs of codeblock flip_cb are +-120 with the wrong sign.
    flip_cb = a tuple of soft-bit positions (column * Z + row) of codeblock 0: the codeword is received at +-120 throughout (no noise) and
    those bits with the wrong sign -- "stuck" bits where the column has two checks: -120 + 96 + 96 stays finite for ever."""
    tbs_bits, nsym, Z, ncb, lay = SHAPES[shape]
    seg = o_segmentation(tbs_bits, BG, MOD, 1, nsym)
    assert (seg.Z, seg.nof_cbs) == (Z, ncb) and all(layers_reached(seg, c) == lay for c in range(ncb)), shape
    rng = np.random.default_rng(seed)
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
    cw = o_pdsch_encode(BG, 0, MOD, 0, 1, nsym, tb)
    noise = rng.standard_normal(cw.size)
    llr = np.round(np.clip(4 * ((1.0 - 2.0 * (cw & 1)) + (sigma or 0.0) * noise), -20, 20) / 20 * 120).astype(np.int8)
    if isinstance(flip_cb, tuple):
        llr = (120 * (1 - 2 * (cw & 1).astype(np.int32))).astype(np.int8)
        F, Kq = seg.nof_filler_bits, seg.E[0] // MOD
        for sb in flip_cb:  # soft bit -> position of the circular buffer -> position behind the fillers -> interleaved LLR
            j = sb - 2 * Z
            assert j >= 20 * Z  # (behind the fillers)
            r = j - F
            k = seg.cw_offset[0] + (r % Kq) * MOD + r // Kq
            llr[k] = -llr[k]
    elif flip_cb >= 0:
        pos = seg.cw_offset[flip_cb] + rng.choice(seg.E[flip_cb], NOF_FLIPS, replace=False)
        llr[pos] = (120 * (2 * (cw[pos] & 1).astype(np.int32) - 1)).astype(np.int8)
    tb.setflags(write=False)
    llr.setflags(write=False)
    return tb, llr


@functools.lru_cache(maxsize=None)
def oracle_of(shape, sigma, seed, flip_cb, max_iter, early_stop):
    """The oracle's chain on the transport block: (TB CRC, TB, (iters min, max), codeblock CRC flags, hard bits, HARQ soft images)."""
    tbs_bits, nsym = SHAPES[shape][:2]
    od = OraclePuschDecoder(BG, MOD, 0, 1, nsym, tbs_bits // 8)
    od.softbuf[:] = 33
    ok, tbo, mm = od.decode(transport_block(shape, sigma, seed, flip_cb)[1], 0, True, max_iter, early_stop)
    return ok, tbo, mm, od.cb_crc.copy(), od.cb_msgs.reshape(od.seg.nof_cbs, -1).copy(), od.softbuf.reshape(od.seg.nof_cbs, -1).copy()


def codeblock_inputs(shape, sigma, seed, flip_cb=-1):
    """Per codeblock what the decoder is given: (dematched image of N soft bits, fillers, CRC polynomial, checked bits)."""
    tbs_bits, nsym, Z, ncb, _ = SHAPES[shape]
    seg = o_segmentation(tbs_bits, BG, MOD, 1, nsym)
    images = oracle_of(shape, sigma, seed, flip_cb, 1, False)[5]
    poly = O.CRC24B if ncb > 1 else O.CRC24A
    return [(images[c], seg.nof_filler_bits, poly, 22 * Z - seg.nof_filler_bits) for c in range(ncb)]


@functools.lru_cache(maxsize=None)
def soft_after(shape, sigma, seed, flip_cb, k):
    """Per codeblock (hard bits, soft bits of all 68 columns) after k iterations without a CRC (k = 0: the decoder's start)."""
    out = []
    for image, nf, _, _ in codeblock_inputs(shape, sigma, seed, flip_cb):
        Z = SHAPES[shape][2]
        if k == 0:
            out.append((None, np.concatenate([np.zeros(2 * Z, np.int8), image])))
        else:
            _, hard, soft = o_ldpc_decode(BG, Z, image, nf, -1, k, want_soft=True)
            out.append((hard, soft))
    return out


def sticky_skips(shape, sigma, seed, flip_cb, max_iter):
    """Per codeblock {(wavefront, layer): visits left out at least}: the pair is saturated at the visit of the first iteration k that STARTS
    with all its inputs infinite (earlier if the layers before it in iteration k - 1 finished the job), and left out in the max_iter - 1 - k
    iterations behind it. From the oracle's soft bits at iteration boundaries, so a lower bound."""
    return [left_out(sat, max_iter) for sat in saturation(shape, sigma, seed, flip_cb, max_iter)]


def saturation(shape, sigma, seed, flip_cb, max_iter):
    """Per codeblock saturated_from (ldpc_saturation_model) of the oracle's soft bits at the start of iterations 0 .. max_iter - 1."""
    Z, ncb, lay = SHAPES[shape][2:5]
    snaps = [soft_after(shape, sigma, seed, flip_cb, k) for k in range(max_iter)]
    return [saturated_from([snaps[k][c][1] for k in range(max_iter)], Z, lay) for c in range(ncb)]


# A soft bit of codeblock 0 of z384 received wrong at full magnitude in column 25, which layers 2 and 3 read and no other of the four: it
# stays finite (-120 + 96 + 96 = 72 at most) and keeps its rows alive for ever; so does a bit of the punctured column 1 next to it in
# those rows. In the oracle's soft bits wavefront 0 then runs layers 0, 2 and 3 to the end and leaves out layer 1 BETWEEN them, and
# wavefront 2 runs layer 3 alone: its address request crosses three set bits.
STUCK = (25 * 384 + 10,)


def crc_is_zero(hard, poly, nbits):
    return O.o_crc_bits(poly, np.unpackbits(hard)[:nbits]) == 0


CASES = [("z384", -1), ("z352", -1), ("z128", -1), ("z256", -1), ("z384_six_layers", -1), ("z384", 1), ("z384_rate_one_third", -1)]
MAX_K = 9


@pytest.mark.parametrize("shape,flip_cb", CASES)
def test_inputs_are_what_the_demapper_and_dematcher_leave(shape, flip_cb):
    Z = SHAPES[shape][2]
    for image, nf, _, _ in codeblock_inputs(shape, SIGMA, 100, flip_cb):
        f0 = 20 * Z - nf  # fillers: the last nf message bits, behind the two punctured columns
        assert (image[f0:f0 + nf] == 127).all() and (np.abs(np.delete(image.astype(np.int32), np.arange(f0, f0 + nf))) <= 120).all()


@pytest.mark.parametrize("shape,flip_cb", CASES)
def test_an_infinite_soft_bit_stays_infinite_with_its_sign(shape, flip_cb):
    seen = 0
    for k in range(1, MAX_K):
        for (_, a), (_, b) in zip(soft_after(shape, SIGMA, 100, flip_cb, k), soft_after(shape, SIGMA, 100, flip_cb, k + 1)):
            at = np.abs(a.astype(np.int32)) == 127
            assert np.array_equal(b[at], a[at]), (shape, k, int(np.sum(b[at] != a[at])))
            seen += int(at.sum())
    assert seen > 0


@pytest.mark.parametrize("shape,flip_cb", CASES)
def test_outputs_do_not_change_once_every_reached_soft_bit_is_saturated(shape, flip_cb):
    Z, ncb, lay = SHAPES[shape][2:5]
    inputs, reached, saturated = codeblock_inputs(shape, SIGMA, 100, flip_cb), (22 + lay) * Z, []
    for c in range(ncb):
        first = None
        for k in range(1, MAX_K + 1):
            hard, soft = soft_after(shape, SIGMA, 100, flip_cb, k)[c]
            if first is None and (np.abs(soft[:reached].astype(np.int32)) == 127).all():
                first = (k, hard, crc_is_zero(hard, *inputs[c][2:]))
            elif first is not None:
                assert np.array_equal(hard, first[1]) and crc_is_zero(hard, *inputs[c][2:]) == first[2], (shape, c, k)
        saturated.append(first[0] if first else None)
    # what the shapes are chosen for: clean codeblocks saturate within a few iterations (and pass their CRC); the codeblock with flipped
    # LLRs, the six-layer shape (untransmitted tail inside its reached columns) and the low rate (the parity columns behind column 25
    # have one check each: soft bit = channel value + one message, at most 24 + 96 here) never do
    if flip_cb >= 0:
        assert saturated[flip_cb] is None and all(s is not None for c, s in enumerate(saturated) if c != flip_cb), saturated
    elif shape in ("z384_six_layers", "z384_rate_one_third"):
        assert saturated == [None] * ncb, saturated
    else:
        assert all(s is not None and s <= 6 for s in saturated), saturated


@pytest.mark.parametrize("shape", ["z384_six_layers", "z384_rate_one_third"])
def test_shapes_that_mix_saturated_and_live_rows(shape):
    """Some (wavefront, layer) pairs are left out from some iteration on, others run to the end."""
    for per in sticky_skips(shape, SIGMA, 100, -1, 6):
        assert min(per.values()) == 0 and max(per.values()) > 0, per


def test_a_stuck_bit_leaves_dead_layers_below_live_ones():
    sat = saturation("z384", None, 100, STUCK, 8)[0]
    assert [sat[(0, m)] is None for m in range(4)] == [True, False, True, True], sat
    assert [sat[(2, m)] is None for m in range(4)] == [False, False, False, True], sat
    assert {(0, 1, 2), (0, 1, 3), (2, 0, 3), (2, 2, 3)} <= {(w, dead, live) for _, w, dead, live in dead_below_live(sat, 8)}
    hard = soft_after("z384", None, 100, STUCK, 8)[0][0]
    assert crc_is_zero(hard, O.CRC24B, 22 * 384 - 8)  # the checks hold the stuck bit on the right side: the codeblock decodes
