"""CPU: the transmitter assembled from oracle pieces (tests/sch_tx.py) equals o_pdsch_encode when nothing is corrupted, and a
corruption behind the codeblock CRCs gives the outcome the GPU tests lean on: every codeblock decodes, the transport-block CRC
fails, the oracle hands out the (corrupted) transport block and clears every codeblock flag (pusch_decoder_impl.cpp:198-222)."""
import numpy as np
import pytest

from oracle_lib import OraclePuschDecoder, o_pdsch_encode, o_segmentation
from sch_tx import cb_payload_range, sch_codeword

# bg, transport block bytes, codeblocks, zero pad
SIZES = [(1, 1000, 1, 0), (2, 40, 1, 0), (1, 1055, 2, 0), (2, 479, 2, 0), (2, 1248, 3, 0), (1, 5252, 5, 0), (2, 1907, 5, 0),
         (1, 8429, 9, 8), (2, 3821, 9, 8), (1, 54753, 52, 0), (2, 24801, 52, 0)]


def _nsym(seg_cbs, tb_bytes, mod, nl, k):
    """About rate 1/2, a multiple of the layers, and short and long segments where there are several codeblocks."""
    per_layer = (2 * (tb_bytes * 8 + 24) + mod * nl - 1) // (mod * nl) + k
    while seg_cbs > 1 and per_layer % seg_cbs == 0:
        per_layer += 1
    return per_layer * nl


def test_uncorrupted_equals_the_oracle_encoder():
    rng = np.random.default_rng(11)
    seen = set()
    for i, (bg, nbytes, ncb, pad) in enumerate(SIZES):
        for j, (rv, limited) in enumerate(((0, False), (2, False), (0, True), (2, True))):
            mod, nl = (1, 2, 4, 6, 8)[(i + j) % 5], 1 + (i + j) % 4
            nsym = _nsym(ncb, nbytes, mod, nl, j)
            seg = o_segmentation(nbytes * 8, bg, mod, nl, nsym)
            assert (seg.nof_cbs, seg.zero_pad) == (ncb, pad), (bg, nbytes, seg.nof_cbs, seg.zero_pad)
            Nref = (seg.N * 2) // 3 if limited else 0
            tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
            cw, payload = sch_codeword(bg, rv, mod, Nref, nl, nsym, tb)
            assert np.array_equal(payload, tb)
            assert np.array_equal(cw, o_pdsch_encode(bg, rv, mod, Nref, nl, nsym, tb)), (bg, nbytes, rv, mod, nl, Nref)
            seen.add((bg, ncb, nl, rv, limited))
    assert {x[2] for x in seen} == {1, 2, 3, 4} and {x[1] for x in seen} == {1, 2, 3, 5, 9, 52}


@pytest.mark.parametrize("bg,nbytes,ncb,pad", SIZES)
def test_corruption_behind_the_codeblock_crcs(bg, nbytes, ncb, pad):
    rng = np.random.default_rng(12 + nbytes)
    mod, nl = 2, 1
    nsym = _nsym(ncb, nbytes, mod, nl, 0)
    seg = o_segmentation(nbytes * 8, bg, mod, nl, nsym)
    tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
    kinds = [dict(tb_crc_flip=0x5)]
    for c in sorted({0, ncb // 2, ncb - 1}):
        lo, hi = cb_payload_range(seg, c)
        kinds.append(dict(flip_bits=[(lo, (lo + hi) // 2, hi)[c % 3]]))
    for kw in kinds:
        cw, payload = sch_codeword(bg, 0, mod, 0, nl, nsym, tb, **kw)
        assert np.array_equal(payload, tb) == ("tb_crc_flip" in kw)
        od = OraclePuschDecoder(bg, mod, 0, nl, nsym, nbytes)
        ok, tbo, mm = od.decode(((1 - 2 * cw.astype(np.int8)) * 60).astype(np.int8), 0, True, 6, True)
        assert not ok and not od.cb_crc.any(), (kw, ok, od.cb_crc)
        if ncb > 1:  # every codeblock passed its own CRC (one iteration each), so the transport block was handed out
            assert mm == (1, 1) and np.array_equal(tbo, payload), kw
        else:  # the codeblock's CRC is the transport block's: the decoder itself fails, nothing is handed out
            assert mm == (6, 6) and not tbo.any(), kw
