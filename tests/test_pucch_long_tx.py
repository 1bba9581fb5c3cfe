"""CPU: the long format-2 transmitter of tests/pucch_long_tx.py. Its shape table covers the framing classes it names (checked with
uci_polar.info), and the coded bits of every shape, descrambled and turned into ideal soft bits, decode to the payload with a passing
CRC through the polar restatement. A group without long PDUs gives pucch_tx.build_grid's grid bit for bit."""
import numpy as np
import pytest

import pucch_long_tx as LT
import pucch_tx as T
import uci_polar as U

# (K, PRB, symbols) -> (E, N, CRC bits, parity-check bits, rate matching)
TABLE = {(12, 2, 1): (32, 32, 6, 3, "none"),
         (19, 3, 1): (48, 64, 6, 3, "shortening"),
         (20, 2, 1): (32, 32, 11, 0, "none"),
         (20, 3, 2): (96, 128, 11, 0, "puncturing"),
         (40, 9, 1): (144, 128, 11, 0, "repetition"),
         (12, 16, 2): (512, 256, 6, 3, "repetition"),
         (100, 16, 2): (512, 512, 11, 0, "none"),
         (500, 16, 2): (512, 512, 11, 0, "none")}


def rate_matching(K_r, E, N):
    """TS 38.212 5.4.1.2."""
    if E >= N:
        return "none" if E == N else "repetition"
    return "puncturing" if 16 * K_r <= 7 * E else "shortening"


def test_shape_table_covers_the_framing_classes():
    assert sorted(LT.SHAPES) == sorted(TABLE)
    for (K, nprb, nsym), (E, N, crc, npc, rm) in TABLE.items():
        assert LT.nof_soft_bits(nprb, nsym) == E and nprb <= 16 and nsym <= 2
        f = U.info(K, E)
        assert f is not None and f["C"] == 1 and f["pad"] == 0, (K, E)
        assert (1 << f["n"], f["L"], f["nPC"], f["K_r"], f["E_r"]) == (N, crc, npc, K + crc, E), (K, E, f)
        assert rate_matching(f["K_r"], E, N) == rm, (K, E)
    assert U.info(20, 32)["K_r"] == 31 and U.info(500, 512)["K_r"] == 511 and U.info(12, 512)["E_r"] == 2 * (1 << U.info(12, 512)["n"])
    assert sorted(LT.REFUSED) == [(12, 1, 1), (21, 2, 1), (501, 16, 2)]
    for K, nprb, nsym in LT.REFUSED:
        assert U.info(K, LT.nof_soft_bits(nprb, nsym)) is None, (K, nprb, nsym)
    # every CRC class, every rate-matching mode and the smallest and largest code of the format are in the table
    assert {v[2] for v in TABLE.values()} == {6, 11} and {v[4] for v in TABLE.values()} == {"none", "shortening", "puncturing", "repetition"}
    assert {v[1] for v in TABLE.values()} >= {32, 512}


@pytest.mark.parametrize("shape", LT.SHAPES)
def test_coded_bits_decode_to_the_payload(shape):
    K, nprb, nsym = shape
    E = LT.nof_soft_bits(nprb, nsym)
    rng = np.random.default_rng(100 + K + E)
    bits = rng.integers(0, 2, K).astype(np.uint8)
    c = LT.f2_cfg(nprb, nsym, 5, 7, 52, 2, rnti=0x4601 + K, n_id=(77 * K) % 1024, n_id_0=(31 * E) % 1024)
    b = LT.coded_bits(c, bits)
    assert b.size == E and not np.array_equal(b, U.encode(K, E, bits))  # scrambled
    # the transmitted REs carry these bits as QPSK, symbol after symbol, PRB after PRB, on the data subcarriers
    q = np.concatenate([v for l, sc, v in LT.f2_long_symbols(c, bits)[1::2]])
    assert np.array_equal((q.real < 0).astype(np.uint8), b[0::2]) and np.array_equal((q.imag < 0).astype(np.uint8), b[1::2])
    llr = (20 * (1 - 2 * (b ^ LT.scrambling(c, E)).astype(np.int64))).astype(np.int8)
    payload, valid = U.decode(K, E, llr)
    assert valid and np.array_equal(payload, bits)


def test_a_group_without_long_pdus_is_the_short_transmitters_grid():
    rng = np.random.default_rng(5)
    c2 = LT.f2_cfg(3, 2, 4, 10, 24, 2, rnti=0x1234, n_id=300, n_id_0=17)
    c1 = c2.copy()
    c1[T.H_FMT], c1[T.H_START], c1[T.H_NSYM], c1[T.H_PRB], c1[T.H_NHARQ] = 1, 0, 14, 2, 2
    cfgs, bits = [c1, c2, c2], [[1, 0], [int(b) for b in rng.integers(0, 2, 7)], [int(b) for b in rng.integers(0, 2, 11)]]
    on = [True, True, False]
    assert np.array_equal(LT.build_grid(9, 2, 24, 0.1, cfgs, bits, on), T.build_grid(9, 2, 24, 0.1, cfgs, bits, on))
    long_bits = [int(b) for b in rng.integers(0, 2, 20)]
    g = LT.build_grid(9, 2, 24, 0.1, cfgs, [bits[0], long_bits, bits[2]], on)
    assert not np.array_equal(g, T.build_grid(9, 2, 24, 0.1, cfgs, bits, on))
    assert np.array_equal(g, LT.build_grid(9, 2, 24, 0.1, cfgs, [bits[0], long_bits, bits[2]], on))  # deterministic in the seed
