"""The PDUs of tests/test_pucch_f34_gpu.py, built once per process with the transmitter of tests/pucch_f34_tx.py; the CPU test
tests/test_pucch_f34_tx.py runs the float64 receiver over those whose outcome depends on the noise. An item is a dict: pdu, K, bits, noise,
grid ([port][14][12 GRID_NPRB] complex64, one grid per item unless stated)."""
import functools

import numpy as np

import pucch_f34_tx as X
import uci_polar as UP

GRID_NPRB = 34
PORTS = (1, 2, 4)
F3_PRBS = (1, 3, 5, 15, 16)  # 12 points; radix-3 passes; radix 5; a larger mixed size; the largest
# (length, hopping, additional DM-RS): one DM-RS symbol; one per hop; 5; 9; four DM-RS symbols (the noise is estimated); 14 both ways
F3_LENGTHS = ((4, 0, 0), (4, 1, 0), (5, 0, 0), (9, 1, 0), (10, 0, 1), (14, 0, 0), (14, 1, 1))
KS = (3, 11, 12, 19, 20, 100)  # short block; CRC6; CRC11
SEED0 = 30000  # of the grids of f3_set: no PDU of the sets sits in a fade that the float64 receiver cannot decode (tests/test_pucch_f34_tx.py)


def klass(K):
    return "short" if K <= 11 else ("crc6" if K <= 19 else "crc11")


def feasible(p, K):
    E = X.nof_soft_bits(p)
    return E > K if K <= 11 else UP.info(K, E) is not None


def roomy(p, K):
    """feasible, and a short-block payload has at least two soft bits per bit (11 bits in 12 soft bits are accepted but cannot be told apart)."""
    return feasible(p, K) and (K > 11 or X.nof_soft_bits(p) >= 2 * K)


def largest_feasible(p, K):
    return K if roomy(p, K) else max(k for k in KS if roomy(p, k))


def item(p, K, noise, seed, on=True):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, K).astype(np.uint8)
    grid = X.build_grid(seed, p["nports"], p["grid_nprb"], noise, [p], [bits], [on])
    return dict(pdu=p, K=K, bits=bits, noise=noise, grid=grid, on=on)


def _ids(rng):
    return dict(nid_hop=int(rng.integers(0, 1024)), nid_scr=int(rng.integers(0, 1024)), rnti=int(rng.integers(1, 65520)), slot=int(rng.integers(0, 20)))


@functools.lru_cache(maxsize=None)
def f3_set(nports):
    """Every PRB count of F3_PRBS with every length of F3_LENGTHS and both modulations on nports ports at 26 dB. The payload size goes round with the
    shape, the modulation and the port count, so that over the three port counts every (size, length) meets all six sizes of KS, three per modulation
    (where the allocation cannot carry one, the largest it can); plus 400 bits on 16 PRB x 14 symbols with QPSK (E = 4608 >= 1088: two polar segments)."""
    rng = np.random.default_rng(100 + nports)
    out, shape = [], 0
    for nprb in F3_PRBS:
        for nsym, hop, add in F3_LENGTHS:
            for pi2 in (0, 1):
                p = X.pdu(3, nsym, nprb, hop, add, pi2, nports=nports, prb=1, prb2=17, grid_nprb=GRID_NPRB, start=int(rng.integers(0, 15 - nsym)), **_ids(rng))
                K = largest_feasible(p, KS[(shape + 3 * pi2 + PORTS.index(nports)) % len(KS)])
                out.append(item(p, K, 0.05, SEED0 + 1000 * nports + 2 * shape + pi2))
            shape += 1
    p = X.pdu(3, 14, 16, 0, 0, pi2=0, nports=nports, prb=3, grid_nprb=GRID_NPRB, **_ids(rng))
    out.append(item(p, 400, 0.05, 1000 * nports + 999))
    return out


@functools.lru_cache(maxsize=None)
def f4_set():
    """Format 4: both sequence lengths, every sequence index, both modulations; length 4 with hopping (E = 6 for pi/2-BPSK on four sequences, the
    smallest there is) and length 14 with additional DM-RS. One PDU per grid."""
    rng = np.random.default_rng(44)
    out, i = [], 0
    for nsf in (2, 4):
        for idx in range(nsf):
            for pi2 in (0, 1):
                for nsym, hop, add in ((4, 1, 0), (14, 0, 1)):
                    p = X.pdu(4, nsym, 1, hop, add, pi2, nsf, idx, nports=PORTS[i % 3], prb=5, prb2=20, grid_nprb=GRID_NPRB, **_ids(rng))
                    out.append(item(p, largest_feasible(p, (3, 11, 12, 20)[(i // 2) % 4]), 0.05, 4000 + i))
                    i += 1
    assert min(X.nof_soft_bits(d["pdu"]) for d in out) == 6
    return out


# (K, format, nof_prb, length, pi/2-BPSK, sequences): two shapes per payload class, small enough for the noise to matter
NOISY_SHAPES = ((3, 4, 1, 4, 1, 4), (11, 3, 1, 4, 0, 0), (12, 3, 1, 5, 1, 0), (19, 4, 1, 14, 0, 2), (20, 3, 1, 4, 0, 0), (100, 3, 3, 5, 0, 0))
NOISY_LEVELS = (0.1, 1.0, 2.5)


@functools.lru_cache(maxsize=None)
def noisy_set():
    """The shapes of NOISY_SHAPES at three noise levels on one and two ports: with at most two DM-RS symbols the noise variance is EPRE / 1000,
    so the demapper saturates and the decoders see nearly hard decisions. tests/test_pucch_f34_tx.py asserts with the float64 receiver that every
    class (short block, CRC6, CRC11) gets both verdicts."""
    rng = np.random.default_rng(9)
    out, i = [], 0
    for K, fmt, nprb, nsym, pi2, nsf in NOISY_SHAPES:
        for noise in NOISY_LEVELS:
            for nports in (1, 2):
                p = X.pdu(fmt, nsym, nprb, 0, 0, pi2, nsf, nsf // 2, nports=nports, prb=7, grid_nprb=GRID_NPRB, **_ids(rng))
                out.append(item(p, K, noise, 7000 + i))
                i += 1
    return out


@functools.lru_cache(maxsize=None)
def multiplexed(nsf):
    """All nsf format-4 PDUs of one PRB, each with a payload of its own, in one two-port grid at 20 dB: (PDUs, bits, grid)."""
    rng = np.random.default_rng(60 + nsf)
    ids = _ids(rng)
    pdus = [X.pdu(4, 14, 1, 1, 1, 0, nsf, idx, nports=2, prb=4, prb2=25, grid_nprb=GRID_NPRB, **dict(ids, rnti=100 + idx)) for idx in range(nsf)]
    bits = [rng.integers(0, 2, K).astype(np.uint8) for K in (7, 12, 20, 11)[:nsf]]
    return pdus, bits, X.build_grid(600 + nsf, 2, GRID_NPRB, 0.1, pdus, bits)


@functools.lru_cache(maxsize=None)
def mixed_items():
    """Format-3 and format-4 PDUs of different sizes, port counts and payload classes side by side on one four-port grid."""
    rng = np.random.default_rng(5)

    def ids():
        return dict(nid_hop=int(rng.integers(0, 1024)), nid_scr=int(rng.integers(0, 1024)), rnti=int(rng.integers(1, 65520)), slot=11)

    def mk(fmt, nsym, nprb, hop, add, pi2, nsf, idx, nports, start, prb, prb2):
        return X.pdu(fmt, nsym, nprb, hop, add, pi2, nsf, idx, nports=nports, start=start, prb=prb, prb2=prb2, grid_nprb=GRID_NPRB, **ids())

    pdus = [mk(3, 14, 5, 0, 1, 0, 0, 0, 4, 0, 0, 0), mk(4, 14, 1, 1, 0, 1, 2, 1, 2, 0, 5, 33), mk(3, 4, 16, 0, 0, 1, 0, 0, 1, 0, 6, 6),
            mk(3, 9, 3, 1, 0, 0, 0, 0, 3, 4, 6, 28), mk(4, 7, 1, 0, 0, 0, 4, 3, 4, 4, 9, 9), mk(3, 10, 1, 0, 1, 0, 0, 0, 2, 4, 10, 10),
            mk(3, 5, 15, 1, 0, 0, 0, 0, 4, 9, 11, 12), mk(4, 4, 1, 1, 0, 1, 4, 2, 1, 0, 32, 23)]
    Ks = [100, 12, 11, 20, 3, 19, 400, 3]
    bits = [rng.integers(0, 2, K).astype(np.uint8) for K in Ks]
    grid = X.build_grid(55, 4, GRID_NPRB, 0.1, pdus, bits)
    return [dict(pdu=p, K=K, bits=b, grid=grid) for p, K, b in zip(pdus, Ks, bits)]
