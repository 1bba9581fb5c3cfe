"""PUCCH format 2 with more than 11 UCI bits: the transmitter of tests/pucch_tx.py with the payload coding of tests/uci_polar.py (TS
38.212 6.3.1: CRC6 / CRC11 and the polar code) in place of the short block code. The 23.5 reference neither sends nor receives such a
PDU; miphy_pucch_process_batch_ex is checked against this transmitter composed with the polar restatements.

Configuration rows are those of pucch_tx (the H_* indices); the bits of a PDU are in pucch_uci_message order, HARQ-ACK, SR, CSI part 1.
build_grid takes format-1, short format-2 and long format-2 PDUs together: a PDU of format 2 is long when it carries 12 bits or more."""
import cmath
import math

import numpy as np

import pucch_tx as T
import uci_polar as U
from pucch_tx import (F2_DATA_SC, F2_DMRS_SC, H_BWP_START, H_FMT, H_NID, H_NID0, H_NPRB, H_NSYM, H_PRB, H_RNTI, H_SLOT, H_START, gold)

# (K, nof_prb, nof_symbols): every framing class a format-2 PDU can reach (E = 16 nof_prb nof_symbols <= 512, one segment).
SHAPES = [(12, 2, 1),     # CRC6, 3 parity-check bits, N = E = 32
          (19, 3, 1),     # CRC6, shortening: E = 48, N = 64
          (20, 2, 1),     # CRC11, K_r = 31 of N = E = 32
          (20, 3, 2),     # CRC11, puncturing: E = 96, N = 128
          (40, 9, 1),     # CRC11, repetition: E = 144, N = 128
          (12, 16, 2),    # CRC6, repetition with E = 2 N = 512
          (100, 16, 2),   # CRC11, N = E = 512
          (500, 16, 2)]   # CRC11, K_r = 511 of N = E = 512: the largest accepted
REFUSED = [(12, 1, 1), (21, 2, 1), (501, 16, 2)]


def nof_soft_bits(nprb, nsym):
    return 16 * nprb * nsym


def scrambling(c, E):
    return gold(int(c[H_RNTI]) * 2 ** 15 + int(c[H_NID]), E)


def coded_bits(c, bits):
    """The E scrambled bits of one long format-2 PDU, as they are modulated."""
    E = nof_soft_bits(int(c[H_NPRB]), int(c[H_NSYM]))
    return U.encode(len(bits), E, np.asarray(bits, np.uint8)) ^ scrambling(c, E)


def f2_long_symbols(c, bits):
    """Transmitted REs of one long format-2 PDU: list of (symbol, subcarrier array, values), DM-RS and mapping as pucch_tx.f2_symbols."""
    c = [int(x) for x in c]
    nprb, nsym, s = c[H_NPRB], c[H_NSYM], c[H_START]
    prb0 = c[H_BWP_START] + c[H_PRB]
    b = coded_bits(c, bits)
    q = ((1 - 2.0 * b[0::2]) + 1j * (1 - 2.0 * b[1::2])) / np.sqrt(2)
    out = []
    data_sc = (12 * np.arange(nprb)[:, None] + np.array(F2_DATA_SC)[None, :]).ravel() + 12 * prb0
    dmrs_sc = (12 * np.arange(nprb)[:, None] + np.array(F2_DMRS_SC)[None, :]).ravel() + 12 * prb0
    for i in range(nsym):
        l = s + i
        c_init = ((14 * c[H_SLOT] + l + 1) * (2 * c[H_NID0] + 1) * 2 ** 17 + 2 * c[H_NID0]) % 2 ** 31
        g = gold(c_init, 8 * prb0 + 8 * nprb)[8 * prb0:]
        r = ((1 - 2.0 * g[0::2]) + 1j * (1 - 2.0 * g[1::2])) / np.sqrt(2)
        out.append((l, dmrs_sc, r))
        out.append((l, data_sc, q[8 * nprb * i:8 * nprb * (i + 1)]))
    return out


def pdu_symbols(c, bits):
    if c[H_FMT] == 1:
        return T.f1_symbols(c, bits)
    return T.f2_symbols(c, bits) if len(bits) <= 11 else f2_long_symbols(c, bits)


def build_grid(seed, nports, grid_nprb, noise_std, cfgs, bits, tx_on):
    """pucch_tx.build_grid (per-PDU complex gain per port and delay ramp, then AWGN; the same draws in the same order, so a group
    without long PDUs gives that function's grid bit for bit) for PDUs of all three kinds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nsc = 12 * grid_nprb
    grid = np.zeros((nports, 14, nsc), np.complex128)
    for c, b, on in zip(cfgs, bits, tx_on):
        gain = (rng.standard_normal(nports) + 1j * rng.standard_normal(nports)) / np.sqrt(2)
        delay = rng.uniform(-0.004, 0.004)
        if not on:
            continue
        h = gain[:, None] * np.array([cmath.exp(-2j * math.pi * delay * kk) for kk in range(nsc)])[None, :]
        for l, sc, v in pdu_symbols(c, b):
            idx = np.arange(sc, sc + 12) if np.isscalar(sc) else sc
            grid[:, l, idx] += h[:, idx] * v[None, :]
    noise = (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * (noise_std / np.sqrt(2))
    return (grid + noise).astype(np.complex64)


def f2_cfg(nprb, nsym, start_symbol, starting_prb, grid_nprb, nports, rnti, n_id, n_id_0, slot=3, numerology=1):
    """A format-2 configuration row whose BWP is the whole grid."""
    c = np.zeros(T.NHDR, np.int64)
    c[H_FMT], c[T.H_NUM], c[H_SLOT], c[T.H_NPORTS], c[H_START], c[H_NSYM] = 2, numerology, slot, nports, start_symbol, nsym
    c[H_BWP_START], c[T.H_BWP_SIZE], c[H_PRB], c[H_NPRB] = 0, grid_nprb, starting_prb, nprb
    c[H_NID], c[H_NID0], c[H_RNTI], c[T.H_GRID_NPRB] = n_id, n_id_0, rnti, grid_nprb
    return c
