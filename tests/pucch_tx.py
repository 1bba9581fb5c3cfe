"""PUCCH formats 1 and 2 transmitter and channel, restated from TS 38.211 6.3.2.2, 6.3.2.4, 6.3.2.5, 6.4.1.3.1 and 6.4.1.3.2 (normal
cyclic prefix, no group or sequence hopping) with the payload coding of tests/uci_short_block.py. It rebuilds the resource grids of
tests/golden/pucch_processor.npz bit for bit from a seed and the PDU configurations: the fixture stores no grid, only its SHA-256.

Grid layout: [port][14][grid_nprb * 12] complex64, the layout of the rest of the uplink.
Configuration rows (int32, the `hdr` of tools/gen_pucch_golden.cpp): see the H_* indices below.
"""
import cmath
import functools
import hashlib
import math

import numpy as np

import uci_short_block as U

(H_FMT, H_NUM, H_SLOT, H_NPORTS, H_START, H_NSYM, H_BWP_START, H_BWP_SIZE, H_PRB, H_HOP, H_PRB2, H_NPRB, H_NID, H_NID0, H_RNTI, H_ICS,
 H_OCC, H_NHARQ, H_NSR, H_NCSI1, H_GRID_NPRB) = range(21)
NHDR = 21
NRE = 12

# TS 38.211 Table 5.2.2.2-2: phi(n) of the length-12 base sequences, u = 0..29.
PHI12 = np.array([
    (-3, 1, -3, -3, -3, 3, -3, -1, 1, 1, 1, -3),
    (-3, 3, 1, -3, 1, 3, -1, -1, 1, 3, 3, 3),
    (-3, 3, 3, 1, -3, 3, -1, 1, 3, -3, 3, -3),
    (-3, -3, -1, 3, 3, 3, -3, 3, -3, 1, -1, -3),
    (-3, -1, -1, 1, 3, 1, 1, -1, 1, -1, -3, 1),
    (-3, -3, 3, 1, -3, -3, -3, -1, 3, -1, 1, 3),
    (1, -1, 3, -1, -1, -1, -3, -1, 1, 1, 1, -3),
    (-1, -3, 3, -1, -3, -3, -3, -1, 1, -1, 1, -3),
    (-3, -1, 3, 1, -3, -1, -3, 3, 1, 3, 3, 1),
    (-3, -1, -1, -3, -3, -1, -3, 3, 1, 3, -1, -3),
    (-3, 3, -3, 3, 3, -3, -1, -1, 3, 3, 1, -3),
    (-3, -1, -3, -1, -1, -3, 3, 3, -1, -1, 1, -3),
    (-3, -1, 3, -3, -3, -1, -3, 1, -1, -3, 3, 3),
    (-3, 1, -1, -1, 3, 3, -3, -1, -1, -3, -1, -3),
    (1, 3, -3, 1, 3, 3, 3, 1, -1, 1, -1, 3),
    (-3, 1, 3, -1, -1, -3, -3, -1, -1, 3, 1, -3),
    (-1, -1, -1, -1, 1, -3, -1, 3, 3, -1, -3, 1),
    (-1, 1, 1, -1, 1, 3, 3, -1, -1, -3, 1, -3),
    (-3, 1, 3, 3, -1, -1, -3, 3, 3, -3, 3, -3),
    (-3, -3, 3, -3, -1, 3, 3, 3, -1, -3, 1, -3),
    (3, 1, 3, 1, 3, -3, -1, 1, 3, 1, -1, -3),
    (-3, 3, 1, 3, -3, 1, 1, 1, 1, 3, -3, 3),
    (-3, 3, 3, 3, -1, -3, -3, -1, -3, 1, 3, -3),
    (3, -1, -3, 3, -3, -1, 3, 3, 3, -3, -1, -3),
    (-3, -1, 1, -3, 1, 3, 3, 3, -1, -3, 3, 3),
    (-3, 3, 1, -1, 3, 3, -3, 1, -1, 1, -1, 1),
    (-1, 1, 3, -3, 1, -1, 1, -1, -1, -3, 1, -1),
    (-3, -3, 3, 3, 3, -3, -1, 1, -3, 3, 1, -3),
    (1, -1, 3, 1, 1, -1, -1, -1, 1, 3, -3, 1),
    (-3, 3, -3, 3, -3, -3, 3, -1, -1, 1, 3, -3),
], np.int64)

# TS 38.211 Table 6.3.2.4.1-2: phi of the orthogonal sequences w_i(m) = exp(j 2 pi phi(m) / N), indexed [N - 1][i].
OCC_PHI = [
    [[0]],
    [[0, 0], [0, 1]],
    [[0, 0, 0], [0, 1, 2], [0, 2, 1]],
    [[0, 0, 0, 0], [0, 2, 0, 2], [0, 0, 2, 2], [0, 2, 2, 0]],
    [[0, 0, 0, 0, 0], [0, 1, 2, 3, 4], [0, 2, 4, 1, 3], [0, 3, 1, 4, 2], [0, 4, 3, 2, 1]],
    [[0, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5], [0, 2, 4, 0, 2, 4], [0, 3, 0, 3, 0, 3], [0, 4, 2, 0, 4, 2], [0, 5, 4, 3, 2, 1]],
    [[0, 0, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6], [0, 2, 4, 6, 1, 3, 5], [0, 3, 6, 2, 5, 1, 4], [0, 4, 1, 5, 2, 6, 3],
     [0, 5, 3, 1, 6, 4, 2], [0, 6, 5, 4, 3, 2, 1]],
]

F2_DMRS_SC = (1, 4, 7, 10)
F2_DATA_SC = (0, 2, 3, 5, 6, 8, 9, 11)


@functools.lru_cache(maxsize=None)
def low_papr_table():
    """[30][12][12] complex64: r_u(n) exp(j alpha_k n), alpha_k = 2 pi k / 12, with single-precision arguments."""
    out = np.zeros((30, NRE, NRE), np.complex64)
    n = np.arange(NRE, dtype=np.float32)
    for u in range(30):
        arg = (PHI12[u].astype(np.float32) * np.float32(np.pi / 4)).astype(np.float32)
        for k in range(NRE):
            alpha = np.float32(np.float32(2 * np.pi) * np.float32(k) / np.float32(NRE))
            # arg + alpha n in one rounding (the reference's build contracts it into a fused multiply-add)
            a = (arg.astype(np.float64) + np.float64(alpha) * n.astype(np.float64)).astype(np.float32).astype(np.float64)
            out[u, k] = [complex(math.cos(x), math.sin(x)) for x in a]  # scalar libm: no vectorised math that may differ per CPU
    return out


def gold(c_init, nbits):
    """TS 38.211 5.2.1 pseudo-random sequence c(0 .. nbits - 1)."""
    return _gold(int(c_init), max(int(nbits), 2304))[:nbits]


@functools.lru_cache(maxsize=4096)
def _gold(c_init, nbits):
    n = nbits + 1600 + 31
    x1 = np.zeros(n, np.uint8)
    x2 = np.zeros(n, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> i) & 1 for i in range(31)]
    for i in range(n - 31):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    out = x1[1600:1600 + nbits] ^ x2[1600:1600 + nbits]
    out.setflags(write=False)
    return out


def alpha_index(n_id, n_slot, symbol, m0):
    """TS 38.211 6.3.2.2.2 with m_cs = 0: index k of alpha = 2 pi k / 12 for the absolute symbol of the slot."""
    c = gold(n_id, 8 * 14 * (n_slot + 1))
    base = 8 * 14 * n_slot + 8 * symbol
    n_cs = sum(int(c[base + m]) << m for m in range(8))
    return (m0 + n_cs) % NRE


def occ(n, i, m):
    """w_i(m) for a sequence of length n (1..7); an index beyond the table gives 1, as the reference's zero-filled table does."""
    ph = OCC_PHI[n - 1][i][m] if i < n else 0
    return cmath.exp(2j * math.pi * ph / n)


def f1_layout(nsym, hop):
    """(dmrs offsets per hop, data offsets per hop) relative to the start symbol."""
    if hop:
        h = nsym // 2
        dm = [[o for o in range(0, nsym, 2) if o < h], [o for o in range(0, nsym, 2) if o >= h]]
        nd = nsym // 2
        pre = nsym // 4
        data = [[1 + 2 * i for i in range(pre)], [1 + 2 * i for i in range(pre, nd)]]
    else:
        dm = [list(range(0, nsym, 2)), []]
        data = [[1 + 2 * i for i in range(nsym // 2)], []]
    return dm, data


def f1_symbols(c, bits):
    """Transmitted REs of one format-1 PDU: list of (symbol, first subcarrier, 12 complex values). bits: the HARQ-ACK bits, or [0]
    for a positive SR alone."""
    c = [int(x) for x in c]
    u = c[H_NID] % 30
    n_slot = c[H_SLOT]
    s = c[H_START]
    hop = c[H_HOP] != 0
    prb = [c[H_BWP_START] + c[H_PRB], c[H_BWP_START] + (c[H_PRB2] if hop else c[H_PRB])]
    if len(bits) == 1:
        d = (1 - 2 * bits[0]) * (1 + 1j) / np.sqrt(2)
    else:
        d = ((1 - 2 * bits[0]) + 1j * (1 - 2 * bits[1])) / np.sqrt(2)
    tab = low_papr_table().astype(np.complex128)
    dm, data = f1_layout(c[H_NSYM], hop)
    out = []
    for h in range(2):
        for m, o in enumerate(dm[h]):
            r = tab[u, alpha_index(c[H_NID], n_slot, s + o, c[H_ICS])]
            out.append((s + o, 12 * prb[h], occ(len(dm[h]), c[H_OCC], m) * r))
        for m, o in enumerate(data[h]):
            r = tab[u, alpha_index(c[H_NID], n_slot, s + o, c[H_ICS])]
            out.append((s + o, 12 * prb[h], occ(len(data[h]), c[H_OCC], m) * d * r))
    return out


def f2_symbols(c, bits):
    """Transmitted REs of one format-2 PDU: list of (symbol, subcarrier array, values)."""
    c = [int(x) for x in c]
    K = len(bits)
    nprb, nsym, s = c[H_NPRB], c[H_NSYM], c[H_START]
    prb0 = c[H_BWP_START] + c[H_PRB]
    E = 16 * nprb * nsym
    b = U.rate_match(U.encode(np.asarray(bits, np.uint8), 2), E) ^ gold(c[H_RNTI] * 2 ** 15 + c[H_NID], E)
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


def build_grid(seed, nports, grid_nprb, noise_std, cfgs, bits, tx_on):
    """The received grid of one group of PDUs sharing a slot: every transmitting PDU goes through its own per-port complex gain and
    delay ramp, then AWGN of standard deviation noise_std per complex dimension pair. Deterministic in `seed` (numpy PCG64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nsc = 12 * grid_nprb
    grid = np.zeros((nports, 14, nsc), np.complex128)
    for c, b, on in zip(cfgs, bits, tx_on):
        gain = (rng.standard_normal(nports) + 1j * rng.standard_normal(nports)) / np.sqrt(2)
        delay = rng.uniform(-0.004, 0.004)  # cycles per subcarrier: up to about +-16 taps of the 4096-point IDFT
        if not on:
            continue
        res = f1_symbols(c, b) if c[H_FMT] == 1 else f2_symbols(c, b)
        h = gain[:, None] * np.array([cmath.exp(-2j * math.pi * delay * kk) for kk in range(nsc)])[None, :]
        for l, sc, v in res:
            idx = np.arange(sc, sc + 12) if np.isscalar(sc) else sc
            grid[:, l, idx] += h[:, idx] * v[None, :]
    noise = (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * (noise_std / np.sqrt(2))
    return (grid + noise).astype(np.complex64)


def grid_hash(grid):
    return hashlib.sha256(np.ascontiguousarray(grid, np.complex64).tobytes()).hexdigest()


def fixture_grids(fx):
    """Rebuilds every group grid of a loaded fixture: a list indexed by group."""
    cfg, grp, bits, nbits, on = fx["cfg"], fx["group"], fx["tx_bits"], fx["tx_nbits"], fx["tx_on"]
    out = []
    for g in range(len(fx["g_seed"])):
        sel = np.nonzero(grp == g)[0]
        out.append(build_grid(int(fx["g_seed"][g]), int(fx["g_nports"][g]), int(fx["g_grid_nprb"][g]), float(fx["g_noise"][g]),
                              [cfg[i] for i in sel], [[int(b) for b in bits[i, :nbits[i]]] for i in sel], [bool(on[i]) for i in sel]))
    return out
