"""The DM-RS estimator for PUSCH on 1..4 layers, on the host, in float64: what miphy_dmrs_pusch_estimate_layers_batch is held to. The 23.5
reference is no oracle here: its estimator runs every layer through a one-layer least-squares fit and never undoes the frequency-domain OCC, so
two layers that share a CDM group come out as h_a +- h_b. The arithmetic is restated from include/miphy.h:

  estimate()        per (rx port, CDM group): least squares against layer 0's pilot, despreading by pairs that stay inside a PRB, the reference's
                    linear interpolator (stride 4; a layer alone in its group: stride 2, everything as the one-layer estimator), the scalars
  make_case()       a grid with the real DM-RS of every layer (Gold sequence, amplitude, OCC weight on the odd pilots of the odd layers) through a
                    smooth channel: one L x P matrix from pusch_layers_cases.channels() times the two-tap profile of tests/test_chest_gpu.py
  chain_tx()        a transport block on L layers through that channel, DM-RS included: what the fused processor receives
  CHAIN_CASES       the transmissions that decode through estimate() -> expected_llr() -> the oracle decoder (test_pusch_layers_estimator.py)

A case is the tuple tests/test_chest_gpu.py uses: (numerology, slot, False, scrambling id, n_scid, scaling, DM-RS symbol mask [14], PRB mask,
first symbol, number of symbols, layers, grid [port][14][nsc])."""
import numpy as np

import oracle_lib as O
import pusch_layers_cases as PL

BETA = 10 ** (3 / 20)  # DM-RS amplitude with two CDM groups without data
CE_DFT, HALF_CP = 4096, 144


def gold_pilots(nprb_grid, slot, l, scr, nscid):
    """Layer 0's pilots of OFDM symbol l counted from PRB 0: complex128 [6 * nprb_grid]."""
    c_init = (((14 * slot + l + 1) * (2 * scr + 1)) % (1 << 31) * (1 << 17) + 2 * scr + nscid) % (1 << 31)
    c = O.o_gold(c_init, 0, 12 * nprb_grid).astype(np.float64)
    return ((1 - 2 * c[0::2]) + 1j * (1 - 2 * c[1::2])) / np.sqrt(2)


def _interpolate(anchors, stride, offset, nout):
    """interpolator_linear_impl.cpp in closed form: anchor m at offset + stride m, edges held."""
    k = np.arange(nout) - offset
    i = np.clip(k // stride, 0, anchors.size - 1)
    i1 = np.minimum(i + 1, anchors.size - 1)
    f = np.where((k <= 0) | (i >= anchors.size - 1), 0.0, (k % stride) / stride)
    return anchors[i] + (anchors[i1] - anchors[i]) * f


def _time_alignment(values_at, mu):
    """values_at: (subcarriers, values) -> seconds: peak of the zero-padded 4096-point IDFT over the first / last 144 taps, first occurrence wins."""
    buf = np.zeros(CE_DFT, np.complex128)
    buf[values_at[0]] = values_at[1]
    p = np.abs(np.fft.ifft(buf)) ** 2
    dly, adv = p[:HALF_CP], p[CE_DFT - HALF_CP:]
    idl, iad = int(np.argmax(dly)), int(np.argmax(adv))
    taps = idl if dly[idl] >= adv[iad] else -(HALF_CP - iad)
    return taps / (CE_DFT * 15000.0 * (1 << mu))


def estimate(mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl, g):
    """-> (ce complex128 [nl][ports][first + nof][nsc], NaN where nothing is written; scalars float64 [ports][nl][5])."""
    assert not type2
    g = np.asarray(g).astype(np.complex128)
    nports, _, nsc = g.shape
    beta = float(scaling)
    prbs = np.nonzero(rb)[0]
    nprb, npil = prbs.size, prbs.size * 6
    dsyms = [l for l in range(first, first + nof) if sm[l]]
    nds = len(dsyms)
    gp = (prbs[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)  # pilot index counted from PRB 0
    cols = (prbs[:, None] * 12 + np.arange(12)[None, :]).reshape(-1)
    ce = np.full((nl, nports, first + nof, nsc), np.nan + 0j, np.complex128)
    sc = np.zeros((nports, nl, 5))
    r = np.stack([gold_pilots(rb.size, slot, l, scr, nscid)[gp] for l in dsyms])  # [nds][np]
    par = np.where(np.arange(npil) % 2, -1.0, 1.0)
    for p in range(nports):
        for grp in range((nl + 1) // 2):
            sub = (prbs[:, None] * 12 + 2 * np.arange(6)[None, :] + grp).reshape(-1)
            x = np.stack([g[p, l, sub] for l in dsyms])
            z = (x * r.conj()).sum(0) / (nds * beta)
            epre = (np.abs(x) ** 2).sum() / (npil * nds)
            pair = 2 * grp + 1 < nl
            if pair:
                s = [(z[0::2] + z[1::2]) / 2, (z[0::2] - z[1::2]) / 2]
                ma, mb = (np.repeat(v.reshape(nprb, 3).mean(1), 6) for v in s)
                resid = x - beta * r * (ma + par * mb)[None, :]
                fitted = 2
            else:
                s = [z]
                resid = x - beta * r * np.repeat(z.reshape(nprb, 6).mean(1), 6)[None, :]
                fitted = 1
            noise = (np.abs(resid) ** 2).sum() / npil * 6 / (6 * nds - fitted) if nds >= 3 else 0.001 * epre
            for k, sl in enumerate(s):
                ly = 2 * grp + k
                resp = _interpolate(sl, 4, 1 + grp, 12 * nprb) if pair else _interpolate(sl, 2, grp, 12 * nprb)
                ce[ly, p, first:, cols] = resp[:, None]
                rsrp = beta ** 2 * (np.abs(sl) ** 2).mean()
                ta = _time_alignment((sub, np.repeat(sl, 2) if pair else sl), mu)
                sc[p, ly] = (rsrp, epre, noise, (rsrp / beta ** 2) / noise if noise != 0 else 1000.0, ta)
    return ce, sc


def profile(nsc, delay, taps=2):
    """The frequency response every coefficient of the L x P matrix is multiplied with: the two taps of tests/test_chest_gpu.py, or one."""
    k = np.arange(nsc)
    if taps == 1:
        return np.exp(-2j * np.pi * k * delay / CE_DFT)
    return (0.8 + 0.3j) * np.exp(-2j * np.pi * k * delay / CE_DFT) + 0.2 * np.exp(-2j * np.pi * k * (delay + 9) / CE_DFT)


def add_dmrs(grid_ports, h, rb, dm_syms, nl, slot, scr, nscid, scaling):
    """Adds the DM-RS of every layer, through h [layer][port][nsc], to grid_ports [port][14][nsc] (the ports of h in order)."""
    prbs = np.nonzero(rb)[0]
    gp = (prbs[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
    par = np.arange(gp.size) % 2  # parity of the allocated pilot index = parity inside the PRB
    for l in dm_syms:
        pil = gold_pilots(rb.size, slot, l, scr, nscid)[gp]
        for ly in range(nl):
            sub = (prbs[:, None] * 12 + 2 * np.arange(6)[None, :] + (ly // 2) % 2).reshape(-1)
            w = np.where((ly % 2 == 1) & (par == 1), -1.0, 1.0)
            for p in range(h.shape[1]):
                grid_ports[p, l, sub] += scaling * h[ly, p, sub] * pil * w


def make_case(rng, nprb_grid, alloc, nports, nl, dm_syms, numerology=1, slot=3, scr=77, nscid=0, scaling=BETA, delay=2.0, taps=2, background=0.05, first=0, nof=14):
    """-> (case, h): a grid of background noise plus the DM-RS of nl layers; h complex128 [layer][port][nsc] is the channel."""
    rb = np.zeros(nprb_grid, np.uint8)
    rb[alloc] = 1
    sm = np.zeros(14, np.uint8)
    sm[dm_syms] = 1
    nsc = nprb_grid * 12
    hm = PL.channels(rng, nl, nports, 1)[0][:, :, 0].astype(np.complex128)
    h = hm[:, :, None] * profile(nsc, delay, taps)[None, None, :]
    g = (rng.standard_normal((nports, 14, nsc)) + 1j * rng.standard_normal((nports, 14, nsc))) * background
    add_dmrs(g, h, rb, [l for l in dm_syms if first <= l < first + nof], nl, slot, scr, nscid, scaling)
    return (numerology, slot, False, scr, nscid, np.float32(scaling), sm, rb, first, nof, nl, g.astype(np.complex64)), h


# ------------------------------------------------------------------------------------------------ grid to bytes
SLOT, SCR = 3, 77
CHAIN_CASES = [  # (layers, ports, modulation, transport block bytes, SNR dB, DM-RS symbols): 24 PRB, delay 2
    (2, 2, 4, 1497, 20.0, (2, 11)),
    (4, 4, 8, 5997, 30.0, (2, 11)),
    (2, 2, 4, 1497, 16.0, (2, 7, 11)),
    # 4001 bytes: the TS 38.214 size next to 4000 (32008 + 24 bits in four codeblocks of 1001 bytes); miphy_pusch_decode_batch refuses 4000, whose
    # codeblock payloads are not byte aligned
    (3, 4, 6, 4001, 24.0, (2, 7, 11)),
]
# the processor's one-layer PDU: one codeblock at rate 0.43. Three DM-RS symbols: with two, the forced noise variance saturates 99 % of its LLRs
# (this channel is weak: RSRP 0.2) and it does not decode at 20 dB
ONE_LAYER_CASE = (1, 2, 4, 745, 20.0, (2, 7, 11))
RETX_CASE = (2, 2, 4, 1497, 4.0, (2, 7, 11))  # rv 0 fails in the host chain at this SNR (it decodes from 6 dB on), rv 2 combined with it decodes


def chain_tx(nl, npt, mod, tb_bytes, snr_db, dmrs, rv=0, seed=None, tb=None, nprb=24, delay=2.0):
    """A transport block on nl layers, DM-RS included, through a smooth channel plus noise on every element.
    -> (c: the allocation as pusch_layers_cases.case(), tb, grid complex64 [4][14][nsc], the estimator case on the grid's first npt ports)."""
    c = PL.case("chain", nl, npt, mod, nprb_grid=nprb, prbs=range(nprb), start=0, nof=14, dmrs=dmrs, noise_var=None, seed=7 * nl + mod if seed is None else seed)
    rng = np.random.default_rng(c["seed"] + 1000 * rv)
    if tb is None:
        tb = np.random.default_rng(c["seed"]).integers(0, 256, tb_bytes, dtype=np.uint8)
    sy, scx = PL.data_positions(c)
    n = sy.size
    bits = O.o_pdsch_encode(1, rv, mod, 0, nl, n * nl, tb)
    scr = bits ^ O.o_gold((c["rnti"] << 15) + c["n_id"], 0, bits.size)
    x = O.o_modulate(mod, scr).reshape(n, nl).T.astype(np.complex128)  # layer ly carries symbols ly, L + ly, ...
    nsc = nprb * 12
    hm = PL.channels(np.random.default_rng(c["seed"]), nl, npt, 1)[0][:, :, 0].astype(np.complex128)  # (the same channel for every rv)
    h = hm[:, :, None] * profile(nsc, delay)[None, None, :]
    g = np.zeros((npt, 14, nsc), np.complex128)
    for p in range(npt):
        g[p, sy, scx] = np.einsum("ln,ln->n", h[:, p, scx], x)
    rb, dm = PL.masks(c)
    add_dmrs(g, h, rb, list(dmrs), nl, SLOT, SCR, 0, BETA)
    g += 10 ** (-snr_db / 20) * np.sqrt(0.5) * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape))
    grid = np.full((4, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    grid[:npt] = g.astype(np.complex64)
    est = (1, SLOT, False, SCR, 0, np.float32(BETA), dm, rb, 0, 14, nl, grid[:npt])
    return c, tb, grid, est


def host_llr(c, grid, est):
    """The host chain in front of the decoder: estimate() -> compact estimate and noise variance of (port 0, layer 0) -> expected_llr()."""
    ce, sc = estimate(*est)
    c = dict(c, compact=True, noise_var=float(np.float32(sc[0, 0, 2])))
    return PL.expected_llr(c, grid, ce[:, :, :1].astype(np.complex64))
