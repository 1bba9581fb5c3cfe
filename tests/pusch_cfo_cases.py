"""The DM-RS estimator that estimates and compensates a carrier frequency offset, on the host, in float64: what
miphy_dmrs_pusch_estimate_cfo_batch is held to. The arithmetic is restated from include/miphy.h:

  symbol_times()    start of the useful part of every OFDM symbol of a slot, in seconds (normal cyclic prefix)
  apply_cfo()       what an offset does to a grid in this model: one phasor per OFDM symbol
  cfo()             per-symbol fits, despreading per symbol, correlation of consecutive DM-RS symbols -> (cfo_hz, rho)
  estimate()        estimate() of tests/pusch_layers_estimator_cases.py on the derotated grid, times the phasor of every symbol
  host_llr()        the host chain in front of the decoder with the per-symbol estimate

A case is the tuple of tests/pusch_layers_estimator_cases.py."""
import numpy as np

import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

OFFSETS_HZ = (0.0, 150.0, 400.0, -1000.0)


def symbol_times(mu, slot):
    """tau_l, l = 0..13: symbol j lasts 2048 + 144 samples at 2048 * 2^mu * 15 kHz, 16 * 2^mu more where (14 slot + j) mod (7 * 2^mu) = 0."""
    cp = np.array([144 + (16 << mu if (14 * slot + j) % (7 << mu) == 0 else 0) for j in range(14)], dtype=np.int64)
    start = np.concatenate(([0], np.cumsum(cp + 2048)[:-1])) + cp
    return start / (2048.0 * 15000.0 * (1 << mu))


def apply_cfo(grid, mu, slot, f_hz, phase0=0.0):
    """grid [..][14][nsc] rotated by exp(j (phase0 + 2 pi f tau_l)) on symbol l; the dtype of the grid is kept."""
    ph = np.exp(1j * (phase0 + 2 * np.pi * f_hz * symbol_times(mu, slot)))
    return (np.asarray(grid) * ph[:, None]).astype(np.asarray(grid).dtype)


def max_gap(case):
    """The longest distance between consecutive DM-RS symbols of the allocation in seconds (0 with one DM-RS symbol)."""
    mu, slot, sm, first, nof = case[0], case[1], case[6], case[8], case[9]
    t = symbol_times(mu, slot)[[l for l in range(first, first + nof) if sm[l]]]
    return float(np.diff(t).max()) if t.size > 1 else 0.0


def cfo(mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl, g):
    """-> (cfo_hz, rho)."""
    assert not type2
    g = np.asarray(g).astype(np.complex128)
    beta = float(scaling)
    prbs = np.nonzero(rb)[0]
    dsyms = [l for l in range(first, first + nof) if sm[l]]
    if len(dsyms) < 2:
        return 0.0, 0.0
    gp = (prbs[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
    r = np.stack([E.gold_pilots(rb.size, slot, l, scr, nscid)[gp] for l in dsyms])
    tau = symbol_times(mu, slot)
    c = np.zeros(len(dsyms) - 1, np.complex128)
    e = np.zeros(len(dsyms) - 1)
    for p in range(g.shape[0]):
        for grp in range((nl + 1) // 2):
            sub = (prbs[:, None] * 12 + 2 * np.arange(6)[None, :] + grp).reshape(-1)
            z = np.stack([g[p, l, sub] for l in dsyms]) * r.conj() / beta  # [nds][np]
            layers = [(z[:, 0::2] + z[:, 1::2]) / 2, (z[:, 0::2] - z[:, 1::2]) / 2] if 2 * grp + 1 < nl else [z]
            for s in layers:
                en = (np.abs(s) ** 2).sum(1)
                c += (s[1:] * s[:-1].conj()).sum(1)
                e += np.sqrt(en[1:] * en[:-1])
    mag = np.abs(c)
    if mag.sum() == 0:
        return 0.0, 0.0
    dt = np.diff(tau[dsyms])
    return float((mag * np.angle(c) / (2 * np.pi * dt)).sum() / mag.sum()), float(mag.sum() / e.sum())


def estimate(mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl, g):
    """-> (ce complex128 [nl][ports][first + nof][nsc] per symbol, NaN where nothing is written; scalars [ports][nl][5]; cfo_hz; rho)."""
    case = (mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl)
    f, rho = cfo(*case, g)
    dsyms = [l for l in range(first, first + nof) if sm[l]]
    tau = symbol_times(mu, slot)
    ph = np.exp(2j * np.pi * f * (tau - tau[dsyms[0]]))
    ce, sc = E.estimate(*case, np.asarray(g).astype(np.complex128) * ph.conj()[None, :, None])
    return ce * ph[None, None, :first + nof, None], sc, f, rho


def host_llr(c, grid, est):
    """estimate() -> per-symbol estimate and noise variance of (port 0, layer 0) -> expected_llr(). -> (llr, cfo_hz, rho)."""
    ce, sc, f, rho = estimate(*est)
    c = dict(c, compact=False, noise_var=float(np.float32(sc[0, 0, 2])))
    return PL.expected_llr(c, grid, ce.astype(np.complex64)), f, rho


def chain_tx(case, f_hz):
    """E.chain_tx() of a chain case with the offset applied to the grid. -> (c, tb, grid complex64 [4][14][nsc], estimator case)."""
    c, tb, grid, est = E.chain_tx(*case)
    grid = apply_cfo(grid, est[0], est[1], f_hz)
    return c, tb, grid, est[:-1] + (grid[:case[1]],)
