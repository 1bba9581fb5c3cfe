"""The DM-RS estimator that follows a channel through the slot, on the host, in float64: what miphy_dmrs_pusch_estimate_tv_batch is held to. The
arithmetic is restated from include/miphy.h on top of tests/pusch_cfo_cases.py (symbol times, the offset) and
tests/pusch_layers_estimator_cases.py (pilots, frequency interpolation, time alignment):

  weights()         w[l][d] of every OFDM symbol l of the slot and every DM-RS symbol d of the allocation, INTERPOLATE or LINE
  estimate()        per-symbol fits, derotated; blended in time, interpolated in frequency, rotated back; scalars from the time mean, the noise
                    against the fit in time; the variation per (port, layer)
  apply_gains()     a per-port, per-symbol complex gain on a received grid: what a channel that changes from symbol to symbol does in this model
  linear_gains()    1 + c_p (tau_l - tau_mid): a LINE (and, between two DM-RS symbols, a polygon) follows it exactly
  two_ray_gains()   two paths per port at Doppler shifts +fd and -fd: a e^{j 2 pi fd tau} + (1 - a) e^{j (theta_p - 2 pi fd tau)}
  host_llr()        the host chain in front of the decoder with the per-symbol estimate
  chain_tx()        a chain case of tests/pusch_layers_estimator_cases.py under two_ray_gains(fd)

A case is the tuple of tests/pusch_layers_estimator_cases.py."""
import numpy as np

import pusch_cfo_cases as F
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

INTERPOLATE, LINE = 1, 2
MODES = (INTERPOLATE, LINE)


def weights(mu, slot, dsyms, mode):
    """-> float64 [14][nds]. Only differences of the symbol times enter."""
    tau = F.symbol_times(mu, slot)
    td = tau[list(dsyms)]
    nds = len(dsyms)
    w = np.zeros((14, nds))
    if nds == 1:
        w[:] = 1.0
        return w
    for l in range(14):
        if mode == INTERPOLATE:
            j = min(max(sum(1 for d in dsyms if d <= l) - 1, 0), nds - 2)
            u = (tau[l] - td[j]) / (td[j + 1] - td[j])
            w[l, j], w[l, j + 1] = 1 - u, u
        else:
            assert mode == LINE
            tm = td.mean()
            w[l] = 1.0 / nds + (tau[l] - tm) * (td - tm) / ((td - tm) ** 2).sum()
    return w


def estimate(mode, mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl, g):
    """-> (ce complex128 [nl][ports][first + nof][nsc] per symbol, NaN where nothing is written; scalars [ports][nl][5]; cfo_hz; rho;
    var float64 [ports][nl])."""
    case = (mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl)
    f, rho = F.cfo(*case, g)
    g = np.asarray(g).astype(np.complex128)
    nports, _, nsc = g.shape
    beta = float(scaling)
    prbs = np.nonzero(rb)[0]
    nprb, npil = prbs.size, prbs.size * 6
    dsyms = [l for l in range(first, first + nof) if sm[l]]
    nds = len(dsyms)
    tau = F.symbol_times(mu, slot)
    ph = np.exp(2j * np.pi * f * (tau - tau[dsyms[0]]))
    w = weights(mu, slot, dsyms, mode)
    gp = (prbs[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
    cols = (prbs[:, None] * 12 + np.arange(12)[None, :]).reshape(-1)
    r = np.stack([E.gold_pilots(rb.size, slot, l, scr, nscid)[gp] for l in dsyms])  # [nds][np]
    par = np.where(np.arange(npil) % 2, -1.0, 1.0)
    ce = np.full((nl, nports, first + nof, nsc), np.nan + 0j, np.complex128)
    sc = np.zeros((nports, nl, 5))
    var = np.zeros((nports, nl))
    fitted = nds if mode == INTERPOLATE else min(nds, 2)
    for p in range(nports):
        for grp in range((nl + 1) // 2):
            sub = (prbs[:, None] * 12 + 2 * np.arange(6)[None, :] + grp).reshape(-1)
            x = np.stack([g[p, l, sub] * ph[l].conj() for l in dsyms])  # derotated DM-RS elements [nds][np]
            z = x * r.conj() / beta
            epre = (np.abs(x) ** 2).sum() / (npil * nds)
            pair = 2 * grp + 1 < nl
            s = [(z[:, 0::2] + z[:, 1::2]) / 2, (z[:, 0::2] - z[:, 1::2]) / 2] if pair else [z]  # S_d per layer: [nds][anchors]
            fit = [w[dsyms] @ v for v in s]  # F_d
            if pair:
                ma, mb = (np.repeat(v.reshape(nds, nprb, 3).mean(2), 6, axis=1) for v in fit)
                resid = x - beta * r * (ma + par[None, :] * mb)
            else:
                resid = x - beta * r * np.repeat(fit[0].reshape(nds, nprb, 6).mean(2), 6, axis=1)
            noise = (np.abs(resid) ** 2).sum() / nprb / (6 * nds - len(s) * fitted) if nds >= 2 else 0.001 * epre
            for k, sl in enumerate(s):
                ly = 2 * grp + k
                mean = sl.mean(0)
                for l in range(first, first + nof):
                    a = w[l] @ sl
                    resp = E._interpolate(a, 4, 1 + grp, 12 * nprb) if pair else E._interpolate(a, 2, grp, 12 * nprb)
                    ce[ly, p, l, cols] = resp * ph[l]
                rsrp = beta ** 2 * (np.abs(mean) ** 2).mean()
                ta = E._time_alignment((sub, np.repeat(mean, 2) if pair else mean), mu)
                sc[p, ly] = (rsrp, epre, noise, (rsrp / beta ** 2) / noise if noise != 0 else 1000.0, ta)
                en = (np.abs(sl) ** 2).sum()
                var[p, ly] = (np.abs(sl - mean[None, :]) ** 2).sum() / en if nds >= 2 and en > 0 else 0.0
    return ce, sc, f, rho, var


def apply_gains(grid, gains):
    """grid [ports][14][nsc] times gains [ports][14] on every subcarrier; the dtype of the grid is kept. Rows of the grid beyond the gains are kept."""
    g = np.array(grid)
    gains = np.asarray(gains)
    g[:gains.shape[0]] = (g[:gains.shape[0]] * gains[:, :, None]).astype(g.dtype)
    return g


def linear_gains(mu, slot, slopes):
    """1 + c_p (tau_l - tau_mid), tau_mid half way between symbols 0 and 13; slopes in 1 / s. -> float64 [ports][14]."""
    tau = F.symbol_times(mu, slot)
    return 1.0 + np.asarray(slopes, dtype=np.float64)[:, None] * (tau - 0.5 * (tau[0] + tau[13]))[None, :]


def two_ray_gains(fd, mu, slot, nports, seed=11):
    """a_p e^{j 2 pi fd tau_l} + (1 - a_p) e^{j (theta_p - 2 pi fd tau_l)}: theta_p drawn from the seed; a_p = 0.6 on the even ports and 0.4 on the odd
    ones, so the ports turn in opposite senses and the offset estimator finds no rotation common to them. fd = 0: constant gains.
    -> complex128 [ports][14]."""
    tau = F.symbol_times(mu, slot)
    theta = np.random.default_rng(seed).uniform(0, 2 * np.pi, nports)
    a = np.where(np.arange(nports) % 2 == 0, 0.6, 0.4)
    x = 2 * np.pi * fd * tau[None, :]
    return a[:, None] * np.exp(1j * x) + (1 - a[:, None]) * np.exp(1j * (theta[:, None] - x))


def host_llr(mode, c, grid, est):
    """estimate() -> per-symbol estimate and noise variance of (port 0, layer 0) -> expected_llr(). -> (llr, cfo_hz, rho, var)."""
    ce, sc, f, rho, var = estimate(mode, *est)
    c = dict(c, compact=False, noise_var=float(np.float32(sc[0, 0, 2])))
    return PL.expected_llr(c, grid, ce.astype(np.complex64)), f, rho, var


def chain_tx(case, fd, snr_db=None):
    """E.chain_tx() of a chain case (at snr_db where given) under two_ray_gains(fd) on its ports.
    -> (c, tb, grid complex64 [4][14][nsc], estimator case)."""
    if snr_db is not None:
        case = case[:4] + (snr_db,) + case[5:]
    c, tb, grid, est = E.chain_tx(*case)
    grid = apply_gains(grid, two_ray_gains(fd, est[0], est[1], case[1]))
    return c, tb, grid, est[:-1] + (grid[:case[1]],)
