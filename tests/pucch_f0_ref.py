"""PUCCH format 0 receiver in numpy float64: the arithmetic stated at the top of csrc/pucch_f0.hip, the closed-form thresholds included.
miphy_pucch_process_f0_batch and miphy_pucch_f0_info are checked against it; tests/test_pucch_f0_tx.py checks it against the transmitter of
tests/pucch_f0_tx.py and the thresholds against direct draws of the statistic."""
import functools
import math

import numpy as np

import pucch_f0_tx as X
import pucch_tx as T

VALID, INVALID = 1, 2  # MIPHY_UCI_STATUS_*
P_FALSE_ALARM = 0.01


def hypotheses(p):
    """Unhopped cyclic shift of every hypothesis, in table order."""
    return [(p["ics"] + m) % 12 for m in X.hypotheses_mcs(p["nharq"], p["nsr"])]


def free_mask(p):
    occupied = p["mask"]
    for k in hypotheses(p):
        occupied |= 1 << k
    return ~occupied & 0xfff


def _bisect(tail, lo, hi, q):
    for _ in range(100):  # the tail falls from 1 to 0
        mid = 0.5 * (lo + hi)
        if tail(mid) > q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def default_threshold(D, F, H, known):
    """The threshold on the metric at a false-alarm probability of 1 % per PDU, union bound over the H hypotheses. Estimated noise: S / (S + N) is
    Beta(D, F D) on noise alone; known noise: D metric is Gamma(D)."""
    q = P_FALSE_ALARM / H
    if known:
        def tail(t):
            term, s = math.exp(-t), 0.0
            for j in range(D):
                s += term
                term *= t / (j + 1)
            return s
        return _bisect(tail, 0.0, 200.0, q) / D
    n = D + F * D - 1

    def tail(x):
        term, s = (1.0 - x) ** n, 0.0
        for j in range(D):
            s += term
            term *= (n - j) / (j + 1) * (x / (1.0 - x))
        return s
    x = _bisect(tail, 0.0, 1.0, q)
    return F * x / (1.0 - x)


def threshold_of(p):
    """What the call compares the metric with: the job's own threshold, or the default as the float the job record carries."""
    if p["threshold"] > 0:
        return float(np.float32(p["threshold"]))
    D, F, H = p["nports"] * p["nsym"], bin(free_mask(p)).count("1"), len(hypotheses(p))
    return float(np.float32(default_threshold(D, F, H, p["noise_var"] > 0)))


def energies(p, grid):
    """E[k'], k' < 12: the unhopped shift energies, summed over ports (outer) and symbols (inner)."""
    r = X.base_sequence(p["nid"] % 30)
    E = np.zeros(12)
    for port in range(p["nports"]):
        for l, prb in enumerate(X.hop_prbs(p)):
            y = grid[port, p["start"] + l, 12 * prb:12 * prb + 12].astype(np.complex128)
            c = np.fft.fft(y * np.conj(r)) / 12
            n_cs = T.alpha_index(p["nid"], p["slot"], p["start"] + l, 0)
            E += np.roll(np.abs(c) ** 2, -n_cs)
    return E


def detect(p, grid):
    """Everything the device writes for one PDU, and how far the decision is from flipping: `gap` = relative distance of the best hypothesis' energy
    from the second best (1 with a single hypothesis), `edge` = relative distance of the metric from the threshold."""
    E = energies(p, grid)
    hyp = hypotheses(p)
    D = p["nports"] * p["nsym"]
    eh = np.array([E[k] for k in hyp])
    best = int(np.argmax(eh))  # the first of the largest
    S = eh[best]
    fm = free_mask(p)
    free = [k for k in range(12) if (fm >> k) & 1]
    nv = float(np.float32(p["noise_var"]))
    sigma2 = nv if nv > 0 else 12 * sum(E[k] for k in free) / (len(free) * D)
    metric = 12 * S / (D * sigma2)
    thr = threshold_of(p)
    valid = metric >= thr
    bits = X.hypothesis_bits(p["nharq"], p["nsr"], best)
    if p["nharq"] == 0:
        bits = [int(valid)]
    others = np.delete(eh, best)
    gap = 1.0 if others.size == 0 else (S - others.max()) / S
    return dict(E=E, best=best, bits=np.array(bits, np.uint8), status=VALID if valid else INVALID, metric=metric, threshold=thr,
                detection_metric=metric / thr, epre_db=10 * math.log10(E.sum() / D), rsrp_db=10 * math.log10(S / D),
                sinr_db=10 * math.log10(S / D / sigma2), gap=gap, edge=abs(metric - thr) / thr)


def near(r):
    """The verdict or the choice may flip in single precision."""
    return r["gap"] <= 1e-3 or r["edge"] <= 1e-3
