"""The SRS cases shared by tests/test_srs_ref.py (CPU) and tests/test_srs_gpu.py: every item is a UE (tests/srs_tx.py) on a grid of its own, with its
per-PRG channel, delay and noise, and the float64 receiver's answer (tests/srs_ref.py), built once.

The shapes are the smallest at which each path of the kernel can go wrong: M = 12 (4 PRB at comb 4: the table), 36 (the shortest Zadoff-Chu), 48 and
72 at comb 2 and comb 4 (sequence hopping switches on at 72) and 1632 (272 PRB at comb 2: N_ZC = 1627), crossed with 1 / 2 / 4 transmit ports, cyclic
shifts below and at or above n_cs_max / 2 (four ports on one comb and on two), 1 / 2 / 4 symbols, 1 and 4 receive ports, every PRG size the rule allows,
hopping 0 / 1 / 2 in slots 0 and 19. Delays are fractions of the unambiguous range of at most 3/4, so |phi| <= 2.5 rad and neither the device nor
the receiver is near the branch cut of atan2; tests/test_srs_ref.py asserts that, and the coverage, for every case."""
import functools

import numpy as np

import srs_ref as R
import srs_tx as X

#        nprb K nap ncs L  R prg hop slot snr_db frac   kbar nid  numerology prb start
SHAPES = [(4, 4, 1, 0, 1, 1, 1, 0, 0, None, 0.0, 0, 0, 0, 0, 13),
          (4, 4, 2, 7, 2, 4, 2, 1, 19, 20, 0.25, 3, 513, 1, 1, 8),
          (4, 4, 4, 3, 4, 1, 4, 2, 0, 30, -0.5, 1, 77, 1, 2, 10),
          (4, 4, 4, 9, 1, 4, 2, 1, 19, None, 0.75, 2, 1023, 1, 0, 0),
          (12, 4, 1, 11, 4, 4, 1, 1, 19, 10, -0.75, 3, 901, 1, 3, 9),
          (12, 4, 2, 2, 1, 1, 4, 2, 0, None, 0.5, 0, 31, 1, 0, 13),
          (12, 4, 4, 6, 2, 1, 4, 0, 7, 20, 0.25, 2, 640, 1, 1, 12),
          (8, 2, 1, 5, 2, 1, 2, 2, 19, 20, -0.25, 1, 300, 1, 2, 4),
          (8, 2, 4, 1, 1, 4, 2, 1, 0, None, 0.75, 0, 29, 1, 0, 13),
          (8, 2, 4, 4, 4, 1, 1, 0, 19, 30, 0.5, 1, 30, 1, 1, 10),
          (16, 4, 2, 0, 4, 4, 4, 2, 19, 20, -0.75, 0, 222, 1, 0, 8),
          (16, 4, 1, 6, 1, 1, 2, 1, 0, None, 0.25, 3, 59, 1, 5, 13),
          (12, 2, 1, 0, 1, 1, 1, 2, 0, 20, 0.5, 1, 5, 1, 0, 13),
          (12, 2, 2, 6, 2, 4, 4, 2, 19, None, -0.5, 0, 6, 1, 2, 12),
          (24, 4, 4, 0, 2, 1, 4, 2, 19, 20, 0.25, 2, 7, 1, 1, 2),
          (24, 4, 4, 10, 4, 4, 2, 1, 0, 30, -0.25, 1, 8, 1, 0, 10),
          (12, 2, 1, 3, 2, 1, 2, 2, 159, 25, 0.125, 0, 444, 4, 0, 6),
          (272, 2, 1, 3, 1, 1, 4, 2, 19, None, 0.75, 1, 9, 1, 2, 13),
          (272, 2, 4, 5, 4, 4, 1, 1, 0, 20, -0.75, 0, 1000, 1, 0, 10),
          (272, 2, 2, 0, 2, 1, 2, 0, 19, 30, 0.5, 1, 123, 1, 1, 11)]


def shape_ue(row):
    nprb, K, nap, ncs, L, nrx, prg, hop, slot, snr, frac, kbar, nid, num, prb, start = row
    return X.ue(R=nrx, nap=nap, start=start, nsym=L, K=K, kbar=kbar, ncs=ncs, nid=nid, hopping=hop, prg=prg, prb=prb, nprb=nprb, slot=slot, numerology=num,
                grid_nprb=prb + nprb + 1)


def make_item(seed, p, snr_db, frac):
    """One UE on a grid of its own: unit-variance channel entries, noise at snr_db below them (None: no noise), a delay of frac of the range."""
    rng = np.random.default_rng(seed)
    Hg = X.prg_channel(rng, p)
    theta = X.theta_of_delay(p, frac * R.max_delay(p))
    std = 0.0 if snr_db is None else 10 ** (-snr_db / 20)
    grid = X.build_grid(seed + 1, p["R"], p["grid_nprb"], std, [(p, Hg, theta)])
    return dict(p=p, Hg=Hg, theta=theta, snr_db=snr_db, frac=frac, grid=grid, ref=R.receive(p, grid))


@functools.lru_cache(maxsize=None)
def shapes_set():
    return [make_item(100 + 2 * i, shape_ue(row), row[9], row[10]) for i, row in enumerate(SHAPES)]


@functools.lru_cache(maxsize=None)
def multiplexed_set():
    """Five UEs without delay in one grid of 4 receive ports and 25 PRBs, symbols 12 and 13, at 25 dB, and the five jobs that receive them: two UEs
    on the two offsets of comb 2 of PRBs 0..7; two one-port UEs on one comb 4 of PRBs 8..19 at cyclic shifts n_cs_max / 2 apart, each received by a
    two-port job whose port 0 is the UE itself (its port 1 is the other one); and a UE on the adjacent PRBs 20..23. Item i: the job p, the UE tx it
    receives at port 0 (and ports 1.. of its own), that UE's channel."""
    rng = np.random.default_rng(7)
    kw = dict(R=4, start=12, nsym=2, slot=3, numerology=1, grid_nprb=25)
    a = X.ue(nap=2, K=2, kbar=0, ncs=1, nid=40, prg=2, prb=0, nprb=8, **kw)
    b = X.ue(nap=1, K=2, kbar=1, ncs=6, nid=41, prg=1, prb=0, nprb=8, hopping=1, **kw)
    c = X.ue(nap=1, K=4, kbar=2, ncs=2, nid=42, prg=2, prb=8, nprb=12, **kw)
    e = X.ue(nap=1, K=4, kbar=2, ncs=8, nid=42, prg=2, prb=8, nprb=12, **kw)
    f = X.ue(nap=1, K=4, kbar=0, ncs=0, nid=43, prg=4, prb=20, nprb=4, hopping=2, **kw)
    ues = [(p, X.prg_channel(rng, p), 0.0) for p in (a, b, c, e, f)]
    grid = X.build_grid(8, 4, 25, 10 ** (-25 / 20), ues)
    jobs = [a, b, dict(c, nap=2), dict(e, nap=2), f]
    return [dict(p=p, tx=tx, Hg=Hg, theta=theta, snr_db=25, frac=0.0, grid=grid, ref=R.receive(p, grid)) for p, (tx, Hg, theta) in zip(jobs, ues)]
