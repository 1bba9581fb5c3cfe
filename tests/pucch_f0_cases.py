"""The PDUs of tests/test_pucch_f0_gpu.py, built once per process with the transmitter of tests/pucch_f0_tx.py, and what the float64 receiver of
tests/pucch_f0_ref.py makes of them (reference(), computed once per set and shared); tests/test_pucch_f0_tx.py checks those outcomes on the CPU.
An item is a dict: pdu, hyp (index of the hypothesis sent, None for nothing), grid ([4][14][12 GRID_NPRB] complex64, shared by the PDUs packed
into it)."""
import functools

import numpy as np

import pucch_f0_ref as R
import pucch_f0_tx as X

GRID_NPRB = 20
GRID_PORTS = 4
NOISE_20DB = 0.1
UCI = ((1, 0), (2, 0), (0, 1), (1, 1), (2, 1))  # (nof_harq_ack, nof_sr)
SHAPES = ((1, 0), (2, 0), (2, 1))  # (symbols, hopping)
NIDS = (0, 29, 30, 411, 777, 1023)  # few identities and slots: the numpy Gold sequence is a Python loop per (identity, length)
SLOTS = {0: (0, 3, 9), 1: (5, 12, 19)}
SEED_SHAPES, SEED_NOISE = 5100, 9400  # tests/test_pucch_f0_tx.py holds the sets built from them to what the GPU tests rely on


class Packer:
    """Places one-PRB PDUs of one or two symbols side by side on grids of GRID_NPRB PRBs, a new grid when one is full."""

    def __init__(self):
        self.used, self.pdus, self.hyps = [], [], []

    def place(self, p, hyp):
        for g in range(len(self.used) + 1):
            if g == len(self.used):
                self.used.append(np.zeros((14, GRID_NPRB), bool)), self.pdus.append([]), self.hyps.append([])
            u = self.used[g]
            s = p["start"]
            first = np.flatnonzero(~u[s] & ~u[s + 1]) if p["nsym"] == 2 and not p["hop"] else np.flatnonzero(~u[s])
            if first.size == 0:
                continue
            prb = prb2 = int(first[0])
            if p["hop"]:  # the second symbol on the highest PRB that is free there
                second = np.flatnonzero(~u[s + 1])
                second = second[second != prb]
                if second.size == 0:
                    continue
                prb2 = int(second[-1])
            u[s, prb] = True
            if p["nsym"] == 2:
                u[s + 1, prb2] = True
            p["prb"], p["prb2"] = prb, prb2 if p["hop"] else 0
            self.pdus[g].append(p), self.hyps[g].append(hyp)
            return g

    def items(self, seed, noise_std):
        out = []
        for g, (pdus, hyps) in enumerate(zip(self.pdus, self.hyps)):
            grid = X.build_grid(seed + g, GRID_PORTS, GRID_NPRB, noise_std, pdus, hyps)
            out += [dict(pdu=p, hyp=h, grid=grid, order=p["order"]) for p, h in zip(pdus, hyps)]
        out.sort(key=lambda d: d["order"])  # the order the PDUs were made in
        return out


def _neighbours(ics, which):
    """used_shifts_mask of neighbours that leaves at least two shifts free next to any set of hypotheses of this PDU."""
    return sum(1 << ((ics + o) % 12) for o in ((), (5,), (5, 11), (2, 5))[which % 4])


@functools.lru_cache(maxsize=None)
def shapes_set():
    """Every port count with every (symbols, hopping), every (HARQ-ACK, SR) and every hypothesis sent, nothing sent included, at 20 dB; the initial
    shift, the start symbol (13 and 12 included), numerology, slot, identity, neighbours' shifts, a known noise variance and an own threshold go round."""
    pk, i = Packer(), 0
    for nports in (1, 2, 3, 4):
        for nsym, hop in SHAPES:
            for nharq, nsr in UCI:
                for hyp in list(range(len(X.hypotheses_mcs(nharq, nsr)))) + [None]:
                    num = i % 2
                    p = X.pdu(nports, nsym, hop, start=((13, 0, 6) if nsym == 1 else (12, 0, 7))[i % 3], ics=i % 12, nharq=nharq, nsr=nsr,
                              mask=_neighbours(i % 12, i // 3), nid=NIDS[i % len(NIDS)], slot=SLOTS[num][(i // 2) % 3], numerology=num, grid_nprb=GRID_NPRB,
                              threshold=3.0 if i % 7 == 3 else 0.0, noise_var=NOISE_20DB ** 2 if i % 5 == 2 else 0.0)
                    p["order"] = i
                    pk.place(p, hyp)
                    i += 1
    return pk.items(SEED_SHAPES, NOISE_20DB)


@functools.lru_cache(maxsize=None)
def multiplexed(kind):
    """UEs that share one PRB through their cyclic shifts, one HARQ-ACK bit each, two ports and two symbols at 20 dB: 'three' (six shifts free), 'six'
    (every shift occupied, the noise variance given) and 'power' (two UEs 10 dB apart)."""
    ics, hyps, gains, nv = {"three": ((0, 1, 2), (1, 0, 1), None, 0.0), "six": (tuple(range(6)), (0, 1, 1, 0, 1, 0), None, NOISE_20DB ** 2),
                            "power": ((0, 3), (1, 1), (0.0, -10.0), 0.0)}[kind]
    mask = sum((1 << s) | (1 << (s + 6)) for s in ics)
    pdus = [X.pdu(2, 2, 0, start=4, prb=7, ics=s, nharq=1, mask=mask, nid=411, slot=12, numerology=1, grid_nprb=GRID_NPRB, noise_var=nv) for s in ics]
    grid = X.build_grid(70 + len(ics), GRID_PORTS, GRID_NPRB, NOISE_20DB, pdus, hyps, gains)
    return [dict(pdu=p, hyp=h, grid=grid) for p, h in zip(pdus, hyps)]


NOISE_PDUS = 4096


@functools.lru_cache(maxsize=None)
def noise_set():
    """4096 PDUs on grids of unit-variance noise, nothing sent: (D, F, H) spread over ports 1..4, one and two symbols, every (HARQ-ACK, SR), masks that
    leave 1 to 11 shifts free, and every fourth PDU with the noise variance given (every shift occupied among them)."""
    rng = np.random.default_rng(SEED_NOISE)
    pk = Packer()
    for i in range(NOISE_PDUS):
        nharq, nsr = UCI[i % 5]
        nsym, hop = SHAPES[(i // 5) % 3]
        num = i % 2
        known = i % 4 == 1
        mask = int(rng.integers(0, 4096)) & int(rng.integers(0, 4096)) if i % 3 else int(rng.integers(0, 4096))
        p = X.pdu(1 + (i // 15) % 4, nsym, hop, start=int(rng.integers(0, 15 - nsym)), ics=int(rng.integers(0, 12)), nharq=nharq, nsr=nsr, mask=mask,
                  nid=NIDS[int(rng.integers(0, len(NIDS)))], slot=SLOTS[num][int(rng.integers(0, 3))], numerology=num, grid_nprb=GRID_NPRB,
                  noise_var=1.0 if known else 0.0)
        if known and i % 8 == 1:
            p["mask"] = 0xfff
        while not known and R.free_mask(p) == 0:
            p["mask"] &= int(rng.integers(0, 4096))
        p["order"] = i
        pk.place(p, None)
    return pk.items(SEED_NOISE, 1.0)


@functools.lru_cache(maxsize=None)
def mixed_items():
    """PDUs of different shapes, port counts and UCI side by side on one four-port grid at 20 dB."""
    rows = ((1, 1, 0, 13, 1, 0, 0), (4, 2, 1, 12, 2, 1, 5), (2, 2, 0, 0, 0, 1, 0), (3, 1, 0, 0, 2, 0, 3), (4, 2, 0, 5, 1, 1, 2), (2, 1, 0, 7, 2, 1, None),
            (1, 2, 1, 8, 1, 0, 1), (3, 2, 1, 2, 0, 1, None))
    pk = Packer()
    for i, (nports, nsym, hop, start, nharq, nsr, hyp) in enumerate(rows):
        p = X.pdu(nports, nsym, hop, start=start, ics=(5 * i) % 12, nharq=nharq, nsr=nsr, mask=_neighbours((5 * i) % 12, i), nid=NIDS[i % len(NIDS)], slot=9,
                  numerology=i % 2, grid_nprb=GRID_NPRB, noise_var=NOISE_20DB ** 2 if i == 4 else 0.0)
        p["order"] = i
        assert pk.place(p, hyp) == 0
    return pk.items(88, NOISE_20DB)


SETS = {"shapes": shapes_set, "three": lambda: multiplexed("three"), "six": lambda: multiplexed("six"), "power": lambda: multiplexed("power"),
        "noise": noise_set, "mixed": mixed_items}
DETERMINISTIC = ("shapes", "three", "six", "power", "mixed")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 receiver's outcome of every item of a set, in item order."""
    return [R.detect(d["pdu"], d["grid"]) for d in SETS[name]()]
