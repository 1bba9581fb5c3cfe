"""Downlink resource grids that already hold signals (CPU only: numpy + oracle_lib).

The transmit-side kernels promise to store only the resource elements they map: a slot's grid is shared by SS/PBCH blocks, PDCCH, CSI-RS
and several PDSCHs. A comparison that starts from zeros cannot see a kernel that stores 0+0j into an element it should skip, so the tests
built on this module start from background(): no element of it is zero, and every row carries -0.0, +inf and quiet NaNs with distinct
payloads. All comparisons are on the bit patterns (.view(np.uint32)). Descriptors are plain dicts, the wrappers apply the oracle to a
caller's grid [ports][14][subcarriers] in place; written_mask() derives from the oracle alone which elements a channel owns."""
import ctypes
import os

import numpy as np

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# -0.0, +inf and six quiet NaNs (exponent all ones, mantissa bit 22 set) of distinct payloads and both signs
SPECIAL_BITS = np.array([0x80000000, 0x7F800000, 0x7FC00000, 0x7FC00001, 0xFFC00002, 0x7FD5A5A5, 0x7FFFFFFF, 0xFFE00100], dtype=np.uint32)

_libm = ctypes.CDLL("libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def db_to_amplitude(x):  # convert_dB_to_amplitude (math_utils.h:101-104), single precision
    return float(_libm.powf(10.0, np.float32(x) / np.float32(20.0)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- background and written masks
def background(shape, rng):
    """complex64 array of `shape` without a zero element: both parts from +-[0.5, 2); in every row (last axis) min(8, row length) elements at
    random positions (one in each eighth of the row) carry one of SPECIAL_BITS in one of their parts; the other part stays an ordinary number."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    g = np.minimum(rng.random(shape + (2,), dtype=np.float32) * np.float32(1.5) + np.float32(0.5), np.float32(1.9999999))
    g.view(np.uint32)[...] |= rng.integers(0, 2, shape + (2,), dtype=np.uint32) << np.uint32(31)  # random signs
    n = shape[-1]
    rows = g.view(np.uint32).reshape(-1, n, 2)
    m, r = min(8, n), np.arange(rows.shape[0])[:, None]
    edges = np.arange(m + 1) * n // m
    pos = edges[:-1] + (rng.random((rows.shape[0], m)) * (edges[1:] - edges[:-1])).astype(np.int64)
    rows[r, pos, rng.integers(0, 2, pos.shape)] = SPECIAL_BITS[rng.permuted(np.tile(np.arange(8), (rows.shape[0], 1)), axis=1)[:, :m]]
    return g.view(np.complex64).reshape(shape)


def finite_copy(g, fill=0.75 - 1.25j):
    """Copy of g whose elements with a non-finite part are replaced by an ordinary value (for what has to go through arithmetic)."""
    out = g.copy()
    out[~(np.isfinite(out.real) & np.isfinite(out.imag))] = fill
    return out


def written_mask(apply, shape, rng):
    """Boolean mask of the elements that apply(grid) stores: it is run on two backgrounds that differ in every word; what comes out bit-equal
    in both was stored (and stored, not accumulated: a sum with the background would differ), everything else must still be its background."""
    b1, b2 = background(shape, rng), background(shape, rng)
    u1, u2 = bits(b1), bits(b2)
    u2[u1 == u2] ^= 1  # no word in common (the patterns stay non-zero and of their kind or become another non-zero number)
    a1, a2 = b1.copy(), b2.copy()
    apply(a1), apply(a2)
    same = (bits(a1) == bits(a2)).reshape(shape + (2,))
    mask = same.all(axis=-1)
    keep1, keep2 = (bits(a1) == bits(b1)).reshape(shape + (2,)).all(axis=-1), (bits(a2) == bits(b2)).reshape(shape + (2,)).all(axis=-1)
    assert not (same.any(axis=-1) & ~mask).any(), "an element was half written"
    assert (mask | (keep1 & keep2)).all(), "an element outside the written mask does not hold its background"
    return mask


# ---------------------------------------------------------------------------------------------- oracle wrappers (in place on grid [ports][14][nsc])
def pdsch_alloc(p):
    dm = np.zeros(14, np.uint8)
    dm[list(p["dmrs_symbols"])] = 1
    return dm, np.nonzero(p["rb"])[0]


def pdsch_data_mask(p):
    """Data REs of a PDSCH PDU as a boolean [14][nsc], straight from the descriptor (type-1 DM-RS, as the processor uses)."""
    nprb, (bs, bz) = p["rb"].size, p["bwp"]
    k, r = np.arange(12), np.arange(nprb)
    ex = np.zeros((14, nprb, 12), bool)
    for s in p["dmrs_symbols"]:
        ex[s] |= ((r >= bs) & (r < bs + bz))[:, None] & ((k % 2) < p["cdm"])[None, :]
    for (pm, rm, sm) in p["reserved"]:
        ex |= (((sm >> np.arange(14)) & 1) == 1)[:, None, None] & (np.asarray(pm) != 0)[None, :, None] & (((rm >> k) & 1) == 1)[None, None, :]
    alloc = np.zeros((14, nprb, 12), bool)
    alloc[p["start"]:p["start"] + p["nof"], p["rb"] != 0, :] = True
    return (alloc & ~ex).reshape(14, nprb * 12)


def o_pdsch_process(p, grid, parts=("data", "dmrs")):
    """pdsch_processor_impl::process on grid: o_pdsch_encode -> o_pdsch_modulate -> o_dmrs_pdsch_map with the parameters the reference processor
    derives from the PDU (pdsch_processor_impl.cpp:198-305): scaling = amplitude of minus the data ratio, DM-RS amplitude of minus the DM-RS
    ratio, type-1 DM-RS, reference point = BWP start or PRB 0. The codeword is kept in p["cw"], the number of data REs in p["nof_re"]."""
    dm, pl = pdsch_alloc(p)
    bs, bz = p["bwp"]
    nprb = p["rb"].size
    if "cw" not in p:
        p["nof_re"] = O.pdsch_nof_re(pl, p["start"], p["nof"], dm, 0, p["cdm"], bs, bz, p["reserved"])
        p["cw"] = O.o_pdsch_encode(p["bg"], p["rv"], p["mod"], p["lbrm_bytes"] * 8, 1, p["nof_re"], p["tb"])
    if "data" in parts:
        n = O.o_pdsch_modulate(p["rnti"], p["n_id"], db_to_amplitude(-p["data_dB"]), 1, [p["mod"]], [p["cw"]], p["start"], p["nof"], dm, 0, p["cdm"], bs, bz, pl,
                               p["reserved"], [p["port"]], nprb, grid)
        assert n == p["nof_re"], (n, p["nof_re"])
    if "dmrs" in parts:
        O.o_dmrs_pdsch_map(p["slot"], bs if p["ref_point_prb0"] else 0, 0, p["scr"], p["n_scid"], db_to_amplitude(-p["dmrs_dB"]), dm, p["rb"], [p["port"]], grid)
    return p["nof_re"]


def o_pdcch(p, grid):
    n = O.o_pdcch_process(p["slot"], p["rnti"], p["n_id_data"], p["n_rnti"], p["n_id_dmrs"], p["ref_point"], p["data_dB"], p["dmrs_dB"], p["payload"], p["AL"],
                          p["start"], p["dur"], p["rb"], grid[p["port"]])
    assert n == 54 * p["AL"], n


def o_ssb(p, grid):
    for port in p["ports"]:  # the same block on every port
        assert O.o_ssb_process(p["N_id"], p["ssb_idx"], p["L_max"], p["hrf"], p["sfn"], p["k_ssb"], p["payload"], p["k0"], p["l0"], p["beta"], grid.shape[2] // 12,
                               grid[port]) == 0


def o_csi_rs(p, grid):
    assert O.o_csi_rs_map(p["slot"], p["scr"], p["amp"], p["start_rb"], p["nof_rb"], p["bes"], p["row"], p["cdm"], p["dens"], p["ports"], p["rm"], p["sm"],
                          grid.shape[2] // 12, grid) == 0


# ---------------------------------------------------------------------------------------------- CSI-RS pattern fixture
def csi_rs_pattern_cases():
    """tests/golden/csi_rs_patterns.npz as a list of dicts: the case parameters and the reference's pattern (bes = PRB begin / end / stride, RE and
    symbol masks per port)."""
    g = np.load(os.path.join(GOLD, "csi_rs_patterns.npz"))
    out = []
    for m, k, rm, sm in zip(g["meta"], g["k_ref"], g["re_mask"], g["symbol_mask"]):
        slot, scr, amp, start_rb, nof_rb, b, e, st, row, cdm, dens, nports, l0 = m
        n = int(nports)
        out.append(dict(slot=int(slot), scr=int(scr), amp=float(amp), start_rb=int(start_rb), nof_rb=int(nof_rb), bes=(int(b), int(e), int(st)), row=int(row),
                        cdm=int(cdm), dens=int(dens), nports=n, l0=int(l0), k_ref=[int(x) for x in k if x >= 0], rm=rm[:n].copy(), sm=sm[:n].copy()))
    return out


def _symbols(c):
    return sorted({s for m in c["sm"] for s in range(14) if (int(m) >> s) & 1})


def _slot_jobs(cases):
    """The two CSI-RS jobs of compose_slot: a CDM job on four ports (rows 4, 5) and a row-1 job, both inside 52 PRBs and in symbols 6..13 (behind
    the CORESET and the SS/PBCH block), in different symbols. None where the cases hold no such pair."""
    for c in cases:
        if c["row"] in (4, 5) and c["start_rb"] + c["nof_rb"] <= 52 and min(_symbols(c)) >= 6:
            for r in cases:
                if r["row"] == 1 and r["dens"] == 3 and r["start_rb"] + r["nof_rb"] <= 52 and min(_symbols(r)) >= 6 and not set(_symbols(r)) & set(_symbols(c)):
                    return r, c
    return None


def csi_rs_coverage_missing(cases):
    """What a set of pattern cases lacks of: every mapping row; all four (start_rb, nof_rb) parities for both half densities of rows 2 and 3 and
    for densities one and three; the pair of jobs compose_slot needs. Empty list: covered."""
    have = {("row", c["row"]) for c in cases}
    have |= {("half", c["row"], c["dens"], c["start_rb"] & 1, c["nof_rb"] & 1) for c in cases if c["dens"] <= 1 and c["row"] in (2, 3)}
    have |= {("dens", c["dens"], c["start_rb"] & 1, c["nof_rb"] & 1) for c in cases if c["dens"] >= 2}
    want = [("row", r) for r, *_ in O.CSI_RS_ROWS]
    want += [("half", r, d, s, n) for r in (2, 3) for d in (0, 1) for s in (0, 1) for n in (0, 1)]
    want += [("dens", d, s, n) for d in (2, 3) for s in (0, 1) for n in (0, 1)]
    return [w for w in want if w not in have] + ([("slot jobs",)] if _slot_jobs(cases) is None else [])


# ---------------------------------------------------------------------------------------------- one composed slot
def _prb_mask(n, prbs):
    m = np.zeros(n, np.uint8)
    m[np.asarray(list(prbs), dtype=int)] = 1
    return m


def _csi_prbs(c):
    b, e, st = c["bes"]
    return [r for r in range(b, e, st) if c["start_rb"] <= r < c["start_rb"] + c["nof_rb"]]


def _coreset_prbs(fr, dur, cce, AL):
    """PRBs of a non-interleaved PDCCH candidate: the CORESET's PRBs are the 6-PRB groups of fr; REG r (time first) sits on PRB r // dur of them,
    CCE j holds REGs 6 j .. 6 j + 5 (TS 38.211 7.3.2.2)."""
    prbs = [6 * g + i for g in np.nonzero(fr)[0] for i in range(6)]
    return prbs[6 * cce // dur:6 * (cce + AL) // dur]


class Slot:
    pass


def compose_slot(rng, nprb, nports=4):
    """One slot's worth of descriptors on a grid [nports][14][nprb * 12] (nprb >= 52, 4 ports) and their oracle result.

    Time / frequency plan: the CORESET is symbols 0..3 of PRBs 0..29 (PDCCH on ports 0 and 1), the SS/PBCH block symbols 2..5 of 20 PRBs from
    PRB 30 up (ports 0 and 2), the CSI-RS jobs sit in symbols 6..13 (all four ports), the PDSCH DM-RS in the symbols of 6..13 that the CSI-RS
    leave free. PDSCH 0 (port 0, BWP from PRB 30) overlaps the block, PDSCH 1 (port 1) starts at symbol 3 behind its port's PDCCH, PDSCH 2
    (port 3) spans most of the grid up to its last PRBs; every PDU reserves the block and the CSI-RS elements (of all ports) inside its allocation."""
    assert nprb >= 52 and nports == 4
    s = Slot()
    s.nprb, s.nports, s.shape = nprb, nports, (nports, 14, nprb * 12)
    # SS/PBCH block: pattern case A (15 kHz), first symbol 2, k_SSB = 0 so that k0 is a multiple of 12
    ssb_prb, L_max = int(rng.integers(30, min(nprb - 20, 40) + 1)), int(rng.choice([4, 8]))
    ssb_idx, hrf = int(rng.choice([0, 2])), int(rng.integers(0, 2))
    s.ssb = [dict(N_id=int(rng.integers(0, 1008)), ssb_idx=ssb_idx, L_max=L_max, hrf=hrf, sfn=int(rng.integers(0, 1024)), k_ssb=0,
                  payload=rng.integers(0, 2, 32, dtype=np.uint8), k0=12 * ssb_prb, l0=2, beta=float(rng.choice([0.0, 3.0, -3.0])), ports=[0, 2],
                  ref=dict(numerology=0, slot=5 * hrf + ssb_idx // 2, scs_khz=15, offset_to_pointA=ssb_prb, case=0))]
    # PDCCH: non-interleaved candidates of CORESETs made of 6-PRB groups below PRB 30
    s.pdcch = []
    for (AL, dur), start, port in zip([(4, 1), (2, 2), (8, 3)], [0, 0, 1], [0, 1, 0]):
        ng = int(rng.integers(-(-AL // dur), 6))  # 6-PRB groups of the CORESET (dur CCEs each), the first one always set, the others anywhere below PRB 30
        fr = np.zeros(5, np.uint8)
        fr[0] = 1
        fr[1 + rng.choice(4, ng - 1, replace=False)] = 1
        cce = AL * int(rng.integers(0, ng * dur // AL))
        A = int(rng.integers(12, min(129, 108 * AL - 24)))
        s.pdcch.append(dict(slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65536)), n_id_data=int(rng.integers(0, 65536)), n_rnti=int(rng.integers(0, 65536)),
                            n_id_dmrs=int(rng.integers(0, 65536)), ref_point=0, data_dB=float(rng.choice([0.0, -3.0, 1.5])), dmrs_dB=float(rng.choice([0.0, 3.0])),
                            payload=rng.integers(0, 2, A, dtype=np.uint8), AL=AL, start=start, dur=dur, rb=_prb_mask(nprb, _coreset_prbs(fr, dur, cce, AL)), port=port,
                            coreset=dict(mapping=1, bwp_start=0, bwp_size=30, fr=fr, reg_bundle=6, interleaver=2, shift=0, cce=cce)))
    # CSI-RS: a row-1 job (density three) on one port and a CDM job on four, both from the pattern fixture, port lists that are not the identity
    row1, cdm4 = _slot_jobs(csi_rs_pattern_cases())
    s.csi = [dict(row1, ports=[2]), dict(cdm4, ports=[2, 0, 3, 1])]
    csi_syms = set(_symbols(row1)) | set(_symbols(cdm4))
    free = [x for x in range(6, 14) if x not in csi_syms]
    # reserved RE patterns: the block, then per CSI-RS job one pattern per distinct symbol mask (the union of the ports' RE masks)
    res_all = [(_prb_mask(nprb, range(ssb_prb, ssb_prb + 20)), 0xFFF, 0xF << 2)]
    for c in s.csi:
        for m in sorted({int(x) for x in c["sm"]}):
            res_all.append((_prb_mask(nprb, _csi_prbs(c)), int(np.bitwise_or.reduce([int(r) for r, x in zip(c["rm"], c["sm"]) if int(x) == m])), m))
    assert len(res_all) <= 4
    hi0 = max(5, nprb - 245)
    plan = [  # mod, bg, rv, port, bwp, PRBs, start, nof, DM-RS symbols, CDM groups, PRB-0 reference, LBRM bytes, code rate
        (2, 2, 0, 0, (30, nprb - 30), range(32, min(nprb - 1, 92)), int(rng.integers(0, 2)), None, 1, 2, 1, 1200, 0.25),
        (6, 1, 2, 1, (0, nprb), range(2, 28), 3, 11, 2, 2, 0, 3168, 0.5),
        (8, 1, 3, 3, (0, nprb), range(hi0, nprb - 2), 0, 14, 3, 1, 0, 3168, 0.7)]
    s.pdsch = []
    for mod, bg, rv, port, bwp, prbs, start, nof, ndm, cdm, prb0, lbrm, rate in plan:
        nof = 14 - start if nof is None else nof
        rb = _prb_mask(nprb, prbs)
        reserved = [(pm & rb, rm, sm) for (pm, rm, sm) in res_all if (pm & rb).any() and any((sm >> x) & 1 for x in range(start, start + nof))]
        p = dict(bg=bg, mod=mod, rv=rv, port=port, bwp=bwp, rb=rb, start=start, nof=nof, dmrs_symbols=tuple(sorted(int(x) for x in rng.choice(free, ndm, replace=False))),
                 cdm=cdm, ref_point_prb0=prb0, lbrm_bytes=lbrm, reserved=reserved, slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65536)),
                 n_id=int(rng.integers(0, 1024)), scr=int(rng.integers(0, 65536)), n_scid=int(rng.integers(0, 2)), dmrs_dB=float(rng.choice([0.0, -3.0, 3.0])),
                 data_dB=float(rng.choice([0.0, 2.0, -1.5])))
        p["tb"] = rng.integers(0, 256, max(8, int(pdsch_data_mask(p).sum() * mod * rate) // 8), dtype=np.uint8)
        s.pdsch.append(p)
    s.channels = ([("ssb", p, o_ssb) for p in s.ssb] + [("pdcch%d" % i, p, o_pdcch) for i, p in enumerate(s.pdcch)]
                  + [("csi%d" % i, p, o_csi_rs) for i, p in enumerate(s.csi)] + [("pdsch%d" % i, p, o_pdsch_process) for i, p in enumerate(s.pdsch)])
    s.background = background(s.shape, rng)
    s.expected = s.background.copy()
    apply_channels(s, s.expected)
    s.masks = {name: written_mask(lambda g, p=p, fn=fn: fn(p, g), s.shape, rng) for name, p, fn in s.channels}
    return s


def apply_channels(s, grid, order=None):
    for i in (range(len(s.channels)) if order is None else order):
        name, p, fn = s.channels[i]
        fn(p, grid)
    return grid
