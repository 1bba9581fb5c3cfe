"""GPU: the downlink mapping kernels on grids that already hold signals. Every device buffer starts as dl_grid.background() (no zero element;
-0.0, +inf and quiet NaNs in every row), with guard elements before (5), between (3) and after (7) the jobs' grids, and must come back
bit-equal to the same buffer with the oracle applied -- the whole buffer: guards, ports and symbols no job names, DM-RS positions of other
CDM groups, reserved REs, PRBs below a reference point, CORESET symbols beyond the duration, the subcarriers next to PSS / SSS. A kernel that
stores anything, 0+0j included, into an element it does not own fails here; from a zero grid it passes."""
import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O
from test_ofdm_gpu import TOL, rel_err
from test_pdsch_mod_gpu import _mod_job, _words

pytestmark = pytest.mark.gpu


class Buffer:
    """Flat complex64 buffer: 5 guard elements, the grids (3 guard elements between two of them), 7 guard elements; all from background()."""

    def __init__(self, shapes, rng):
        parts, self.offsets, self.shapes, off = [D.background(5, rng)], [], [tuple(s) for s in shapes], 5
        for i, sh in enumerate(self.shapes):
            if i:
                parts.append(D.background(3, rng))
                off += 3
            self.offsets.append(off)
            parts.append(D.background(sh, rng).reshape(-1))
            off += parts[-1].size
        parts.append(D.background(7, rng))
        self.start = np.concatenate(parts)
        self.want = self.start.copy()

    def grid(self, i):
        """View of grid i of the expected buffer (the oracle wrappers work on it in place)."""
        o, sh = self.offsets[i], self.shapes[i]
        return self.want[o:o + int(np.prod(sh))].reshape(sh)

    def device(self):
        import torch
        return torch.from_numpy(self.start.copy()).cuda()

    def check(self, got_d, what=""):
        import torch
        torch.cuda.synchronize()
        got = got_d.cpu().numpy()
        bad = np.nonzero((D.bits(got) != D.bits(self.want)).reshape(-1, 2).any(axis=1))[0]
        if bad.size:
            where = []
            for e in bad[:4]:
                i = int(np.searchsorted(self.offsets, e, side="right")) - 1
                pos = np.unravel_index(int(e) - self.offsets[i], self.shapes[i]) if i >= 0 and e - self.offsets[i] < np.prod(self.shapes[i]) else "guard"
                where.append((int(e), i, pos, got[e], self.want[e], "background" if D.bits(self.want[e:e + 1]).tolist() == D.bits(self.start[e:e + 1]).tolist() else "mapped"))
            raise AssertionError("%s: %d elements differ; first (element, grid, position, got, want, kind): %s" % (what, bad.size, where))


def _jobs_arg(jobs, on_device):
    import torch
    return torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs


def _reserved(rng, nprb, n, syms=None):
    out = []
    for r in range(n):
        sm = int(rng.integers(1, 1 << 14))
        if syms is not None and r == 0:
            sm |= sum(1 << s for s in syms)  # at least one pattern overlaps the DM-RS symbols
        out.append(((rng.uniform(size=nprb) < 0.4).astype(np.uint8), int(rng.integers(1, 4096)), sm))
    return out


# ------------------------------------------------------------------------------------------------------------------- a. PDSCH modulator
# mod, codeword offset modulo 8, DM-RS type 2, CDM groups, reserved patterns, (start, nof), DM-RS symbols, port, bwp, PRB range the allocation is drawn from,
# scaling. Aligned 16QAM / 256QAM codewords take the kernel's two-sweep path, offset 3 its element loop (byte-wise bits); QPSK / 64QAM have an even
# (16-bit loads) and an odd start; type 2 with three CDM groups leaves no data in the DM-RS symbol (the symbol's workgroup returns early).
MOD_JOBS = [
    (1, 0, 0, 2, 0, (0, 14), (2,), 0, (0, 30), (0, 30), 1.0),
    (2, 0, 1, 1, 1, (2, 10), (3,), 1, (0, 30), (2, 28), 0.5),
    (2, 5, 0, 1, 2, (0, 14), (2, 11), 2, (4, 20), (0, 30), float("inf")),
    (4, 0, 0, 2, 3, (0, 14), (2, 7), 0, (0, 30), (3, 27), float("inf")),
    (4, 3, 1, 3, 0, (1, 9), (2,), 1, (0, 30), (0, 30), 1.0),
    (6, 2, 1, 2, 4, (0, 14), (2, 3), 2, (0, 30), (1, 29), 0.5),
    (6, 7, 0, 2, 1, (2, 10), (4,), 0, (0, 30), (0, 30), 1.0),
    (8, 0, 1, 3, 2, (0, 14), (2,), 1, (0, 30), (0, 30), 1.0),
    (8, 3, 0, 1, 1, (1, 9), (3, 8), 2, (0, 30), (5, 25), 0.5),
    (8, 0, 0, 2, 4, (0, 14), (2, 11), 0, (6, 18), (1, 29), 0.5),
    (4, 4, 1, 1, 1, (2, 10), (2,), 1, (0, 30), (0, 30), 1.0),
    (1, 1, 1, 2, 2, (0, 14), (2, 9), 2, (0, 30), (4, 26), float("inf")),
]


@pytest.fixture(scope="module")
def mod_case():
    return _build_mod_case()


def _build_mod_case():
    import miphy
    rng = np.random.default_rng(701)
    shapes = [(3, 14, 30 * 12)] * len(MOD_JOBS) + [(1, 14, 275 * 12)]
    buf = Buffer(shapes, rng)
    specs = []
    for (mod, cwo, type2, cdm, nres, (start, nof), dsyms, port, bwp, (p0, p1), scaling) in MOD_JOBS:
        rb = np.zeros(30, np.uint8)
        rb[p0:p1] = rng.uniform(size=p1 - p0) < 0.7
        rb[[p0, p1 - 1]] = 1
        specs.append((mod, cwo, type2, cdm, _reserved(rng, 30, nres, dsyms), start, nof, dsyms, port, bwp, rb, scaling))
    rb = np.zeros(275, np.uint8)  # PRBs in all five words of the mask, a single PRB in bit 274
    for a, b in ((3, 11), (60, 71), (128, 136), (190, 201), (274, 275)):
        rb[a:b] = 1
    specs.append((8, 0, 0, 2, _reserved(rng, 275, 2, (2,)), 0, 14, (2,), 0, (0, 275), rb, 1.0))
    jobs, cws, cw_off = [], [], 0
    for i, (mod, cwo, type2, cdm, reserved, start, nof, dsyms, port, (bs, bz), rb, scaling) in enumerate(specs):
        dm = np.zeros(14, np.uint8)
        dm[list(dsyms)] = 1
        pl = np.nonzero(rb)[0]
        pad = (cwo - cw_off) % 8
        cws.append(rng.integers(0, 2, pad, dtype=np.uint8))
        cw_off += pad
        nre = O.pdsch_nof_re(pl, start, nof, dm, type2, cdm, bs, bz, reserved)
        cw = rng.integers(0, 2, nre * mod, dtype=np.uint8)
        rnti, n_id = int(rng.integers(1, 65536)), int(rng.integers(0, 1024))
        assert O.o_pdsch_modulate(rnti, n_id, scaling, 1, [mod], [cw], start, nof, dm, type2, cdm, bs, bz, pl, reserved, [port], rb.size, buf.grid(i)) == nre
        j = _mod_job(miphy, rnti, n_id, scaling, mod, port, start, nof, dm, type2, cdm, bs, bz, pl, reserved, rb.size, cw_off=cw_off, grid_off=buf.offsets[i])
        assert j["nof_bits"] == cw.size and cw_off % 8 == cwo
        if type2 and cdm == 3:  # no data RE in a DM-RS symbol
            assert O.pdsch_nof_re(pl, dsyms[0], 1, dm, type2, cdm, bs, bz, reserved) == 0
        jobs.append(j)
        cws.append(cw)
        cw_off += cw.size
    return buf, np.array(jobs, dtype=miphy.PdschModJob), np.concatenate(cws + [np.zeros(16, np.uint8)])


@pytest.mark.parametrize("on_device", [False, True])
def test_pdsch_modulator_on_a_background(ctx, mod_case, on_device):
    import torch
    buf, jobs, cw = mod_case
    n = len(MOD_JOBS)
    assert {int(j["mod"]) for j in jobs} == {1, 2, 4, 6, 8} and (buf.want != buf.start).any()
    gd, cw_d = buf.device(), torch.from_numpy(cw).cuda()
    ctx.pdsch_modulate_batch(_jobs_arg(jobs[:n], on_device), cw_d, gd)   # the batch of 30-PRB grids
    ctx.pdsch_modulate_batch(_jobs_arg(jobs[n:], on_device), cw_d, gd)   # the 275-PRB job
    buf.check(gd, "pdsch_modulate_batch")


# ------------------------------------------------------------------------------------------------------------------- b. PDSCH DM-RS
# DM-RS type 2, ports of the job, ports of the grid, symbols, reference point, first allocated PRB, grid PRBs
DMRS_JOBS = [
    (0, 1, 3, (2,), 0, 0, 24),
    (0, 4, 5, (2, 3), 0, 4, 24),
    (0, 8, 8, (2, 3, 10, 11), 5, 2, 24),      # PRBs 2..4 are allocated but lie below the reference point: they keep the background
    (1, 12, 12, (2, 3), 7, 3, 24),
    (1, 4, 6, (0, 5, 13), 3, 3, 24),
    (0, 2, 2, (3, 4), 9, 0, 275),
]


@pytest.fixture(scope="module")
def dmrs_case():
    return _build_dmrs_case()


def _build_dmrs_case():
    import miphy
    rng = np.random.default_rng(702)
    buf = Buffer([(gp, 14, nprb * 12) for (_, _, gp, _, _, _, nprb) in DMRS_JOBS], rng)
    jobs = np.zeros(len(DMRS_JOBS), dtype=miphy.DmrsPdschJob)
    for i, (type2, nports, gp, syms, ref, first, nprb) in enumerate(DMRS_JOBS):
        rb = (rng.uniform(size=nprb) < 0.6).astype(np.uint8)
        rb[:first] = 0
        rb[[first, nprb - 1]] = 1
        ports = rng.permutation(gp)[:nports]
        while nports > 1 and np.array_equal(ports, np.arange(nports)):
            ports = rng.permutation(gp)[:nports]
        if nports == 1:
            ports = np.array([gp - 1])
        sm = np.zeros(14, np.uint8)
        sm[list(syms)] = 1
        slot, scr, nscid, amp = int(rng.integers(0, 20)), int(rng.integers(0, 65536)), int(rng.integers(0, 2)), float(rng.choice([1.0, 1.4125375, 0.7071]))
        assert O.o_dmrs_pdsch_map(slot, ref, type2, scr, nscid, amp, sm, rb, ports, buf.grid(i)) == 0
        j = jobs[i]
        j["slot_in_frame"], j["reference_point_k_rb"], j["scrambling_id"], j["amplitude"] = slot, ref, scr, amp
        j["dmrs_type"], j["n_scid"], j["nof_ports"] = 2 if type2 else 1, nscid, nports
        j["ports"][:nports] = ports
        j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"], j["grid_offset"] = sum(1 << s for s in syms), nprb, _words(rb), buf.offsets[i]
        if first < ref:  # the PRBs below the reference point hold the background in the expectation
            o, w = buf.offsets[i], buf.grid(i)
            assert np.array_equal(D.bits(w[:, :, :ref * 12]), D.bits(buf.start[o:o + w.size].reshape(w.shape)[:, :, :ref * 12]))
    return buf, jobs


@pytest.mark.parametrize("on_device", [False, True])
def test_pdsch_dmrs_on_a_background(ctx, dmrs_case, on_device):
    buf, jobs = dmrs_case
    gd = buf.device()
    ctx.dmrs_pdsch_map_batch(_jobs_arg(jobs, on_device), gd)
    buf.check(gd, "dmrs_pdsch_map_batch")


# ------------------------------------------------------------------------------------------------------------------- c. PDSCH processor and plan
def _pdsch_pdus(miphy, pdus, grid_offsets):
    """PdschPdu records of dl_grid PDSCH dicts -> (records, transport-block buffer)."""
    out = np.zeros(len(pdus), dtype=miphy.PdschPdu)
    tbs, tb_off = [], 0
    for q, p, go in zip(out, pdus, grid_offsets):
        q["slot_in_frame"], q["rnti"], q["n_id"], q["dmrs_scrambling_id"], q["tbs_lbrm_bytes"], q["tb_bytes"] = p["slot"], p["rnti"], p["n_id"], p["scr"], p["lbrm_bytes"], p["tb"].size
        q["ratio_pdsch_dmrs_to_sss_dB"], q["ratio_pdsch_data_to_sss_dB"] = p["dmrs_dB"], p["data_dB"]
        q["bg"], q["rv"], q["mod"], q["port"], q["start_symbol"], q["nof_symbols"] = p["bg"], p["rv"], p["mod"], p["port"], p["start"], p["nof"]
        q["nof_cdm_groups_without_data"], q["n_scid"], q["ref_point_prb0"], q["nof_reserved"] = p["cdm"], p["n_scid"], p["ref_point_prb0"], len(p["reserved"])
        q["dmrs_symbols_mask"] = sum(1 << s for s in p["dmrs_symbols"])
        q["grid_nof_prb"], q["bwp_start_rb"], q["bwp_size_rb"], q["rb_mask"] = p["rb"].size, p["bwp"][0], p["bwp"][1], _words(p["rb"])
        for r, (pm, rm, sm) in enumerate(p["reserved"]):
            q["reserved"][r]["prb_mask"], q["reserved"][r]["re_mask"], q["reserved"][r]["symbols"] = _words(pm), rm, sm
        q["tb_offset"], q["grid_offset"] = tb_off, go
        tbs.append(np.concatenate([p["tb"], np.zeros(-p["tb"].size % 16, np.uint8)]))
        tb_off += tbs[-1].size
    return out, np.concatenate(tbs)


def _single_prb_pdu(rng, prb, mod, cdm, tb_bytes):
    rb = np.zeros(25, np.uint8)
    rb[prb] = 1
    return dict(bg=2, mod=mod, rv=0, port=0, bwp=(0, 25), rb=rb, start=0, nof=14, dmrs_symbols=(2,), cdm=cdm, ref_point_prb0=0, lbrm_bytes=400, reserved=[],
                slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), scr=int(rng.integers(0, 65536)), n_scid=1,
                dmrs_dB=0.0, data_dB=-3.0, tb=rng.integers(0, 256, tb_bytes, dtype=np.uint8))


def test_pdsch_processor_and_plan_on_a_background(ctx):
    import torch
    import miphy
    rng = np.random.default_rng(703)
    s = D.compose_slot(rng, 52, 4)
    singles = [_single_prb_pdu(rng, 0, 4, 2, 20), _single_prb_pdu(rng, 24, 1, 1, 8)]  # (two CDM groups of type 1: no data RE in the DM-RS symbol)
    buf = Buffer([s.shape, (1, 14, 300), (1, 14, 300)], rng)
    pdus = s.pdsch + singles
    where = [0, 0, 0, 1, 2]
    for p, g in zip(pdus, where):
        D.o_pdsch_process(p, buf.grid(g))
    rec, tb = _pdsch_pdus(miphy, pdus, [buf.offsets[g] for g in where])
    for q, p in zip(rec, pdus):
        assert miphy.pdsch_pdu_nof_re(q) == p["nof_re"]
    tb_d = torch.from_numpy(tb).cuda()
    gd = buf.device()
    ctx.pdsch_process_batch(rec, tb_d, gd)
    buf.check(gd, "pdsch_process_batch")
    plan = miphy.PdschProcessPlan(ctx, rec)
    try:
        for run in range(2):
            gd = buf.device()
            plan.run(tb_d, gd)
            buf.check(gd, "PdschProcessPlan.run %d" % run)
    finally:
        torch.cuda.synchronize()
        plan.close()


# ------------------------------------------------------------------------------------------------------------------- d. PDCCH
def test_pdcch_on_a_background(ctx):
    import torch
    import miphy
    from test_pdcch_proc_gpu import _pdu
    rng = np.random.default_rng(704)
    sizes = [24, 106]
    buf = Buffer([(3, 14, n * 12) for n in sizes], rng)
    used = [np.zeros((3, 14, n), bool) for n in sizes]
    pdus, pays, po, per_grid, starts = [], [], 0, [0, 0], set()
    for _ in range(2000):  # place non-overlapping candidates, seven on each grid (bounded: the grids fill up)
        if len(pdus) == 14:
            break
        g = 0 if per_grid[0] < 7 and (per_grid[1] == 7 or rng.integers(0, 2)) else 1
        nprb = sizes[g]
        AL, dur, port = int(rng.choice([1, 2, 4, 8, 16])), int(rng.integers(1, 4)), int(rng.integers(0, 3))
        start = int(rng.integers(0, 14 - dur))  # 0 .. 13 - duration
        if (6 * AL) % dur or 6 * AL // dur > nprb:
            continue
        n_rb = 6 * AL // dur
        cand = np.nonzero(~used[g][port, start:start + dur].any(axis=0))[0]
        if cand.size < n_rb:
            continue
        rb = np.zeros(nprb, np.uint8)
        rb[rng.choice(cand, n_rb, replace=False)] = 1
        used[g][port, start:start + dur] |= rb.astype(bool)
        A = int(rng.integers(12, min(129, 108 * AL - 24)))
        pay = rng.integers(0, 2, A, dtype=np.uint8)
        slot, rnti, nd, nr, ndm = int(rng.integers(0, 20)), int(rng.integers(1, 65536)), int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), int(rng.integers(0, 65536))
        ref = int(rng.integers(0, int(np.nonzero(rb)[0][0]) + 1))
        xdb, ddb = float(rng.choice([0.0, -3.0, 1.5])), float(rng.choice([0.0, 3.0]))
        assert O.o_pdcch_process(slot, rnti, nd, nr, ndm, ref, xdb, ddb, pay, AL, start, dur, rb, buf.grid(g)[port]) == 54 * AL
        pdus.append(_pdu(miphy, slot, rnti, nd, nr, ndm, ref, xdb, ddb, A, AL, start, dur, rb, po, buf.offsets[g], port))
        pays.append(pay)
        po += A
        per_grid[g] += 1
        starts.add(start)
    assert len(pdus) == 14 and per_grid == [7, 7] and len(starts) >= 4 and len({int(p["aggregation_level"]) for p in pdus}) >= 3
    # what the PDUs own is [start, start + duration) of their PRBs: everything else of the expectation is still the background
    for g in range(2):
        o, w = buf.offsets[g], buf.grid(g)
        kept = (D.bits(w) == D.bits(buf.start[o:o + w.size].reshape(w.shape))).reshape(w.shape + (2,)).all(axis=-1)
        assert kept[~np.repeat(used[g], 12, axis=2)].all() and not kept[np.repeat(used[g], 12, axis=2)].any()
    gd = buf.device()
    ctx.pdcch_process_batch(np.array(pdus, dtype=miphy.PdcchPdu), torch.from_numpy(np.concatenate(pays)).cuda(), gd)
    buf.check(gd, "pdcch_process_batch")


# ------------------------------------------------------------------------------------------------------------------- e. SS/PBCH block
def test_ssb_on_a_background(ctx):
    import miphy
    from test_ssb_proc_gpu import _pdu
    rng = np.random.default_rng(705)
    nprb, n = 52, 12
    buf = Buffer([(3, 14, nprb * 12)] * n, rng)
    pdus = []
    for i in range(n):
        N_id, L_max = int(rng.integers(0, 1008)), int(rng.choice([4, 8, 64]))
        ssb_idx, hrf, sfn, kssb = int(rng.integers(0, L_max)), int(rng.integers(0, 2)), int(rng.integers(0, 1024)), int(rng.integers(0, 24))
        k0, l0, beta = int(rng.integers(0, nprb * 12 - 240 + 1)), int(rng.integers(0, 11)), float(rng.choice([0.0, 3.0, -3.0]))
        p = dict(N_id=N_id, ssb_idx=ssb_idx, L_max=L_max, hrf=hrf, sfn=sfn, k_ssb=kssb, payload=rng.integers(0, 2, 32, dtype=np.uint8), k0=k0, l0=l0, beta=beta, ports=[0, 2])
        D.o_ssb(p, buf.grid(i))
        pdus.append(_pdu(miphy, N_id, ssb_idx, L_max, hrf, sfn, kssb, p["payload"], k0, l0, beta, nprb, [0, 2], buf.offsets[i]))
    # The block's elements beside PSS and SSS -- subcarriers 0..55 and 183..239 of symbol l0; 48..55 and 183..191 of symbol l0 + 2, whose outer 48 + 48
    # subcarriers carry PBCH -- hold whatever the oracle leaves there (the background: like the reference it maps nothing on them); the comparison
    # of the whole buffer covers them.
    g0, p0 = buf.grid(0), pdus[0]
    k0, l0 = int(p0["ssb_first_subcarrier"]), int(p0["ssb_first_symbol"])
    for l, cols in ((l0, list(range(56)) + list(range(183, 240))), (l0 + 2, list(range(48, 56)) + list(range(183, 192)))):
        assert np.array_equal(D.bits(g0[0, l, k0 + np.array(cols)]), D.bits(buf.start[buf.offsets[0]:][:g0.size].reshape(g0.shape)[0, l, k0 + np.array(cols)]))
    gd = buf.device()
    ctx.ssb_process_batch(np.array(pdus, dtype=miphy.SsbPdu), gd)
    buf.check(gd, "ssb_process_batch")


# ------------------------------------------------------------------------------------------------------------------- f. CSI-RS sweep
@pytest.fixture(scope="module")
def csi_case():
    return _build_csi_case()


def _build_csi_case():
    import miphy
    rng = np.random.default_rng(706)
    cases = D.csi_rs_pattern_cases()
    sizes = [int(rng.choice([n for n in (52, 80, 133, 275) if n >= max(c["bes"][1], c["start_rb"] + c["nof_rb"])])) for c in cases]
    buf = Buffer([(16, 14, n * 12) for n in sizes], rng)
    assert any(o % (16 * 14 * n * 12) for o, n in zip(buf.offsets, sizes))
    jobs = np.zeros(len(cases), dtype=miphy.CsiRsJob)
    for i, (c, nprb) in enumerate(zip(cases, sizes)):
        ports = rng.permutation(16)[:c["nports"]]
        while np.array_equal(ports, np.arange(c["nports"])):
            ports = rng.permutation(16)[:c["nports"]]
        D.o_csi_rs(dict(c, ports=ports), buf.grid(i))
        j = jobs[i]
        j["slot_in_frame"], j["scrambling_id"], j["amplitude"], j["start_rb"], j["nof_rb"] = c["slot"], c["scr"], c["amp"], c["start_rb"], c["nof_rb"]
        j["rb_begin"], j["rb_end"], j["rb_stride"], j["grid_nof_prb"], j["mapping_row"], j["cdm"], j["freq_density"] = *c["bes"], nprb, c["row"], c["cdm"], c["dens"]
        j["nof_ports"] = c["nports"]
        j["ports"][:c["nports"]] = ports
        j["re_mask"][:c["nports"]], j["symbol_mask"][:c["nports"]] = c["rm"], c["sm"]
        j["grid_offset"] = buf.offsets[i]
    return buf, jobs


@pytest.mark.parametrize("on_device", [False, True])
def test_csi_rs_sweep_on_a_background(ctx, csi_case, on_device):
    buf, jobs = csi_case
    gd = buf.device()
    ctx.csi_rs_map_batch(_jobs_arg(jobs, on_device), gd)
    buf.check(gd, "csi_rs_map_batch")


# ------------------------------------------------------------------------------------------------------------------- g. composed slot
@pytest.mark.parametrize("nprb", [52, 275])
def test_composed_slot_in_two_orders(ctx, nprb):
    """SS/PBCH block, three PDCCH PDUs, two CSI-RS jobs and three PDSCH PDUs onto one grid through the four entry points, enqueued on one stream
    without waiting for the device, in two orders; then (52 PRB) through the OFDM modulator."""
    import torch
    import miphy
    from test_pdcch_proc_gpu import _pdu as pdcch_pdu
    from test_ssb_proc_gpu import _pdu as ssb_pdu
    rng = np.random.default_rng(707 + nprb)
    s = D.compose_slot(rng, nprb, 4)
    buf = Buffer([s.shape], rng)
    go = buf.offsets[0]
    buf.grid(0)[...] = s.expected
    buf.start[go:go + s.expected.size] = s.background.reshape(-1)
    ssb = np.array([ssb_pdu(miphy, p["N_id"], p["ssb_idx"], p["L_max"], p["hrf"], p["sfn"], p["k_ssb"], p["payload"], p["k0"], p["l0"], p["beta"], nprb, p["ports"], go)
                    for p in s.ssb], dtype=miphy.SsbPdu)
    pdcch, pays, po = [], [], 0
    for p in s.pdcch:
        pdcch.append(pdcch_pdu(miphy, p["slot"], p["rnti"], p["n_id_data"], p["n_rnti"], p["n_id_dmrs"], p["ref_point"], p["data_dB"], p["dmrs_dB"], p["payload"].size, p["AL"],
                               p["start"], p["dur"], p["rb"], po, go, p["port"]))
        pays.append(p["payload"])
        po += p["payload"].size
    pdcch = np.array(pdcch, dtype=miphy.PdcchPdu)
    csi = np.zeros(len(s.csi), dtype=miphy.CsiRsJob)
    for j, c in zip(csi, s.csi):
        j["slot_in_frame"], j["scrambling_id"], j["amplitude"], j["start_rb"], j["nof_rb"] = c["slot"], c["scr"], c["amp"], c["start_rb"], c["nof_rb"]
        j["rb_begin"], j["rb_end"], j["rb_stride"], j["grid_nof_prb"], j["mapping_row"], j["cdm"], j["freq_density"] = *c["bes"], nprb, c["row"], c["cdm"], c["dens"]
        j["nof_ports"] = c["nports"]
        j["ports"][:c["nports"]] = c["ports"]
        j["re_mask"][:c["nports"]], j["symbol_mask"][:c["nports"]], j["grid_offset"] = c["rm"], c["sm"], go
    pdsch, tb = _pdsch_pdus(miphy, s.pdsch, [go] * len(s.pdsch))
    pay_d, tb_d = torch.from_numpy(np.concatenate(pays)).cuda(), torch.from_numpy(tb).cuda()
    calls = [lambda g: ctx.ssb_process_batch(ssb, g), lambda g: ctx.pdcch_process_batch(pdcch, pay_d, g), lambda g: ctx.csi_rs_map_batch(csi, g),
             lambda g: ctx.pdsch_process_batch(pdsch, tb_d, g)]
    ga, gb = buf.device(), buf.device()
    for c in calls:          # order A: SSB, PDCCH, CSI-RS, PDSCH
        c(ga)
    for c in calls[::-1]:    # order B: PDSCH, CSI-RS, PDCCH, SSB
        c(gb)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(ga).view(torch.int32), torch.view_as_real(gb).view(torch.int32))
    buf.check(ga, "order A")
    buf.check(gb, "order B")
    # the union of the written masks is what differs from the background (outside it every element is still the background)
    union = np.zeros(s.shape, bool)
    for m in s.masks.values():
        union |= m
    got = ga.cpu().numpy()[go:go + s.expected.size].reshape(s.shape)
    kept = (D.bits(got) == D.bits(s.background)).reshape(s.shape + (2,)).all(axis=-1)
    assert kept[~union].all() and not kept[union].all()
    if nprb != 52:
        return
    # OFDM modulator on the four ports of both grids (non-finite background elements replaced), against the oracle on the expected grid
    cfg, ocfg = miphy.OfdmConfig(1, nprb, 1024, 0, 0.01, 0.0, 3.5e9), O.OfdmCfg(1, nprb, 1024, 0, 0.01, 3.5e9)
    want = D.finite_copy(s.expected)
    ns = cfg.slot_size(0)
    jobs = np.zeros(4, dtype=miphy.OfdmJob)
    for p in range(4):
        jobs[p] = (p * ns, p * 14 * nprb * 12, 0, 0)
    exp = [O.o_ofdm_mod_slot(ocfg, 0, want[p]) for p in range(4)]
    for name, gdev in (("A", ga), ("B", gb)):
        fin = D.finite_copy(gdev.cpu().numpy()[go:go + s.expected.size])
        assert np.array_equal(D.bits(fin), D.bits(want.reshape(-1)))
        y_d = torch.zeros(4 * ns, dtype=torch.complex64, device="cuda")
        ctx.ofdm_modulate_slots(cfg, jobs, torch.from_numpy(fin).cuda(), y_d)
        torch.cuda.synchronize()
        y = y_d.cpu().numpy().reshape(4, ns)
        for p in range(4):
            assert rel_err(y[p], exp[p]) < TOL, (name, p, rel_err(y[p], exp[p]))
