"""GPU: PDSCH on one codeword and 1..4 layers -- miphy_pdsch_modulate_layers_batch against o_pdsch_modulate, miphy_pdsch_encode_batch at 2, 3 and 4
layers against o_pdsch_encode (tests/test_sch_gpu.py encodes on two layers of base graph 1 only, so this is not covered there), and
miphy_pdsch_process_layers_batch against the composition o_pdsch_encode(L) -> o_pdsch_modulate -> o_dmrs_pdsch_map(ports). Every comparison is
on the bits of buffers that start as dl_grid.background(), guard elements and ports a job does not name included.

Four layers: the oracle takes them as two codeword arguments and is handed the one codeword in that form (pdsch_layers_cases.oracle_modulate);
tests/test_pdsch_layers.py checks with the oracle alone that this states x^(ly)(i) = d(4 i + ly) of one codeword."""
import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O
import pdsch_layers_cases as PC
from test_pdsch_layers import _words, mod_layers_job

pytestmark = pytest.mark.gpu
CASES = PC.cases()
IDS = [c["name"] for c in CASES]
G = PC.GUARD


# ---------------------------------------------------------------------------------------------------- modulator
def _buffers(cases):
    """Flat background [guard | grid | guard] per case, the codewords at 16-byte slots plus each case's own byte offset, and the offsets."""
    grids, cws, goff, coff, g0, c0 = [], [], [], [], 0, 0
    for c in cases:
        n = int(np.prod(PC.grid_shape(c)))
        bg = D.background(n + 2 * G, np.random.default_rng(len(c["name"]) + n))
        bg[G:G + n] = PC.background(c).reshape(-1)
        grids.append(bg)
        goff.append(g0 + G)
        g0 += bg.size
        cw = PC.codeword(c)
        coff.append(c0 + c["cw_pad"])
        cws.append(np.concatenate([np.full(c["cw_pad"], 3, np.uint8), cw, np.full((-(c["cw_pad"] + cw.size)) % 16 + 16, 3, np.uint8)]))
        c0 += cws[-1].size
    return grids, np.concatenate(cws), goff, coff


def _modulate(ctx, cases, on_device=False):
    """One call for `cases`; returns the list of their buffers [guard | grid | guard] afterwards."""
    import torch
    import miphy
    grids, cw, goff, coff = _buffers(cases)
    jobs = np.array([mod_layers_job(miphy, c, cw_off=co, grid_off=go) for c, go, co in zip(cases, goff, coff)], dtype=miphy.PdschModLayersJob)
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_layers_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs, torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    got, out, o = gd.cpu().numpy(), [], 0
    for g in grids:
        out.append(got[o:o + g.size])
        o += g.size
    return out


@pytest.fixture(scope="module")
def alone(ctx):
    """Every case in a call of its own (host jobs): computed once, shared and left unchanged."""
    return {c["name"]: _modulate(ctx, [c])[0] for c in CASES}


def _expected(c, apply):
    bg = _buffers([c])[0][0]
    grid = bg[G:bg.size - G].reshape(PC.grid_shape(c)).copy()
    rc = apply(c, grid)
    want = bg.copy()
    want[G:bg.size - G] = grid.reshape(-1)
    return want, rc


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_modulator_matches_oracle(alone, c):
    """Bit-equal to o_pdsch_modulate on a grid that already holds signals, guards and unnamed ports included."""
    want, rc = _expected(c, PC.oracle_modulate)
    diff = int((D.bits(alone[c["name"]]) != D.bits(want)).sum())
    print("%s: oracle returns %d for %d REs per layer; %d words differ" % (c["name"], rc, PC.nof_re(c), diff))
    assert rc == PC.nof_re(c)
    assert diff == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_one_batch_of_all_cases_equals_each_case_alone(ctx, alone, on_device):
    got = _modulate(ctx, CASES, on_device)
    for c, g in zip(CASES, got):
        assert np.array_equal(D.bits(g), D.bits(alone[c["name"]])), c["name"]


def test_one_layer_equals_the_one_layer_entry_point(ctx, alone):
    """L = 1 through the new entry point writes the bytes miphy_pdsch_modulate_batch writes (base.port names the port there)."""
    import torch
    import miphy
    ones = [c for c in CASES if c["L"] == 1]
    assert {c["mod"] for c in ones} == {1, 2, 4, 6, 8}
    grids, cw, goff, coff = _buffers(ones)
    jobs = np.zeros(len(ones), dtype=miphy.PdschModJob)
    for i, (c, go, co) in enumerate(zip(ones, goff, coff)):
        jobs[i] = mod_layers_job(miphy, c, cw_off=co, grid_off=go)["base"]
        jobs[i]["port"] = c["ports"][0]
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_batch(jobs, torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(np.concatenate([alone[c["name"]] for c in ones])))


def _one_case_call(ctx, miphy, c, edit, on_device=False, extra=()):
    """The case's job, edited, in a call; returns (error text or None, the buffer afterwards, its background)."""
    import torch
    grids, cw, goff, coff = _buffers([c])
    j = mod_layers_job(miphy, c, cw_off=coff[0], grid_off=goff[0])
    edit(j)
    jobs = np.array([j] + list(extra), dtype=miphy.PdschModLayersJob)
    gd = torch.from_numpy(grids[0]).cuda()
    err = None
    try:
        ctx.pdsch_modulate_layers_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs, torch.from_numpy(cw).cuda(), gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return err, gd.cpu().numpy(), grids[0]


def _set(path, value):
    def edit(j):
        rec = j
        for k in path[:-1]:
            rec = rec[k]
        rec[path[-1]] = value
    return edit


MOD_REJECTIONS = [  # one per rule of the entry point: (what to break, the message)
    (_set(("nof_layers",), 0), "number of layers"), (_set(("nof_layers",), 5), "number of layers"),
    (_set(("ports",), [1, 1, 0, 0]), "share port"), (_set(("ports",), [0, 16, 0, 0]), "invalid port"),
    (lambda j: _set(("base", "nof_bits"), int(j["base"]["nof_bits"]) // 2)(j), "codeword of"),  # REs x mod: the layers forgotten
    (_set(("base", "mod"), 3), "modulation"), (_set(("base", "nof_symbols"), 15), "time allocation"), (_set(("base", "dmrs_type"), 0), "DM-RS type"),
    (_set(("base", "nof_cdm_groups_without_data"), 3), "CDM groups"), (_set(("base", "grid_nof_prb"), 276), "grid / BWP"),
    (_set(("base", "bwp_size_rb"), 276), "grid / BWP"), (_set(("base", "nof_reserved"), 5), "reserved RE patterns"),
    (_set(("base", "n_id"), 1024), "scrambling identifiers"), (_set(("base", "rnti"), 65536), "scrambling identifiers"),
]


@pytest.mark.parametrize("k", range(len(MOD_REJECTIONS)))
def test_modulator_rejects_host_jobs(ctx, k):
    """MIPHY_EINVAL before anything is enqueued: the grid still holds its background."""
    import miphy
    edit, msg = MOD_REJECTIONS[k]
    c = next(c for c in CASES if c["name"] == "d_L2_mod4_aligned")
    err, got, bg = _one_case_call(ctx, miphy, c, edit)
    assert err is not None and "miphy error -1" in err and msg in err, err
    assert np.array_equal(D.bits(got), D.bits(bg))


def test_device_job_with_five_layers_is_skipped(ctx, alone):
    """A device-resident job reaches the kernels unseen by the host: one with L = 5 is left at once, its neighbour in the batch is mapped."""
    import miphy
    c = next(c for c in CASES if c["name"] == "d_L2_mod4_aligned")
    err, got, bg = _one_case_call(ctx, miphy, c, _set(("nof_layers",), 5), on_device=True)
    assert err is None and np.array_equal(D.bits(got), D.bits(bg))
    bad = mod_layers_job(miphy, c, cw_off=0, grid_off=G)
    bad["nof_layers"], bad["base"]["scaling"] = 5, 3.0  # same grid as the good job: anything it wrote would show
    err, got, bg = _one_case_call(ctx, miphy, c, lambda j: None, on_device=True, extra=[bad])
    assert err is None and np.array_equal(D.bits(got), D.bits(alone[c["name"]]))


# ---------------------------------------------------------------------------------------------------- encoder on 2..4 layers
def test_encoder_on_two_to_four_layers(ctx):
    """One small transport block per base graph at 2, 3 and 4 layers, REs per layer that the codeblocks do not divide."""
    import torch
    import miphy
    rng = np.random.default_rng(94)
    descs, tbs, tb_off, cw_off = [], [], 0, 0
    for bg, tb_bytes, mod, nre, rv, Nref in ((1, 1100, 4, 1301, 0, 0), (2, 481, 6, 517, 2, 0), (2, 40, 2, 133, 3, 2000), (1, 2200, 8, 1003, 1, 20000)):
        for L in (2, 3, 4):
            tb = rng.integers(0, 256, tb_bytes, dtype=np.uint8)
            descs.append((bg, rv, mod, L, Nref, nre * L, tb.size, tb_off, cw_off))
            tbs.append(tb)
            tb_off += (tb.size + 15) // 16 * 16
            cw_off += nre * L * mod
    d = np.zeros(len(descs), dtype=miphy.PdschTbDesc)
    tb_all = np.zeros(tb_off + 16, np.uint8)
    for i, x in enumerate(descs):
        d[i] = x
        tb_all[x[7]:x[7] + tbs[i].size] = tbs[i]
    cw_d = torch.full((cw_off,), 9, dtype=torch.uint8, device="cuda")
    ctx.pdsch_encode_batch(d, torch.from_numpy(tb_all).cuda(), cw_d)
    torch.cuda.synchronize()
    cw = cw_d.cpu().numpy()
    for i, (bg, rv, mod, L, Nref, nsym, nb, to, co) in enumerate(descs):
        assert np.array_equal(cw[co:co + nsym * mod], O.o_pdsch_encode(bg, rv, mod, Nref, L, nsym, tbs[i])), descs[i]


# ---------------------------------------------------------------------------------------------------- processor
NPRB, NPORTS = 52, 4


def _pdus():
    """Four PDUs of L = 1, 2, 3, 4 layers on disjoint PRBs of one grid: both base graphs, rv 0 and 2, a reserved pattern, port lists out of order."""
    rng = np.random.default_rng(2024)
    out = []
    for L, ports, prbs, mod, bg, rv, dsyms, start, nof, prb0, bwp, nres, (ddb, xdb), lbrm in (
            (1, (2,), range(0, 10), 2, 2, 0, (2,), 0, 14, 0, (0, NPRB), 0, (0.0, 0.0), 1200),
            (2, (1, 3), range(10, 22), 4, 1, 2, (2, 11), 1, 13, 0, (0, NPRB), 1, (-3.0, 1.5), 3168),
            (3, (0, 2, 1), range(22, 36), 6, 2, 2, (3,), 2, 10, 1, (20, 30), 0, (3.0, 0.0), 3168),
            (4, (3, 1, 0, 2), range(36, 52), 8, 1, 0, (2, 7), 0, 14, 0, (0, NPRB), 0, (0.0, -2.0), 3168)):
        rb = np.zeros(NPRB, np.uint8)
        rb[list(prbs)] = 1
        reserved = [(rb & (rng.uniform(size=NPRB) < 0.5).astype(np.uint8), 0x3C5, (1 << 4) | (1 << 11))][:nres]
        p = dict(L=L, ports=list(ports), rb=rb, mod=mod, bg=bg, rv=rv, dmrs_symbols=dsyms, start=start, nof=nof, ref_point_prb0=prb0, bwp=bwp, cdm=2, reserved=reserved,
                 dmrs_dB=ddb, data_dB=xdb, lbrm_bytes=lbrm, slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)),
                 scr=int(rng.integers(0, 65536)), n_scid=int(rng.integers(0, 2)))
        p["nof_re"] = int(D.pdsch_data_mask(p).sum())
        p["tb"] = rng.integers(0, 256, min(3824 // 8 if bg == 2 else 10 ** 6, max(8, int(p["nof_re"] * L * mod * 0.4) // 8)), dtype=np.uint8)
        out.append(p)
    return out


def _case_of(p):
    """The PDU's modulator configuration as a case of pdsch_layers_cases (for the oracle wrappers there)."""
    return dict(name="pdu", L=p["L"], mod=p["mod"], nprb_grid=NPRB, prbs=np.nonzero(p["rb"])[0].astype(np.uint16), start=p["start"], nof=p["nof"], dmrs=p["dmrs_symbols"], type2=0,
                cdm=p["cdm"], bwp=p["bwp"], reserved=p["reserved"], ports=p["ports"], grid_ports=NPORTS, scaling=D.db_to_amplitude(-p["data_dB"]), cw_pad=0, rnti=p["rnti"],
                n_id=p["n_id"])


def _o_process(p, grid):
    """The composition o_pdsch_encode(L) -> o_pdsch_modulate -> o_dmrs_pdsch_map(ports) on grid [ports][14][nsc] in place, with the scalings of tests/test_pdsch_proc_gpu.py (dl_grid.o_pdsch_process);
    returns what the modulator step returns."""
    L, c = p["L"], _case_of(p)
    if "cw" not in p:
        p["cw"] = O.o_pdsch_encode(p["bg"], p["rv"], p["mod"], p["lbrm_bytes"] * 8, L, p["nof_re"] * L, p["tb"])
    rc = PC.oracle_modulate(c, grid, p["cw"])
    O.o_dmrs_pdsch_map(p["slot"], p["bwp"][0] if p["ref_point_prb0"] else 0, 0, p["scr"], p["n_scid"], D.db_to_amplitude(-p["dmrs_dB"]), PC.dmrs_mask(c), p["rb"], p["ports"],
                       grid)
    return rc


def _records(miphy, pdus, layers=True):
    rec = np.zeros(len(pdus), dtype=miphy.PdschLayersPdu if layers else miphy.PdschPdu)
    tb_off, tbs = 0, []
    for r, p in zip(rec, pdus):
        b = r["base"] if layers else r
        b["slot_in_frame"], b["rnti"], b["n_id"], b["dmrs_scrambling_id"], b["tbs_lbrm_bytes"], b["tb_bytes"] = p["slot"], p["rnti"], p["n_id"], p["scr"], p["lbrm_bytes"], p["tb"].size
        b["ratio_pdsch_dmrs_to_sss_dB"], b["ratio_pdsch_data_to_sss_dB"] = p["dmrs_dB"], p["data_dB"]
        b["bg"], b["rv"], b["mod"], b["start_symbol"], b["nof_symbols"] = p["bg"], p["rv"], p["mod"], p["start"], p["nof"]
        b["port"] = 15 if layers else p["ports"][0]  # ignored by the layered entry point
        b["nof_cdm_groups_without_data"], b["n_scid"], b["ref_point_prb0"], b["nof_reserved"] = p["cdm"], p["n_scid"], p["ref_point_prb0"], len(p["reserved"])
        b["dmrs_symbols_mask"] = sum(1 << s for s in p["dmrs_symbols"])
        b["grid_nof_prb"], b["bwp_start_rb"], b["bwp_size_rb"], b["rb_mask"] = NPRB, p["bwp"][0], p["bwp"][1], _words(p["rb"])
        for k, (pm, rm, sm) in enumerate(p["reserved"]):
            b["reserved"][k]["prb_mask"], b["reserved"][k]["re_mask"], b["reserved"][k]["symbols"] = _words(pm), rm, sm
        b["tb_offset"], b["grid_offset"] = tb_off, G
        if layers:
            r["nof_layers"] = p["L"]
            r["ports"][:p["L"]] = p["ports"]
        tbs.append(np.concatenate([p["tb"], np.zeros((-p["tb"].size) % 16, np.uint8)]))
        tb_off += tbs[-1].size
    return rec, np.concatenate(tbs + [np.zeros(16, np.uint8)])


def _grid_background():
    return D.background(G + NPORTS * 14 * NPRB * 12 + G, np.random.default_rng(808))


def _process(c, rec, tb, layers=True):
    import torch
    gd = torch.from_numpy(_grid_background()).cuda()
    (c.pdsch_process_layers_batch if layers else c.pdsch_process_batch)(rec, torch.from_numpy(tb).cuda(), gd)
    torch.cuda.synchronize()
    return gd.cpu().numpy()


@pytest.fixture(scope="module")
def processed(ctx):
    import miphy
    pdus = _pdus()
    rec, tb = _records(miphy, pdus)
    return pdus, rec, tb, _process(ctx, rec, tb)


def _inner(buf):
    return buf[G:buf.size - G].reshape(NPORTS, 14, NPRB * 12)


def test_processor_batch_matches_oracle_chain(processed):
    import miphy
    pdus, rec, tb, got = processed
    bg = _grid_background()
    assert np.array_equal(D.bits(got[:G]), D.bits(bg[:G])) and np.array_equal(D.bits(got[-G:]), D.bits(bg[-G:]))
    want = _inner(bg).copy()
    rcs = [_o_process(p, want) for p in pdus]
    for p, r, rc in zip(pdus, rec, rcs):  # the PDUs own disjoint PRBs: each is judged on its own columns, the one-layer PDU first
        assert miphy.pdsch_layers_pdu_nof_re(r) == p["nof_re"]
        cols = np.repeat(p["rb"] != 0, 12)
        diff = int((D.bits(_inner(got)[:, :, cols]) != D.bits(want[:, :, cols])).sum())
        print("L = %d: the oracle's modulator returns %d for %d REs per layer; %d words differ" % (p["L"], rc, p["nof_re"], diff))
        assert rc == p["nof_re"] and diff == 0, p["L"]
    assert np.array_equal(D.bits(_inner(got)), D.bits(want))


def test_processor_result_is_independent_of_order_and_history(ctx, processed):
    """Bit-equal with the PDUs enqueued in the opposite order, and on a context that has run nothing before (the session's context has grown its
    workspaces under every other test)."""
    import miphy
    pdus, rec, tb, got = processed
    assert np.array_equal(D.bits(_process(ctx, rec[::-1].copy(), tb)), D.bits(got))
    fresh = miphy.Context(0)
    try:
        assert np.array_equal(D.bits(_process(fresh, rec, tb)), D.bits(got))
        # ... and after a larger batch of another shape on that context
        big = np.concatenate([rec[3:4]] * 3 + [rec[0:1]] * 2)
        _process(fresh, big, tb)
        assert np.array_equal(D.bits(_process(fresh, rec, tb)), D.bits(got))
    finally:
        fresh.close()


def test_processor_one_layer_batch_equals_the_one_layer_entry_point(ctx):
    import miphy
    pdus = [dict(p, L=1, ports=p["ports"][:1], tb=p["tb"][:max(8, p["tb"].size // p["L"])]) for p in _pdus()]
    rec, tb = _records(miphy, pdus)
    rec1, tb1 = _records(miphy, pdus, layers=False)
    assert np.array_equal(tb, tb1)
    got, got1 = _process(ctx, rec, tb), _process(ctx, rec1, tb1, layers=False)
    assert np.array_equal(D.bits(got), D.bits(got1))
    assert not np.array_equal(D.bits(got), D.bits(_grid_background()))


def _pb(field, value):
    return lambda r: r["base"].__setitem__(field, value)


PROC_REJECTIONS = [
    (lambda r: r.__setitem__("nof_layers", 0), "number of layers"), (lambda r: r.__setitem__("nof_layers", 5), "number of layers"),
    (lambda r: r.__setitem__("ports", [3, 3, 0, 0]), "share port"), (lambda r: r.__setitem__("ports", [1, 16, 0, 0]), "invalid port"),
    (_pb("mod", 3), "modulation"), (_pb("nof_symbols", 15), "time allocation"), (_pb("nof_cdm_groups_without_data", 3), "CDM groups"),
    (_pb("grid_nof_prb", 276), "grid / BWP|empty allocation"), (_pb("bwp_size_rb", 276), "grid / BWP"), (_pb("nof_reserved", 5), "reserved RE patterns"), (_pb("n_id", 1024), "scrambling identifiers"),
    (_pb("rnti", 65536), "scrambling identifiers"), (_pb("dmrs_symbols_mask", 0), "DM-RS symbol mask"), (_pb("dmrs_symbols_mask", 1 << 0), "outside the time allocation"),
    (_pb("tbs_lbrm_bytes", 0), "LBRM"), (_pb("tbs_lbrm_bytes", 3169), "LBRM"), (_pb("bg", 3), "base graph"), (_pb("rv", 4), "redundancy version"),
    (_pb("rb_mask", [0, 0, 0, 0, 0]), "empty allocation"), (_pb("tb_bytes", 0), "transport block"),
    (_pb("tb_bytes", 54754), "transport block of 54754 bytes"),                                      # 53 codeblocks of base graph 1
    (lambda r: (_pb("bg", 2)(r), _pb("tb_bytes", 24802)(r)), "transport block of 24802 bytes"),     # 53 codeblocks of base graph 2
    (lambda r: (_pb("ref_point_prb0", 1)(r), _pb("bwp_start_rb", 60)(r), _pb("bwp_size_rb", 10)(r)), "reference point"),
]


@pytest.mark.parametrize("k", range(len(PROC_REJECTIONS)))
def test_processor_rejects(ctx, k):
    """MIPHY_EINVAL for a batch whose second PDU breaks one rule (the batch is the first two PDUs of the fixture, valid as they stand), before
    anything is enqueued: the grid still holds its background."""
    import torch
    import miphy
    edit, msg = PROC_REJECTIONS[k]
    pdus = _pdus()
    rec, tb = _records(miphy, [pdus[0], pdus[1]])
    edit(rec[1])
    bg = _grid_background()
    gd = torch.from_numpy(bg).cuda()
    with pytest.raises(RuntimeError, match=msg) as e:
        ctx.pdsch_process_layers_batch(rec, torch.from_numpy(tb).cuda(), gd)
    assert "miphy error -1" in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))


ALIKE_REJECTIONS = [  # (what to break in the base record, its port, the message all three processor forms give)
    (lambda b, port: b.__setitem__("mod", 3), "invalid modulation"), (lambda b, port: port(16), "invalid port"),
    (lambda b, port: b.__setitem__("grid_nof_prb", 276), "invalid or empty allocation"), (lambda b, port: b.__setitem__("n_id", 1024), "invalid scrambling identifiers"),
    (lambda b, port: b.__setitem__("rnti", 65536), "invalid scrambling identifiers"),
    (lambda b, port: (b.__setitem__("ref_point_prb0", 1), b.__setitem__("bwp_start_rb", 60), b.__setitem__("bwp_size_rb", 10)), "reference point outside the grid"),
]


@pytest.mark.parametrize("k", range(len(ALIKE_REJECTIONS)))
def test_processor_forms_refuse_alike(ctx, k):
    """Two valid one-layer PDUs of which the second breaks one rule: miphy_pdsch_process_batch, the prepared plan and
    miphy_pdsch_process_layers_batch give the same message with MIPHY_EINVAL and leave the grid at its background."""
    import torch
    import miphy
    edit, msg = ALIKE_REJECTIONS[k]
    pdus = [dict(p, L=1, ports=p["ports"][:1], tb=p["tb"][:max(8, p["tb"].size // p["L"])]) for p in _pdus()[:2]]
    rec, tb = _records(miphy, pdus)
    rec1, tb1 = _records(miphy, pdus, layers=False)
    edit(rec[1]["base"], lambda v: rec[1]["ports"].__setitem__(0, v))
    edit(rec1[1], lambda v: rec1[1].__setitem__("port", v))
    bg = _grid_background()
    tb_d = torch.from_numpy(tb).cuda()
    for call in (lambda g: ctx.pdsch_process_batch(rec1, tb_d, g), lambda g: miphy.PdschProcessPlan(ctx, rec1), lambda g: ctx.pdsch_process_layers_batch(rec, tb_d, g)):
        gd = torch.from_numpy(bg).cuda()
        with pytest.raises(RuntimeError) as e:
            call(gd)
        assert "miphy error -1" in str(e.value) and msg in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))
