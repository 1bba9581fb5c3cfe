"""GPU: PDSCH with precoding -- miphy_pdsch_modulate_precoded_batch, miphy_dmrs_pdsch_map_precoded_batch and miphy_pdsch_process_precoded_batch against
the numerical contract of tests/pdsch_precoded_cases.py (y = sum W x in float64, tolerance 2 x 2 L x 2^-24 x A, derived there), against the layered
modulator bit for bit where the matrices are permutations, and against the device composition modulator -> miphy_channel_precode_batch bit for bit.
Every comparison starts from dl_grid.background() grids with guard elements and is on the bit patterns outside what the job owns."""
import itertools

import numpy as np
import pytest

import dl_grid as D
import pdsch_layers_cases as PC
import pdsch_mapped_cases as MC
import pdsch_precoded_cases as XC
from test_pdsch_layers import mod_layers_job
from test_pdsch_layers_gpu import _buffers, _modulate
from test_pdsch_mapped_gpu import NPORTS, NPRB, _lists, _records as _mapped_records
from test_pdsch_precoded import dmrs_precoded_job, mod_precoded_job, precoding_record

pytestmark = pytest.mark.gpu
G = XC.GUARD
LC = {c["name"]: c for c in PC.cases()}
NAN = np.complex64(np.nan + 1j * np.nan)


# ---------------------------------------------------------------------------------------------------- one call
def _pc_case(pc):
    return dict(pc["c"], grid_ports=pc["grid_ports"])


def _weights(xs):
    """The weights array of a batch: W of each case behind a gap of 1, 2, 3 NaN entries (a weight read from a gap poisons the result); the offsets."""
    parts, offs, o = [], [], 0
    for i, x in enumerate(xs):
        gap = np.full(1 + i % 3, NAN, np.complex64)
        parts += [gap, x["W"].reshape(-1)]
        offs.append(o + gap.size)
        o += gap.size + x["W"].size
    parts.append(np.full(2, NAN, np.complex64))
    return np.concatenate(parts), offs


def _jobs(miphy, pcs):
    cases = [_pc_case(pc) for pc in pcs]
    grids, cw, goff, coff = _buffers(cases)
    lists, loff = _lists(cases, ["vmap" in c for c in cases])
    w, woff = _weights(pcs)
    jobs = np.array([mod_precoded_job(miphy, pc, lo, wo, cw_off=co, grid_off=go) for pc, lo, wo, go, co in zip(pcs, loff, woff, goff, coff)],
                    dtype=miphy.PdschModPrecodedJob)
    return jobs, lists, w, grids, cw


def _split(got, grids):
    out, o = [], 0
    for g in grids:
        out.append(got[o:o + g.size])
        o += g.size
    return out


def _run(ctx, jobs, lists, w, grids, cw, on_device=False):
    """One call; returns (error text or None, the buffers [guard | grid | guard] afterwards)."""
    import torch
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    err = None
    try:
        if on_device:
            ctx.pdsch_modulate_precoded_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), torch.from_numpy(lists.view(np.int16).copy()).cuda(),
                                              torch.from_numpy(w).cuda(), torch.from_numpy(cw).cuda(), gd)
        else:
            ctx.pdsch_modulate_precoded_batch(jobs, lists, w, torch.from_numpy(cw).cuda(), gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return err, _split(gd.cpu().numpy(), grids)


def _inner(buf, x):
    return buf[G:buf.size - G].reshape(XC.grid_shape(x) if "c" in x else (x["grid_ports"], 14, x["nprb_grid"] * 12))


def _guards_kept(got, bg):
    return np.array_equal(D.bits(got[:G]), D.bits(bg[:G])) and np.array_equal(D.bits(got[-G:]), D.bits(bg[-G:]))


def _check(pc, got, bg, statement=None):
    assert _guards_kept(got, bg), pc["name"]
    XC.check_grid(pc, _inner(got, pc), _inner(bg, pc), *(XC.data_statement(pc) if statement is None else statement))


def _one(ctx, pc, on_device=False):
    import miphy
    jobs, lists, w, grids, cw = _jobs(miphy, [pc])
    err, got = _run(ctx, jobs, lists, w, grids, cw, on_device)
    assert err is None, err
    return got[0], grids[0]


# ---------------------------------------------------------------------------------------------------- (a) sweep
SWEEP = [XC.precoded(c, P, 4) for c in PC.cases() if c["name"].startswith("sweep_") for P in (c["L"], min(2 * c["L"], 16))]


def test_sweep_is_what_it_should_be():
    assert len(SWEEP) == 40 and {(pc["L"], pc["c"]["mod"]) for pc in SWEEP} == {(L, m) for L in (1, 2, 3, 4) for m in (1, 2, 4, 6, 8)}
    assert all(list(pc["c"]["prbs"]) == [1, 2, 4] and pc["nof_prg"] == 2 for pc in SWEEP)  # PRBs 1, 2 in PRG 0 and PRB 4 in PRG 1


@pytest.mark.parametrize("pc", SWEEP, ids=lambda pc: pc["name"])
def test_sweep_within_the_contract(ctx, pc):
    _check(pc, *_one(ctx, pc))


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_sweep_in_one_batch(ctx, on_device):
    import miphy
    jobs, lists, w, grids, cw = _jobs(miphy, SWEEP)
    assert {int(j["precoding"]["weights_offset"]) % 2 for j in jobs} == {0, 1}
    err, got = _run(ctx, jobs, lists, w, grids, cw, on_device)
    assert err is None, err
    for pc, g, bg in zip(SWEEP, got, grids):
        _check(pc, g, bg)


# ---------------------------------------------------------------------------------------------------- (b) permutation matrices
@pytest.mark.parametrize("name", ["g_ports_2031_L4_mod2", "h_type1_cdm1_L2_mod6", "h_type1_cdm2_L3_mod4", "h_type2_cdm3_L2_mod8"])
def test_permutation_matrices_copy_the_layers_bit_for_bit(ctx, name):
    """Every PRG has another permutation (weight 1 + 0j from layer ly to port sigma_g(ly), zeros elsewhere, two ports more than layers): a port holds in
    each PRG the bits miphy_pdsch_modulate_layers_batch writes for the layer sent there, the ports no layer is sent to hold +-0."""
    c = LC[name]
    L, P = c["L"], c["L"] + 2
    pc = XC.precoded(c, P, 4, tag="_perm")
    arrangements = list(itertools.permutations(range(P), L))  # 12, 60 or 360 of them: a stride of 7 visits them all
    sigma = np.array([arrangements[(7 * g + 1) % len(arrangements)] for g in range(pc["nof_prg"])])
    assert len({tuple(s) for s in sigma}) == pc["nof_prg"]
    pc["W"] = np.zeros((pc["nof_prg"], P, L), np.complex64)
    for g in range(pc["nof_prg"]):
        pc["W"][g, sigma[g], np.arange(L)] = 1.0
    got, bg = _one(ctx, pc)
    layered = _modulate(ctx, [c])[0]
    lay = layered[G:layered.size - G].reshape(PC.grid_shape(c))
    sy, col = XC.data_positions(c)
    x = lay[np.asarray(c["ports"])[:, None], sy[None, :], col[None, :]]  # [L][n], the device's own layer symbols
    want = np.zeros((P, sy.size), np.complex64)
    prg = (col // 12) // 4
    for ly in range(L):
        want[sigma[prg, ly], np.arange(sy.size)] = x[ly]
    have = _inner(got, pc)[np.arange(P)[:, None], sy[None, :], col[None, :]]
    sent = np.zeros((P, sy.size), bool)
    for ly in range(L):
        sent[sigma[prg, ly], np.arange(sy.size)] = True
    assert len(set(prg.tolist())) >= 2
    assert np.array_equal(D.bits(have).reshape(P, -1, 2)[sent], D.bits(want).reshape(P, -1, 2)[sent])
    assert ((D.bits(have).reshape(P, -1, 2)[~sent] & 0x7FFFFFFF) == 0).all()  # +-0
    owned = XC.owned_mask(pc, sy, col)
    assert np.array_equal(D.bits(_inner(got, pc)).reshape(owned.shape + (2,))[~owned], D.bits(_inner(bg, pc)).reshape(owned.shape + (2,))[~owned])
    assert _guards_kept(got, bg)


# ---------------------------------------------------------------------------------------------------- (c) fused equals composed
COMPOSED = ["b_L3_mod8", "c_L4_mod8"] + ["d_L%d_mod%d_%s" % (L, m, t) for L, m in ((2, 4), (3, 4), (2, 8), (3, 8)) for t in ("odd", "aligned")] + \
           ["e_275prb_L2_mod8", "e_275prb_L2_mod6"]


@pytest.mark.parametrize("name", COMPOSED)
def test_fused_equals_composed(ctx, name):
    """The fused entry point against: the layered modulator onto an L-port staging grid, the data REs gathered in numpy, miphy_channel_precode_batch with
    one job per PRG, the results scattered back -- bit for bit, and the result is within the contract."""
    import torch
    import miphy
    c = LC[name]
    pc = XC.precoded(c, 4, 4)
    got, bg = _one(ctx, pc)
    layered = _modulate(ctx, [c])[0]
    lay = layered[G:layered.size - G].reshape(PC.grid_shape(c))
    sy, col = XC.data_positions(c)
    x = lay[np.asarray(c["ports"])[:, None], sy[None, :], col[None, :]]
    prg = (col // 12) // pc["prg_size"]
    L, P = pc["L"], pc["P"]
    jobs, xin, where, io, oo = [], [], [], 0, 0
    for g in sorted(set(prg.tolist())):
        idx = np.nonzero(prg == g)[0]
        j = np.zeros(1, dtype=miphy.PrecodeJob)[0]
        j["nof_re"], j["nof_layers"], j["nof_ports"], j["weights_offset"] = idx.size, L, P, g * P * L
        j["in_offset"], j["in_stride"], j["out_offset"], j["out_stride"] = io, idx.size, oo, idx.size
        jobs.append(j), xin.append(x[:, idx].reshape(-1)), where.append((idx, oo))
        io += L * idx.size
        oo += P * idx.size
    out = torch.zeros(oo, dtype=torch.complex64, device="cuda")
    ctx.channel_precode_batch(np.array(jobs, dtype=miphy.PrecodeJob), pc["W"].reshape(-1), torch.from_numpy(np.concatenate(xin)).cuda(), out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    composed = _inner(bg, pc).copy()
    for idx, o in where:
        composed[np.asarray(pc["ports"])[:, None], sy[idx][None, :], col[idx][None, :]] = out[o:o + P * idx.size].reshape(P, idx.size)
    diff = int((D.bits(_inner(got, pc)) != D.bits(composed)).sum())
    print("%s: %d words differ between the fused and the composed grid (%d PRGs)" % (name, diff, len(where)))
    assert diff == 0
    _check(pc, got, bg)


# ---------------------------------------------------------------------------------------------------- (d) PRG geometry
@pytest.mark.parametrize("prg_size, nof_prg", [(1, 275), (2, 138), (4, 69), (275, 1)], ids=["prg1", "prg2", "prg4", "wideband"])
def test_prg_geometry_on_scattered_prbs(ctx, prg_size, nof_prg):
    pc = XC.precoded(LC["f_scattered_L3_mod4"], 4, prg_size)
    assert pc["nof_prg"] == nof_prg and pc["W"].shape == (nof_prg, 4, 3)
    _check(pc, *_one(ctx, pc))


# ---------------------------------------------------------------------------------------------------- (e) mapping order
def _interleaved():
    out = []
    for L in (2, 4):
        kw = dict(start=1, nof=3, dmrs=(2,), cdm=1)
        out.append(XC.precoded(MC._mapped("prec_bundle2_L%d_mod4" % L, L, 4, 8, range(8), (2, 0, 8, 0), **kw), 4, 4))
        out.append(XC.precoded(MC._mapped("prec_bundle4_L%d_mod6" % L, L, 6, 16, range(16), (4, 0, 16, 0), **kw), 4, 2))
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
@pytest.mark.parametrize("pc", _interleaved(), ids=lambda pc: pc["name"])
def test_prg_follows_the_grid_prb_not_the_list(ctx, pc, on_device):
    c = pc["c"]
    assert list(c["prbs"]) != sorted(c["prbs"])
    got, bg = _one(ctx, pc, on_device)
    _check(pc, got, bg)
    # the statement with the PRG taken from the PRB's place in the list is another one, and the device does not meet it
    sy, col = XC.data_positions(c)
    place = np.argsort(c["prbs"].astype(int))[np.searchsorted(np.sort(c["prbs"].astype(int)), col // 12)]
    y, A = XC.precode_ref(pc["W"][place // pc["prg_size"]], PC.layer_symbols(c, exact=True))
    have = _inner(got, pc)[np.asarray(pc["ports"])[:, None], sy[None, :], col[None, :]]
    assert XC.excess(have, y, A, pc["L"])[0] > 1.0


# ---------------------------------------------------------------------------------------------------- (f) ports
def test_antenna_ports_on_grid_ports_out_of_order(ctx):
    pc = XC.precoded(LC["sweep_L2_mod4"], 4, 4, ports=(5, 0, 9, 2), grid_ports=10, tag="_ports")
    got, bg = _one(ctx, pc)
    _check(pc, got, bg)
    others = [p for p in range(10) if p not in pc["ports"]]
    assert len(others) == 6 and np.array_equal(D.bits(_inner(got, pc)[others]), D.bits(_inner(bg, pc)[others]))


# ---------------------------------------------------------------------------------------------------- (j) one layer
def test_one_layer_with_weight_one_equals_the_one_layer_entry_point(ctx):
    """L = 1, P = 1, W = 1 + 0j on the case's own port: the bytes miphy_pdsch_modulate_batch writes."""
    import torch
    import miphy
    ones = [c for c in PC.cases() if c["L"] == 1]
    assert {c["mod"] for c in ones} == {1, 2, 4, 6, 8}
    pcs = []
    for c in ones:
        pc = XC.precoded(c, 1, 4, ports=c["ports"], grid_ports=c["grid_ports"])
        pc["W"] = np.ones_like(pc["W"])
        pcs.append(pc)
    jobs, lists, w, grids, cw = _jobs(miphy, pcs)
    err, got = _run(ctx, jobs, lists, w, grids, cw)
    assert err is None, err
    one = np.zeros(len(ones), dtype=miphy.PdschModJob)
    for i, j in enumerate(jobs):
        one[i] = j["mapped"]["layers"]["base"]
        one[i]["port"] = ones[i]["ports"][0]
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_batch(one, torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(np.concatenate(got)), D.bits(gd.cpu().numpy()))
    assert not np.array_equal(D.bits(np.concatenate(got)), D.bits(np.concatenate(grids)))


# ---------------------------------------------------------------------------------------------------- (g) DM-RS
DMRS = XC.dmrs_cases()


def _dmrs_buffers(dcs):
    grids, goff, o = [], [], 0
    for k, dc in enumerate(dcs):
        grids.append(D.background(G + dc["grid_ports"] * 14 * dc["nprb_grid"] * 12 + G, np.random.default_rng(500 + k + len(dc["name"]))))
        goff.append(o + G)
        o += grids[-1].size
    return grids, goff


def _dmrs_run(ctx, dcs, on_device=False, edit=None):
    import torch
    import miphy
    grids, goff = _dmrs_buffers(dcs)
    w, woff = _weights(dcs)
    jobs = np.array([dmrs_precoded_job(miphy, dc, wo, go) for dc, wo, go in zip(dcs, woff, goff)], dtype=miphy.DmrsPdschPrecodedJob)
    if edit:
        edit(jobs, w)
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    err = None
    try:
        if on_device:
            ctx.dmrs_pdsch_map_precoded_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), torch.from_numpy(w).cuda(), gd)
        else:
            ctx.dmrs_pdsch_map_precoded_batch(jobs, w, gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return err, _split(gd.cpu().numpy(), grids), grids


def _dmrs_check(dc, got, bg):
    assert _guards_kept(got, bg), dc["name"]
    sy, col, y, A = XC.dmrs_statement(dc)
    x = dict(dc, c=dict(nprb_grid=dc["nprb_grid"]))  # (check_grid reads the grid's shape from a case)
    XC.check_grid(x, _inner(got, dc), _inner(bg, dc), sy, col, y, A, dc["name"])
    return sy, col


@pytest.mark.parametrize("dc", DMRS, ids=lambda d: d["name"])
def test_dmrs_within_the_contract(ctx, dc):
    """The union of the oracle's per-layer masks is written on every antenna port, within the tolerance; everything else -- the REs of a CDM group
    without a layer, the PRBs below the reference point, the ports of the grid that are no antenna port -- holds its background."""
    err, got, grids = _dmrs_run(ctx, [dc])
    assert err is None, err
    sy, col = _dmrs_check(dc, got[0], grids[0])
    if dc["L"] <= 2:  # CDM group 1 (and 2) are empty: nothing of them is in the written mask
        k = col % 12
        assert set(((k % 2) if not dc["type2"] else (k % 6) // 2).tolist()) == {0}


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_dmrs_in_one_batch(ctx, on_device):
    err, got, grids = _dmrs_run(ctx, DMRS, on_device)
    assert err is None, err
    for dc, g, bg in zip(DMRS, got, grids):
        _dmrs_check(dc, g, bg)


def test_dmrs_with_a_permutation_copies_the_dmrs_ports_bit_for_bit(ctx):
    """L = 4 of type 1 through the permutation (2, 0, 3, 1): antenna port sigma(ly) holds the bits miphy_dmrs_pdsch_map_batch writes for DM-RS port ly on
    the REs of its CDM group, and +-0 on those of the other group."""
    import torch
    import miphy
    dc = dict(next(d for d in DMRS if d["name"] == "dmrs_type1_L4_P4"))
    sigma = np.array([2, 0, 3, 1])
    dc["W"] = np.zeros_like(dc["W"])
    dc["W"][:, sigma, np.arange(4)] = 1.0
    err, got, grids = _dmrs_run(ctx, [dc])
    assert err is None, err
    plain = np.zeros(1, dtype=miphy.DmrsPdschJob)
    plain[0] = dmrs_precoded_job(miphy, dc, 0, G)["base"]
    plain[0]["ports"][:4] = sigma
    zeros = np.zeros_like(grids[0])
    gd = torch.from_numpy(zeros).cuda()
    ctx.dmrs_pdsch_map_batch(plain, gd)
    torch.cuda.synchronize()
    want, have = _inner(gd.cpu().numpy(), dc), _inner(got[0], dc)
    written = want != 0
    assert written.any() and np.array_equal(D.bits(have).reshape(written.shape + (2,))[written], D.bits(want).reshape(written.shape + (2,))[written])
    union = np.broadcast_to(written.any(axis=0), written.shape)
    assert ((D.bits(have).reshape(written.shape + (2,))[union & ~written] & 0x7FFFFFFF) == 0).all()
    assert np.array_equal(D.bits(have).reshape(written.shape + (2,))[~union], D.bits(_inner(grids[0], dc)).reshape(written.shape + (2,))[~union])


# ---------------------------------------------------------------------------------------------------- (h) processor
def _proc_pdus():
    """Two PDUs on disjoint PRBs of the 30-PRB, 4-port grid of tests/test_pdsch_mapped_gpu.py: L = 2, 64QAM, 6 PRBs with a list in another order; L = 4,
    256QAM, 24 PRBs without a list. Each with its precoding onto the four ports."""
    rng = np.random.default_rng(7741)
    out = []
    for L, prbs, listed, mod, bg, rv, dsyms, start, nof, prb0, bwp, (ddb, xdb), lbrm, aports, prg_size in (
            (2, [4, 5, 0, 1, 2, 3], True, 6, 2, 0, (3, 10), 2, 11, 0, (0, NPRB), (-3.0, 1.5), 3168, (2, 0, 3, 1), 4),
            (4, np.arange(6, 30), False, 8, 1, 0, (2, 7), 0, 14, 1, (6, 24), (3.0, -2.0), 3168, (0, 1, 2, 3), 2)):
        rb = np.zeros(NPRB, np.uint8)
        rb[np.asarray(prbs, int)] = 1
        p = dict(L=L, ports=list(range(L)), rb=rb, prbs=np.asarray(prbs, np.uint16), listed=listed, mod=mod, bg=bg, rv=rv, dmrs_symbols=dsyms, start=start, nof=nof,
                 ref_point_prb0=prb0, bwp=bwp, cdm=2, reserved=[], dmrs_dB=ddb, data_dB=xdb, lbrm_bytes=lbrm, slot=int(rng.integers(0, 20)),
                 rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), scr=int(rng.integers(0, 65536)), n_scid=int(rng.integers(0, 2)))
        p["nof_re"] = int(D.pdsch_data_mask(p).sum())
        p["tb"] = rng.integers(0, 256, min(3824 // 8 if bg == 2 else 10 ** 6, max(8, int(p["nof_re"] * L * mod * 0.4) // 8)), dtype=np.uint8)
        nof_prg = -(-NPRB // prg_size)
        p["pre"] = dict(L=L, P=4, prg_size=prg_size, nof_prg=nof_prg, ports=list(aports), W=XC.weights("processor %d" % L, (nof_prg, 4, L)))
        out.append(p)
    return out


def _proc_records(miphy, pdus):
    mapped, lists, tb = _mapped_records(miphy, pdus)
    w, woff = _weights([p["pre"] for p in pdus])
    rec = np.zeros(len(pdus), dtype=miphy.PdschPrecodedPdu)
    for r, m, p, wo in zip(rec, mapped, pdus, woff):
        r["mapped"] = m
        r["mapped"]["layers"]["ports"][:] = 0xFF  # ignored
        r["precoding"] = precoding_record(miphy, p["pre"], wo)
    return rec, lists, w, tb


def _proc_background():
    return D.background(G + NPORTS * 14 * NPRB * 12 + G, np.random.default_rng(810))


def _proc_chain(ctx, miphy, pdus, rec, lists, w, tb):
    """miphy_pdsch_encode_batch -> miphy_pdsch_modulate_precoded_batch -> miphy_dmrs_pdsch_map_precoded_batch with what the processor derives from the PDUs."""
    import torch
    td = np.zeros(len(pdus), dtype=miphy.PdschTbDesc)
    mj = np.zeros(len(pdus), dtype=miphy.PdschModPrecodedJob)
    dj = np.zeros(len(pdus), dtype=miphy.DmrsPdschPrecodedJob)
    cw_off = 0
    for i, (p, r) in enumerate(zip(pdus, rec)):
        L, b = p["L"], r["mapped"]["layers"]["base"]
        td[i] = (p["bg"], p["rv"], p["mod"], L, p["lbrm_bytes"] * 8, p["nof_re"] * L, p["tb"].size, int(b["tb_offset"]), cw_off)
        c = dict(name="pdu", L=L, mod=p["mod"], nprb_grid=NPRB, prbs=p["prbs"], start=p["start"], nof=p["nof"], dmrs=p["dmrs_symbols"], type2=0, cdm=p["cdm"], bwp=p["bwp"],
                 reserved=[], ports=p["ports"], grid_ports=NPORTS, scaling=D.db_to_amplitude(-p["data_dB"]), cw_pad=0, rnti=p["rnti"], n_id=p["n_id"])
        assert PC.nof_re(c) == p["nof_re"]
        mj[i]["mapped"]["layers"] = mod_layers_job(miphy, c, cw_off=cw_off, grid_off=G)
        mj[i]["mapped"]["prb_list_offset"], mj[i]["mapped"]["nof_prb"] = r["mapped"]["prb_list_offset"], r["mapped"]["nof_prb"]
        mj[i]["precoding"] = dj[i]["precoding"] = r["precoding"]
        d = dj[i]["base"]
        d["slot_in_frame"], d["reference_point_k_rb"], d["scrambling_id"] = p["slot"], p["bwp"][0] if p["ref_point_prb0"] else 0, p["scr"]
        d["amplitude"], d["dmrs_type"], d["n_scid"], d["nof_ports"] = D.db_to_amplitude(-p["dmrs_dB"]), 1, p["n_scid"], L
        d["symbols_mask"], d["grid_nof_prb"], d["rb_mask"], d["grid_offset"] = b["dmrs_symbols_mask"], NPRB, b["rb_mask"], G
        cw_off += (p["nof_re"] * L * p["mod"] + 15) // 16 * 16
    cw_d = torch.zeros(cw_off + 64, dtype=torch.uint8, device="cuda")
    gd = torch.from_numpy(_proc_background()).cuda()
    ctx.pdsch_encode_batch(td, torch.from_numpy(tb).cuda(), cw_d)
    ctx.pdsch_modulate_precoded_batch(mj, lists, w, cw_d, gd)
    ctx.dmrs_pdsch_map_precoded_batch(dj, w, gd)
    torch.cuda.synchronize()
    return gd.cpu().numpy()


def test_processor_equals_the_device_chain(ctx):
    import torch
    import miphy
    pdus = _proc_pdus()
    rec, lists, w, tb = _proc_records(miphy, pdus)
    assert int(rec[0]["mapped"]["nof_prb"]) == 6 and int(rec[1]["mapped"]["nof_prb"]) == 0
    bg = _proc_background()
    gd = torch.from_numpy(bg).cuda()
    ctx.pdsch_process_precoded_batch(rec, lists, w, torch.from_numpy(tb).cuda(), gd)
    torch.cuda.synchronize()
    got = gd.cpu().numpy()
    chain = _proc_chain(ctx, miphy, pdus, rec, lists, w, tb)
    diff = int((D.bits(got) != D.bits(chain)).sum())
    print("processor against the device chain: %d words differ" % diff)
    assert diff == 0 and _guards_kept(got, bg)
    inner, inner_bg = got[G:-G].reshape(NPORTS, 14, NPRB * 12), bg[G:-G].reshape(NPORTS, 14, NPRB * 12)
    for p in pdus:  # every antenna port was written on the PDU's PRBs, data and DM-RS symbols alike, and nothing outside its time allocation
        cols = np.repeat(p["rb"] != 0, 12)
        sym = np.zeros(14, bool)
        sym[p["start"]:p["start"] + p["nof"]] = True
        block = D.bits(inner[:, sym][:, :, cols]) != D.bits(inner_bg[:, sym][:, :, cols])
        assert block.reshape(NPORTS, int(sym.sum()), -1).any(axis=2).all()
        assert np.array_equal(D.bits(inner[:, ~sym][:, :, cols]), D.bits(inner_bg[:, ~sym][:, :, cols]))


# ---------------------------------------------------------------------------------------------------- (i) rules
def _pset(field, value):
    return lambda p, nw: p.__setitem__(field, value)


def _ports(idx, value):
    return lambda p, nw: p["ports"].__setitem__(idx, value)


def _weights_beyond(p, nw):
    p["weights_offset"] = nw - int(p["nof_prg"]) * int(p["nof_ports"]) * int(p["nof_layers"]) + 1


# One break per rule of a precoding, for a job of two layers on four ports: (what to break, the rule's message)
RULES = [(_pset("nof_layers", 0), "precoding: invalid number of layers 0"), (_pset("nof_layers", 5), "precoding: invalid number of layers 5"),
         (_pset("nof_layers", 1), "precoding: 1 layers for a job of 2"), (_pset("nof_ports", 1), "precoding: invalid number of antenna ports 1 (2..16)"),
         (_pset("nof_ports", 17), "precoding: invalid number of antenna ports 17"), (lambda p, nw: p["ports"].__setitem__(3, p["ports"][0]), "distinct grid ports below 16"),
         (_ports(1, 16), "distinct grid ports below 16"), (_pset("prg_size", 0), "precoding: invalid PRG size 0"), (_pset("nof_prg", 0), "number of PRGs 0"),
         (_pset("nof_prg", 1), "1 PRGs of 4 PRBs do not reach PRB"), (_weights_beyond, "exceed the")]
RULE_IDS = ["layers_0", "layers_5", "layers_not_the_jobs", "ports_below_layers", "ports_17", "ports_shared", "port_16", "prg_size_0", "nof_prg_0", "prgs_short_of_rb_mask",
            "weights_beyond_array"]


def _rule_pcs():
    """The job to break between two good ones: sweep_L2_mod4 (PRBs 1, 2, 4 of six) on four ports with two PRGs of 4 -- one PRG less does not reach PRB 4."""
    return [XC.precoded(LC["sweep_L3_mod6"], 3, 4), XC.precoded(LC["sweep_L2_mod4"], 4, 4, tag="_rule"), XC.precoded(LC["sweep_L4_mod8"], 8, 4)]


@pytest.mark.parametrize("k", range(len(RULES)), ids=RULE_IDS)
def test_modulator_refuses_a_host_job_that_breaks_a_precoding_rule(ctx, k):
    import miphy
    edit, msg = RULES[k]
    jobs, lists, w, grids, cw = _jobs(miphy, _rule_pcs())
    edit(jobs[1]["precoding"], w.size)
    err, got = _run(ctx, jobs, lists, w, grids, cw)
    assert err is not None and "miphy error -1" in err and "pdsch_modulate_precoded: job 1: " in err and msg in err, err
    for g, bg in zip(got, grids):
        assert np.array_equal(D.bits(g), D.bits(bg))


@pytest.mark.parametrize("k", range(len(RULES)), ids=RULE_IDS)
def test_modulator_skips_a_device_job_that_breaks_a_precoding_rule(ctx, k):
    import miphy
    edit, msg = RULES[k]
    pcs = _rule_pcs()
    jobs, lists, w, grids, cw = _jobs(miphy, pcs)
    edit(jobs[1]["precoding"], w.size)
    err, got = _run(ctx, jobs, lists, w, grids, cw, on_device=True)
    assert err is None, err
    assert np.array_equal(D.bits(got[1]), D.bits(grids[1]))
    _check(pcs[0], got[0], grids[0]), _check(pcs[2], got[2], grids[2])


def test_modulator_holds_a_precoded_job_to_the_rules_of_the_mapped_entry_point(ctx):
    """The job's own rules and the list rule reach the precoded entry point too: on the host with their messages, on the device by skipping."""
    import miphy
    pc = _interleaved()[0]
    for on_device in (False, True):
        for edit, msg in ((lambda j, l: j["mapped"]["layers"]["base"].__setitem__("mod", 3), "invalid modulation order 3"),
                          (lambda j, l: l.__setitem__(int(j["mapped"]["prb_list_offset"]) + 3, l[int(j["mapped"]["prb_list_offset"]) + 1]), "appears twice")):
            jobs, lists, w, grids, cw = _jobs(miphy, [pc])
            edit(jobs[0], lists)
            err, got = _run(ctx, jobs, lists, w, grids, cw, on_device)
            assert np.array_equal(D.bits(got[0]), D.bits(grids[0]))
            assert (err is None) if on_device else (err is not None and "miphy error -1" in err and "pdsch_modulate_precoded: job 0: " in err and msg in err), err


def _dmrs_rule_cases():
    by = {d["name"]: d for d in DMRS}
    return [by["dmrs_type1_L3_P3"], by["dmrs_type2_L2_P8"], by["dmrs_type1_L4_P4"]]


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
@pytest.mark.parametrize("k", range(len(RULES)), ids=RULE_IDS)
def test_dmrs_precoding_rules(ctx, k, on_device):
    """The middle job (two DM-RS ports onto eight antenna ports, PRGs of 4 over PRBs up to 9) breaks one rule: refused on the host with the rule's message
    and every grid at its background; skipped on the device, its neighbours written."""
    edit, msg = RULES[k]
    dcs = _dmrs_rule_cases()
    err, got, grids = _dmrs_run(ctx, dcs, on_device, lambda jobs, w: edit(jobs[1]["precoding"], w.size))
    if on_device:
        assert err is None, err
        assert np.array_equal(D.bits(got[1]), D.bits(grids[1]))
        _dmrs_check(dcs[0], got[0], grids[0]), _dmrs_check(dcs[2], got[2], grids[2])
    else:
        assert err is not None and "miphy error -1" in err and "dmrs_pdsch_map_precoded: job 1: " in err and msg in err, err
        for g, bg in zip(got, grids):
            assert np.array_equal(D.bits(g), D.bits(bg))


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_dmrs_job_with_five_ports_is_refused_or_skipped(ctx, on_device):
    def edit(jobs, w):
        jobs[1]["base"]["nof_ports"] = 5
        jobs[1]["precoding"]["nof_layers"] = 5
    dcs = _dmrs_rule_cases()
    err, got, grids = _dmrs_run(ctx, dcs, on_device, edit)
    assert np.array_equal(D.bits(got[1]), D.bits(grids[1]))
    assert (err is None) if on_device else ("miphy error -1" in err and "invalid number of DM-RS ports 5" in err), err


def _proc_edit_precoding(k):
    return lambda rec, lists, w: RULES[k][0](rec[0]["precoding"], w.size)


PROC_BREAKS = [(_proc_edit_precoding(k), RULES[k][1]) for k in range(len(RULES))] + [
    (lambda rec, lists, w: lists.__setitem__(int(rec[0]["mapped"]["prb_list_offset"]) + 3, lists[int(rec[0]["mapped"]["prb_list_offset"]) + 1]), "PRB list entry 3: PRB 5 appears twice"),
    (lambda rec, lists, w: rec[0]["mapped"].__setitem__("nof_prb", 5), "PRB list of 5 entries for the 6 PRBs of rb_mask"),
    (lambda rec, lists, w: rec[0]["mapped"]["layers"]["base"].__setitem__("mod", 3), "invalid modulation order 3"),
    (lambda rec, lists, w: rec[0]["mapped"]["layers"]["base"].__setitem__("rv", 4), "invalid redundancy version"),
    (lambda rec, lists, w: rec[0]["mapped"]["layers"].__setitem__("nof_layers", 5), "invalid number of layers 5"),
]
PROC_IDS = RULE_IDS + ["list_duplicate", "list_count", "modulation", "redundancy_version", "five_layers"]


@pytest.mark.parametrize("k", range(len(PROC_BREAKS)), ids=PROC_IDS)
def test_processor_refuses(ctx, k):
    """PDU 0 of the two (two layers on four ports, a list) breaks one rule of its precoding, of its list or of the mapped processor, behind a valid PDU 1 placed
    first: MIPHY_EINVAL with the rule's message before anything is enqueued, the grid at its background."""
    import torch
    import miphy
    edit, msg = PROC_BREAKS[k]
    pdus = _proc_pdus()
    rec, lists, w, tb = _proc_records(miphy, pdus)
    edit(rec, lists, w)
    rec = rec[::-1].copy()  # the broken PDU is PDU 1 of the call
    bg = _proc_background()
    gd = torch.from_numpy(bg).cuda()
    with pytest.raises(RuntimeError) as e:
        ctx.pdsch_process_precoded_batch(rec, lists, w, torch.from_numpy(tb).cuda(), gd)
    assert "miphy error -1" in str(e.value) and "pdsch_process_precoded: PDU 1: " in str(e.value) and msg in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))
