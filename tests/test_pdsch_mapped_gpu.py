"""GPU: PDSCH with the PRBs of a job in mapping order (interleaved VRB-to-PRB mapping, TS 38.211 7.3.1.6) -- miphy_pdsch_modulate_mapped_batch
against o_pdsch_modulate, which walks its prb_list as given (tests/test_pdsch_mapped.py checks with the oracle alone that this states "the i-th data
RE in list order carries x^(ly)(i)"), with host jobs and with device-resident jobs and lists; the list rule, host and device; and
miphy_pdsch_process_mapped_batch against the chain o_pdsch_encode -> o_pdsch_modulate(list) -> o_dmrs_pdsch_map(mask). Every comparison is on the
bits of buffers that start as dl_grid.background(), guard elements and ports a job does not name included."""
import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O
import pdsch_layers_cases as PC
import pdsch_mapped_cases as MC
from test_pdsch_layers import _words
from test_pdsch_layers_gpu import _buffers
from test_pdsch_mapped import mod_mapped_job

pytestmark = pytest.mark.gpu
CASES = MC.cases()
IDS = [c["name"] for c in CASES]
SMALL = MC.small(CASES)
G = PC.GUARD


# ---------------------------------------------------------------------------------------------------- modulator
def _lists(cases, with_list):
    """The list array of a batch: the list of each case that has one behind a gap of 1, 2, 3, ... foreign entries, so that the offsets are odd and
    even; returns (array, offset per case or None)."""
    parts, offs, o = [], [], 0
    for i, (c, w) in enumerate(zip(cases, with_list)):
        if not w:
            offs.append(None)
            continue
        gap = np.full(1 + i % 3, 0xFFFF, np.uint16)  # no PRB: an entry read from a gap breaks the rule
        parts += [gap, c["prbs"].astype(np.uint16)]
        offs.append(o + gap.size)
        o += gap.size + c["prbs"].size
    parts.append(np.full(3, 0xFFFF, np.uint16))
    return np.concatenate(parts), offs


def _jobs(miphy, cases, with_list=None):
    with_list = [True] * len(cases) if with_list is None else with_list
    grids, cw, goff, coff = _buffers(cases)
    lists, loff = _lists(cases, with_list)
    jobs = np.array([mod_mapped_job(miphy, c, lo, cw_off=co, grid_off=go) for c, lo, go, co in zip(cases, loff, goff, coff)], dtype=miphy.PdschModMappedJob)
    return jobs, lists, grids, cw


def _run(ctx, jobs, lists, grids, cw, on_device=False):
    """One call; returns (error text or None, the list of the buffers [guard | grid | guard] afterwards)."""
    import torch
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    err = None
    try:
        if on_device:
            ctx.pdsch_modulate_mapped_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), torch.from_numpy(lists.view(np.int16).copy()).cuda(),
                                            torch.from_numpy(cw).cuda(), gd)
        else:
            ctx.pdsch_modulate_mapped_batch(jobs, lists, torch.from_numpy(cw).cuda(), gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    got, out, o = gd.cpu().numpy(), [], 0
    for g in grids:
        out.append(got[o:o + g.size])
        o += g.size
    return err, out


def _expected(c, prbs=None):
    """The buffer of the case alone after o_pdsch_modulate with the list (prbs: another order), and what the oracle returns."""
    bg = _buffers([c])[0][0]
    grid = bg[G:bg.size - G].reshape(PC.grid_shape(c)).copy()
    rc = PC.oracle_modulate(c if prbs is None else dict(c, prbs=prbs), grid)
    want = bg.copy()
    want[G:bg.size - G] = grid.reshape(-1)
    return want, rc


@pytest.fixture(scope="module")
def expected():
    """The oracle's buffer of every case: computed once, shared and left unchanged."""
    out = {}
    for c in CASES:
        want, rc = _expected(c)
        assert rc == PC.nof_re(c), c["name"]
        out[c["name"]] = want
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_modulator_matches_oracle(ctx, expected, c, on_device):
    """Bit-equal to o_pdsch_modulate with the list, on a grid that already holds signals, guards and unnamed ports included."""
    import miphy
    err, got = _run(ctx, *_jobs(miphy, [c]), on_device=on_device)
    assert err is None, err
    diff = int((D.bits(got[0]) != D.bits(expected[c["name"]])).sum())
    print("%s: %d words differ from the oracle's grid" % (c["name"], diff))
    assert diff == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_one_mixed_batch(ctx, expected, on_device):
    """All the small cases in one call, each list at its own offset (odd ones included), a job without a list in between: that one's grid is what
    miphy_pdsch_modulate_layers_batch writes for it, the others' the oracle's."""
    import miphy
    mid = len(SMALL) // 2
    cases = SMALL[:mid] + [SMALL[0]] + SMALL[mid:]
    with_list = [True] * mid + [False] + [True] * (len(SMALL) - mid)
    jobs, lists, grids, cw = _jobs(miphy, cases, with_list)
    assert {int(j["prb_list_offset"]) % 2 for j in jobs if j["nof_prb"]} == {0, 1} and int(jobs[mid]["nof_prb"]) == 0
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=on_device)
    assert err is None, err
    for i, (c, g) in enumerate(zip(cases, got)):
        if i != mid:
            assert np.array_equal(D.bits(g), D.bits(expected[c["name"]])), c["name"]
    layered = _layers_call(ctx, miphy, [cases[mid]])[0]
    assert np.array_equal(D.bits(got[mid]), D.bits(layered))
    assert not np.array_equal(D.bits(layered), D.bits(expected[cases[mid]["name"]]))  # (the ascending grid is another one)
    assert np.array_equal(D.bits(layered), D.bits(_expected(cases[mid], np.sort(cases[mid]["prbs"]))[0]))


def _layers_call(ctx, miphy, cases):
    import torch
    jobs, lists, grids, cw = _jobs(miphy, cases, [False] * len(cases))
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_layers_batch(np.ascontiguousarray(jobs["layers"]), torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    got, out, o = gd.cpu().numpy(), [], 0
    for g in grids:
        out.append(got[o:o + g.size])
        o += g.size
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_batch_without_lists_equals_the_layered_entry_point(ctx, on_device):
    import miphy
    jobs, lists, grids, cw = _jobs(miphy, SMALL, [False] * len(SMALL))
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=on_device)
    assert err is None, err
    want = _layers_call(ctx, miphy, SMALL)
    for c, g, w, bg in zip(SMALL, got, want, grids):
        assert np.array_equal(D.bits(g), D.bits(w)), c["name"]
        assert not np.array_equal(D.bits(g), D.bits(bg)), c["name"]
    # ... and with no list array at all
    import torch
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_mapped_batch(jobs, None, torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(np.concatenate(want)))


# ---- the list rule. The case is partial_bundles_L3_mod4: list [12 13 14 15 8 9 10 11 16 17 18] on a grid of 30 PRBs
def _rule_case():
    return next(c for c in CASES if c["name"] == "partial_bundles_L3_mod4")


def _dup(j, lists):
    lists[int(j["prb_list_offset"]) + 5] = lists[int(j["prb_list_offset"]) + 2]  # 14 twice, 9 missing


def _beyond_grid(j, lists):
    lists[int(j["prb_list_offset"]) + 4] = 30  # PRB 30 of a grid of 30 in place of 8


def _outside_mask(j, lists):
    lists[int(j["prb_list_offset"]) + 4] = 7  # PRB 7 in place of 8: inside the grid, not in rb_mask


def _count(j, lists):
    j["nof_prb"] = int(j["nof_prb"]) - 1  # ten distinct allocated PRBs for a mask of eleven


def _beyond_array(j, lists):
    j["prb_list_offset"] = lists.size - int(j["nof_prb"]) + 1  # the last entry would lie behind the array


RULE_BREAKS = [(_dup, "PRB 14 appears twice"), (_beyond_grid, "PRB 30 outside the grid of 30 PRBs"), (_outside_mask, "PRB 7 is not in rb_mask"),
               (_count, "PRB list of 10 entries for the 11 PRBs of rb_mask"), (_beyond_array, "exceeds the")]
RULE_IDS = ["duplicate", "beyond_grid", "outside_mask", "count", "beyond_array"]


@pytest.mark.parametrize("k", range(len(RULE_BREAKS)), ids=RULE_IDS)
def test_host_job_breaking_a_list_rule_is_refused(ctx, k):
    """MIPHY_EINVAL with the rule's message before anything is enqueued: the grid still holds its background."""
    import miphy
    edit, msg = RULE_BREAKS[k]
    jobs, lists, grids, cw = _jobs(miphy, [_rule_case()])
    edit(jobs[0], lists)
    err, got = _run(ctx, jobs, lists, grids, cw)
    assert err is not None and "miphy error -1" in err and "pdsch_modulate_mapped: job 0: " in err and msg in err, err
    assert np.array_equal(D.bits(got[0]), D.bits(grids[0]))


@pytest.mark.parametrize("k", range(len(RULE_BREAKS)), ids=RULE_IDS)
def test_device_job_breaking_a_list_rule_is_skipped(ctx, expected, k):
    """The same breaks in a device-resident job between two good ones: its grid keeps the background, the neighbours match the oracle."""
    import miphy
    edit, msg = RULE_BREAKS[k]
    a, b = SMALL[1], SMALL[-1]
    jobs, lists, grids, cw = _jobs(miphy, [a, _rule_case(), b])
    edit(jobs[1], lists)
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=True)
    assert err is None, err
    assert np.array_equal(D.bits(got[1]), D.bits(grids[1]))
    assert np.array_equal(D.bits(got[0]), D.bits(expected[a["name"]])) and np.array_equal(D.bits(got[2]), D.bits(expected[b["name"]]))


# ---------------------------------------------------------------------------------------------------- processor
NPRB, NPORTS = 30, 4


def _pdus():
    """Three PDUs on disjoint PRBs of one grid of 30: the partial-bundle allocation on two layers (PRBs 8..18), the type-0 one on one layer moved to
    a region above it (PRBs 19..29 hold its VRBs 0, 1, 6, 7, 8 of a region of 11 at L = 2), and one without a list (PRBs 0..5)."""
    rng = np.random.default_rng(3816)
    out = []
    for L, ports, prbs, listed, mod, bg, rv, dsyms, start, nof, prb0, bwp, (ddb, xdb), lbrm in (
            (2, (1, 3), MC.vrb_to_prb(4, 5, 19, 5)[3:14], True, 4, 1, 0, (3, 10), 2, 11, 1, (5, 19), (-3.0, 1.5), 3168),
            (1, (2,), MC.vrb_to_prb(2, 19, 11, 19)[[0, 1, 6, 7, 8]], True, 6, 2, 2, (2,), 0, 14, 0, (0, NPRB), (0.0, 0.0), 1200),
            (3, (0, 2, 1), np.arange(0, 6), False, 2, 2, 0, (2, 7), 1, 13, 0, (0, NPRB), (3.0, -2.0), 3168)):
        rb = np.zeros(NPRB, np.uint8)
        rb[np.asarray(prbs, int)] = 1
        p = dict(L=L, ports=list(ports), rb=rb, prbs=np.asarray(prbs, np.uint16), listed=listed, mod=mod, bg=bg, rv=rv, dmrs_symbols=dsyms, start=start, nof=nof,
                 ref_point_prb0=prb0, bwp=bwp, cdm=2, reserved=[], dmrs_dB=ddb, data_dB=xdb, lbrm_bytes=lbrm, slot=int(rng.integers(0, 20)),
                 rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)), scr=int(rng.integers(0, 65536)), n_scid=int(rng.integers(0, 2)))
        p["nof_re"] = int(D.pdsch_data_mask(p).sum())
        p["tb"] = rng.integers(0, 256, min(3824 // 8 if bg == 2 else 10 ** 6, max(8, int(p["nof_re"] * L * mod * 0.4) // 8)), dtype=np.uint8)
        out.append(p)
    assert list(out[0]["prbs"]) == [12, 13, 14, 15, 8, 9, 10, 11, 16, 17, 18] and list(out[1]["prbs"]) == [19, 24, 27, 22, 23]
    return out


def _o_process(p, grid):
    """o_pdsch_encode(L) -> o_pdsch_modulate(list) -> o_dmrs_pdsch_map(mask) on grid [ports][14][nsc] in place; returns what the modulator returns."""
    c = dict(name="pdu", L=p["L"], mod=p["mod"], nprb_grid=NPRB, prbs=p["prbs"], start=p["start"], nof=p["nof"], dmrs=p["dmrs_symbols"], type2=0, cdm=p["cdm"],
             bwp=p["bwp"], reserved=p["reserved"], ports=p["ports"], grid_ports=NPORTS, scaling=D.db_to_amplitude(-p["data_dB"]), cw_pad=0, rnti=p["rnti"], n_id=p["n_id"])
    cw = O.o_pdsch_encode(p["bg"], p["rv"], p["mod"], p["lbrm_bytes"] * 8, p["L"], p["nof_re"] * p["L"], p["tb"])
    rc = PC.oracle_modulate(c, grid, cw)
    O.o_dmrs_pdsch_map(p["slot"], p["bwp"][0] if p["ref_point_prb0"] else 0, 0, p["scr"], p["n_scid"], D.db_to_amplitude(-p["dmrs_dB"]), PC.dmrs_mask(c), p["rb"],
                       p["ports"], grid)
    return rc


def _records(miphy, pdus):
    rec = np.zeros(len(pdus), dtype=miphy.PdschMappedPdu)
    tb_off, tbs, lists = 0, [], [np.full(1, 0xFFFF, np.uint16)]
    for r, p in zip(rec, pdus):
        b = r["layers"]["base"]
        b["slot_in_frame"], b["rnti"], b["n_id"], b["dmrs_scrambling_id"], b["tbs_lbrm_bytes"], b["tb_bytes"] = p["slot"], p["rnti"], p["n_id"], p["scr"], p["lbrm_bytes"], p["tb"].size
        b["ratio_pdsch_dmrs_to_sss_dB"], b["ratio_pdsch_data_to_sss_dB"] = p["dmrs_dB"], p["data_dB"]
        b["bg"], b["rv"], b["mod"], b["start_symbol"], b["nof_symbols"], b["port"] = p["bg"], p["rv"], p["mod"], p["start"], p["nof"], 15
        b["nof_cdm_groups_without_data"], b["n_scid"], b["ref_point_prb0"], b["nof_reserved"] = p["cdm"], p["n_scid"], p["ref_point_prb0"], 0
        b["dmrs_symbols_mask"] = sum(1 << s for s in p["dmrs_symbols"])
        b["grid_nof_prb"], b["bwp_start_rb"], b["bwp_size_rb"], b["rb_mask"] = NPRB, p["bwp"][0], p["bwp"][1], _words(p["rb"])
        b["tb_offset"], b["grid_offset"] = tb_off, G
        r["layers"]["nof_layers"] = p["L"]
        r["layers"]["ports"][:p["L"]] = p["ports"]
        if p["listed"]:
            r["prb_list_offset"], r["nof_prb"] = sum(x.size for x in lists), p["prbs"].size
            lists.append(p["prbs"])
        tbs.append(np.concatenate([p["tb"], np.zeros((-p["tb"].size) % 16, np.uint8)]))
        tb_off += tbs[-1].size
    return rec, np.concatenate(lists), np.concatenate(tbs + [np.zeros(16, np.uint8)])


def _grid_background():
    return D.background(G + NPORTS * 14 * NPRB * 12 + G, np.random.default_rng(809))


def _inner(buf):
    return buf[G:buf.size - G].reshape(NPORTS, 14, NPRB * 12)


def test_processor_batch_matches_oracle_chain(ctx):
    """Three PDUs in one call; the DM-RS REs are part of the comparison."""
    import torch
    import miphy
    pdus = _pdus()
    assert list(pdus[1]["prbs"]) != sorted(pdus[1]["prbs"]) and list(pdus[0]["prbs"]) != sorted(pdus[0]["prbs"])
    rec, lists, tb = _records(miphy, pdus)
    bg = _grid_background()
    gd = torch.from_numpy(bg).cuda()
    ctx.pdsch_process_mapped_batch(rec, lists, torch.from_numpy(tb).cuda(), gd)
    torch.cuda.synchronize()
    got = gd.cpu().numpy()
    assert np.array_equal(D.bits(got[:G]), D.bits(bg[:G])) and np.array_equal(D.bits(got[-G:]), D.bits(bg[-G:]))
    want = _inner(bg).copy()
    for p, r in zip(pdus, rec):  # the PDUs own disjoint PRBs: each is judged on its own columns
        rc = _o_process(p, want)
        assert miphy.pdsch_layers_pdu_nof_re(r["layers"]) == p["nof_re"] == rc
        cols = np.repeat(p["rb"] != 0, 12)
        diff = int((D.bits(_inner(got)[:, :, cols]) != D.bits(want[:, :, cols])).sum())
        print("L = %d, list %s: %d words differ" % (p["L"], [int(x) for x in p["prbs"]] if p["listed"] else None, diff))
        assert diff == 0
        dm = np.zeros(14, bool)
        dm[list(p["dmrs_symbols"])] = True
        assert not np.array_equal(D.bits(_inner(got)[p["ports"][0]][dm][:, cols]), D.bits(_inner(bg)[p["ports"][0]][dm][:, cols]))  # the DM-RS symbols were written
    assert np.array_equal(D.bits(_inner(got)), D.bits(want))
    # the PDU without a list alone: the bytes miphy_pdsch_process_layers_batch writes
    one, _, tb1 = _records(miphy, pdus[2:])
    ga, gb = torch.from_numpy(bg).cuda(), torch.from_numpy(bg).cuda()
    ctx.pdsch_process_mapped_batch(one, None, torch.from_numpy(tb1).cuda(), ga)
    ctx.pdsch_process_layers_batch(np.ascontiguousarray(one["layers"]), torch.from_numpy(tb1).cuda(), gb)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(ga.cpu().numpy()), D.bits(gb.cpu().numpy())) and not np.array_equal(D.bits(ga.cpu().numpy()), D.bits(bg))


def test_processor_refuses_a_batch_with_a_duplicate_in_the_second_list(ctx):
    """MIPHY_EINVAL with the rule's message and the grid at its background, on a context that has run nothing before (its workspaces are not
    allocated yet: the refused call must not need them); the same context then processes the intact batch to the bits of the session's context.
    The workspace itself cannot be read through the interface: that nothing is enqueued or allocated before the last PDU and list have passed
    is the order of miphy_pdsch_process_mapped_batch, which this test can only witness from outside."""
    import torch
    import miphy
    pdus = _pdus()
    rec, lists, tb = _records(miphy, pdus)
    bad = lists.copy()
    o = int(rec[1]["prb_list_offset"])
    bad[o + 3] = bad[o + 1]
    bg = _grid_background()
    tb_d = torch.from_numpy(tb).cuda()
    good = torch.from_numpy(bg).cuda()
    ctx.pdsch_process_mapped_batch(rec, lists, tb_d, good)
    fresh = miphy.Context(0)
    try:
        gd = torch.from_numpy(bg).cuda()
        with pytest.raises(RuntimeError, match="pdsch_process_mapped: PDU 1: PRB list entry 3: PRB %d appears twice" % int(bad[o + 1])) as e:
            fresh.pdsch_process_mapped_batch(rec, bad, tb_d, gd)
        assert "miphy error -1" in str(e.value)
        torch.cuda.synchronize()
        assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))
        fresh.pdsch_process_mapped_batch(rec, lists, tb_d, gd)
        torch.cuda.synchronize()
        assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(good.cpu().numpy())) and not np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))
    finally:
        fresh.close()
