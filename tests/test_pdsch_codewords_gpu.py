"""GPU: PDSCH on two codewords and 5..8 layers -- miphy_pdsch_modulate_codewords_batch against o_pdsch_modulate with two codeword arguments (which
tests/test_pdsch_codewords.py holds to TS 38.211 in numpy), and miphy_pdsch_process_codewords_batch against the chain o_pdsch_encode per transport
block -> o_pdsch_modulate -> o_dmrs_pdsch_map on L ports. Every comparison is on the bits of buffers that start as dl_grid.background(), guard
elements and ports a job does not name included."""
import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O
import pdsch_codewords_cases as CC
import pdsch_layers_cases as PC
import pdsch_mapped_cases as MC
from test_pdsch_codewords import GARBAGE, mod_codewords_job
from test_pdsch_layers import _words

pytestmark = pytest.mark.gpu
CASES = CC.cases()
IDS = [c["name"] for c in CASES]
G = CC.GUARD


# ---------------------------------------------------------------------------------------------------- modulator
def _listed(c):
    """Whether the case's job carries its list: always where the order is not ascending, and on half of the others."""
    return list(c["prbs"]) != sorted(c["prbs"]) or len(c["name"]) % 2 == 0


def _buffers(cases):
    """Flat background [guard | grid | guard] per case, the codewords (one or two per case) at 16-byte slots plus their own byte offsets, the lists
    behind gaps of foreign entries, and the offsets."""
    grids, cws, lists, goff, coff, loff, g0, c0, l0 = [], [], [], [], [], [], 0, 0, 0
    for i, c in enumerate(cases):
        n = int(np.prod(PC.grid_shape(c)))
        bg = D.background(n + 2 * G, np.random.default_rng(len(c["name"]) + n))
        bg[G:G + n] = PC.background(c).reshape(-1)
        grids.append(bg)
        goff.append(g0 + G)
        g0 += bg.size
        offs = []
        for cw, pad in zip(CC.codewords(c), c["cw_pads"]) if "mods" in c else ((PC.codeword(c), c["cw_pad"]),):
            offs.append(c0 + pad)
            cws.append(np.concatenate([np.full(pad, 3, np.uint8), cw, np.full((-(pad + cw.size)) % 16 + 16, 3, np.uint8)]))
            c0 += cws[-1].size
        coff.append(tuple(offs) if len(offs) == 2 else (offs[0], 0))
        if _listed(c):
            gap = np.full(1 + i % 3, 0xFFFF, np.uint16)  # no PRB: an entry read from a gap breaks the rule
            lists += [gap, c["prbs"].astype(np.uint16)]
            loff.append(l0 + gap.size)
            l0 += gap.size + c["prbs"].size
        else:
            assert list(c["prbs"]) == sorted(c["prbs"])
            loff.append(None)
    lists.append(np.full(3, 0xFFFF, np.uint16))
    return grids, np.concatenate(cws), np.concatenate(lists), goff, coff, loff


def _jobs(miphy, cases):
    grids, cw, lists, goff, coff, loff = _buffers(cases)
    jobs = np.array([mod_codewords_job(miphy, c, lo, cw_offs=co, grid_off=go) for c, lo, co, go in zip(cases, loff, coff, goff)], dtype=miphy.PdschModCodewordsJob)
    return jobs, lists, grids, cw


def _run(ctx, jobs, lists, grids, cw, on_device=False):
    """One call; returns (error text or None, the list of the buffers [guard | grid | guard] afterwards)."""
    import torch
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    err = None
    try:
        if on_device:
            ctx.pdsch_modulate_codewords_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), torch.from_numpy(lists.view(np.int16).copy()).cuda(),
                                               torch.from_numpy(cw).cuda(), gd)
        else:
            ctx.pdsch_modulate_codewords_batch(jobs, lists, torch.from_numpy(cw).cuda(), gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    got, out, o = gd.cpu().numpy(), [], 0
    for g in grids:
        out.append(got[o:o + g.size])
        o += g.size
    return err, out


@pytest.fixture(scope="module")
def alone(ctx):
    """Every case in a call of its own (host jobs): computed once, shared and left unchanged."""
    import miphy
    out = {}
    for c in CASES:
        err, got = _run(ctx, *_jobs(miphy, [c]))
        assert err is None, (c["name"], err)
        out[c["name"]] = got[0]
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_modulator_matches_oracle(alone, c):
    """Bit-equal to o_pdsch_modulate with both codewords on a grid that already holds signals, guards and unnamed ports included."""
    bg = _buffers([c])[0][0]
    grid = bg[G:bg.size - G].reshape(PC.grid_shape(c)).copy()
    rc = CC.oracle_modulate(c, grid)
    want = bg.copy()
    want[G:bg.size - G] = grid.reshape(-1)
    diff = int((D.bits(alone[c["name"]]) != D.bits(want)).sum())
    print("%s: oracle returns %d for %d REs per layer; %d words differ" % (c["name"], rc, PC.nof_re(c), diff))
    assert rc == PC.nof_re(c)
    assert diff == 0
    assert not np.array_equal(D.bits(want), D.bits(bg))


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_one_batch_of_all_cases_equals_each_case_alone(ctx, alone, on_device):
    import miphy
    err, got = _run(ctx, *_jobs(miphy, CASES), on_device=on_device)
    assert err is None, err
    for c, g in zip(CASES, got):
        assert np.array_equal(D.bits(g), D.bits(alone[c["name"]])), c["name"]


ONE_CODEWORD = ("sweep_L1_mod4", "sweep_L3_mod6", "a_bpsk_L4", "c_L4_mod8", "d_L2_mod4_odd", "g_ports_2031_L4_mod2", "h_type2_cdm3_L2_mod8", "i_scaling_nan")


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_one_to_four_layers_equal_the_mapped_entry_point(ctx, on_device):
    """L = 1..4 through the new entry point writes the bytes miphy_pdsch_modulate_mapped_batch writes; mod1, nof_bits1 and cw1_offset hold garbage."""
    import torch
    import miphy
    ones = [c for c in PC.cases() if c["name"] in ONE_CODEWORD]
    assert len(ones) == len(ONE_CODEWORD) and {c["L"] for c in ones} == {1, 2, 3, 4}
    jobs, lists, grids, cw = _jobs(miphy, ones)
    assert (jobs["mod1"] == GARBAGE["mod1"]).all() and (jobs["cw1_offset"] == GARBAGE["cw1_offset"]).all()
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=on_device)
    assert err is None, err
    mj = jobs["mapped"].copy()
    for j, c in zip(mj, ones):
        j["layers"]["nof_layers"], j["layers"]["ports"] = c["L"], 0
        j["layers"]["ports"][:c["L"]] = c["ports"]
    gd = torch.from_numpy(np.concatenate(grids)).cuda()
    ctx.pdsch_modulate_mapped_batch(mj, lists, torch.from_numpy(cw).cuda(), gd)
    torch.cuda.synchronize()
    want = gd.cpu().numpy()
    assert np.array_equal(D.bits(np.concatenate(got)), D.bits(want)) and not np.array_equal(D.bits(want), D.bits(np.concatenate(grids)))


def _rule_case():
    return next(c for c in CASES if c["name"] == "b_L6_mod4_6")


def _edit(field, value):
    def edit(j):
        j[field] = value(j) if callable(value) else value
    return edit


def _port(k, value):
    def edit(j):
        j["ports"][k] = value
    return edit


def _base(field, value):
    def edit(j):
        j["mapped"]["layers"]["base"][field] = value(j) if callable(value) else value
    return edit


MOD_REJECTIONS = [  # one per new rule of the entry point: (what to break, the message)
    (_edit("nof_layers", 0), "invalid number of layers 0"), (_edit("nof_layers", 9), "invalid number of layers 9"),
    (_port(5, 0), "distinct grid ports below 16"), (_port(3, 16), "distinct grid ports below 16"),
    (_edit("mod1", 3), "invalid modulation order 3 of codeword 1"),
    (_edit("nof_bits1", lambda j: int(j["nof_bits1"]) + 1), "codeword 1 of"),
    (_base("nof_bits", lambda j: int(j["mapped"]["layers"]["base"]["nof_bits"]) - 1), "codeword 0 of"),
    (_base("mod", 3), "invalid modulation order 3"), (_base("n_id", 1024), "scrambling identifiers"),
]


@pytest.mark.parametrize("k", range(len(MOD_REJECTIONS)))
def test_modulator_rejects_host_jobs(ctx, k):
    """MIPHY_EINVAL with the rule's message before anything is enqueued: the grid still holds its background."""
    import miphy
    edit, msg = MOD_REJECTIONS[k]
    jobs, lists, grids, cw = _jobs(miphy, [CASES[0], _rule_case()])
    edit(jobs[1])
    err, got = _run(ctx, jobs, lists, grids, cw)
    assert err is not None and "miphy error -1" in err and "pdsch_modulate_codewords: job 1: " in err and msg in err, err
    assert np.array_equal(D.bits(np.concatenate(got)), D.bits(np.concatenate(grids)))


def test_host_job_breaking_a_list_rule_is_refused(ctx):
    import miphy
    c = next(c for c in CASES if c["name"] == "i_interleaved_L5")
    jobs, lists, grids, cw = _jobs(miphy, [c])
    lists = lists.copy()
    lists[jobs[0]["mapped"]["prb_list_offset"] + 1] = lists[jobs[0]["mapped"]["prb_list_offset"]]
    err, got = _run(ctx, jobs, lists, grids, cw)
    assert err is not None and "miphy error -1" in err and "pdsch_modulate_codewords: job 0: " in err and "appears twice" in err, err
    assert np.array_equal(D.bits(got[0]), D.bits(grids[0]))


DEVICE_SKIPS = [_edit("nof_layers", 9), _port(5, 0), _edit("nof_bits1", lambda j: int(j["nof_bits1"]) + 1), _edit("mod1", 3),
                _base("nof_bits", lambda j: int(j["mapped"]["layers"]["base"]["nof_bits"]) - 1)]


@pytest.mark.parametrize("k", range(len(DEVICE_SKIPS)))
def test_device_job_breaking_a_rule_is_skipped_whole(ctx, alone, k):
    """Device-resident jobs reach the kernels unseen by the host. The bad job sits between two valid ones and aims, with another scaling, at the grid
    of the first: anything it stored of either codeword would show there; the valid jobs are written."""
    import miphy
    c, other = _rule_case(), CASES[0]
    jobs, lists, grids, cw = _jobs(miphy, [c, c, other])
    jobs[1]["mapped"]["layers"]["base"]["grid_offset"] = jobs[0]["mapped"]["layers"]["base"]["grid_offset"]
    jobs[1]["mapped"]["layers"]["base"]["scaling"] = 3.0
    DEVICE_SKIPS[k](jobs[1])
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=True)
    assert err is None, err
    assert np.array_equal(D.bits(got[0]), D.bits(alone[c["name"]]))
    assert np.array_equal(D.bits(got[1]), D.bits(grids[1]))  # the bad job's own grid: untouched too
    assert np.array_equal(D.bits(got[2]), D.bits(alone[other["name"]]))


def test_device_batch_of_bad_jobs_leaves_the_grid_untouched(ctx):
    import miphy
    c = _rule_case()
    jobs, lists, grids, cw = _jobs(miphy, [c] * len(DEVICE_SKIPS))
    for j, edit in zip(jobs, DEVICE_SKIPS):
        edit(j)
    err, got = _run(ctx, jobs, lists, grids, cw, on_device=True)
    assert err is None and np.array_equal(D.bits(np.concatenate(got)), D.bits(np.concatenate(grids)))


# ---------------------------------------------------------------------------------------------------- processor
NPRB, NPORTS = 52, 8


def _pdus():
    """Five PDUs on disjoint PRBs of one grid: L = 5 with (bg 1, 3 codeblocks, 16QAM, rv 0) + (bg 2, 1 codeblock, QPSK, rv 2) on the DM-RS pair
    (2, 3); L = 8 with (256QAM, 64QAM), both of several codeblocks, on the pairs (2, 3) and (10, 11); L = 6 with a list of interleaved bundles of 2;
    and, in the same batch, L = 2 without a list and L = 3 with one. Each transport block is a dict (bg, rv, mod, tb)."""
    rng = np.random.default_rng(5838)
    out = []
    for L, ports, prbs, listed, tbs, dsyms, start, nof, prb0, bwp, (ddb, xdb), lbrm in (
            (5, (4, 0, 2, 1, 3), np.arange(0, 20), False, ((1, 0, 4, 2200), (2, 2, 2, 400)), (2, 3), 0, 14, 0, (0, NPRB), (0.0, 0.0), 3168),
            (8, (7, 1, 3, 0, 2, 6, 5, 4), np.arange(20, 36), False, ((1, 0, 8, 5000), (1, 1, 6, 3000)), (2, 3, 10, 11), 0, 14, 0, (0, NPRB), (-3.0, 1.5), 3168),
            (6, (0, 5, 1, 4, 2, 3), MC.vrb_to_prb(2, 36, 10, 36), True, ((2, 0, 6, 300), (1, 3, 4, 700)), (3, 4), 2, 11, 1, (36, 10), (3.0, -2.0), 3168),
            (2, (6, 2), np.arange(46, 49), False, ((2, 2, 4, 60),), (2,), 1, 13, 0, (0, NPRB), (0.0, 0.0), 1200),
            (3, (1, 7, 0), np.array([51, 49, 50]), True, ((1, 0, 2, 40),), (2, 7), 0, 14, 0, (0, NPRB), (1.0, 0.0), 3168)):
        rb = np.zeros(NPRB, np.uint8)
        rb[np.asarray(prbs, int)] = 1
        p = dict(L=L, ports=list(ports), rb=rb, prbs=np.asarray(prbs, np.uint16), listed=listed, dmrs_symbols=dsyms, start=start, nof=nof, ref_point_prb0=prb0, bwp=bwp,
                 cdm=2, reserved=[], dmrs_dB=ddb, data_dB=xdb, lbrm_bytes=lbrm, slot=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65536)),
                 n_id=int(rng.integers(0, 1024)), scr=int(rng.integers(0, 65536)), n_scid=int(rng.integers(0, 2)))
        p["nof_re"] = int(D.pdsch_data_mask(p).sum())
        p["tbs"] = [dict(bg=bg, rv=rv, mod=mod, tb=rng.integers(0, 256, nbytes, dtype=np.uint8)) for bg, rv, mod, nbytes in tbs]
        out.append(p)
    assert list(out[2]["prbs"]) != sorted(out[2]["prbs"])
    return out


def _nof_codeblocks(t):
    B = t["tb"].size * 8 + (16 if t["tb"].size * 8 <= 3824 else 24)
    K = 8448 if t["bg"] == 1 else 3840
    return 1 if B <= K else -(-B // (K - 24))


def _o_process(p, grid):
    """o_pdsch_encode per transport block on its own layers -> o_pdsch_modulate(both codewords, the list) -> o_dmrs_pdsch_map(L ports) on grid
    [ports][14][nsc] in place; returns what the modulator returns."""
    Ls = [x for x in CC.split(p["L"]) if x]
    if "cws" not in p:
        p["cws"] = [O.o_pdsch_encode(t["bg"], t["rv"], t["mod"], p["lbrm_bytes"] * 8, Lq, p["nof_re"] * Lq, t["tb"]) for t, Lq in zip(p["tbs"], Ls)]
    dm = np.zeros(14, np.uint8)
    dm[list(p["dmrs_symbols"])] = 1
    rc = O.o_pdsch_modulate(p["rnti"], p["n_id"], D.db_to_amplitude(-p["data_dB"]), p["L"], [t["mod"] for t in p["tbs"]], p["cws"], p["start"], p["nof"], dm, 0, p["cdm"],
                            p["bwp"][0], p["bwp"][1], p["prbs"], p["reserved"], p["ports"], NPRB, grid)
    assert O.o_dmrs_pdsch_map(p["slot"], p["bwp"][0] if p["ref_point_prb0"] else 0, 0, p["scr"], p["n_scid"], D.db_to_amplitude(-p["dmrs_dB"]), dm, p["rb"], p["ports"],
                              grid) == 0
    return rc


def _fill_base(b, p, t, tb_off):
    b["slot_in_frame"], b["rnti"], b["n_id"], b["dmrs_scrambling_id"], b["tbs_lbrm_bytes"], b["tb_bytes"] = p["slot"], p["rnti"], p["n_id"], p["scr"], p["lbrm_bytes"], t["tb"].size
    b["ratio_pdsch_dmrs_to_sss_dB"], b["ratio_pdsch_data_to_sss_dB"] = p["dmrs_dB"], p["data_dB"]
    b["bg"], b["rv"], b["mod"], b["start_symbol"], b["nof_symbols"], b["port"] = t["bg"], t["rv"], t["mod"], p["start"], p["nof"], 15
    b["nof_cdm_groups_without_data"], b["n_scid"], b["ref_point_prb0"], b["nof_reserved"] = p["cdm"], p["n_scid"], p["ref_point_prb0"], 0
    b["dmrs_symbols_mask"] = sum(1 << s for s in p["dmrs_symbols"])
    b["grid_nof_prb"], b["bwp_start_rb"], b["bwp_size_rb"], b["rb_mask"] = NPRB, p["bwp"][0], p["bwp"][1], _words(p["rb"])
    b["tb_offset"], b["grid_offset"] = tb_off, G


def _records(miphy, pdus, mapped=False):
    """PdschCodewordsPdu records (mapped: PdschMappedPdu records of PDUs of one transport block), the list array and the transport blocks."""
    rec = np.zeros(len(pdus), dtype=miphy.PdschMappedPdu if mapped else miphy.PdschCodewordsPdu)
    tb_off, tbs, lists = 0, [], [np.full(1, 0xFFFF, np.uint16)]
    for r, p in zip(rec, pdus):
        m, offs = (r if mapped else r["mapped"]), []
        for t in p["tbs"]:
            offs.append(tb_off)
            tbs.append(np.concatenate([t["tb"], np.zeros((-t["tb"].size) % 16, np.uint8)]))
            tb_off += tbs[-1].size
        _fill_base(m["layers"]["base"], p, p["tbs"][0], offs[0])
        if p["listed"]:
            m["prb_list_offset"], m["nof_prb"] = sum(x.size for x in lists), p["prbs"].size
            lists.append(p["prbs"])
        if mapped:
            m["layers"]["nof_layers"] = p["L"]
            m["layers"]["ports"][:p["L"]] = p["ports"]
            continue
        m["layers"]["nof_layers"], m["layers"]["ports"] = 66, [88, 88, 88, 88]  # ignored
        r["nof_layers"], r["ports"] = p["L"], 222
        r["ports"][:p["L"]] = p["ports"]
        if len(p["tbs"]) == 2:
            t = p["tbs"][1]
            r["bg1"], r["rv1"], r["mod1"], r["tb_bytes1"], r["tb_offset1"] = t["bg"], t["rv"], t["mod"], t["tb"].size, offs[1]
        else:
            r["bg1"], r["rv1"], r["mod1"], r["tb_bytes1"], r["tb_offset1"] = 7, 9, 3, 10 ** 6, 1 << 40  # ignored
    return rec, np.concatenate(lists), np.concatenate(tbs + [np.zeros(16, np.uint8)])


def _grid_background():
    return D.background(G + NPORTS * 14 * NPRB * 12 + G, np.random.default_rng(810))


def _inner(buf):
    return buf[G:buf.size - G].reshape(NPORTS, 14, NPRB * 12)


def _process(c, rec, lists, tb, mapped=False):
    import torch
    gd = torch.from_numpy(_grid_background()).cuda()
    (c.pdsch_process_mapped_batch if mapped else c.pdsch_process_codewords_batch)(rec, lists, torch.from_numpy(tb).cuda(), gd)
    torch.cuda.synchronize()
    return gd.cpu().numpy()


@pytest.fixture(scope="module")
def processed(ctx):
    import miphy
    pdus = _pdus()
    rec, lists, tb = _records(miphy, pdus)
    return pdus, rec, lists, tb, _process(ctx, rec, lists, tb)


def test_processor_pdus_are_what_they_claim():
    pdus = _pdus()
    assert [p["L"] for p in pdus] == [5, 8, 6, 2, 3]
    assert [_nof_codeblocks(t) for t in pdus[0]["tbs"]] == [3, 1] and [(t["bg"], t["mod"], t["rv"]) for t in pdus[0]["tbs"]] == [(1, 4, 0), (2, 2, 2)]
    assert min(_nof_codeblocks(t) for t in pdus[1]["tbs"]) > 1 and [t["mod"] for t in pdus[1]["tbs"]] == [8, 6]
    assert pdus[0]["dmrs_symbols"] == (2, 3) and pdus[1]["dmrs_symbols"] == (2, 3, 10, 11)


def test_processor_batch_matches_oracle_chain(processed):
    import miphy
    pdus, rec, lists, tb, got = processed
    bg = _grid_background()
    assert np.array_equal(D.bits(got[:G]), D.bits(bg[:G])) and np.array_equal(D.bits(got[-G:]), D.bits(bg[-G:]))
    want = _inner(bg).copy()
    for p, r in zip(pdus, rec):  # the PDUs own disjoint PRBs: each is judged on its own columns
        rc = _o_process(p, want)
        assert miphy.pdsch_codewords_pdu_nof_re(r) == p["nof_re"] == rc
        cols = np.repeat(p["rb"] != 0, 12)
        diff = int((D.bits(_inner(got)[:, :, cols]) != D.bits(want[:, :, cols])).sum())
        print("L = %d: %d REs per layer, %d words differ" % (p["L"], rc, diff))
        assert diff == 0, p["L"]
        dm = np.zeros(14, bool)
        dm[list(p["dmrs_symbols"])] = True
        for port in p["ports"]:  # the DM-RS symbols of every port were written
            assert not np.array_equal(D.bits(_inner(got)[port][dm][:, cols]), D.bits(_inner(bg)[port][dm][:, cols]))
    assert np.array_equal(D.bits(_inner(got)), D.bits(want))


def test_processor_one_codeword_pdus_equal_the_mapped_entry_point(ctx, processed):
    """The PDUs of two and three layers, in a batch with the others, own the bytes miphy_pdsch_process_mapped_batch writes for them."""
    import miphy
    pdus, rec, lists, tb, got = processed
    ones = [p for p in pdus if p["L"] <= 4]
    assert len(ones) == 2
    mrec, mlists, mtb = _records(miphy, ones, mapped=True)
    want = _process(ctx, mrec, mlists, mtb, mapped=True)
    cols = np.repeat(sum(p["rb"] for p in ones) != 0, 12)
    assert np.array_equal(D.bits(_inner(got)[:, :, cols]), D.bits(_inner(want)[:, :, cols]))
    assert not np.array_equal(D.bits(_inner(want)[:, :, cols]), D.bits(_inner(_grid_background())[:, :, cols]))
    # ... and alone through the new entry point: the same buffer, byte for byte
    rec1, lists1, tb1 = _records(miphy, ones)
    assert np.array_equal(D.bits(_process(ctx, rec1, lists1, tb1)), D.bits(want))


def test_processor_result_is_independent_of_order_and_history(ctx, processed):
    """Bit-equal with the PDUs enqueued in the opposite order, and on a context that has run nothing before (the session's context has grown its
    workspaces under every other test), also after a larger batch of another shape on it."""
    import miphy
    pdus, rec, lists, tb, got = processed
    assert np.array_equal(D.bits(_process(ctx, rec[::-1].copy(), lists, tb)), D.bits(got))
    fresh = miphy.Context(0)
    try:
        assert np.array_equal(D.bits(_process(fresh, rec, lists, tb)), D.bits(got))
        big = np.concatenate([rec[1:2]] * 3 + [rec[3:4]] * 2)
        _process(fresh, big, lists, tb)
        assert np.array_equal(D.bits(_process(fresh, rec, lists, tb)), D.bits(got))
    finally:
        fresh.close()


def _pb(field, value):
    return lambda r: r["mapped"]["layers"]["base"].__setitem__(field, value)


def _few_res(r):
    """One PRB over the symbols 2..4 with the DM-RS pair (2, 3): 12 REs per layer, and 13 codeblocks in transport block 1."""
    b = r["mapped"]["layers"]["base"]
    b["rb_mask"], b["start_symbol"], b["nof_symbols"], b["tb_bytes"] = [1, 0, 0, 0, 0], 2, 3, 8
    r["bg1"], r["tb_bytes1"] = 1, 13000


PROC_REJECTIONS = [
    (lambda r: (r.__setitem__("bg1", 1), r.__setitem__("tb_bytes1", 54754)), "transport block of 54754 bytes"),  # 53 codeblocks in the second block only
    (lambda r: r.__setitem__("rv1", 4), "redundancy version"),
    (_pb("nof_cdm_groups_without_data", 1), "5 layers need 2 CDM groups without data"),
    (_pb("dmrs_symbols_mask", 1 << 2), "double-symbol DM-RS"),
    (_pb("dmrs_symbols_mask", 7 << 2), "double-symbol DM-RS"),
    (_few_res, "12 REs per layer cannot carry 13 codeblocks"),
    (lambda r: r.__setitem__("mod1", 3), "modulation"),
    # (a rule of the PDU itself, which every processor states as "pdsch_process: PDU <i>: ...": transport block 1 is refused in the same words)
    (lambda r: r.__setitem__("bg1", 3), "pdsch_process: PDU 1: invalid base graph"),
    (lambda r: r.__setitem__("nof_layers", 9), "number of layers"), (lambda r: r.__setitem__("nof_layers", 0), "number of layers"),
    (lambda r: r["ports"].__setitem__(4, r["ports"][0]), "distinct grid ports below 16"),
]


@pytest.mark.parametrize("k", range(len(PROC_REJECTIONS)))
def test_processor_rejects(ctx, k):
    """MIPHY_EINVAL for a batch whose second PDU (the one of five layers) breaks one rule, before anything is enqueued: the grid still holds its
    background."""
    import torch
    import miphy
    edit, msg = PROC_REJECTIONS[k]
    pdus = _pdus()
    rec, lists, tb = _records(miphy, [pdus[3], pdus[0]])
    edit(rec[1])
    bg = _grid_background()
    gd = torch.from_numpy(bg).cuda()
    with pytest.raises(RuntimeError, match=msg) as e:
        ctx.pdsch_process_codewords_batch(rec, lists, torch.from_numpy(tb).cuda(), gd)
    assert "miphy error -1" in str(e.value) and ("pdsch_process_codewords: PDU 1: " in str(e.value) or msg.startswith("pdsch_process: ")), str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))


def test_processor_refuses_on_a_context_that_has_run_nothing(processed):
    """The refused call must not need workspaces: a context without any refuses the batch alike, and then processes the intact one to the same bits."""
    import torch
    import miphy
    pdus, rec, lists, tb, got = processed
    bad = rec.copy()
    bad[-1]["rv1"], bad[1]["rv1"] = 4, 4  # (ignored in the PDU of one transport block, refused in the other)
    bg = _grid_background()
    gd = torch.from_numpy(bg).cuda()
    fresh = miphy.Context(0)
    try:
        with pytest.raises(RuntimeError, match="PDU 1: invalid redundancy version"):
            fresh.pdsch_process_codewords_batch(bad, lists, torch.from_numpy(tb).cuda(), gd)
        torch.cuda.synchronize()
        assert np.array_equal(D.bits(gd.cpu().numpy()), D.bits(bg))
        assert np.array_equal(D.bits(_process(fresh, rec, lists, tb)), D.bits(got))
    finally:
        fresh.close()
