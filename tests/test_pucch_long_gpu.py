"""GPU: miphy_pucch_process_batch_ex, format-2 PDUs above 11 bits. The 23.5 reference refuses such a PDU, so the check is a
composition: the soft bits and the channel state information of a long PDU must be those miphy_pucch_process_batch (pinned to the
reference by test_pucch_proc_gpu.py) gives for the same allocation with a short payload, bit for bit, and payload and status must be
what the polar restatements (tests/uci_polar.py at list size 1, tests/uci_polar_list.py at 2 / 4 / 8) give on those downloaded soft
bits, bit for bit. The transmitter is tests/pucch_long_tx.py. The restatements run once per module.

Noise. With at most two DM-RS symbols the estimator replaces the noise variance by EPRE / 1000, so the demapper saturates and the decoder
sees nearly hard decisions; at a noise deviation of 0.3 and 0.6 per RE against unit-power Rayleigh gains per port, PDUs of every shape
but (12 bits, 512 soft bits) fall on both sides of the CRC. The conditions on the verdicts are asserted in
test_the_set_has_both_verdicts_in_each_crc_class."""
import ctypes as C
import functools

import numpy as np
import pytest

import miphy
import pucch_long_tx as LT
import pucch_tx as T
import uci_polar as U
import uci_polar_list as UL
from test_pucch_tx import FX

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_NPRB = 52
PORTS = (1, 2, 4)
LEVELS = (0.0, 0.3, 0.6)
LIST_SIZES = (1, 2, 4, 8)
PAY, LLR = 0xEE, 99  # sentinels
GRID_SEED = 600  # of the grids of shape_set(): chosen so that the conditions of test_the_set_has_both_verdicts_in_each_crc_class hold
# (start symbol, starting PRB) of the shapes of LT.SHAPES in a 52-PRB grid, and of the two silent PDUs behind them
PLACES = [(1, 0), (1, 2), (1, 5), (4, 30), (1, 7), (4, 33), (7, 1), (12, 36), (1, 16), (1, 18)]
SILENT = [(12, 2, 1), (40, 9, 1)]  # one per CRC class, in the grids of the first noise level


def split(K):
    """(HARQ-ACK, SR, CSI part 1) bit counts of a K-bit payload, each a uint8."""
    return (5, 1, K - 6) if K <= 261 else (K - 355, 100, 255)


def job_of(c, counts, grid_offset, payload_offset, llr_offset):
    j = np.zeros(1, miphy.PucchJob)[0]
    j["format"], j["numerology"], j["slot"], j["nof_ports"] = c[T.H_FMT], c[T.H_NUM], c[T.H_SLOT], c[T.H_NPORTS]
    j["start_symbol"], j["nof_symbols"], j["intra_slot_hopping"] = c[T.H_START], c[T.H_NSYM], c[T.H_HOP]
    j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"], j["second_hop_prb"] = c[T.H_BWP_START], c[T.H_BWP_SIZE], c[T.H_PRB], c[T.H_PRB2]
    j["nof_prb"], j["initial_cyclic_shift"], j["time_domain_occ"] = c[T.H_NPRB], c[T.H_ICS], c[T.H_OCC]
    j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"] = counts
    j["n_id"], j["n_id_0"], j["rnti"], j["grid_nprb"] = c[T.H_NID], c[T.H_NID0], c[T.H_RNTI], c[T.H_GRID_NPRB]
    j["grid_offset"], j["payload_offset"], j["llr_offset"] = grid_offset, payload_offset, llr_offset
    return j


def layout(pdus):
    """Payload and soft-bit offsets with sentinel bytes between the PDUs: (payload offsets, llr offsets, payload bytes, llr bytes)."""
    po, lo, p, l = [], [], 3, 1
    for d in pdus:
        po.append(p), lo.append(l)
        p += max(d["K"], 11) + 5
        l += d["E"] + 7
    return po, lo, p + 8, l + 8


def jobs_of(pdus, short=False):
    po, lo, npay, nllr = layout(pdus)
    jobs = np.zeros(len(pdus), miphy.PucchJob)
    for i, d in enumerate(pdus):
        jobs[i] = job_of(d["cfg"], (0, 0, 4) if short and d["K"] > 11 else d["counts"], d["grid_offset"], po[i], lo[i])
    return jobs, po, lo, npay, nllr


def run(ctx, jobs, grid_d, npay, nllr, L=None, with_llr=True):
    """(payload, result records, soft bits) after the old entry point (L None) or the new one at list size L."""
    n = len(jobs)
    pay = torch.full((npay,), PAY, dtype=torch.uint8, device="cuda")
    res = torch.full(((n + 2) * miphy.PucchResult.itemsize,), PAY, dtype=torch.uint8, device="cuda")
    llr = torch.full((nllr,), LLR, dtype=torch.int8, device="cuda")
    if L is None:
        ctx.pucch_process_batch(jobs, grid_d, pay, res, llr if with_llr else None)
    else:
        ctx.pucch_process_batch_ex(jobs, L, grid_d, pay, res, llr if with_llr else None)
    torch.cuda.synchronize()
    return pay.cpu().numpy(), res.cpu().numpy().view(miphy.PucchResult), llr.cpu().numpy()


CSI = ("epre_db", "rsrp_db", "sinr_db", "time_alignment_s")


def long_pdu(K, nprb, nsym, place, nports, grid_nprb, rng, on=True):
    c = LT.f2_cfg(nprb, nsym, place[0], place[1], grid_nprb, nports, rnti=int(rng.integers(1, 65520)), n_id=int(rng.integers(0, 1024)),
                  n_id_0=int(rng.integers(0, 65536)), slot=int(rng.integers(0, 20)))
    return dict(cfg=c, K=K, E=16 * nprb * nsym, counts=split(K), bits=rng.integers(0, 2, K).astype(np.uint8), on=on, nports=nports)


@functools.lru_cache(maxsize=None)
def shape_set():
    """Every shape of LT.SHAPES with 1, 2 and 4 ports in a noise-free grid and at two noise levels, one 52-PRB grid per (ports, level),
    plus one silent transmitter per CRC class in the grids of the first noise level. Returns (PDUs, flat grids)."""
    pdus, grids, off = [], [], 0
    for nports in PORTS:
        for lv, noise in enumerate(LEVELS):
            rng = np.random.default_rng(1000 * nports + lv)
            grp = [long_pdu(K, nprb, nsym, PLACES[i], nports, GRID_NPRB, rng) for i, (K, nprb, nsym) in enumerate(LT.SHAPES)]
            if lv == 1:
                grp += [long_pdu(K, nprb, nsym, PLACES[8 + i], nports, GRID_NPRB, rng, on=False) for i, (K, nprb, nsym) in enumerate(SILENT)]
            g = LT.build_grid(GRID_SEED + 10 * nports + lv, nports, GRID_NPRB, noise, [d["cfg"] for d in grp], [d["bits"] for d in grp], [d["on"] for d in grp])
            for d in grp:
                d["noise"], d["grid_offset"] = noise, off
            pdus += grp
            grids.append(g.ravel())
            off += g.size
    return pdus, np.concatenate(grids)


@pytest.fixture(scope="module")
def ref_set(ctx):
    """The set's soft bits and records from the OLD entry point on the same jobs with a short payload, and the restatements' payload and
    verdict on those soft bits at every list size."""
    pdus, grids = shape_set()
    grid_d = torch.from_numpy(grids).cuda()
    jobs, po, lo, npay, nllr = jobs_of(pdus, short=True)
    _, res, llr = run(ctx, jobs, grid_d, npay, nllr)
    ref = []
    for i, d in enumerate(pdus):
        soft = llr[lo[i]:lo[i] + d["E"]].copy()
        dec = {1: U.decode(d["K"], d["E"], soft)}
        for L in LIST_SIZES[1:]:
            dec[L] = UL.decode(d["K"], d["E"], soft, L)
        ref.append(dict(llr=soft, res=res[i].copy(), dec=dec))
    jobs, po, lo, npay, nllr = jobs_of(pdus)
    whole = run(ctx, jobs, grid_d, npay, nllr, 1)  # the whole set in one call of the new entry point
    return grid_d, ref, whole


def check_long(d, r, pay, res, llr, L, tag):
    """One long PDU's outputs (payload bytes from its offset, record, soft bits from its offset) against its reference r."""
    assert np.array_equal(llr[:d["E"]], r["llr"]), tag
    for k in CSI:
        assert res[k].tobytes() == r["res"][k].tobytes(), (tag, k)
    assert res["detection_metric"] == 0, tag
    want, valid = r["dec"][L]
    assert np.array_equal(pay[:d["K"]], want), (tag, int((pay[:d["K"]] != want).sum()))
    assert res["status"] == (U.STATUS_VALID if valid else U.STATUS_INVALID), (tag, int(res["status"]))
    if d["on"] and d["noise"] == 0.0:  # HARQ-ACK, SR, CSI part 1 in the order they were sent
        assert res["status"] == U.STATUS_VALID and np.array_equal(pay[:d["K"]], d["bits"]), tag


@pytest.mark.parametrize("nports", PORTS)
def test_every_shape_equals_the_short_run_and_the_polar_restatements(ctx, ref_set, nports):
    pdus, _ = shape_set()
    grid_d, ref, _ = ref_set
    sel = [i for i, d in enumerate(pdus) if d["nports"] == nports]
    assert len(sel) == 3 * len(LT.SHAPES) + len(SILENT)
    sub = [pdus[i] for i in sel]
    jobs, po, lo, npay, nllr = jobs_of(sub)
    touched_p, touched_l = np.zeros(npay, bool), np.zeros(nllr, bool)
    for k, d in enumerate(sub):
        touched_p[po[k]:po[k] + d["K"]] = True
        touched_l[lo[k]:lo[k] + d["E"]] = True
    for L in LIST_SIZES:
        pay, res, llr = run(ctx, jobs, grid_d, npay, nllr, L)
        for k, i in enumerate(sel):
            check_long(sub[k], ref[i], pay[po[k]:], res[k], llr[lo[k]:], L, (sub[k]["K"], sub[k]["E"], nports, sub[k]["noise"], sub[k]["on"], L))
        assert (pay[~touched_p] == PAY).all() and (llr[~touched_l] == LLR).all() and (res[len(sub):].view(np.uint8) == PAY).all()


def test_the_set_has_both_verdicts_in_each_crc_class(ref_set):
    pdus, _ = shape_set()
    _, ref, whole = ref_set
    assert [int(s) for s in whole[1][:len(pdus)]["status"]] == [U.STATUS_VALID if r["dec"][1][1] else U.STATUS_INVALID for r in ref]
    for crc6 in (True, False):
        v = [r["dec"][1][1] for d, r in zip(pdus, ref) if (d["K"] <= 19) == crc6]
        print("CRC%d: %d VALID, %d INVALID at list size 1" % (6 if crc6 else 11, sum(v), len(v) - sum(v)))
        assert sum(v) >= 3 and len(v) - sum(v) >= 3
    rescued = [(d["K"], d["E"], d["nports"], d["noise"]) for d, r in zip(pdus, ref) if d["K"] >= 20 and not r["dec"][1][1] and r["dec"][8][1]]
    print("INVALID at list size 1, VALID at 8:", rescued)
    assert rescued
    assert {(d["K"], d["cfg"][T.H_NPRB], d["cfg"][T.H_NSYM]) for d in pdus if d["on"]} == set(LT.SHAPES)


@functools.lru_cache(maxsize=None)
def mixed_group():
    """One 52-PRB, 4-port grid with format-1 PDUs on PRBs 0..3 (two of them sharing a PRB by their OCC), short and long format-2 PDUs
    on the PRBs behind, interleaved in the job order."""
    rng = np.random.default_rng(321)
    pdus = []

    def f1(prb, occ, nharq, nports):
        c = LT.f2_cfg(0, 14, 0, prb, GRID_NPRB, nports, 0, int(rng.integers(0, 1024)), 0, slot=7)
        c[T.H_FMT], c[T.H_OCC], c[T.H_ICS], c[T.H_NHARQ] = 1, occ, int(rng.integers(0, 12)), nharq
        return dict(cfg=c, K=nharq, E=0, counts=(nharq, 0, 0), bits=rng.integers(0, 2, max(nharq, 1)).astype(np.uint8) * (nharq > 0), on=True, nports=nports)

    def f2(K, nprb, nsym, place, nports):
        d = long_pdu(K, nprb, nsym, place, nports, GRID_NPRB, rng)
        if K <= 11:
            d["counts"] = (min(K, 2), 1 if K > 3 else 0, K - min(K, 2) - (1 if K > 3 else 0))
        return d

    longs = [f2(12, 2, 1, (0, 4), 4), f2(20, 2, 1, (0, 6), 2), f2(40, 9, 1, (0, 8), 1), f2(100, 16, 2, (2, 4), 4), f2(19, 3, 1, (0, 17), 3),
             f2(500, 16, 2, (4, 20), 2), f2(20, 3, 2, (6, 4), 1)]
    shorts = [f2(3, 1, 1, (0, 20), 4), f2(11, 2, 2, (2, 20), 2), f2(7, 16, 1, (8, 4), 1), f2(4, 1, 2, (9, 21), 3)]
    f1s = [f1(0, 0, 2, 4), f1(1, 1, 1, 2), f1(1, 2, 0, 2), f1(3, 0, 2, 1)]
    f1s[2]["cfg"][T.H_NID], f1s[2]["cfg"][T.H_ICS] = f1s[1]["cfg"][T.H_NID], f1s[1]["cfg"][T.H_ICS]
    pdus = [longs[0], f1s[0], shorts[0], longs[1], longs[2], f1s[1], shorts[1], longs[3], f1s[2], longs[4], shorts[2], longs[5], f1s[3],
            shorts[3], longs[6]]
    for d in pdus:
        d["grid_offset"], d["noise"] = 0, 0.3
    g = LT.build_grid(77, 4, GRID_NPRB, 0.3, [d["cfg"] for d in pdus], [[int(b) for b in d["bits"]] for d in pdus], [True] * len(pdus))
    return pdus, g.ravel()


def nbytes(d):
    return d["K"]  # payload bytes a PDU writes: K for format 2, nof_harq_ack for format 1


def test_mixed_batch_on_one_shared_grid(ctx):
    pdus, grid = mixed_group()
    grid_d = torch.from_numpy(grid).cuda()
    L = 4
    jobs, po, lo, npay, nllr = jobs_of(pdus)
    pay, res, llr = run(ctx, jobs, grid_d, npay, nllr, L)
    # the short and format-1 PDUs alone through the old entry point, at the same offsets
    keep = [i for i, d in enumerate(pdus) if d["cfg"][T.H_FMT] == 1 or d["K"] <= 11]
    assert len(keep) == 8 and len(pdus) - len(keep) == 7
    opay, ores, ollr = run(ctx, jobs[keep], grid_d, npay, nllr)
    for k, i in enumerate(keep):
        d = pdus[i]
        assert res[i].tobytes() == ores[k].tobytes(), i
        assert np.array_equal(pay[po[i]:po[i] + nbytes(d)], opay[po[i]:po[i] + nbytes(d)]), i
        assert np.array_equal(llr[lo[i]:lo[i] + d["E"]], ollr[lo[i]:lo[i] + d["E"]]), i
    # every PDU alone through the new entry point
    touched_p, touched_l = np.zeros(npay, bool), np.zeros(nllr, bool)
    for i, d in enumerate(pdus):
        apay, ares, allr = run(ctx, jobs[i:i + 1], grid_d, npay, nllr, L)
        assert res[i].tobytes() == ares[0].tobytes(), i
        assert np.array_equal(pay[po[i]:po[i] + nbytes(d)], apay[po[i]:po[i] + nbytes(d)]), i
        assert np.array_equal(llr[lo[i]:lo[i] + d["E"]], allr[lo[i]:lo[i] + d["E"]]), i
        touched_p[po[i]:po[i] + nbytes(d)] = True
        touched_l[lo[i]:lo[i] + d["E"]] = True
        if d["K"] > 11:  # and the long ones are what the restatement makes of their soft bits
            want, valid = UL.decode(d["K"], d["E"], llr[lo[i]:lo[i] + d["E"]], L)
            assert np.array_equal(pay[po[i]:po[i] + d["K"]], want) and res[i]["status"] == (U.STATUS_VALID if valid else U.STATUS_INVALID), i
    assert (pay[~touched_p] == PAY).all() and (llr[~touched_l] == LLR).all() and (res[len(pdus):].view(np.uint8) == PAY).all()
    assert sum(1 for i, d in enumerate(pdus) if d["K"] > 11 and res[i]["status"] == U.STATUS_VALID) >= 3


def test_whole_short_fixture_is_the_old_entry_point_byte_for_byte(ctx):
    from test_pucch_proc_gpu import device_grids, make_jobs
    fx = dict(np.load(FX))
    fx["grids"] = T.fixture_grids(fx)
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    jobs = make_jobs(fx, range(n), offs)
    old = run(ctx, jobs, grid_d, 11 * n + 8, 512 * n + 8)
    assert (old[1][:n]["status"] != PAY).all()
    for L in (1, 8):
        new = run(ctx, jobs, grid_d, 11 * n + 8, 512 * n + 8, L)
        for a, b in zip(old, new):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), L


def test_sentinels_and_no_llr_out(ctx, ref_set):
    pdus, _ = shape_set()
    grid_d, ref, _ = ref_set
    sel = [i for i, d in enumerate(pdus) if d["nports"] == 2 and d["noise"] == 0.6][::2] + [i for i, d in enumerate(pdus) if d["nports"] == 4 and d["noise"] == 0.3]
    sub = [pdus[i] for i in sel]
    jobs, po, lo, npay, nllr = jobs_of(sub)
    for L in (1, 8):
        pay, res, llr = run(ctx, jobs, grid_d, npay, nllr, L)
        touched_p, touched_l = np.zeros(npay, bool), np.zeros(nllr, bool)
        for k, d in enumerate(sub):
            touched_p[po[k]:po[k] + d["K"]] = True
            touched_l[lo[k]:lo[k] + d["E"]] = True
            check_long(d, ref[sel[k]], pay[po[k]:], res[k], llr[lo[k]:], L, (k, L))
        assert (pay[~touched_p] == PAY).all(), "payload bytes past K"
        assert (llr[~touched_l] == LLR).all(), "soft bits past E"
        assert (res[len(sub):].view(np.uint8) == PAY).all(), "records of other PDUs"
        pay2, res2, llr2 = run(ctx, jobs, grid_d, npay, nllr, L, with_llr=False)
        assert np.array_equal(pay, pay2) and np.array_equal(res.view(np.uint8), res2.view(np.uint8)) and (llr2 == LLR).all()
    # a call with PDUs in the middle of the result array: the records on either side stay as they were
    n = len(sub)
    pay = torch.full((npay,), PAY, dtype=torch.uint8, device="cuda")
    res = torch.full(((n + 2) * miphy.PucchResult.itemsize,), PAY, dtype=torch.uint8, device="cuda")
    ctx.pucch_process_batch_ex(jobs[2:5], 2, grid_d, pay, res[2 * miphy.PucchResult.itemsize:])
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(miphy.PucchResult)
    assert (r[:2].view(np.uint8) == PAY).all() and (r[5:].view(np.uint8) == PAY).all() and (r[2:5]["status"] != PAY).all()


def test_the_old_entry_point_still_skips_long_device_jobs(ctx):
    """Jobs the new entry point serves from host memory; as device jobs of the old one, the long ones are skipped (nothing of them is
    written) and the others come out as in the new call."""
    pdus, grid = mixed_group()
    grid_d = torch.from_numpy(grid).cuda()
    jobs, po, lo, npay, nllr = jobs_of(pdus)
    new = run(ctx, jobs, grid_d, npay, nllr, 1)
    old = run(ctx, torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), grid_d, npay, nllr)
    with pytest.raises(Exception):  # and as host jobs they are refused
        ctx.pucch_process_batch(jobs, grid_d, torch.zeros(npay, dtype=torch.uint8, device="cuda"),
                                torch.zeros(len(jobs) * miphy.PucchResult.itemsize, dtype=torch.uint8, device="cuda"))
    for i, d in enumerate(pdus):
        if d["K"] > 11:
            assert (old[1][i:i + 1].view(np.uint8) == PAY).all() and (old[0][po[i]:po[i] + d["K"]] == PAY).all(), i
            assert (old[2][lo[i]:lo[i] + d["E"]] == LLR).all() and new[1][i]["status"] in (U.STATUS_VALID, U.STATUS_INVALID), i
        else:
            assert old[1][i].tobytes() == new[1][i].tobytes() and np.array_equal(old[0][po[i]:po[i] + nbytes(d)], new[0][po[i]:po[i] + nbytes(d)]), i
            assert np.array_equal(old[2][lo[i]:lo[i] + d["E"]], new[2][lo[i]:lo[i] + d["E"]]), i


def test_a_call_of_several_pieces_equals_the_one_piece_call(ctx):
    """40 long PDUs of pairwise different (K, E), each in a noise-free one-port grid of its own, so 40 code blocks travel with the call."""
    rng = np.random.default_rng(55)
    pdus, grids, off, seen = [], [], 0, set()
    for i in range(52):
        nprb, nsym = 1 + (5 * i + 3) % 16, 1 + i % 2
        E = 16 * nprb * nsym
        K = 12 + i // 4 if i % 4 == 0 else 20 + 3 * i
        if U.info(K, E) is None or (K, E) in seen:  # (a few of the smallest allocations cannot carry their K)
            continue
        seen.add((K, E))
        d = long_pdu(K, nprb, nsym, (int(rng.integers(0, 13)), int(rng.integers(0, 17 - nprb))), 1, 16, rng)
        g = LT.build_grid(500 + i, 1, 16, 0.0, [d["cfg"]], [d["bits"]], [True])
        d["grid_offset"], d["noise"] = off, 0.0
        pdus.append(d), grids.append(g.ravel())
        off += g.size
    assert len(pdus) >= 36 and sum(1 for d in pdus if d["K"] <= 19) >= 5
    grid_d = torch.from_numpy(np.concatenate(grids)).cuda()
    jobs, po, lo, npay, nllr = jobs_of(pdus)
    one = run(ctx, jobs, grid_d, npay, nllr, 2)
    assert miphy.lib().miphy_debug_uci_polar_pieces() == 1
    for k, d in enumerate(pdus):
        assert one[1][k]["status"] == U.STATUS_VALID and np.array_equal(one[0][po[k]:po[k] + d["K"]], d["bits"]), (d["K"], d["E"])
    try:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(6000)
        many = run(ctx, jobs, grid_d, npay, nllr, 2)
        assert miphy.lib().miphy_debug_uci_polar_pieces() >= 5
        many_ws = run(ctx, jobs, grid_d, npay, nllr, 2, with_llr=False)
    finally:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(0)
    for a, b in zip(one, many):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(one[0], many_ws[0]) and np.array_equal(one[1].view(np.uint8), many_ws[1].view(np.uint8))


def _bad(field, value):
    def f(jobs):
        jobs[0][field] = value
    return f


def _bits(h, s, c, nprb=None, nsym=None):
    def f(jobs):
        jobs[0]["nof_harq_ack"], jobs[0]["nof_sr"], jobs[0]["nof_csi_part1"] = h, s, c
        if nprb:
            jobs[0]["nof_prb"], jobs[0]["nof_symbols"] = nprb, nsym
    return f


# (case, list size, argument replaced by NULL, change to the jobs, text of the rule)
REJECTIONS = [("list size 0", 0, None, None, "list size"), ("list size 3", 3, None, None, "list size"), ("list size 16", 16, None, None, "list size"),
              ("null context", 1, 0, None, "null argument"), ("null jobs", 1, 1, None, "null argument"), ("null grid", 1, 4, None, "null argument"),
              ("null payload", 1, 5, None, "null argument"), ("null results", 1, 6, None, "null argument"),
              ("five ports", 1, None, _bad("nof_ports", 5), "invalid PDU"), ("17 PRB", 2, None, _bad("nof_prb", 17), "invalid PDU"),
              ("format 3", 4, None, _bad("format", 3), "invalid PDU"), ("2 bits", 8, None, _bits(2, 0, 0), "invalid PDU"),
              ("hopping", 1, None, _bad("intra_slot_hopping", 1), "invalid PDU"), ("beyond the BWP", 1, None, _bad("starting_prb", 51), "invalid PDU"),
              ("CSI part 2 on a long PDU", 1, None, _bad("nof_csi_part2", 1), "CSI part 2"),
              ("CSI part 2 on a short PDU", 1, None, lambda jobs: (_bits(2, 1, 4)(jobs), _bad("nof_csi_part2", 3)(jobs)), "CSI part 2"),
              ("12 bits on 16", 1, None, _bits(5, 1, 6, 1, 1), "K_r + nPC < E_r"), ("21 bits on 32", 8, None, _bits(5, 1, 15, 2, 1), "K_r + nPC < E_r"),
              ("501 bits on 512", 2, None, _bits(200, 100, 201, 16, 2), "K_r + nPC < E_r")]


@pytest.mark.parametrize("case,L,null,change,rule", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections_write_nothing(ctx, case, L, null, change, rule):
    pdus, grid = mixed_group()
    grid_d = torch.from_numpy(grid).cuda()
    jobs, po, lo, npay, nllr = jobs_of(pdus[:4])  # long, format 1, short, long
    good = jobs.copy()
    if change:
        change(jobs)
    pay = torch.full((npay,), PAY, dtype=torch.uint8, device="cuda")
    res = torch.full((6 * miphy.PucchResult.itemsize,), PAY, dtype=torch.uint8, device="cuda")
    llr = torch.full((nllr,), LLR, dtype=torch.int8, device="cuda")

    def call(j, n, L, null=None):
        args = [ctx.h, C.c_void_p(j.ctypes.data), n, L, C.c_void_p(grid_d.data_ptr()), C.c_void_p(pay.data_ptr()), C.c_void_p(res.data_ptr()),
                C.c_void_p(llr.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        if null is not None:
            args[null] = None
        return miphy.lib().miphy_pucch_process_batch_ex(*args)

    assert call(jobs, jobs.size, L, null) == -1  # MIPHY_EINVAL
    assert rule in miphy.lib().miphy_last_error().decode(), miphy.lib().miphy_last_error().decode()
    if null is None:  # the binding raises on it
        with pytest.raises(Exception):
            ctx.pucch_process_batch_ex(jobs, L, grid_d, pay, res, llr)
    assert call(good, 0, 1) == 0  # n == 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((pay == PAY).all()) and bool((res == PAY).all()) and bool((llr == LLR).all())
    if case == "501 bits on 512":  # and the same buffers are taken with the jobs as they were
        assert call(good, good.size, L) == 0
        torch.cuda.synchronize()
        assert bool((res.cpu().view(torch.uint8)[:4 * miphy.PucchResult.itemsize:miphy.PucchResult.itemsize] != PAY).all())
        assert bool((res[4 * miphy.PucchResult.itemsize:] == PAY).all())
