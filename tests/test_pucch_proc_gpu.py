"""GPU: miphy_pucch_process_batch (csrc/pucch.hip) against tests/golden/pucch_processor.npz, recorded from the reference's own PUCCH
processor. The grids are rebuilt by tests/pucch_tx.py (their hashes are checked on the CPU by test_pucch_tx.py).

Tolerances. The reference's AVX2 ZF equaliser multiplies by an approximate reciprocal (about 12 bits), this kernel divides exactly, so
its equalised values differ by up to about 4e-4 relative. Summed over the PDU these errors do not cancel where the channel estimate
varies across the PRB (noisy cases): the format-1 detection metric is compared within 3e-3 relative, which is 1.7 times the largest
deviation of an exact-division restatement on this fixture, plus 1e-4 of the threshold for metrics near zero, and the status is not
compared where the reference metric is within 3e-3 of the threshold. The format-2 soft bits are compared within one step. EPRE and
RSRP do not go through the equaliser and are compared within 1e-4 relative, the SINR within 0.01 dB, the time alignment within 1.01
IDFT taps."""
import numpy as np
import pytest

import miphy
import pucch_tx as T
from test_pucch_tx import FX

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return miphy.Context(0)


@pytest.fixture(scope="module")
def fx():
    d = dict(np.load(FX))
    d["grids"] = T.fixture_grids(d)
    return d


def make_jobs(fx, idx, grid_off):
    """PucchJob records of the fixture cases idx; grid_off[g]: cf_t offset of group g's grid in the device buffer."""
    cfg = fx["cfg"]
    jobs = np.zeros(len(idx), miphy.PucchJob)
    for n, i in enumerate(idx):
        c = cfg[i]
        j = jobs[n]
        j["format"], j["numerology"], j["slot"], j["nof_ports"] = c[T.H_FMT], c[T.H_NUM], c[T.H_SLOT], c[T.H_NPORTS]
        j["start_symbol"], j["nof_symbols"], j["intra_slot_hopping"] = c[T.H_START], c[T.H_NSYM], c[T.H_HOP]
        j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"], j["second_hop_prb"] = c[T.H_BWP_START], c[T.H_BWP_SIZE], c[T.H_PRB], c[T.H_PRB2]
        j["nof_prb"], j["initial_cyclic_shift"], j["time_domain_occ"] = c[T.H_NPRB], c[T.H_ICS], c[T.H_OCC]
        j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"] = c[T.H_NHARQ], c[T.H_NSR], c[T.H_NCSI1]
        j["n_id"], j["n_id_0"], j["rnti"] = c[T.H_NID], c[T.H_NID0], c[T.H_RNTI]
        j["grid_nprb"] = c[T.H_GRID_NPRB]
        j["grid_offset"] = grid_off[fx["group"][i]]
        j["payload_offset"] = 11 * n
        j["llr_offset"] = 512 * n
    return jobs


def device_grids(fx, copies=1):
    flat = [g.ravel() for g in fx["grids"]] * copies
    offs = np.cumsum([0] + [f.size for f in flat])
    return torch.from_numpy(np.concatenate(flat)).cuda(), offs


def run(ctx, jobs, grid_d, on_device=False, llr_len=None, stream=None):
    n = len(jobs)
    pay = torch.full((max(11 * n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    res = torch.full((max(n, 1) * miphy.PucchResult.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    llr = torch.full((llr_len or max(512 * n, 1),), 99, dtype=torch.int8, device="cuda")
    j = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs
    ctx.pucch_process_batch(j, grid_d, pay, res, llr)
    torch.cuda.synchronize()
    return pay.cpu().numpy(), res.cpu().numpy().view(miphy.PucchResult)[:n], llr.cpu().numpy()


def check_case(fx, i, pay, r):
    """List of mismatches of case i (payload at pay[:11], result record r) against the reference."""
    cfg = fx["cfg"][i]
    err = []
    n = int(fx["payload_len"][i])
    metric_ref = float(fx["metric"][i])
    exempt = cfg[T.H_FMT] == 1 and abs(metric_ref - 1.0) < 3e-3
    if float(fx["rsrp_db"][i]) < float(fx["epre_db"][i]) - 90:
        # Users sharing a PRB in a noise-free grid while this one is silent: its least-squares estimate is the float rounding residue
        # of the others' cancelling signals, so only the verdict is meaningful.
        return [] if r["status"] == fx["status"][i] else ["status %d != %d" % (r["status"], fx["status"][i])]
    if not exempt:
        if r["status"] != fx["status"][i]:
            err.append("status %d != %d" % (r["status"], fx["status"][i]))
        if not np.array_equal(pay[:n], fx["payload"][i, :n]):
            err.append("payload %s != %s" % (pay[:n], fx["payload"][i, :n]))
    if cfg[T.H_FMT] == 1:
        if abs(r["detection_metric"] - metric_ref) > 3e-3 * abs(metric_ref) + 1e-4:  # absolute floor: 1e-4 of the threshold
            err.append("metric %.7g != %.7g" % (r["detection_metric"], metric_ref))
    for k in ("epre_db", "rsrp_db"):
        a, b = 10 ** (r[k] / 10.0), 10 ** (float(fx[k][i]) / 10.0)
        if not abs(a - b) <= 1e-4 * abs(b):
            err.append("%s %.7g != %.7g" % (k, r[k], fx[k][i]))
    sa, sb = float(r["sinr_db"]), float(fx["sinr_db"][i])
    if not (abs(sa - sb) <= 0.01 or (sa >= 60 and sb >= 60)):
        err.append("sinr %.5g != %.5g" % (sa, sb))
    tap = 1.0 / (4096 * 15e3 * (1 << int(cfg[T.H_NUM])))
    if not abs(float(r["time_alignment_s"]) - float(fx["ta_s"][i])) <= 1.01 * tap:
        err.append("ta %.4g != %.4g taps" % (r["time_alignment_s"] / tap, fx["ta_s"][i] / tap))
    return err


def test_fixture_every_case(ctx, fx):
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    jobs = make_jobs(fx, range(n), offs)
    jobs["llr_offset"] = fx["llr_offset"][:-1]
    pay, res, llr = run(ctx, jobs, grid_d, llr_len=int(fx["llr_offset"][-1]))
    bad = {}
    for i in range(n):
        e = check_case(fx, i, pay[11 * i:11 * i + 11], res[i])
        if e:
            bad[i] = e
    ref_llr = fx["llr"].astype(np.int64)
    got = llr[:ref_llr.size].astype(np.int64)
    d = np.abs(got - ref_llr)
    print("F1 metric max rel err %.3g" % max(abs(res[i]["detection_metric"] - fx["metric"][i]) / max(abs(fx["metric"][i]), 1e-30)
                                           for i in range(n) if fx["cfg"][i, T.H_FMT] == 1))
    print("F2 LLR max diff %d, identical %.5f" % (d.max(), (d == 0).mean()))
    assert not bad, "%d cases differ, e.g. %s" % (len(bad), list(bad.items())[:8])
    assert d.max() <= 1 and (d == 0).mean() >= 0.999


WIDE_NPRB, WIDE_PORTS = 273, 4


def wide_layout(fx, f1_copies):
    """Places the group grids into a stack of 273-PRB, 4-port slot grids, the rest of each slot grid random. A format-2 group keeps its
    absolute PRBs (its pilots depend on them) at a port offset, format-2 groups of one slot grid on disjoint ports; the format-1 groups,
    `f1_copies` times, follow side by side at PRB and port offsets of their own. Returns the stack and, per placed group,
    (group, slot, PRB offset, port offset)."""
    rng = np.random.default_rng(11)
    nsc = 12 * WIDE_NPRB
    grp_fmt = np.zeros(len(fx["grids"]), np.int32)
    grp_fmt[fx["group"]] = fx["cfg"][:, T.H_FMT]
    slots, place = [], []  # per slot: [ports used by format 2, PRB width of its format-2 region, PRB cursor of format 1]
    for g in np.nonzero(grp_fmt == 2)[0]:
        n, w = fx["grids"][g].shape[0], fx["grids"][g].shape[2] // 12
        sl = next((k for k, u in enumerate(slots) if u[0] + n <= WIDE_PORTS), None)
        if sl is None:
            slots.append([0, 0, 0])
            sl = len(slots) - 1
        place.append((int(g), sl, 0, slots[sl][0]))
        slots[sl][0] += n
        slots[sl][1] = slots[sl][2] = max(slots[sl][1], w)
    sl = 0
    for _ in range(f1_copies):
        for g in np.nonzero(grp_fmt == 1)[0]:
            n, w = fx["grids"][g].shape[0], fx["grids"][g].shape[2] // 12
            while sl < len(slots) and slots[sl][2] + w > WIDE_NPRB:
                sl += 1
            if sl == len(slots):
                slots.append([0, 0, 0])
            used = slots[sl][2]
            d = used + int(rng.integers(0, min(3, WIDE_NPRB - used - w) + 1))
            place.append((int(g), sl, d, int(rng.integers(0, WIDE_PORTS - n + 1))))
            slots[sl][2] = d + w
    shape = (len(slots), WIDE_PORTS, 14, nsc)
    wide = (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64) * 3
    for g, sl, d, q in place:
        grid = fx["grids"][g]
        wide[sl, q:q + grid.shape[0], :, 12 * d:12 * d + grid.shape[2]] = grid
    return wide, place


def test_wide_grid_batch_host_and_device_jobs(ctx, fx):
    """The fixture in one launch on 273-PRB, 4-port slot grids (wide_layout: format 1 twice, at PRB offsets through the BWP start, and
    format 2 at its absolute PRBs; all at port offsets through grid_offset), formats mixed in a shuffled order, once with host jobs and
    once with device jobs. Every PDU's results equal those of its case in the compact single-launch run."""
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    ref_pay, ref_res, ref_llr = run(ctx, make_jobs(fx, range(n), offs), grid_d)
    wide, place = wide_layout(fx, 2)
    assert wide.shape[0] < 400
    wide_d = torch.from_numpy(wide.ravel()).cuda()
    nsc = 12 * WIDE_NPRB
    cases = []
    for copy_idx, (g, sl, d, q) in enumerate(place):
        for i in np.nonzero(fx["group"] == g)[0]:
            cases.append((int(i), sl, d, q))
    order = np.random.default_rng(5).permutation(len(cases))
    jobs = np.zeros(len(cases), miphy.PucchJob)
    for k, t in enumerate(order):
        i, sl, d, q = cases[t]
        j = make_jobs(fx, [i], offs)[0]
        j["grid_offset"] = (sl * WIDE_PORTS + q) * 14 * nsc  # port offset q
        j["bwp_start_rb"] += d  # PRB offset d (0 for format 2)
        j["grid_nprb"] = WIDE_NPRB
        j["payload_offset"], j["llr_offset"] = 11 * k, 512 * k
        jobs[k] = j
    assert len(jobs) >= 1600
    for on_device in (False, True):
        pay, res, llr = run(ctx, jobs, wide_d, on_device=on_device)
        for k, t in enumerate(order):
            i = cases[t][0]
            m = int(fx["payload_len"][i])
            assert np.array_equal(pay[11 * k:11 * k + m], ref_pay[11 * i:11 * i + m]), (on_device, i)
            assert res[k].tobytes()[4:] == ref_res[i].tobytes()[4:] and res[k]["status"] == ref_res[i]["status"], (on_device, i)
            if fx["cfg"][i, T.H_FMT] == 2:
                e = 16 * int(fx["cfg"][i, T.H_NPRB]) * int(fx["cfg"][i, T.H_NSYM])
                assert np.array_equal(llr[512 * k:512 * k + e], ref_llr[512 * i:512 * i + e]), (on_device, i)


def test_one_and_zero(ctx, fx):
    grid_d, offs = device_grids(fx)
    for i in (0, len(fx["cfg"]) - 1):
        jobs = make_jobs(fx, [i], offs)
        jobs["llr_offset"] = 0
        pay, res, _ = run(ctx, jobs, grid_d)
        assert not check_case(fx, i, pay, res[0])
    pay = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    res = torch.full((24,), 7, dtype=torch.uint8, device="cuda")
    ctx.pucch_process_batch(np.zeros(0, miphy.PucchJob), grid_d, pay, res)
    torch.cuda.synchronize()
    assert (pay.cpu().numpy() == 7).all() and (res.cpu().numpy() == 7).all()


def test_skipped_device_jobs_and_unused_bytes_untouched(ctx, fx):
    grid_d, offs = device_grids(fx)
    cfg = fx["cfg"]
    i1 = int(np.nonzero((cfg[:, T.H_FMT] == 1) & (cfg[:, T.H_NHARQ] == 1))[0][0])
    i2 = int(np.nonzero(cfg[:, T.H_FMT] == 2)[0][0])
    jobs = make_jobs(fx, [i1, i2, i1, i2], offs)
    jobs["llr_offset"] = [0, 512, 1024, 1536]
    jobs[2]["nof_symbols"] = 3     # format 1 needs 4..14 symbols
    jobs[3]["nof_csi_part2"] = 1   # format 2 without CSI part 2
    pay, res, llr = run(ctx, jobs, grid_d, on_device=True)
    k2 = int(fx["payload_len"][i2])
    assert (pay[1:11] == 0xEE).all() and (pay[11 + k2:] == 0xEE).all()
    assert (res[2:].view(np.uint8) == 0xEE).all()
    assert (llr[:512] == 99).all() and (llr[1024:] == 99).all()
    m = 16 * int(cfg[i2, T.H_NPRB]) * int(cfg[i2, T.H_NSYM])
    assert (llr[512 + m:1024] == 99).all() and (llr[512:512 + m] != 99).any()
    assert not check_case(fx, i1, pay[0:11], res[0]) and not check_case(fx, i2, pay[11:22], res[1])


@pytest.mark.parametrize("field,value", [("format", 0), ("format", 3), ("nof_ports", 0), ("nof_ports", 5), ("nof_symbols", 3),
                                         ("nof_symbols", 15), ("start_symbol", 11), ("time_domain_occ", 7), ("nof_harq_ack", 3),
                                         ("starting_prb", 400), ("grid_nprb", 1), ("numerology", 5), ("slot", 20),
                                         ("initial_cyclic_shift", 12), ("n_id", 1024), ("occ_beyond_hop", None),
                                         ("f2_symbols", 3), ("f2_prb", 17), ("f2_hop", 1), ("f2_csi2", 1), ("f2_bits", 2),
                                         ("f2_bits", 12), ("f2_bwp", None)])
def test_invalid_host_jobs_rejected(ctx, fx, field, value):
    grid_d, offs = device_grids(fx)
    cfg = fx["cfg"]
    i1 = int(np.nonzero((cfg[:, T.H_FMT] == 1) & (cfg[:, T.H_NSYM] == 14) & (cfg[:, T.H_HOP] == 0))[0][0])
    i2 = int(np.nonzero((cfg[:, T.H_FMT] == 2) & (cfg[:, T.H_NHARQ] >= 1))[0][0])
    jobs = make_jobs(fx, [i1, i2], offs)
    if field == "occ_beyond_hop":
        jobs[0]["intra_slot_hopping"], jobs[0]["nof_symbols"], jobs[0]["time_domain_occ"] = 1, 4, 1
    elif field.startswith("f2_"):
        j = jobs[1]
        if field == "f2_symbols":
            j["nof_symbols"] = value
        elif field == "f2_prb":
            j["nof_prb"], j["bwp_size_rb"] = value, 32
        elif field == "f2_hop":
            j["intra_slot_hopping"] = 1
        elif field == "f2_csi2":
            j["nof_csi_part2"] = 1
        elif field == "f2_bits":
            j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"] = value, 0, 0
        else:
            j["starting_prb"] = j["bwp_size_rb"] - j["nof_prb"] + 1
    else:
        jobs[0][field] = value
    pay = torch.full((22,), 0xEE, dtype=torch.uint8, device="cuda")
    res = torch.full((48,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception):
        ctx.pucch_process_batch(jobs, grid_d, pay, res)
    torch.cuda.synchronize()
    assert (pay.cpu().numpy() == 0xEE).all() and (res.cpu().numpy() == 0xEE).all()


def test_graph_capture_replay(ctx, fx):
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    jobs = make_jobs(fx, range(n), offs)
    ref_pay, ref_res, _ = run(ctx, jobs, grid_d)
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    pay = torch.full((11 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * miphy.PucchResult.itemsize, dtype=torch.uint8, device="cuda")
    llr = torch.zeros(512 * n, dtype=torch.int8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.pucch_process_batch(jobs_d, grid_d, pay, res, llr, stream=s)  # warm-up (gold tables, staging)
    torch.cuda.synchronize()
    pay.fill_(0xEE), res.fill_(0xEE)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.pucch_process_batch(jobs_d, grid_d, pay, res, llr, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(pay.cpu().numpy(), ref_pay[:11 * n])
    assert np.array_equal(res.cpu().numpy(), ref_res.view(np.uint8).ravel())
