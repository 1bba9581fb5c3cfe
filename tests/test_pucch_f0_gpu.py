"""GPU: miphy_pucch_process_f0_batch, PUCCH format 0. The 23.5 reference cannot express such a PDU, so every check is against the numpy transmitter
(tests/pucch_f0_tx.py) and the float64 receiver (tests/pucch_f0_ref.py):
 - energy_out against the float64 E[k'] within 1e-5 of the PDU's sum of the twelve: float32 sums of 12 terms give about 2e-6, the margin is fivefold
   (worst measured on the MI355X over all the PDUs below: 2.24e-7);
 - payload and status equal to the receiver's; detection_metric, EPRE and RSRP within 1e-4 relative, SINR within 0.01 dB, time alignment exactly 0.
The PDUs are those of tests/pucch_f0_cases.py; tests/test_pucch_f0_tx.py checks on the CPU what the float64 receiver makes of them, and that no
decision of the deterministic sets (and at most 1 % of those of the noise set) is close enough to a tie or a threshold to flip in single precision.
Every call starts with sentinel bytes in payload, records (two more than there are jobs) and energies, and only owned bytes may change."""
import ctypes as C

import numpy as np
import pytest

import miphy
import pucch_f0_cases as G
import pucch_f0_ref as R
import pucch_f0_tx as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAY, EN = 0xEE, 7.5  # sentinels
RES = miphy.PucchResult.itemsize


def nbytes(p):
    return p["nharq"] + p["nsr"]


def prepare(items):
    """Jobs over one concatenation of the items' distinct grids, with sentinel bytes between the PDUs' payloads and energies."""
    jobs = np.zeros(len(items), miphy.PucchF0Job)
    grids, goff, total, po, eo, p_, e_ = [], {}, 0, [], [], 3, 5
    for i, d in enumerate(items):
        if id(d["grid"]) not in goff:
            goff[id(d["grid"])] = total
            grids.append(d["grid"].ravel())
            total += d["grid"].size
        po.append(p_), eo.append(e_)
        jobs[i] = X.job_of(d["pdu"], goff[id(d["grid"])], p_, e_)
        p_ += nbytes(d["pdu"]) + 3
        e_ += 12 + 3
    return dict(jobs=jobs, grid=torch.from_numpy(np.concatenate(grids)).cuda(), po=po, eo=eo, npay=p_ + 8, nen=e_ + 8)


def buffers(pre, njobs):
    return (torch.full((pre["npay"],), PAY, dtype=torch.uint8, device="cuda"), torch.full(((njobs + 2) * RES,), PAY, dtype=torch.uint8, device="cuda"),
            torch.full((pre["nen"],), EN, dtype=torch.float32, device="cuda"))


def run(ctx, pre, jobs=None, with_energy=True, on_device=False):
    """(payload, records, energies) of one call; every buffer starts as sentinels, two records more than jobs."""
    jobs = pre["jobs"] if jobs is None else jobs
    pay, res, en = buffers(pre, len(jobs))
    j = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs
    ctx.pucch_process_f0_batch(j, pre["grid"], pay, res, en if with_energy else None, jobs_on_device=on_device)
    torch.cuda.synchronize()
    return pay.cpu().numpy(), res.cpu().numpy().view(miphy.PucchResult), en.cpu().numpy()


def touched(pre, items, only=None):
    """Masks of the payload bytes and energy floats the items own (only: those items alone)."""
    tp, te = np.zeros(pre["npay"], bool), np.zeros(pre["nen"], bool)
    for i, d in enumerate(items):
        if only is not None and i not in only:
            continue
        tp[pre["po"][i]:pre["po"][i] + nbytes(d["pdu"])] = True
        te[pre["eo"][i]:pre["eo"][i] + 12] = True
    return tp, te


def assert_sentinels(pre, items, out, only=None):
    pay, res, en = out
    tp, te = touched(pre, items, only)
    assert (pay[~tp] == PAY).all(), "payload bytes outside the PDUs"
    assert (en[~te] == EN).all(), "energies outside the PDUs"
    n = len(items) if only is None else len(res) - 2
    assert (res[n:].view(np.uint8) == PAY).all(), "records of other PDUs"
    written = range(n) if only is None else sorted(only)
    assert all((res[i]["reserved"] == PAY).all() for i in written)


WORST = {"energy": 0.0}


def check_items(items, refs, pre, out, loose=()):
    """Everything one call wrote for `items` against the float64 receiver; loose: items whose decision may flip in single precision (payload, status
    and what depends on the choice are not compared)."""
    pay, res, en = out
    bad = []  # every mismatch of the call, so that one run shows them all

    def want(ok, *what):
        if not ok:
            bad.append(what)

    for i, (d, ref) in enumerate(zip(items, refs)):
        p, r = d["pdu"], res[i]
        tag = "PDU %d: %d ports, %d symbols, hop %d, start %d, ics %d, harq %d, sr %d, mask %03x, noise_var %g, sent %s" % (
            i, p["nports"], p["nsym"], p["hop"], p["start"], p["ics"], p["nharq"], p["nsr"], p["mask"], p["noise_var"], d["hyp"])
        E = en[pre["eo"][i]:pre["eo"][i] + 12].astype(np.float64)
        err = np.abs(E - ref["E"]).max() / ref["E"].sum()
        WORST["energy"] = max(WORST["energy"], err)
        want(err <= 1e-5, tag, "energies", err)
        a, b = 10 ** (float(r["epre_db"]) / 10), 10 ** (ref["epre_db"] / 10)
        want(abs(a - b) <= 1e-4 * b, tag, "epre", a, b)
        want(float(r["time_alignment_s"]) == 0.0, tag, "time alignment", float(r["time_alignment_s"]))
        if i in loose:
            continue
        got = pay[pre["po"][i]:pre["po"][i] + nbytes(p)]
        want(np.array_equal(got, ref["bits"]) and int(r["status"]) == ref["status"], tag, "payload, status, expected", list(got), int(r["status"]), list(ref["bits"]),
             ref["status"])
        want(abs(float(r["detection_metric"]) - ref["detection_metric"]) <= 1e-4 * ref["detection_metric"], tag, "detection metric",
             float(r["detection_metric"]), ref["detection_metric"])
        a, b = 10 ** (float(r["rsrp_db"]) / 10), 10 ** (ref["rsrp_db"] / 10)
        want(abs(a - b) <= 1e-4 * b, tag, "rsrp", a, b)
        want(abs(float(r["sinr_db"]) - ref["sinr_db"]) <= 0.01, tag, "sinr_db", float(r["sinr_db"]), ref["sinr_db"])
    assert not bad, "%d mismatches, the first: %s" % (len(bad), bad[:12])


def test_every_shape(ctx):
    """Ports 1..4; one and two symbols, hopping on and off; every (HARQ-ACK, SR) and every hypothesis sent, nothing sent included; all twelve initial
    shifts; start symbols 13 and 12 among them; numerologies 0 and 1; slots 0 to 19 (tests/test_pucch_f0_tx.py asserts the coverage)."""
    items, refs = G.shapes_set(), G.reference("shapes")
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, refs, pre, out)
    assert_sentinels(pre, items, out)
    sent = [i for i, d in enumerate(items) if d["hyp"] is not None]
    assert all(out[1][i]["status"] == R.VALID for i in sent)
    print("worst energy error so far, relative to the sum of the twelve: %.3g" % WORST["energy"])
    # without energy_out: the same payloads and records
    out2 = run(ctx, pre, with_energy=False)
    assert np.array_equal(out[0], out2[0]) and np.array_equal(out[1].view(np.uint8), out2[1].view(np.uint8)) and (out2[2] == EN).all()


@pytest.mark.parametrize("kind", ["three", "six", "power"])
def test_ues_multiplexed_on_one_prb_each_decode_their_own_bits(ctx, kind):
    items, refs = G.multiplexed(kind), G.reference(kind)
    assert len({id(d["grid"]) for d in items}) == 1 and len({(d["pdu"]["prb"], d["pdu"]["start"]) for d in items}) == 1
    free = bin(R.free_mask(items[0]["pdu"])).count("1")
    assert (len(items), free) == {"three": (3, 6), "six": (6, 0), "power": (2, 8)}[kind]
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, refs, pre, out)
    assert_sentinels(pre, items, out)
    for i, d in enumerate(items):
        p = d["pdu"]
        assert out[1][i]["status"] == R.VALID and list(out[0][pre["po"][i]:pre["po"][i] + 1]) == X.hypothesis_bits(p["nharq"], p["nsr"], d["hyp"]), (kind, i)
    if kind == "six":  # full occupancy without a noise variance is refused, and nothing is written
        jobs = pre["jobs"].copy()
        jobs["noise_var"][3] = 0
        pay, res, en = buffers(pre, len(jobs))
        with pytest.raises(Exception, match="job 3: no free cyclic shift to estimate the noise from"):
            ctx.pucch_process_f0_batch(jobs, pre["grid"], pay, res, en)
        torch.cuda.synchronize()
        assert bool((pay == PAY).all()) and bool((res == PAY).all()) and bool((en == EN).all())
    if kind == "power":
        assert float(out[1][0]["rsrp_db"]) - float(out[1][1]["rsrp_db"]) > 5


def test_noise_only_verdicts_equal_the_receivers(ctx):
    """4096 PDUs of noise alone in one call. The verdicts and payloads equal the float64 receiver's except where tests/test_pucch_f0_tx.py found the
    decision near a tie or a threshold: at most 1 % of the PDUs."""
    items, refs = G.noise_set(), G.reference("noise")
    loose = {i for i, r in enumerate(refs) if R.near(r)}
    assert len(items) == 4096 and len(loose) <= len(items) // 100
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, refs, pre, out, loose)
    assert_sentinels(pre, items, out)
    nvalid = int((out[1][:len(items)]["status"] == R.VALID).sum())
    print("VALID verdicts on noise alone: %d of %d on the device, %d by the float64 receiver" % (nvalid, len(items), sum(r["status"] == R.VALID for r in refs)))
    assert nvalid <= 64 + len(loose)
    print("worst energy error so far, relative to the sum of the twelve: %.3g" % WORST["energy"])


def with_thresholds(jobs):
    jobs = jobs.copy()
    jobs["threshold"] = [miphy.pucch_f0_info(j)["threshold"] for j in jobs]
    return jobs


def test_device_resident_jobs_give_the_bytes_of_host_jobs(ctx):
    items = G.mixed_items()
    pre = prepare(items)
    host = run(ctx, pre)
    check_items(items, G.reference("mixed"), pre, host)
    jobs = with_thresholds(pre["jobs"])
    dev = run(ctx, pre, jobs=jobs, on_device=True)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()
    # a device job that breaks a rule, and one without a threshold, are skipped with nothing written; their neighbours are processed
    broken = jobs.copy()
    broken["nof_ports"][2] = 5
    broken["threshold"][5] = 0
    out = run(ctx, pre, jobs=broken, on_device=True)
    keep = set(range(len(items))) - {2, 5}
    assert_sentinels(pre, items, out, only=keep)
    assert (out[1][[2, 5]].view(np.uint8) == PAY).all()
    for i in keep:
        assert out[1][i].tobytes() == host[1][i].tobytes(), i
        assert out[0][pre["po"][i]:pre["po"][i] + nbytes(items[i]["pdu"])].tobytes() == host[0][pre["po"][i]:pre["po"][i] + nbytes(items[i]["pdu"])].tobytes(), i
        assert out[2][pre["eo"][i]:pre["eo"][i] + 12].tobytes() == host[2][pre["eo"][i]:pre["eo"][i] + 12].tobytes(), i


def test_device_jobs_captured_in_a_graph(ctx):
    """The call only enqueues: with device-resident jobs it is captured and replayed, with the bytes of the direct call."""
    items = G.mixed_items()
    pre = prepare(items)
    want = run(ctx, pre)
    jobs_d = torch.from_numpy(with_thresholds(pre["jobs"]).view(np.uint8).copy()).cuda()
    pay, res, en = buffers(pre, len(items))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.pucch_process_f0_batch(jobs_d, pre["grid"], pay, res, en, jobs_on_device=True, stream=s)  # warm-up (Gold tables)
    torch.cuda.synchronize()
    pay.fill_(PAY), res.fill_(PAY), en.fill_(EN)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.pucch_process_f0_batch(jobs_d, pre["grid"], pay, res, en, jobs_on_device=True, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert pay.cpu().numpy().tobytes() == want[0].tobytes() and res.cpu().numpy().tobytes() == want[1].tobytes() and en.cpu().numpy().tobytes() == want[2].tobytes()


def test_mixed_batch_on_one_grid_equals_the_single_runs(ctx):
    items = G.mixed_items()
    assert len({id(d["grid"]) for d in items}) == 1
    occupied = np.zeros((14, G.GRID_NPRB), int)
    for d in items:  # the allocations do not overlap
        for l, prb in enumerate(X.hop_prbs(d["pdu"])):
            occupied[d["pdu"]["start"] + l, prb] += 1
    assert occupied.max() == 1
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, G.reference("mixed"), pre, out)
    assert_sentinels(pre, items, out)
    for i, d in enumerate(items):
        one = run(ctx, pre, jobs=pre["jobs"][i:i + 1])
        assert one[1][0].tobytes() == out[1][i].tobytes(), i
        for k, off, n in ((0, pre["po"][i], nbytes(d["pdu"])), (2, pre["eo"][i], 12)):
            assert one[k][off:off + n].tobytes() == out[k][off:off + n].tobytes(), (i, k)
        tp, te = touched(pre, items, only={i})
        assert (one[0][~tp] == PAY).all() and (one[2][~te] == EN).all() and (one[1][1:].view(np.uint8) == PAY).all(), i


def _set(field, value, job):
    def f(jobs):
        jobs[job][field] = value
    return f


# (case, argument replaced by NULL, change to the jobs of G.mixed_items(), text of the rule); the code is MIPHY_EINVAL
REJECTIONS = [("null context", 0, None, "null argument"), ("null jobs", 1, None, "null argument"), ("null grid", 4, None, "null argument"),
              ("null payload", 5, None, "null argument"), ("null results", 6, None, "null argument"), ("format 1", None, _set("format", 1, 3), "job 3: the format is not 0"),
              ("three symbols", None, _set("nof_symbols", 3, 2), "job 2: invalid symbol range"),
              ("hopping with one symbol", None, _set("intra_slot_hopping", 1, 0), "job 0: intra_slot_hopping"),
              ("five ports", None, _set("nof_ports", 5, 7), "job 7: invalid number of receive ports"),
              ("shift 12", None, _set("initial_cyclic_shift", 12, 1), "job 1: initial_cyclic_shift"), ("no UCI bits", None, _set("nof_sr", 0, 2), "job 2: no UCI bits"),
              ("empty free set", None, _set("used_shifts_mask", 0xfff, 6), "job 6: no free cyclic shift"),
              ("negative threshold", None, _set("threshold", -1.0, 5), "job 5: threshold and noise_var")]


@pytest.mark.parametrize("case,null,change,rule", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_a_rejected_batch_writes_nothing(ctx, case, null, change, rule):
    items = G.mixed_items()
    pre = prepare(items)
    jobs = pre["jobs"].copy()
    if change:
        change(jobs)
    pay, res, en = buffers(pre, len(jobs))

    def call(j, n, null=None):
        args = [ctx.h, C.c_void_p(j.ctypes.data), 0, n, C.c_void_p(pre["grid"].data_ptr()), C.c_void_p(pay.data_ptr()), C.c_void_p(res.data_ptr()),
                C.c_void_p(en.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        if null is not None:
            args[null] = None
        return miphy.lib().miphy_pucch_process_f0_batch(*args)

    assert call(jobs, jobs.size, null) == -1
    assert rule in miphy.lib().miphy_last_error().decode(), miphy.lib().miphy_last_error().decode()
    assert call(pre["jobs"], 0) == 0  # n == 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((pay == PAY).all()) and bool((res == PAY).all()) and bool((en == EN).all())
    if case == "format 1":  # and the same buffers are taken with the jobs as they were
        assert call(pre["jobs"], jobs.size) == 0
        torch.cuda.synchronize()
        assert bool((res.cpu()[:jobs.size * RES:RES] != PAY).all()) and bool((res[jobs.size * RES:] == PAY).all())


def test_the_old_entry_points_give_the_same_bytes_as_before(ctx):
    """miphy_pucch_process_batch on the short fixture and miphy_pucch_process_f34_batch on six PDUs of its noisy set: the same bytes before and after
    calls of the new entry point on the same context."""
    import pucch_f34_cases as G34
    import pucch_tx as T
    from test_pucch_f34_gpu import prepare as prepare34
    from test_pucch_f34_gpu import run as run34
    from test_pucch_proc_gpu import check_case, device_grids, make_jobs
    from test_pucch_proc_gpu import run as run_old
    from test_pucch_tx import FX
    fx = dict(np.load(FX))
    fx["grids"] = T.fixture_grids(fx)
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    jobs = make_jobs(fx, range(n), offs)
    pre34 = prepare34(G34.noisy_set()[:6])
    before, before34 = run_old(ctx, jobs, grid_d), run34(ctx, pre34, 2)
    items = G.mixed_items()
    pre = prepare(items)
    run(ctx, pre)
    run(ctx, pre, jobs=with_thresholds(pre["jobs"]), on_device=True)
    after, after34 = run_old(ctx, jobs, grid_d), run34(ctx, pre34, 2)
    for a, b in list(zip(before, after)) + list(zip(before34, after34)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    bad = [m for m in (check_case(fx, i, after[0][11 * i:11 * i + 11], after[1][i]) for i in range(n)) if m]
    assert not bad, bad[:5]
