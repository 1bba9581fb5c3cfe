"""GPU: miphy_pucch_process_f34_batch, PUCCH formats 3 and 4. The 23.5 reference refuses both formats, so every check is against the numpy
transmitter (tests/pucch_f34_tx.py), the float64 receiver (tests/pucch_f34_ref.py) or a composition of blocks that are pinned already:
 - est_out against the float64 estimate within 1e-6 at unit scale (of the PDU's largest estimate when that exceeds 1), the bound
   tests/test_chest_tp_gpu.py has for the low-PAPR pilots these estimates are products of (worst case measured on the MI355X over all the
   PDUs below: 3.6e-7); the noise variance within 1e-4 relative, the tolerance of the EPRE it is derived from;
 - the CSI within the tolerances of tests/test_pucch_proc_gpu.py (EPRE, RSRP 1e-4 relative; SINR 0.01 dB or both >= 60 dB; time alignment 1.01 taps);
 - the soft bits byte for byte against host extraction, miphy_channel_equalize_batch, miphy_transform_deprecode_batch, the float32
   despreading in the stated order, the oracle's soft demapper and Gold sequence, fed the kernel's own est_out (the method of
   tests/test_pusch_demod_tp_gpu.py);
 - payload and status against the short-block restatement or the polar restatements at the call's list size on those soft bits (the method of
   tests/test_pucch_long_gpu.py).
The PDUs are those of tests/pucch_f34_cases.py; tests/test_pucch_f34_tx.py checks on the CPU what the float64 receiver makes of them."""
import ctypes as C

import numpy as np
import pytest

import miphy
import oracle_lib as O
import pucch_f34_cases as G
import pucch_f34_ref as R
import pucch_f34_tx as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAY, LLR, EST = 0xEE, 99, 7.5  # sentinels
RES = miphy.PucchResult.itemsize


def est_floats(p):
    return 2 * p["nports"] * (2 if p["hop"] else 1) * 12 * p["nprb"] + p["nports"]


def prepare(items):
    """Jobs over one concatenation of the items' grids (an item without a grid of its own shares the one in front of it), with sentinel bytes
    between the PDUs' payloads, soft bits and estimates."""
    jobs = np.zeros(len(items), miphy.PucchF34Job)
    grids, goff, po, lo, eo, p_, l_, e_, last = [], 0, [], [], [], 3, 1, 5, None
    for i, d in enumerate(items):
        if d["grid"] is not last:
            last = d["grid"]
            grids.append(last.ravel())
            goff += last.size
        po.append(p_), lo.append(l_), eo.append(e_)
        jobs[i] = X.job_of(d["pdu"], d["K"], goff - last.size, p_, l_, e_)
        p_ += d["K"] + 5
        l_ += X.nof_soft_bits(d["pdu"]) + 7
        e_ += est_floats(d["pdu"]) + 3
    return dict(jobs=jobs, grid=torch.from_numpy(np.concatenate(grids)).cuda(), po=po, lo=lo, eo=eo, npay=p_ + 8, nllr=l_ + 8, nest=e_ + 8)


def run(ctx, pre, L, jobs=None, with_llr=True, with_est=True):
    """(payload, records, soft bits, estimates) of one call; every buffer starts as sentinels, two records more than jobs."""
    jobs = pre["jobs"] if jobs is None else jobs
    pay = torch.full((pre["npay"],), PAY, dtype=torch.uint8, device="cuda")
    res = torch.full(((len(jobs) + 2) * RES,), PAY, dtype=torch.uint8, device="cuda")
    llr = torch.full((pre["nllr"],), LLR, dtype=torch.int8, device="cuda")
    est = torch.full((pre["nest"],), EST, dtype=torch.float32, device="cuda")
    ctx.pucch_process_f34_batch(jobs, L, pre["grid"], pay, res, llr if with_llr else None, est if with_est else None)
    torch.cuda.synchronize()
    return pay.cpu().numpy(), res.cpu().numpy().view(miphy.PucchResult), llr.cpu().numpy(), est.cpu().numpy()


def touched(pre, items, only=None):
    """Masks of the payload bytes, soft bits and estimate floats the items own (only: that item alone)."""
    tp, tl, te = np.zeros(pre["npay"], bool), np.zeros(pre["nllr"], bool), np.zeros(pre["nest"], bool)
    for i, d in enumerate(items):
        if only is not None and i != only:
            continue
        tp[pre["po"][i]:pre["po"][i] + d["K"]] = True
        tl[pre["lo"][i]:pre["lo"][i] + X.nof_soft_bits(d["pdu"])] = True
        te[pre["eo"][i]:pre["eo"][i] + est_floats(d["pdu"])] = True
    return tp, tl, te


def assert_sentinels(pre, items, out):
    pay, res, llr, est = out
    tp, tl, te = touched(pre, items)
    assert (pay[~tp] == PAY).all(), "payload bytes outside the PDUs"
    assert (llr[~tl] == LLR).all(), "soft bits outside the PDUs"
    assert (est[~te] == EST).all(), "estimates outside the PDUs"
    assert (res[len(items):].view(np.uint8) == PAY).all(), "records of other PDUs"
    assert (res[:len(items)]["reserved"] == PAY).all()


def device_estimate(p, est):
    """(h [port][hop][M] complex64, noise variance [port] float32) of a PDU's est_out range."""
    nh, M, n = 2 if p["hop"] else 1, 12 * p["nprb"], p["nports"]
    return est[:2 * n * nh * M].view(np.complex64).reshape(n, nh, M), est[2 * n * nh * M:2 * n * nh * M + n]


def composition(ctx, items, ests):
    """The soft bits of every item from its device estimate through the pinned blocks, each as one batched call."""
    ej, tj = np.zeros(len(items), miphy.EqualizerJob), np.zeros(len(items), miphy.TransformDeprecodeJob)
    ys, hs, yoff, zoff, voff = [], [], 0, 0, 0
    for i, (d, e) in enumerate(zip(items, ests)):
        p = d["pdu"]
        h, nvar = device_estimate(p, e)
        M = 12 * p["nprb"]
        _, data = X.layout(p["nsym"], p["hop"], p["add"])
        prb = X.hop_prbs(p)
        order = [(o, int(o in data[1])) for o in range(p["nsym"]) if o in data[0] + data[1]]
        y = np.stack([np.concatenate([d["grid"][port, p["start"] + o, 12 * prb[hop]:12 * prb[hop] + M] for o, hop in order]) for port in range(p["nports"])])
        hh = np.stack([np.concatenate([h[port, hop] for o, hop in order]) for port in range(p["nports"])])
        ej[i] = (y.shape[1], p["nports"], 1, [0, 0], nvar[0], 1.0, yoff, yoff, zoff, zoff)
        tj[i] = (M, len(order), zoff, zoff, zoff, voff)
        ys.append(y.reshape(-1)), hs.append(hh.reshape(-1))
        yoff += y.size
        zoff += y.shape[1]
        voff += len(order)
    z, zv = torch.zeros(zoff, dtype=torch.complex64, device="cuda"), torch.zeros(zoff, dtype=torch.float32, device="cuda")
    ctx.channel_equalize_batch(ej, torch.from_numpy(np.concatenate(ys)).cuda(), torch.from_numpy(np.concatenate(hs)).cuda(), z, zv)
    yd, vd = torch.zeros(zoff, dtype=torch.complex64, device="cuda"), torch.zeros(voff, dtype=torch.float32, device="cuda")
    ctx.transform_deprecode_batch(tj, z, zv, yd, vd)
    torch.cuda.synchronize()
    yh, vh = yd.cpu().numpy(), vd.cpu().numpy()
    out = []
    for i, d in enumerate(items):
        p = d["pdu"]
        M, nd = int(tj[i]["M"]), int(tj[i]["nof_symbols"])
        z0, v0 = int(tj[i]["out_symbols_offset"]), int(tj[i]["out_noise_var_offset"])
        sym, var = yh[z0:z0 + nd * M].reshape(nd, M), vh[v0:v0 + nd]
        if p["fmt"] == 4:  # float32 throughout: the products by +-1 and +-j and the division by 2 or 4 are exact
            sym = np.stack([R.despread(s, p) for s in sym])
            var = var / np.float32(p["occ_len"])
            assert sym.dtype == np.complex64 and var.dtype == np.float32
        mod = 1 if p["pi2"] else 2
        raw = O.o_demodulate_soft(mod, sym.reshape(-1), np.repeat(var, sym.shape[1])).astype(np.int16)
        sign = 1 - 2 * O.o_gold((p["rnti"] << 15) + p["nid_scr"], 0, raw.size).astype(np.int16)
        out.append((raw * sign).astype(np.int8))
    return out


WORST = {"est": 0.0}


def check_items(ctx, items, pre, out, L, decoded=True):
    """Everything one call wrote for `items` against the references. decoded: the PDUs were sent at 20 dB or better, so they come out with their own
    bits and VALID (the float64 receiver does the same, tests/test_pucch_f34_tx.py)."""
    pay, res, llr, est = out
    ests = [est[pre["eo"][i]:pre["eo"][i] + est_floats(d["pdu"])] for i, d in enumerate(items)]
    want_llr = composition(ctx, items, ests)
    bad = []  # every mismatch of the call, so that one run shows them all

    def want(ok, *what):
        if not ok:
            bad.append(what)

    for i, d in enumerate(items):
        p, K, E = d["pdu"], d["K"], X.nof_soft_bits(d["pdu"])
        tag = "PDU %d: format %d, %d PRB, %d symbols, hop %d, add %d, pi2 %d, occ %d/%d, %d ports, K %d, L %d" % (
            i, p["fmt"], p["nprb"], p["nsym"], p["hop"], p["add"], p["pi2"], p["occ_idx"], p["occ_len"], p["nports"], K, L)
        h_ref, nvar_ref, csi = R.estimate(p, d["grid"])
        h, nvar = device_estimate(p, ests[i])
        err = np.abs(h.astype(np.complex128) - h_ref).max() / max(1.0, np.abs(h_ref).max())
        WORST["est"] = max(WORST["est"], err)
        want(err <= 1e-6, tag, "estimate", err)
        want(np.all(np.abs(nvar - nvar_ref) <= 1e-4 * nvar_ref), tag, "noise variance", nvar, nvar_ref)
        r = res[i]
        for k in ("epre_db", "rsrp_db"):
            a, b = 10 ** (float(r[k]) / 10), 10 ** (csi[k] / 10)
            want(abs(a - b) <= 1e-4 * abs(b), tag, k, a, b)
        sa, sb = float(r["sinr_db"]), csi["sinr_db"]
        want(abs(sa - sb) <= 0.01 or (sa >= 60 and sb >= 60), tag, "sinr_db", sa, sb)
        tap = 1.0 / (4096 * (15 << p["numerology"]) * 1000.0)
        want(abs(float(r["time_alignment_s"]) - csi["time_alignment_s"]) <= 1.01 * tap, tag, "time alignment in taps", float(r["time_alignment_s"]) / tap,
             csi["time_alignment_s"] / tap)
        want(r["detection_metric"] == 0, tag, "detection metric")
        soft = llr[pre["lo"][i]:pre["lo"][i] + E]
        want(np.array_equal(soft, want_llr[i]), tag, "soft bits that differ from the composition", int((soft != want_llr[i]).sum()), E)
        bits, status = R.decode(p, K, soft, L)
        got = pay[pre["po"][i]:pre["po"][i] + K]
        want(np.array_equal(got, bits) and int(r["status"]) == status, tag, "payload bits that differ, status, expected", int((got != bits).sum()), int(r["status"]), status)
        if decoded:
            want(np.array_equal(got, d["bits"]), tag, "not the bits that were sent")
            want(status == 1 or (K <= 11 and E < 32), tag, "not VALID")  # (a short-block codeword cut below its 32 bits may stay under the detector's threshold)
    assert not bad, "%d mismatches, the first: %s" % (len(bad), bad[:12])


@pytest.mark.parametrize("nports", G.PORTS)
def test_format3_every_size_and_length(ctx, nports):
    items = G.f3_set(nports)
    assert {d["pdu"]["nprb"] for d in items} == set(G.F3_PRBS) and {(d["pdu"]["nsym"], d["pdu"]["hop"], d["pdu"]["add"]) for d in items} == set(G.F3_LENGTHS)
    assert {d["pdu"]["pi2"] for d in items} == {0, 1} and {d["K"] for d in items} >= set(G.KS) | {400}
    pre = prepare(items)
    out = run(ctx, pre, 1)
    check_items(ctx, items, pre, out, 1)
    assert_sentinels(pre, items, out)
    print("worst estimate error so far, at unit scale: %.3g" % WORST["est"])


def test_format3_over_the_port_counts_every_shape_meets_every_payload_size():
    seen = {}
    for nports in G.PORTS:
        for d in G.f3_set(nports)[:-1]:
            p = d["pdu"]
            seen.setdefault((p["nprb"], p["nsym"], p["hop"], p["add"]), set()).add((p["pi2"], d["K"]))
    assert len(seen) == len(G.F3_PRBS) * len(G.F3_LENGTHS)
    for shape, v in seen.items():
        assert {m for m, _ in v} == {0, 1}, shape
        fits = {K for K in G.KS if G.feasible(X.pdu(3, shape[1], shape[0], shape[2], shape[3], 0), K)}  # with QPSK, the larger E
        assert {K for _, K in v} >= {K for K in fits if G.feasible(X.pdu(3, shape[1], shape[0], shape[2], shape[3], 1), K)}, (shape, v)


def test_format4_every_sequence(ctx):
    items = G.f4_set()
    assert {(d["pdu"]["occ_len"], d["pdu"]["occ_idx"], d["pdu"]["pi2"], d["pdu"]["nsym"]) for d in items} == \
        {(n, i, m, s) for n in (2, 4) for i in range(n) for m in (0, 1) for s in (4, 14)}
    pre = prepare(items)
    out = run(ctx, pre, 2)
    check_items(ctx, items, pre, out, 2)
    assert_sentinels(pre, items, out)


@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_noisy_payloads_equal_the_restatements_at_every_list_size(ctx, L):
    items = G.noisy_set()
    pre = prepare(items)
    out = run(ctx, pre, L)
    check_items(ctx, items, pre, out, L, decoded=False)
    seen = {}
    for d, r in zip(items, out[1]):
        seen.setdefault(G.klass(d["K"]), set()).add(int(r["status"]))
    assert seen == {"short": {1, 2}, "crc6": {1, 2}, "crc11": {1, 2}}, seen
    # without llr_out the soft bits of the polar-coded PDUs pass through the context's workspace: the same payloads and records
    out2 = run(ctx, pre, L, with_llr=False, with_est=False)
    assert np.array_equal(out[0], out2[0]) and np.array_equal(out[1].view(np.uint8), out2[1].view(np.uint8))
    assert (out2[2] == LLR).all() and (out2[3] == EST).all()


@pytest.mark.parametrize("nsf", [2, 4])
def test_all_sequences_of_one_prb_in_one_batch(ctx, nsf):
    pdus, bits, grid = G.multiplexed(nsf)
    items = [dict(pdu=p, K=len(b), bits=b, grid=grid) for p, b in zip(pdus, bits)]
    pre = prepare(items)
    pay, res, llr, est = run(ctx, pre, 1)
    for i, d in enumerate(items):
        assert res[i]["status"] == 1 and np.array_equal(pay[pre["po"][i]:pre["po"][i] + d["K"]], d["bits"]), (nsf, i)
    assert len({b.tobytes() for b in bits}) == nsf


def test_mixed_batch_on_one_grid_equals_the_single_runs(ctx):
    items = G.mixed_items()
    occupied = np.zeros((14, G.GRID_NPRB), int)
    for d in items:  # the allocations do not overlap
        p = d["pdu"]
        split = p["nsym"] // 2 if p["hop"] else p["nsym"]
        for o in range(p["nsym"]):
            prb = X.hop_prbs(p)[int(o >= split)]
            occupied[p["start"] + o, prb:prb + p["nprb"]] += 1
    assert occupied.max() == 1
    pre = prepare(items)
    L = 4
    out = run(ctx, pre, L)
    check_items(ctx, items, pre, out, L)
    assert_sentinels(pre, items, out)
    for i, d in enumerate(items):
        one = run(ctx, pre, L, jobs=pre["jobs"][i:i + 1])
        assert one[1][0].tobytes() == out[1][i].tobytes(), i
        for k, off, n in ((0, pre["po"][i], d["K"]), (2, pre["lo"][i], X.nof_soft_bits(d["pdu"])), (3, pre["eo"][i], est_floats(d["pdu"]))):
            assert one[k][off:off + n].tobytes() == out[k][off:off + n].tobytes(), (i, k)
        tp, tl, te = touched(pre, items, only=i)
        assert (one[0][~tp] == PAY).all() and (one[2][~tl] == LLR).all() and (one[3][~te] == EST).all() and (one[1][1:].view(np.uint8) == PAY).all(), i


def _set(field, value, job=1):
    def f(jobs):
        jobs[job][field] = value
    return f


# (case, list size, argument replaced by NULL, change to the jobs, code, text of the rule)
REJECTIONS = [("list size 3", 3, None, None, -1, "list size"), ("list size 0", 0, None, None, -1, "list size"), ("null context", 1, 0, None, -1, "null argument"),
              ("null jobs", 1, 1, None, -1, "null argument"), ("null grid", 1, 4, None, -1, "null argument"), ("null payload", 1, 5, None, -1, "null argument"),
              ("null results", 1, 6, None, -1, "null argument"), ("2 PRBs", 1, None, _set("nof_prb", 2, 0), -4, "length-24"),
              ("7 PRBs", 2, None, _set("nof_prb", 7, 0), -1, "job 0: format 3 on 7 PRBs"), ("occ index", 4, None, _set("occ_index", 2), -1, "job 1: occ_index 2"),
              ("CSI part 2", 8, None, _set("nof_csi_part2", 1, 2), -1, "job 2: CSI part 2"), ("five ports", 1, None, _set("nof_ports", 5, 3), -1, "job 3: invalid number"),
              ("too many bits", 1, None, _set("nof_csi_part1", 1800, 0), -1, "12 to 1706 bits"), ("format 2", 1, None, _set("format", 2, 3), -1, "job 3: format 2")]


@pytest.mark.parametrize("case,L,null,change,code,rule", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_a_rejected_batch_writes_nothing(ctx, case, L, null, change, code, rule):
    items = G.mixed_items()[:4]  # format 3, format 4, format 3, format 3
    pre = prepare(items)
    jobs = pre["jobs"].copy()
    if change:
        change(jobs)
    pay = torch.full((pre["npay"],), PAY, dtype=torch.uint8, device="cuda")
    res = torch.full((6 * RES,), PAY, dtype=torch.uint8, device="cuda")
    llr = torch.full((pre["nllr"],), LLR, dtype=torch.int8, device="cuda")
    est = torch.full((pre["nest"],), EST, dtype=torch.float32, device="cuda")

    def call(j, n, L, null=None):
        args = [ctx.h, C.c_void_p(j.ctypes.data), n, L, C.c_void_p(pre["grid"].data_ptr()), C.c_void_p(pay.data_ptr()), C.c_void_p(res.data_ptr()),
                C.c_void_p(llr.data_ptr()), C.c_void_p(est.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        if null is not None:
            args[null] = None
        return miphy.lib().miphy_pucch_process_f34_batch(*args)

    assert call(jobs, jobs.size, L, null) == code
    assert rule in miphy.lib().miphy_last_error().decode(), miphy.lib().miphy_last_error().decode()
    assert call(pre["jobs"], 0, 1) == 0  # n == 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((pay == PAY).all()) and bool((res == PAY).all()) and bool((llr == LLR).all()) and bool((est == EST).all())
    if case == "format 2":  # and the same buffers are taken with the jobs as they were
        assert call(pre["jobs"], 4, 1) == 0
        torch.cuda.synchronize()
        assert bool((res.cpu()[:4 * RES:RES] != PAY).all()) and bool((res[4 * RES:] == PAY).all())


def test_the_old_entry_points_give_the_same_bytes_as_before(ctx):
    """miphy_pucch_process_batch on the short fixture: against the fixture's recorded results (tests/test_pucch_proc_gpu.py), and the same bytes before
    and after calls of the new entry point on the same context."""
    import pucch_tx as T
    from test_pucch_proc_gpu import check_case, device_grids, make_jobs
    from test_pucch_proc_gpu import run as run_old
    from test_pucch_tx import FX
    fx = dict(np.load(FX))
    fx["grids"] = T.fixture_grids(fx)
    grid_d, offs = device_grids(fx)
    n = len(fx["cfg"])
    jobs = make_jobs(fx, range(n), offs)
    before = run_old(ctx, jobs, grid_d)
    items = G.noisy_set()[:6]
    run(ctx, prepare(items), 8)
    after = run_old(ctx, jobs, grid_d)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    bad = [m for m in (check_case(fx, i, after[0][11 * i:11 * i + 11], after[1][i]) for i in range(n)) if m]
    assert not bad, bad[:5]
