"""GPU: miphy_prach_detect_batch / miphy_prach_generate_batch (csrc/prach.hip) against tests/golden/prach_detector.npz, recorded from
the reference's own PRACH detector and generator, and against the float64 restatement of tests/prach_ref.py. The symbols are rebuilt
by prach_ref (their hashes are checked on the CPU by test_prach_ref.py), which also states the tolerances and checks that the
reference's recorded values lie within them of the restatement.

Per requested preamble: the device's peak bin must hold a float64 power within 2 TOL_P of the maximum, and be the reference's bin where
no other bin comes that close; delay_n, its sign, delay_n_maximum, N_CS are exact; peak power, metric and RSSI lie within TOL_P, TOL_M
and 1e-5 of the reference's; `detected` equals the reference's wherever its metric is farther than TOL_M from the threshold (at most
0.5 % of the pairs are not), and always agrees with the device's own metric and delay."""
import numpy as np
import pytest

import miphy
import prach_ref as P
from test_prach_ref import BAND_CAP, FX, TOL_M, TOL_P, TOL_RSSI, in_band

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0xEE
REC = miphy.PrachPreambleResult.itemsize


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return miphy.Context(0)


@pytest.fixture(scope="module")
def fx():
    d = dict(np.load(FX))
    d["symbols"] = P.fixture_symbols(d)
    return d


def make_jobs(fx, idx, sym_off, pre_off, idft=1536):
    """PrachJob records of the fixture cases idx; sym_off[n] / pre_off[n]: cf_t / record offsets of the n-th job."""
    jobs = np.zeros(len(idx), miphy.PrachJob)
    for n, i in enumerate(idx):
        c = fx["cfg"][i]
        j = jobs[n]
        j["format"], j["ra_scs"], j["root_sequence_index"], j["zero_correlation_zone"] = c[P.C_FMT], c[P.C_SCS], c[P.C_ROOT], c[P.C_ZCZ]
        j["start_preamble_index"], j["nof_preamble_indices"], j["idft_size"] = c[P.C_START], c[P.C_NOF], idft
        j["symbol_offset"], j["preamble_offset"] = sym_off[n], pre_off[n]
    return jobs


def packed(fx, idx):
    """Symbols and record ranges of the cases idx laid out back to back: device symbols, symbol offsets, record offsets, record count."""
    flat = [fx["symbols"][i] for i in idx]
    sym_off = np.cumsum([0] + [len(f) for f in flat])[:-1]
    pre_off = np.cumsum([0] + [int(fx["cfg"][i, P.C_NOF]) for i in idx])
    return torch.from_numpy(np.concatenate(flat)).cuda(), sym_off, pre_off[:-1], int(pre_off[-1])


def run(ctx, jobs, sym_d, nrec, on_device=False, stream=None):
    n = len(jobs)
    res = torch.full((max(n, 1) * miphy.PrachResult.itemsize,), SENT, dtype=torch.uint8, device="cuda")
    pre = torch.full((max(nrec, 1) * REC,), SENT, dtype=torch.uint8, device="cuda")
    j = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs
    ctx.prach_detect_batch(j, sym_d, res, pre, stream=stream)
    torch.cuda.synchronize()
    return res.cpu().numpy().view(miphy.PrachResult)[:n], pre.cpu().numpy().view(miphy.PrachPreambleResult)[:nrec]


def check_case(fx, i, r, recs, idft=1536, stats=None):
    """Mismatches of case i (result record r, its preamble records recs). At 1536 the values are compared with the reference's, at any
    other size (which the recorder did not run) with the restatement."""
    c = fx["cfg"][i]
    d = P.derive(c[P.C_FMT], c[P.C_SCS], c[P.C_ZCZ], idft)
    err = []
    sym = fx["symbols"][i]
    rssi64 = P.rssi(sym)
    rssi_ref = float(fx["rssi"][i]) if idft == 1536 else rssi64
    if (r["delay_n_maximum"], r["n_cs"], r["n_cs_limited"]) != (d["delay_n_maximum"], d["n_cs"], d["n_cs_limited"]):
        err.append("derived %s" % r)
    if abs(float(r["rssi"]) - rssi_ref) > TOL_RSSI * rssi_ref:
        err.append("rssi %g vs %g" % (r["rssi"], rssi_ref))
    nof = int(c[P.C_NOF])
    assert len(recs) == nof
    if nof == 0:
        return err
    if not rssi64 > 0:
        if recs.view(np.uint8).any():
            err.append("all-zero symbol: records not zero")
        return err
    pw = P.correlation_power(sym, c, P.header_tables(), idft)
    peak = pw.max(axis=1)
    rows = np.arange(nof)
    idx = recs["peak_index"].astype(np.int64)
    if (idx >= idft).any():
        return err + ["peak index out of range"]
    if not (pw[rows, idx] >= (1 - 2 * TOL_P) * peak).all():
        err.append("peak bin not a maximum: %s" % np.nonzero(pw[rows, idx] < (1 - 2 * TOL_P) * peak)[0][:5])
    if idft == 1536:
        lo, hi = fx["peak_offset"][i], fx["peak_offset"][i + 1]
        ref_idx, ref_pow, ref_met = fx["peak_index"][lo:hi], fx["peak_power"][lo:hi].astype(np.float64), fx["peak_metric"][lo:hi].astype(np.float64)
        det = set(fx["det_index"][fx["det_offset"][i]:fx["det_offset"][i + 1]])
        ref_det = np.array([c[P.C_START] + k in det for k in range(nof)])
        single = (pw >= (1 - 2 * TOL_P) * peak[:, None]).sum(axis=1) == 1
        if not (idx == ref_idx)[single].all():
            err.append("peak bin differs from the reference's: %s" % np.nonzero((idx != ref_idx) & single)[0][:5])
    else:
        ref_pow, ref_met = peak, peak / (rssi64 * d["L"] ** 3)
        ref_det = ~(ref_met < float(P.THRESHOLD)) & (np.abs(P.delay_of(pw.argmax(axis=1), idft)) < d["delay_n_maximum"])
    if not (recs["delay_n"] == P.delay_of(idx, idft)).all():
        err.append("delay_n")
    dp = np.abs(recs["peak_power"].astype(np.float64) - ref_pow) / ref_pow
    dm = np.abs(recs["metric"].astype(np.float64) - ref_met) / ref_met
    if dp.max() > TOL_P:
        err.append("peak power off by %.2e" % dp.max())
    if dm.max() > TOL_M:
        err.append("metric off by %.2e" % dm.max())
    own = ~(recs["metric"] < P.THRESHOLD) & (np.abs(recs["delay_n"]) < d["delay_n_maximum"])
    if not (recs["detected"] == own).all():
        err.append("detected disagrees with the record's own metric and delay")
    band = in_band(ref_met)
    if not (recs["detected"].astype(bool) == ref_det)[~band].all():
        err.append("detected differs from the reference: %s" % np.nonzero((recs["detected"].astype(bool) != ref_det) & ~band)[0][:5])
    if stats is not None:
        stats["pairs"] += nof
        stats["band"] += int(band.sum())
        stats["dp"], stats["dm"] = max(stats["dp"], dp.max()), max(stats["dm"], dm.max())
    return err


@pytest.mark.parametrize("on_device", [False, True])
def test_fixture_cases(ctx, fx, on_device):
    idx = list(range(len(fx["cfg"])))
    sym_d, sym_off, pre_off, nrec = packed(fx, idx)
    res, pre = run(ctx, make_jobs(fx, idx, sym_off, pre_off), sym_d, nrec, on_device)
    stats = dict(pairs=0, band=0, dp=0.0, dm=0.0)
    bad = {}
    for n, i in enumerate(idx):
        e = check_case(fx, i, res[n], pre[pre_off[n]:pre_off[n] + int(fx["cfg"][i, P.C_NOF])], stats=stats)
        if e:
            bad[i] = e
    print("pairs %d, in the threshold band %d, largest deviation: peak power %.2e, metric %.2e" % (stats["pairs"], stats["band"], stats["dp"], stats["dm"]))
    assert not bad, "%d cases differ, e.g. %s" % (len(bad), dict(list(bad.items())[:5]))
    assert stats["band"] <= BAND_CAP * stats["pairs"]


def test_generated_sequences(ctx, fx):
    reqs = [(0, r, 0, 0) for r in range(838)] + [(4, r, 0, 0) for r in range(138)]
    reqs += [tuple(int(v) for v in c) for c in fx["gen_full_long_cfg"]] + [tuple(int(v) for v in c) for c in fx["gen_full_short_cfg"]]
    jobs = np.zeros(len(reqs), miphy.PrachGenJob)
    for n, (f, r, z, k) in enumerate(reqs):
        jobs[n] = (f, r, z, 0, k, 840 * n)
    for on_device in (False, True):
        out = torch.full((840 * len(reqs),), complex(7, 7), dtype=torch.complex64, device="cuda")
        ctx.prach_generate_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs, out)
        torch.cuda.synchronize()
        y = out.cpu().numpy().reshape(len(reqs), 840)
        assert np.abs(y[:838, fx["gen_positions_long"]] - fx["gen_roots_long"]).max() < 1e-5
        assert np.abs(y[838:976, fx["gen_positions_short"]] - fx["gen_roots_short"]).max() < 1e-5
        assert np.abs(y[976:984, :839] - fx["gen_full_long"]).max() < 1e-5
        assert np.abs(y[984:992, :139] - fx["gen_full_short"]).max() < 1e-5
        assert (y[:838, 839:] == complex(7, 7)).all() and (y[838:976, 139:] == complex(7, 7)).all()
    bad = jobs[:2].copy()
    bad[1]["restricted_set"] = 1
    out = torch.full((1680,), complex(7, 7), dtype=torch.complex64, device="cuda")
    with pytest.raises(Exception):
        ctx.prach_generate_batch(bad, out)
    ctx.prach_generate_batch(torch.from_numpy(bad.view(np.uint8).copy()).cuda(), out)  # on the device the bad one is skipped
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    assert (y[840:] == complex(7, 7)).all() and (y[:839] != complex(7, 7)).all()


def test_batch_of_512_is_bit_identical_to_cases_alone(ctx, fx):
    ncase = len(fx["cfg"])
    alone = {}
    for i in range(ncase):
        sym_d, so, po, nrec = packed(fx, [i])
        alone[i] = run(ctx, make_jobs(fx, [i], so, po), sym_d, nrec)
    rng = np.random.default_rng(5)
    idx = [n % ncase for n in range(512)]
    # symbols and record ranges placed in two different shuffled orders
    order_s, order_r = rng.permutation(512), rng.permutation(512)
    sym_off, pre_off = np.zeros(512, np.int64), np.zeros(512, np.int64)
    pos = 0
    for n in order_s:
        sym_off[n] = pos
        pos += len(fx["symbols"][idx[n]]) + int(rng.integers(0, 3))
    buf = np.zeros(pos, np.complex64)
    for n in range(512):
        buf[sym_off[n]:sym_off[n] + len(fx["symbols"][idx[n]])] = fx["symbols"][idx[n]]
    pos = 0
    for n in order_r:
        pre_off[n] = pos
        pos += int(fx["cfg"][idx[n], P.C_NOF])
    sym_d = torch.from_numpy(buf).cuda()
    jobs = make_jobs(fx, idx, sym_off, pre_off)
    for on_device in (False, True):
        res, pre = run(ctx, jobs, sym_d, pos, on_device)
        for n, i in enumerate(idx):
            nof = int(fx["cfg"][i, P.C_NOF])
            assert res[n].tobytes() == alone[i][0][0].tobytes(), (on_device, n)
            assert pre[pre_off[n]:pre_off[n] + nof].tobytes() == alone[i][1].tobytes(), (on_device, n)


def test_idft_3072_against_restatement(ctx, fx):
    idx = list(range(0, len(fx["cfg"]), 9))
    sym_d, sym_off, pre_off, nrec = packed(fx, idx)
    stats = dict(pairs=0, band=0, dp=0.0, dm=0.0)
    for on_device in (False, True):
        res, pre = run(ctx, make_jobs(fx, idx, sym_off, pre_off, 3072), sym_d, nrec, on_device)
        bad = {}
        for n, i in enumerate(idx):
            e = check_case(fx, i, res[n], pre[pre_off[n]:pre_off[n] + int(fx["cfg"][i, P.C_NOF])], 3072, stats)
            if e:
                bad[i] = e
        assert not bad, bad
    print("3072: pairs %d, band %d, largest deviation: peak power %.2e, metric %.2e" % (stats["pairs"], stats["band"], stats["dp"], stats["dm"]))
    assert stats["band"] <= BAND_CAP * stats["pairs"]
    # both sizes in one batch
    jobs = np.concatenate([make_jobs(fx, idx[:4], sym_off[:4], pre_off[:4], 1536), make_jobs(fx, idx[4:8], sym_off[4:8], pre_off[4:8], 3072)])
    res, pre = run(ctx, jobs, sym_d, int(pre_off[8]))
    for n, i in enumerate(idx[:8]):
        assert not check_case(fx, i, res[n], pre[pre_off[n]:pre_off[n] + int(fx["cfg"][i, P.C_NOF])], 1536 if n < 4 else 3072)


def test_one_and_zero_jobs_empty_range_and_zero_symbol(ctx, fx):
    cfg = fx["cfg"]
    empty = int(np.nonzero(cfg[:, P.C_NOF] == 0)[0][0])
    zero = int(np.nonzero((fx["tx_n"] == 0) & (fx["noise"] == 0) & (cfg[:, P.C_NOF] > 0))[0][0])
    for i in (0, len(cfg) - 1, empty, zero):
        sym_d, so, po, nrec = packed(fx, [i])
        res, pre = run(ctx, make_jobs(fx, [i], so, po), sym_d, nrec)
        assert not check_case(fx, i, res[0], pre)
    assert not fx["symbols"][zero].any()
    sym_d, so, po, nrec = packed(fx, [zero])
    res, pre = run(ctx, make_jobs(fx, [zero], so, po), sym_d, nrec)
    assert res[0]["rssi"] == 0 and not pre.view(np.uint8).any()
    # an empty range writes the occasion's result and no preamble record
    sym_d, so, po, _ = packed(fx, [empty])
    res, pre = run(ctx, make_jobs(fx, [empty], so, po), sym_d, 4)
    assert res[0]["delay_n_maximum"] > 0 and (pre.view(np.uint8) == SENT).all()
    # n = 0
    r = torch.full((16,), 7, dtype=torch.uint8, device="cuda")
    p = torch.full((40,), 7, dtype=torch.uint8, device="cuda")
    ctx.prach_detect_batch(np.zeros(0, miphy.PrachJob), sym_d, r, p)
    torch.cuda.synchronize()
    assert (r.cpu().numpy() == 7).all() and (p.cpu().numpy() == 7).all()


def pick(fx, short):
    cfg = fx["cfg"]
    m = (cfg[:, P.C_NOF] == 64) & ((cfg[:, P.C_FMT] >= 4) == short)
    return int(np.nonzero(m)[0][0])


@pytest.mark.parametrize("field,value", [("restricted_set", 1), ("restricted_set", 2), ("zero_correlation_zone", 16), ("range", (60, 5)),
                                         ("range", (0, 65)), ("idft_size", 768), ("idft_size", 2048), ("idft_size", 4608),
                                         ("format", 14), ("short_ra_scs", 4), ("short_ra_scs", 5)])
def test_invalid_host_jobs_rejected(ctx, fx, field, value):
    idx = [pick(fx, False), pick(fx, True)]
    sym_d, so, po, nrec = packed(fx, idx)
    jobs = make_jobs(fx, idx, so, po)
    if field == "range":
        jobs[0]["start_preamble_index"], jobs[0]["nof_preamble_indices"] = value
    elif field == "short_ra_scs":
        jobs[1]["ra_scs"] = value  # a long RA subcarrier spacing (4, 5) with a short format
    else:
        jobs[0][field] = value
    res = torch.full((2 * miphy.PrachResult.itemsize,), SENT, dtype=torch.uint8, device="cuda")
    pre = torch.full((nrec * REC,), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception):
        ctx.prach_detect_batch(jobs, sym_d, res, pre)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == SENT).all() and (pre.cpu().numpy() == SENT).all()


def test_skipped_device_jobs_and_unused_bytes_untouched(ctx, fx):
    a, b = pick(fx, False), pick(fx, True)
    idx = [a, b, a, b, a]
    sym_d, so, _, _ = packed(fx, idx)
    po = np.array([3, 80, 160, 240, 320])  # gaps of 13 .. 16 records between the ranges
    jobs = make_jobs(fx, idx, so, po)
    jobs[2]["restricted_set"] = 1
    jobs[3]["idft_size"] = 2048
    jobs[4]["start_preamble_index"], jobs[4]["nof_preamble_indices"] = 10, 20
    res, pre = run(ctx, jobs, sym_d, 400, on_device=True)
    raw = pre.view(np.uint8).reshape(400, REC)
    assert not check_case(fx, a, res[0], pre[3:67]) and not check_case(fx, b, res[1], pre[80:144])
    assert (res[2:4].view(np.uint8) == SENT).all()
    assert (raw[:3] == SENT).all() and (raw[67:80] == SENT).all() and (raw[144:320] == SENT).all() and (raw[340:] == SENT).all()
    assert (raw[320:340] != SENT).any(axis=1).all()
    # the third occasion's sub-range equals the same preambles of the full range
    assert pre[320:340].tobytes() == pre[3 + 10:3 + 30].tobytes()


def test_graph_capture_replay_with_changed_symbols(ctx, fx):
    idx = [i for i in range(len(fx["cfg"])) if fx["cfg"][i, P.C_FMT] < 4][:24]
    sym_d, so, po, nrec = packed(fx, idx)
    other = torch.from_numpy(np.concatenate([fx["symbols"][i] for i in idx[::-1]])).cuda()  # the same lengths, other contents
    jobs = make_jobs(fx, idx, so, po)
    ref_a = run(ctx, jobs, sym_d, nrec)
    ref_b = run(ctx, jobs, other, nrec)
    assert ref_a[1].tobytes() != ref_b[1].tobytes()
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    buf = sym_d.clone()
    res = torch.zeros(len(idx) * miphy.PrachResult.itemsize, dtype=torch.uint8, device="cuda")
    pre = torch.zeros(nrec * REC, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.prach_detect_batch(jobs_d, buf, res, pre, stream=s)  # warm-up (twiddles)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.prach_detect_batch(jobs_d, buf, res, pre, stream=s)
    for ref, src in ((ref_a, sym_d), (ref_b, other), (ref_a, sym_d)):
        buf.copy_(src)
        res.fill_(SENT), pre.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy(), ref[0].view(np.uint8).ravel())
        assert np.array_equal(pre.cpu().numpy(), ref[1].view(np.uint8).ravel())
