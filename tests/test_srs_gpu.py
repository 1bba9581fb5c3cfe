"""GPU: miphy_srs_pilots_batch and miphy_srs_estimate_batch. The 23.5 reference has no SRS code, so every check is against the numpy transmitter
(tests/srs_tx.py) and the float64 receiver (tests/srs_ref.py) on the cases of tests/srs_cases.py, whose coverage and conditions tests/test_srs_ref.py
asserts on the CPU:
 - pilots within 2e-6 absolute of the float64 sequences (unit modulus, integer-reduced phase, single-precision sine and cosine);
 - H and H_wb within 1e-4 of the job's largest |H|; phi (read back from time_alignment_s) within 1e-5 rad; noise_var within 1e-2 relative where noise
   was added (all cases are at or below 30 dB) and below 1e-7 of the EPRE where not; EPRE and RSRP within 1e-4 relative; SINR within 0.05 dB where noise
   was added. The bound on H comes from the single-precision rounding of the compensation angle (about 2e-5 rad at 300 rad, times five). The kernel
   refers that angle to the PRG centre and takes phi in double, so it stays far inside.
   Worst measured on the MI355X over all cases (3/4 of the delay range at M = 1632 among them, 3845 rad at the last element): H 1.48e-7 and H_wb
   2.41e-7 of the largest |H|, phi 7.8e-8 rad, pilots 2.23e-7, noise_var / EPRE without noise 2.3e-14.
Every call starts with sentinels in h_out, in the records (two more than there are jobs) and in pilots, and only owned elements may change."""
import ctypes as C

import numpy as np
import pytest

import miphy
import srs_cases as G
import srs_tx as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BYTE, HS = 0xEE, np.complex64(7.5 - 3.25j)  # sentinels
RES = miphy.SrsResult.itemsize
WORST = dict(h=0.0, h_wb=0.0, phi=0.0, pilots=0.0, noise_free=0.0)


def sizes(p):
    d = X.derive(p)
    return d["G"] * p["R"] * p["nap"], p["nsym"] * p["nap"] * d["M"]


def prepare(items):
    """Jobs over one concatenation of the items' distinct grids, with sentinel elements between the jobs' estimates and pilots."""
    jobs = np.zeros(len(items), miphy.SrsJob)
    grids, goff, total, ho, po, h_, p_ = [], {}, 0, [], [], 3, 5
    for i, it in enumerate(items):
        if id(it["grid"]) not in goff:
            goff[id(it["grid"])] = total
            grids.append(it["grid"].ravel())
            total += it["grid"].size
        ho.append(h_), po.append(p_)
        jobs[i] = X.job_of(it["p"], goff[id(it["grid"])], h_, p_)
        nh, npil = sizes(it["p"])
        h_ += nh + 3
        p_ += npil + 2
    return dict(jobs=jobs, grid=torch.from_numpy(np.concatenate(grids)).cuda(), ho=ho, po=po, nh=h_ + 8, npil=p_ + 8)


def buffers(pre, njobs):
    return (torch.full((pre["nh"],), complex(HS), dtype=torch.complex64, device="cuda"), torch.full(((njobs + 2) * RES,), BYTE, dtype=torch.uint8, device="cuda"))


def run(ctx, pre, jobs=None, on_device=False):
    """(h, records) of one call; both buffers start as sentinels, two records more than jobs."""
    jobs = pre["jobs"] if jobs is None else jobs
    h, res = buffers(pre, len(jobs))
    j = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs
    ctx.srs_estimate_batch(j, pre["grid"], h, res, jobs_on_device=on_device)
    torch.cuda.synchronize()
    return h.cpu().numpy(), res.cpu().numpy().view(miphy.SrsResult)


def assert_sentinels(pre, items, out, only=None):
    h, res = out
    owned = np.zeros(pre["nh"], bool)
    n = len(res) - 2
    written = range(n) if only is None else sorted(only)
    for i in written:
        owned[pre["ho"][i]:pre["ho"][i] + sizes(items[i]["p"])[0]] = True
    assert (h[~owned] == HS).all(), "estimates outside the jobs"
    assert (res[n:].view(np.uint8) == BYTE).all(), "records beyond the jobs"
    for i in range(n):
        if i in written:
            assert (res[i]["reserved"].view(np.uint8) == BYTE).all(), i
        else:
            assert (res[i:i + 1].view(np.uint8) == BYTE).all(), i


def check_items(items, pre, out):
    """Everything one call wrote for `items` against the float64 receiver."""
    h, res = out
    bad = []  # every mismatch of the call, so that one run shows them all

    def want(ok, *what):
        if not ok:
            bad.append(what)

    for i, it in enumerate(items):
        p, ref, r, d = it["p"], it["ref"], res[i], X.derive(it["p"])
        tag = "job %d: %s" % (i, p)
        H = h[pre["ho"][i]:pre["ho"][i] + ref["H"].size].astype(np.complex128).reshape(ref["H"].shape)
        scale = np.abs(ref["H"]).max()
        e = np.abs(H - ref["H"]).max() / scale
        WORST["h"] = max(WORST["h"], e)
        want(e <= 1e-4, tag, "H", e)
        hwb = r["h_wb"][..., 0].astype(np.complex128) + 1j * r["h_wb"][..., 1]
        e = np.abs(hwb - ref["h_wb"]).max() / scale
        WORST["h_wb"] = max(WORST["h_wb"], e)
        want(e <= 1e-4, tag, "H_wb", e)
        want(not hwb[p["R"]:].any() and not hwb[:, p["nap"]:].any() and not r["rsrp_db"][p["nap"]:].any(), tag, "entries of unused ports")
        phi = -float(r["time_alignment_s"]) * 2 * np.pi * 15e3 * 2 ** p["numerology"] * p["K"] * d["P"]
        WORST["phi"] = max(WORST["phi"], abs(phi - ref["phi"]))
        want(abs(phi - ref["phi"]) <= 1e-5, tag, "phi", phi, ref["phi"])
        epre = 10 ** (float(r["epre_db"]) / 10)
        want(abs(epre - ref["epre"]) <= 1e-4 * ref["epre"], tag, "epre", epre, ref["epre"])
        rsrp = 10 ** (r["rsrp_db"][:p["nap"]].astype(np.float64) / 10)
        want((np.abs(rsrp - ref["rsrp"]) <= 1e-4 * ref["rsrp"]).all(), tag, "rsrp", rsrp, ref["rsrp"])
        if it["snr_db"] is None:
            WORST["noise_free"] = max(WORST["noise_free"], float(r["noise_var"]) / epre)
            want(0 <= float(r["noise_var"]) < 1e-7 * epre, tag, "noise_var of a noise-free grid over the EPRE", float(r["noise_var"]) / epre)
        else:
            assert it["snr_db"] <= 30
            want(abs(float(r["noise_var"]) - ref["noise_var"]) <= 1e-2 * ref["noise_var"], tag, "noise_var", float(r["noise_var"]), ref["noise_var"])
            want(abs(float(r["sinr_db"]) - 10 * np.log10(ref["sinr"])) <= 0.05, tag, "sinr_db", float(r["sinr_db"]), 10 * np.log10(ref["sinr"]))
    assert not bad, "%d mismatches, the first: %s" % (len(bad), bad[:8])


def report():
    print("worst so far: H %.3g and H_wb %.3g of the largest |H|, phi %.3g rad, pilots %.3g, noise_var / EPRE without noise %.3g" % (
        WORST["h"], WORST["h_wb"], WORST["phi"], WORST["pilots"], WORST["noise_free"]))


def test_pilots(ctx):
    items = G.shapes_set() + G.multiplexed_set()
    pre = prepare(items)
    for on_device in (False, True):
        pil = torch.full((pre["npil"],), complex(HS), dtype=torch.complex64, device="cuda")
        j = torch.from_numpy(pre["jobs"].view(np.uint8).copy()).cuda() if on_device else pre["jobs"]
        ctx.srs_pilots_batch(j, pil, jobs_on_device=on_device)
        torch.cuda.synchronize()
        got, owned = pil.cpu().numpy(), np.zeros(pre["npil"], bool)
        for i, it in enumerate(items):
            want = X.pilots(it["p"]).ravel()
            mine = got[pre["po"][i]:pre["po"][i] + want.size]
            owned[pre["po"][i]:pre["po"][i] + want.size] = True
            e = np.abs(mine - want).max()
            WORST["pilots"] = max(WORST["pilots"], e)
            assert e <= 2e-6, (i, it["p"], e)
        assert (got[~owned] == HS).all(), "pilots outside the jobs"
    report()


def test_every_shape(ctx):
    """M = 12, 36, 48, 72 and 1632; 1 / 2 / 4 transmit ports on one comb and on two; 1 / 2 / 4 symbols; 1 and 4 receive ports; every PRG size;
    hopping 0 / 1 / 2; slots 0 and 19; delays up to 3/4 of the range; with and without noise (tests/test_srs_ref.py asserts the coverage)."""
    items = G.shapes_set()
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, pre, out)
    assert_sentinels(pre, items, out)
    report()


def test_ues_multiplexed_in_one_grid_and_one_call(ctx):
    """Other comb offset, other cyclic shift (as the second port of a two-port job), adjacent PRBs: each job finds its own UE."""
    items = G.multiplexed_set()
    assert len({id(it["grid"]) for it in items}) == 1
    pre = prepare(items)
    out = run(ctx, pre)
    check_items(items, pre, out)
    assert_sentinels(pre, items, out)
    for i, it in enumerate(items):  # and what it finds is the channel that was sent, to the noise of 25 dB averaged over a PRG
        H = out[0][pre["ho"][i]:pre["ho"][i] + it["ref"]["H"].size].reshape(it["ref"]["H"].shape)
        for port in range(it["tx"]["nap"]):
            assert np.abs(H[:, :, port] - it["Hg"][:, :, port]).max() <= 0.15, (i, port)
    report()


def batch_of_64():
    base = G.shapes_set() + G.multiplexed_set()
    return [base[(7 * k) % len(base)] for k in range(64)]


def test_a_job_alone_and_in_a_batch_of_64_in_two_orders_gives_the_same_bits(ctx):
    items = batch_of_64()
    pre = prepare(items)
    first = run(ctx, pre)
    perm = np.random.default_rng(5).permutation(64)
    second = run(ctx, pre, jobs=pre["jobs"][perm])
    assert first[0].tobytes() == second[0].tobytes()
    assert first[1][:64][perm].tobytes() == second[1][:64].tobytes()
    for i in (0, 9, 24, 37, 63):  # position 24 is the largest case: 272 PRB, four ports on two combs, four symbols, four receive ports
        alone = run(ctx, pre, jobs=pre["jobs"][i:i + 1])
        nh = sizes(items[i]["p"])[0]
        assert alone[0][pre["ho"][i]:pre["ho"][i] + nh].tobytes() == first[0][pre["ho"][i]:pre["ho"][i] + nh].tobytes(), i
        assert alone[1][0].tobytes() == first[1][i].tobytes(), i
        owned = np.zeros(pre["nh"], bool)
        owned[pre["ho"][i]:pre["ho"][i] + nh] = True
        assert (alone[0][~owned] == HS).all() and (alone[1][1:].view(np.uint8) == BYTE).all(), i


def test_device_resident_jobs_equal_host_jobs_and_an_invalid_one_is_skipped(ctx):
    items = G.shapes_set()[:12] + G.multiplexed_set()
    pre = prepare(items)
    host = run(ctx, pre)
    dev = run(ctx, pre, on_device=True)
    assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes()
    broken = pre["jobs"].copy()
    broken["nof_tx_ports"][6] = 3
    broken["comb_offset"][9] = broken["comb_size"][9]
    out = run(ctx, pre, jobs=broken, on_device=True)
    keep = set(range(len(items))) - {6, 9}
    assert_sentinels(pre, items, out, only=keep)
    for i in keep:
        nh = sizes(items[i]["p"])[0]
        assert out[1][i].tobytes() == host[1][i].tobytes(), i
        assert out[0][pre["ho"][i]:pre["ho"][i] + nh].tobytes() == host[0][pre["ho"][i]:pre["ho"][i] + nh].tobytes(), i
    pil = torch.full((pre["npil"],), complex(HS), dtype=torch.complex64, device="cuda")
    ctx.srs_pilots_batch(torch.from_numpy(broken.view(np.uint8).copy()).cuda(), pil, jobs_on_device=True)
    torch.cuda.synchronize()
    got = pil.cpu().numpy()
    for i in (6, 9):
        assert (got[pre["po"][i]:pre["po"][i] + sizes(items[i]["p"])[1]] == HS).all(), i


def test_device_jobs_captured_in_a_graph(ctx):
    """The call only enqueues: with device-resident jobs it is captured once and replayed three times, each time with the bytes of the direct call."""
    items = G.shapes_set()[:12] + G.multiplexed_set()
    pre = prepare(items)
    want = run(ctx, pre)
    jobs_d = torch.from_numpy(pre["jobs"].view(np.uint8).copy()).cuda()
    h, res = buffers(pre, len(items))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.srs_estimate_batch(jobs_d, pre["grid"], h, res, jobs_on_device=True, stream=s)  # warm-up (Gold tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.srs_estimate_batch(jobs_d, pre["grid"], h, res, jobs_on_device=True, stream=s)
    for _ in range(3):
        h.fill_(complex(HS)), res.fill_(BYTE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert h.cpu().numpy().tobytes() == want[0].tobytes() and res.cpu().numpy().tobytes() == want[1].tobytes()


def _set(**fields):
    def f(job):
        for k, v in fields.items():
            job[k] = v
    return f


# (case, argument replaced by NULL, change to the last job, code, text of the rule)
REJECTIONS = [("null context", 0, None, -1, "null argument"), ("null jobs", 1, None, -1, "null argument"), ("null grid", 4, None, -1, "null argument"),
              ("null h_out", 5, None, -1, "null argument"), ("null results", 6, None, -1, "null argument"),
              ("three transmit ports", None, _set(nof_tx_ports=3), -1, "invalid number of transmit ports"),
              ("five receive ports", None, _set(nof_rx_ports=5), -1, "invalid number of receive ports"),
              ("window too narrow", None, _set(grid_nprb=3), -1, "leaves the grid window"),
              ("prg of one PRB for two ports at comb 4", None, _set(nof_tx_ports=2, prg_size=1), -1, "not a multiple of the ports that share the comb"),
              ("24 elements", None, _set(start_prb=0, nof_prb=8), -4, "Table 5.2.2.2-4")]


@pytest.mark.parametrize("case,null,change,code,rule", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_a_rejected_batch_writes_nothing(ctx, case, null, change, code, rule):
    items = G.multiplexed_set()  # the last job: comb 4, one port, 4 PRB
    pre = prepare(items)
    jobs = pre["jobs"].copy()
    if change:
        change(jobs[-1])
    h, res = buffers(pre, len(jobs))
    pil = torch.full((pre["npil"],), complex(HS), dtype=torch.complex64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(j, n, null=None):
        args = [ctx.h, C.c_void_p(j.ctypes.data), 0, n, C.c_void_p(pre["grid"].data_ptr()), C.c_void_p(h.data_ptr()), C.c_void_p(res.data_ptr()), stream]
        if null is not None:
            args[null] = None
        return miphy.lib().miphy_srs_estimate_batch(*args)

    assert call(jobs, jobs.size, null) == code
    assert rule in miphy.lib().miphy_last_error().decode(), miphy.lib().miphy_last_error().decode()
    if change:  # the pilots call applies the same rules
        assert miphy.lib().miphy_srs_pilots_batch(ctx.h, C.c_void_p(jobs.ctypes.data), 0, jobs.size, C.c_void_p(pil.data_ptr()), stream) == code
        assert ("job %d: " % (jobs.size - 1)) in miphy.lib().miphy_last_error().decode() and rule in miphy.lib().miphy_last_error().decode()
    assert call(pre["jobs"], 0) == 0  # n == 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((h == complex(HS)).all()) and bool((res == BYTE).all()) and bool((pil == complex(HS)).all())
