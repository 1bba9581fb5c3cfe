"""GPU: miphy_precoding_weights_batch against the float32 restatement of tests/precoding_weights_ref.py, byte for byte, on the cases of
tests/precoding_weights_cases.py (tests/test_precoding_weights.py holds that restatement to float64 numpy.linalg on the CPU and asserts the coverage):
every A x U x l for one UE; 2, 3 and 4 UEs with L = A and L < A at reg = 0 and reg > 0; a band that starts off the output PRGs (overlaps of 1 and 3
PRBs) with output PRGs below and above it; 65 output PRGs (the lane form over a wavefront border); one wideband PRG over 72 SRS PRGs and six PRGs of 12
(the wave form over 64 lanes and over a workgroup); 8 and 9 SRS PRGs under a PRG (the border between the forms); zero and rank-deficient channels.
Every call starts with sentinels in the weights and the metrics, and only owned elements may change."""
import ctypes as C

import numpy as np
import pytest

import miphy
import precoding_weights_cases as G
import precoding_weights_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WS, MS = np.complex64(7.5 - 3.25j), np.float32(-123.5)  # sentinels


@pytest.fixture(scope="module")
def prepared():
    """All cases as one batch, their float32 reference computed once: (jobs, records, h on the device, layout, expected weights, expected metrics)."""
    jobs = G.all_jobs()
    rec, h, lay = G.records(miphy, jobs)
    w, m = np.full(lay["nw"], WS, np.complex64), np.full(lay["nm"], MS, np.float32)
    with np.errstate(all="ignore"):
        for j, ues in zip(jobs, lay["ues"]):
            for (wo, nw, mo, nm), (W, M) in zip(ues, R.weights32(j)):
                w[wo:wo + nw], m[mo:mo + nm] = W.ravel(), M.ravel()
    return dict(jobs=jobs, rec=rec, h=torch.from_numpy(h).cuda(), lay=lay, w=w, m=m)


def buffers(pre):
    return (torch.full((pre["lay"]["nw"],), complex(WS), dtype=torch.complex64, device="cuda"),
            torch.full((pre["lay"]["nm"],), float(MS), dtype=torch.float32, device="cuda"))


def run(ctx, pre, rec=None, on_device=False, metrics=True):
    rec = pre["rec"] if rec is None else rec
    w, m = buffers(pre)
    j = torch.from_numpy(rec.view(np.uint8).copy()).cuda() if on_device else rec
    ctx.precoding_weights_batch(j, pre["h"], w, m if metrics else None, jobs_on_device=on_device)
    torch.cuda.synchronize()
    return w.cpu().numpy(), m.cpu().numpy()


def expected(pre, only=None):
    """The buffers with the jobs `only` (default: all) written and sentinels everywhere else."""
    if only is None:
        return pre["w"], pre["m"]
    w, m = np.full_like(pre["w"], WS), np.full_like(pre["m"], MS)
    for i in only:
        for wo, nw, mo, nm in pre["lay"]["ues"][i]:
            w[wo:wo + nw], m[mo:mo + nm] = pre["w"][wo:wo + nw], pre["m"][mo:mo + nm]
    return w, m


def same(got, want, what):
    """Byte equality, with the first differing elements in the message."""
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(len(got), -1) != want.view(np.uint32).reshape(len(want), -1)).any(axis=1))
        raise AssertionError("%s: %d elements differ, the first at %d: %r != %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def test_every_case_in_one_batch_equals_the_float32_restatement(ctx, prepared):
    w, m = run(ctx, prepared)
    assert np.isfinite(w.view(np.float32)).all() and np.isfinite(m).all()
    for i, (j, ues) in enumerate(zip(prepared["jobs"], prepared["lay"]["ues"])):  # per job first, for a message that names the case
        for k, (wo, nw, mo, nm) in enumerate(ues):
            tag = "job %d (A %d, layers %s, S %d, wave %s) UE %d" % (i, j["A"], [u["l"] for u in j["ues"]], j["S"], R.wave_form(j), k)
            same(w[wo:wo + nw], prepared["w"][wo:wo + nw], tag + " weights")
            same(m[mo:mo + nm], prepared["m"][mo:mo + nm], tag + " metrics")
    same(w, prepared["w"], "weights and the sentinels around them")
    same(m, prepared["m"], "metrics and the sentinels around them")


def test_metrics_null(ctx, prepared):
    w, m = run(ctx, prepared, metrics=False)
    same(w, prepared["w"], "weights")
    assert (m == MS).all()


def test_a_job_alone_and_in_a_batch_of_64_in_two_orders_gives_the_same_bits(ctx, prepared):
    n = len(prepared["jobs"])
    pick = np.array([(7 * k) % n for k in range(64)])  # both forms, 65 PRGs and the wideband PRG among them; jobs repeat and rewrite the same bytes
    want = expected(prepared, only=set(pick.tolist()))
    first = run(ctx, prepared, rec=prepared["rec"][pick])
    second = run(ctx, prepared, rec=prepared["rec"][pick][np.random.default_rng(5).permutation(64)])
    for got in (first, second):
        same(got[0], want[0], "weights"), same(got[1], want[1], "metrics")
    forms = {R.wave_form(prepared["jobs"][i]) for i in pick}
    assert forms == {False, True}
    for i in sorted({int(x) for x in pick[[0, 9, 24, 37, 63]]} | {n - 1}):
        want = expected(prepared, only=[i])
        got = run(ctx, prepared, rec=prepared["rec"][i:i + 1])
        same(got[0], want[0], "job %d alone: weights" % i), same(got[1], want[1], "job %d alone: metrics" % i)


def test_device_resident_jobs_equal_host_jobs_and_an_invalid_one_is_skipped(ctx, prepared):
    got = run(ctx, prepared, on_device=True)
    same(got[0], prepared["w"], "weights"), same(got[1], prepared["m"], "metrics")
    broken = prepared["rec"].copy()
    n = len(broken)
    broken["nof_ports"][3] = 5
    broken["ue"]["nof_layers"][24, 1] = 3  # more layers than the UE has ports
    broken["ue"]["weights_offset"][30, 0] = prepared["lay"]["nw"]  # its weights would leave the buffer
    broken["amplitude"][40] = 0.0
    want = expected(prepared, only=set(range(n)) - {3, 24, 30, 40})
    got = run(ctx, prepared, rec=broken, on_device=True)
    same(got[0], want[0], "weights"), same(got[1], want[1], "metrics")


def test_device_jobs_captured_in_a_graph(ctx, prepared):
    """The call only enqueues: with device-resident jobs it is captured once and replayed three times, each time with the bytes of the direct call."""
    jobs_d = torch.from_numpy(prepared["rec"].view(np.uint8).copy()).cuda()
    w, m = buffers(prepared)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.precoding_weights_batch(jobs_d, prepared["h"], w, m, jobs_on_device=True, stream=s)  # warm-up: the code objects are loaded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.precoding_weights_batch(jobs_d, prepared["h"], w, m, jobs_on_device=True, stream=s)
    for _ in range(3):
        w.fill_(complex(WS)), m.fill_(float(MS))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(w.cpu().numpy(), prepared["w"], "weights"), same(m.cpu().numpy(), prepared["m"], "metrics")


def _set(**fields):
    def f(rec):
        for k, v in fields.items():
            if k.startswith("ue"):
                rec["ue"][int(k[2])][k[4:]] = v
            else:
                rec[k] = v
    return f


# (case, argument replaced by NULL, change to the last job, text of the rule)
REJECTIONS = [("null context", 0, None, "null argument"), ("null jobs", 1, None, "null argument"), ("null h", 4, None, "null argument"),
              ("null weights", 5, None, "null argument"),
              ("no UE", None, _set(nof_ues=0), "nof_ues is 1..4"),
              ("five ports", None, _set(nof_ports=5), "nof_ports is 1..4"),
              ("no PRG", None, _set(nof_prg=0), "prg_size and nof_prg are at least 1"),
              ("negative reg", None, _set(reg=-1.0), "reg is finite and not negative"),
              ("zero amplitude", None, _set(amplitude=0.0), "amplitude is a positive normal number"),
              ("SRS PRGs of 3", None, _set(ue0_prg_size=3), "SRS prg_size of a UE is 1, 2 or 4"),
              ("band of 6 PRB", None, _set(ue0_nof_prb=6), "the sounded band of a UE"),
              ("three UE ports", None, _set(ue0_nof_ue_ports=3), "nof_ue_ports of a UE is 1, 2 or 4"),
              ("no layer", None, _set(ue1_nof_layers=0), "nof_layers of a UE is 1..nof_ue_ports"),
              ("five layers", None, _set(ue0_nof_layers=2, ue0_nof_ue_ports=4, ue1_nof_layers=1, nof_ports=2), "at most 4 and at most nof_ports"),
              ("weights outside", None, _set(ue1_weights_offset=2 ** 31), "leave `weights`")]


@pytest.mark.parametrize("case,null,change,rule", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_a_rejected_batch_writes_nothing(ctx, prepared, case, null, change, rule):
    rec = prepared["rec"][20:32].copy()  # the last one: two UEs
    assert rec["nof_ues"][-1] >= 2
    if change:
        change(rec[-1])
    w, m = buffers(prepared)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(j, n, null=None):
        args = [ctx.h, C.c_void_p(j.ctypes.data), 0, n, C.c_void_p(prepared["h"].data_ptr()), C.c_void_p(w.data_ptr()), w.numel(),
                C.c_void_p(m.data_ptr()), stream]
        if null is not None:
            args[null] = None
        return miphy.lib().miphy_precoding_weights_batch(*args)

    assert call(rec, rec.size, null) == -1
    msg = miphy.lib().miphy_last_error().decode()
    assert rule in msg and (null is not None or "job %d: " % (rec.size - 1) in msg), msg
    assert call(prepared["rec"], 0) == 0  # n == 0 enqueues nothing
    torch.cuda.synchronize()
    assert bool((w == complex(WS)).all()) and bool((m == float(MS)).all())
