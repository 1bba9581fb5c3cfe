"""GPU: miphy_channel_precode_batch (channel_precoder::apply_precoding, batched) against the numerical contract of tests/pdsch_precoded_cases.py: every
(layers, ports) pair with every size in ONE batch at odd offsets and strides, with host jobs and with device-resident jobs; the output starts as
dl_grid.background() and everything outside the rows a job owns (guards, the gaps between rows) is compared on its bits; the job rules, host and device."""
import numpy as np
import pytest

import dl_grid as D
import pdsch_precoded_cases as XC

pytestmark = pytest.mark.gpu
LP = [(1, 1), (1, 4), (2, 2), (2, 4), (3, 4), (4, 4), (4, 8), (4, 16), (2, 16)]
NOF_RE = [1, 63, 64, 65, 257, 3300]
G = XC.GUARD


def _batch(miphy):
    """One job per (L, P) and size. Weights: the matrices back to back behind gaps of 1, 2, 3 foreign entries. Input: layer rows at a stride of
    nof_re + 1 or + 2 behind an odd offset. Output: [guard | rows at a stride of nof_re + 1 .. 3 | guard] per job, from the background."""
    jobs, ws, xs, outs, meta = [], [], [], [], []
    wo = xo = oo = 0
    for k, ((L, P), n) in enumerate((lp, n) for lp in LP for n in NOF_RE):
        W = XC.weights("precoder %d" % k, (P, L))
        x = XC.weights("precoder input %d" % k, (L, n)) * np.float32(1.5)
        gap_w, in_stride, out_stride = 1 + k % 3, n + 1 + k % 2, n + 1 + k % 3
        ws += [np.full(gap_w, np.nan + 1j * np.nan, np.complex64), W.reshape(-1)]
        xin = np.full(1 + L * in_stride, np.nan + 1j * np.nan, np.complex64)  # (a NaN read from a gap poisons the result)
        for ly in range(L):
            xin[1 + ly * in_stride:1 + ly * in_stride + n] = x[ly]
        out = D.background(G + P * out_stride + G, np.random.default_rng(1000 + k))
        j = np.zeros(1, dtype=miphy.PrecodeJob)[0]
        j["nof_re"], j["nof_layers"], j["nof_ports"], j["weights_offset"] = n, L, P, wo + gap_w
        j["in_offset"], j["in_stride"], j["out_offset"], j["out_stride"] = xo + 1, in_stride, oo + G, out_stride
        jobs.append(j), xs.append(xin), outs.append(out), meta.append((L, P, n, out_stride, W, x))
        wo += gap_w + W.size
        xo += xin.size
        oo += out.size
    return np.array(jobs, dtype=miphy.PrecodeJob), np.concatenate(ws), np.concatenate(xs), outs, meta


def _run(ctx, jobs, w, x, outs, on_device):
    import torch
    od = torch.from_numpy(np.concatenate(outs)).cuda()
    err = None
    try:
        if on_device:
            ctx.channel_precode_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(x).cuda(), od)
        else:
            ctx.channel_precode_batch(jobs, w, torch.from_numpy(x).cuda(), od)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    got, out, o = od.cpu().numpy(), [], 0
    for b in outs:
        out.append(got[o:o + b.size])
        o += b.size
    return err, out


def _check_job(got, bg, m, what):
    L, P, n, out_stride, W, x = m
    rows = np.zeros(bg.size, bool)
    for a in range(P):
        rows[G + a * out_stride:G + a * out_stride + n] = True
    keep = np.repeat(~rows, 2)
    assert np.array_equal(D.bits(got)[keep], D.bits(bg)[keep]), "%s: a guard or a gap between rows lost its background" % what
    y, A = XC.precode_ref(W, x)
    XC.assert_within(got[rows].reshape(P, n), y, A, L, what)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_jobs", "device_jobs"])
def test_one_batch_of_every_shape(ctx, on_device):
    import miphy
    jobs, w, x, outs, meta = _batch(miphy)
    assert {int(j["weights_offset"]) % 2 for j in jobs} == {0, 1} and {int(j["out_stride"]) % 2 for j in jobs} == {0, 1}
    err, got = _run(ctx, jobs, w, x, outs, on_device)
    assert err is None, err
    for g, bg, m in zip(got, outs, meta):
        _check_job(g, bg, m, "L = %d, P = %d, %d REs" % m[:3])


def _few_ports(j, w):
    j["nof_ports"] = int(j["nof_layers"]) - 1


def _beyond_weights(j, w):
    j["weights_offset"] = w.size - int(j["nof_ports"]) * int(j["nof_layers"]) + 1


def _empty_beyond_weights(j, w):
    j["nof_re"] = 0
    _beyond_weights(j, w)


BREAKS = [(_few_ports, "invalid number of antenna ports 3 (4..16)"), (_beyond_weights, "exceed the"), (_empty_beyond_weights, "exceed the")]
BREAK_IDS = ["ports_below_layers", "weights_beyond_array", "no_re_and_weights_beyond_array"]


def _three_jobs(miphy):
    """The jobs (2, 4) x 65, (4, 8) x 64 and (4, 4) x 257 of the batch; the middle one is the one to break."""
    jobs, w, x, outs, meta = _batch(miphy)
    pick = [LP.index(lp) * len(NOF_RE) + NOF_RE.index(n) for lp, n in (((2, 4), 65), ((4, 8), 64), ((4, 4), 257))]
    jobs = jobs[pick].copy()
    o = 0
    for j, k in zip(jobs, pick):
        j["out_offset"] = o + G
        o += outs[k].size
    return jobs, w, x, [outs[k] for k in pick], [meta[k] for k in pick]


@pytest.mark.parametrize("k", range(len(BREAKS)), ids=BREAK_IDS)
def test_host_job_breaking_a_rule_is_refused(ctx, k):
    """MIPHY_EINVAL with the rule's message before anything is enqueued: every output still holds its background."""
    import miphy
    edit, msg = BREAKS[k]
    jobs, w, x, outs, meta = _three_jobs(miphy)
    edit(jobs[1], w)
    err, got = _run(ctx, jobs, w, x, outs, False)
    assert err is not None and "miphy error -1" in err and "channel_precode: job 1: " in err and msg in err, err
    for g, bg in zip(got, outs):
        assert np.array_equal(D.bits(g), D.bits(bg))


@pytest.mark.parametrize("k", range(len(BREAKS)), ids=BREAK_IDS)
def test_device_job_breaking_a_rule_is_skipped(ctx, k):
    """The same job on the device between two good ones: its output keeps the background, the neighbours are written."""
    import miphy
    edit, msg = BREAKS[k]
    jobs, w, x, outs, meta = _three_jobs(miphy)
    edit(jobs[1], w)
    err, got = _run(ctx, jobs, w, x, outs, True)
    assert err is None, err
    assert np.array_equal(D.bits(got[1]), D.bits(outs[1]))
    for i in (0, 2):
        _check_job(got[i], outs[i], meta[i], "neighbour %d" % i)
