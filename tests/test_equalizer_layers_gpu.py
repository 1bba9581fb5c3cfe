"""GPU: miphy_channel_equalize_layers_batch (1..4 layers on 1..4 ports) against the numpy float32 restatement of its arithmetic
(tests/pusch_layers_cases.py zf_single, pinned to the oracle and to float64 in tests/test_pusch_layers.py) and against the old entry point."""
import numpy as np
import pytest

import pusch_layers_cases as PL

pytestmark = pytest.mark.gpu
GUARD = 7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(ctx, cases, device_jobs=False, entry="channel_equalize_layers_batch"):
    """cases: list of (y [P][n], h [L][P][n], noise_var, tx). One batch; GUARD sentinel elements between the outputs of the jobs.
    Returns [(x [L][n], nv [L][n])] and the two raw output arrays."""
    import torch
    import miphy
    jobs, ys, hs = [], [], []
    yo = ho = zo = 0
    spans = []
    for y, h, nvar, tx in cases:
        nl, npt, n = h.shape
        zo += GUARD
        jobs.append(PL.equalizer_job(miphy, n, npt, nl, nvar, tx, yo, ho, zo, zo))
        spans.append((zo, nl, n))
        ys.append(y.reshape(-1))
        hs.append(h.reshape(-1))
        yo += y.size
        ho += h.size
        zo += nl * n
    zo += GUARD
    jobs = np.array(jobs, dtype=miphy.EqualizerJob)
    if device_jobs:
        jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    y_d = torch.from_numpy(np.concatenate(ys)).cuda()
    h_d = torch.from_numpy(np.concatenate(hs)).cuda()
    z_d = torch.full((zo,), 77.0 + 5.0j, dtype=torch.complex64, device="cuda")
    v_d = torch.full((zo,), -3.0, dtype=torch.float32, device="cuda")
    getattr(ctx, entry)(jobs, y_d, h_d, z_d, v_d)
    torch.cuda.synchronize()
    z, v = z_d.cpu().numpy(), v_d.cpu().numpy()
    return [(z[o:o + nl * n].reshape(nl, n), v[o:o + nl * n].reshape(nl, n)) for o, nl, n in spans], z, v, spans


def _guards_untouched(z, v, spans):
    keep = np.ones(z.size, bool)
    for o, nl, n in spans:
        keep[o:o + nl * n] = False
    assert np.all(z[keep] == np.complex64(77.0 + 5.0j)) and np.all(v[keep] == -3.0)


def _case(rng, nl, npt, n, nvar=0.03):
    h, _ = PL.channels(rng, nl, npt, n)
    y = (rng.standard_normal((npt, n)) + 1j * rng.standard_normal((npt, n))).astype(np.complex64)
    return y, h, nvar


@pytest.mark.parametrize("device_jobs", [False, True])
def test_all_topologies_bit_equal_to_the_restatement(ctx, device_jobs):
    """1 000 elements (no multiple of the 256-thread tile) and 1 300 (two blocks) per topology, tx_scaling 1 and != 1, one batch, guards between."""
    rng = np.random.default_rng(5)
    cases = []
    for nl, npt in PL.TOPOLOGIES:
        for n, tx in ((1000, 1.0), (1300, 0.6)):
            y, h, nvar = _case(rng, nl, npt, n)
            cases.append((y, h, nvar, tx))
    out, z, v, spans = _run(ctx, cases, device_jobs)
    for (y, h, nvar, tx), (x, nv) in zip(cases, out):
        ex, ev = PL.zf_single(y, h, nvar, tx)
        assert np.array_equal(_bits(x), _bits(ex)), h.shape
        assert np.array_equal(_bits(nv), _bits(ev)), h.shape
    _guards_untouched(z, v, spans)


def test_reference_topologies_byte_equal_to_the_old_entry_point(ctx):
    rng = np.random.default_rng(6)
    cases = []
    for nl, npt in ((1, 1), (1, 2), (1, 3), (1, 4), (2, 2)):
        y, h, nvar = _case(rng, nl, npt, 1000)
        h[:, :, 17] = 0
        cases.append((y, h, nvar, 0.9))
    new = _run(ctx, cases)[0]
    old = _run(ctx, cases, entry="channel_equalize_batch")[0]
    for (x, nv), (xo, nvo) in zip(new, old):
        assert np.array_equal(_bits(x), _bits(xo)) and np.array_equal(_bits(nv), _bits(nvo))


def test_abnormal_elements_give_zero_and_infinity_on_every_layer(ctx):
    rng = np.random.default_rng(7)
    cases, dead = [], []
    for nl, npt in PL.TOPOLOGIES:
        y, h, nvar = _case(rng, nl, npt, 300)
        h[nl - 1, :, 5] = 0  # an all-zero channel column: the last layer does not arrive
        d = [5]
        if nl == 2:
            h[1, :, 9] = h[0, :, 9]  # two equal columns
            d.append(9)
        cases.append((y, h, nvar, 1.0))
        dead.append(d)
    for bad in (0.0, -0.1, float("nan")):
        y, h, _ = _case(rng, 3, 4, 300)
        cases.append((y, h, bad, 1.0))
        dead.append(list(range(300)))
    out = _run(ctx, cases)[0]
    for (y, h, nvar, tx), (x, nv), d in zip(cases, out, dead):
        assert np.all(x[:, d] == 0) and np.all(np.isposinf(nv[:, d])), (h.shape, nvar)
        ex, ev = PL.zf_single(y, h, nvar, tx)
        assert np.array_equal(_bits(x), _bits(ex)) and np.array_equal(_bits(nv), _bits(ev))
        if len(d) < 300:
            assert np.all(np.isfinite(np.delete(nv, d, axis=1)))


@pytest.mark.parametrize("nl,npt,tx", [(2, 1, 1.0), (3, 2, 1.0), (0, 2, 1.0), (5, 4, 1.0), (1, 5, 1.0), (2, 2, 0.0)])
def test_rejections(ctx, nl, npt, tx):
    """Host jobs: MIPHY_EINVAL and nothing written (the good job in front of the bad one included); device jobs: the bad one skipped, its neighbour done."""
    import torch
    import miphy
    rng = np.random.default_rng(8)
    y, h, nvar = _case(rng, 2, 2, 100)
    n_bad = max(nl, 1) * 100
    good = PL.equalizer_job(miphy, 100, 2, 2, nvar, 1.0, 0, 0, 0, 0)
    bad = PL.equalizer_job(miphy, 100, npt, nl, nvar, tx, 0, 0, 200, 200)
    jobs = np.array([good, bad], dtype=miphy.EqualizerJob)
    big = torch.zeros(5 * 5 * 100, dtype=torch.complex64, device="cuda")
    y_d, h_d = big.clone(), big.clone()
    y_d[:200] = torch.from_numpy(y.reshape(-1)).cuda()
    h_d[:400] = torch.from_numpy(h.reshape(-1)).cuda()
    z_d = torch.full((200 + n_bad,), 9.0 + 0j, dtype=torch.complex64, device="cuda")
    v_d = torch.full((200 + n_bad,), 9.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):
        ctx.channel_equalize_layers_batch(jobs, y_d, h_d, z_d, v_d)
    torch.cuda.synchronize()
    assert torch.all(z_d == 9.0) and torch.all(v_d == 9.0)
    ctx.channel_equalize_layers_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), y_d, h_d, z_d, v_d)
    torch.cuda.synchronize()
    ex, ev = PL.zf_single(y, h, nvar, 1.0)
    assert np.array_equal(_bits(z_d[:200].cpu().numpy().reshape(2, 100)), _bits(ex))
    assert np.array_equal(_bits(v_d[:200].cpu().numpy().reshape(2, 100)), _bits(ev))
    assert torch.all(z_d[200:] == 9.0) and torch.all(v_d[200:] == 9.0)
