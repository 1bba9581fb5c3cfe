"""GPU: miphy_channel_equalize_mmse_batch (MMSE-IRC, 1..4 layers on 1..4 ports) against the numpy float32 restatement of its arithmetic
(tests/pusch_mmse_cases.py mmse_single, held to numpy.linalg in float64 in tests/test_pusch_mmse.py): bit for bit. The upper triangle and
the imaginary parts of the diagonal of every covariance matrix on the device are NaN: only the lower triangle may be read."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_mmse_cases as MM

pytestmark = pytest.mark.gpu
GUARD = 7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _poisoned(cov):
    """[matrices][P][P] complex64 with everything the kernel must not read turned into NaN."""
    c = np.array(cov, np.complex64)
    p = c.shape[-1]
    up = np.triu(np.ones((p, p), bool), 1)
    c[:, up] = np.nan + 1j * np.nan
    d = np.arange(p)
    c.imag[:, d, d] = np.nan  # (the real parts stay)
    assert np.array_equal(c.real[:, d, d], np.asarray(cov).real[:, d, d], equal_nan=True)
    return c


def _run(ctx, cases, device_jobs=False):
    """cases: list of (y [P][n], h [L][P][n], cov [matrices][P][P], tx, re_per_cov). One batch; GUARD sentinel elements between the outputs of
    the jobs. Returns [(x [L][n], nv [L][n])] and the two raw output arrays."""
    import torch
    import miphy
    jobs, ys, hs, cs, spans = [], [], [], [], []
    yo = ho = co = zo = 0
    for y, h, cov, tx, per in cases:
        nl, npt, n = h.shape
        cov = _poisoned(np.asarray(cov).reshape(-1, npt, npt))
        assert cov.shape[0] >= (-(-n // per) if per else 1)
        zo += GUARD
        jobs.append(MM.equalizer_mmse_job(miphy, n, npt, nl, tx, per, yo, ho, co, zo, zo))
        spans.append((zo, nl, n))
        ys.append(y.reshape(-1))
        hs.append(h.reshape(-1))
        cs.append(cov.reshape(-1))
        yo += y.size
        ho += h.size
        co += cov.size
        zo += nl * n
    zo += GUARD
    jobs = np.array(jobs, dtype=miphy.EqualizerMmseJob)
    if device_jobs:
        jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    y_d = torch.from_numpy(np.concatenate(ys)).cuda()
    h_d = torch.from_numpy(np.concatenate(hs)).cuda()
    c_d = torch.from_numpy(np.concatenate(cs)).cuda()
    z_d = torch.full((zo,), 77.0 + 5.0j, dtype=torch.complex64, device="cuda")
    v_d = torch.full((zo,), -3.0, dtype=torch.float32, device="cuda")
    ctx.channel_equalize_mmse_batch(jobs, y_d, h_d, c_d, z_d, v_d)
    torch.cuda.synchronize()
    z, v = z_d.cpu().numpy(), v_d.cpu().numpy()
    keep = np.ones(z.size, bool)
    for o, nl, n in spans:
        keep[o:o + nl * n] = False
    assert np.all(z[keep] == np.complex64(77.0 + 5.0j)) and np.all(v[keep] == -3.0), "written outside the jobs' records"
    return [(z[o:o + nl * n].reshape(nl, n), v[o:o + nl * n].reshape(nl, n)) for o, nl, n in spans]


def _covs(rng, npt, count):
    """`count` matrices: white noise 0.03 plus one (even) or two (odd) interferers up to 20 dB above it."""
    return np.stack([MM.coloured(rng, npt, 0.03, rng.uniform(0, 100, 1 + k % 2)) for k in range(count)]).astype(np.complex64)


def _case(rng, nl, npt, n, tx, per):
    h, _ = PL.channels(rng, nl, npt, n)
    y = (rng.standard_normal((npt, n)) + 1j * rng.standard_normal((npt, n))).astype(np.complex64)
    return y, h, _covs(rng, npt, -(-n // per) if per else 1), tx, per


def _assert_restated(cases, out):
    for (y, h, cov, tx, per), (x, nv) in zip(cases, out):
        ex, ev = MM.mmse_single(y, h, cov, tx, per)
        assert np.array_equal(_bits(x), _bits(ex)), (h.shape, tx, per)
        assert np.array_equal(_bits(nv), _bits(ev)), (h.shape, tx, per)


@pytest.mark.parametrize("device_jobs", [False, True])
def test_all_topologies_bit_equal_to_the_restatement(ctx, device_jobs):
    """1 000 elements (no multiple of the 256-thread tile, of 96 or of 144: the last matrix serves a short run) and 1 300 (two blocks) per
    topology, tx_scaling 1 and 0.6, one matrix for all elements and one per 96 / 144, one batch, guards between."""
    rng = np.random.default_rng(15)
    cases = []
    for k, (nl, npt) in enumerate(PL.TOPOLOGIES):
        pers = (0, 96, 144)
        for m, (n, tx) in enumerate(((1000, 1.0), (1300, 0.6), (1000, 0.6), (1300, 1.0))):  # both lengths at both scalings
            cases.append(_case(rng, nl, npt, n, tx, pers[(k + m) % 3]))
    assert {(c[1].shape[0], c[1].shape[1], c[4]) for c in cases} >= {(nl, npt, per) for nl, npt in PL.TOPOLOGIES for per in (0, 96, 144)}
    out = _run(ctx, cases, device_jobs)
    _assert_restated(cases, out)
    assert all(np.all(np.isfinite(nv)) for _, nv in out)


def test_abnormal_elements_give_zero_and_infinity_on_every_layer(ctx):
    """An all-zero channel column (gamma = 0), a singular covariance matrix (rank one, nothing loaded: a pivot is exactly 0) and one with a NaN,
    each for the 100 elements it serves: symbol 0 and +inf on every layer there, finite elsewhere, the restatement's bits everywhere."""
    rng = np.random.default_rng(17)
    sig = np.array([1, 1j, -1, -1j]) * 0.5  # unit-modulus signature: every product of the factorisation is exact
    cases, dead = [], []
    for nl, npt in PL.TOPOLOGIES:
        y, h, cov, tx, per = _case(rng, nl, npt, 300, 1.0, 100)
        h[nl - 1, :, 5] = 0  # the last layer does not arrive
        cov[1] = np.outer(sig[:npt], sig[:npt].conj()) if npt > 1 else 0.0
        cases.append((y, h, cov, tx, per))
        dead.append([5] + list(range(100, 200)))
        y, h, cov, tx, per = _case(rng, nl, npt, 300, 0.6, 100)
        cov[2, npt - 1, 0] = np.nan
        cases.append((y, h, cov, tx, per))
        dead.append(list(range(200, 300)))
    out = _run(ctx, cases)
    _assert_restated(cases, out)
    for (y, h, cov, tx, per), (x, nv), d in zip(cases, out, dead):
        assert np.all(x[:, d] == 0) and np.all(np.isposinf(nv[:, d])), h.shape
        assert np.all(np.isfinite(np.delete(nv, d, axis=1))) and np.all(np.delete(nv, d, axis=1) > 0), h.shape


@pytest.mark.parametrize("nl,npt,tx", [(2, 1, 1.0), (3, 2, 1.0), (0, 2, 1.0), (5, 4, 1.0), (1, 5, 1.0), (2, 2, 0.0)])
def test_rejections(ctx, nl, npt, tx):
    """Host jobs: MIPHY_EINVAL and nothing written (the good job in front of the bad one included); device jobs: the bad one skipped, its neighbour done."""
    import torch
    import miphy
    rng = np.random.default_rng(18)
    y, h, cov, _, _ = _case(rng, 2, 2, 100, 1.0, 0)
    n_bad = max(nl, 1) * 100
    good = MM.equalizer_mmse_job(miphy, 100, 2, 2, 1.0, 0, 0, 0, 0, 0, 0)
    bad = MM.equalizer_mmse_job(miphy, 100, npt, nl, tx, 0, 0, 0, 0, 200, 200)
    jobs = np.array([good, bad], dtype=miphy.EqualizerMmseJob)
    big = torch.zeros(5 * 5 * 100, dtype=torch.complex64, device="cuda")
    y_d, h_d = big.clone(), big.clone()
    y_d[:200] = torch.from_numpy(y.reshape(-1)).cuda()
    h_d[:400] = torch.from_numpy(h.reshape(-1)).cuda()
    c_d = torch.zeros(25, dtype=torch.complex64, device="cuda")
    c_d[:4] = torch.from_numpy(cov.reshape(-1)).cuda()
    z_d = torch.full((200 + n_bad,), 9.0 + 0j, dtype=torch.complex64, device="cuda")
    v_d = torch.full((200 + n_bad,), 9.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="miphy error -1"):
        ctx.channel_equalize_mmse_batch(jobs, y_d, h_d, c_d, z_d, v_d)
    torch.cuda.synchronize()
    assert torch.all(z_d == 9.0) and torch.all(v_d == 9.0)
    ctx.channel_equalize_mmse_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), y_d, h_d, c_d, z_d, v_d)
    torch.cuda.synchronize()
    ex, ev = MM.mmse_single(y, h, cov, 1.0)
    assert np.array_equal(_bits(z_d[:200].cpu().numpy().reshape(2, 100)), _bits(ex))
    assert np.array_equal(_bits(v_d[:200].cpu().numpy().reshape(2, 100)), _bits(ev))
    assert torch.all(z_d[200:] == 9.0) and torch.all(v_d[200:] == 9.0)
