"""GPU: miphy_transform_deprecode_batch, the de-precoder of a transform-precoded PUSCH (TS 38.211 6.3.1.4 read backwards) -- the IDFT of
M = 12 N_PRB points at every one of the 53 sizes (25 of them through the radix-5 pass), and the noise variance of the symbol -- against
numpy in float64 (tests/pusch_tp_ref.py).
Tolerances: symbols max |err| <= 4e-6 * rms(output), the bound tests/test_ofdm_gpu.py holds every DFT size to; the variance 2e-6 relative
(log2 M roundings of a tree sum of positive numbers and one division)."""
import numpy as np
import pytest

import pusch_tp_ref as R

pytestmark = pytest.mark.gpu
TOL = 4e-6
VTOL = 2e-6
SIZES = [12 * n for n in R.tp_sizes()]


def rel_err(a, b):
    return float(np.abs(a - b).max() / np.sqrt(np.mean(np.abs(b) ** 2)))


def _run(ctx, Ms, x, v, rows=3, device_jobs=False, ex_pad=5):
    """One job of `rows` rows per entry of Ms, inputs back to back, outputs with `ex_pad` sentinels behind every job. Returns (y per job, v per job,
    the whole output arrays)."""
    import torch
    import miphy
    jobs = np.zeros(len(Ms), dtype=miphy.TransformDeprecodeJob)
    ioff = yoff = voff = 0
    where = []
    for i, M in enumerate(Ms):
        jobs[i] = (M, rows, ioff, ioff, yoff, voff)
        where.append((yoff, voff))
        ioff += rows * M
        yoff += rows * M + ex_pad
        voff += rows + ex_pad
    y_d = torch.full((yoff,), 77 + 77j, dtype=torch.complex64, device="cuda")
    v_d = torch.full((voff,), -77.0, dtype=torch.float32, device="cuda")
    j = torch.from_numpy(jobs.view(np.uint8)).cuda() if device_jobs else jobs
    ctx.transform_deprecode_batch(j, torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), y_d, v_d)
    torch.cuda.synchronize()
    y, vv = y_d.cpu().numpy(), v_d.cpu().numpy()
    ys, vs = [], []
    for (yo, vo), M in zip(where, Ms):
        ys.append(y[yo:yo + rows * M].reshape(rows, M))
        vs.append(vv[vo:vo + rows])
        assert np.all(y[yo + rows * M:yo + rows * M + ex_pad] == 77 + 77j) and np.all(vv[vo + rows:vo + rows + ex_pad] == -77.0), M  # nothing behind the job
    return ys, vs, y, vv


@pytest.mark.parametrize("device_jobs", [False, True])
def test_all_53_sizes_against_numpy(ctx, device_jobs):
    """Every size in one call, three distinct rows each: the symbols within TOL of numpy's float64 IFFT of the same single-precision inputs,
    the variance within VTOL of the float64 mean. The worst distance per size is printed."""
    rng = np.random.default_rng(53)
    n = 3 * sum(SIZES)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    v = rng.uniform(0.01, 2.0, n).astype(np.float32)
    ys, vs, _, _ = _run(ctx, SIZES, x, v, device_jobs=device_jobs)
    off, worst, worst_v = 0, {}, 0.0
    for M, y, vb in zip(SIZES, ys, vs):
        for r in range(3):
            ey, ev = R.deprecode(x[off:off + M], v[off:off + M])
            worst[M] = max(worst.get(M, 0.0), rel_err(y[r], ey))
            worst_v = max(worst_v, abs(float(vb[r]) - ev) / ev)
            off += M
    for M in SIZES:
        print("M = %4d (%3d PRB%s): worst |err| / rms = %.3g" % (M, M // 12, ", radix 5" if M % 5 == 0 else "", worst[M]))
    print("worst over the 53 sizes: %.3g; worst relative distance of the variance: %.3g" % (max(worst.values()), worst_v))
    bad = {M: e for M, e in worst.items() if not e < TOL}
    assert not bad, bad
    assert worst_v <= VTOL, worst_v


def test_abnormal_elements(ctx):
    """An element whose variance is not positive and finite (the equalisers write symbol 0 and +inf; here the symbol is left non-zero on purpose)
    enters the transform as 0 and is left out of the mean: rows with one, several and all elements abnormal, at a power of two times three, a
    size with a factor 5 and the largest."""
    rng = np.random.default_rng(7)
    Ms = [48, 60, 3240]
    x = np.concatenate([(rng.standard_normal(3 * M) + 1j * rng.standard_normal(3 * M)).astype(np.complex64) for M in Ms])
    v = rng.uniform(0.01, 2.0, x.size).astype(np.float32)
    off = 0
    for M in Ms:
        v[off + M // 2] = np.inf                                      # row 0: one
        sel = off + M + rng.choice(M, M // 3, replace=False)          # row 1: several, of every kind
        v[sel] = np.resize(np.array([np.inf, np.nan, 0.0, -1.0, -np.inf], np.float32), sel.size)
        v[off + 2 * M:off + 3 * M] = np.inf                           # row 2: all
        off += 3 * M
    ys, vs, _, _ = _run(ctx, Ms, x, v)
    off = 0
    for M, y, vb in zip(Ms, ys, vs):
        for r in range(3):
            ey, ev = R.deprecode(x[off:off + M], v[off:off + M])
            if r < 2:
                assert rel_err(y[r], ey) < TOL and abs(float(vb[r]) - ev) <= VTOL * ev, (M, r)
            else:
                assert not y[r].any() and vb[r] == np.inf, (M, r)
            off += M


def test_rows_do_not_depend_on_the_batch(ctx):
    """The additions run in one order whatever the launch: a row alone and the same row among the 53 sizes give the same bits."""
    rng = np.random.default_rng(9)
    M = 3000
    x = (rng.standard_normal(3 * M) + 1j * rng.standard_normal(3 * M)).astype(np.complex64)
    v = rng.uniform(0.01, 2.0, 3 * M).astype(np.float32)
    y1, v1, _, _ = _run(ctx, [M], x, v)
    pre = 3 * 12
    xm = np.concatenate([np.ones(pre, np.complex64), x, np.ones(3 * 96, np.complex64)])
    vm = np.concatenate([np.ones(pre, np.float32), v, np.ones(3 * 96, np.float32)])
    ym, vmo, _, _ = _run(ctx, [12, M, 96], xm, vm, device_jobs=True)
    assert np.array_equal(y1[0].view(np.uint32), ym[1].view(np.uint32)) and np.array_equal(v1[0].view(np.uint32), vmo[1].view(np.uint32))


@pytest.mark.parametrize("M", [0, 7 * 12, 11 * 12, 36 + 1, 271 * 12, 4096])
def test_unsupported_size_is_refused_and_skipped(ctx, M):
    """A host job with a size outside the 53 is MIPHY_EUNSUPP by message with nothing written, the good job in front of it included; a
    device-resident one is skipped and its neighbour served."""
    import torch
    import miphy
    jobs = np.zeros(2, dtype=miphy.TransformDeprecodeJob)
    jobs[0] = (24, 1, 0, 0, 0, 0)
    jobs[1] = (M, 1, 24, 24, 24, 1)
    x = torch.ones(24 + 4200, dtype=torch.complex64, device="cuda")
    v = torch.ones(24 + 4200, dtype=torch.float32, device="cuda")
    y = torch.full((24 + 4200,), 77 + 77j, dtype=torch.complex64, device="cuda")
    vo = torch.full((4,), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="not supported"):
        ctx.transform_deprecode_batch(jobs, x, v, y, vo)
    torch.cuda.synchronize()
    assert bool((y == 77 + 77j).all()) and bool((vo == -77.0).all())
    ctx.transform_deprecode_batch(torch.from_numpy(jobs.view(np.uint8)).cuda(), x, v, y, vo)
    torch.cuda.synchronize()
    yh, vh = y.cpu().numpy(), vo.cpu().numpy()
    assert abs(yh[0] - np.sqrt(24)) < 1e-5 and np.abs(yh[1:24]).max() < 1e-5 and vh[0] == 1.0  # the IDFT of a constant
    assert np.all(yh[24:] == 77 + 77j) and np.all(vh[1:] == -77.0)


def test_dft_batch_still_refuses_a_factor_five(ctx):
    """The radix-5 pass serves the de-precoder only: miphy_dft_batch keeps its sizes."""
    import torch
    x = torch.zeros(60, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match="not supported"):
        ctx.dft_batch(60, 1, 1, x, torch.zeros_like(x))
