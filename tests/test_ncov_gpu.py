"""GPU: miphy_pusch_noise_covariance_batch against the float64 restatement (tests/pusch_mmse_cases.py covariance): every element within
1e-4 sqrt(C_pp C_qq) -- the tolerance the estimator's noise scalar is held to (tests/chest_batch.py) -- exact Hermitian symmetry, a real
diagonal, the same bits alone and inside a batch, and the estimator's own noise_var on the diagonal. 24-PRB grids with that file's background
noise plus a rank-one interferer, so the off-diagonal entries are no differences of nearly equal numbers. Sentinel: 77 + 5j."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import pusch_mmse_cases as MM
from chest_batch import run as run_chest

pytestmark = pytest.mark.gpu
GUARD = 5
SENTINEL = np.complex64(77.0 + 5.0j)
ALLOCATIONS = {"five": [6, 7, 8, 9, 10], "split": [3, 4, 9, 10, 11, 17, 23]}  # 5 PRBs: the last PRG is short at 2 and 4; pieces of 2, 3, 1 and 1
DMRS = ([2], [2, 11], [2, 7, 11])
PRGS = (0, 1, 2, 4)


def _interfered(rng, case, amp=0.1):
    """The estimator case with a rank-one interferer on every element of its grid."""
    g = case[-1].astype(np.complex128)
    a = (rng.standard_normal(g.shape[0]) + 1j * rng.standard_normal(g.shape[0])) / np.sqrt(2)
    q = ((1 - 2.0 * rng.integers(0, 2, g.shape[1:])) + 1j * (1 - 2.0 * rng.integers(0, 2, g.shape[1:]))) / np.sqrt(2)
    return case[:-1] + ((g + amp * a[:, None, None] * q[None]).astype(np.complex64),)


def _cases(seed, alloc, dsyms):
    rng = np.random.default_rng(seed)
    return [_interfered(rng, E.make_case(rng, 24, ALLOCATIONS[alloc], npt, nl, dsyms, delay=float(k % 3), slot=k, scr=200 + k)[0])
            for k, (nl, npt) in enumerate(PL.TOPOLOGIES)]


def _run(ctx, items, device=None, edit=None, expect_refusal=False):
    """items: list of (case, prg_size, loading); the grid of a case travels once. One batch; GUARD sentinels around every job's matrices.
    Returns per job the matrices [PRG][P][P] as the device wrote them (None for a job whose record kept its sentinels)."""
    import torch
    import miphy
    grids, g_off_of, g_off = [], {}, 0
    jobs, spans, c_off = [], [], GUARD
    for case, prg, loading in items:
        if id(case) not in g_off_of:
            g_off_of[id(case)] = g_off
            grids.append(case[-1].reshape(-1))
            g_off += case[-1].size
        npt = case[-1].shape[0]
        nprg = MM.nof_prg(int(case[7].sum()), prg)
        jobs.append(MM.ncov_job(miphy, case, prg, loading, g_off_of[id(case)], c_off))
        spans.append((c_off, nprg, npt))
        c_off += nprg * npt * npt + GUARD
    jobs = np.array(jobs, dtype=miphy.PuschNcovJob)
    if edit is not None:
        edit(jobs)
    g_d = torch.from_numpy(np.concatenate(grids)).cuda()
    c_d = torch.full((c_off,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    if expect_refusal:
        with pytest.raises(RuntimeError, match="miphy error -1"):
            ctx.pusch_noise_covariance_batch(jobs, g_d, c_d)
        torch.cuda.synchronize()
        assert bool((c_d == complex(SENTINEL)).all()), "a refused batch writes nothing"
        return None
    if device is None:
        ctx.pusch_noise_covariance_batch(jobs, g_d, c_d)
    else:
        hint = dict(max_ports=int(jobs["base"]["nof_rx_ports"].max()), max_layers=int(jobs["base"]["nof_tx_layers"].max())) if device == "hint" else {}
        ctx.pusch_noise_covariance_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), g_d, c_d, **hint)
    torch.cuda.synchronize()
    c = c_d.cpu().numpy()
    keep = np.ones(c.size, bool)
    out = []
    for o, nprg, npt in spans:
        keep[o:o + nprg * npt * npt] = False
        m = c[o:o + nprg * npt * npt].reshape(nprg, npt, npt)
        out.append(None if np.all(m == SENTINEL) else m)
    assert np.all(c[keep] == SENTINEL), "written outside the jobs' records"
    return out


def _assert_matrices(got, case, prg, loading):
    exp = MM.covariance(case, prg, loading)
    assert got is not None and got.shape == exp.shape
    d = np.sqrt(np.real(np.einsum("jpp->jp", exp)))
    err = np.abs(got - exp) / (d[:, :, None] * d[:, None, :])
    assert err.max() <= 1e-4, (case[10], got.shape, prg, err.max())
    assert np.array_equal(got, got.conj().transpose(0, 2, 1))
    assert np.all(np.einsum("jpp->jp", got).imag == 0) and np.all(np.einsum("jpp->jp", got).real > 0)


@pytest.mark.parametrize("dsyms", DMRS, ids=lambda d: "dmrs" + "_".join(map(str, d)))
@pytest.mark.parametrize("alloc", list(ALLOCATIONS))
def test_every_topology_and_prg_size(ctx, alloc, dsyms):
    """All ten topologies x prg_size 0, 1, 2, 4 as one batch of host jobs and one of device-resident jobs (without and with the hint): the same bits."""
    cases = _cases(70 + len(dsyms), alloc, dsyms)
    items = [(case, prg, 0.05 * (k % 2)) for k, case in enumerate(cases) for prg in PRGS]
    host = _run(ctx, items)
    for got, (case, prg, loading) in zip(host, items):
        _assert_matrices(got, case, prg, loading)
    for device in ("nohint", "hint"):
        dev = _run(ctx, items, device=device)
        assert all(d is not None and d.tobytes() == h.tobytes() for d, h in zip(dev, host)), device


def test_same_bits_alone_and_in_a_batch(ctx):
    cases = _cases(80, "split", [2, 7, 11])
    items = [(cases[k], prg, 0.0) for k, prg in ((9, 2), (0, 0), (4, 1), (6, 4), (2, 0), (8, 1), (5, 2))]
    batch = _run(ctx, items)
    for k in (0, 3, 6):
        alone = _run(ctx, [items[k]])[0]
        assert alone.tobytes() == batch[k].tobytes(), k
    again = _run(ctx, items)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, batch)), "run to run"


def test_widest_grid(ctx):
    """275 PRBs on four ports and four layers: one matrix from 825 pilot pairs (fourteen passes of a wavefront), and one per PRB (275 PRGs,
    35 workgroups per job); an allocation in every 64-bit word of rb_mask."""
    from chest_batch import SCATTERED
    rng = np.random.default_rng(81)
    full = _interfered(rng, E.make_case(rng, 275, slice(0, 275), 4, 4, [2, 11])[0])
    scat = _interfered(rng, E.make_case(rng, 275, SCATTERED, 3, 2, [2, 7, 11], numerology=3, slot=79)[0])
    items = [(full, 0, 0.0), (full, 1, 0.0), (scat, 4, 0.1), (full, 64, 0.0)]
    for got, (case, prg, loading) in zip(_run(ctx, items), items):
        _assert_matrices(got, case, prg, loading)


def test_diagonal_is_the_estimators_noise_variance(ctx):
    """Three DM-RS symbols, one and two layers, no interferer: the whole-allocation diagonal against the noise_var that
    miphy_dmrs_pusch_estimate_layers_batch writes for that port (one group: the divisor is the same), 1e-4 relative."""
    rng = np.random.default_rng(82)
    cases = [E.make_case(rng, 24, ALLOCATIONS[a], npt, nl, [2, 7, 11], delay=1.0, scr=300 + nl)[0]
             for a in ALLOCATIONS for nl, npt in PL.TOPOLOGIES if nl <= 2]
    est = run_chest(ctx, cases, "dmrs_pusch_estimate_layers_batch", E.estimate, check=False)
    cov = _run(ctx, [(case, 0, 0.0) for case in cases])
    for case, (_, sc), c in zip(cases, est, cov):
        for p in range(c.shape[1]):
            for ly in range(case[10]):
                assert abs(c[0, p, p].real - sc[p, ly, 2]) <= 1e-4 * sc[p, ly, 2], (case[10], p, ly, c[0, p, p], sc[p, ly, 2])


BREACHES = [("loading", -1.0), ("loading", float("nan")), ("hop_symbol", 7)]


@pytest.mark.parametrize("field,value", BREACHES, ids=["negative_loading", "nan_loading", "hopping"])
def test_rejections(ctx, field, value):
    """Host jobs: MIPHY_EINVAL and nothing written, the good jobs around the bad one included. Device-resident jobs: the bad one is skipped,
    its neighbours give the bytes of a host run without it."""
    cases = _cases(83, "five", [2, 7, 11])
    items = [(cases[4], 2, 0.0), (cases[7], 1, 0.0), (cases[1], 0, 0.1)]

    def breach(jobs):
        (jobs if field == "loading" else jobs["base"])[field][1] = value
        if field == "hop_symbol":
            jobs["base"]["rb_mask2"][1] = jobs["base"]["rb_mask"][1]

    _run(ctx, items, edit=breach, expect_refusal=True)
    sound = _run(ctx, [items[0], items[2]])
    for device in ("nohint", "hint"):
        dev = _run(ctx, items, device=device, edit=breach)
        assert dev[1] is None, "a skipped job writes nothing"
        assert dev[0].tobytes() == sound[0].tobytes() and dev[2].tobytes() == sound[1].tobytes(), device
