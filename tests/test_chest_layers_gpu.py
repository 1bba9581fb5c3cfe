"""GPU: miphy_dmrs_pusch_estimate_layers_batch against the float64 restatement of tests/pusch_layers_estimator_cases.py, with the tolerances of
tests/chest_batch.py (coefficients 1e-4 of the largest estimate, RSRP / EPRE / noise / SNR 1e-4 relative, time alignment 1.01 IDFT taps). The
grids carry that file's background noise, so no scalar compared is a difference of nearly equal numbers. Sentinels: estimate 1.0, scalars -77."""
import numpy as np
import pytest

import pusch_layers_estimator_cases as E
from chest_batch import SC_SENTINEL, SCATTERED, run as run_batch, select_ports

pytestmark = pytest.mark.gpu


def run(ctx, cases, sels=None, entry="dmrs_pusch_estimate_layers_batch", **kw):
    """chest_batch.run() for the layered entry point against the restatement."""
    return run_batch(ctx, cases, entry, E.estimate, sels, **kw)


TWO_PIECES = list(range(2, 10)) + list(range(14, 18))  # 12 PRBs: a pair must not reach across the gap, interpolation does


def test_small_and_split_allocations(ctx):
    """1 PRB (three pairs, both interpolation edges inside it), 2 PRBs, 12 PRBs in two pieces; 1, 2, 3 and 4 DM-RS symbols."""
    rng = np.random.default_rng(61)
    cases = [E.make_case(rng, 24, [7], 2, 2, [2, 11], delay=1.0)[0],
             E.make_case(rng, 24, [22, 23], 4, 4, [2, 7, 11], delay=3.0)[0],
             E.make_case(rng, 24, TWO_PIECES, 3, 3, [2, 5, 8, 11], delay=2.0)[0],
             E.make_case(rng, 24, TWO_PIECES, 2, 2, [3], delay=0.0)[0]]
    out = run(ctx, cases)
    nv = [float(sc[0, 0, 2] / sc[0, 0, 1]) for _, sc in out]  # below three DM-RS symbols the noise variance is forced to EPRE / 1000
    assert abs(nv[0] - 1e-3) < 1e-7 and abs(nv[3] - 1e-3) < 1e-7 and abs(nv[1] - 1e-3) > 1e-4 and abs(nv[2] - 1e-3) > 1e-4, nv


def test_every_topology(ctx):
    """L = 2, 3, 4 on P = L .. 4, one batch; three DM-RS symbols (the fitted noise rule) on every other job."""
    rng = np.random.default_rng(62)
    cases = [E.make_case(rng, 24, slice(3 + nl, 9 + nl + npt), npt, nl, [2, 7, 11] if k % 2 else [2, 11], delay=float(k % 4), slot=k, scr=100 + k)[0]
             for k, (nl, npt) in enumerate(E.PL.LAYERED)]
    run(ctx, cases)


def test_widest_grid(ctx):
    """Across the 64-PRB mask words of a 275-PRB grid, and the full 275 PRBs (1 650 pilots: the bound of the kernel's LDS arrays), compact."""
    rng = np.random.default_rng(63)
    cases = [E.make_case(rng, 275, SCATTERED, 2, 2, [2, 7, 11], numerology=3, slot=79, delay=1.0)[0],
             E.make_case(rng, 275, slice(0, 275), 4, 4, [2], delay=2.0)[0],
             E.make_case(rng, 275, [274], 3, 3, [2, 11], delay=0.0)[0]]
    run(ctx, cases, compact=True)


def test_partial_slot_compact_and_full(ctx):
    """first_symbol > 0: nothing in front of it is written; a DM-RS bit behind the allocation does not count. ce_compact: one row, bit for bit
    row first_symbol of the full estimate, the scalars the same."""
    rng = np.random.default_rng(64)
    cases = [E.make_case(rng, 24, TWO_PIECES, 2, 2, [3, 10], first=2, nof=10, delay=2.0)[0],
             E.make_case(rng, 25, slice(3, 20), 4, 3, [2, 7, 12], first=1, nof=11, delay=3.0)[0]]
    full = run(ctx, cases)
    comp = run(ctx, cases, compact=True)
    for i, (case, (fce, fsc), (cce, csc)) in enumerate(zip(cases, full, comp)):
        assert cce.shape[2] == 1 and cce[:, :, 0].tobytes() == np.ascontiguousarray(fce[:, :, case[8]]).tobytes(), i
        assert csc.tobytes() == fsc.tobytes(), i


def test_port_selection(ctx):
    """The job receives on the grid ports it names, in its order; the other ports of the grid are NaN."""
    rng = np.random.default_rng(65)
    cases, sels = [], []
    for nl, sel in ((2, [3, 1]), (2, [1, 3, 0]), (3, [3, 2, 0]), (4, [3, 2, 1, 0])):
        c, sl = select_ports(E.make_case(rng, 24, TWO_PIECES, 4, nl, [2, 7, 11], delay=1.0, scr=300 + nl)[0], sel)
        cases.append(c)
        sels.append(sl)
    run(ctx, cases, sels)


def test_numerologies(ctx):
    rng = np.random.default_rng(66)
    cases = [E.make_case(rng, 24, slice(5, 17), 2, 2, [2, 11], numerology=mu, slot=10 * (1 << mu) - 1, scr=65535, nscid=1, delay=float(3 - mu))[0] for mu in range(4)]
    out = run(ctx, cases)
    for mu, (_, sc) in enumerate(out):
        tap = 1.0 / (4096 * 15000.0 * (1 << mu))
        assert np.abs(sc[..., 4] - (3 - mu) * tap).max() <= 1.01 * tap, (mu, sc[..., 4])


def _mixed(rng):
    return [E.make_case(rng, 24, slice(2, 2 + 3 * nl), npt, nl, dsyms, delay=float(nl - 1), slot=nl)[0]
            for nl, npt, dsyms in ((1, 2, [2, 11]), (2, 2, [2, 7, 11]), (3, 4, [2]), (4, 4, [2, 7, 11]), (1, 1, [2, 7, 11]))]


def test_mixed_batch_and_one_layer_bytes(ctx):
    """L = 1, 2, 3 and 4 in one batch; the jobs on one layer give the bytes of miphy_dmrs_pusch_estimate_batch."""
    cases = _mixed(np.random.default_rng(67))
    out = run(ctx, cases, room_4x4=True)
    ones = [i for i, c in enumerate(cases) if c[10] == 1]
    ref = run(ctx, [cases[i] for i in ones], room_4x4=True, check=False, entry="dmrs_pusch_estimate_batch")
    for (rce, rsc), i in zip(ref, ones):
        assert out[i][0].tobytes() == rce.tobytes() and out[i][1].tobytes() == rsc.tobytes(), i


def test_device_resident_jobs(ctx):
    """Jobs in device memory, without and with the port / layer hint, write what host jobs write and nothing else."""
    cases = _mixed(np.random.default_rng(68))
    host = run(ctx, cases, room_4x4=True)
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, device=device, room_4x4=True, check=False)
        for i, ((hce, hsc), (dce, dsc)) in enumerate(zip(host, dev)):
            assert hce.tobytes() == dce.tobytes() and hsc.tobytes() == dsc.tobytes(), (device, i)


def test_hopping_is_refused(ctx):
    """A host job with hop_symbol != 0: MIPHY_EINVAL, nothing enqueued -- the jobs in front of it included."""
    cases = _mixed(np.random.default_rng(69))[:3]
    run(ctx, cases, hop=(2, 7))


def test_device_resident_jobs_that_break_a_rule(ctx):
    """Nobody checks device-resident jobs on the host: the kernels hold them to the rules of host jobs (chest_job_rule), skip a job that breaks one
    and still serve its neighbours. 1, 2 and 3 layers, sound and broken side by side; every breach is one that could not touch memory even if
    the check were lost. The broken jobs' records keep their sentinels, the sound jobs give the bytes of a host run of the sound jobs alone."""
    rng = np.random.default_rng(70)
    cases, sels = [], []
    for k, nl in enumerate((1, 2, 3, 1, 2, 3)):  # two ports each; three layers on two ports: two of the four ports of a case the builder can make
        case = E.make_case(rng, 24, slice(2 + k, 8 + 2 * k), 4 if nl == 3 else 2, nl, [2, 7, 11], delay=float(k % 3), slot=k, scr=40 + k)[0]
        case, sel = select_ports(case, [3, 1]) if nl == 3 else (case, None)
        cases.append(case)
        sels.append(sel)
    sound, broken = [0, 2, 4], {1: ("scaling", 0.0), 3: ("hop_symbol", 7), 5: ("symbols_mask", 0)}
    assert sorted(cases[i][10] for i in sound) == sorted(cases[i][10] for i in broken) == [1, 2, 3]

    def breach(jobs):
        for i, (field, value) in broken.items():
            jobs[i][field] = value

    host = run(ctx, [cases[i] for i in sound], [sels[i] for i in sound])
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, sels, device=device, check=False, edit=breach)
        for (hce, hsc), i in zip(host, sound):
            assert hce.tobytes() == dev[i][0].tobytes() and hsc.tobytes() == dev[i][1].tobytes(), (device, i)
        for i in broken:
            assert np.all(dev[i][0] == 1.0) and np.all(dev[i][1] == np.float32(SC_SENTINEL)), (device, i, "a skipped job writes nothing")
