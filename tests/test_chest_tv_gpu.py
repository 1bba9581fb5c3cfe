"""GPU: miphy_dmrs_pusch_estimate_tv_batch against the float64 restatement of tests/pusch_tv_cases.py. Tolerances: those of
tests/test_chest_cfo_gpu.py (coefficients 1e-4 of the largest estimate, RSRP / EPRE / noise / SNR 1e-4 relative, time alignment 1.01 IDFT taps, the
offset as the phase it turns the longest DM-RS gap by, 2 pi |cfo_hz - expected| max dt <= 1e-4 rad, rho 1e-4 relative) and the variation 1e-4
relative. The grids carry the background noise of tests/pusch_layers_estimator_cases.py under two_ray_gains(fd) and an offset; |f| max dt <= 0.15
cycles and fd <= 300 Hz keep the correlation away from the wrap at half a cycle. Sentinels: estimate 1.0, scalars -77, {cfo_hz, rho} -55, var -33."""
import numpy as np
import pytest

import pusch_cfo_cases as F
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import pusch_tv_cases as T

pytestmark = pytest.mark.gpu

CE_GUARD, SC_GUARD, CFO_GUARD, VAR_GUARD, SC_SENTINEL, CFO_SENTINEL, VAR_SENTINEL = 5, 3, 1, 2, -77.0, -55.0, -33.0
TWO_PIECES = list(range(2, 10)) + list(range(14, 18))  # 12 PRBs: a pair must not reach across the gap, interpolation does
_expected = {}


def tv_case(mode, f_hz, fd, *args, **kw):
    """(mode, E.make_case() under two_ray_gains(fd) and the offset f_hz)."""
    case = E.make_case(*args, **kw)[0]
    assert abs(f_hz) * F.max_gap(case) <= 0.15 and fd <= 300.0, (f_hz, fd, F.max_gap(case))
    g = T.apply_gains(case[-1], T.two_ray_gains(fd, case[0], case[1], case[-1].shape[0]))
    return mode, case[:-1] + (F.apply_cfo(g, case[0], case[1], f_hz),)


def expected(mc):
    if id(mc) not in _expected:  # (the entry keeps the case object alive: its id is not reused)
        _expected[id(mc)] = (mc, T.estimate(mc[0], *mc[1]))
    return _expected[id(mc)][1]


def run(ctx, cases, device=None, check=True, edit=None, refused=False):
    """The cases as one batch. device: None (host jobs), "nohint" or "hint". edit: called with the job records before they are sent. refused: the
    call must fail with MIPHY_EINVAL and write nothing. Returns per job (estimate [nl][ports][rows][nsc], scalars [ports][nl][5], {cfo_hz, rho},
    var [ports][nl]) as the device wrote them; everything outside the records must keep its sentinel."""
    import torch
    import miphy
    jobs = np.zeros(len(cases), dtype=miphy.PuschChestTvJob)
    grids, g_off, ce_off, sc_off, cfo_off, var_off, shapes = [], 0, CE_GUARD, SC_GUARD, CFO_GUARD, VAR_GUARD, []
    for i, (mode, (mu, slot, t2, scr, nscid, scaling, sm, rb, first, nof, nl, g)) in enumerate(cases):
        j = jobs[i]["base"]["base"]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = mu, slot, scr, scaling
        j["n_scid"], j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"] = nscid, nl, g.shape[0], first, nof
        j["rx_ports"] = [0, 1, 2, 3]
        j["symbols_mask"] = sum(int(b) << l for l, b in enumerate(sm))
        j["grid_nof_prb"] = rb.size
        j["rb_mask"] = PL.mask_words(rb)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = g_off, ce_off, sc_off
        jobs[i]["base"]["cfo_offset"], jobs[i]["var_offset"], jobs[i]["time_mode"] = cfo_off, var_off, mode
        grids.append(g.reshape(-1))
        g_off += g.size
        shapes.append((nl, g.shape[0], first + nof, g.shape[2]))
        ce_off += int(np.prod(shapes[-1])) + CE_GUARD
        sc_off += g.shape[0] * nl * 5 + SC_GUARD
        cfo_off += 2 + CFO_GUARD
        var_off += g.shape[0] * nl + VAR_GUARD
    if edit is not None:
        edit(jobs)
    g_d = torch.from_numpy(np.concatenate(grids).astype(np.complex64)).cuda()
    ce_d = torch.ones(ce_off, dtype=torch.complex64, device="cuda")
    sc_d = torch.full((sc_off,), SC_SENTINEL, dtype=torch.float32, device="cuda")
    cfo_d = torch.full((cfo_off,), CFO_SENTINEL, dtype=torch.float32, device="cuda")
    var_d = torch.full((var_off,), VAR_SENTINEL, dtype=torch.float32, device="cuda")
    if refused:
        with pytest.raises(RuntimeError, match="miphy error -1: miphy_dmrs_pusch_estimate_tv_batch: job 1:"):  # (the prefix names the entry point)
            ctx.dmrs_pusch_estimate_tv_batch(jobs, g_d, ce_d, sc_d, cfo_d, var_d)
        torch.cuda.synchronize()
        assert bool((ce_d == 1.0).all()) and bool((sc_d == SC_SENTINEL).all()) and bool((cfo_d == CFO_SENTINEL).all()) and bool((var_d == VAR_SENTINEL).all()), \
            "a refused batch writes nothing"
        return None
    if device is None:
        ctx.dmrs_pusch_estimate_tv_batch(jobs, g_d, ce_d, sc_d, cfo_d, var_d)
    else:
        b = jobs["base"]["base"]
        hint = dict(max_ports=int(b["nof_rx_ports"].max()), max_layers=min(4, int(b["nof_tx_layers"].max()))) if device == "hint" else {}
        ctx.dmrs_pusch_estimate_tv_batch(torch.from_numpy(jobs.view(np.uint8)).cuda(), g_d, ce_d, sc_d, cfo_d, var_d, **hint)
    torch.cuda.synchronize()
    ce, sc, cfo, var = ce_d.cpu().numpy(), sc_d.cpu().numpy(), cfo_d.cpu().numpy(), var_d.cpu().numpy()
    used_ce, used_sc, used_cfo, used_var = np.zeros(ce.size, bool), np.zeros(sc.size, bool), np.zeros(cfo.size, bool), np.zeros(var.size, bool)
    out = []
    for i, shp in enumerate(shapes):
        c0, s0 = int(jobs[i]["base"]["base"]["ce_offset"]), int(jobs[i]["base"]["base"]["scalars_offset"])
        f0, v0 = int(jobs[i]["base"]["cfo_offset"]), int(jobs[i]["var_offset"])
        n_ce, n_pl = int(np.prod(shp)), shp[0] * shp[1]
        used_ce[c0:c0 + n_ce] = used_sc[s0:s0 + 5 * n_pl] = used_cfo[f0:f0 + 2] = used_var[v0:v0 + n_pl] = True
        out.append((ce[c0:c0 + n_ce].reshape(shp), sc[s0:s0 + 5 * n_pl].reshape(shp[1], shp[0], 5), cfo[f0:f0 + 2], var[v0:v0 + n_pl].reshape(shp[1], shp[0])))
    assert np.all(ce[~used_ce] == 1.0) and np.all(sc[~used_sc] == np.float32(SC_SENTINEL)) and np.all(cfo[~used_cfo] == np.float32(CFO_SENTINEL)) \
        and np.all(var[~used_var] == np.float32(VAR_SENTINEL)), "written outside the jobs' records"
    if not check:
        return out
    for i, mc in enumerate(cases):
        a = mc[1]
        mu, rb, first = a[0], a[7], a[8]
        exp_ce, exp_sc, exp_f, exp_rho, exp_var = expected(mc)
        got_ce, got_sc, got_cfo, got_var = out[i]
        mask = np.repeat(rb.astype(bool), 12)
        assert np.all(got_ce[:, :, :first] == 1.0), "rows in front of the allocation are left untouched"
        assert np.all(got_ce[..., ~mask] == 1.0), "unallocated PRBs are left untouched"
        got_ce, exp_ce = got_ce[:, :, first:], exp_ce[:, :, first:]
        err = np.abs(got_ce[..., mask] - exp_ce[..., mask]).max() / np.abs(exp_ce[..., mask]).max()
        turn = 2 * np.pi * abs(float(got_cfo[0]) - exp_f) * F.max_gap(a)
        rho_err = abs(float(got_cfo[1]) - exp_rho) / exp_rho if exp_rho else abs(float(got_cfo[1]))
        var_err = (np.abs(got_var - exp_var) / (np.abs(exp_var) + 1e-30)).max()
        print("job %d mode %d: estimate error %.3g of the largest estimate; cfo_hz %.4f (expected %.4f: %.3g rad over the longest gap); rho %.6f (relative error "
              "%.3g); var %.4g .. %.4g (relative error %.3g)" % (i, mc[0], err, got_cfo[0], exp_f, turn, got_cfo[1], rho_err, exp_var.min(), exp_var.max(), var_err))
        assert err < 1e-4, (i, err)
        assert turn <= 1e-4, (i, got_cfo[0], exp_f)
        assert rho_err <= 1e-4, (i, got_cfo[1], exp_rho)
        assert var_err <= 1e-4, (i, got_var, exp_var)
        for k in range(4):
            rel = np.abs(got_sc[..., k] - exp_sc[..., k]) / (np.abs(exp_sc[..., k]) + 1e-30)
            print("job %d: scalar %d relative error %.3g" % (i, k, rel.max()))
            assert rel.max() < 1e-4, (i, k, got_sc[..., k], exp_sc[..., k])
        tap = 1.0 / (4096 * 15000.0 * (1 << mu))
        assert np.abs(got_sc[..., 4] - exp_sc[..., 4]).max() <= 1.01 * tap, (i, got_sc[..., 4], exp_sc[..., 4])
    return out


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


DMRS_SETS = ([3], [2, 11], [2, 7, 11], [2, 5, 8, 11])


@pytest.mark.parametrize("mode", T.MODES, ids=("interpolate", "line"))
def test_allocations_and_dmrs_sets(ctx, mode):
    """12 PRBs, 12 PRBs in two pieces and one PRB (three pairs, edges held), each with one, two, three and four DM-RS symbols. One DM-RS symbol gives
    {0, 0} and var = 0."""
    rng = np.random.default_rng(91)
    cases = [tv_case(mode, (400.0, -400.0, 150.0)[(a + len(ds)) % 3], 100.0 * (1 + (a + len(ds)) % 3), rng, 24, alloc, npt, nl, ds, delay=float(a))
             for a, (alloc, npt, nl) in enumerate(((slice(5, 17), 2, 2), (TWO_PIECES, 3, 3), ([7], 4, 4))) for ds in DMRS_SETS]
    out = run(ctx, cases)
    for i in range(0, len(cases), len(DMRS_SETS)):
        assert out[i][2][0] == 0.0 and out[i][2][1] == 0.0 and np.all(out[i][3] == 0.0)


@pytest.mark.parametrize("mode", T.MODES, ids=("interpolate", "line"))
def test_every_topology(ctx, mode):
    """L = 1 .. 4 on P = L .. 4, one batch, the DM-RS sets in turn."""
    rng = np.random.default_rng(92)
    cases = [tv_case(mode, (0.0, 400.0, -400.0)[k % 3], 100.0 * (k % 4), rng, 24, slice(3 + nl, 9 + nl + npt), npt, nl, DMRS_SETS[1 + k % 3], delay=float(k % 4),
                     slot=k, scr=100 + k)
             for k, (nl, npt) in enumerate(PL.TOPOLOGIES)]
    run(ctx, cases)


@pytest.mark.parametrize("mode", T.MODES, ids=("interpolate", "line"))
def test_window_with_dmrs_on_its_first_symbol(ctx, mode):
    """first_symbol = 2, nof_symbols = 10: nothing in front of the window is written, DM-RS bits outside it do not count, the first symbol carries DM-RS
    and symbols 10 and 11 are extrapolated; numerology 0, where symbol 7 carries the long prefix inside a gap."""
    rng = np.random.default_rng(93)
    cases = [tv_case(mode, 400.0, 200.0, rng, 24, TWO_PIECES, 2, 2, [0, 2, 6, 9, 13], first=2, nof=10, delay=2.0),
             tv_case(mode, -400.0, 300.0, rng, 24, slice(5, 17), 4, 3, [2, 9], first=2, nof=10, delay=1.0),
             tv_case(mode, 150.0, 100.0, rng, 24, slice(5, 17), 2, 1, [2, 6, 9], first=2, nof=10, numerology=0, slot=0, delay=1.0)]
    run(ctx, cases)


def test_widest_allocation(ctx):
    """275 PRBs on 4 x 4 with four DM-RS symbols: 1 650 pilots, the bound of the kernel's arrays and its largest LDS use."""
    rng = np.random.default_rng(94)
    run(ctx, [tv_case(T.INTERPOLATE, 400.0, 200.0, rng, 275, slice(0, 275), 4, 4, [2, 5, 8, 11], delay=2.0)])


def _mixed(rng):
    return [tv_case(mode, f, fd, rng, 24, slice(2, 2 + 3 * nl), npt, nl, dsyms, delay=float(nl - 1), slot=nl)
            for mode, f, fd, nl, npt, dsyms in ((T.LINE, 400.0, 100.0, 1, 2, [2, 11]), (T.INTERPOLATE, -400.0, 200.0, 2, 2, [2, 7, 11]), (T.LINE, 0.0, 300.0, 3, 4, [2]),
                                                (T.INTERPOLATE, 150.0, 300.0, 4, 4, [2, 5, 8, 11]), (T.LINE, -400.0, 200.0, 1, 1, [2, 7, 11]))]


def test_mixed_batch_gives_each_job_the_bytes_it_has_alone(ctx):
    """Jobs with different modes, offsets, layer counts and DM-RS sets in one batch: estimate, scalars, {cfo_hz, rho} and var of every job are, bit for
    bit, those of the job run alone (fixed summation order, no atomics)."""
    cases = _mixed(np.random.default_rng(95))
    out = run(ctx, cases)
    for i, c in enumerate(cases):
        alone = run(ctx, [c], check=False)[0]
        assert same_bytes(out[i], alone), i


def test_device_resident_jobs(ctx):
    """Jobs in device memory, without and with the port / layer hint, write what host jobs write and nothing else."""
    cases = _mixed(np.random.default_rng(96))
    host = run(ctx, cases)
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, device=device, check=False)
        for i, (h, d) in enumerate(zip(host, dev)):
            assert same_bytes(h, d), (device, i)


def _set(path, value):
    def edit(job):
        rec = job
        for name in path[:-1]:
            rec = rec[name]
        if path[-1] == "reserved":
            rec["reserved"][3] = value
        else:
            rec[path[-1]] = value
        if path[-1] == "hop_symbol":
            rec["rb_mask2"] = rec["rb_mask"]
    return edit


BREACHES = {"mode0": _set(("time_mode",), 0), "mode3": _set(("time_mode",), 3), "reserved": _set(("reserved",), 1), "compact": _set(("base", "base", "ce_compact"), 1),
            "hopping": _set(("base", "base", "hop_symbol"), 7), "layers5": _set(("base", "base", "nof_tx_layers"), 5)}


@pytest.mark.parametrize("breach", BREACHES, ids=list(BREACHES))
def test_host_jobs_that_break_a_rule_are_refused(ctx, breach):
    """A mode outside {1, 2}, a reserved byte, ce_compact, hopping, five layers: MIPHY_EINVAL with nothing enqueued -- the jobs in front included."""
    cases = _mixed(np.random.default_rng(97))[:3]
    run(ctx, cases, edit=lambda jobs: BREACHES[breach](jobs[1]), refused=True)


def test_device_resident_jobs_that_break_a_rule_are_skipped(ctx):
    """The same breaches in device memory: the broken jobs keep their sentinels, the sound ones give the bytes of a host run of the sound jobs."""
    rng = np.random.default_rng(98)
    names = list(BREACHES)
    cases = [tv_case(T.MODES[k % 2], 400.0, 200.0, rng, 24, slice(2 + k, 8 + 2 * k), 2, (1, 2)[k % 2], [2, 7, 11], delay=float(k % 3), slot=k, scr=40 + k)
             for k in range(2 * len(names))]
    sound, broken = list(range(0, len(cases), 2)), dict(zip(range(1, len(cases), 2), names))

    def breach(jobs):
        for i, name in broken.items():
            BREACHES[name](jobs[i])

    host = run(ctx, [cases[i] for i in sound])
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, device=device, check=False, edit=breach)
        for h, i in zip(host, sound):
            assert same_bytes(h, dev[i]), (device, i)
        for i in broken:
            assert np.all(dev[i][0] == 1.0) and np.all(dev[i][1] == np.float32(SC_SENTINEL)) and np.all(dev[i][2] == np.float32(CFO_SENTINEL)) \
                and np.all(dev[i][3] == np.float32(VAR_SENTINEL)), (device, i)
