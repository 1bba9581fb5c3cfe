"""GPU: miphy_dmrs_pusch_estimate_cfo_batch against the float64 restatement of tests/pusch_cfo_cases.py. Tolerances: those of
tests/test_chest_layers_gpu.py (coefficients 1e-4 of the largest estimate, RSRP / EPRE / noise / SNR 1e-4 relative, time alignment 1.01 IDFT
taps); the offset as the phase it turns the longest DM-RS gap by, 2 pi |cfo_hz - expected| max dt <= 1e-4 rad (the coefficient bound expressed as
a phase); rho 1e-4 relative. The grids carry the background noise of tests/pusch_layers_estimator_cases.py, rotated with the rest. Every offset
keeps |f| max dt <= 0.4 cycles, away from the wrap at 0.5. Sentinels: estimate 1.0, scalars -77, {cfo_hz, rho} -55."""
import numpy as np
import pytest

import pusch_cfo_cases as F
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

pytestmark = pytest.mark.gpu

CE_GUARD, SC_GUARD, CFO_GUARD, SC_SENTINEL, CFO_SENTINEL = 5, 3, 1, -77.0, -55.0
TWO_PIECES = list(range(2, 10)) + list(range(14, 18))  # 12 PRBs: a pair must not reach across the gap, interpolation does
_expected = {}


def offset_case(f_hz, *args, **kw):
    """E.make_case() with the offset applied to the grid."""
    case = E.make_case(*args, **kw)[0]
    assert abs(f_hz) * F.max_gap(case) <= 0.4, (f_hz, F.max_gap(case))
    return case[:-1] + (F.apply_cfo(case[-1], case[0], case[1], f_hz),)


def expected(case):
    if id(case) not in _expected:  # (the entry keeps the case object alive: its id is not reused)
        _expected[id(case)] = (case, F.estimate(*case))
    return _expected[id(case)][1]


def run(ctx, cases, device=None, check=True, edit=None, refused=False):
    """The cases as one batch. device: None (host jobs), "nohint" or "hint". edit: called with the job records before they are sent. refused: the
    call must fail with MIPHY_EINVAL and write nothing. Returns per job (estimate [nl][ports][rows][nsc], scalars [ports][nl][5], {cfo_hz, rho})
    as the device wrote them; everything outside the records must keep its sentinel."""
    import torch
    import miphy
    jobs = np.zeros(len(cases), dtype=miphy.PuschChestCfoJob)
    grids, g_off, ce_off, sc_off, cfo_off, shapes = [], 0, CE_GUARD, SC_GUARD, CFO_GUARD, []
    for i, (mu, slot, t2, scr, nscid, scaling, sm, rb, first, nof, nl, g) in enumerate(cases):
        j = jobs[i]["base"]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = mu, slot, scr, scaling
        j["n_scid"], j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"] = nscid, nl, g.shape[0], first, nof
        j["rx_ports"] = [0, 1, 2, 3]
        j["symbols_mask"] = sum(int(b) << l for l, b in enumerate(sm))
        j["grid_nof_prb"] = rb.size
        j["rb_mask"] = PL.mask_words(rb)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = g_off, ce_off, sc_off
        jobs[i]["cfo_offset"] = cfo_off
        grids.append(g.reshape(-1))
        g_off += g.size
        shapes.append((nl, g.shape[0], first + nof, g.shape[2]))
        ce_off += int(np.prod(shapes[-1])) + CE_GUARD
        sc_off += g.shape[0] * nl * 5 + SC_GUARD
        cfo_off += 2 + CFO_GUARD
    if edit is not None:
        edit(jobs)
    g_d = torch.from_numpy(np.concatenate(grids).astype(np.complex64)).cuda()
    ce_d = torch.ones(ce_off, dtype=torch.complex64, device="cuda")
    sc_d = torch.full((sc_off,), SC_SENTINEL, dtype=torch.float32, device="cuda")
    cfo_d = torch.full((cfo_off,), CFO_SENTINEL, dtype=torch.float32, device="cuda")
    if refused:
        with pytest.raises(RuntimeError, match="miphy error -1: miphy_dmrs_pusch_estimate_cfo_batch: job 1:"):  # (the prefix names the entry point)
            ctx.dmrs_pusch_estimate_cfo_batch(jobs, g_d, ce_d, sc_d, cfo_d)
        torch.cuda.synchronize()
        assert bool((ce_d == 1.0).all()) and bool((sc_d == SC_SENTINEL).all()) and bool((cfo_d == CFO_SENTINEL).all()), "a refused batch writes nothing"
        return None
    if device is None:
        ctx.dmrs_pusch_estimate_cfo_batch(jobs, g_d, ce_d, sc_d, cfo_d)
    else:
        hint = dict(max_ports=int(jobs["base"]["nof_rx_ports"].max()), max_layers=min(4, int(jobs["base"]["nof_tx_layers"].max()))) if device == "hint" else {}
        ctx.dmrs_pusch_estimate_cfo_batch(torch.from_numpy(jobs.view(np.uint8)).cuda(), g_d, ce_d, sc_d, cfo_d, **hint)
    torch.cuda.synchronize()
    ce, sc, cfo = ce_d.cpu().numpy(), sc_d.cpu().numpy(), cfo_d.cpu().numpy()
    used_ce, used_sc, used_cfo = np.zeros(ce.size, bool), np.zeros(sc.size, bool), np.zeros(cfo.size, bool)
    out = []
    for i, shp in enumerate(shapes):
        c0, s0, f0 = int(jobs[i]["base"]["ce_offset"]), int(jobs[i]["base"]["scalars_offset"]), int(jobs[i]["cfo_offset"])
        n_ce, n_sc = int(np.prod(shp)), shp[0] * shp[1] * 5
        used_ce[c0:c0 + n_ce] = used_sc[s0:s0 + n_sc] = used_cfo[f0:f0 + 2] = True
        out.append((ce[c0:c0 + n_ce].reshape(shp), sc[s0:s0 + n_sc].reshape(shp[1], shp[0], 5), cfo[f0:f0 + 2]))
    assert np.all(ce[~used_ce] == 1.0) and np.all(sc[~used_sc] == np.float32(SC_SENTINEL)) and np.all(cfo[~used_cfo] == np.float32(CFO_SENTINEL)), \
        "written outside the jobs' records"
    if not check:
        return out
    for i, a in enumerate(cases):
        mu, rb, first = a[0], a[7], a[8]
        exp_ce, exp_sc, exp_f, exp_rho = expected(a)
        got_ce, got_sc, got_cfo = out[i]
        mask = np.repeat(rb.astype(bool), 12)
        assert np.all(got_ce[:, :, :first] == 1.0), "rows in front of the allocation are left untouched"
        assert np.all(got_ce[..., ~mask] == 1.0), "unallocated PRBs are left untouched"
        got_ce, exp_ce = got_ce[:, :, first:], exp_ce[:, :, first:]
        err = np.abs(got_ce[..., mask] - exp_ce[..., mask]).max() / np.abs(exp_ce[..., mask]).max()
        turn = 2 * np.pi * abs(float(got_cfo[0]) - exp_f) * F.max_gap(a)
        rho_err = abs(float(got_cfo[1]) - exp_rho) / exp_rho if exp_rho else abs(float(got_cfo[1]))
        print("job %d: estimate error %.3g of the largest estimate; cfo_hz %.4f (expected %.4f: %.3g rad over the longest gap); rho %.6f (relative error %.3g)"
              % (i, err, got_cfo[0], exp_f, turn, got_cfo[1], rho_err))
        assert err < 1e-4, (i, err)
        assert turn <= 1e-4, (i, got_cfo[0], exp_f)
        assert rho_err <= 1e-4, (i, got_cfo[1], exp_rho)
        for k in range(4):
            rel = np.abs(got_sc[..., k] - exp_sc[..., k]) / (np.abs(exp_sc[..., k]) + 1e-30)
            print("job %d: scalar %d relative error %.3g" % (i, k, rel.max()))
            assert rel.max() < 1e-4, (i, k, got_sc[..., k], exp_sc[..., k])
        tap = 1.0 / (4096 * 15000.0 * (1 << mu))
        assert np.abs(got_sc[..., 4] - exp_sc[..., 4]).max() <= 1.01 * tap, (i, got_sc[..., 4], exp_sc[..., 4])
    return out


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_small_and_split_allocations(ctx):
    """1 PRB, 2 PRBs, 12 PRBs in two pieces; 1, 2, 3 and 4 DM-RS symbols, unequal gaps (2, 5, 11) included; one DM-RS symbol gives {0, 0}."""
    rng = np.random.default_rng(81)
    cases = [offset_case(-1000.0, rng, 24, [7], 2, 2, [2, 11], delay=1.0),
             offset_case(400.0, rng, 24, [22, 23], 4, 4, [2, 5, 11], delay=3.0),
             offset_case(-1000.0, rng, 24, TWO_PIECES, 3, 3, [2, 5, 8, 11], delay=2.0),
             offset_case(400.0, rng, 24, TWO_PIECES, 2, 1, [2, 3, 11], delay=2.0),
             offset_case(400.0, rng, 24, TWO_PIECES, 2, 2, [3], delay=0.0),
             offset_case(0.0, rng, 24, [0], 1, 1, [2, 7, 11], delay=0.0)]
    out = run(ctx, cases)
    assert out[4][2][0] == 0.0 and out[4][2][1] == 0.0


def test_every_topology(ctx):
    """L = 1 .. 4 on P = L .. 4, one batch; three DM-RS symbols (the fitted noise rule) on every other job; offsets 0, 400 and -1000 Hz in turn."""
    rng = np.random.default_rng(82)
    cases = [offset_case((0.0, 400.0, -1000.0)[k % 3], rng, 24, slice(3 + nl, 9 + nl + npt), npt, nl, [2, 7, 11] if k % 2 else [2, 11], delay=float(k % 4),
                         slot=k, scr=100 + k)
             for k, (nl, npt) in enumerate(PL.TOPOLOGIES)]
    run(ctx, cases)


def test_widest_grid(ctx):
    """Across the 64-PRB mask words of a 275-PRB grid, and the full 275 PRBs on 4 x 4 (1 650 pilots: the bound of the kernels' arrays)."""
    rng = np.random.default_rng(83)
    cases = [offset_case(400.0, rng, 275, [63, 64, 65, 127, 128, 191, 192, 255, 256, 274], 2, 2, [2, 7, 11], numerology=3, slot=79, delay=1.0),
             offset_case(-1000.0, rng, 275, slice(0, 275), 4, 4, [2, 11], delay=2.0),
             offset_case(400.0, rng, 275, [274], 3, 3, [2, 11], delay=0.0)]
    run(ctx, cases)


def test_partial_slots_prefixes_and_numerologies(ctx):
    """first_symbol > 0 (nothing in front of it is written, a DM-RS bit outside the allocation does not count); numerology 0, where symbol 7 carries the
    long prefix inside a gap (2 -> 11, 6 -> 9), 1 and 2. At numerology 2 symbol 0 of slots 0 and 38 carries the long prefix and symbol 0 of slots 1 and
    39 does not; tau_l is the start of the USEFUL part, so the prefix of symbol 0 is in front of every tau of the slot and leaves their differences:
    with a DM-RS symbol on symbol 0 a kernel that counted it would be off by 16 * 2^mu samples per gap."""
    rng = np.random.default_rng(84)
    cases = [offset_case(-1000.0, rng, 24, TWO_PIECES, 2, 2, [3, 10], first=2, nof=10, delay=2.0),
             offset_case(400.0, rng, 25, slice(3, 20), 4, 3, [0, 2, 7, 12], first=1, nof=11, delay=3.0),
             offset_case(400.0, rng, 24, slice(5, 17), 2, 2, [2, 11], numerology=0, slot=9, delay=1.0),
             offset_case(-1000.0, rng, 24, slice(5, 17), 2, 1, [4, 6, 9], numerology=0, slot=0, delay=1.0),
             offset_case(-1000.0, rng, 24, slice(5, 17), 2, 2, [0, 11], numerology=2, slot=0, delay=1.0),
             offset_case(-1000.0, rng, 24, slice(5, 17), 2, 2, [0, 11], numerology=2, slot=1, delay=1.0),
             offset_case(400.0, rng, 24, slice(5, 17), 3, 2, [0, 5, 13], numerology=2, slot=38, delay=0.0),
             offset_case(400.0, rng, 24, slice(5, 17), 3, 2, [0, 5, 13], numerology=2, slot=39, delay=0.0)]
    run(ctx, cases)
    assert F.max_gap(cases[6]) == F.max_gap(cases[7]) and F.max_gap(cases[2]) > 9 * (2048 + 144) / 30.72e6


def _mixed(rng):
    return [offset_case(f, rng, 24, slice(2, 2 + 3 * nl), npt, nl, dsyms, delay=float(nl - 1), slot=nl)
            for f, nl, npt, dsyms in ((400.0, 1, 2, [2, 11]), (-1000.0, 2, 2, [2, 7, 11]), (0.0, 3, 4, [2]), (150.0, 4, 4, [2, 7, 11]), (-400.0, 1, 1, [2, 7, 11]))]


def test_mixed_batch_gives_each_job_the_bytes_it_has_alone(ctx):
    """Jobs with different offsets, layer counts and DM-RS sets in one batch: every job's estimate, scalars and {cfo_hz, rho} are, bit for bit, those of
    the job run alone (fixed summation order, no atomics)."""
    cases = _mixed(np.random.default_rng(85))
    out = run(ctx, cases)
    for i, c in enumerate(cases):
        alone = run(ctx, [c], check=False)[0]
        assert same_bytes(out[i], alone), i


def test_device_resident_jobs(ctx):
    """Jobs in device memory, without and with the port / layer hint, write what host jobs write and nothing else."""
    cases = _mixed(np.random.default_rng(86))
    host = run(ctx, cases)
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, device=device, check=False)
        for i, (h, d) in enumerate(zip(host, dev)):
            assert same_bytes(h, d), (device, i)


BREACHES = (("ce_compact", 1), ("hop_symbol", 7), ("nof_tx_layers", 5))


@pytest.mark.parametrize("field,value", BREACHES)
def test_host_jobs_that_break_a_rule_are_refused(ctx, field, value):
    """ce_compact, hopping, five layers: MIPHY_EINVAL with nothing enqueued -- the jobs in front of it included."""
    cases = _mixed(np.random.default_rng(87))[:3]

    def breach(jobs):
        jobs[1]["base"][field] = value
        if field == "hop_symbol":
            jobs[1]["base"]["rb_mask2"] = jobs[1]["base"]["rb_mask"]

    run(ctx, cases, edit=breach, refused=True)


def test_device_resident_jobs_that_break_a_rule_are_skipped(ctx):
    """The same breaches in device memory: the broken jobs keep their sentinels, the sound ones give the bytes of a host run of the sound jobs."""
    rng = np.random.default_rng(88)
    cases = [offset_case(400.0, rng, 24, slice(2 + k, 8 + 2 * k), 2, nl, [2, 7, 11], delay=float(k % 3), slot=k, scr=40 + k) for k, nl in enumerate((1, 2, 2, 1, 2, 2))]
    sound, broken = [0, 2, 4], dict(zip((1, 3, 5), BREACHES))

    def breach(jobs):
        for i, (field, value) in broken.items():
            jobs[i]["base"][field] = value

    host = run(ctx, [cases[i] for i in sound])
    for device in ("nohint", "hint"):
        dev = run(ctx, cases, device=device, check=False, edit=breach)
        for h, i in zip(host, sound):
            assert same_bytes(h, dev[i]), (device, i)
        for i in broken:
            assert np.all(dev[i][0] == 1.0) and np.all(dev[i][1] == np.float32(SC_SENTINEL)) and np.all(dev[i][2] == np.float32(CFO_SENTINEL)), (device, i)
