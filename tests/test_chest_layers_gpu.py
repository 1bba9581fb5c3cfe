"""GPU: miphy_dmrs_pusch_estimate_layers_batch against the float64 restatement of tests/pusch_layers_estimator_cases.py, with the tolerances of
tests/test_chest_gpu.py (coefficients 1e-4 of the largest estimate, RSRP / EPRE / noise / SNR 1e-4 relative, time alignment 1.01 IDFT taps). The
grids carry that file's background noise, so no scalar compared is a difference of nearly equal numbers. Sentinels: estimate 1.0, scalars -77."""
import numpy as np
import pytest

import pusch_layers_estimator_cases as E

pytestmark = pytest.mark.gpu

CE_GUARD, SC_GUARD, SC_SENTINEL = 5, 3, -77.0
_expected = {}  # restatement per case object, computed once


def expected(case, sel):
    key = (id(case), tuple(sel) if sel is not None else None)
    if key not in _expected:
        g = case[-1]
        _expected[key] = (case, E.estimate(*(case if sel is None else case[:-1] + (np.ascontiguousarray(g[sel]),))))
    return _expected[key][1]


def select_ports(case, sel):
    g = case[-1].copy()
    assert g.shape[0] == 4
    g[[p for p in range(4) if p not in sel]] = np.nan
    return case[:-1] + (g,), list(sel)


def run(ctx, cases, sels=None, compact=False, device=None, room_4x4=False, check=True, entry="dmrs_pusch_estimate_layers_batch", hop=None):
    """The cases as one batch (tests/test_chest_gpu.py's run() for the layered entry point). Returns per job (estimate [nl][ports][rows][nsc],
    scalars [ports][nl][5]) as written; everything outside the records must keep its sentinel."""
    import torch
    import miphy
    sels = sels or [None] * len(cases)
    jobs = np.zeros(len(cases), dtype=miphy.PuschChestJob)
    grids, g_off, ce_off, sc_off, shapes = [], 0, CE_GUARD, SC_GUARD, []
    for i, ((mu, slot, t2, scr, nscid, scaling, sm, rb, first, nof, nl, g), sel) in enumerate(zip(cases, sels)):
        nsc = g.shape[2]
        nports = g.shape[0] if sel is None else len(sel)
        j = jobs[i]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = mu, slot, scr, scaling
        j["n_scid"], j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"] = nscid, nl, nports, first, nof
        if sel is None:
            j["rx_ports"] = [0, 1, 2, 3]
        else:
            spare = [p for p in range(4) if p not in sel]
            j["rx_ports"] = list(sel) + spare[:1] * (4 - len(sel))
        j["ce_compact"] = int(compact)
        j["symbols_mask"] = sum(int(b) << l for l, b in enumerate(sm))
        j["grid_nof_prb"] = rb.size
        m = [0] * 5
        for r in np.nonzero(rb)[0]:
            m[r >> 6] |= 1 << (int(r) & 63)
        j["rb_mask"] = m
        if hop is not None and i == hop[0]:
            j["hop_symbol"], j["rb_mask2"] = hop[1], m
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = g_off, ce_off, sc_off
        grids.append(g.reshape(-1))
        g_off += g.size
        rows = 1 if compact else first + nof
        shapes.append((nl, nports, rows, nsc))
        ce_off += (16 if room_4x4 else nl * nports) * rows * nsc + CE_GUARD
        sc_off += (16 if room_4x4 else nports * nl) * 5 + SC_GUARD
    g_d = torch.from_numpy(np.concatenate(grids)).cuda()
    ce_d = torch.ones(ce_off, dtype=torch.complex64, device="cuda")
    sc_d = torch.full((sc_off,), SC_SENTINEL, dtype=torch.float32, device="cuda")
    call = getattr(ctx, entry)
    if hop is not None:
        with pytest.raises(RuntimeError, match="miphy error -1"):
            call(jobs, g_d, ce_d, sc_d)
        torch.cuda.synchronize()
        assert bool((ce_d == 1.0).all()) and bool((sc_d == SC_SENTINEL).all()), "a refused batch writes nothing"
        return None
    if device is None:
        call(jobs, g_d, ce_d, sc_d)
    else:
        hint = dict(max_ports=int(jobs["nof_rx_ports"].max()), max_layers=int(jobs["nof_tx_layers"].max())) if device == "hint" else {}
        call(torch.from_numpy(jobs.view(np.uint8)).cuda(), g_d, ce_d, sc_d, **hint)
    torch.cuda.synchronize()
    ce, sc = ce_d.cpu().numpy(), sc_d.cpu().numpy()
    used_ce, used_sc = np.zeros(ce.size, bool), np.zeros(sc.size, bool)
    out = []
    for i, shp in enumerate(shapes):
        c0, s0 = int(jobs[i]["ce_offset"]), int(jobs[i]["scalars_offset"])
        n_ce, n_sc = int(np.prod(shp)), shp[0] * shp[1] * 5
        used_ce[c0:c0 + n_ce] = True
        used_sc[s0:s0 + n_sc] = True
        out.append((ce[c0:c0 + n_ce].reshape(shp), sc[s0:s0 + n_sc].reshape(shp[1], shp[0], 5)))
    assert np.all(ce[~used_ce] == 1.0) and np.all(sc[~used_sc] == np.float32(SC_SENTINEL)), "written outside the jobs' records"
    if not check:
        return out
    for i, (a, sel) in enumerate(zip(cases, sels)):
        mu, rb, first = a[0], a[7], a[8]
        exp_ce, exp_sc = expected(a, sel)
        got_ce, got_sc = out[i]
        mask = np.repeat(rb.astype(bool), 12)
        if compact:
            exp_ce = exp_ce[:, :, first:first + 1]
        else:
            assert np.all(got_ce[:, :, :first] == 1.0), "rows in front of the allocation are left untouched"
            got_ce, exp_ce = got_ce[:, :, first:], exp_ce[:, :, first:]
        err = np.abs(got_ce[..., mask] - exp_ce[..., mask]).max() / np.abs(exp_ce[..., mask]).max()
        print("job %d: estimate error %.3g of the largest estimate" % (i, err))
        assert err < 1e-4, (i, err)
        assert np.all(got_ce[..., ~mask] == 1.0), "unallocated PRBs are left untouched"
        for k in range(4):
            rel = np.abs(got_sc[..., k] - exp_sc[..., k]) / (np.abs(exp_sc[..., k]) + 1e-30)
            print("job %d: scalar %d relative error %.3g" % (i, k, rel.max()))
            assert rel.max() < 1e-4, (i, k, got_sc[..., k], exp_sc[..., k])
        tap = 1.0 / (4096 * 15000.0 * (1 << mu))
        assert np.abs(got_sc[..., 4] - exp_sc[..., 4]).max() <= 1.01 * tap, (i, got_sc[..., 4], exp_sc[..., 4])
    return out


TWO_PIECES = list(range(2, 10)) + list(range(14, 18))  # 12 PRBs: a pair must not reach across the gap, interpolation does
SCATTERED = [63, 64, 65, 127, 128, 191, 192, 255, 256, 274]  # on a 275-PRB grid: an allocation in every 64-bit word of rb_mask


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
