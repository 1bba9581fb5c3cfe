"""One batch of DM-RS estimator jobs on the GPU, for tests/test_chest_gpu.py (expected values: the CPU oracle) and tests/test_chest_layers_gpu.py
(expected values: the float64 restatement of tests/pusch_layers_estimator_cases.py).

Tolerances (floating point; the reference's own vector test uses 5e-4 on every output, port_channel_estimator_test.cpp:114-169):
channel coefficients 1e-4 * max|h| (the reference interpolates by repeated float accumulation, the kernel in closed form),
RSRP / EPRE / noise / SNR 1e-4 relative, time alignment exact to one IDFT tap (1/(4096*scs))."""
import numpy as np
import pytest

CE_GUARD, SC_GUARD, SC_SENTINEL = 5, 3, -77.0  # elements between the records of two jobs; the estimate's sentinel is 1.0
SCATTERED = [63, 64, 65, 127, 128, 191, 192, 255, 256, 274]  # on a 275-PRB grid: an allocation in every 64-bit word of rb_mask
_expected = {}  # expected values per (function, case object, port selection), computed once


def select_ports(case, sel):
    """A case built on four grid ports, received on the ports `sel` only: the other ports of the grid become NaN, so that a read of a port the
    job does not name cannot go unnoticed. Returns (case, sel) for run(..., sels=...)."""
    g = case[-1].copy()
    assert g.shape[0] == 4 and len(set(sel)) == len(sel) and all(0 <= p < 4 for p in sel)
    g[[p for p in range(4) if p not in sel]] = np.nan
    return case[:-1] + (g,), list(sel)


def expected(estimate, case, sel):
    key = (estimate, id(case), tuple(sel) if sel is not None else None)
    if key not in _expected:  # (the entry keeps the case object alive: its id is not reused)
        _expected[key] = (case, estimate(*(case if sel is None else case[:-1] + (np.ascontiguousarray(case[-1][sel]),))))
    return _expected[key][1]


def run(ctx, cases, entry, estimate, sels=None, compact=False, device=None, room_4x4=False, check=True, hop=None, edit=None):
    """Runs the cases as one batch through the entry point `entry` and compares every job with estimate(*case). sels: per case None (the grid's
    ports 0..n-1 in order) or the list of grid ports the job receives on (the grid then has four ports; the unused tail of rx_ports names a port
    outside the selection). compact: ce_compact = 1 (one row per (layer, port)). device: None (host descriptors), "nohint" or "hint" (descriptors
    in device memory, without / with the largest port and layer counts of the batch). room_4x4: every job's estimate and scalar records are
    followed by room for the (layer, port) pairs up to 4 x 4 that it does not have, which must stay untouched. Records are separated by guard
    elements. hop: (job, symbol) -- that job asks for hopping and the batch must be refused. edit: called with the job records before they are sent.
    Returns per job (estimate [nl][ports][rows][nsc], scalars [ports][nl][5]) as the device wrote them."""
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
    if edit is not None:
        edit(jobs)
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
    # nothing but the records themselves is written: guards, and the room behind the records
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
        exp_ce, exp_sc = expected(estimate, a, sel)
        got_ce, got_sc = out[i]
        assert got_sc.shape == exp_sc.shape
        mask = np.repeat(rb.astype(bool), 12)
        if compact:  # one row, valid for every symbol of the allocation: the expected rows are all the same
            exp_ce = exp_ce[:, :, first:first + 1]
        else:
            assert np.all(got_ce[:, :, :first] == 1.0), "rows in front of the allocation are left untouched"
            got_ce, exp_ce = got_ce[:, :, first:], exp_ce[:, :, first:]
        err = np.abs(got_ce[..., mask] - exp_ce[..., mask]).max() / np.abs(exp_ce[..., mask]).max()
        print("job %d: estimate error %.3g of the largest estimate" % (i, err))
        assert err < 1e-4, (i, err)
        assert np.all(got_ce[..., ~mask] == 1.0), "unallocated PRBs are left untouched (they keep the caller's initial value)"
        for k in range(4):
            rel = np.abs(got_sc[..., k] - exp_sc[..., k]) / (np.abs(exp_sc[..., k]) + 1e-30)
            print("job %d: scalar %d relative error %.3g" % (i, k, rel.max()))
            assert rel.max() < 1e-4, (i, k, got_sc[..., k], exp_sc[..., k])
        tap = 1.0 / (4096 * 15000.0 * (1 << mu))
        assert np.abs(got_sc[..., 4] - exp_sc[..., 4]).max() <= 1.01 * tap, (i, got_sc[..., 4], exp_sc[..., 4])
    return out
