"""GPU: PUSCH demodulator kernel (RE extraction + ZF/MRC equalisation + soft demapping + descrambling) through the
C ABI against the oracle (bit-exact: both sides use single IEEE operations in the same order) and against reference-produced
LLRs from tests/golden/pusch_demod.npz (stated tolerance: one quantisation step, see test_oracle_golden.py)."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _mask_words(rb):
    w = np.zeros(5, dtype=np.uint64)
    for r in np.nonzero(rb)[0]:
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def _job(miphy, rnti, n_id, mod, start, nof, dm, type2, cdm, rb, ports, ce_syms, grid_off=0, ce_off=0, sc_off=0, llr_off=0):
    j = np.zeros(1, dtype=miphy.PuschDemodJob)[0]
    j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = rnti, n_id, mod, ports, start, nof
    j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"] = 2 if type2 else 1, cdm, ce_syms
    j["rx_ports"] = [0, 1, 2, 3]
    j["dmrs_symbols_mask"] = sum(1 << int(s) for s in np.nonzero(dm)[0])
    j["grid_nof_prb"] = rb.size
    j["rb_mask"] = _mask_words(rb)
    j["grid_offset"], j["ce_offset"], j["scalars_offset"], j["llr_offset"] = grid_off, ce_off, sc_off, llr_off
    j["nof_llr"] = miphy.pusch_demod_nof_llr(j)
    return j


def _run(ctx, jobs, grids, ces, nvs, total_llr):
    import torch
    import miphy
    g = torch.from_numpy(np.concatenate([x.reshape(-1) for x in grids])).cuda()
    h = torch.from_numpy(np.concatenate([x.reshape(-1) for x in ces])).cuda()
    sc = np.zeros(5 * len(nvs), dtype=np.float32)
    sc[2::5] = nvs
    out = torch.full((total_llr + 64,), 99, dtype=torch.int8, device="cuda")
    ctx.pusch_demodulate_batch(np.array(jobs, dtype=miphy.PuschDemodJob), g, h, torch.from_numpy(sc).cuda(), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_golden_vectors_and_oracle(ctx):
    import miphy
    d = np.load(os.path.join(GOLD, "pusch_demod.npz"))
    n = sum(1 for k in d.files if k.startswith("grid_"))
    jobs, grids, ces, nvs, offs, exp = [], [], [], [], [], []
    goff = coff = loff = 0
    for i in range(n):
        rnti, n_id, mod, start, nof, cdm, nv = d["meta_%d" % i]
        grid, ce, rb, dm = d["grid_%d" % i], d["ce_%d" % i], d["rb_%d" % i], d["dm_%d" % i]
        j = _job(miphy, int(rnti), int(n_id), int(mod), int(start), int(nof), dm, 0, int(cdm), rb, grid.shape[0], 14, goff, coff, 5 * i, loff)
        assert j["nof_llr"] == d["llr_%d" % i].size
        jobs.append(j)
        grids.append(grid)
        ces.append(ce)
        nvs.append(nv)
        offs.append((loff, int(j["nof_llr"])))
        exp.append(O.o_pusch_demodulate(int(rnti), int(n_id), int(mod), int(start), int(nof), dm, 0, int(cdm), rb, grid, ce, float(nv))[0])
        goff += grid.size
        coff += ce.size
        loff += int(j["nof_llr"]) + 3  # deliberately unaligned codeword starts
    out = _run(ctx, jobs, grids, ces, nvs, loff)
    for i, (o, ln) in enumerate(offs):
        got = out[o:o + ln]
        assert np.array_equal(got, exp[i]), (i, int(np.abs(got.astype(int) - exp[i].astype(int)).max()))
        ref = d["llr_%d" % i]
        diff = np.abs(got.astype(int) - ref.astype(int))
        assert diff.max() <= 1 and (diff == 0).mean() > 0.97
        assert np.all(out[o + ln:o + ln + 3] == 99)  # nothing written past the codeword


@pytest.mark.parametrize("mod,ports,cdm,type2,nprb,start,nof,dsyms", [
    (8, 1, 2, 0, 273, 0, 14, (2,)),          # the 100 MHz workload of the benchmark
    (6, 4, 1, 0, 106, 0, 14, (2, 7, 11)),
    (4, 2, 2, 0, 52, 2, 12, (3, 10)),
    (2, 1, 1, 0, 25, 0, 14, (2, 11)),
    (1, 2, 2, 0, 11, 1, 9, (4,)),
    (6, 1, 1, 1, 40, 0, 14, (2,)),            # DM-RS type 2
    (8, 3, 2, 1, 33, 0, 13, (2, 11)),
    (4, 2, 3, 1, 20, 0, 14, (2,)),            # type 2, all CDM groups: no data on the DM-RS symbol
])
def test_random_allocations_match_oracle(ctx, mod, ports, cdm, type2, nprb, start, nof, dsyms):
    import miphy
    rng = np.random.default_rng(1000 * mod + nprb)
    nsc = nprb * 12
    rb = (rng.uniform(size=nprb) < 0.85).astype(np.uint8)
    rb[nprb // 2] = 1
    if nprb == 273:
        rb[:] = 1
    dm = np.zeros(14, np.uint8)
    dm[list(dsyms)] = 1
    grid = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    ce = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    ce[0, start, 7] = 0
    grid[0, start + 1, 3] = np.nan
    rnti, n_id, nv = int(rng.integers(1, 65536)), int(rng.integers(0, 1024)), float(rng.uniform(0.01, 0.5))
    exp, _, _ = O.o_pusch_demodulate(rnti, n_id, mod, start, nof, dm, type2, cdm, rb, grid, ce, nv)
    j = _job(miphy, rnti, n_id, mod, start, nof, dm, type2, cdm, rb, ports, 14)
    assert j["nof_llr"] == exp.size
    out = _run(ctx, [j], [grid], [ce], [nv], exp.size)
    assert np.array_equal(out[:exp.size], exp)


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("mod,ports,cdm,type2,nprb,start,nof,dsyms,pad", [
    (8, 1, 2, 0, 273, 0, 14, (2,), 0),      # the benchmark's slot: every request of a thread in flight at once (demod_columns_deep)
    (6, 1, 2, 0, 106, 0, 14, (2, 7, 11), 0),
    (4, 1, 1, 0, 52, 2, 12, (3, 10), 0),
    (2, 1, 1, 1, 25, 1, 9, (4,), 0),         # DM-RS type 2, a partial slot
    (8, 1, 2, 0, 40, 0, 14, (2,), 3),        # codeword at an odd address: the byte-wise store path of the same walk
    (4, 1, 3, 1, 20, 0, 14, (2,), 0),        # type 2, all CDM groups: no data on the DM-RS symbol
    (6, 2, 2, 0, 60, 0, 14, (2, 11), 0),     # two ports with the compact estimate: the general walk
    (1, 1, 2, 0, 30, 0, 14, (2,), 0),        # pi/2-BPSK: the general walk
])
def test_compact_estimate_matches_oracle(ctx, mod, ports, cdm, type2, nprb, start, nof, dsyms, pad, device_jobs):
    """The estimate as ONE row per port (ce_compact, what the estimator of this library hands over): the demodulator then keeps the channel
    row in registers, and with one port it requests the samples of all OFDM symbols at once. Same LLRs as the oracle fed with that row
    on every symbol, including a zero channel coefficient, a NaN sample and partial allocations; descriptors in host and in device memory."""
    import torch
    import miphy
    rng = np.random.default_rng(2000 * mod + nprb + pad)
    nsc = nprb * 12
    rb = (rng.uniform(size=nprb) < 0.85).astype(np.uint8)
    rb[nprb // 2] = 1
    if nprb == 273:
        rb[:] = 1
    dm = np.zeros(14, np.uint8)
    dm[list(dsyms)] = 1
    grid = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    row = (rng.standard_normal((ports, 1, nsc)) + 1j * rng.standard_normal((ports, 1, nsc))).astype(np.complex64)
    row[0, 0, 12 * (nprb // 2) + 5] = 0
    grid[0, start + 1, 12 * (nprb // 2) + 3] = np.nan
    rnti, n_id, nv = int(rng.integers(1, 65536)), int(rng.integers(0, 1024)), float(rng.uniform(0.01, 0.5))
    exp, _, _ = O.o_pusch_demodulate(rnti, n_id, mod, start, nof, dm, type2, cdm, rb, grid, np.repeat(row, 14, axis=1), nv)
    j = _job(miphy, rnti, n_id, mod, start, nof, dm, type2, cdm, rb, ports, 14, llr_off=pad)
    j["ce_compact"] = 1
    assert j["nof_llr"] == exp.size
    g = torch.from_numpy(grid.reshape(-1)).cuda()
    h = torch.from_numpy(row.reshape(-1)).cuda()
    sc = np.zeros(5, dtype=np.float32)
    sc[2] = nv
    out = torch.full((exp.size + pad + 64,), 99, dtype=torch.int8, device="cuda")
    jobs = np.array([j], dtype=miphy.PuschDemodJob)
    ctx.pusch_demodulate_batch(torch.from_numpy(jobs.view(np.uint8)).cuda() if device_jobs else jobs, g, h, torch.from_numpy(sc).cuda(), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[pad:pad + exp.size], exp)
    assert np.all(got[:pad] == 99) and np.all(got[pad + exp.size:] == 99)
    if device_jobs and nprb == 273:
        # captured once it has run at its size on a context of its own, the call stays valid after a larger call has grown that context's
        # sequence workspace
        gctx = miphy.Context(0)
        try:
            jobs_d, sc_d = torch.from_numpy(jobs.view(np.uint8)).cuda(), torch.from_numpy(sc).cuda()
            gctx.pusch_demodulate_batch(jobs_d, g, h, sc_d, out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gctx.pusch_demodulate_batch(jobs_d, g, h, sc_d, out, torch.cuda.current_stream())
            stride = (exp.size + 15) // 16 * 16
            many = np.repeat(jobs, 64)
            many["llr_offset"] = np.arange(64) * stride
            out_many = torch.zeros(64 * stride, dtype=torch.int8, device="cuda")
            gctx.pusch_demodulate_batch(many, g, h, sc_d, out_many)
            torch.cuda.synchronize()
            assert np.array_equal(out_many.cpu().numpy().reshape(64, stride)[:, :exp.size], np.tile(exp, (64, 1)))
            out.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[pad:pad + exp.size], exp)
            assert np.all(got[:pad] == 99) and np.all(got[pad + exp.size:] == 99)
            del graph
        finally:
            torch.cuda.synchronize()
            gctx.close()


def test_rejections(ctx):
    """pusch_demodulator_impl.cpp:76-83 asserts the codeword length and the single layer; the C ABI reports MIPHY_EINVAL."""
    import torch
    import miphy
    rb = np.ones(10, np.uint8)
    dm = np.zeros(14, np.uint8)
    dm[2] = 1
    x = torch.zeros(4 * 14 * 120, dtype=torch.complex64, device="cuda")
    f = torch.zeros(16, dtype=torch.float32, device="cuda")
    o = torch.zeros(40000, dtype=torch.int8, device="cuda")
    for bad in (dict(nof_llr=8), dict(mod=3), dict(nof_rx_ports=5), dict(dmrs_type=3), dict(nof_cdm_groups_without_data=3), dict(nof_symbols=15),
                dict(ce_nof_symbols=5)):
        j = _job(miphy, 1, 2, 4, 0, 14, dm, 0, 2, rb, 1, 14)
        for k, v in bad.items():
            j[k] = v
        with pytest.raises(RuntimeError):
            ctx.pusch_demodulate_batch(np.array([j], dtype=miphy.PuschDemodJob), x, x, f, o)


@pytest.mark.parametrize("mod,ports,cdm", [(2, 1, 2), (4, 2, 2), (6, 1, 1), (8, 4, 2), (1, 1, 2)])
def test_placeholders_and_evm_match_oracle(ctx, mod, ports, cdm):
    """UCI on PUSCH: repetition placeholders in the descrambler (bit-exact LLRs against the oracle) and the per-symbol EVM sums
    (EVM within 2e-6 relative of the oracle's sequential sum: the kernel adds in a tree)."""
    import torch
    import miphy
    rng = np.random.default_rng(900 + mod)
    nprb = 31
    nsc = nprb * 12
    rb = np.zeros(nprb, np.uint8)
    rb[1:27] = 1
    dm = np.zeros(14, np.uint8)
    dm[[3, 10]] = 1
    grid = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    ce = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    n_re = O.pusch_nof_re(1, 12, dm, 0, cdm, rb)
    ph = np.sort(rng.choice(n_re, 53, replace=False)).astype(np.uint16) if mod >= 2 else np.zeros(0, np.uint16)
    j = _job(miphy, 0x1234, 77, mod, 1, 12, dm, 0, cdm, rb, ports, 14)
    j["placeholders_offset"], j["nof_placeholders"], j["evm_offset"] = 5, ph.size, 3
    g = torch.from_numpy(grid.reshape(-1)).cuda()
    h = torch.from_numpy(ce.reshape(-1)).cuda()
    sc = np.zeros(5, np.float32)
    sc[2] = 0.07
    out = torch.full((int(j["nof_llr"]) + 64,), 99, dtype=torch.int8, device="cuda")
    ph_d = torch.from_numpy(np.concatenate([np.zeros(5, np.uint16), ph, np.zeros(3, np.uint16)]).view(np.int16)).cuda()
    evm_d = torch.full((3 + 14 + 2,), -1.0, dtype=torch.float32, device="cuda")
    ctx.pusch_demodulate_batch_ex(np.array([j], dtype=miphy.PuschDemodJob), g, h, torch.from_numpy(sc).cuda(), out, ph_d, evm_d)
    torch.cuda.synchronize()
    o, oe = O.o_pusch_demodulate_ex(0x1234, 77, mod, 1, 12, dm, 0, cdm, rb, grid, ce, 0.07, placeholders=ph)
    got = out.cpu().numpy()
    assert np.array_equal(got[:o.size], o) and np.all(got[o.size:] == 99)
    e = evm_d.cpu().numpy()
    assert np.all(e[:3] == -1.0) and np.all(e[17:] == -1.0) and e[3] == 0.0 and e[3 + 13] == 0.0  # symbols outside the allocation contribute 0
    evm = float(np.sqrt(e[3:17].astype(np.float64).sum() / n_re))
    assert abs(evm - oe) <= 2e-6 * oe + 1e-7, (evm, oe)


@pytest.mark.parametrize("mod", [6, 2])
def test_placeholders_and_evm_with_device_jobs(ctx, mod):
    """pusch_demodulate_batch_ex with the jobs in device memory: the launch is sized for the widest grid, the two pointers (not the jobs)
    choose the kernel instance, and the workgroups of a chunk behind a narrow allocation leave in front of the barriers of the EVM sum.
    Two transmissions on a 24-PRB grid, symbols 2..13, DM-RS on 2 and 11, two receive ports: 22 PRB (two chunks, eight live lanes in
    the second; data on the DM-RS symbols) and 4 PRB (none), each with a short placeholder list and its EVM sums between sentinels;
    two jobs leave compute units idle, so the symbols are cut into parts as well. At modulation order 6 an element's chips straddle a
    word. LLRs bit-equal to the oracle, each EVM within the tolerance of test_placeholders_and_evm_match_oracle; host- and
    device-resident jobs, and the same jobs as layered records on one layer, give the same bytes; nothing else is written."""
    import torch
    import miphy
    rng = np.random.default_rng(7700 + mod)
    nprb, ports, start, nof = 24, 2, 2, 12
    nsc = nprb * 12
    dm = np.zeros(14, np.uint8)
    dm[[2, 11]] = 1
    rbs = [np.ones(nprb, np.uint8), np.zeros(nprb, np.uint8)]
    rbs[0][[5, 17]] = 0
    rbs[1][[3, 4, 9, 20]] = 1
    cdms, rntis, n_ids, nvs = [1, 2], [0x4321, 17], [1001, 5], [0.07, 0.2]
    grid = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    ce = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    jobs, phs, exp, n_res = [], [], [], []
    llr_off, ph_off, evm_off = 8, 5, 3  # the first codeword aligned, the second at an odd address
    for k in range(2):
        n_re = O.pusch_nof_re(start, nof, dm, 0, cdms[k], rbs[k])
        ph = np.sort(rng.choice(n_re, 9, replace=False)).astype(np.uint16)
        ph[0], ph[-1] = 0, n_re - 1  # the first and the last element of the codeword
        j = _job(miphy, rntis[k], n_ids[k], mod, start, nof, dm, 0, cdms[k], rbs[k], ports, 14, sc_off=5 * k, llr_off=llr_off)
        j["placeholders_offset"], j["nof_placeholders"], j["evm_offset"] = ph_off, ph.size, evm_off
        assert j["nof_llr"] == n_re * mod
        jobs.append(j)
        phs.append(ph)
        n_res.append(n_re)
        exp.append(O.o_pusch_demodulate_ex(rntis[k], n_ids[k], mod, start, nof, dm, 0, cdms[k], rbs[k], grid, ce, nvs[k], placeholders=ph))
        llr_off = (llr_off + n_re * mod + 8) // 8 * 8 + 3
        ph_off += ph.size + 3
        evm_off += 14 + 2
    assert n_res == [22 * (10 * 12 + 2 * 6), 4 * 10 * 12]
    jobs = np.array(jobs, dtype=miphy.PuschDemodJob)
    ljobs = np.zeros(2, dtype=miphy.PuschDemodLayersJob)
    ljobs["base"], ljobs["nof_tx_layers"] = jobs, 1
    ph_all = np.full(ph_off, 0xffff, np.uint16)
    for j, ph in zip(jobs, phs):
        ph_all[int(j["placeholders_offset"]):int(j["placeholders_offset"]) + ph.size] = ph
    g = torch.from_numpy(grid.reshape(-1)).cuda()
    h = torch.from_numpy(ce.reshape(-1)).cuda()
    sc = np.zeros(10, np.float32)
    sc[2::5] = nvs
    sc_d = torch.from_numpy(sc).cuda()
    ph_d = torch.from_numpy(ph_all.view(np.int16)).cuda()

    def run(entry, records, device_jobs):
        out = torch.full((llr_off + 64,), 99, dtype=torch.int8, device="cuda")
        evm_d = torch.full((evm_off,), -1.0, dtype=torch.float32, device="cuda")
        entry(torch.from_numpy(records.view(np.uint8)).cuda() if device_jobs else records, g, h, sc_d, out, ph_d, evm_d)
        torch.cuda.synchronize()
        return out.cpu().numpy(), evm_d.cpu().numpy()

    got, e = run(ctx.pusch_demodulate_batch_ex, jobs, True)
    used, summed = np.zeros(got.size, bool), np.zeros(e.size, bool)
    for k, j in enumerate(jobs):
        lo, eo = int(j["llr_offset"]), int(j["evm_offset"])
        o, oe = exp[k]
        assert np.array_equal(got[lo:lo + o.size], o), (k, np.nonzero(got[lo:lo + o.size] != o)[0][:8])
        used[lo:lo + o.size] = True
        summed[eo:eo + 14] = True
        assert e[eo] == 0.0 and e[eo + 1] == 0.0  # symbols outside the allocation contribute 0
        evm = float(np.sqrt(e[eo:eo + 14].astype(np.float64).sum() / n_res[k]))
        print("job %d: EVM %.9g, oracle %.9g" % (k, evm, oe))
        assert abs(evm - oe) <= 2e-6 * oe + 1e-7, (k, evm, oe)
    assert np.all(got[~used] == 99) and np.all(e[~summed] == -1.0)
    for entry, records, device_jobs in ((ctx.pusch_demodulate_batch_ex, jobs, False), (ctx.pusch_demodulate_layers_batch_ex, ljobs, False),
                                        (ctx.pusch_demodulate_layers_batch_ex, ljobs, True)):
        got2, e2 = run(entry, records, device_jobs)
        assert np.array_equal(got2, got) and np.array_equal(e2.view(np.uint32), e.view(np.uint32)), (entry.__name__, device_jobs)


# ------------------------------------------------------------------------------------------------ port lists, short estimates, the symbol split
def _item(rng, mod, sel, compact, cdm, type2, rb, start, nof, dsyms, ce_rows=14):
    """One transmission received on the grid ports `sel` of a four-port grid (the other ports are NaN: a read of a port the job does not name
    shows up in the LLRs), with its oracle LLRs. The estimate has len(sel) ports in the job's order: one row (compact) or ce_rows rows.
    As elsewhere in this file: one zero channel coefficient and one NaN sample inside the allocation."""
    nprb = rb.size
    nsc = nprb * 12
    dm = np.zeros(14, np.uint8)
    dm[list(dsyms)] = 1
    grid = np.full((4, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    grid[sel] = (rng.standard_normal((len(sel), 14, nsc)) + 1j * rng.standard_normal((len(sel), 14, nsc))).astype(np.complex64)
    rows = 1 if compact else ce_rows
    est = (rng.standard_normal((len(sel), rows, nsc)) + 1j * rng.standard_normal((len(sel), rows, nsc))).astype(np.complex64)
    mid = int(np.nonzero(rb)[0][rb.sum() // 2])
    est[0, 0 if compact else start, 12 * mid + 5] = 0
    grid[sel[-1], start + 1, 12 * mid + 3] = np.nan
    rnti, n_id, nv = int(rng.integers(1, 65536)), int(rng.integers(0, 1024)), float(rng.uniform(0.01, 0.5))
    exp = O.o_pusch_demodulate(rnti, n_id, mod, start, nof, dm, type2, cdm, rb, grid[sel], np.repeat(est, 14, axis=1) if compact else est, nv)[0]
    return dict(mod=mod, sel=list(sel), compact=compact, cdm=cdm, type2=type2, rb=rb, start=start, nof=nof, dm=dm, rows=rows, grid=grid, est=est,
                rnti=rnti, n_id=n_id, nv=nv, exp=exp)


LLR_SENTINEL = 99


def _run_items(ctx, items, order, llr_offsets, device_jobs, rng):
    """Launches items[order[k]] with its codeword at llr_offsets[k] as one batch (copies of an item share its grid, estimate and scalars) and
    requires every codeword to equal the item's oracle LLRs and every other byte of the output to keep its sentinel. The scalars array
    is random but for the noise variances, each job's block starts at an offset of its own that is no multiple of five, and the unused tail
    of rx_ports names a port outside the selection."""
    import torch
    import miphy
    g_off, e_off, s_off = [], [], []
    go = eo = 0
    so = 3
    for it in items:
        g_off.append(go)
        e_off.append(eo)
        s_off.append(so)
        go += it["grid"].size
        eo += it["est"].size
        so += 5 * len(it["sel"]) + 1
    sc = rng.uniform(0.6, 50.0, so + 8).astype(np.float32)  # a noise variance taken from elsewhere is finite, and wrong
    for it, s in zip(items, s_off):
        sc[s + 2] = it["nv"]
    jobs = []
    for k, lo in zip(order, llr_offsets):
        it = items[k]
        j = _job(miphy, it["rnti"], it["n_id"], it["mod"], it["start"], it["nof"], it["dm"], it["type2"], it["cdm"], it["rb"], len(it["sel"]),
                 it["rows"] if not it["compact"] else 14, g_off[k], e_off[k], s_off[k], lo)
        spare = [p for p in range(4) if p not in it["sel"]]
        j["rx_ports"] = it["sel"] + spare[:1] * (4 - len(it["sel"]))
        j["ce_compact"] = int(it["compact"])
        assert j["nof_llr"] == it["exp"].size
        jobs.append(j)
    jobs = np.array(jobs, dtype=miphy.PuschDemodJob)
    total = max(lo + items[k]["exp"].size for k, lo in zip(order, llr_offsets)) + 64
    out = torch.full((total,), LLR_SENTINEL, dtype=torch.int8, device="cuda")
    g = torch.from_numpy(np.concatenate([it["grid"].reshape(-1) for it in items])).cuda()
    # (behind the last estimate: NaN for as much as a stride of 14 rows on four ports could reach, so that a wrong stride reads a wrong value)
    tail = np.full(4 * 14 * max(it["rb"].size for it in items) * 12, np.nan + 1j * np.nan, np.complex64)
    h = torch.from_numpy(np.concatenate([it["est"].reshape(-1) for it in items] + [tail])).cuda()
    ctx.pusch_demodulate_batch(torch.from_numpy(jobs.view(np.uint8)).cuda() if device_jobs else jobs, g, h, torch.from_numpy(sc).cuda(), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    used = np.zeros(total, bool)
    for n, (k, lo) in enumerate(zip(order, llr_offsets)):
        exp = items[k]["exp"]
        assert not used[lo:lo + exp.size].any()
        used[lo:lo + exp.size] = True
        bad = np.nonzero(got[lo:lo + exp.size] != exp)[0]
        assert bad.size == 0, (n, k, bad.size, bad[:8], got[lo:lo + exp.size][bad[:8]], exp[bad[:8]])
    assert np.all(got[~used] == LLR_SENTINEL), "bytes between the codewords were written"


def _offsets(sizes, pads=(3, 2, 1, 0, 6, 5, 4, 7)):
    """Codeword starts with guard bytes in between, at every residue modulo 8 in turn (odd, 2 mod 4, aligned)."""
    offs, cur = [], 0
    for n, sz in enumerate(sizes):
        cur = (cur + 7) // 8 * 8 + pads[n % len(pads)]
        offs.append(cur)
        cur += sz + 1
    return offs


@pytest.mark.parametrize("device_jobs", [False, True])
def test_port_selection_matches_oracle(ctx, device_jobs):
    """rx_ports on all three walks over the OFDM symbols: one port with the compact estimate (every request in flight at once), several
    ports with the compact estimate and the full estimate (the general walk), pi/2-BPSK. One batch; the noise variance of every job sits
    at scalars_offset + 2 of a scalars_offset of its own."""
    rng = np.random.default_rng(5100)
    rb = (rng.uniform(size=30) < 0.85).astype(np.uint8)
    rb[[0, 29]] = 1
    items = [_item(rng, 6, [2], True, 2, 0, rb, 0, 14, (2,)),
             _item(rng, 4, [3, 0], True, 1, 0, rb, 2, 12, (3, 10)),
             _item(rng, 8, [2, 0, 3, 1], True, 2, 0, rb, 0, 14, (2, 11)),
             _item(rng, 6, [1, 3, 0], False, 2, 1, rb, 0, 13, (2, 7, 11)),
             _item(rng, 1, [1], True, 2, 0, rb, 1, 9, (4,)),
             _item(rng, 2, [3], True, 1, 0, rb, 0, 14, (2,))]
    offs = _offsets([it["exp"].size for it in items])
    _run_items(ctx, items, range(len(items)), offs, device_jobs, rng)


@pytest.mark.parametrize("device_jobs", [False, True])
def test_estimates_shorter_than_a_slot(ctx, device_jobs):
    """The estimator writes first_symbol + nof_symbols rows per port: ce_nof_symbols is the stride between the ports of a full estimate."""
    rng = np.random.default_rng(5200)
    rb = np.ones(13, np.uint8)
    rb[4] = 0
    items = [_item(rng, 4, [3, 1], False, 2, 0, rb, 1, 9, (4,), ce_rows=10),
             _item(rng, 6, [1, 0, 3, 2], False, 1, 0, rb, 1, 9, (2, 7), ce_rows=10),
             _item(rng, 8, [0, 2], False, 2, 0, rb, 0, 12, (2, 11), ce_rows=12),
             _item(rng, 2, [2, 3, 1, 0], False, 2, 1, rb, 0, 12, (3,), ce_rows=12)]
    offs = _offsets([it["exp"].size for it in items])
    _run_items(ctx, items, range(len(items)), offs, device_jobs, rng)


@pytest.fixture(scope="module")
def split_items():
    """Eight transmissions of 22 PRB on a 24-PRB grid: two chunks of subcarriers, the second with 8 live lanes."""
    rng = np.random.default_rng(5300)
    rb = np.ones(24, np.uint8)
    rb[[5, 17]] = 0
    return [_item(rng, 8, [1], True, 2, 0, rb, 0, 14, (2,)),
            _item(rng, 6, [3], True, 1, 1, rb, 1, 9, (4, 8)),
            _item(rng, 4, [2, 0], True, 1, 0, rb, 2, 12, (3, 10)),
            _item(rng, 2, [0, 3], False, 3, 1, rb, 0, 13, (2,), ce_rows=14),
            _item(rng, 1, [2], True, 2, 0, rb, 1, 9, (4,)),
            _item(rng, 6, [1, 2], False, 2, 0, rb, 0, 13, (2, 7, 11), ce_rows=13),
            _item(rng, 8, [3, 1], True, 2, 1, rb, 2, 12, (2, 11)),
            _item(rng, 2, [0], True, 1, 0, rb, 0, 14, (2, 11))]


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_every_symbol_split(ctx, split_items, q, device_jobs):
    """A batch that leaves compute units idle cuts the OFDM symbols of every transmission into up to four parts, one workgroup each; a part
    starts at the data elements in front of its first symbol and may own no symbol at all (9 symbols in 4 parts). The batch sizes make
    compute units // (transmissions x 2 chunks) equal q = 1, 2, 3 and 4 with host descriptors (asserted for the chip at hand); with
    descriptors in device memory the launch is sized for the widest grid instead. Every copy of every transmission must equal the
    oracle, codewords at every alignment, the bytes between them untouched."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus // (2 * q)
    assert n >= len(split_items) and cus // (n * 2) == q, (cus, n, q)
    order = [k % len(split_items) for k in range(n)]
    offs = _offsets([split_items[k]["exp"].size for k in order])
    assert any(o % 2 for o in offs) and any(o % 4 == 2 for o in offs)
    _run_items(ctx, split_items, order, offs, device_jobs, np.random.default_rng(q))
