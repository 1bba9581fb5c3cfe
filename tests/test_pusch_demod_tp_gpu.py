"""GPU: miphy_pusch_demodulate_tp_batch(_ex), the fused demodulator of a transform-precoded PUSCH (DFT-s-OFDM). Its LLRs are bit-identical to
the composition of the blocks it fuses: extraction of the allocated elements on the host, miphy_channel_equalize_batch,
miphy_transform_deprecode_batch (each pinned by its own tests), the oracle's soft demapper on the de-precoded symbols and the oracle's Gold
sequence -- the device functions are shared, so the same inputs give the same bits."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
START, NOF, DMRS = 2, 12, (2, 11)  # symbols 2..13 with DM-RS on 2 and 11: ten data symbols
DATA = [l for l in range(START, START + NOF) if l not in DMRS]


def _mask_words(first, nprb):
    w = np.zeros(5, dtype=np.uint64)
    for r in range(first, first + nprb):
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def _job(miphy, grid_prb, first, nprb, mod, ports, compact, rnti, n_id, grid_off, ce_off, sc_off, llr_off):
    j = np.zeros(1, dtype=miphy.PuschDemodJob)[0]
    j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = rnti, n_id, mod, ports, START, NOF
    j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 1, 2, 14, int(compact)
    j["rx_ports"] = [0, 1, 2, 3]
    j["dmrs_symbols_mask"] = sum(1 << l for l in DMRS)
    j["grid_nof_prb"], j["rb_mask"] = grid_prb, _mask_words(first, nprb)
    j["grid_offset"], j["ce_offset"], j["scalars_offset"], j["llr_offset"] = grid_off, ce_off, sc_off, llr_off
    j["nof_llr"] = miphy.pusch_demod_nof_llr(j)
    assert j["nof_llr"] == len(DATA) * 12 * nprb * mod
    return j


def _make(rng, grid_prb, first, nprb, ports, compact):
    """Grid and estimate of one transmission; one subcarrier of the allocation has no channel on any port (an abnormal element in every symbol)."""
    nsc = grid_prb * 12
    grid = (rng.standard_normal((ports, 14, nsc)) + 1j * rng.standard_normal((ports, 14, nsc))).astype(np.complex64)
    ce = (rng.standard_normal((ports, 1 if compact else 14, nsc)) + 1j * rng.standard_normal((ports, 1 if compact else 14, nsc))).astype(np.complex64)
    ce[:, :, first * 12 + (5 * nprb) % (12 * nprb)] = 0
    return grid, ce


def _composition(ctx, items):
    """items: (grid, ce, compact, first, nprb, ports, mod, rnti, n_id, noise_var, placeholders). The stages one by one, each as one batched call.
    Returns per item (descrambled LLRs int8, de-precoded symbols [10][M], variance per symbol [10], LLRs before descrambling)."""
    import torch
    import miphy
    ej = np.zeros(len(items), dtype=miphy.EqualizerJob)
    tj = np.zeros(len(items), dtype=miphy.TransformDeprecodeJob)
    ys, hs, yoff, hoff, zoff, voff = [], [], 0, 0, 0, 0
    for i, (grid, ce, compact, first, nprb, ports, mod, rnti, n_id, nv, ph) in enumerate(items):
        M = 12 * nprb
        sub = slice(first * 12, first * 12 + M)
        y = np.stack([np.concatenate([grid[p, l, sub] for l in DATA]) for p in range(ports)])  # [port][symbol-major elements]
        h = np.stack([np.concatenate([ce[p, 0 if compact else l, sub] for l in DATA]) for p in range(ports)])
        ej[i] = (y.shape[1], ports, 1, [0, 0], nv, 1.0, yoff, hoff, zoff, zoff)
        tj[i] = (M, len(DATA), zoff, zoff, zoff, voff)
        ys.append(y.reshape(-1)), hs.append(h.reshape(-1))
        yoff += y.size
        hoff += h.size
        zoff += y.shape[1]
        voff += len(DATA)
    z = torch.zeros(zoff, dtype=torch.complex64, device="cuda")
    zv = torch.zeros(zoff, dtype=torch.float32, device="cuda")
    ctx.channel_equalize_batch(ej, torch.from_numpy(np.concatenate(ys)).cuda(), torch.from_numpy(np.concatenate(hs)).cuda(), z, zv)
    yd = torch.zeros(zoff, dtype=torch.complex64, device="cuda")
    vd = torch.zeros(voff, dtype=torch.float32, device="cuda")
    ctx.transform_deprecode_batch(tj, z, zv, yd, vd)
    torch.cuda.synchronize()
    yh, vh, zvh = yd.cpu().numpy(), vd.cpu().numpy(), zv.cpu().numpy()
    out = []
    for i, (grid, ce, compact, first, nprb, ports, mod, rnti, n_id, nv, ph) in enumerate(items):
        M, n = 12 * nprb, len(DATA) * 12 * nprb
        z0, v0 = int(tj[i]["out_symbols_offset"]), int(tj[i]["out_noise_var_offset"])
        assert np.isinf(zvh[z0:z0 + n]).sum() == len(DATA)  # the dead subcarrier, once per symbol
        sym, var = yh[z0:z0 + n], vh[v0:v0 + len(DATA)]
        raw = O.o_demodulate_soft(mod, sym, np.repeat(var, M)).astype(np.int16)
        sign = 1 - 2 * O.o_gold((rnti << 15) + n_id, 0, n * mod).astype(np.int16)
        for re in ph:  # TS 38.211 6.3.1.1: bit 1 of a placeholder element takes the chip of bit 0, the bits behind it none
            sign[re * mod + 1] = sign[re * mod]
            sign[re * mod + 2:(re + 1) * mod] = 1
        out.append(((raw * sign).astype(np.int8), sym.reshape(len(DATA), M), var, raw.astype(np.int8)))
    return out


def _fused(ctx, jobs, grids, ces, nvs, total_llr, device_jobs, ex=None, fill=99):
    """ex: None, or (placeholder array, EVM floats) for the _ex entry point. Returns (llr bytes, EVM floats or None)."""
    import torch
    import miphy
    g = torch.from_numpy(np.concatenate([x.reshape(-1) for x in grids])).cuda()
    h = torch.from_numpy(np.concatenate([x.reshape(-1) for x in ces])).cuda()
    sc = np.zeros(5 * len(nvs), dtype=np.float32)
    sc[2::5] = nvs
    out = torch.full((total_llr + 64,), fill, dtype=torch.int8, device="cuda")
    ja = np.array(jobs, dtype=miphy.PuschDemodJob)
    j = torch.from_numpy(ja.view(np.uint8)).cuda() if device_jobs else ja
    evm = None
    if ex is None:
        ctx.pusch_demodulate_tp_batch(j, g, h, torch.from_numpy(sc).cuda(), out)
    else:
        ph, nevm = ex
        ph_d = torch.from_numpy(np.asarray(ph, np.uint16).view(np.int16)).cuda() if ph is not None else None
        evm = torch.full((nevm,), -1.0, dtype=torch.float32, device="cuda") if nevm else None
        ctx.pusch_demodulate_tp_batch_ex(j, g, h, torch.from_numpy(sc).cuda(), out, ph_d, evm)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (evm.cpu().numpy() if evm is not None else None)


ALLOCATIONS = ((1, 3), (2, 7), (5, 11), (6, 1), (10, 13), (15, 4), (20, 2))  # (PRBs, first PRB) on the 24-PRB grid
MODS = (1, 2, 4, 6, 8)
PORTS = (1, 2, 4)


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("compact", [True, False])
def test_llrs_equal_the_composition(ctx, compact, device_jobs):
    """35 transmissions in one call: every allocation with every modulation, the port counts and the two codeword alignments (first LLR at an
    even and at an odd address) going round so that each modulation meets each of them; sizes mixed in the batch. Bit-identical LLRs, nothing
    written between or behind the codewords."""
    import miphy
    rng = np.random.default_rng(100 + 2 * compact + device_jobs)
    items, jobs, grids, ces, nvs, where = [], [], [], [], [], []
    goff = coff = loff = 0
    k = 0
    for a, (nprb, first) in enumerate(ALLOCATIONS):
        for m, mod in enumerate(MODS):
            ports = PORTS[(a + m) % 3]
            loff += (a + m + k) % 2  # first_llr 0 and 1
            grid, ce = _make(rng, 24, first, nprb, ports, compact)
            rnti, n_id, nv = int(rng.integers(1, 65536)), int(rng.integers(0, 1024)), float(np.float32(rng.uniform(0.01, 0.5)))
            j = _job(miphy, 24, first, nprb, mod, ports, compact, rnti, n_id, goff, coff, 5 * k, loff)
            items.append((grid, ce, compact, first, nprb, ports, mod, rnti, n_id, nv, ()))
            jobs.append(j), grids.append(grid), ces.append(ce), nvs.append(nv), where.append((loff, int(j["nof_llr"])))
            goff += grid.size
            coff += ce.size
            loff += int(j["nof_llr"]) + 3
            k += 1
    assert {(it[6], it[5]) for it in items} == {(m, p) for m in MODS for p in PORTS}
    exp = _composition(ctx, items)
    got, _ = _fused(ctx, jobs, grids, ces, nvs, loff, device_jobs)
    written = np.zeros(got.size, bool)
    for i, (o, n) in enumerate(where):
        assert np.array_equal(got[o:o + n], exp[i][0]), (i, items[i][4:7], int(np.abs(got[o:o + n].astype(int) - exp[i][0].astype(int)).max()))
        assert exp[i][0].any()
        written[o:o + n] = True
    assert np.all(got[~written] == 99)


def test_widest_allocation(ctx):
    """270 PRB in a 273-PRB grid: M = 3240 = 8 * 81 * 5, one radix-8, four radix-3 passes and one radix-5 pass, 256QAM, host job."""
    import miphy
    rng = np.random.default_rng(270)
    grid, ce = _make(rng, 273, 2, 270, 1, True)
    j = _job(miphy, 273, 2, 270, 8, 1, True, 0x4601, 900, 0, 0, 0, 0)
    exp = _composition(ctx, [(grid, ce, True, 2, 270, 1, 8, 0x4601, 900, 0.05, ())])[0][0]
    got, _ = _fused(ctx, [j], [grid], [ce], [0.05], exp.size, False)
    assert np.array_equal(got[:exp.size], exp) and np.all(got[exp.size:] == 99)


def test_a_symbol_without_a_normal_element_gives_zero_llrs(ctx):
    """A noise variance of zero makes every element abnormal: the symbol's variance is +inf and the demapper gives zero LLRs, as on CP-OFDM."""
    import miphy
    rng = np.random.default_rng(3)
    grid, ce = _make(rng, 24, 4, 5, 2, True)
    j = _job(miphy, 24, 4, 5, 4, 2, True, 1, 2, 0, 0, 0, 0)
    got, _ = _fused(ctx, [j], [grid], [ce], [0.0], int(j["nof_llr"]), False)
    assert not got[:int(j["nof_llr"])].any() and np.all(got[int(j["nof_llr"]):] == 99)


@pytest.mark.parametrize("mod,ports", [(2, 1), (4, 2), (6, 4), (8, 1), (1, 2)])
def test_placeholders_and_evm(ctx, mod, ports):
    """_ex: the LLRs do not change when EVM is asked for; with a placeholder list (mod >= 2) they carry the pattern of CP-OFDM (bit 1 with the
    chip of bit 0, the bits behind it not descrambled); the EVM sums are those of the de-precoded symbols (2e-6 relative: a tree sum against a
    sequential one), 0 on the symbols without data, and bit-equal between a batch of one and a batch of many."""
    import miphy
    rng = np.random.default_rng(40 + mod)
    nprb, first = 6, 9
    M = 12 * nprb
    n_re = len(DATA) * M
    grid, ce = _make(rng, 24, first, nprb, ports, True)
    ph = np.sort(rng.choice(n_re, 41, replace=False)).astype(np.uint16) if mod >= 2 else np.zeros(0, np.uint16)
    nv = 0.07
    plain = _composition(ctx, [(grid, ce, True, first, nprb, ports, mod, 0x1234, 77, nv, ())])[0]
    withph = _composition(ctx, [(grid, ce, True, first, nprb, ports, mod, 0x1234, 77, nv, ph)])[0]
    j = _job(miphy, 24, first, nprb, mod, ports, True, 0x1234, 77, 0, 0, 0, 1)
    j["evm_offset"] = 3
    n = int(j["nof_llr"])
    # EVM only
    got, evm = _fused(ctx, [j], [grid], [ce], [nv], n + 1, False, ex=(None, 3 + 14 + 2))
    assert np.array_equal(got[1:1 + n], plain[0]) and got[0] == 99 and np.all(got[1 + n:] == 99)
    assert np.all(evm[:3] == -1.0) and np.all(evm[17:] == -1.0)
    hard = O.nr_modulate((plain[3] <= 0).astype(np.uint8), mod).reshape(len(DATA), M)  # hard decision on the soft bits before descrambling
    for l in range(14):
        if l in DATA:
            e = float((np.abs(hard[DATA.index(l)].astype(np.complex128) - plain[1][DATA.index(l)]) ** 2).sum())
            assert abs(evm[3 + l] - e) <= 2e-6 * e + 1e-9, (l, evm[3 + l], e)
        else:
            assert evm[3 + l] == 0.0, l
    # placeholders and EVM; a batch of many gives the sums of the batch of one, bit for bit
    jp = j.copy()
    jp["placeholders_offset"], jp["nof_placeholders"] = 5, ph.size
    phs = np.concatenate([np.zeros(5, np.uint16), ph, np.zeros(3, np.uint16)])
    got1, evm1 = _fused(ctx, [jp], [grid], [ce], [nv], n + 1, False, ex=(phs, 17))
    assert np.array_equal(got1[1:1 + n], withph[0]) and np.all(got1[1 + n:] == 99)
    assert np.array_equal(evm1.view(np.uint32), evm[:17].view(np.uint32))  # (the EVM is taken before descrambling: no placeholder in it)
    many, stride = [], (n + 16) // 16 * 16
    for i in range(9):
        q = jp.copy()
        q["llr_offset"], q["evm_offset"] = 1 + i * stride, 3 + 14 * i
        many.append(q)
    gotm, evmm = _fused(ctx, many, [grid], [ce], [nv], 9 * stride, True, ex=(phs, 3 + 14 * 9))
    for i in range(9):
        assert np.array_equal(gotm[1 + i * stride:1 + i * stride + n], withph[0]), i
        assert np.array_equal(evmm[3 + 14 * i:3 + 14 * (i + 1)].view(np.uint32), evm[3:17].view(np.uint32)), i


BREAKS = [("non_contiguous", "contiguous"), ("seven_prb", "2\\^a"), ("dmrs_type_2", "type 1"), ("one_cdm_group", "two CDM groups")]


@pytest.mark.parametrize("what,message", BREAKS)
def test_rule_breaks(ctx, what, message):
    """A host job that breaks a rule of the waveform is refused by message with nothing enqueued (the good job in front of it included); the same
    job in device memory is skipped, its LLRs and EVM sums left as they were, and its neighbour served."""
    import miphy
    rng = np.random.default_rng(11)
    grid, ce = _make(rng, 24, 3, 8, 1, True)
    good = _job(miphy, 24, 3, 8, 2, 1, True, 5, 6, 0, 0, 0, 0)
    n = int(good["nof_llr"])
    bad = good.copy()
    if what == "non_contiguous":
        bad["rb_mask"] = _mask_words(3, 4) | _mask_words(8, 4)
    elif what == "seven_prb":
        bad["rb_mask"] = _mask_words(3, 7)
    elif what == "dmrs_type_2":
        bad["dmrs_type"] = 2
    else:
        bad["nof_cdm_groups_without_data"] = 1
    bad["nof_llr"] = miphy.pusch_demod_nof_llr(bad)  # (consistent with its own allocation: only the waveform's rule is broken)
    bad["llr_offset"], bad["evm_offset"] = n + 8, 14
    total = n + 8 + int(bad["nof_llr"])
    with pytest.raises(RuntimeError, match=message):
        _fused(ctx, [good, bad], [grid], [ce], [0.1], total, False)
    with pytest.raises(RuntimeError, match=message):
        _fused(ctx, [good, bad], [grid], [ce], [0.1], total, False, ex=(None, 28))
    exp = _composition(ctx, [(grid, ce, True, 3, 8, 1, 2, 5, 6, 0.1, ())])[0][0]
    for ex in (None, (None, 28)):
        got, evm = _fused(ctx, [good, bad], [grid], [ce], [0.1], total, True, ex=ex)
        assert np.array_equal(got[:n], exp) and np.all(got[n:] == 99)
        if evm is not None:
            assert np.all(evm[:14] >= 0) and np.all(evm[14:] == -1.0)
