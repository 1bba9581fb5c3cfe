"""GPU: fused PUSCH processor entry point (estimate + demodulate + decode in one call) on slots built by the device
transmit chain: the transport blocks come back, the HARQ retransmission path works, and the results equal those of the three
entry points called one by one (each of which has its own parity tests against the oracle). Second half of the file: slots built on the
host (tests/pusch_tx.py) with the caller's own port lists, pinned to the oracle chain."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RB_ALL = lambda nprb: [(0xFFFFFFFFFFFFFFFF if nprb >= 64 * (k + 1) else ((1 << max(0, nprb - 64 * k)) - 1)) for k in range(5)]


def _build_slot(ctx, miphy, torch, nprb, mod, tbs_bits, slot, rnti, n_id, scr, snr_db, rv, seed):
    rng = np.random.default_rng(seed)
    nsc, nre = nprb * 12, nprb * 156
    G = nre * mod
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
    bg = 1 if tbs_bits > 3824 else 2
    td = np.zeros(1, dtype=miphy.PdschTbDesc)
    td[0] = (bg, rv, mod, 1, 0, nre, tb.size, 0, 0)
    cw = torch.zeros(G, dtype=torch.uint8, device="cuda")
    ctx.pdsch_encode_batch(td, torch.from_numpy(tb).cuda(), cw)
    grid = torch.zeros(14 * nsc, dtype=torch.complex64, device="cuda")
    mj = np.zeros(1, dtype=miphy.PdschModJob)
    j = mj[0]
    j["rnti"], j["n_id"], j["scaling"], j["mod"], j["port"], j["start_symbol"], j["nof_symbols"] = rnti, n_id, 1.0, mod, 0, 0, 14
    j["dmrs_type"], j["nof_cdm_groups_without_data"], j["dmrs_symbols_mask"] = 1, 2, 1 << 2
    j["grid_nof_prb"], j["bwp_start_rb"], j["bwp_size_rb"], j["nof_bits"], j["rb_mask"] = nprb, 0, nprb, G, RB_ALL(nprb)
    ctx.pdsch_modulate_batch(mj, cw, grid)
    dj = np.zeros(1, dtype=miphy.DmrsPdschJob)
    q = dj[0]
    q["slot_in_frame"], q["scrambling_id"], q["amplitude"], q["dmrs_type"], q["nof_ports"] = slot, scr, 10 ** (3 / 20), 1, 1
    q["symbols_mask"], q["grid_nof_prb"], q["rb_mask"] = 1 << 2, nprb, RB_ALL(nprb)
    ctx.dmrs_pdsch_map_batch(dj, grid)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    grid += torch.view_as_complex(torch.randn(14 * nsc, 2, device="cuda", generator=g) * (10 ** (-snr_db / 20) * 0.7071))
    return tb, bg, grid


def test_process_batch_recovers_transport_blocks_and_matches_the_separate_calls(ctx):
    import torch
    import miphy
    cases = [(273, 8, 319784, 33.0), (106, 6, 83976, 26.0), (52, 4, 20496, 21.0), (25, 2, 3848, 16.0)]  # SNRs with margin: the reference chain loses 12 % of the 16QAM blocks at 18 dB
    pdus = np.zeros(len(cases), dtype=miphy.PuschPdu)
    grids, tbs, goff, tboff, cboff = [], [], 0, 0, 0
    for i, (nprb, mod, tbs_bits, snr) in enumerate(cases):
        tb, bg, grid = _build_slot(ctx, miphy, torch, nprb, mod, tbs_bits, 7 + i, 0x4601 + i, 900 + i, 40 + i, snr, 0, 10 + i)
        p = pdus[i]
        p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, 7 + i, 0x4601 + i, 900 + i, 40 + i
        p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb.size, cboff, mod, 1, 0, 14
        p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = bg, 0, 1, [0, 1, 2, 3], 1, 6
        p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"], p["grid_offset"], p["tb_offset"] = 1 << 2, nprb, RB_ALL(nprb), goff, tboff
        grids.append(grid)
        tbs.append(tb)
        goff += grid.numel()
        tboff += tb.size
        cboff += miphy.sch_segmentation(tb.size, bg).nof_cbs
    grid_d = torch.cat(grids)
    soft = torch.full((cboff * miphy.HARQ_CB_STRIDE,), 5, dtype=torch.int8, device="cuda")
    msgs = torch.zeros(cboff * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc = torch.zeros(cboff, dtype=torch.uint8, device="cuda")
    out = torch.zeros(tboff, dtype=torch.uint8, device="cuda")
    res = torch.zeros(len(cases) * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(len(cases) * 20, dtype=torch.float32, device="cuda")
    ctx.pusch_process_batch(pdus, grid_d, soft, msgs, crc, out, res, sc)
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(miphy.PuschResult)
    o = out.cpu().numpy()
    scal = sc.cpu().numpy().reshape(len(cases), 4, 5)
    for i, tb in enumerate(tbs):
        assert r[i]["tb_crc_ok"] != 0, i
        t0 = int(pdus[i]["tb_offset"])
        assert np.array_equal(o[t0:t0 + tb.size], tb), i
        assert np.isfinite(scal[i, 0]).all() and scal[i, 0, 0] > 0 and scal[i, 0, 2] > 0  # RSRP and noise variance of port 0 are reported
    # the same through the three entry points
    for i, (nprb, mod, tbs_bits, snr) in enumerate(cases):
        nsc = nprb * 12
        cj = np.zeros(1, dtype=miphy.PuschChestJob)
        c = cj[0]
        c["numerology"], c["slot_in_frame"], c["scrambling_id"], c["scaling"] = 1, 7 + i, 40 + i, np.float32(10.0) ** np.float32(3.0 / 20.0)
        c["nof_tx_layers"], c["nof_rx_ports"], c["first_symbol"], c["nof_symbols"], c["rx_ports"] = 1, 1, 0, 14, [0, 1, 2, 3]
        c["symbols_mask"], c["grid_nof_prb"], c["rb_mask"] = 1 << 2, nprb, RB_ALL(nprb)
        ce = torch.zeros(14 * nsc, dtype=torch.complex64, device="cuda")
        s1 = torch.zeros(20, dtype=torch.float32, device="cuda")
        ctx.dmrs_pusch_estimate_batch(cj, grids[i], ce, s1)
        dq = np.zeros(1, dtype=miphy.PuschDemodJob)
        q = dq[0]
        q["rnti"], q["n_id"], q["mod"], q["nof_rx_ports"], q["start_symbol"], q["nof_symbols"] = 0x4601 + i, 900 + i, mod, 1, 0, 14
        q["dmrs_type"], q["nof_cdm_groups_without_data"], q["ce_nof_symbols"], q["rx_ports"] = 1, 2, 14, [0, 1, 2, 3]
        q["dmrs_symbols_mask"], q["grid_nof_prb"], q["rb_mask"] = 1 << 2, nprb, RB_ALL(nprb)
        q["nof_llr"] = miphy.pusch_demod_nof_llr(q)
        llr = torch.zeros(int(q["nof_llr"]), dtype=torch.int8, device="cuda")
        ctx.pusch_demodulate_batch(dq, grids[i], ce, s1, llr)
        td = np.zeros(1, dtype=miphy.PuschTbDesc)
        bg = int(pdus[i]["bg"])
        ncb = miphy.sch_segmentation(tbs[i].size, bg).nof_cbs
        td[0] = (bg, 0, mod, 1, 1, 1, 6, 0, nprb * 156, tbs[i].size, 0, 0, 0)
        so2 = torch.full((ncb * miphy.HARQ_CB_STRIDE,), 5, dtype=torch.int8, device="cuda")  # same stale content as the fused run
        ms2 = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        cr2 = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
        ou2 = torch.zeros(tbs[i].size, dtype=torch.uint8, device="cuda")
        re2 = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        ctx.pusch_decode_batch(td, llr, so2, ms2, cr2, ou2, re2)
        torch.cuda.synchronize()
        r2 = re2.cpu().numpy().view(miphy.PuschResult)[0]
        assert (r2["tb_crc_ok"], r2["iters_min"], r2["iters_max"], r2["nof_decoded"]) == (r[i]["tb_crc_ok"], r[i]["iters_min"], r[i]["iters_max"],
                                                                                      r[i]["nof_decoded"]), i
        assert np.array_equal(s1.cpu().numpy()[:5], scal[i, 0]), i
        h0 = int(pdus[i]["harq_cb_index"])
        assert torch.equal(so2, soft[h0 * miphy.HARQ_CB_STRIDE:(h0 + ncb) * miphy.HARQ_CB_STRIDE]), i  # identical HARQ soft bits


def test_retransmission_through_the_processor(ctx):
    """HARQ through the fused entry point: at 21 dB the first 64QAM R=0.85 transmission fails; redundancy versions 2, 3, 1 are combined
    in the device-resident HARQ buffers until the transport block comes out. (With one DM-RS symbol the reference's estimator caps the
    SNR at 27 dB, so most LLRs saturate and combining needs more transmissions than an ideal receiver: the oracle decoder fed with
    the same LLRs behaves identically.)"""
    import torch
    import miphy
    nprb, mod, tbs_bits, SNR = 106, 6, 83976, 21.0
    soft = msgs = crc = out = None
    oks, tb = [], None
    for t, (slot, rv) in enumerate(((3, 0), (4, 2), (5, 3), (6, 1))):
        tb, bg, grid = _build_slot(ctx, miphy, torch, nprb, mod, tbs_bits, slot, 0x1234, 77, 9, SNR, rv, 99)
        if soft is None:
            ncb = miphy.sch_segmentation(tb.size, bg).nof_cbs
            soft = torch.zeros(ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
            msgs = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
            crc = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
            out = torch.zeros(tb.size, dtype=torch.uint8, device="cuda")
        res = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        sc = torch.zeros(20, dtype=torch.float32, device="cuda")
        pd = np.zeros(1, dtype=miphy.PuschPdu)
        p = pd[0]
        p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, slot, 0x1234, 77, 9
        p["tb_bytes"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb.size, mod, 1, 0, 14
        p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = bg, rv, 1 if t == 0 else 0, [0, 1, 2, 3], 1, 6
        p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"] = 1 << 2, nprb, RB_ALL(nprb)
        ctx.pusch_process_batch(pd, grid, soft, msgs, crc, out, res, sc)
        torch.cuda.synchronize()
        oks.append(int(res.cpu().numpy().view(miphy.PuschResult)[0]["tb_crc_ok"]))
        if oks[-1]:
            break
    assert oks[0] == 0 and oks[-1] == 1, oks
    assert np.array_equal(out.cpu().numpy(), tb)


# ------------------------------------------------------------------------------------------------ slots of the host transmitter, against the oracle
# The slots come from tests/pusch_tx.py (no device code on the transmit side; tests/test_pusch_tx.py receives every one of them with the oracle
# chain alone). Two levels, as in tests/test_pusch_uci_gpu.py:
#   exact: the estimator is a floating-point kernel (1e-4 against the oracle, tests/test_chest_gpu.py), everything behind it is bit-exact. So the
#          estimator entry point is called on its own for the same jobs (ce_compact = 1: what the fused call asks for; deterministic), its row and
#          its noise variance of logical port 0 go through the oracle's demodulator and decoder, and the fused call must give exactly that.
#   chain: the oracle chain with the oracle's own estimate gives the same transport block and verdict (the PDUs have margin), and the scalars
#          of the fused call agree with the oracle's within the estimator tolerances.
import oracle_lib as O  # noqa: E402
import pusch_tx as T  # noqa: E402

STALE_SOFT, STALE_TB, SC_SENTINEL = 33, 0xEE, -77.0


def _mask_words(rb):
    m = [0] * 5
    for r in np.nonzero(rb)[0]:
        m[int(r) >> 6] |= 1 << (int(r) & 63)
    return m


def _rx_ports(sel):
    spare = [p for p in range(4) if p not in sel]  # the unused tail names a port outside the selection (NaN in the grid), never one out of range
    return list(sel) + spare[:1] * (4 - len(sel))


def _estimate_alone(ctx, entries, grid_d, grid_offs):
    """miphy_dmrs_pusch_estimate_batch for the PDUs of `entries` as one batch: per PDU (row [ports][nsc], scalars [ports][5])."""
    import torch
    import miphy
    cj = np.zeros(len(entries), dtype=miphy.PuschChestJob)
    ce_off, offs = 3, []
    for i, (e, go) in enumerate(zip(entries, grid_offs)):
        c, rb, dm = e["case"], e["rb"], e["dm"]
        j = cj[i]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = c["mu"], c["slot"], c["scr"], T.CHEST_SCALING
        j["n_scid"], j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"] = c["n_scid"], 1, len(c["ports"]), c["start"], c["nof"]
        j["rx_ports"], j["ce_compact"] = _rx_ports(c["ports"]), 1
        j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"] = sum(1 << int(l) for l in np.nonzero(dm)[0]), rb.size, _mask_words(rb)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = go, ce_off, 20 * i
        offs.append(ce_off)
        ce_off += len(c["ports"]) * rb.size * 12 + 3
    ce_d = torch.zeros(ce_off, dtype=torch.complex64, device="cuda")
    sc_d = torch.full((20 * len(entries),), SC_SENTINEL, dtype=torch.float32, device="cuda")
    ctx.dmrs_pusch_estimate_batch(cj, grid_d, ce_d, sc_d)
    torch.cuda.synchronize()
    ce, sc = ce_d.cpu().numpy(), sc_d.cpu().numpy().reshape(-1, 4, 5)
    return [(ce[o:o + len(e["case"]["ports"]) * e["rb"].size * 12].reshape(len(e["case"]["ports"]), -1), sc[i, :len(e["case"]["ports"])])
            for i, (e, o) in enumerate(zip(entries, offs))]


def _upload_grids(entries):
    import torch
    parts, offs, go = [], [], 0
    for e in entries:
        gap = np.full(7, np.nan + 1j * np.nan, np.complex64)
        parts += [gap, e["grid"].reshape(-1)]
        offs.append(go + gap.size)
        go += gap.size + e["grid"].size
    return torch.from_numpy(np.concatenate(parts)).cuda(), offs


def _exact_reference(ctx, entries, grid_d, grid_offs):
    """Per PDU what the fused call must give exactly. Advances the entries' oracle decoders (HARQ state)."""
    refs = []
    for e, (row, sc) in zip(entries, _estimate_alone(ctx, entries, grid_d, grid_offs)):
        dec = e["decoder"]
        nobs = dec.seg.nof_cbs if e["new_data"] else int((dec.cb_crc == 0).sum())
        r = T.oracle_receive(e["case"], e["grid"], e["rb"], e["dm"], e["rv"], e["new_data"], dec, ce_row=row, noise_var=sc[0, 2], want_evm=True)
        refs.append(dict(sc=sc, ok=r["ok"], tb=r["tb"], iters=r["iters"], nobs=nobs, evm=r["evm"], cb_crc=dec.cb_crc.copy(),
                         soft=dec.softbuf.reshape(dec.seg.nof_cbs, dec.seg.N).copy()))
    return refs


def _entry(case, tb, grid, rb, dm, rv=0, new_data=True, decoder=None):
    if decoder is None:
        decoder = O.OraclePuschDecoder(case["bg"], case["mod"], case["Nref"], 1, T.nof_data_re(rb, dm, case["start"], case["nof"]), tb.size)
        decoder.softbuf[:] = STALE_SOFT
    return dict(case=case, tb=tb, grid=grid, rb=rb, dm=dm, rv=rv, new_data=new_data, decoder=decoder)


def _process_and_check(ctx, entries, refs, grid_d, grid_offs, bufs, with_evm):
    """The fused call on `entries` (HARQ buffers `bufs`: soft, msgs, crc, cb index per PDU, number of slots) against the exact references."""
    import torch
    import miphy
    n = len(entries)
    soft, msgs, crc, cb_index, nslots = bufs
    pdus = np.zeros(n, dtype=miphy.PuschPdu)
    tb_offs, tboff = [], 5
    for i, (e, go) in enumerate(zip(entries, grid_offs)):
        c, rb, dm, p = e["case"], e["rb"], e["dm"], pdus[i]
        p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = c["mu"], c["slot"], c["rnti"], c["n_id"], c["scr"]
        p["Nref"], p["tb_bytes"], p["harq_cb_index"], p["n_scid"], p["mod"], p["nof_rx_ports"] = c["Nref"], e["tb"].size, cb_index[i], c["n_scid"], c["mod"], len(c["ports"])
        p["start_symbol"], p["nof_symbols"], p["bg"], p["rv"], p["new_data"], p["rx_ports"] = c["start"], c["nof"], c["bg"], e["rv"], int(e["new_data"]), _rx_ports(c["ports"])
        p["use_early_stop"], p["nof_ldpc_iterations"], p["dmrs_symbols_mask"] = 1, 6, sum(1 << int(l) for l in np.nonzero(dm)[0])
        p["grid_nof_prb"], p["rb_mask"], p["grid_offset"], p["tb_offset"] = rb.size, _mask_words(rb), go, tboff
        tb_offs.append(tboff)
        tboff += e["tb"].size + 5
    out = torch.full((tboff,), STALE_TB, dtype=torch.uint8, device="cuda")
    res = torch.full((n * miphy.PuschResult.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    sc_d = torch.full((n * 20 + 4,), SC_SENTINEL, dtype=torch.float32, device="cuda")
    evm_d = torch.full((n + 2,), -1.0, dtype=torch.float32, device="cuda")
    if with_evm:
        ctx.pusch_process_batch_ex(pdus, None, grid_d, soft, msgs, crc, out, res, sc_d, None, evm_d)
    else:
        ctx.pusch_process_batch(pdus, grid_d, soft, msgs, crc, out, res, sc_d)
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(miphy.PuschResult)
    o, scal, crc_h = out.cpu().numpy(), sc_d.cpu().numpy(), crc.cpu().numpy()
    soft_h = soft.cpu().numpy().reshape(nslots, miphy.HARQ_CB_STRIDE)
    assert np.all(scal[n * 20:] == np.float32(SC_SENTINEL))
    used_tb, used_cb = np.zeros(o.size, bool), np.zeros(nslots, bool)
    for i, (e, ref) in enumerate(zip(entries, refs)):
        name, nports, dec = e["case"]["name"], len(e["case"]["ports"]), e["decoder"]
        ncb, N = dec.seg.nof_cbs, dec.seg.N
        got = (bool(r[i]["tb_crc_ok"]), int(r[i]["iters_min"]), int(r[i]["iters_max"]), int(r[i]["nof_decoded"]), int(r[i]["nof_codeblocks_total"]))
        assert got == (ref["ok"], ref["iters"][0], ref["iters"][1], ref["nobs"], ncb), (name, got, ref["ok"], ref["iters"], ref["nobs"], ncb)
        used_tb[tb_offs[i]:tb_offs[i] + e["tb"].size] = True
        if ref["cb_crc"].all():  # (the oracle writes the transport block once every codeblock has passed its CRC)
            assert np.array_equal(o[tb_offs[i]:tb_offs[i] + e["tb"].size], ref["tb"]), name
        if ref["ok"]:
            assert np.array_equal(ref["tb"], e["tb"]), name
        h0 = cb_index[i]
        used_cb[h0:h0 + ncb] = True
        assert np.array_equal(crc_h[h0:h0 + ncb], ref["cb_crc"]), (name, crc_h[h0:h0 + ncb], ref["cb_crc"])
        for cb in range(ncb):
            bad = np.nonzero(soft_h[h0 + cb, :N] != ref["soft"][cb])[0]
            assert bad.size == 0, (name, cb, bad.size, bad[:8], soft_h[h0 + cb, bad[:8]], ref["soft"][cb, bad[:8]])
        block = scal[20 * i:20 * i + 20].reshape(4, 5)
        assert np.array_equal(block[:nports], ref["sc"]), (name, block, ref["sc"])  # the estimator on its own, same jobs
        assert np.all(block[nports:] == np.float32(SC_SENTINEL)), (name, block)    # rows of ports the PDU does not have
        if with_evm:
            e_dev = float(evm_d[i].item())
            assert abs(e_dev - ref["evm"]) <= 1e-3 * ref["evm"], (name, e_dev, ref["evm"])
    assert np.all(o[~used_tb] == STALE_TB), "bytes between the transport blocks were written"
    assert np.all(soft_h[~used_cb] == STALE_SOFT) and np.all(crc_h[~used_cb] == 1), "HARQ slots of no PDU were written"
    if with_evm:
        ev = evm_d.cpu().numpy()
        assert np.all(ev[n:] == -1.0)
    return scal[:20 * n].reshape(n, 4, 5)


def _harq_buffers(entries, gap=1):
    import torch
    import miphy
    cb_index, slot = [], gap
    for e in entries:
        cb_index.append(slot)
        slot += e["decoder"].seg.nof_cbs + gap  # an unused slot between the PDUs: it keeps its stale content
    soft = torch.full((slot * miphy.HARQ_CB_STRIDE,), STALE_SOFT, dtype=torch.int8, device="cuda")
    msgs = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc = torch.ones(slot, dtype=torch.uint8, device="cuda")
    return soft, msgs, crc, cb_index, slot


def _check_chain_level(entries, scalars, chain):
    """The oracle chain with the oracle's own estimate: same verdict and transport block (PDUs with margin); the device's scalars within the
    estimator tolerances of tests/test_chest_gpu.py: 1e-4 relative, the time alignment to one IDFT tap."""
    for i, (e, ch) in enumerate(zip(entries, chain)):
        c, nports = e["case"], len(e["case"]["ports"])
        assert ch["ok"] == c["ok"] and (not ch["ok"] or np.array_equal(ch["tb"], e["tb"])), c["name"]
        got, exp = scalars[i, :nports], ch["sc"][:, 0]
        for k in range(4):
            rel = np.abs(got[:, k] - exp[:, k]) / (np.abs(exp[:, k]) + 1e-30)
            assert rel.max() < 1e-4, (c["name"], k, got[:, k], exp[:, k])
        tap = 1.0 / (4096 * 15000.0 * (1 << c["mu"]))
        assert np.abs(got[:, 4] - exp[:, 4]).max() <= 1.01 * tap, (c["name"], got[:, 4], exp[:, 4])


@pytest.mark.parametrize("with_evm", [False, True])
def test_process_batch_on_host_built_slots_matches_the_oracle(ctx, with_evm):
    """Five PDUs in one batch: two, four, three and one receive ports taken from four-port grids in the PDU's own order, partial slots, one to
    three DM-RS symbols, numerologies 0..3, n_scid = 1, a limited buffer (Nref), both base graphs, a scattered allocation on the widest grid
    and one PDU that must fail its CRC; distinct grid, transport-block and HARQ offsets, stale HARQ content. with_evm: through
    miphy_pusch_process_batch_ex with the EVM and no UCI (EVM within 1e-3 relative of the oracle's, the bound of
    tests/test_pusch_uci_gpu.py for the same quantity)."""
    entries = [_entry(*T.build(c["name"])) for c in T.PROC_CASES]
    assert any(e["case"]["Nref"] for e in entries) and {e["case"]["bg"] for e in entries} == {1, 2} and not all(e["case"]["ok"] for e in entries)
    chain = [T.oracle_receive(e["case"], e["grid"], e["rb"], e["dm"]) for e in entries]
    grid_d, grid_offs = _upload_grids(entries)
    refs = _exact_reference(ctx, entries, grid_d, grid_offs)
    assert [r["ok"] for r in refs] == [e["case"]["ok"] for e in entries]
    scalars = _process_and_check(ctx, entries, refs, grid_d, grid_offs, _harq_buffers(entries), with_evm)
    _check_chain_level(entries, scalars, chain)


def test_retransmissions_on_host_built_slots_match_the_oracle(ctx):
    """The two-port HARQ case (rv 0, 2, 3, 1 in consecutive slots, new_data = 1, 0, 0, ...) on device-resident HARQ buffers: after every
    transmission the soft buffers, CRC flags and results are exactly the oracle decoder's; the first transmission fails, the last succeeds."""
    bufs, dec, oks = None, None, []
    for t, (slot, rv) in enumerate(T.HARQ_SEQUENCE):
        e = _entry(*T.build(T.HARQ_CASE["name"], slot, rv), rv=rv, new_data=t == 0, decoder=dec)
        dec = e["decoder"]
        if bufs is None:
            bufs = _harq_buffers([e])
        grid_d, grid_offs = _upload_grids([e])
        refs = _exact_reference(ctx, [e], grid_d, grid_offs)
        _process_and_check(ctx, [e], refs, grid_d, grid_offs, bufs, False)
        oks.append(refs[0]["ok"])
        if oks[-1]:
            break
    assert len(oks) >= 2 and not oks[0] and oks[-1], oks
