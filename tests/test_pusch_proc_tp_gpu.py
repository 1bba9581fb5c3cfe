"""GPU: miphy_pusch_process_tp_batch(_ex), the fused processor of a transform-precoded PUSCH (DFT-s-OFDM), on the slots of tests/pusch_tp_tx.py
(built on the host from TS 38.211; tests/test_pusch_tp.py shows that the restated receiver decodes every one): every transport block comes back
with its CRC, the multiplexed UCI fields decode to the bits that were sent, and the bytes are those of the stages called one by one."""
import numpy as np
import pytest

import pusch_tp_tx as T
import uci_short_block as U

pytestmark = pytest.mark.gpu


def _mask_words(first, nprb):
    w = np.zeros(5, dtype=np.uint64)
    for r in range(first, first + nprb):
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def _batch(miphy):
    """PDUs, UCI records and the concatenated grids of every case of TP_CASES."""
    built = [T.build(c["name"]) for c in T.TP_CASES]
    pdus = np.zeros(len(built), dtype=miphy.PuschTpPdu)
    uci = np.zeros(len(built), dtype=miphy.PuschUci)
    uci["has_codeword"] = 1
    goff = tboff = cboff = uoff = 0
    for i, (c, tb, grid, rb, dm, u, ucase, ph) in enumerate(built):
        p = pdus[i]["base"]
        p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = c["mu"], c["slot"], c["rnti"], c["n_id"], c["scr"]
        p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb.size, cboff, c["mod"], len(c["ports"]), 0, 14
        p["bg"], p["rv"], p["new_data"], p["use_early_stop"], p["nof_ldpc_iterations"] = c["bg"], 0, 1, 1, 6
        p["rx_ports"] = list(c["ports"]) + [0] * (4 - len(c["ports"]))
        p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"] = sum(1 << l for l in c["dmrs"]), c["nprb_grid"], _mask_words(c["first"], c["nprb"])
        p["grid_offset"], p["tb_offset"] = goff, tboff
        pdus[i]["hopping"] = c["hopping"]
        if u:
            G = [g * c["mod"] for g in u["G_re"]]
            q = uci[i]
            q["nof_harq_ack_bits"], q["nof_csi_part1_bits"], q["nof_csi_part2_bits"] = u["O"]
            q["nof_enc_harq_ack_bits"], q["nof_enc_csi_part1_bits"], q["nof_enc_csi_part2_bits"] = G
            q["nof_harq_ack_rvd"] = u["rvd_re"] * c["mod"]
            q["harq_ack_offset"], q["csi_part1_offset"], q["csi_part2_offset"] = uoff + 3, uoff + 3 + G[0] + 1, uoff + 3 + G[0] + 1 + G[1] + 2
            uoff += 3 + sum(G) + 3 + 8
        goff += grid.size
        tboff += tb.size
        cboff += miphy.sch_segmentation(tb.size, c["bg"]).nof_cbs
    return built, pdus, uci, np.concatenate([b[2].reshape(-1) for b in built]), tboff, cboff, max(uoff, 8)


def _buffers(torch, miphy, n, tboff, cboff, uoff):
    return dict(soft=torch.full((cboff * miphy.HARQ_CB_STRIDE,), 5, dtype=torch.int8, device="cuda"),
                msgs=torch.zeros(cboff * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda"), crc=torch.zeros(cboff, dtype=torch.uint8, device="cuda"),
                out=torch.zeros(tboff, dtype=torch.uint8, device="cuda"), res=torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda"),
                sc=torch.full((n * 20,), -3.0, dtype=torch.float32, device="cuda"), ul=torch.full((uoff,), 77, dtype=torch.int8, device="cuda"),
                evm=torch.full((n,), -1.0, dtype=torch.float32, device="cuda"))


def test_transport_blocks_uci_and_the_stages_one_by_one(ctx):
    import torch
    import miphy
    built, pdus, uci, grid, tboff, cboff, uoff = _batch(miphy)
    n = len(built)
    g = torch.from_numpy(grid).cuda()
    B = _buffers(torch, miphy, n, tboff, cboff, uoff)
    ctx.pusch_process_tp_batch_ex(pdus, uci, g, B["soft"], B["msgs"], B["crc"], B["out"], B["res"], B["sc"], B["ul"], B["evm"])
    # the UCI fields behind it, on the same stream
    jobs, field = miphy.pusch_uci_field_jobs(np.ascontiguousarray(pdus["base"]), uci)
    pay = torch.full((16 * max(len(jobs), 1),), 0xAA, dtype=torch.uint8, device="cuda")
    st = torch.full((max(len(jobs), 1),), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.uci_decode_batch(jobs, B["ul"], pay, st)
    torch.cuda.synchronize()
    r = B["res"].cpu().numpy().view(miphy.PuschResult)
    o, evm, scal = B["out"].cpu().numpy(), B["evm"].cpu().numpy(), B["sc"].cpu().numpy().reshape(n, 4, 5)
    for i, (c, tb, *_rest) in enumerate(built):
        t0 = int(pdus[i]["base"]["tb_offset"])
        assert r[i]["tb_crc_ok"] != 0, c["name"]
        assert np.array_equal(o[t0:t0 + tb.size], tb), c["name"]
        np_ = len(c["ports"])
        assert np.isfinite(scal[i, :np_]).all() and np.all(scal[i, :np_, 0] > 0) and np.all(scal[i, np_:] == -3.0), c["name"]
        assert 0 < evm[i] < 1.0, (c["name"], evm[i])
    # UCI: the sent bits
    k = 0
    payh, sth = pay.cpu().numpy(), st.cpu().numpy()
    for i, (c, tb, _g, _rb, _dm, u, ucase, ph) in enumerate(built):
        if not u:
            continue
        for f, (nb, m) in enumerate(zip(u["O"], u["msgs"])):
            if nb:
                off = int(jobs[k]["payload_offset"])
                assert np.array_equal(payh[off:off + nb], m), (c["name"], f)
                assert nb <= 2 or sth[k] == U.STATUS_VALID
                k += 1
    assert k == len(jobs) and k > 0

    # ---- the same through the stages, one PDU at a time
    ulh, softh = B["ul"].cpu().numpy(), B["soft"]
    plain = _buffers(torch, miphy, n, tboff, cboff, uoff)
    no_uci = [i for i in range(n) if not built[i][5]]
    ctx.pusch_process_tp_batch(pdus[no_uci], g, plain["soft"], plain["msgs"], plain["crc"], plain["out"], plain["res"], plain["sc"])
    torch.cuda.synchronize()
    po, pr = plain["out"].cpu().numpy(), plain["res"].cpu().numpy().view(miphy.PuschResult)
    for k, i in enumerate(no_uci):  # the plain entry point on the PDUs without UCI: the same transport blocks and results
        t0 = int(pdus[i]["base"]["tb_offset"])
        assert np.array_equal(po[t0:t0 + built[i][1].size], built[i][1]) and pr[k].tobytes() == r[i].tobytes(), built[i][0]["name"]
    for i, (c, tb, _g, rb, dm, u, ucase, ph) in enumerate(built):
        p = pdus[i]["base"]
        nsc, np_ = c["nprb_grid"] * 12, len(c["ports"])
        cj = np.zeros(1, dtype=miphy.PuschChestTpJob)
        b = cj[0]["base"]
        b["numerology"], b["slot_in_frame"], b["scrambling_id"], b["scaling"] = c["mu"], c["slot"], c["scr"], np.float32(10.0) ** np.float32(3.0 / 20.0)
        b["nof_tx_layers"], b["nof_rx_ports"], b["first_symbol"], b["nof_symbols"], b["rx_ports"], b["ce_compact"] = 1, np_, 0, 14, p["rx_ports"], 1
        b["symbols_mask"], b["grid_nof_prb"], b["rb_mask"], b["grid_offset"] = p["dmrs_symbols_mask"], c["nprb_grid"], p["rb_mask"], p["grid_offset"]
        cj[0]["hopping"] = c["hopping"]
        ce = torch.zeros(np_ * nsc, dtype=torch.complex64, device="cuda")
        s1 = torch.full((20,), -3.0, dtype=torch.float32, device="cuda")
        ctx.dmrs_pusch_estimate_tp_batch(cj, g, ce, s1)
        dq = np.zeros(1, dtype=miphy.PuschDemodJob)
        q = dq[0]
        q["rnti"], q["n_id"], q["mod"], q["nof_rx_ports"], q["start_symbol"], q["nof_symbols"] = c["rnti"], c["n_id"], c["mod"], np_, 0, 14
        q["dmrs_type"], q["nof_cdm_groups_without_data"], q["ce_nof_symbols"], q["ce_compact"], q["rx_ports"] = 1, 2, 14, 1, p["rx_ports"]
        q["dmrs_symbols_mask"], q["grid_nof_prb"], q["rb_mask"], q["grid_offset"] = p["dmrs_symbols_mask"], c["nprb_grid"], p["rb_mask"], p["grid_offset"]
        q["nof_llr"] = miphy.pusch_demod_nof_llr(q)
        nre = int(q["nof_llr"]) // c["mod"]
        ph_d = None
        xj = None
        if u:
            xj = np.zeros(1, dtype=miphy.UlschDemuxJob)
            x = xj[0]
            x["mod"], x["nof_layers"], x["start_symbol"], x["nof_symbols"], x["dmrs_type"], x["nof_cdm_groups_without_data"] = c["mod"], 1, 0, 14, 1, 2
            x["dmrs_symbols_mask"], x["nof_prb"], x["nof_harq_ack_rvd"] = p["dmrs_symbols_mask"], c["nprb"], uci[i]["nof_harq_ack_rvd"]
            for k2 in ("nof_enc_harq_ack_bits", "nof_enc_csi_part1_bits", "nof_enc_csi_part2_bits", "nof_harq_ack_bits", "nof_csi_part1_bits",
                       "nof_csi_part2_bits", "harq_ack_offset", "csi_part1_offset", "csi_part2_offset"):
                x[k2] = uci[i][k2]
            phl = miphy.ulsch_placeholders(x)
            assert np.array_equal(phl, np.asarray(ph, np.uint16))
            q["nof_placeholders"] = phl.size
            ph_d = torch.from_numpy(np.concatenate([phl, np.zeros(1, np.uint16)]).view(np.int16)).cuda()
        llr = torch.zeros(2 * int(q["nof_llr"]) + 32, dtype=torch.int8, device="cuda")
        es = torch.zeros(14, dtype=torch.float32, device="cuda")
        ctx.pusch_demodulate_tp_batch_ex(dq, g, ce, s1, llr, ph_d, es)
        nof_sch, sch_off = int(q["nof_llr"]), 0
        if u:
            nin, nof_sch = miphy.ulsch_demux_sizes(xj[0])
            assert nin == int(q["nof_llr"])
            sch_off = (nin + 15) // 16 * 16
            xj[0]["in_offset"], xj[0]["sch_offset"] = 0, sch_off
            ul2 = torch.full((uoff,), 77, dtype=torch.int8, device="cuda")
            ctx.ulsch_demultiplex_batch(xj, llr, llr, ul2, ul2, ul2)
        ncb = miphy.sch_segmentation(tb.size, c["bg"]).nof_cbs
        td = np.zeros(1, dtype=miphy.PuschTbDesc)
        td[0] = (c["bg"], 0, c["mod"], 1, 1, 1, 6, 0, nof_sch // c["mod"], tb.size, 0, sch_off, 0)
        so2 = torch.full((ncb * miphy.HARQ_CB_STRIDE,), 5, dtype=torch.int8, device="cuda")
        ms2 = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        cr2 = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
        ou2 = torch.zeros(tb.size, dtype=torch.uint8, device="cuda")
        re2 = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        ctx.pusch_decode_batch(td, llr, so2, ms2, cr2, ou2, re2)
        torch.cuda.synchronize()
        r2 = re2.cpu().numpy().view(miphy.PuschResult)[0]
        assert r2.tobytes() == r[i].tobytes(), c["name"]
        assert np.array_equal(ou2.cpu().numpy(), tb), c["name"]
        assert np.array_equal(s1.cpu().numpy().view(np.uint32), scal[i].reshape(-1).view(np.uint32)), c["name"]
        h0 = int(p["harq_cb_index"])
        assert torch.equal(so2, softh[h0 * miphy.HARQ_CB_STRIDE:(h0 + ncb) * miphy.HARQ_CB_STRIDE]), c["name"]  # identical HARQ soft bits: identical LLRs
        e2 = np.float32(np.sqrt(np.float32(es.cpu().numpy().sum(dtype=np.float32)) / np.float32(nre)))
        assert abs(float(e2) - float(evm[i])) <= 1e-6 * float(evm[i]), (c["name"], e2, evm[i])
        if u:
            assert np.array_equal(ul2.cpu().numpy(), ulh), c["name"]


def test_rule_breaks_are_refused_before_anything_runs(ctx):
    """Seven PRB, a gap in the allocation, n_scid = 1, an unknown hopping mode: MIPHY_EINVAL by message; 4 PRB: MIPHY_EUNSUPP (no DM-RS table).
    Nothing is enqueued: the outputs keep their bytes."""
    import torch
    import miphy
    built, pdus, uci, grid, tboff, cboff, uoff = _batch(miphy)
    g = torch.from_numpy(grid).cuda()
    for what, message in (("seven", "2\\^a"), ("gap", "contiguous"), ("n_scid", "n_ID"), ("hopping", "hopping"), ("four", "Tables")):
        bad = pdus.copy()
        b = bad[3]["base"]
        if what == "seven":
            b["rb_mask"] = _mask_words(1, 7)
        elif what == "gap":
            b["rb_mask"] = _mask_words(1, 2) | _mask_words(5, 3)
        elif what == "four":
            b["rb_mask"] = _mask_words(1, 4)
        elif what == "n_scid":
            b["n_scid"] = 1
        else:
            bad[3]["hopping"] = 3
        B = _buffers(torch, miphy, len(built), tboff, cboff, uoff)
        with pytest.raises(RuntimeError, match=message):
            ctx.pusch_process_tp_batch_ex(bad, uci, g, B["soft"], B["msgs"], B["crc"], B["out"], B["res"], B["sc"], B["ul"], B["evm"])
        torch.cuda.synchronize()
        assert not B["out"].any() and not B["res"].any() and bool((B["sc"] == -3.0).all()) and bool((B["evm"] == -1.0).all()) and bool((B["ul"] == 77).all())
