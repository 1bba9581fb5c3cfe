"""GPU: miphy_pusch_process_layers_batch_ex -- one codeword on 1..4 layers with multiplexed UCI and the EVM behind one host call. The four
transmissions of tests/pusch_layers_uci_cases.py (shown to decode in the host chain by tests/test_pusch_layers_uci.py) and a one-layer PDU with a
two-bit HARQ-ACK, in one batch: byte for byte what the layered estimator, the _ex demodulator, the demultiplexer and the decoder give when called one
after the other on the same stream; the UCI fields decode to the sent bits with the field decoders enqueued behind the call; the one-layer PDU is
miphy_pusch_process_batch_ex; without UCI and EVM the call is miphy_pusch_process_layers_batch; a PDU that breaks a rule is refused with nothing
written."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import pusch_layers_uci_cases as U
from test_pusch_process_layers_gpu import Harq, fill_pdu

pytestmark = pytest.mark.gpu
ONE_LAYER = dict(nl=E.ONE_LAYER_CASE[0], npt=E.ONE_LAYER_CASE[1], mod=E.ONE_LAYER_CASE[2], tb_bytes=E.ONE_LAYER_CASE[3], snr_db=E.ONE_LAYER_CASE[4],
                 O=(2, 0, 0), G_re=(18, 0, 0), rvd_re=40)
NAMES = ["A", "B", "C", "D", "one"]
UCI_FRONT, UCI_GAP, UCI_SENTINEL = 7, 5, 99
_cache = {}


def transmissions():
    """-> list of (t, grid) in NAMES order, built once."""
    if not _cache:
        for name in NAMES:
            t = U.build(name, ONE_LAYER if name == "one" else None)
            _cache[name] = (t, U.chain_tx(t["c"], t["scr"], t["snr_db"])[0])
    return [_cache[name] for name in NAMES]


def batch(miphy, txs):
    """-> (PuschLayersPdu array, PuschUci array, grid, codeblocks, transport block bytes, soft bits of the UCI buffer)."""
    n = len(txs)
    pdus, uci = np.zeros(n, dtype=miphy.PuschLayersPdu), np.zeros(n, dtype=miphy.PuschUci)
    grids, goff, tboff, cboff, uoff = [], 0, 0, 0, UCI_FRONT
    for i, (t, grid) in enumerate(txs):
        c = t["c"]
        fill_pdu(miphy, pdus[i]["base"], pdus[i], (t["nl"], t["npt"], t["mod"], t["tb_bytes"] or 0, t["snr_db"], c["dmrs"]), c, 0, cboff, goff, tboff)
        u, G = uci[i], t["mc"][9]
        u["nof_harq_ack_bits"], u["nof_csi_part1_bits"], u["nof_csi_part2_bits"] = t["O"]
        u["nof_enc_harq_ack_bits"], u["nof_enc_csi_part1_bits"], u["nof_enc_csi_part2_bits"] = G
        u["nof_harq_ack_rvd"], u["has_codeword"] = t["mc"][5], int(t["tb"] is not None)
        u["harq_ack_offset"], u["csi_part1_offset"], u["csi_part2_offset"] = uoff, uoff + G[0] + UCI_GAP, uoff + G[0] + G[1] + 2 * UCI_GAP
        uoff += sum(G) + 3 * UCI_GAP
        grids.append(grid.reshape(-1))
        goff += grid.size
        if t["tb"] is not None:
            tboff += t["tb"].size
            cboff += miphy.sch_segmentation(t["tb"].size, 1).nof_cbs
    return pdus, uci, np.concatenate(grids), cboff, tboff, uoff


def separate_calls(ctx, torch, miphy, pdus, uci, txs, grid_d, h, sc_d, uci_d):
    """Layered estimator, _ex demodulator, demultiplexer and decoder one after the other on the current stream. -> the EVM sums [n][14] (device)."""
    n = pdus.size
    cj = np.zeros(n, dtype=miphy.PuschChestJob)
    dj = np.zeros(n, dtype=miphy.PuschDemodLayersJob)
    xj = np.zeros(n, dtype=miphy.UlschDemuxJob)
    td, with_tb, phs = [], [], []
    ce_off = llr_off = po = 0
    for i in range(n):
        p, nl, c, u = pdus[i]["base"], int(pdus[i]["nof_tx_layers"]), txs[i][0]["c"], uci[i]
        j = cj[i]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = p["numerology"], p["slot_in_frame"], p["dmrs_scrambling_id"], np.float32(10.0) ** np.float32(3.0 / 20.0)
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, p["nof_rx_ports"], 0, 14, p["rx_ports"]
        j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"] = 1, p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"]
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = p["grid_offset"], ce_off, 80 * i
        dj[i] = PL.demod_job(miphy, dict(c, compact=True), grid_off=int(p["grid_offset"]), ce_off=ce_off, sc_off=80 * i, llr_off=llr_off)
        nllr = int(dj[i]["base"]["nof_llr"])
        x = xj[i]
        x["mod"], x["nof_layers"], x["start_symbol"], x["nof_symbols"], x["dmrs_type"], x["nof_cdm_groups_without_data"] = p["mod"], nl, 0, 14, 1, 2
        x["dmrs_symbols_mask"], x["nof_prb"], x["nof_harq_ack_rvd"] = p["dmrs_symbols_mask"], p["grid_nof_prb"], u["nof_harq_ack_rvd"]
        for f in ("nof_enc_harq_ack_bits", "nof_enc_csi_part1_bits", "nof_enc_csi_part2_bits", "nof_harq_ack_bits", "nof_csi_part1_bits", "nof_csi_part2_bits",
                  "harq_ack_offset", "csi_part1_offset", "csi_part2_offset"):
            x[f] = u[f]
        nin, nsch = miphy.ulsch_demux_sizes(x)
        assert nin == nllr
        ph = miphy.ulsch_placeholders(x)
        dj[i]["base"]["placeholders_offset"], dj[i]["base"]["nof_placeholders"], dj[i]["base"]["evm_offset"] = po, ph.size, 14 * i
        phs.append(ph)
        po += ph.size
        x["in_offset"] = llr_off
        llr_off += (nllr + 15) & ~15
        x["sch_offset"] = llr_off
        if u["has_codeword"]:
            td.append((1, p["rv"], p["mod"], nl, p["new_data"], 1, 6, 0, nsch // int(p["mod"]), p["tb_bytes"], p["harq_cb_index"], llr_off, p["tb_offset"]))
            with_tb.append(i)
        llr_off += (nsch + 15) & ~15
        ce_off += nl * int(p["nof_rx_ports"]) * int(p["grid_nof_prb"]) * 12
    td = np.array(td, dtype=miphy.PuschTbDesc)
    ce_d = torch.zeros(ce_off, dtype=torch.complex64, device="cuda")
    llr_d = torch.zeros(llr_off, dtype=torch.int8, device="cuda")
    ph_d = torch.from_numpy(np.concatenate(phs + [np.zeros(1, np.uint16)]).view(np.int16)).cuda()
    sums_d = torch.zeros(14 * n, dtype=torch.float32, device="cuda")
    res_d = torch.zeros(max(1, td.size) * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    ctx.dmrs_pusch_estimate_layers_batch(cj, grid_d, ce_d, sc_d)
    ctx.pusch_demodulate_layers_batch_ex(dj, grid_d, ce_d, sc_d, llr_d, ph_d, sums_d)
    ctx.ulsch_demultiplex_batch(xj, llr_d, llr_d, uci_d, uci_d, uci_d)
    ctx.pusch_decode_batch(td, llr_d, h.soft, h.msgs, h.crc, h.out, res_d)
    h.res.zero_()
    r, k = h.res.view(n, -1), res_d.view(max(1, td.size), -1)
    for q, i in enumerate(with_tb):
        r[i] = k[q]
    return sums_d


@pytest.fixture(scope="module")
def processed(ctx):
    """The batch through _ex and through the separate calls, once for the tests of this module."""
    import torch
    import miphy
    txs = transmissions()
    pdus, uci, grid, ncb, tb_total, ulen = batch(miphy, txs)
    n = pdus.size
    grid_d = torch.from_numpy(grid).cuda()
    fused, apart = Harq(torch, miphy, ncb, tb_total, n), Harq(torch, miphy, ncb, tb_total, n)
    sc_f = torch.full((80 * n,), -77.0, dtype=torch.float32, device="cuda")
    uci_f = torch.full((ulen + 9,), UCI_SENTINEL, dtype=torch.int8, device="cuda")
    sc_a, uci_a = sc_f.clone(), uci_f.clone()
    evm = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    ctx.pusch_process_layers_batch_ex(pdus, uci, grid_d, *fused.args(), sc_f, uci_f, evm)
    # the field decoders behind it, no synchronisation in between
    sj, sf, pj, pf = miphy.pusch_uci_jobs(pdus["base"], uci)
    payload = torch.full((int(sum(sum(t["O"]) for t, _ in txs)) + 4,), 0xEE, dtype=torch.uint8, device="cuda")
    st_s = torch.zeros(max(1, sj.size), dtype=torch.uint8, device="cuda")
    st_p = torch.zeros(max(1, pj.size), dtype=torch.uint8, device="cuda")
    ctx.uci_decode_batch(sj, uci_f, payload, st_s)
    ctx.uci_polar_decode_batch(pj, uci_f, payload, st_p)
    sums = separate_calls(ctx, torch, miphy, pdus, uci, txs, grid_d, apart, sc_a, uci_a)
    torch.cuda.synchronize()
    return dict(txs=txs, pdus=pdus, uci=uci, grid_d=grid_d, fused=fused, apart=apart, sc_f=sc_f, sc_a=sc_a, uci_f=uci_f, uci_a=uci_a, evm=evm.cpu().numpy(),
                sums=sums.cpu().numpy().reshape(n, 14), jobs=(sj, sf, pj, pf), payload=payload.cpu().numpy(), st_s=st_s.cpu().numpy(), st_p=st_p.cpu().numpy())


def test_bytes_of_the_separate_calls(processed):
    import torch
    r = processed
    assert r["fused"].same(torch, r["apart"]), "transport blocks, result records and HARQ arrays equal the separate calls"
    assert r["sc_f"].cpu().numpy().tobytes() == r["sc_a"].cpu().numpy().tobytes()
    assert torch.equal(r["uci_f"], r["uci_a"])
    ul = r["uci_f"].cpu().numpy()
    used = np.zeros(ul.size, bool)
    for u in r["uci"]:
        for off, g in (("harq_ack_offset", "nof_enc_harq_ack_bits"), ("csi_part1_offset", "nof_enc_csi_part1_bits"), ("csi_part2_offset", "nof_enc_csi_part2_bits")):
            used[int(u[off]):int(u[off]) + int(u[g])] = True
    assert np.all(ul[~used] == UCI_SENTINEL)


def test_evm(processed):
    """evm_out against sqrt(sum of the 14 sums / (REs x L)) in float64: thirteen additions, one division and one square root in single precision,
    16 x 2^-24 relative."""
    r = processed
    for i, (t, _) in enumerate(r["txs"]):
        ref = np.sqrt(r["sums"][i].astype(np.float64).sum() / (PL.nof_re(t["c"]) * t["nl"]))
        print("EVM %s: %.6g, from the sums %.6g, relative error %.3g" % (t["name"], r["evm"][i], ref, abs(r["evm"][i] - ref) / ref))
        assert ref > 0 and abs(r["evm"][i] - ref) <= 16 * 2.0 ** -24 * ref, (t["name"], r["evm"][i], ref)


def test_fields_and_transport_blocks(processed):
    import miphy
    r = processed
    sj, sf, pj, pf = r["jobs"]
    seen = 0
    for jobs, field, status in ((sj, sf, r["st_s"]), (pj, pf, r["st_p"])):
        for j, f, st in zip(jobs, field, status):
            t = r["txs"][int(f) // 3][0]
            sent = t["payloads"][int(f) % 3]
            o = int(j["payload_offset"])
            assert st == miphy.UCI_STATUS_VALID and np.array_equal(r["payload"][o:o + sent.size], sent), (t["name"], int(f) % 3)
            seen += 1
    assert seen == sum(1 for t, _ in r["txs"] for o in t["O"] if o) and pj.size == 1
    out = r["fused"].out.cpu().numpy()
    res = r["fused"].res.cpu().numpy().view(miphy.PuschResult)
    for i, (t, _) in enumerate(r["txs"]):
        if t["tb"] is not None:
            t0 = int(r["pdus"][i]["base"]["tb_offset"])
            assert res[i]["tb_crc_ok"] == 1 and np.array_equal(out[t0:t0 + t["tb"].size], t["tb"]), t["name"]
        else:
            assert res[i].tobytes() == bytes(miphy.PuschResult.itemsize), t["name"]


def test_one_layer_pdu_is_the_one_layer_entry_point(ctx, processed):
    import torch
    import miphy
    r = processed
    k = NAMES.index("one")
    t = r["txs"][k][0]
    base, u = np.ascontiguousarray(r["pdus"]["base"][k:k + 1]), r["uci"][k:k + 1].copy()
    base[0]["harq_cb_index"], base[0]["tb_offset"] = 0, 0
    G = int(u[0]["nof_enc_harq_ack_bits"])
    u[0]["harq_ack_offset"], u[0]["csi_part1_offset"], u[0]["csi_part2_offset"] = 3, 3 + G, 3 + G
    ncb = miphy.sch_segmentation(t["tb"].size, 1).nof_cbs
    h1 = Harq(torch, miphy, ncb, t["tb"].size, 1)
    sc1 = torch.full((20,), -77.0, dtype=torch.float32, device="cuda")
    ul1 = torch.full((G + 6,), UCI_SENTINEL, dtype=torch.int8, device="cuda")
    evm1 = torch.zeros(1, dtype=torch.float32, device="cuda")
    ctx.pusch_process_batch_ex(base, u, r["grid_d"], *h1.args(), sc1, ul1, evm1)
    torch.cuda.synchronize()
    assert np.array_equal(h1.out.cpu().numpy(), t["tb"])
    isz = miphy.PuschResult.itemsize
    assert h1.res.cpu().numpy().tobytes() == r["fused"].res.cpu().numpy()[k * isz:(k + 1) * isz].tobytes()
    assert sc1.cpu().numpy().tobytes() == r["sc_f"].cpu().numpy()[80 * k:80 * k + 20].tobytes()
    o = int(r["uci"][k]["harq_ack_offset"])
    assert ul1.cpu().numpy()[3:3 + G].tobytes() == r["uci_f"].cpu().numpy()[o:o + G].tobytes()
    assert evm1.cpu().numpy().tobytes() == r["evm"][k:k + 1].tobytes()


def test_without_uci_and_evm_it_is_the_plain_call(ctx):
    """uci = None, evm = None: the bytes of miphy_pusch_process_layers_batch (the PDUs with a transport block, whose UCI is then taken for data)."""
    import torch
    import miphy
    txs = [x for x in transmissions() if x[0]["tb"] is not None]
    pdus, _, grid, ncb, tb_total, _ = batch(miphy, txs)
    grid_d = torch.from_numpy(grid).cuda()
    a, b = Harq(torch, miphy, ncb, tb_total, len(txs)), Harq(torch, miphy, ncb, tb_total, len(txs))
    sc_a = torch.full((80 * len(txs),), -77.0, dtype=torch.float32, device="cuda")
    sc_b = sc_a.clone()
    ctx.pusch_process_layers_batch_ex(pdus, None, grid_d, *a.args(), sc_a, None, None)
    ctx.pusch_process_layers_batch(pdus, grid_d, *b.args(), sc_b)
    torch.cuda.synchronize()
    assert a.same(torch, b) and sc_a.cpu().numpy().tobytes() == sc_b.cpu().numpy().tobytes()


def _too_large(uci):
    uci[1]["nof_enc_csi_part1_bits"] = 1 << 22  # more than the allocation holds: miphy_ulsch_demux_sizes fails


def _neither(uci):
    uci[1]["has_codeword"] = 0
    uci[1]["nof_harq_ack_bits"] = uci[1]["nof_csi_part1_bits"] = uci[1]["nof_csi_part2_bits"] = 0


@pytest.mark.parametrize("edit,with_uci_out", [(_too_large, True), (None, False), (_neither, True)], ids=["fields_do_not_fit", "no_uci_buffer", "neither"])
def test_rule_breaking_pdu_is_refused(ctx, edit, with_uci_out):
    import torch
    import miphy
    txs = transmissions()[:2]
    pdus, uci, grid, ncb, tb_total, ulen = batch(miphy, txs)
    if edit:
        edit(uci)
    h = Harq(torch, miphy, ncb, tb_total, 2)
    before = [x.clone() for x in h.args()]
    sc = torch.full((160,), -77.0, dtype=torch.float32, device="cuda")
    ul = torch.full((ulen,), UCI_SENTINEL, dtype=torch.int8, device="cuda")
    evm = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):
        ctx.pusch_process_layers_batch_ex(pdus, uci, torch.from_numpy(grid).cuda(), *h.args(), sc, ul if with_uci_out else None, evm)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(h.args(), before)) and bool((sc == -77.0).all())
    assert bool((ul == UCI_SENTINEL).all()) and bool((evm == -1.0).all())
