"""GPU: miphy_pusch_process_layers_tv_batch -- the layered _ex processor with the estimator that follows a channel through the slot in front and a
per-symbol estimate behind it. One batch of six PDUs: the five chain cases of tests/pusch_layers_estimator_cases.py under two_ray_gains(FD_HZ) (shown
to decode through the restatement by tests/test_pusch_tv.py, where the CFO chain fails cases 0, 1 and 3) and transmission A of
tests/pusch_layers_uci_cases.py -- multiplexed HARQ-ACK and CSI part 1 -- under the constant gains of fd = 0; the EVM is asked for. Byte for byte
what miphy_dmrs_pusch_estimate_tv_batch, miphy_pusch_demodulate_layers_batch_ex on the per-symbol estimate, the demultiplexer and the decoder give
when called one after the other; every block is recovered; miphy_pusch_process_layers_cfo_batch on the same grids fails the PDUs its restatement
fails on the CPU; a PDU that breaks a rule, or a mode that is none, is refused with nothing written."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_uci_cases as U
import pusch_tv_cases as T
from test_pusch_process_layers_gpu import Harq
from test_pusch_process_layers_uci_gpu import UCI_SENTINEL, batch
from test_pusch_tv import CFO_CHAIN_FAILS, CHAIN, FD_HZ

pytestmark = pytest.mark.gpu
CFO_SENTINEL, VAR_SENTINEL = -55.0, -33.0
_cache = []


def transmissions():
    """-> list of (t, grid): t as pusch_layers_uci_cases.build() returns it; the chain cases carry no UCI. Built once."""
    if not _cache:
        for case in CHAIN:
            c, tb, grid, est = T.chain_tx(case, FD_HZ)
            nl, npt, mod, tb_bytes, snr_db, _ = case
            no_uci = (None,) * 5 + (0,) + (None,) * 3 + ((0, 0, 0),)  # (mux case: reserved HARQ-ACK bits at 5, encoded field sizes at 9)
            _cache.append((dict(name="chain%d" % len(_cache), nl=nl, npt=npt, mod=mod, tb_bytes=tb_bytes, snr_db=snr_db, c=c, O=(0, 0, 0), mc=no_uci, tb=tb, payloads=[]),
                           grid))
        t = U.build("A")
        grid, est = U.chain_tx(t["c"], t["scr"], t["snr_db"])
        _cache.append((t, T.apply_gains(grid, T.two_ray_gains(0.0, est[0], est[1], t["npt"]))))
    return _cache


def separate_calls(ctx, torch, miphy, mode, pdus, uci, txs, grid_d, h, sc_d, uci_d, cfo_d, var_d):
    """The new estimator, the _ex demodulator on the per-symbol estimate, the demultiplexer (PDUs with UCI) and the decoder one after the other on the
    current stream. -> the EVM sums [n][14] (device)."""
    n = pdus.size
    cj = np.zeros(n, dtype=miphy.PuschChestTvJob)
    dj = np.zeros(n, dtype=miphy.PuschDemodLayersJob)
    xj, td, phs = [], [], []
    ce_off = llr_off = po = 0
    for i in range(n):
        p, nl, c, u = pdus[i]["base"], int(pdus[i]["nof_tx_layers"]), txs[i][0]["c"], uci[i]
        j = cj[i]["base"]["base"]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = p["numerology"], p["slot_in_frame"], p["dmrs_scrambling_id"], np.float32(10.0) ** np.float32(3.0 / 20.0)
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, p["nof_rx_ports"], 0, 14, p["rx_ports"]
        j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"] = 0, p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"]
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = p["grid_offset"], ce_off, 80 * i
        cj[i]["base"]["cfo_offset"], cj[i]["var_offset"], cj[i]["time_mode"] = 2 * i, 16 * i, mode
        dj[i] = PL.demod_job(miphy, dict(c, compact=False), grid_off=int(p["grid_offset"]), ce_off=ce_off, sc_off=80 * i, llr_off=llr_off)
        assert dj[i]["base"]["ce_nof_symbols"] == 14 and dj[i]["base"]["ce_compact"] == 0
        nllr = nsch = int(dj[i]["base"]["nof_llr"])
        dj[i]["base"]["evm_offset"] = 14 * i
        cw_off = llr_off
        llr_off += (nllr + 15) & ~15
        sch_off = cw_off
        if int(u["nof_harq_ack_bits"]) + int(u["nof_csi_part1_bits"]) + int(u["nof_csi_part2_bits"]):
            x = np.zeros(1, dtype=miphy.UlschDemuxJob)[0]
            x["mod"], x["nof_layers"], x["start_symbol"], x["nof_symbols"], x["dmrs_type"], x["nof_cdm_groups_without_data"] = p["mod"], nl, 0, 14, 1, 2
            x["dmrs_symbols_mask"], x["nof_prb"], x["nof_harq_ack_rvd"] = p["dmrs_symbols_mask"], p["grid_nof_prb"], u["nof_harq_ack_rvd"]
            for f in ("nof_enc_harq_ack_bits", "nof_enc_csi_part1_bits", "nof_enc_csi_part2_bits", "nof_harq_ack_bits", "nof_csi_part1_bits", "nof_csi_part2_bits",
                      "harq_ack_offset", "csi_part1_offset", "csi_part2_offset"):
                x[f] = u[f]
            nin, nsch = miphy.ulsch_demux_sizes(x)
            assert nin == nllr
            ph = miphy.ulsch_placeholders(x)
            dj[i]["base"]["placeholders_offset"], dj[i]["base"]["nof_placeholders"] = po, ph.size
            phs.append(ph)
            po += ph.size
            x["in_offset"], x["sch_offset"] = cw_off, llr_off
            sch_off = llr_off
            llr_off += (nsch + 15) & ~15
            xj.append(x)
        td.append((1, p["rv"], p["mod"], nl, p["new_data"], 1, 6, 0, nsch // int(p["mod"]), p["tb_bytes"], p["harq_cb_index"], sch_off, p["tb_offset"]))
        ce_off += nl * int(p["nof_rx_ports"]) * 14 * int(p["grid_nof_prb"]) * 12
    td, xa = np.array(td, dtype=miphy.PuschTbDesc), np.zeros(len(xj), dtype=miphy.UlschDemuxJob)
    for k, x in enumerate(xj):
        xa[k] = x
    ce_d = torch.zeros(ce_off, dtype=torch.complex64, device="cuda")
    llr_d = torch.zeros(llr_off, dtype=torch.int8, device="cuda")
    ph_d = torch.from_numpy(np.concatenate(phs + [np.zeros(1, np.uint16)]).view(np.int16)).cuda()
    sums_d = torch.zeros(14 * n, dtype=torch.float32, device="cuda")
    ctx.dmrs_pusch_estimate_tv_batch(cj, grid_d, ce_d, sc_d, cfo_d, var_d)
    ctx.pusch_demodulate_layers_batch_ex(dj, grid_d, ce_d, sc_d, llr_d, ph_d, sums_d)
    ctx.ulsch_demultiplex_batch(xa, llr_d, llr_d, uci_d, uci_d, uci_d)
    ctx.pusch_decode_batch(td, llr_d, *h.args())
    return sums_d


@pytest.fixture(scope="module")
def processed(ctx):
    """The batch through the new processor (INTERPOLATE, and LINE on its own), through the separate calls and through the CFO processor, once."""
    import torch
    import miphy
    txs = transmissions()
    pdus, uci, grid, ncb, tb_total, ulen = batch(miphy, txs)
    n = pdus.size
    grid_d = torch.from_numpy(grid).cuda()
    fused, apart, plain, line = (Harq(torch, miphy, ncb, tb_total, n) for _ in range(4))
    sc_f = torch.full((80 * n,), -77.0, dtype=torch.float32, device="cuda")
    uci_f = torch.full((ulen + 9,), UCI_SENTINEL, dtype=torch.int8, device="cuda")
    cfo_f = torch.full((2 * n + 3,), CFO_SENTINEL, dtype=torch.float32, device="cuda")
    var_f = torch.full((16 * n + 3,), VAR_SENTINEL, dtype=torch.float32, device="cuda")
    sc_a, uci_a, cfo_a, var_a, sc_p, uci_p, cfo_p = sc_f.clone(), uci_f.clone(), cfo_f.clone(), var_f.clone(), sc_f.clone(), uci_f.clone(), cfo_f.clone()
    sc_l, uci_l, cfo_l, var_l = sc_f.clone(), uci_f.clone(), cfo_f.clone(), var_f.clone()
    evm = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    evm_p, evm_l = evm.clone(), evm.clone()
    ctx.pusch_process_layers_tv_batch(pdus, uci, grid_d, *fused.args(), sc_f, uci_f, evm, cfo_f, miphy.TIME_INTERPOLATE, var_f)
    sums = separate_calls(ctx, torch, miphy, miphy.TIME_INTERPOLATE, pdus, uci, txs, grid_d, apart, sc_a, uci_a, cfo_a, var_a)
    ctx.pusch_process_layers_cfo_batch(pdus, uci, grid_d, *plain.args(), sc_p, uci_p, evm_p, cfo_p)
    ctx.pusch_process_layers_tv_batch(pdus, uci, grid_d, *line.args(), sc_l, uci_l, evm_l, cfo_l, miphy.TIME_LINE, var_l)
    torch.cuda.synchronize()
    return dict(txs=txs, pdus=pdus, uci=uci, fused=fused, apart=apart, plain=plain, line=line, sc_f=sc_f, sc_a=sc_a, uci_f=uci_f, uci_a=uci_a, cfo_f=cfo_f.cpu().numpy(),
                cfo_a=cfo_a.cpu().numpy(), var_f=var_f.cpu().numpy(), var_a=var_a.cpu().numpy(), evm=evm.cpu().numpy(), sums=sums.cpu().numpy().reshape(n, 14))


def test_bytes_of_the_separate_calls(processed):
    import torch
    r = processed
    assert r["fused"].same(torch, r["apart"]), "transport blocks, result records and HARQ arrays equal the separate calls"
    assert r["sc_f"].cpu().numpy().tobytes() == r["sc_a"].cpu().numpy().tobytes()
    assert torch.equal(r["uci_f"], r["uci_a"]) and not bool((r["uci_f"] == UCI_SENTINEL).all())
    assert r["cfo_f"].tobytes() == r["cfo_a"].tobytes() and r["var_f"].tobytes() == r["var_a"].tobytes()
    n = len(r["txs"])
    assert np.all(r["cfo_f"][2 * n:] == np.float32(CFO_SENTINEL)) and np.all(r["cfo_f"][:2 * n] != np.float32(CFO_SENTINEL))
    for i, (t, _) in enumerate(r["txs"]):  # var_out: [port][layer] of the PDU, the rest of its sixteen untouched
        k = t["nl"] * t["npt"]
        assert np.all(r["var_f"][16 * i:16 * i + k] >= 0) and np.all(r["var_f"][16 * i + k:16 * (i + 1)] == np.float32(VAR_SENTINEL)), t["name"]
    assert np.all(r["var_f"][16 * n:] == np.float32(VAR_SENTINEL))


def test_evm(processed):
    """evm_out against sqrt(sum of the demodulator's 14 sums / (REs x L)) in float64, as tests/test_pusch_process_layers_uci_gpu.py: thirteen additions,
    one division and one square root in single precision, 16 x 2^-24 relative."""
    r = processed
    for i, (t, _) in enumerate(r["txs"]):
        ref = np.sqrt(r["sums"][i].astype(np.float64).sum() / (PL.nof_re(t["c"]) * t["nl"]))
        print("EVM %s: %.6g, from the sums %.6g" % (t["name"], r["evm"][i], ref))
        assert ref > 0 and abs(r["evm"][i] - ref) <= 16 * 2.0 ** -24 * ref, (t["name"], r["evm"][i], ref)


def test_every_block_is_recovered(processed):
    """INTERPOLATE recovers all six; LINE is reported (on the CPU it decodes the five chain cases at FD_HZ too)."""
    import miphy
    r = processed
    out = r["fused"].out.cpu().numpy()
    res = r["fused"].res.cpu().numpy().view(miphy.PuschResult)
    res_l = r["line"].res.cpu().numpy().view(miphy.PuschResult)
    for i, (t, _) in enumerate(r["txs"]):
        t0 = int(r["pdus"][i]["base"]["tb_offset"])
        k = t["nl"] * t["npt"]
        print("%s: cfo_hz %.3f, rho %.4f, largest var %.4f, crc %d (LINE: crc %d)"
              % (t["name"], r["cfo_f"][2 * i], r["cfo_f"][2 * i + 1], r["var_f"][16 * i:16 * i + k].max(), res[i]["tb_crc_ok"], res_l[i]["tb_crc_ok"]))
        assert res[i]["tb_crc_ok"] == 1 and np.array_equal(out[t0:t0 + t["tb"].size], t["tb"]), t["name"]


def test_the_cfo_processor_fails_what_its_restatement_fails(processed):
    """miphy_pusch_process_layers_cfo_batch on the same grids: a CRC failure for the chain cases the CFO chain fails on the CPU (tests/test_pusch_tv.py),
    the others and the PDU with constant gains pass."""
    import miphy
    r = processed
    res = r["plain"].res.cpu().numpy().view(miphy.PuschResult)
    assert [int(x["tb_crc_ok"]) for x in res] == [0 if k in CFO_CHAIN_FAILS else 1 for k in range(len(CHAIN))] + [1]


def _five_layers(pdus, uci):
    pdus[1]["nof_tx_layers"] = 5
    return 1


def _no_dmrs(pdus, uci):
    pdus[1]["base"]["dmrs_symbols_mask"] = 0
    return 1


def _uci_does_not_fit(pdus, uci):
    uci[5]["nof_enc_csi_part1_bits"] = 1 << 22
    return 1


def _no_mode(pdus, uci):
    return 0


def _mode_three(pdus, uci):
    return 3


@pytest.mark.parametrize("edit", [_five_layers, _no_dmrs, _uci_does_not_fit, _no_mode, _mode_three])
def test_rule_breaking_pdu_or_mode_is_refused(ctx, edit):
    import torch
    import miphy
    txs = transmissions()
    pdus, uci, grid, ncb, tb_total, ulen = batch(miphy, txs)
    mode = edit(pdus, uci)
    n = pdus.size
    h = Harq(torch, miphy, ncb, tb_total, n)
    before = [x.clone() for x in h.args()]
    sc = torch.full((80 * n,), -77.0, dtype=torch.float32, device="cuda")
    ul = torch.full((ulen,), UCI_SENTINEL, dtype=torch.int8, device="cuda")
    evm = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    cfo = torch.full((2 * n,), CFO_SENTINEL, dtype=torch.float32, device="cuda")
    var = torch.full((16 * n,), VAR_SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="miphy error -1"):
        ctx.pusch_process_layers_tv_batch(pdus, uci, torch.from_numpy(grid).cuda(), *h.args(), sc, ul, evm, cfo, mode, var)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(h.args(), before)) and bool((sc == -77.0).all())
    assert bool((ul == UCI_SENTINEL).all()) and bool((evm == -1.0).all()) and bool((cfo == CFO_SENTINEL).all()) and bool((var == VAR_SENTINEL).all())
