"""GPU: miphy_pusch_process_layers_batch -- the layered estimator, the layered demodulator and the decoder behind one host call. The chain cases of
tests/pusch_layers_estimator_cases.py (shown to decode in the host chain by tests/test_pusch_layers_estimator.py) come back as their transport blocks,
byte for byte what the three entry points give when called one after the other on the same stream; a PDU on one layer gives the bytes of
miphy_pusch_process_batch; a retransmission combines in the HARQ arrays; a PDU that breaks a rule is refused with nothing written."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

pytestmark = pytest.mark.gpu
ONE_LAYER = E.ONE_LAYER_CASE
_tx = {}


def tx(case, rv=0):
    if (case, rv) not in _tx:
        _tx[(case, rv)] = E.chain_tx(*case, rv=rv)
    return _tx[(case, rv)]


def fill_pdu(miphy, p, lp, case, c, rv, cb_index, grid_off, tb_off):
    nl, npt, mod, tb_bytes, _, dmrs = case
    rb, dm = PL.masks(c)
    p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, E.SLOT, c["rnti"], c["n_id"], E.SCR
    p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb_bytes, cb_index, mod, npt, 0, 14
    p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = 1, rv, int(rv == 0), [0, 1, 2, 3], 1, 6
    p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"] = sum(1 << int(s) for s in np.nonzero(dm)[0]), rb.size, PL.mask_words(rb)
    p["grid_offset"], p["tb_offset"] = grid_off, tb_off
    if lp is not None:
        lp["nof_tx_layers"] = nl


class Harq:
    def __init__(self, torch, miphy, ncb, tb_total, n):
        self.soft = torch.full((ncb * miphy.HARQ_CB_STRIDE,), 5, dtype=torch.int8, device="cuda")
        self.msgs = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        self.crc = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
        self.out = torch.full((tb_total,), 0xEE, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")

    def args(self):
        return self.soft, self.msgs, self.crc, self.out, self.res

    def same(self, torch, other):
        return all(torch.equal(a, b) for a, b in zip(self.args(), other.args()))


def batch(miphy, cases, rvs):
    """-> (PuschLayersPdu array, grid, transport blocks, codeblocks, PL cases)."""
    pdus = np.zeros(len(cases), dtype=miphy.PuschLayersPdu)
    grids, tbs, cs, goff, tboff, cboff = [], [], [], 0, 0, 0
    for i, (case, rv) in enumerate(zip(cases, rvs)):
        c, tb, grid, _ = tx(case, rv)
        fill_pdu(miphy, pdus[i]["base"], pdus[i], case, c, rv, cboff, goff, tboff)
        grids.append(grid.reshape(-1))
        tbs.append(tb)
        cs.append(c)
        goff += grid.size
        tboff += tb.size
        cboff += miphy.sch_segmentation(tb.size, 1).nof_cbs
    return pdus, np.concatenate(grids), tbs, cboff, cs


def separate_calls(ctx, torch, miphy, pdus, cs, grid_d, h, sc_d):
    """The three entry points one after the other on the current stream, on the layouts the processor uses."""
    n = pdus.size
    cj = np.zeros(n, dtype=miphy.PuschChestJob)
    dj = np.zeros(n, dtype=miphy.PuschDemodLayersJob)
    td = np.zeros(n, dtype=miphy.PuschTbDesc)
    ce_off = llr_off = 0
    for i in range(n):
        p, nl, c = pdus[i]["base"], int(pdus[i]["nof_tx_layers"]), cs[i]
        j = cj[i]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = p["numerology"], p["slot_in_frame"], p["dmrs_scrambling_id"], np.float32(10.0) ** np.float32(3.0 / 20.0)
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, p["nof_rx_ports"], 0, 14, p["rx_ports"]
        j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"] = 1, p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"]
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = p["grid_offset"], ce_off, 80 * i
        dj[i] = PL.demod_job(miphy, dict(c, compact=True), grid_off=int(p["grid_offset"]), ce_off=ce_off, sc_off=80 * i, llr_off=llr_off)
        nllr = int(dj[i]["base"]["nof_llr"])
        td[i] = (1, p["rv"], p["mod"], nl, p["new_data"], 1, 6, 0, nllr // int(p["mod"]), p["tb_bytes"], p["harq_cb_index"], llr_off, p["tb_offset"])
        ce_off += nl * int(p["nof_rx_ports"]) * int(p["grid_nof_prb"]) * 12
        llr_off += (nllr + 15) & ~15
    ce_d = torch.zeros(ce_off, dtype=torch.complex64, device="cuda")
    llr_d = torch.zeros(llr_off, dtype=torch.int8, device="cuda")
    ctx.dmrs_pusch_estimate_layers_batch(cj, grid_d, ce_d, sc_d)
    ctx.pusch_demodulate_layers_batch(dj, grid_d, ce_d, sc_d, llr_d)
    ctx.pusch_decode_batch(td, llr_d, *h.args())


def process_and_compare(ctx, cases, rvs=None, harq=None):
    import torch
    import miphy
    rvs = rvs or [0] * len(cases)
    pdus, grid, tbs, ncb, cs = batch(miphy, cases, rvs)
    grid_d = torch.from_numpy(grid).cuda()
    fused, apart = harq or (Harq(torch, miphy, ncb, sum(t.size for t in tbs), len(cases)), Harq(torch, miphy, ncb, sum(t.size for t in tbs), len(cases)))
    sc_f = torch.full((80 * len(cases),), -77.0, dtype=torch.float32, device="cuda")
    sc_a = sc_f.clone()
    ctx.pusch_process_layers_batch(pdus, grid_d, *fused.args(), sc_f)
    separate_calls(ctx, torch, miphy, pdus, cs, grid_d, apart, sc_a)
    torch.cuda.synchronize()
    assert fused.same(torch, apart), "transport blocks, result records and HARQ arrays equal the three separate calls"
    assert sc_f.cpu().numpy().tobytes() == sc_a.cpu().numpy().tobytes()
    res = fused.res.cpu().numpy().view(miphy.PuschResult)
    return pdus, grid_d, tbs, res, fused, apart, sc_f.cpu().numpy().reshape(len(cases), 80)


def test_mixed_batch_recovers_the_transport_blocks(ctx):
    import torch
    import miphy
    cases = list(E.CHAIN_CASES) + [ONE_LAYER]
    pdus, grid_d, tbs, res, fused, _, sc = process_and_compare(ctx, cases)
    out = fused.out.cpu().numpy()
    for i, tb in enumerate(tbs):
        t0 = int(pdus[i]["base"]["tb_offset"])
        assert res[i]["tb_crc_ok"] == 1 and np.array_equal(out[t0:t0 + tb.size], tb), i
        nl, npt = cases[i][0], cases[i][1]
        assert np.all(sc[i, :5 * nl * npt] != -77.0) and np.all(sc[i, 5 * nl * npt:] == -77.0), i
    # the PDU on one layer: the bytes of miphy_pusch_process_batch for its base record
    k = len(cases) - 1
    base = np.ascontiguousarray(pdus["base"][k:k + 1])
    ncb = miphy.sch_segmentation(tbs[k].size, 1).nof_cbs
    base[0]["harq_cb_index"], base[0]["tb_offset"] = 0, 0
    h1 = Harq(torch, miphy, ncb, tbs[k].size, 1)
    sc1 = torch.full((20,), -77.0, dtype=torch.float32, device="cuda")
    ctx.pusch_process_batch(base, grid_d, *h1.args(), sc1)
    torch.cuda.synchronize()
    assert np.array_equal(h1.out.cpu().numpy(), tbs[k])
    assert h1.res.cpu().numpy().tobytes() == fused.res.cpu().numpy()[k * miphy.PuschResult.itemsize:].tobytes()
    assert sc1.cpu().numpy().tobytes() == sc[k, :20].tobytes()


@pytest.mark.parametrize("case", E.CHAIN_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_single_pdu(ctx, case):
    pdus, _, tbs, res, fused, _, _ = process_and_compare(ctx, [case])
    assert res[0]["tb_crc_ok"] == 1 and np.array_equal(fused.out.cpu().numpy(), tbs[0])


def test_retransmission(ctx):
    """rv 0 where the host chain fails, then rv 2 combined in the HARQ arrays: as through the separate calls, and the block comes out."""
    _, _, _, res0, fused, apart, _ = process_and_compare(ctx, [E.RETX_CASE], rvs=[0])
    assert res0[0]["tb_crc_ok"] == 0
    _, _, tbs, res2, fused, _, _ = process_and_compare(ctx, [E.RETX_CASE], rvs=[2], harq=(fused, apart))
    assert res2[0]["tb_crc_ok"] == 1 and np.array_equal(fused.out.cpu().numpy(), tbs[0])


@pytest.mark.parametrize("layers,ports", [(3, 2), (0, 2), (5, 4)])
def test_rule_breaking_pdu_is_refused(ctx, layers, ports):
    import torch
    import miphy
    cases = [E.CHAIN_CASES[0], E.CHAIN_CASES[0]]
    pdus, grid, tbs, ncb, _ = batch(miphy, cases, [0, 0])
    pdus[1]["nof_tx_layers"], pdus[1]["base"]["nof_rx_ports"] = layers, ports
    h = Harq(torch, miphy, ncb, sum(t.size for t in tbs), 2)
    before = [a.clone() for a in h.args()]
    sc = torch.full((160,), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"miphy error -1: pusch_process: PDU 1: "):
        ctx.pusch_process_layers_batch(pdus, torch.from_numpy(grid).cuda(), *h.args(), sc)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(h.args(), before)) and bool((sc == -77.0).all())
