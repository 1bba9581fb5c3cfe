"""GPU: miphy_pusch_process_layers_mmse_batch on the transmissions that zero forcing loses to an interferer (tests/pusch_mmse_cases.py IRC_CASES at
INR_DB, shown on the host by tests/test_pusch_mmse.py): the transport blocks come back with their CRC, the same grids through
miphy_pusch_process_layers_batch fail theirs, and the fused call gives the bytes of its four stages called one after the other."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_mmse_cases as MM
from test_pusch_process_layers_gpu import Harq, fill_pdu

pytestmark = pytest.mark.gpu
_tx = {}


def tx(case):
    if case not in _tx:
        _tx[case] = MM.interfered_tx(*case, MM.INR_DB)
    return _tx[case]


def batch(miphy, cases, prgs, loadings):
    """-> (PuschMmsePdu array, grid, transport blocks, codeblocks, PL cases)."""
    pdus = np.zeros(len(cases), dtype=miphy.PuschMmsePdu)
    grids, tbs, cs, goff, tboff, cboff = [], [], [], 0, 0, 0
    for i, case in enumerate(cases):
        c, tb, grid, _ = tx(case)
        fill_pdu(miphy, pdus[i]["base"]["base"], pdus[i]["base"], case, c, 0, cboff, goff, tboff)
        pdus[i]["prg_size"], pdus[i]["loading"] = prgs[i], loadings[i]
        grids.append(grid.reshape(-1))
        tbs.append(tb)
        cs.append(c)
        goff += grid.size
        tboff += tb.size
        cboff += miphy.sch_segmentation(tb.size, 1).nof_cbs
    return pdus, np.concatenate(grids), tbs, cboff, cs


def separate_calls(ctx, torch, miphy, pdus, cs, cases, grid_d, h, sc_d):
    """The four entry points one after the other on the current stream, on the layouts the processor uses."""
    n = pdus.size
    nj = np.zeros(n, dtype=miphy.PuschNcovJob)
    mj = np.zeros(n, dtype=miphy.PuschDemodMmseJob)
    td = np.zeros(n, dtype=miphy.PuschTbDesc)
    ce_off = llr_off = cov_off = 0
    for i in range(n):
        p, nl, c = pdus[i]["base"]["base"], int(pdus[i]["base"]["nof_tx_layers"]), cs[i]
        npt, prg = int(p["nof_rx_ports"]), int(pdus[i]["prg_size"])
        j = nj["base"][i]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = p["numerology"], p["slot_in_frame"], p["dmrs_scrambling_id"], np.float32(10.0) ** np.float32(3.0 / 20.0)
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, npt, 0, 14, p["rx_ports"]
        j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"], j["rb_mask"] = 1, p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"]
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = p["grid_offset"], ce_off, 80 * i
        nj[i]["cov_offset"], nj[i]["loading"], nj[i]["prg_size"] = cov_off, pdus[i]["loading"], prg
        mj["base"][i] = PL.demod_job(miphy, dict(c, compact=True), grid_off=int(p["grid_offset"]), ce_off=ce_off, sc_off=80 * i, llr_off=llr_off)
        mj[i]["cov_offset"], mj[i]["prg_size"] = cov_off, prg
        nllr = int(mj[i]["base"]["base"]["nof_llr"])
        td[i] = (1, p["rv"], p["mod"], nl, p["new_data"], 1, 6, 0, nllr // int(p["mod"]), p["tb_bytes"], p["harq_cb_index"], llr_off, p["tb_offset"])
        ce_off += nl * npt * int(p["grid_nof_prb"]) * 12
        llr_off += (nllr + 15) & ~15
        cov_off += miphy.pusch_noise_covariance_nof_prg(nj[i]) * npt * npt
    ce_d = torch.zeros(ce_off, dtype=torch.complex64, device="cuda")
    cov_d = torch.zeros(cov_off, dtype=torch.complex64, device="cuda")
    llr_d = torch.zeros(llr_off, dtype=torch.int8, device="cuda")
    ctx.dmrs_pusch_estimate_layers_batch(np.ascontiguousarray(nj["base"]), grid_d, ce_d, sc_d)
    ctx.pusch_noise_covariance_batch(nj, grid_d, cov_d)
    ctx.pusch_demodulate_layers_mmse_batch(mj, grid_d, ce_d, cov_d, llr_d)
    ctx.pusch_decode_batch(td, llr_d, *h.args())


@pytest.mark.parametrize("prg,loading", [(0, 0.0), (4, 0.01)])
def test_irc_returns_what_zero_forcing_loses(ctx, prg, loading):
    import torch
    import miphy
    cases = list(MM.IRC_CASES)
    n = len(cases)
    pdus, grid, tbs, ncb, cs = batch(miphy, cases, [prg] * n, [loading] * n)
    grid_d = torch.from_numpy(grid).cuda()
    total = sum(t.size for t in tbs)
    fused, apart, zf = (Harq(torch, miphy, ncb, total, n) for _ in range(3))
    sc_f = torch.full((80 * n,), -77.0, dtype=torch.float32, device="cuda")
    sc_a, sc_z = sc_f.clone(), sc_f.clone()
    ctx.pusch_process_layers_mmse_batch(pdus, None, grid_d, *fused.args(), sc_f)
    separate_calls(ctx, torch, miphy, pdus, cs, cases, grid_d, apart, sc_a)
    ctx.pusch_process_layers_batch(np.ascontiguousarray(pdus["base"]), grid_d, *zf.args(), sc_z)  # the yardstick: existing code on the same grids
    torch.cuda.synchronize()
    res = fused.res.cpu().numpy().view(miphy.PuschResult)
    res_zf = zf.res.cpu().numpy().view(miphy.PuschResult)
    out = fused.out.cpu().numpy()
    for i, tb in enumerate(tbs):
        t0 = int(pdus[i]["base"]["base"]["tb_offset"])
        assert res[i]["tb_crc_ok"] == 1 and np.array_equal(out[t0:t0 + tb.size], tb), ("IRC", i)
        assert res_zf[i]["tb_crc_ok"] == 0, ("zero forcing", i)
    assert fused.same(torch, apart), "transport blocks, result records and HARQ arrays equal the four separate calls"
    assert sc_f.cpu().numpy().tobytes() == sc_a.cpu().numpy().tobytes() == sc_z.cpu().numpy().tobytes(), "the estimator's scalars stay what they are"


@pytest.mark.parametrize("loading", [-1.0, float("nan"), float("inf")])
def test_bad_loading_is_refused(ctx, loading):
    import torch
    import miphy
    cases = [MM.IRC_CASES[2], MM.IRC_CASES[2]]
    pdus, grid, tbs, ncb, _ = batch(miphy, cases, [0, 0], [0.0, loading])
    h = Harq(torch, miphy, ncb, sum(t.size for t in tbs), 2)
    before = [a.clone() for a in h.args()]
    sc = torch.full((160,), -77.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"miphy error -1: pusch_process: PDU 1: "):
        ctx.pusch_process_layers_mmse_batch(pdus, None, torch.from_numpy(grid).cuda(), *h.args(), sc)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(h.args(), before)) and bool((sc == -77.0).all())
