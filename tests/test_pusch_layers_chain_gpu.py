"""GPU: a transport block sent on 2 and on 4 layers, from the resource grid to its bytes on the device: miphy_pusch_demodulate_layers_batch with the
true channel as the estimate, then miphy_pusch_decode_batch(nof_layers = L) on the same stream. The transmitter is the host's
(tests/pusch_layers_cases.py: the oracle's encoder and mapper); tests/test_pusch_layers.py shows that these transmissions decode in the host chain."""
import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nl,npt,mod,tb_bytes,snr_db", PL.CHAIN_CASES)
def test_grid_to_transport_block(ctx, nl, npt, mod, tb_bytes, snr_db):
    import torch
    import miphy
    c, tb, grid, ce = PL.chain_transmission(nl, npt, mod, tb_bytes, snr_db)
    nsym = PL.nof_re(c) * nl
    seg = O.o_segmentation(tb_bytes * 8, 1, mod, nl, nsym)
    assert seg.nof_cbs >= 2
    jobs = np.array([PL.demod_job(miphy, c)], dtype=miphy.PuschDemodLayersJob)
    sc = np.zeros(5, np.float32)
    sc[2] = c["noise_var"]
    llr_d = torch.zeros(nsym * mod, dtype=torch.int8, device="cuda")
    d = np.zeros(1, dtype=miphy.PuschTbDesc)
    d[0] = (1, 0, mod, nl, 1, 1, 6, 0, nsym, tb_bytes, 0, 0, 0)
    soft_d = torch.full((seg.nof_cbs * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(seg.nof_cbs * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.zeros(seg.nof_cbs, dtype=torch.uint8, device="cuda")
    tb_d = torch.full((tb_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    ctx.pusch_demodulate_layers_batch(jobs, torch.from_numpy(grid.reshape(-1)).cuda(), torch.from_numpy(ce.reshape(-1)).cuda(), torch.from_numpy(sc).cuda(),
                                      llr_d, stream=stream)
    ctx.pusch_decode_batch(d, llr_d, soft_d, msgs_d, crc_d, tb_d, res_d, stream=stream)
    torch.cuda.synchronize()
    res = res_d.cpu().numpy().view(miphy.PuschResult)[0]
    assert res["tb_crc_ok"] == 1 and res["nof_codeblocks_total"] == seg.nof_cbs
    assert np.array_equal(tb_d.cpu().numpy(), tb)
    ok, out, mm = O.OraclePuschDecoder(1, mod, 0, nl, nsym, tb_bytes).decode(llr_d.cpu().numpy(), 0, True, 6, True)
    assert ok and np.array_equal(out, tb)
    assert (int(res["iters_min"]), int(res["iters_max"])) == mm
