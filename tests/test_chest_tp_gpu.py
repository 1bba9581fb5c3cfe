"""GPU: the DM-RS of a transform-precoded PUSCH (TS 38.211 6.4.1.1.1.2). miphy_dmrs_pusch_tp_pilots_batch against the numpy restatement of
the low-PAPR sequences and their hopping (tests/pusch_tp_ref.py), and miphy_dmrs_pusch_estimate_tp_batch against
miphy_port_channel_estimate_batch (pinned to the oracle by tests/test_chest_gpu.py) fed those pilots: the same kernel, so the same bytes."""
import numpy as np
import pytest

import pusch_tp_ref as R

pytestmark = pytest.mark.gpu
DSYMS = (2, 7, 11)


def _mask_words(first, nprb):
    w = np.zeros(5, dtype=np.uint64)
    for r in range(first, first + nprb):
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def _job(miphy, grid_prb, first, nprb, ports, slot, n_id_rs, hopping, compact=1, dsyms=DSYMS, pilots_off=0, grid_off=0, ce_off=0, sc_off=0):
    j = np.zeros(1, dtype=miphy.PuschChestTpJob)[0]
    b = j["base"]
    b["numerology"], b["slot_in_frame"], b["scrambling_id"], b["scaling"] = 1, slot, n_id_rs, np.float32(10.0) ** np.float32(3.0 / 20.0)
    b["nof_tx_layers"], b["nof_rx_ports"], b["first_symbol"], b["nof_symbols"], b["rx_ports"], b["ce_compact"] = 1, ports, 0, 14, [0, 1, 2, 3], compact
    b["symbols_mask"], b["grid_nof_prb"], b["rb_mask"] = sum(1 << l for l in dsyms), grid_prb, _mask_words(first, nprb)
    b["grid_offset"], b["ce_offset"], b["scalars_offset"], b["pilots_offset"] = grid_off, ce_off, sc_off, pilots_off
    j["hopping"] = hopping
    return j


@pytest.mark.parametrize("device_jobs", [False, True])
def test_pilots_match_the_restatement(ctx, device_jobs):
    """The three hopping modes, slots 0 and 19 of the frame at 30 kHz, 2, 5, 6, 12 and 270 PRB (lengths 12, 30, 36, 72 -- the first with v -- and
    1620), three DM-RS symbols each, in one call. Within 1e-6: the angle is a fraction below 2 of pi rounded to single precision (3.7e-7 rad) plus
    two units in the last place of sincospi. Nothing is written between the jobs' pilots."""
    import torch
    import miphy
    jobs, exp, off = [], [], 0
    for hopping in (0, 1, 2):
        for slot in (0, 19):
            for nprb in (2, 5, 6, 12, 270):
                n_id = (37 * nprb + 101 * slot + 500 * hopping) % 1008
                jobs.append(_job(miphy, 273, 1, nprb, 1, slot, n_id, hopping, pilots_off=off))
                exp.append((off, R.dmrs_pilots(n_id, hopping, slot, DSYMS, nprb)))
                off += 3 * 6 * nprb + 2
    out = torch.full((off,), 7 + 7j, dtype=torch.complex64, device="cuda")
    ja = np.array(jobs, dtype=miphy.PuschChestTpJob)
    ctx.dmrs_pusch_tp_pilots_batch(torch.from_numpy(ja.view(np.uint8)).cuda() if device_jobs else ja, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for j, (o, e) in zip(jobs, exp):
        d = np.abs(got[o:o + e.size].astype(np.complex128) - e.reshape(-1)).max()
        worst = max(worst, d)
        assert d <= 1e-6, (int(j["hopping"]), int(j["base"]["slot_in_frame"]), e.shape, d)
        assert np.all(got[o + e.size:o + e.size + 2] == 7 + 7j)
    print("worst distance of the device pilots from the restatement: %.3g" % worst)
    # the cases exercise what they are meant to: group hopping moves u, sequence hopping draws both v
    assert len({R.dmrs_uv(int(j["base"]["scrambling_id"]), 1, int(j["base"]["slot_in_frame"]), l, 72)[0] for j in jobs if j["hopping"] == 1 for l in DSYMS}) > 3
    assert {R.dmrs_uv(int(j["base"]["scrambling_id"]), 2, int(j["base"]["slot_in_frame"]), l, 72)[1] for j in jobs if j["hopping"] == 2 for l in DSYMS} == {0, 1}


@pytest.mark.parametrize("device_jobs", [False, True])
def test_estimator_equals_the_port_estimator_fed_the_pilots(ctx, device_jobs):
    """Estimate and scalars bit-identical to miphy_port_channel_estimate_batch with the device pilots: 2, 5, 6 and 12 PRB on a 24-PRB grid and 270
    on 273, one to four ports, compact and per-symbol estimates, the three hopping modes, two and three DM-RS symbols."""
    import torch
    import miphy
    rng = np.random.default_rng(31)
    cases = [(24, 3, 2, 1, 0, 1, (2, 11)), (24, 7, 5, 2, 1, 0, DSYMS), (24, 11, 6, 4, 2, 1, (2, 11)), (24, 9, 12, 3, 2, 0, DSYMS), (273, 2, 270, 2, 1, 1, DSYMS)]
    jobs, grids = [], []
    goff = coff = poff = 0
    for k, (gprb, first, nprb, ports, hopping, compact, dsyms) in enumerate(cases):
        nsc = gprb * 12
        grids.append((rng.standard_normal((4, 14, nsc)) + 1j * rng.standard_normal((4, 14, nsc))).astype(np.complex64))
        jobs.append(_job(miphy, gprb, first, nprb, ports, 19 - k, 100 + 200 * k, hopping, compact, dsyms, poff, goff, coff, 20 * k))
        goff += grids[-1].size
        coff += ports * (1 if compact else 14) * nsc
        poff += len(dsyms) * 6 * nprb
    ja = np.array(jobs, dtype=miphy.PuschChestTpJob)
    g = torch.from_numpy(np.concatenate([x.reshape(-1) for x in grids])).cuda()
    pil = torch.zeros(poff, dtype=torch.complex64, device="cuda")
    ctx.dmrs_pusch_tp_pilots_batch(ja, pil)
    ce1 = torch.full((coff,), 5 + 5j, dtype=torch.complex64, device="cuda")
    sc1 = torch.full((20 * len(cases),), -5.0, dtype=torch.float32, device="cuda")
    ctx.port_channel_estimate_batch(np.ascontiguousarray(ja["base"]), g, pil, ce1, sc1)
    ce2, sc2 = torch.full_like(ce1, 5 + 5j), torch.full_like(sc1, -5.0)
    if device_jobs:
        ctx.dmrs_pusch_estimate_tp_batch(torch.from_numpy(ja.view(np.uint8)).cuda(), g, ce2, sc2, max_ports=4)
    else:
        ctx.dmrs_pusch_estimate_tp_batch(ja, g, ce2, sc2)
    torch.cuda.synchronize()
    a, b = ce1.cpu().numpy(), ce2.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.any(a != 5 + 5j)
    s1, s2 = sc1.cpu().numpy(), sc2.cpu().numpy()
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    for k, c in enumerate(cases):
        assert np.all(np.isfinite(s1[20 * k:20 * k + 5 * c[3]])) and s1[20 * k] > 0 and np.all(s1[20 * k + 5 * c[3]:20 * (k + 1)] == -5.0)


@pytest.mark.parametrize("nprb", [1, 3, 4])
def test_lengths_without_a_table_are_refused(ctx, nprb):
    """1, 3 and 4 PRB (lengths 6, 18 and 24) need tables the library does not hold: refused by message on the host with nothing enqueued, the good job
    in front included; skipped in device memory, where the good job is served."""
    import torch
    import miphy
    good = _job(miphy, 24, 0, 2, 1, 3, 45, 0, pilots_off=0)
    bad = _job(miphy, 24, 5, nprb, 1, 3, 45, 0, pilots_off=40, ce_off=24 * 12, sc_off=20)
    ja = np.array([good, bad], dtype=miphy.PuschChestTpJob)
    out = torch.full((40 + 3 * 24 + 4,), 7 + 7j, dtype=torch.complex64, device="cuda")
    g = torch.ones(4 * 14 * 288, dtype=torch.complex64, device="cuda")
    ce = torch.full((2 * 288,), 5 + 5j, dtype=torch.complex64, device="cuda")
    sc = torch.full((40,), -5.0, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="Tables"):
        ctx.dmrs_pusch_tp_pilots_batch(ja, out)
    with pytest.raises(RuntimeError, match="Tables"):
        ctx.dmrs_pusch_estimate_tp_batch(ja, g, ce, sc)
    torch.cuda.synchronize()
    assert bool((out == 7 + 7j).all()) and bool((ce == 5 + 5j).all()) and bool((sc == -5.0).all())
    jd = torch.from_numpy(ja.view(np.uint8)).cuda()
    ctx.dmrs_pusch_tp_pilots_batch(jd, out)
    ctx.dmrs_pusch_estimate_tp_batch(jd, g, ce, sc, max_ports=1)
    torch.cuda.synchronize()
    o, c, s = out.cpu().numpy(), ce.cpu().numpy(), sc.cpu().numpy()
    assert np.abs(o[:36].astype(np.complex128) - R.dmrs_pilots(45, 0, 3, DSYMS, 2).reshape(-1)).max() <= 1e-6 and np.all(o[36:] == 7 + 7j)
    assert np.all(c[:24] != 5 + 5j) and np.all(c[24:] == 5 + 5j) and np.all(s[:5] != -5.0) and np.all(s[5:] == -5.0)


@pytest.mark.parametrize("field,value,message", [("hopping", 3, "hopping"), ("scrambling_id", 1008, "n_ID"), ("n_scid", 1, "n_ID"), ("nof_tx_layers", 2, "one layer"),
                                                 ("hop_symbol", 7, "hopping"), ("seven", 7, "2\\^a"), ("gap", 0, "contiguous"), ("slot_in_frame", 20, "slot")])
def test_rule_breaks_are_refused(ctx, field, value, message):
    import torch
    import miphy
    j = _job(miphy, 24, 2, 6, 1, 3, 45, 0)
    if field == "hopping":
        j["hopping"] = value
    elif field == "seven":
        j["base"]["rb_mask"] = _mask_words(2, 7)
    elif field == "gap":
        j["base"]["rb_mask"] = _mask_words(2, 3) | _mask_words(6, 3)
    else:
        j["base"][field] = value
    out = torch.full((200,), 7 + 7j, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match=message):
        ctx.dmrs_pusch_tp_pilots_batch(np.array([j], dtype=miphy.PuschChestTpJob), out)
    ctx.dmrs_pusch_tp_pilots_batch(torch.from_numpy(np.array([j], dtype=miphy.PuschChestTpJob).view(np.uint8)).cuda(), out)
    torch.cuda.synchronize()
    assert bool((out == 7 + 7j).all())
