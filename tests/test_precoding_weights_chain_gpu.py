"""GPU: the weights of miphy_precoding_weights_batch plug into the precoded PDSCH modulator without leaving the device. A UE sounds 8 PRB (comb 2, noise
free) towards 4 gNB ports; miphy_srs_estimate_batch -> miphy_precoding_weights_batch (PRGs of 2 PRB) -> miphy_pdsch_modulate_precoded_batch with
device-resident jobs that point at the weights buffer as it was written. The receiver is numpy: y(k) = H_dl(k) grid[:, k] with the channel that was
sounded (downlink = the transpose of the uplink matrix) and x^ = pinv(H_dl(k) W) y, which must be the layer symbols miphy_pdsch_modulate_layers_batch
makes of the same codeword within 1e-4 of the largest symbol: float32 rounding through a pseudo-inverse whose condition the channel's singular values
(1 and 1/2) keep at 2. With two UEs of one layer each at reg = 0, what a UE receives of the other UE's stream on its own receive eigen-direction must
stay below 1e-4 of what it receives of its own.
The channels are one matrix with prescribed singular values per UE (tests/precoding_weights_cases.py), scaled by a real gain per SRS PRG."""
import numpy as np
import pytest

import miphy
import pdsch_layers_cases as PC
import pdsch_precoded_cases as XC
import precoding_weights_cases as G
import srs_tx as X
from test_pdsch_layers_gpu import _modulate
from test_pdsch_precoded import mod_precoded_job

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, NPRB_GRID, PRB0, NPRB, PRG = 4, 12, 2, 8, 2


def sounding(rng, V, kbar):
    """(SRS parameters, Hg [G][A][U] complex128, left singular vectors): two UE ports, one matrix scaled by a real gain per PRG."""
    p = X.ue(R=A, nap=2, K=2, kbar=kbar, nprb=NPRB, prg=PRG, prb=PRB0, grid_nprb=NPRB_GRID, start=13)
    Q = G.unitary(rng, 2)
    h_dl = Q @ np.hstack([np.diag(G.SIGMA[:2]), np.zeros((2, A - 2))]) @ V.conj().T  # U x A
    gains = 1 + 0.3 * rng.uniform(-1, 1, NPRB // PRG)
    return p, gains[:, None, None] * h_dl.T[None], Q


def estimate(ctx, ues):
    """miphy_srs_estimate_batch of the UEs' soundings in one grid: the device tensor h and each UE's offset in it."""
    grid = X.build_grid(1, A, NPRB_GRID, 0.0, [(p, Hg, 0.0) for p, Hg, _ in ues])
    nh = (NPRB // PRG) * A * 2
    jobs = np.array([X.job_of(p, 0, 5 + i * (nh + 3)) for i, (p, _, _) in enumerate(ues)], miphy.SrsJob)
    h = torch.zeros(5 + len(ues) * (nh + 3), dtype=torch.complex64, device="cuda")
    res = torch.zeros(len(ues) * miphy.SrsResult.itemsize, dtype=torch.uint8, device="cuda")
    ctx.srs_estimate_batch(jobs, torch.from_numpy(grid.ravel()).cuda(), h, res)
    return h, [int(j["h_offset"]) for j in jobs]


def weights_job(h_offsets, layers, nw_per_layer):
    rec = np.zeros(1, miphy.PrecodingWeightsJob)
    rec["nof_ues"], rec["nof_ports"], rec["prg_size"], rec["nof_prg"], rec["reg"], rec["amplitude"] = len(layers), A, PRG, NPRB_GRID // PRG, 0.0, 1.0
    wo = 7
    for k, (ho, l) in enumerate(zip(h_offsets, layers)):
        u = rec["ue"][0, k]
        u["h_offset"], u["weights_offset"], u["metrics_offset"] = ho, wo, 0
        u["start_prb"], u["nof_prb"], u["prg_size"], u["nof_ue_ports"], u["nof_layers"] = PRB0, NPRB, PRG, 2, l
        wo += nw_per_layer * l + 3
    return rec, wo


def pdsch_case(name, L):
    return PC._case(name, L, 2, NPRB_GRID, range(PRB0, PRB0 + NPRB), start=3, nof=2)


def transmit(ctx, cases, w, w_offsets):
    """miphy_pdsch_modulate_precoded_batch of the cases, each onto the four ports of a grid of its own, with device-resident jobs and the device weights
    `w` as they are; returns the grids [case][port][14][nsc] and the layer symbols [L][n] of miphy_pdsch_modulate_layers_batch on the same codewords."""
    n = A * 14 * 12 * NPRB_GRID
    cws, coff = [], []
    for c in cases:
        coff.append(sum(x.size for x in cws))
        cw = PC.codeword(c)
        cws.append(np.concatenate([cw, np.zeros((-cw.size) % 16 + 16, np.uint8)]))
    jobs = []
    for i, (c, wo) in enumerate(zip(cases, w_offsets)):
        pc = dict(c=c, L=c["L"], P=A, prg_size=PRG, nof_prg=NPRB_GRID // PRG, ports=list(range(A)))
        jobs.append(mod_precoded_job(miphy, pc, None, wo, cw_off=coff[i], grid_off=i * n))
    jobs = np.array(jobs, dtype=miphy.PdschModPrecodedJob)
    gd = torch.zeros(len(cases) * n, dtype=torch.complex64, device="cuda")
    ctx.pdsch_modulate_precoded_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda(), None, w, torch.from_numpy(np.concatenate(cws)).cuda(), gd)
    torch.cuda.synchronize()
    grids = gd.cpu().numpy().reshape(len(cases), A, 14, 12 * NPRB_GRID)
    xs = []
    for c, buf in zip(cases, _modulate(ctx, cases)):
        lay = buf[XC.GUARD:buf.size - XC.GUARD].reshape(PC.grid_shape(c))
        sy, col = XC.data_positions(c)
        xs.append(lay[np.asarray(c["ports"])[:, None], sy[None, :], col[None, :]])
    return grids, xs


def test_one_ue_two_layers_through_the_channel_that_was_sounded(ctx):
    rng = np.random.default_rng(21)
    p, Hg, _ = ue = sounding(rng, G.unitary(rng, A), 0)
    h, ho = estimate(ctx, [ue])
    nprg = NPRB_GRID // PRG
    rec, nw = weights_job(ho, [2], nprg * A)
    w = torch.full((nw,), complex("nan"), dtype=torch.complex64, device="cuda")
    ctx.precoding_weights_batch(rec, h, w)
    c = pdsch_case("chain_one_ue_L2", 2)
    grids, xs = transmit(ctx, [c], w, [int(rec["ue"]["weights_offset"][0, 0])])
    W = w.cpu().numpy()[7:7 + nprg * A * 2].reshape(nprg, A, 2).astype(complex)
    sy, col = XC.data_positions(c)
    x, worst = xs[0].astype(complex), 0.0
    assert sy.size == 2 * 12 * NPRB and np.abs(x).min() > 0
    for i in range(sy.size):
        prb = col[i] // 12
        h_dl = Hg[(prb - PRB0) // PRG].T  # U x A
        eff = h_dl @ W[prb // PRG]
        assert np.linalg.cond(eff) <= 100
        xh = np.linalg.pinv(eff) @ (h_dl @ grids[0][:, sy[i], col[i]].astype(complex))
        worst = max(worst, np.abs(xh - x[:, i]).max())
    print("largest |x^ - x| %.3g of the largest symbol" % (worst / np.abs(x).max()))
    assert worst <= 1e-4 * np.abs(x).max()
    for g in range(NPRB // PRG):  # and the two streams arrive orthogonal, with the gains of the two singular values: eigen-beamforming
        eff = Hg[g].T @ W[g + PRB0 // PRG]
        gram = eff.conj().T @ eff
        assert abs(gram[0, 1]) <= 1e-4 * gram[0, 0].real and abs(gram[1, 1].real / gram[0, 0].real - 0.25) <= 1e-4


def test_two_ues_of_one_layer_do_not_hear_each_other(ctx):
    rng = np.random.default_rng(22)
    Q = G.unitary(rng, A)
    ues = [sounding(rng, G.near_identity(rng, A) @ Q[:, [k, 1 - k, 2, 3]], k) for k in (0, 1)]  # a UE's strongest direction is the other's second; the other comb offset
    h, ho = estimate(ctx, ues)
    nprg = NPRB_GRID // PRG
    rec, nw = weights_job(ho, [1, 1], nprg * A)
    w = torch.full((nw,), complex("nan"), dtype=torch.complex64, device="cuda")
    ctx.precoding_weights_batch(rec, h, w)
    cases = [pdsch_case("chain_two_ues_%d" % k, 1) for k in (0, 1)]
    grids, xs = transmit(ctx, cases, w, [int(rec["ue"]["weights_offset"][0, k]) for k in (0, 1)])
    sy, col = XC.data_positions(cases[0])
    worst = 0.0
    for k, (p, Hg, Qk) in enumerate(ues):
        for i in range(sy.size):
            row = Qk[:, 0].conj() @ Hg[(col[i] // 12 - PRB0) // PRG].T  # the UE's strongest receive direction behind its channel: 1 x A
            own, other = abs(row @ grids[k][:, sy[i], col[i]].astype(complex)), abs(row @ grids[1 - k][:, sy[i], col[i]].astype(complex))
            assert own > 0.1
            worst = max(worst, other / own)
    print("largest share of the other UE's stream: %.3g" % worst)
    assert worst <= 1e-4
