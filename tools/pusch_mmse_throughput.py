#!/usr/bin/env python3
"""Throughput probe of the MMSE-IRC receive path next to the zero-forcing one: 273 PRB x 14 symbols (DM-RS on symbol 2, two CDM groups without
data), 256QAM, the compact estimate, `--jobs` transmissions per launch, each with a grid of its own. Legs, at 1 x 4, 2 x 4 and 4 x 4:
miphy_pusch_demodulate_layers_batch (zero forcing), miphy_pusch_demodulate_layers_mmse_batch with a covariance matrix per four PRBs and with
one for the allocation, and miphy_pusch_noise_covariance_batch on the same grids at both PRG sizes. Device-resident jobs (no staging copy in
the timed region), HIP events around `--iters` back-to-back launches after a warm-up of every leg; the legs are timed in turn `--rounds`
times, and the median, the fastest and the slowest round are printed, so the spread stands next to every figure.
Run on the MI355X:  python tools/pusch_mmse_throughput.py [--jobs 1024] [--iters 20] [--rounds 5] [--out profiles/pusch_mmse_throughput.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

NPRB, MOD, PRG = 273, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    args = ap.parse_args()
    import torch
    import miphy
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    ctx = miphy.Context(0)
    n, nsc = args.jobs, NPRB * 12
    nre = nsc * 13
    nprg = -(-NPRB // PRG)
    gen = torch.Generator(device="cuda").manual_seed(0)
    grid = torch.randn(n * 4 * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)  # [job][4 ports][14][nsc] complex
    ce = torch.randn(n * 16 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)         # [job][<= 4 layers][<= 4 ports][nsc] complex
    sc = torch.full((5 * n,), 0.01, dtype=torch.float32, device="cuda")
    llr = torch.zeros(n * nre * 4 * MOD + 64, dtype=torch.int8, device="cuda")
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((nprg, 4)) + 1j * rng.standard_normal((nprg, 4))) / np.sqrt(2)
    one = 0.01 * (np.eye(4)[None] + 10.0 * a[:, :, None] * a[:, None, :].conj())  # white noise plus an interferer 10 dB above it, per PRG
    cov = torch.from_numpy(np.tile(one.astype(np.complex64).reshape(-1), n)).cuda()   # [job][PRG][4][4], read by the demodulator
    cov_out = torch.zeros(n * nprg * 16, dtype=torch.complex64, device="cuda")           # written by the covariance kernel
    idx = np.arange(n, dtype=np.uint64)

    def masks(j):
        for r in range(NPRB):
            j["rb_mask"][:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)

    def demod_jobs(nl, npt, prg):
        mj = np.zeros(n, dtype=miphy.PuschDemodMmseJob)
        lj = mj["base"]
        j = lj["base"]
        j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = 0x4601, 900, MOD, npt, 0, 14
        j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 1, 2, 14, 1
        j["rx_ports"] = [0, 1, 2, 3]
        j["dmrs_symbols_mask"], j["grid_nof_prb"] = 1 << 2, NPRB
        masks(j)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (4 * 14 * nsc), idx * (16 * nsc), idx * 5
        j["llr_offset"], j["nof_llr"] = idx * (nre * 4 * MOD), nre * nl * MOD
        lj["nof_tx_layers"] = nl
        mj["cov_offset"], mj["prg_size"] = idx * (nprg * 16), prg
        assert miphy.pusch_demod_layers_nof_llr(lj[0]) == nre * nl * MOD
        return torch.from_numpy(np.ascontiguousarray(lj).view(np.uint8).copy()).cuda(), torch.from_numpy(mj.view(np.uint8).copy()).cuda()

    def ncov_jobs(nl, npt, prg):
        nj = np.zeros(n, dtype=miphy.PuschNcovJob)
        j = nj["base"]
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = 1, 3, 77, np.float32(10 ** (3 / 20))
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, npt, 0, 14, [0, 1, 2, 3]
        j["symbols_mask"], j["grid_nof_prb"] = 1 << 2, NPRB
        masks(j)
        j["grid_offset"] = idx * (4 * 14 * nsc)
        nj["cov_offset"], nj["loading"], nj["prg_size"] = idx * (nprg * 16), 0.0, prg
        assert miphy.pusch_noise_covariance_nof_prg(nj[0]) == (nprg if prg else 1)
        return torch.from_numpy(nj.view(np.uint8).copy()).cuda()

    legs = []
    for nl, npt in ((1, 4), (2, 4), (4, 4)):
        zf_d, _ = demod_jobs(nl, npt, 0)
        legs.append(("L%d_P%d_zf" % (nl, npt), nl, lambda d=zf_d: ctx.pusch_demodulate_layers_batch(d, grid, ce, sc, llr)))
        for prg in (PRG, 0):
            _, mm_d = demod_jobs(nl, npt, prg)
            legs.append(("L%d_P%d_mmse_prg%d" % (nl, npt, prg), nl, lambda d=mm_d: ctx.pusch_demodulate_layers_mmse_batch(d, grid, ce, cov, llr)))
            nc_d = ncov_jobs(nl, npt, prg)
            legs.append(("L%d_P%d_ncov_prg%d" % (nl, npt, prg), 0, lambda d=nc_d, p=npt, l=nl: ctx.pusch_noise_covariance_batch(d, grid, cov_out, max_ports=p, max_layers=l)))
    for _, _, run in legs:  # warm-up of every shape
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, _, run in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.iters)
    lines = []
    for name, nl, _ in legs:
        t = sorted(ms[name])
        med = t[len(t) // 2]
        rec = {"leg": name, "jobs": n, "ms_per_launch_median": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4), "slots_per_s": round(n / (med * 1e-3))}
        if nl:
            rec["llr_per_s"] = round(n * nre * nl * MOD / (med * 1e-3))
        lines.append(json.dumps(rec))
        print(lines[-1])
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
