#!/usr/bin/env python3
"""Throughput probe of the PUSCH demodulator on 1..4 transmit layers (csrc/pusch_demod.hip): 273 PRB x 14 symbols (DM-RS on symbol 2, two CDM
groups without data), 256QAM, the compact estimate, `--jobs` transmissions per launch, each with a grid of its own. Legs: one layer through
miphy_pusch_demodulate_batch and through miphy_pusch_demodulate_layers_batch (on one port, the benchmark's slot, and on four), two and four
layers on four ports. Device-resident jobs (no staging copy in the timed region), HIP events around `--iters` back-to-back launches after a
warm-up of every leg; the legs are timed in turn `--rounds` times, and the median, the fastest and the slowest round are printed, so the spread
stands next to every figure.
Run on the MI355X:  python tools/pusch_layers_throughput.py [--jobs 1024] [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

NPRB, MOD = 273, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import miphy
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    ctx = miphy.Context(0)
    n, nsc = args.jobs, NPRB * 12
    nre = nsc * 13
    gen = torch.Generator(device="cuda").manual_seed(0)
    grid = torch.randn(n * 4 * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)  # [job][4 ports][14][nsc] complex
    ce = torch.randn(n * 16 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)         # [job][<= 4 layers][<= 4 ports][nsc] complex
    sc = torch.full((5 * n,), 0.01, dtype=torch.float32, device="cuda")
    llr = torch.zeros(n * nre * 4 * MOD + 64, dtype=torch.int8, device="cuda")

    def jobs_for(nl, npt):
        lj = np.zeros(n, dtype=miphy.PuschDemodLayersJob)
        j = lj["base"]
        j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = 0x4601, 900, MOD, npt, 0, 14
        j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 1, 2, 14, 1
        j["rx_ports"] = [0, 1, 2, 3]
        j["dmrs_symbols_mask"], j["grid_nof_prb"] = 1 << 2, NPRB
        for r in range(NPRB):
            j["rb_mask"][:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)
        idx = np.arange(n, dtype=np.uint64)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (4 * 14 * nsc), idx * (16 * nsc), idx * 5
        j["llr_offset"], j["nof_llr"] = idx * (nre * 4 * MOD), nre * nl * MOD
        lj["nof_tx_layers"] = nl
        assert miphy.pusch_demod_layers_nof_llr(lj[0]) == nre * nl * MOD
        return (torch.from_numpy(np.ascontiguousarray(j).view(np.uint8).copy()).cuda(), torch.from_numpy(lj.view(np.uint8).copy()).cuda())

    legs = []
    for name, nl, npt, old in (("L1_P1_one_layer_entry", 1, 1, True), ("L1_P1_layers_entry", 1, 1, False), ("L1_P4_one_layer_entry", 1, 4, True),
                               ("L1_P4_layers_entry", 1, 4, False), ("L2_P4_layers_entry", 2, 4, False), ("L4_P4_layers_entry", 4, 4, False)):
        base_d, layers_d = jobs_for(nl, npt)
        if old:
            legs.append((name, nl, lambda d=base_d: ctx.pusch_demodulate_batch(d, grid, ce, sc, llr)))
        else:
            legs.append((name, nl, lambda d=layers_d: ctx.pusch_demodulate_layers_batch(d, grid, ce, sc, llr)))
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
    for name, nl, _ in legs:
        t = sorted(ms[name])
        med = t[len(t) // 2]
        print(json.dumps({"leg": name, "jobs": n, "ms_per_launch_median": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                          "llr_per_s": round(n * nre * nl * MOD / (med * 1e-3)), "slots_per_s": round(n / (med * 1e-3))}))
    ctx.close()


if __name__ == "__main__":
    main()
