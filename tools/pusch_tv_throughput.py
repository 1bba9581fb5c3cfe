#!/usr/bin/env python3
"""Throughput probe of the estimator that follows a channel through the slot (csrc/chest.hip: cfo_corr_kernel, chest_tv_kernel) against the estimator
that compensates a carrier frequency offset only (cfo_corr_kernel, chest_cfo_kernel, unchanged), on the same jobs and in both time modes.

Legs: the benchmark's shape -- 273 PRB, four receive ports, one layer -- with DM-RS on symbols (2, 11) and (2, 5, 8, 11), `--jobs` device-resident jobs
with the port and layer hint, a grid of random samples per job; and 24 PRB on 4 x 4 with the same DM-RS sets, a batch of 1024. All three entry points
store the same bytes (an estimate per symbol) and read the DM-RS elements twice (two launches); the new kernel interpolates nds vectors per subcarrier
where the CFO kernel interpolates one, and blends them for every stored element.

HIP events around `--iters` back-to-back calls after a warm-up of every leg; the legs are timed in turn `--rounds` times; median, fastest and slowest
round are printed, one JSON record per line, the ratio to the CFO leg of the same jobs with them.
Run on the MI355X:  python tools/pusch_tv_throughput.py [--jobs 256] [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NPT = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=256, help="jobs per call at 273 PRB")
    ap.add_argument("--small-jobs", type=int, default=1024, help="jobs per call at 24 PRB on 4 x 4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import miphy
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    ctx = miphy.Context(0)
    legs = []  # (name, run, jobs per call, bytes the estimator stores per call, name of the CFO leg on the same jobs)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for nprb, nl, n in ((273, 1, args.jobs), (24, 4, args.small_jobs)):
        nsc = nprb * 12
        grid = torch.randn(n * NPT * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)
        ce = torch.zeros(n * nl * NPT * 14 * nsc * 2, device="cuda", dtype=torch.float32)
        sc = torch.zeros(80 * n, dtype=torch.float32, device="cuda")
        cfo = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        var = torch.zeros(16 * n, dtype=torch.float32, device="cuda")
        idx = np.arange(n, dtype=np.uint64)
        for dmrs in ((2, 11), (2, 5, 8, 11)):
            fj = np.zeros(n, dtype=miphy.PuschChestCfoJob)
            j = fj["base"]
            j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = 1, 3, 77, 10 ** (3 / 20)
            j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, NPT, 0, 14, [0, 1, 2, 3]
            j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"] = 0, sum(1 << s for s in dmrs), nprb
            words = np.zeros(5, np.uint64)
            for r in range(nprb):
                words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
            j["rb_mask"] = words
            j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (NPT * 14 * nsc), idx * (nl * NPT * 14 * nsc), idx * 80
            fj["cfo_offset"] = 2 * idx
            tag, stored = "%dprb_L%d_P4_dmrs%s" % (nprb, nl, "_".join(map(str, dmrs))), n * nl * NPT * 14 * nsc * 8
            d_cfo = torch.from_numpy(fj.view(np.uint8).copy()).cuda()
            base = "estimate_%s_cfo_entry" % tag
            legs.append((base, lambda d=d_cfo, nl=nl, a=(grid, ce, sc, cfo): ctx.dmrs_pusch_estimate_cfo_batch(d, *a, max_ports=NPT, max_layers=nl), n, stored, None))
            for mode, mname in ((miphy.TIME_INTERPOLATE, "interpolate"), (miphy.TIME_LINE, "line")):
                vj = np.zeros(n, dtype=miphy.PuschChestTvJob)
                vj["base"], vj["var_offset"], vj["time_mode"] = fj, 16 * idx, mode
                d_tv = torch.from_numpy(vj.view(np.uint8).copy()).cuda()
                legs.append(("estimate_%s_tv_entry_%s" % (tag, mname),
                             lambda d=d_tv, nl=nl, a=(grid, ce, sc, cfo, var): ctx.dmrs_pusch_estimate_tv_batch(d, *a, max_ports=NPT, max_layers=nl), n, stored, base))

    for _, run, _, _, _ in legs:
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, run, _, _, _ in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.iters)
    med = {name: sorted(t)[len(t) // 2] for name, t in ms.items()}
    for name, _, jobs, stored, base in legs:
        t = sorted(ms[name])
        rec = {"leg": name, "jobs": jobs, "ms_per_call_median": round(med[name], 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
               "jobs_per_s": round(jobs / (med[name] * 1e-3)), "estimate_bytes_stored": stored, "estimate_store_gbyte_per_s": round(stored / (med[name] * 1e-3) / 1e9, 1)}
        if base:
            rec["ratio_to_cfo_entry"] = round(med[name] / med[base], 3)
        print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
