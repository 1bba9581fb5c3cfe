#!/usr/bin/env python3
"""Throughput probe of miphy_pusch_demodulate_tp_batch (transform precoding: csrc/pusch_demod.hip, csrc/tp_device.h) next to its yardstick,
miphy_pusch_demodulate_batch (CP-OFDM) on the very same jobs: 1024 slots of 270 PRB in a 273-PRB grid, 14 symbols with DM-RS (type 1, two CDM
groups without data) on two of them -- twelve data symbols --, compact estimate, QPSK and 256QAM, one and four receive ports. Both kernels read
the same samples and coefficients and write the same number of soft bits, so the ratio of the two times is what the transform in LDS costs.
  device_us: HIP events around the call's work, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so the events
             see the kernels back to back; the two entry points alternate, each figure is the median of --reps runs.
One JSON line per configuration. Run on the MI355X:  python tools/pusch_tp_throughput.py [--reps 11] [--slots 1024]
A run for counters (one configuration, --reps calls of the transform-precoded entry point and nothing else):
  rocprofv3 --pmc COUNTERS -d OUT -- python tools/pusch_tp_throughput.py --only MOD PORTS --reps 3
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

GRID_PRB, FIRST, NPRB, DMRS = 273, 2, 270, (2, 11)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--only", type=int, nargs=2, metavar=("MOD", "PORTS"), help="this configuration, the transform-precoded entry point only, no timing")
    args = ap.parse_args()
    import torch
    import miphy
    ctx = miphy.Context(0)
    n, nsc = args.slots, GRID_PRB * 12
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = 10_000_000 / e0.elapsed_time(e1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def device_us(call):
        torch.cuda._sleep(int(3.0 * cycles_per_ms))
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for mod, ports in ([tuple(args.only)] if args.only else [(2, 1), (8, 1), (2, 4), (8, 4)]):
        grid = torch.view_as_complex(torch.randn(n * ports * 14 * nsc, 2, device="cuda", generator=gen))
        ce = torch.view_as_complex(torch.randn(n * ports * nsc, 2, device="cuda", generator=gen))
        sc = torch.full((5 * n,), 0.05, dtype=torch.float32, device="cuda")
        jobs = np.zeros(n, dtype=miphy.PuschDemodJob)
        jobs["rnti"], jobs["n_id"], jobs["mod"], jobs["nof_rx_ports"], jobs["start_symbol"], jobs["nof_symbols"] = 0x4601, 900, mod, ports, 0, 14
        jobs["dmrs_type"], jobs["nof_cdm_groups_without_data"], jobs["ce_nof_symbols"], jobs["ce_compact"] = 1, 2, 14, 1
        jobs["rx_ports"] = [0, 1, 2, 3]
        jobs["dmrs_symbols_mask"], jobs["grid_nof_prb"] = sum(1 << l for l in DMRS), GRID_PRB
        w = np.zeros(5, dtype=np.uint64)
        for r in range(FIRST, FIRST + NPRB):
            w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
        jobs["rb_mask"] = w
        nof_llr = miphy.pusch_demod_nof_llr(jobs[0])
        stride = (nof_llr + 255) // 256 * 256
        jobs["nof_llr"] = nof_llr
        jobs["grid_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(ports * 14 * nsc)
        jobs["ce_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(ports * nsc)
        jobs["scalars_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(5)
        jobs["llr_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        llr = torch.zeros(n * stride, dtype=torch.int8, device="cuda")
        tp = lambda: ctx.pusch_demodulate_tp_batch(jobs, grid, ce, sc, llr)
        cp = lambda: ctx.pusch_demodulate_batch(jobs, grid, ce, sc, llr)
        if args.only:
            for _ in range(args.reps):
                tp()
            torch.cuda.synchronize()
            continue
        for _ in range(3):
            tp()
            cp()
        torch.cuda.synchronize()
        t_tp, t_cp = [], []
        for _ in range(args.reps):
            t_tp.append(device_us(tp))
            t_cp.append(device_us(cp))
        m_tp, m_cp = float(np.median(t_tp)), float(np.median(t_cp))
        # bytes both kernels move: samples of the data symbols and the coefficients of every port, the scrambling words, the soft bits
        nbytes = n * (ports * (12 + 1) * NPRB * 12 * 8 + nof_llr // 8 + nof_llr)
        print(json.dumps({"slots": n, "nof_prb": NPRB, "data_symbols": 12, "mod": mod, "ports": ports, "reps": args.reps,
                          "tp_device_us": round(m_tp, 1), "cp_ofdm_device_us": round(m_cp, 1), "ratio": round(m_tp / m_cp, 2),
                          "tp_min_us": round(min(t_tp), 1), "tp_max_us": round(max(t_tp), 1), "cp_min_us": round(min(t_cp), 1), "cp_max_us": round(max(t_cp), 1),
                          "tp_gb_per_s": round(nbytes / m_tp / 1e3, 1), "cp_ofdm_gb_per_s": round(nbytes / m_cp / 1e3, 1)}), flush=True)
        del grid, ce, llr
    ctx.close()


if __name__ == "__main__":
    main()
