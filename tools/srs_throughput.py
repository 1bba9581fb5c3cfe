#!/usr/bin/env python3
"""Throughput probe of miphy_srs_estimate_batch (csrc/srs.hip) on its two reference workloads, host jobs, from one run:
  small: n jobs of 48 PRB at comb 2, 2 transmit ports, 2 symbols, 2 receive ports, PRGs of 4 PRB (M = 288);
  large: n jobs of 272 PRB at comb 4, 4 transmit ports on two combs, 4 symbols, 4 receive ports, PRGs of 4 PRB (M = 816);
for n = 1, 64 and 1024 (--jobs) on a 273-PRB grid of unit-variance noise: the time of the kernel does not depend on the samples. The jobs of a call
read the same grid window, as the UEs of one slot do.
  device_us: HIP events around --calls calls, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so the events see the
             kernels back to back, divided by --calls; the two workloads alternate; median, minimum and maximum over --reps windows.
  grid_bytes: what the kernel reads of the grid per call, 2 x 8 bytes per SRS element of every job (the grid is read twice: once for the delay, once
             for the PRGs), and grid_gb_per_s that over the median, to set against the bandwidth of L2 and HBM. Jobs that share a window read the same
             bytes, so at 64 and 1024 jobs this is a rate out of the caches.
One JSON line per workload and size. The measuring runs in a child process under --time-limit seconds, and every step of it (set-up, warm-up, each timed
window) under --step-limit seconds, so a hang ends the run instead of holding the device.
Run on the MI355X:  python tools/srs_throughput.py [--reps 11] [--calls 10] [--jobs 1,64,1024]"""
import argparse
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

GRID_PRB, PORTS = 273, 4
WORKLOADS = {"small": dict(nof_prb=48, comb_size=2, nof_tx_ports=2, nof_symbols=2, nof_rx_ports=2, cyclic_shift=1, combs=1),
             "large": dict(nof_prb=272, comb_size=4, nof_tx_ports=4, nof_symbols=4, nof_rx_ports=4, cyclic_shift=7, combs=2)}


def srs_jobs(miphy, n, w):
    jobs = np.zeros(n, miphy.SrsJob)
    i = np.arange(n)
    for k in ("nof_prb", "comb_size", "nof_tx_ports", "nof_symbols", "nof_rx_ports", "cyclic_shift"):
        jobs[k] = w[k]
    jobs["numerology"], jobs["slot"], jobs["prg_size"], jobs["grid_nprb"], jobs["hopping"] = 1, 3, 4, GRID_PRB, 1
    jobs["start_symbol"], jobs["n_id"], jobs["comb_offset"] = 14 - w["nof_symbols"], i % 1024, i % w["comb_size"]
    nof_h = w["nof_prb"] // 4 * w["nof_rx_ports"] * w["nof_tx_ports"]
    jobs["h_offset"] = nof_h * i
    return jobs, nof_h


def grid_bytes(n, w):
    return n * 2 * 8 * w["nof_rx_ports"] * w["nof_symbols"] * w["combs"] * (12 * w["nof_prb"] // w["comb_size"])


def measure(args):
    def step(name):
        signal.alarm(args.step_limit)  # the default action ends the process: a step that hangs does not outlive its limit
        print("# " + name, file=sys.stderr, flush=True)

    step("set-up")
    import torch
    import miphy
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    ctx = miphy.Context(0)
    sizes = [int(x) for x in args.jobs.split(",")]
    nmax = max(sizes)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    grid = torch.view_as_complex(torch.randn(PORTS * 14 * GRID_PRB * 12, 2, device="cuda", generator=gen))
    h = torch.zeros(nmax * 68 * 16, dtype=torch.complex64, device="cuda")
    res = torch.zeros(nmax * miphy.SrsResult.itemsize, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = 10_000_000 / e0.elapsed_time(e1)

    def window(call):
        torch.cuda._sleep(int(args.spin_ms * cycles_per_ms))
        e0.record()
        for _ in range(args.calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls

    for n in sizes:
        calls, times = {}, {}
        for name, w in WORKLOADS.items():
            jobs, nof_h = srs_jobs(miphy, n, w)
            assert nof_h * n <= h.numel()
            calls[name] = (lambda j: lambda: ctx.srs_estimate_batch(j, grid, h, res))(jobs)
            times[name] = []
        step("warm-up, %d jobs" % n)
        for _ in range(3):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        for r in range(args.reps):
            step("window %d" % r)
            for name, call in calls.items():
                times[name].append(window(call))
        for name, w in WORKLOADS.items():
            t, b = times[name], grid_bytes(n, w)
            print(json.dumps(dict(entry_point="srs_estimate_batch", workload="%s: %d PRB, comb %d, %d tx ports, %d symbols, %d rx ports" % (
                name, w["nof_prb"], w["comb_size"], w["nof_tx_ports"], w["nof_symbols"], w["nof_rx_ports"]), jobs=n, reps=args.reps, calls_per_window=args.calls,
                device_us_median=round(float(np.median(t)), 1), device_us_min=round(min(t), 1), device_us_max=round(max(t), 1),
                us_per_job=round(float(np.median(t)) / n, 3), grid_bytes=b, grid_gb_per_s=round(b / float(np.median(t)) / 1e3, 2))), flush=True)
    signal.alarm(0)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--jobs", default="1,64,1024", help="batch sizes, comma separated")
    ap.add_argument("--spin-ms", type=float, default=5.0)
    ap.add_argument("--time-limit", type=int, default=240, help="seconds for the whole run")
    ap.add_argument("--step-limit", type=int, default=90, help="seconds for each step of it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert all(1 <= int(x) <= 4096 for x in args.jobs.split(","))
    if args.child:
        return measure(args)
    try:  # a fresh child does the measuring; this process never opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.time_limit)
    except subprocess.TimeoutExpired:
        sys.exit("srs_throughput: the run exceeded its time limit of %d s" % args.time_limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
