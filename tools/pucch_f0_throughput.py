#!/usr/bin/env python3
"""Throughput probe of miphy_pucch_process_f0_batch (csrc/pucch_f0.hip) next to the existing PUCCH kernel nearest in size, miphy_pucch_process_batch on
as many format-1 PDUs, from the same run:
  format0: n PDUs of two symbols on two receive ports, two HARQ-ACK bits and an SR opportunity (eight hypotheses), host jobs;
  format1: n PDUs of four symbols on two receive ports, one HARQ-ACK bit, host jobs;
for n = 1, 64 and 1024 (--pdus) on a 273-PRB grid of unit-variance noise: the time of these kernels does not depend on the samples.
  device_us: HIP events around --calls calls, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so the events see the
             kernels back to back, divided by --calls; the two entry points alternate; median, minimum and maximum over --reps windows.
One JSON line per entry point and size. The measuring runs in a child process under --time-limit seconds, and every step of it (set-up, warm-up, each
timed window) under --step-limit seconds, so a hang ends the run instead of holding the device.
Run on the MI355X:  python tools/pucch_f0_throughput.py [--reps 11] [--calls 10] [--pdus 1,64,1024]"""
import argparse
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

GRID_PRB, PORTS = 273, 2


def f0_jobs(miphy, n):
    jobs = np.zeros(n, miphy.PucchF0Job)
    i = np.arange(n)
    jobs["numerology"], jobs["slot"], jobs["nof_ports"], jobs["nof_symbols"], jobs["nof_harq_ack"], jobs["nof_sr"] = 1, 3, PORTS, 2, 2, 1
    jobs["start_symbol"], jobs["starting_prb"], jobs["initial_cyclic_shift"] = 2 * ((i // GRID_PRB) % 7), i % GRID_PRB, i % 12
    jobs["bwp_size_rb"], jobs["grid_nprb"], jobs["n_id"] = GRID_PRB, GRID_PRB, 77
    jobs["payload_offset"], jobs["energy_offset"] = 3 * i, 12 * i
    return jobs


def f1_jobs(miphy, n):
    jobs = np.zeros(n, miphy.PucchJob)
    i = np.arange(n)
    jobs["format"], jobs["numerology"], jobs["slot"], jobs["nof_ports"], jobs["nof_symbols"], jobs["nof_harq_ack"] = 1, 1, 3, PORTS, 4, 1
    jobs["start_symbol"], jobs["starting_prb"], jobs["initial_cyclic_shift"] = 4 * ((i // GRID_PRB) % 3), i % GRID_PRB, i % 12
    jobs["bwp_size_rb"], jobs["grid_nprb"], jobs["n_id"] = GRID_PRB, GRID_PRB, 77
    jobs["payload_offset"] = 3 * i
    return jobs


def measure(args):
    def step(name):
        signal.alarm(args.step_limit)  # the default action ends the process: a step that hangs does not outlive its limit
        print("# " + name, file=sys.stderr, flush=True)

    step("set-up")
    import torch
    import miphy
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    ctx = miphy.Context(0)
    sizes = [int(x) for x in args.pdus.split(",")]
    nmax = max(sizes)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    grid = torch.view_as_complex(torch.randn(PORTS * 14 * GRID_PRB * 12, 2, device="cuda", generator=gen))
    pay = torch.zeros(3 * nmax, dtype=torch.uint8, device="cuda")
    res = torch.zeros(nmax * miphy.PucchResult.itemsize, dtype=torch.uint8, device="cuda")
    en = torch.zeros(12 * nmax, dtype=torch.float32, device="cuda")
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
        ja, jb = f0_jobs(miphy, n), f1_jobs(miphy, n)
        f0 = lambda: ctx.pucch_process_f0_batch(ja, grid, pay, res, en)
        f1 = lambda: ctx.pucch_process_batch(jb, grid, pay, res)
        step("warm-up, %d PDUs" % n)
        for _ in range(3):
            f0()
            f1()
        torch.cuda.synchronize()
        t_a, t_b = [], []
        for r in range(args.reps):
            step("window %d" % r)
            t_a.append(window(f0))
            t_b.append(window(f1))
        for name, what, t in (("pucch_process_f0_batch", "format-0 PDUs of 2 symbols, 2 ports, 8 hypotheses", t_a),
                              ("pucch_process_batch", "format-1 PDUs of 4 symbols, 2 ports", t_b)):
            print(json.dumps(dict(entry_point=name, workload=what, pdus=n, reps=args.reps, calls_per_window=args.calls,
                                  device_us_median=round(float(np.median(t)), 1), device_us_min=round(min(t), 1), device_us_max=round(max(t), 1),
                                  us_per_pdu=round(float(np.median(t)) / n, 3))), flush=True)
    signal.alarm(0)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pdus", default="1,64,1024", help="batch sizes, comma separated")
    ap.add_argument("--spin-ms", type=float, default=5.0)
    ap.add_argument("--time-limit", type=int, default=240, help="seconds for the whole run")
    ap.add_argument("--step-limit", type=int, default=90, help="seconds for each step of it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert all(1 <= int(x) <= 4096 for x in args.pdus.split(","))
    if args.child:
        return measure(args)
    try:  # a fresh child does the measuring; this process never opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.time_limit)
    except subprocess.TimeoutExpired:
        sys.exit("pucch_f0_throughput: the run exceeded its time limit of %d s" % args.time_limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
