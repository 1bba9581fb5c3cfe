#!/usr/bin/env python3
"""Throughput probe of miphy_precoding_weights_batch (csrc/precoding_weights.hip) beside miphy_srs_estimate_batch on the soundings that feed it, host
jobs, from one run: --jobs (1024) jobs of 272 PRB sounded at PRGs of 4 PRB towards A = 4 antenna ports (random matrices: the time of the kernel does not
depend on the values), legs
  su4_prg4 / su4_prg2: one UE of 4 ports and 4 layers, output PRGs of 4 and of 2 PRB (68 and 136 of them; the lane form);
  mu4_prg4 / mu4_prg2: four UEs of 1 port and 1 layer each;
  wideband_su4:        one UE of 4 ports and 4 layers, one output PRG over the 68 SRS PRGs (the wave form);
  srs_4tx / srs_1tx:   miphy_srs_estimate_batch of the soundings of the su4 legs (one job of 4 transmit ports, comb 4 on two combs, 4 symbols, 4 receive
                       ports per precoding job) and of the mu4 legs (four jobs of 1 transmit port, 1 symbol per precoding job): the yardstick.
  device_us: HIP events around --calls calls, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so the events see the
             kernels back to back, divided by --calls; the legs alternate; median, minimum and maximum over --reps windows.
One JSON line per leg. The measuring runs in a child process under --time-limit seconds, and every step of it under --step-limit seconds, so a hang
ends the run instead of holding the device.
Run on the MI355X:  python tools/precoding_weights_throughput.py [--reps 11] [--calls 10] [--jobs 1024]"""
import argparse
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

A, NOF_PRB, SRS_PRG, GRID_PRB = 4, 272, 4, 273
G = NOF_PRB // SRS_PRG
LEGS = {"su4_prg4": dict(ues=1, U=4, l=4, S=4, nof_prg=68), "su4_prg2": dict(ues=1, U=4, l=4, S=2, nof_prg=136),
        "mu4_prg4": dict(ues=4, U=1, l=1, S=4, nof_prg=68), "mu4_prg2": dict(ues=4, U=1, l=1, S=2, nof_prg=136),
        "wideband_su4": dict(ues=1, U=4, l=4, S=275, nof_prg=1)}


def weights_jobs(miphy, n, leg):
    """n jobs of the leg; UE k of job i reads the block (i ues + k) of `h` and owns the block (i ues + k) of the weights and of the metrics."""
    jobs = np.zeros(n, miphy.PrecodingWeightsJob)
    jobs["nof_ues"], jobs["nof_ports"], jobs["prg_size"], jobs["nof_prg"], jobs["reg"], jobs["amplitude"] = leg["ues"], A, leg["S"], leg["nof_prg"], 0.01, 1.0
    nh, nw, nm = G * A * leg["U"], leg["nof_prg"] * A * leg["l"], 3 * leg["nof_prg"] * leg["l"]
    for k in range(leg["ues"]):
        block = np.arange(n, dtype=np.int64) * leg["ues"] + k
        u = jobs["ue"][:, k]
        u["h_offset"], u["weights_offset"], u["metrics_offset"] = block * nh, block * nw, block * nm
        u["start_prb"], u["nof_prb"], u["prg_size"], u["nof_ue_ports"], u["nof_layers"] = 0, NOF_PRB, SRS_PRG, leg["U"], leg["l"]
        jobs["ue"][:, k] = u
    return jobs, n * leg["ues"] * nh, n * leg["ues"] * nw, n * leg["ues"] * nm


def srs_jobs(miphy, n, tx):
    jobs = np.zeros(n, miphy.SrsJob)
    i = np.arange(n)
    jobs["nof_prb"], jobs["comb_size"], jobs["nof_tx_ports"], jobs["nof_symbols"], jobs["nof_rx_ports"] = NOF_PRB, 4, tx, 4 if tx == 4 else 1, A
    jobs["cyclic_shift"], jobs["numerology"], jobs["slot"], jobs["prg_size"], jobs["grid_nprb"], jobs["hopping"] = 7 if tx == 4 else 0, 1, 3, SRS_PRG, GRID_PRB, 1
    jobs["start_symbol"], jobs["n_id"], jobs["comb_offset"] = 14 - jobs["nof_symbols"], i % 1024, i % 4
    jobs["h_offset"] = G * A * tx * i
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
    n = args.jobs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    grid = torch.view_as_complex(torch.randn(A * 14 * GRID_PRB * 12, 2, device="cuda", generator=gen))
    h = torch.view_as_complex(torch.randn(n * 4 * G * A, 2, device="cuda", generator=gen))  # 4 = ues x U of every leg
    h_srs = torch.zeros(n * 4 * G * A, dtype=torch.complex64, device="cuda")
    res = torch.zeros(4 * n * miphy.SrsResult.itemsize, dtype=torch.uint8, device="cuda")
    calls, info = {}, {}
    for name, leg in LEGS.items():
        jobs, nh, nw, nm = weights_jobs(miphy, n, leg)
        assert nh <= h.numel()
        w, m = torch.zeros(nw, dtype=torch.complex64, device="cuda"), torch.zeros(nm, dtype=torch.float32, device="cuda")
        calls[name] = (lambda j, w, m: lambda: ctx.precoding_weights_batch(j, h, w, m))(jobs, w, m)
        inf = miphy.precoding_weights_info(jobs[0])
        info[name] = dict(entry_point="precoding_weights_batch", form="wave" if inf["wave_form"] else "lane", output_prgs=n * leg["nof_prg"],
                          ues=leg["ues"], ue_ports=leg["U"], layers=leg["l"], output_prg_size=leg["S"])
    for name, (tx, per_job) in {"srs_4tx": (4, 1), "srs_1tx": (1, 4)}.items():
        jobs = srs_jobs(miphy, n * per_job, tx)
        calls[name] = (lambda j: lambda: ctx.srs_estimate_batch(j, grid, h_srs, res))(jobs)
        info[name] = dict(entry_point="srs_estimate_batch", srs_jobs=n * per_job, tx_ports=tx, symbols=4 if tx == 4 else 1)
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

    step("warm-up")
    for _ in range(3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for r in range(args.reps):
        step("window %d" % r)
        for name, call in calls.items():
            times[name].append(window(call))
    for name, t in times.items():
        print(json.dumps(dict(leg=name, jobs=n, reps=args.reps, calls_per_window=args.calls, device_us_median=round(float(np.median(t)), 1),
                              device_us_min=round(min(t), 1), device_us_max=round(max(t), 1), us_per_job=round(float(np.median(t)) / n, 3), **info[name])),
              flush=True)
    signal.alarm(0)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--spin-ms", type=float, default=5.0)
    ap.add_argument("--time-limit", type=int, default=240, help="seconds for the whole run")
    ap.add_argument("--step-limit", type=int, default=90, help="seconds for each step of it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert 1 <= args.jobs <= 4096
    if args.child:
        return measure(args)
    try:  # a fresh child does the measuring; this process never opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.time_limit)
    except subprocess.TimeoutExpired:
        sys.exit("precoding_weights_throughput: the run exceeded its time limit of %d s" % args.time_limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
