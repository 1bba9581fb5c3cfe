#!/usr/bin/env python3
"""Throughput probe of miphy_pucch_process_f34_batch (csrc/pucch_f34.hip) on a slot's worth of PDUs, next to the one existing yardstick of the
uplink control path, miphy_pucch_process_batch_ex on as many 16-PRB format-2 PDUs, from the same run:
  f34:     --pdus format-3 PDUs of 4 PRB x 14 symbols (QPSK, E = 1152) side by side on a 273-PRB grid plus --pdus format-4 PDUs (four sequences
           per PRB on 16 PRBs, E = 72), every PDU --bits bits (polar coded above 11), --ports receive ports, list size --list-size;
  format2: 2 x --pdus format-2 PDUs of 16 PRB x 2 symbols (E = 512) with the same bits, ports and list size.
The grid holds unit-variance noise: the time of these kernels does not depend on the samples, and the polar decoder works through every field.
  device_us: HIP events around --calls calls, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so the events see the
             kernels back to back, divided by --calls; the two entry points alternate; median, minimum and maximum over --reps windows.
One JSON line per entry point and a last one with the ratio. The measuring runs in a child process under --time-limit seconds, and every step of
it (set-up, warm-up, each timed window) under --step-limit seconds, so a hang ends the run instead of holding the device.
Run on the MI355X:  python tools/pucch_f34_throughput.py [--reps 21] [--calls 10] [--pdus 64] [--bits 40] [--ports 4] [--list-size 1]"""
import argparse
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

GRID_PRB = 273


def split(K):
    return min(K, 8), 0, K - min(K, 8)


def f34_jobs(miphy, n, bits, ports):
    jobs = np.zeros(2 * n, miphy.PucchF34Job)
    jobs["numerology"], jobs["slot"], jobs["nof_ports"], jobs["start_symbol"], jobs["nof_symbols"] = 1, 3, ports, 0, 14
    jobs["bwp_size_rb"], jobs["grid_nprb"], jobs["n_id_hopping"], jobs["n_id_scrambling"] = GRID_PRB, GRID_PRB, 77, 99
    jobs["nof_harq_ack"], jobs["nof_sr"], jobs["nof_csi_part1"] = split(bits)
    jobs["rnti"] = 1 + np.arange(2 * n)
    f3, f4 = jobs[:n], jobs[n:]
    f3["format"], f3["nof_prb"] = 3, 4
    f3["starting_prb"] = 4 * (np.arange(n) % 64)
    f4["format"], f4["nof_prb"], f4["occ_length"] = 4, 1, 4
    f4["occ_index"], f4["starting_prb"] = np.arange(n) % 4, 256 + (np.arange(n) // 4) % 16
    info = [miphy.pucch_f34_info(j) for j in (f3[0], f4[0])]
    stride = 1152
    assert max(int(i["E"]) for i in info) <= stride
    jobs["payload_offset"] = np.arange(2 * n, dtype=np.uint64) * np.uint64(bits)
    jobs["llr_offset"] = np.arange(2 * n, dtype=np.uint64) * np.uint64(stride)
    return jobs, 2 * n * stride


def f2_jobs(miphy, n, bits, ports):
    jobs = np.zeros(n, miphy.PucchJob)
    jobs["format"], jobs["numerology"], jobs["slot"], jobs["nof_ports"], jobs["nof_symbols"], jobs["nof_prb"] = 2, 1, 3, ports, 2, 16
    jobs["start_symbol"], jobs["starting_prb"] = 2 * (np.arange(n) % 7), 16 * (np.arange(n) % 17)
    jobs["bwp_size_rb"], jobs["grid_nprb"], jobs["n_id"], jobs["n_id_0"] = GRID_PRB, GRID_PRB, 99, 77
    h, s, c = split(bits)
    jobs["nof_harq_ack"], jobs["nof_sr"], jobs["nof_csi_part1"] = h, s, c
    jobs["rnti"] = 1 + np.arange(n)
    jobs["payload_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    jobs["llr_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(512)
    return jobs, n * 512


def measure(args):
    def step(name):
        signal.alarm(args.step_limit)  # the default action ends the process: a step that hangs does not outlive its limit
        print("# " + name, file=sys.stderr, flush=True)

    step("set-up")
    import torch
    import miphy
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    ctx = miphy.Context(0)
    n, bits, ports, L = args.pdus, args.bits, args.ports, args.list_size
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    grid = torch.view_as_complex(torch.randn(ports * 14 * GRID_PRB * 12, 2, device="cuda", generator=gen))
    ja, nllr_a = f34_jobs(miphy, n, bits, ports)
    jb, nllr_b = f2_jobs(miphy, 2 * n, bits, ports)
    pay = torch.zeros(2 * n * bits, dtype=torch.uint8, device="cuda")
    res = torch.zeros(2 * n * miphy.PucchResult.itemsize, dtype=torch.uint8, device="cuda")
    llr = torch.zeros(max(nllr_a, nllr_b), dtype=torch.int8, device="cuda")
    f34 = lambda: ctx.pucch_process_f34_batch(ja, L, grid, pay, res, llr)
    f2 = lambda: ctx.pucch_process_batch_ex(jb, L, grid, pay, res, llr)
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
        f34()
        f2()
    torch.cuda.synchronize()
    t_a, t_b = [], []
    for r in range(args.reps):
        step("window %d" % r)
        t_a.append(window(f34))
        t_b.append(window(f2))
    signal.alarm(0)
    common = {"pdus": 2 * n, "bits": bits, "ports": ports, "list_size": L, "reps": args.reps, "calls_per_window": args.calls}
    out = []
    for name, what, t in (("pucch_process_f34_batch", "%d format-3 PDUs of 4 PRB x 14 symbols + %d format-4 PDUs" % (n, n), t_a),
                          ("pucch_process_batch_ex", "%d format-2 PDUs of 16 PRB x 2 symbols" % (2 * n), t_b)):
        out.append(dict(common, entry_point=name, workload=what, device_us_median=round(float(np.median(t)), 1), device_us_min=round(min(t), 1),
                        device_us_max=round(max(t), 1), us_per_pdu=round(float(np.median(t)) / (2 * n), 3)))
        print(json.dumps(out[-1]), flush=True)
    print(json.dumps(dict(common, ratio_f34_over_format2=round(out[0]["device_us_median"] / out[1]["device_us_median"], 2))), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pdus", type=int, default=64, help="format-3 PDUs, and as many format-4 PDUs")
    ap.add_argument("--bits", type=int, default=40)
    ap.add_argument("--ports", type=int, default=4)
    ap.add_argument("--list-size", type=int, default=1)
    ap.add_argument("--spin-ms", type=float, default=5.0)
    ap.add_argument("--time-limit", type=int, default=240, help="seconds for the whole run")
    ap.add_argument("--step-limit", type=int, default=90, help="seconds for each step of it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert 1 <= args.pdus <= 64 and 3 <= args.bits <= 255 and 1 <= args.ports <= 4
    if args.child:
        return measure(args)
    try:  # a fresh child does the measuring; this process never opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.time_limit)
    except subprocess.TimeoutExpired:
        sys.exit("pucch_f34_throughput: the run exceeded its time limit of %d s" % args.time_limit)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
