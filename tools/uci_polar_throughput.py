#!/usr/bin/env python3
"""Throughput probe of miphy_uci_polar_decode_batch (csrc/uci_polar.hip) next to its yardstick, miphy_polar_decode_batch with the same
single code and as many codewords as the fields have segments. Batches of 16, 1024 and 65536 fields of one shape, and a mixed draw of
shapes. The jobs are host memory, so a call has a host part (framing, code construction or cache, staging) and a device part (the
staging copies and the kernels); they are reported separately, each as the median of `--reps` runs:
  host_us:   time until the call returns, stream idle before it;
  device_us: HIP events around the call's work, recorded behind a spin kernel that keeps the stream busy while the host enqueues, so
             the events see the copies and kernels back to back and not the host's enqueue time.
The mixed draw of 65536 fields constructs tens of thousands of codes per call and stages hundreds of MiB of tables; it runs with
three repetitions.
Kernel time proper comes from a kernel trace, in a run of its own per configuration (the trace slows the host):
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/uci_polar_throughput.py --trace A E FIELDS [--reps 6]
makes --reps calls of each entry point and nothing else; the sum of the durations of uci_polar_decode_kernel (and of
polar_decode_kernel) in OUT's kernel statistics, divided by --reps, is the kernel time of one call.
--list L (2, 4 or 8) measures miphy_uci_polar_decode_list_batch at that list size instead (uci_polar_scl_kernel for the fields of 20
bits and more); the same command without it gives the list-size-1 figures to put next to them. --shape A E keeps one shape.
Run on the MI355X:  python tools/uci_polar_throughput.py [--reps 15] [--list L] [--shape A E]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))

SHAPES = [(20, 128), (64, 256), (500, 1100), (1706, 3500)]


def draw_mixed(rng, n, miphy):
    A, E = np.zeros(n, np.int64), np.zeros(n, np.int64)
    i = 0
    while i < n:
        a = int(rng.integers(12, 120)) if rng.random() < 0.5 else int(round(np.exp(rng.uniform(np.log(12), np.log(1706)))))
        e = int(rng.integers(a + 16, 6 * a + 400))
        try:
            miphy.uci_polar_info(a, e)
        except RuntimeError:
            continue
        A[i], E[i] = a, e
        i += 1
    return A, E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 1024, 65536])
    ap.add_argument("--mixed-max", type=int, default=65536, help="largest batch that also runs the mixed draw")
    ap.add_argument("--list", type=int, default=1, choices=(1, 2, 4, 8), help="list size; above 1 the list entry point is measured")
    ap.add_argument("--shape", type=int, nargs=2, metavar=("A", "E"), help="this shape only, no mixed draw")
    ap.add_argument("--trace", type=int, nargs=3, metavar=("A", "E", "FIELDS"), help="one configuration, --reps calls of each entry point, "
                    "no timing: the run to put under a kernel trace")
    args = ap.parse_args()
    import torch
    import miphy
    ctx = miphy.Context(0)
    rng = np.random.default_rng(0)
    # cycles of torch.cuda._sleep per millisecond
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = 10_000_000 / e0.elapsed_time(e1)

    def measure(call, reps):
        if args.trace:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            return 0.0, 1.0
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        host, dev = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            host.append((time.perf_counter() - t) * 1e6)
        torch.cuda.synchronize()
        spin_ms = max(2.0, 3.0 * float(np.median(host)) / 1e3)
        for _ in range(reps):
            torch.cuda._sleep(int(spin_ms * cycles_per_ms))
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(host)), float(np.median(dev))

    for n in ([args.trace[2]] if args.trace else args.sizes):
        for shape in ([tuple(args.trace[:2])] if args.trace else [tuple(args.shape)] if args.shape else SHAPES + (["mixed"] if n <= args.mixed_max else [])):
            reps = min(args.reps, 3) if shape == "mixed" and n > 1024 else args.reps
            if shape == "mixed":
                A, E = draw_mixed(rng, n, miphy)
            else:
                A, E = np.full(n, shape[0]), np.full(n, shape[1])
            jobs = np.zeros(n, miphy.UciPolarJob)
            jobs["nof_bits"], jobs["nof_llr"] = A, E
            jobs["llr_offset"] = np.concatenate([[0], np.cumsum(E)[:-1]])
            jobs["payload_offset"] = np.concatenate([[0], np.cumsum(A)[:-1]])
            llr = torch.from_numpy(rng.integers(-60, 61, int(E.sum())).astype(np.int8)).cuda()
            pay = torch.zeros(int(A.sum()), dtype=torch.uint8, device="cuda")
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            if args.list > 1:
                host_us, dev_us = measure(lambda: ctx.uci_polar_decode_list_batch(jobs, args.list, llr, pay, st), reps)
            else:
                host_us, dev_us = measure(lambda: ctx.uci_polar_decode_batch(jobs, llr, pay, st), reps)
            row = {"list": args.list, "fields": n, "reps": reps, "A": int(A[0]) if shape != "mixed" else "mixed", "E": int(E[0]) if shape != "mixed" else "mixed",
                   "host_us": round(host_us, 1), "device_us": round(dev_us, 1), "pieces": int(miphy.lib().miphy_debug_uci_polar_pieces()),
                   "fields_per_s_device": round(n / dev_us * 1e6)}
            if shape != "mixed":  # the yardstick: the same code, one codeword per segment, tables cached on the device
                f = miphy.uci_polar_info(*shape)
                code = miphy.PolarCode(int(f["K_r"]), int(f["E_r"]), 10, 1)
                ncw = n * int(f["C"])
                msg = torch.zeros(ncw * int(f["K_r"]), dtype=torch.uint8, device="cuda")
                ref_host, ref_dev = measure(lambda: ctx.polar_decode_batch(code, ncw, llr, msg), reps)
                row.update({"segments": int(f["C"]), "polar_decode_batch_host_us": round(ref_host, 1), "polar_decode_batch_device_us": round(ref_dev, 1),
                            "device_ratio": round(dev_us / ref_dev, 2)})
            if not args.trace:
                print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
