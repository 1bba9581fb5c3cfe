#!/usr/bin/env python3
"""Throughput probe of miphy_uci_decode_batch (csrc/uci.hip): fields per second for a slot-sized batch (16 fields) and a large one (65536),
timed with HIP events around `--iters` back-to-back launches with device-resident jobs (no staging copy in the timed region), after a
warm-up. Fields: K = 11 (the most codewords per lane) or a mix of every K, Qm = 2, E = 64 soft bits unless --E is given.
Run on the MI355X:  python tools/uci_throughput.py [--iters 200] [--E 64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--E", type=int, default=64)
    args = ap.parse_args()
    import torch
    import miphy
    ctx = miphy.Context(0)
    rng = np.random.default_rng(0)
    out = []
    for mix in ("K11", "mixed"):
        for n in (16, 65536):
            K = np.full(n, 11) if mix == "K11" else rng.integers(3, 12, n)
            jobs = np.zeros(n, miphy.UciFieldJob)
            jobs["nof_bits"], jobs["mod"], jobs["nof_llr"] = K, 2, args.E
            jobs["llr_offset"] = np.arange(n, dtype=np.uint64) * args.E
            jobs["payload_offset"] = np.arange(n, dtype=np.uint64) * 11
            llr = torch.from_numpy(rng.integers(-60, 61, n * args.E).astype(np.int8)).cuda()
            pay = torch.zeros(n * 11, dtype=torch.uint8, device="cuda")
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            jd = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
            for _ in range(10):
                ctx.uci_decode_batch(jd, llr, pay, st)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                ctx.uci_decode_batch(jd, llr, pay, st)
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / args.iters
            out.append({"fields": n, "K": mix, "E": args.E, "us_per_launch": round(us, 2), "fields_per_s": round(n / us * 1e6)})
            print(json.dumps(out[-1]))
    ctx.close()


if __name__ == "__main__":
    main()
