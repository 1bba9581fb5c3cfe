#!/usr/bin/env python3
"""Times miphy_pucch_process_batch on one slot of a loaded cell: a 273-PRB, 4-port grid (30 kHz), 1008 format-1 PDUs (84 PRBs x 12
cyclic shifts, 14 symbols, half of them with intra-slot hopping, 1 or 2 HARQ-ACK bits) and 128 format-2 PDUs (4 PRBs, 2 symbols,
11 bits). Device-resident jobs, as a slot batch would hold them. Prints one JSON line: microseconds per batch and PDUs per second.
Run:  python tools/pucch_throughput.py [--iters N]

--entry ex times miphy_pucch_process_batch_ex instead, which takes host jobs only; --jobs host gives the old entry point host jobs
too, for a like-for-like comparison. --long K,PRB,SYMBOLS turns the 128 format-2 PDUs into long ones (K bits above 11 on PRB x SYMBOLS,
polar-coded; --entry ex only) and --list L sets the list size of their decoder. With host jobs the line also has the host's time
per call (enqueue only)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
import miphy  # noqa: E402


def slot_jobs(long=None):
    jobs = []
    for prb in range(84):
        for ics in range(12):
            j = np.zeros((), miphy.PucchJob)
            j["format"], j["numerology"], j["slot"], j["nof_ports"] = 1, 1, 7, 4
            j["start_symbol"], j["nof_symbols"], j["intra_slot_hopping"] = 0, 14, prb % 2
            j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"], j["second_hop_prb"] = 0, 273, prb, 272 - prb
            j["initial_cyclic_shift"], j["time_domain_occ"], j["nof_harq_ack"], j["n_id"] = ics, ics % 3, 1 + ics % 2, 511
            j["grid_nprb"] = 273
            jobs.append(j)
    for k in range(128):
        j = np.zeros((), miphy.PucchJob)
        j["format"], j["numerology"], j["slot"], j["nof_ports"] = 2, 1, 7, 4
        j["start_symbol"], j["nof_symbols"], j["nof_prb"] = 12, 2, 4
        j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"] = 0, 273, 84 + (k % 40) * 4
        j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"], j["n_id"], j["n_id_0"], j["rnti"] = 4, 1, 6, 77, 901, 0x4601 + k
        j["grid_nprb"], j["payload_offset"], j["llr_offset"] = 273, 0, 512 * k
        if long:
            K, j["nof_prb"], j["nof_symbols"] = long
            j["start_symbol"] = 14 - long[2]
            j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"] = (5, 1, K - 6) if K <= 261 else (K - 355, 100, 255)
        jobs.append(j)
    jobs = np.array(jobs, miphy.PucchJob)
    stride = max(11, long[0]) if long else 11
    jobs["payload_offset"] = stride * np.arange(len(jobs))
    return jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--entry", choices=("old", "ex"), default="old")
    ap.add_argument("--jobs", choices=("device", "host"), default=None, help="default: device for --entry old; --entry ex takes host jobs only")
    ap.add_argument("--long", default=None, help="K,PRB,SYMBOLS of the 128 format-2 PDUs, K > 11 (--entry ex)")
    ap.add_argument("--list", type=int, default=1, help="list size of the polar decoder (--entry ex)")
    a = ap.parse_args()
    long = tuple(int(x) for x in a.long.split(",")) if a.long else None
    host = a.entry == "ex" or a.jobs == "host"
    if a.entry == "ex" and a.jobs == "device":
        ap.error("--entry ex takes host jobs only")
    if long and a.entry != "ex":
        ap.error("--long needs --entry ex")
    ctx = miphy.Context(0)
    jobs = slot_jobs(long)
    n = len(jobs)
    rng = np.random.default_rng(1)
    grid = torch.from_numpy((rng.standard_normal(4 * 14 * 273 * 12) + 1j * rng.standard_normal(4 * 14 * 273 * 12)).astype(np.complex64)).cuda()
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
    pay = torch.zeros(int(jobs["payload_offset"][-1]) + 512, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * miphy.PucchResult.itemsize, dtype=torch.uint8, device="cuda")
    llr = torch.zeros(512 * 128, dtype=torch.int8, device="cuda")
    if a.entry == "ex":
        def call():
            ctx.pucch_process_batch_ex(jobs, a.list, grid, pay, res, llr)
    else:
        ctx.pucch_process_batch(jobs, grid, pay, res, llr)  # host jobs once: validated, MIPHY_EINVAL raises
        j = jobs if host else jobs_d

        def call():
            ctx.pucch_process_batch(j, grid, pay, res, llr)
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    w0 = time.perf_counter()
    for _ in range(a.iters):
        call()
    w1 = time.perf_counter()
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / a.iters
    out = {"pdus": n, "format1": int((jobs["format"] == 1).sum()), "format2": int((jobs["format"] == 2).sum()),
           "us_per_batch": round(us, 2), "pdus_per_s": round(n / us * 1e6)}
    if a.entry == "ex" or a.jobs:
        out.update(entry=a.entry, jobs="host" if host else "device")
    if host:
        out["host_us_per_call"] = round((w1 - w0) * 1e6 / a.iters, 2)
    if a.entry == "ex":
        out.update(long=a.long, list=a.list, valid=int((res.cpu().numpy().view(miphy.PucchResult)["status"] == 1).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
