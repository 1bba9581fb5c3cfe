#!/usr/bin/env python3
"""Times the PDSCH modulator and the PDSCH processor on one codeword and L = 1, 2, 4 layers against the one-layer entry points, on the same
allocation in the same session: 273 PRB, 256QAM (--mod 8, the default; --mod 6 takes the general element loop), 14 symbols (DM-RS on symbol 2, two CDM groups without data: 42 588 data REs per layer), a batch
of --batch transmissions per call, one stream, calls back to back between two device events.
- "modulate": miphy_pdsch_modulate_batch (one layer per job) and miphy_pdsch_modulate_layers_batch at L = 1, 2, 4 on random codewords, with host
  jobs (validated and staged by every call: at this size the host's work per job outlasts the device's, so the figure is the enqueue rate)
  and with device-resident jobs (two launches per call: the device's rate). Per call, per mapped (RE, layer), and the bytes the modulator must
  store (8 per mapped (RE, layer)) over the call time against the HBM rates of the MI355X (8 TB/s peak, about 6.3 TB/s achievable). The call
  time includes the scrambling-sequence kernel, so this is the entry point's store rate, not the mapping kernel's alone.
- "process": miphy_pdsch_process_batch and miphy_pdsch_process_layers_batch at L = 1, 2, 4 (encoder, modulator, DM-RS). The transport block is
  3/4 of the codeword, capped at the encoder's 52 codeblocks of base graph 1 (54 753 bytes): the code rate falls with L and is printed.
Every figure is the median of --reps repetitions of --iters calls, the variants alternating; the spread (min .. max) is printed with it. One
JSON line per variant. There is no CPU path: without a device this fails.
- --mapping ascending | interleaved2 | interleaved4 times, instead of the above, miphy_pdsch_modulate_mapped_batch next to
  miphy_pdsch_modulate_layers_batch (the yardstick) at L = 1, 2, 4 with device-resident jobs: without lists (the same bytes) and with every job's
  PRBs in the interleaved order of TS 38.211 7.3.1.6 at bundle size 2 or 4 (miphy_vrb_to_prb_list). Kernel times proper:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/pdsch_layers_throughput.py --mapping interleaved2 --trace --reps 2
- --precoding PORTS times, instead of the above, miphy_pdsch_modulate_precoded_batch onto PORTS antenna ports next to
  miphy_pdsch_modulate_layers_batch (the yardstick) at every L of 1, 2, 4 that PORTS can carry, with device-resident jobs and weights (every job its own
  matrices, PRGs of --prg-size PRBs), the two alternating. Per call, per stored (RE, port), and the bytes stored (8 per (RE, port); the yardstick
  stores 8 per (RE, layer)). With --trace the yardstick is left out, so that a kernel trace holds pdsch_mod_precoded_kernel alone.
- --codewords times, instead of the above, miphy_pdsch_modulate_codewords_batch on two codewords -- L = 5 at (256QAM, 256QAM), L = 8 at (256QAM,
  256QAM) and L = 8 at (256QAM, 16QAM) -- next to its yardstick: two back-to-back miphy_pdsch_modulate_layers_batch calls with L0 and L1 layers on the
  same allocation and the same grid ports, which are the stores the new call makes without the shared symbol setup and launch pair. Device-resident
  jobs, the two alternating. Per call, per mapped (RE, layer), and the bytes stored.
Run:  python tools/pdsch_layers_throughput.py [--batch N] [--iters N] [--reps R] [--mod 1|2|4|6|8] [--mapping M | --precoding PORTS [--prg-size S] | --codewords]
      [--trace]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
import miphy  # noqa: E402

NPRB, NSC = 273, 273 * 12
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes per second
TB_MAX_BYTES = 54753                       # 52 codeblocks of base graph 1


def rb_words():
    w = np.zeros(5, dtype=np.uint64)
    for r in range(NPRB):
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def mod_jobs(n, L, layered, mod):
    """n transmissions on L layers each; the one-layer form (layered = False, L = 1) for miphy_pdsch_modulate_batch."""
    jobs = np.zeros(n, dtype=miphy.PdschModLayersJob if layered else miphy.PdschModJob)
    b = jobs["base"] if layered else jobs
    b["rnti"], b["n_id"], b["scaling"], b["mod"], b["nof_symbols"] = 0x4601 + np.arange(n), 935, 0.7943282, mod, 14
    b["dmrs_type"], b["nof_cdm_groups_without_data"], b["dmrs_symbols_mask"] = 1, 2, 1 << 2
    b["grid_nof_prb"], b["bwp_size_rb"], b["rb_mask"] = NPRB, NPRB, rb_words()
    nre = miphy.pdsch_mod_nof_re(b[0])
    b["nof_bits"] = nre * L * mod
    b["cw_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(nre * L * mod)
    b["grid_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(L * 14 * NSC)
    if layered:
        jobs["nof_layers"], jobs["ports"] = L, np.arange(4) % L
    return jobs, nre


def proc_pdus(n, L, layered, mod):
    pdus = np.zeros(n, dtype=miphy.PdschLayersPdu if layered else miphy.PdschPdu)
    b = pdus["base"] if layered else pdus
    b["slot_in_frame"], b["rnti"], b["n_id"], b["dmrs_scrambling_id"], b["tbs_lbrm_bytes"] = 7, 0x4601 + np.arange(n), 935, 42, 3168
    b["bg"], b["mod"], b["nof_symbols"], b["nof_cdm_groups_without_data"], b["dmrs_symbols_mask"] = 1, mod, 14, 2, 1 << 2
    b["grid_nof_prb"], b["bwp_size_rb"], b["rb_mask"] = NPRB, NPRB, rb_words()
    nre = miphy.pdsch_pdu_nof_re(b[0])
    tb_bytes = min(TB_MAX_BYTES, nre * L * mod * 3 // 4 // 8)
    b["tb_bytes"] = tb_bytes
    b["tb_offset"] = np.arange(n, dtype=np.uint64) * np.uint64((tb_bytes + 15) // 16 * 16)
    b["grid_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(L * 14 * NSC)
    if layered:
        pdus["nof_layers"], pdus["ports"] = L, np.arange(4) % L
    return pdus, nre, tb_bytes


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def measure(fns, iters, reps):
    """Median and spread in microseconds per call of each function, alternating them."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t[k].append(timed(fn, iters))
    return [(float(np.median(v)), float(min(v)), float(max(v))) for v in t]


def mapped_section(ctx, a, grid, gen):
    """--mapping: per L the layered entry point (the yardstick of the session), the mapped entry point without lists (nof_prb = 0: the same bytes)
    and, unless the mapping is "ascending", the mapped entry point with every job's list in the interleaved order of TS 38.211 7.3.1.6 at bundle
    size 2 or 4 (every job its own copy of the list) -- device-resident jobs and lists, the three alternating."""
    n, mod = a.batch, a.mod
    bundle = {"ascending": 0, "interleaved2": 2, "interleaved4": 4}[a.mapping]
    fns, meta = [], []
    for L in (1, 2, 4):
        jobs, nre = mod_jobs(n, L, True, mod)
        cw = torch.randint(0, 2, (n * nre * L * mod,), dtype=torch.uint8, device="cuda", generator=gen)
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        fns.append(lambda j=d_jobs, cw=cw: ctx.pdsch_modulate_layers_batch(j, cw, grid))
        meta.append(("layers_entry", "ascending", L, nre))
        for mapping in ([] if a.trace and bundle else ["ascending"]) + ([a.mapping] if bundle else []):
            mj = np.zeros(n, dtype=miphy.PdschModMappedJob)
            mj["layers"] = jobs
            lists = None
            if mapping != "ascending":
                one = miphy.vrb_to_prb_list(bundle, 0, NPRB, 0)[0]
                mj["prb_list_offset"], mj["nof_prb"] = np.arange(n) * one.size, one.size
                lists = torch.from_numpy(np.tile(one, n).view(np.int16)).cuda()
            d_mj = torch.from_numpy(mj.view(np.uint8).copy()).cuda()
            fns.append(lambda j=d_mj, ls=lists, cw=cw: ctx.pdsch_modulate_mapped_batch(j, ls, cw, grid))
            meta.append(("mapped_entry", mapping, L, nre))
    for (name, mapping, L, nre), (us, lo, hi) in zip(meta, measure(fns, a.iters, a.reps)):
        mapped = n * nre * L
        print(json.dumps({"what": "modulate", "entry": name, "mapping": mapping, "jobs": "device", "layers": L, "mod": mod, "batch": n, "re_per_layer": nre,
                          "us_per_call": round(us, 2), "us_per_call_spread": [round(lo, 2), round(hi, 2)], "ps_per_re_layer": round(us * 1e6 / mapped, 2),
                          "store_GBps": round(mapped * 8 / us * 1e-3, 1)}), flush=True)


def precoded_section(ctx, a, gen):
    """--precoding: per L the layered entry point (the yardstick of the session) and the precoded entry point onto a.precoding antenna ports, without
    lists -- device-resident jobs and weights, alternating."""
    n, mod, P = a.batch, a.mod, a.precoding
    grid = torch.zeros(n * max(P, 4) * 14 * NSC, dtype=torch.complex64, device="cuda")
    nof_prg = -(-NPRB // a.prg_size)
    fns, meta = [], []
    for L in (1, 2, 4):
        if L > P:
            continue
        jobs, nre = mod_jobs(n, L, True, mod)
        cw = torch.randint(0, 2, (n * nre * L * mod,), dtype=torch.uint8, device="cuda", generator=gen)
        if not a.trace:
            d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
            fns.append(lambda j=d_jobs, cw=cw: ctx.pdsch_modulate_layers_batch(j, cw, grid))
            meta.append(("layers_entry", L, L, nre))
        pj = np.zeros(n, dtype=miphy.PdschModPrecodedJob)
        pj["mapped"]["layers"] = jobs
        pj["mapped"]["layers"]["base"]["grid_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(P * 14 * NSC)
        pc = pj["precoding"]
        pc["nof_layers"], pc["nof_ports"], pc["ports"], pc["prg_size"], pc["nof_prg"] = L, P, np.arange(16), a.prg_size, nof_prg
        pc["weights_offset"] = np.arange(n) * (nof_prg * P * L)
        w = torch.view_as_complex(torch.rand((n * nof_prg * P * L, 2), dtype=torch.float32, device="cuda", generator=gen) - 0.5)
        d_pj = torch.from_numpy(pj.view(np.uint8).copy()).cuda()
        fns.append(lambda j=d_pj, w=w, cw=cw: ctx.pdsch_modulate_precoded_batch(j, None, w, cw, grid))
        meta.append(("precoded_entry", L, P, nre))
    for (name, L, ports, nre), (us, lo, hi) in zip(meta, measure(fns, a.iters, a.reps)):
        stored = n * nre * ports
        print(json.dumps({"what": "modulate", "entry": name, "jobs": "device", "layers": L, "ports": ports, "prg_size": a.prg_size, "mod": mod, "batch": n,
                          "re_per_layer": nre, "us_per_call": round(us, 2), "us_per_call_spread": [round(lo, 2), round(hi, 2)],
                          "ps_per_re_port": round(us * 1e6 / stored, 2), "store_GBps": round(stored * 8 / us * 1e-3, 1)}), flush=True)


def codewords_section(ctx, a, gen):
    """--codewords: per (L, mod0, mod1) the yardstick (two layered calls, L0 and L1 layers) and the codewords entry point, device-resident jobs,
    alternating."""
    n = a.batch
    grid = torch.zeros(n * 8 * 14 * NSC, dtype=torch.complex64, device="cuda")
    goff = np.arange(n, dtype=np.uint64) * np.uint64(8 * 14 * NSC)
    fns, meta = [], []
    for L, mods in ((5, (8, 8)), (8, (8, 8)), (8, (8, 4))):
        L0, L1 = L // 2, L - L // 2
        halves, cws = [], []
        for Lq, mod, first in ((L0, mods[0], 0), (L1, mods[1], L0)):
            jobs, nre = mod_jobs(n, Lq, True, mod)
            jobs["base"]["grid_offset"], jobs["ports"] = goff, first + np.arange(4) % Lq
            halves.append(jobs)
            cws.append(torch.randint(0, 2, (n * nre * Lq * mod,), dtype=torch.uint8, device="cuda", generator=gen))
        cw = torch.cat(cws)
        d0, d1 = (torch.from_numpy(h.view(np.uint8).copy()).cuda() for h in halves)
        fns.append(lambda d0=d0, d1=d1, c0=cws[0], c1=cws[1]: (ctx.pdsch_modulate_layers_batch(d0, c0, grid), ctx.pdsch_modulate_layers_batch(d1, c1, grid)))
        meta.append(("two_layers_calls", L, mods, nre))
        cj = np.zeros(n, dtype=miphy.PdschModCodewordsJob)
        cj["mapped"]["layers"] = halves[0]
        cj["nof_layers"], cj["ports"], cj["mod1"] = L, np.arange(8), mods[1]
        cj["nof_bits1"] = halves[1]["base"]["nof_bits"]
        cj["cw1_offset"] = np.uint64(cws[0].numel()) + halves[1]["base"]["cw_offset"]
        d_cj = torch.from_numpy(cj.view(np.uint8).copy()).cuda()
        fns.append(lambda j=d_cj, cw=cw: ctx.pdsch_modulate_codewords_batch(j, None, cw, grid))
        meta.append(("codewords_entry", L, mods, nre))
    for (name, L, mods, nre), (us, lo, hi) in zip(meta, measure(fns, a.iters, a.reps)):
        mapped = n * nre * L
        print(json.dumps({"what": "modulate", "entry": name, "jobs": "device", "layers": L, "mods": list(mods), "batch": n, "re_per_layer": nre,
                          "us_per_call": round(us, 2), "us_per_call_spread": [round(lo, 2), round(hi, 2)], "ps_per_re_layer": round(us * 1e6 / mapped, 2),
                          "store_GBps": round(mapped * 8 / us * 1e-3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mod", type=int, default=8, choices=(1, 2, 4, 6, 8), help="bits per symbol")
    ap.add_argument("--mapping", choices=("ascending", "interleaved2", "interleaved4"), default=None,
                    help="time miphy_pdsch_modulate_mapped_batch next to miphy_pdsch_modulate_layers_batch instead (device jobs, L = 1, 2, 4)")
    ap.add_argument("--trace", action="store_true",
                    help="with --precoding: leave out the yardstick; with --mapping interleaved2 / interleaved4: leave out the mapped entry point without lists, so that a kernel trace of the run "
                         "holds pdsch_mod_mapped_kernel at that mapping alone, next to pdsch_mod_layers_kernel")
    ap.add_argument("--precoding", type=int, default=None, metavar="PORTS",
                    help="time miphy_pdsch_modulate_precoded_batch onto PORTS (1..16) antenna ports next to miphy_pdsch_modulate_layers_batch instead (device jobs)")
    ap.add_argument("--prg-size", type=int, default=4, help="with --precoding: PRBs per PRG")
    ap.add_argument("--codewords", action="store_true",
                    help="time miphy_pdsch_modulate_codewords_batch on two codewords (L = 5 and 8) next to two miphy_pdsch_modulate_layers_batch calls instead (device jobs)")
    a = ap.parse_args()
    n, mod = a.batch, a.mod
    ctx = miphy.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    if a.precoding is not None:
        precoded_section(ctx, a, gen)
        return
    if a.codewords:
        codewords_section(ctx, a, gen)
        return
    grid = torch.zeros(n * 4 * 14 * NSC, dtype=torch.complex64, device="cuda")
    if a.mapping is not None:
        mapped_section(ctx, a, grid, gen)
        return
    variants = [("one_layer_entry", 1, False), ("layers_entry", 1, True), ("layers_entry", 2, True), ("layers_entry", 4, True)]

    # ---- modulator alone
    fns, meta = [], []
    for name, L, layered in variants:
        jobs, nre = mod_jobs(n, L, layered, mod)
        cw = torch.randint(0, 2, (n * nre * L * mod,), dtype=torch.uint8, device="cuda", generator=gen)
        call = ctx.pdsch_modulate_layers_batch if layered else ctx.pdsch_modulate_batch
        for where, j in (("host", jobs), ("device", torch.from_numpy(jobs.view(np.uint8).copy()).cuda())):
            fns.append(lambda call=call, j=j, cw=cw: call(j, cw, grid))
            meta.append((name, where, L, nre))
    for (name, where, L, nre), (us, lo, hi) in zip(meta, measure(fns, a.iters, a.reps)):
        mapped = n * nre * L
        print(json.dumps({"what": "modulate", "entry": name, "jobs": where, "layers": L, "mod": mod, "batch": n, "re_per_layer": nre, "us_per_call": round(us, 2),
                          "us_per_call_spread": [round(lo, 2), round(hi, 2)], "ps_per_re_layer": round(us * 1e6 / mapped, 2),
                          "store_GBps": round(mapped * 8 / us * 1e-3, 1), "share_of_hbm_achievable": round(mapped * 8 / (us * 1e-6) / HBM_ACHIEVABLE, 4),
                          "share_of_hbm_peak": round(mapped * 8 / (us * 1e-6) / HBM_PEAK, 4)}), flush=True)

    # ---- processor
    fns, meta = [], []
    for name, L, layered in variants:
        pdus, nre, tb_bytes = proc_pdus(n, L, layered, mod)
        tb = torch.randint(0, 256, (n * ((tb_bytes + 15) // 16 * 16) + 16,), dtype=torch.uint8, device="cuda", generator=gen)
        call = ctx.pdsch_process_layers_batch if layered else ctx.pdsch_process_batch
        fns.append(lambda call=call, pdus=pdus, tb=tb: call(pdus, tb, grid))
        meta.append((name, L, nre, tb_bytes))
    for (name, L, nre, tb_bytes), (us, lo, hi) in zip(meta, measure(fns, a.iters, a.reps)):
        mapped = n * nre * L
        print(json.dumps({"what": "process", "entry": name, "layers": L, "mod": mod, "batch": n, "re_per_layer": nre, "tb_bytes": tb_bytes,
                          "code_rate": round(tb_bytes * 8 / (nre * L * mod), 3), "us_per_call": round(us, 2), "us_per_call_spread": [round(lo, 2), round(hi, 2)],
                          "ps_per_re_layer": round(us * 1e6 / mapped, 2), "tb_Gbps": round(n * tb_bytes * 8 / us * 1e-3, 1)}), flush=True)


if __name__ == "__main__":
    main()
