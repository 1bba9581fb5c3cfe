#!/usr/bin/env python3
"""Throughput probe of the estimator that estimates and compensates a carrier frequency offset (csrc/chest.hip: cfo_corr_kernel, chest_cfo_kernel)
and of the fused processor behind it.

Estimator legs: 273 PRB, four receive ports, L = 1, 2, 4, DM-RS on symbols (2, 11) and (2, 7, 11), `--jobs` device-resident jobs with the port and
layer hint, a grid of random samples per job. miphy_dmrs_pusch_estimate_cfo_batch against the yardstick miphy_dmrs_pusch_estimate_layers_batch with
ce_compact = 0 on the same jobs: it writes the same bytes (an estimate per symbol) and reads the DM-RS once, where the new entry point reads them
twice and launches twice.

Processor legs: one transport block on L = 2 and L = 4 (256QAM, four ports, DM-RS on 2, 7, 11, `--snr` dB, no offset applied, so that both decode and
the decoder does the same work), its grid copied `--slots` times; miphy_pusch_process_layers_cfo_batch against miphy_pusch_process_layers_batch_ex.

HIP events around `--iters` back-to-back calls after a warm-up of every leg; the legs are timed in turn `--rounds` times; median, fastest and slowest
round are printed, one JSON record per line. Run on the MI355X:  python tools/pusch_cfo_throughput.py [--jobs 1024] [--slots 256] [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pusch_layers_estimator_throughput import mask_all, tb_size, NPRB, MOD, NPT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--snr", type=float, default=40.0)
    ap.add_argument("--tb-bytes", type=int, default=13000, help="transport block bytes per layer")
    ap.add_argument("--no-processor", action="store_true")
    args = ap.parse_args()
    import torch
    import miphy
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    ctx = miphy.Context(0)
    nsc = NPRB * 12
    legs = []  # (name, run, slots per call, bytes the estimator stores per call)

    # ---- estimator
    n = args.jobs
    gen = torch.Generator(device="cuda").manual_seed(0)
    grid = torch.randn(n * NPT * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)
    ce = torch.zeros(n * 16 * 14 * nsc * 2, device="cuda", dtype=torch.float32)
    sc = torch.zeros(80 * n, dtype=torch.float32, device="cuda")
    cfo = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    idx = np.arange(n, dtype=np.uint64)
    for dmrs in ((2, 11), (2, 7, 11)):
        for nl in (1, 2, 4):
            fj = np.zeros(n, dtype=miphy.PuschChestCfoJob)
            j = fj["base"]
            j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = 1, 3, 77, 10 ** (3 / 20)
            j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, NPT, 0, 14, [0, 1, 2, 3]
            j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"] = 0, sum(1 << s for s in dmrs), NPRB
            mask_all(j)
            j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (NPT * 14 * nsc), idx * (16 * 14 * nsc), idx * 80
            fj["cfo_offset"] = 2 * idx
            d_cfo = torch.from_numpy(fj.view(np.uint8).copy()).cuda()
            d_lay = torch.from_numpy(np.ascontiguousarray(fj["base"]).view(np.uint8).copy()).cuda()
            tag, stored = "L%d_P4_dmrs%s" % (nl, "_".join(map(str, dmrs))), n * nl * NPT * 14 * nsc * 8
            legs.append(("estimate_%s_layers_entry_per_symbol" % tag, lambda d=d_lay, nl=nl: ctx.dmrs_pusch_estimate_layers_batch(d, grid, ce, sc, max_ports=NPT, max_layers=nl), n, stored))
            legs.append(("estimate_%s_cfo_entry" % tag, lambda d=d_cfo, nl=nl: ctx.dmrs_pusch_estimate_cfo_batch(d, grid, ce, sc, cfo, max_ports=NPT, max_layers=nl), n, stored))

    # ---- processor
    keep = []
    if not args.no_processor:
        import pusch_layers_cases as PL
        import pusch_layers_estimator_cases as E
        m, dmrs = args.slots, (2, 7, 11)
        for nl in (2, 4):
            tb_bytes = tb_size(args.tb_bytes * nl)
            c, tb, g1, _ = E.chain_tx(nl, NPT, MOD, tb_bytes, args.snr, dmrs, nprb=NPRB)
            ncb = miphy.sch_segmentation(tb_bytes, 1).nof_cbs
            grid_p = torch.from_numpy(np.nan_to_num(g1).reshape(-1)).cuda().repeat(m)
            pdus = np.zeros(m, dtype=miphy.PuschLayersPdu)
            p = pdus["base"]
            p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, E.SLOT, c["rnti"], c["n_id"], E.SCR
            p["tb_bytes"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb_bytes, MOD, NPT, 0, 14
            p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = 1, 0, 1, [0, 1, 2, 3], 1, 6
            p["dmrs_symbols_mask"], p["grid_nof_prb"] = sum(1 << s for s in dmrs), NPRB
            mask_all(p)
            pidx = np.arange(m, dtype=np.uint64)
            p["harq_cb_index"], p["grid_offset"], p["tb_offset"] = pidx * ncb, pidx * g1.size, pidx * tb_bytes
            pdus["nof_tx_layers"] = nl
            for name in ("plain", "cfo"):
                h = (torch.zeros(m * ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda"), torch.zeros(m * ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda"),
                     torch.zeros(m * ncb, dtype=torch.uint8, device="cuda"), torch.zeros(m * tb_bytes, dtype=torch.uint8, device="cuda"),
                     torch.zeros(m * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda"))
                scp = torch.zeros(80 * m, dtype=torch.float32, device="cuda")
                cfo_p = torch.zeros(2 * m, dtype=torch.float32, device="cuda")
                keep.append((name, nl, h[4], h[3], tb, m))
                if name == "plain":
                    run = lambda pdus=pdus, grid_p=grid_p, h=h, scp=scp: ctx.pusch_process_layers_batch_ex(pdus, None, grid_p, *h, scp, None, None)  # noqa: E731
                    stored = m * nl * NPT * nsc * 8
                else:
                    run = lambda pdus=pdus, grid_p=grid_p, h=h, scp=scp, cfo_p=cfo_p: ctx.pusch_process_layers_cfo_batch(pdus, None, grid_p, *h, scp, None, None, cfo_p)  # noqa: E731
                    stored = m * nl * NPT * 14 * nsc * 8
                legs.append(("process_L%d_P4_%s" % (nl, name), run, m, stored))

    for _, run, _, _ in legs:
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    for name, nl, res, out, tb, m in keep:
        ok = int((res.cpu().numpy().view(miphy.PuschResult)["tb_crc_ok"] != 0).sum())
        print(json.dumps({"processor": name, "layers": nl, "transport_blocks": m, "tb_crc_ok": ok, "tb_bytes": int(tb.size),
                          "first_block_equal": bool(np.array_equal(out[:tb.size].cpu().numpy(), tb))}))
    ms = {name: [] for name, _, _, _ in legs}
    for _ in range(args.rounds):
        for name, run, _, _ in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.iters)
    for name, _, slots, stored in legs:
        t = sorted(ms[name])
        med = t[len(t) // 2]
        print(json.dumps({"leg": name, "slots": slots, "ms_per_call_median": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
                          "slots_per_s": round(slots / (med * 1e-3)), "estimate_bytes_stored": stored,
                          "estimate_store_gbyte_per_s": round(stored / (med * 1e-3) / 1e9, 1)}))
    ctx.close()


if __name__ == "__main__":
    main()
