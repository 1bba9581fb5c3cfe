#!/usr/bin/env python3
"""Throughput probe of the layered DM-RS estimator (csrc/chest.hip: chest_layers_kernel) and of the fused processor on two and four layers.

Estimator legs: 273 PRB, DM-RS on symbol 2, four receive ports, the compact estimate, `--jobs` slots per call, device-resident jobs with the port and
layer hint, a grid of random samples per job. miphy_dmrs_pusch_estimate_layers_batch on L = 2 and L = 4 against miphy_dmrs_pusch_estimate_batch on the
same jobs: the latter runs one workgroup per layer, the former one per CDM group (MIPHY_LIBRARY may name another build of the library for an A-B; the
legs of entry points it lacks are left out).

Processor legs: one transport block on L = 2 and L = 4 (256QAM, four ports, `--snr` dB, the transmitter of tests/pusch_layers_estimator_cases.py),
its grid copied `--slots` times so that every PDU reads a grid and HARQ buffers of its own; miphy_pusch_process_layers_batch end to end beside its
three stages called one after the other, in slots/s and information Gbit/s, with the number of transport blocks whose CRC passed.

HIP events around `--iters` back-to-back calls after a warm-up of every leg; the legs are timed in turn `--rounds` times; median, fastest and slowest
round are printed. Run on the MI355X:  python tools/pusch_layers_estimator_throughput.py [--jobs 1024] [--slots 256] [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NPRB, MOD, NPT = 273, 8, 4


def mask_all(j):
    for r in range(NPRB):
        j["rb_mask"][:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)


def tb_size(target_bytes):
    """The TS 38.214 transport block size (base graph 1, several codeblocks) at or above the target: codeblock payloads are whole bytes."""
    b = target_bytes
    while True:
        bits = 8 * b + 24
        ncb = -(-bits // (8448 - 24))
        if bits % (8 * ncb) == 0:
            return b
        b += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--snr", type=float, default=40.0)
    ap.add_argument("--tb-bytes", type=int, default=13000, help="transport block bytes per layer (the host encoder stops at 52 codeblocks)")
    ap.add_argument("--no-processor", action="store_true")
    args = ap.parse_args()
    import torch
    import miphy
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    ctx = miphy.Context(0)
    nsc = NPRB * 12
    legs = []  # (name, run, slots per call, information bits per call)

    # ---- estimator
    n = args.jobs
    gen = torch.Generator(device="cuda").manual_seed(0)
    grid = torch.randn(n * NPT * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)
    ce = torch.zeros(n * 16 * nsc * 2, device="cuda", dtype=torch.float32)
    sc = torch.zeros(80 * n, dtype=torch.float32, device="cuda")
    for nl in (2, 4):
        j = np.zeros(n, dtype=miphy.PuschChestJob)
        j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = 1, 3, 77, 10 ** (3 / 20)
        j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"], j["rx_ports"] = nl, NPT, 0, 14, [0, 1, 2, 3]
        j["ce_compact"], j["symbols_mask"], j["grid_nof_prb"] = 1, 1 << 2, NPRB
        mask_all(j)
        idx = np.arange(n, dtype=np.uint64)
        j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (NPT * 14 * nsc), idx * (16 * nsc), idx * 80
        d = torch.from_numpy(j.view(np.uint8).copy()).cuda()
        legs.append(("estimate_L%d_P4_per_layer_entry" % nl, lambda d=d, nl=nl: ctx.dmrs_pusch_estimate_batch(d, grid, ce, sc, max_ports=NPT, max_layers=nl), n, 0))
        if hasattr(miphy.lib(), "miphy_dmrs_pusch_estimate_layers_batch"):
            legs.append(("estimate_L%d_P4_layers_entry" % nl, lambda d=d, nl=nl: ctx.dmrs_pusch_estimate_layers_batch(d, grid, ce, sc, max_ports=NPT, max_layers=nl), n, 0))

    # ---- processor
    keep = []
    if not args.no_processor and hasattr(miphy.lib(), "miphy_pusch_process_layers_batch"):
        import pusch_layers_cases as PL
        import pusch_layers_estimator_cases as E
        m = args.slots
        for nl in (2, 4):
            tb_bytes = tb_size(args.tb_bytes * nl)
            c, tb, g1, _ = E.chain_tx(nl, NPT, MOD, tb_bytes, args.snr, (2,), nprb=NPRB)
            ncb = miphy.sch_segmentation(tb_bytes, 1).nof_cbs
            grid_p = torch.from_numpy(np.nan_to_num(g1).reshape(-1)).cuda().repeat(m)
            rb, dm = PL.masks(c)
            pdus = np.zeros(m, dtype=miphy.PuschLayersPdu)
            p = pdus["base"]
            p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, E.SLOT, c["rnti"], c["n_id"], E.SCR
            p["tb_bytes"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb_bytes, MOD, NPT, 0, 14
            p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = 1, 0, 1, [0, 1, 2, 3], 1, 6
            p["dmrs_symbols_mask"], p["grid_nof_prb"] = 1 << 2, NPRB
            mask_all(p)
            idx = np.arange(m, dtype=np.uint64)
            p["harq_cb_index"], p["grid_offset"], p["tb_offset"] = idx * ncb, idx * g1.size, idx * tb_bytes
            pdus["nof_tx_layers"] = nl
            soft = torch.zeros(m * ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
            msgs = torch.zeros(m * ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
            crc = torch.zeros(m * ncb, dtype=torch.uint8, device="cuda")
            out = torch.zeros(m * tb_bytes, dtype=torch.uint8, device="cuda")
            res = torch.zeros(m * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
            scp = torch.zeros(80 * m, dtype=torch.float32, device="cuda")
            # the three stages on the processor's layouts
            cj = np.zeros(m, dtype=miphy.PuschChestJob)
            cj["numerology"], cj["slot_in_frame"], cj["scrambling_id"], cj["scaling"] = 1, E.SLOT, E.SCR, np.float32(10.0) ** np.float32(3.0 / 20.0)
            cj["nof_tx_layers"], cj["nof_rx_ports"], cj["first_symbol"], cj["nof_symbols"], cj["rx_ports"] = nl, NPT, 0, 14, [0, 1, 2, 3]
            cj["ce_compact"], cj["symbols_mask"], cj["grid_nof_prb"] = 1, 1 << 2, NPRB
            mask_all(cj)
            cj["grid_offset"], cj["ce_offset"], cj["scalars_offset"] = idx * g1.size, idx * (nl * NPT * nsc), idx * 80
            dj = np.zeros(m, dtype=miphy.PuschDemodLayersJob)
            dj[:] = PL.demod_job(miphy, dict(c, compact=True))
            nllr = int(dj[0]["base"]["nof_llr"])
            stride = (nllr + 15) & ~15
            dj["base"]["grid_offset"], dj["base"]["ce_offset"], dj["base"]["scalars_offset"], dj["base"]["llr_offset"] = cj["grid_offset"], cj["ce_offset"], idx * 80, idx * stride
            td = np.zeros(m, dtype=miphy.PuschTbDesc)
            td["bg"], td["mod"], td["nof_layers"], td["new_data"], td["use_early_stop"], td["nof_ldpc_iterations"] = 1, MOD, nl, 1, 1, 6
            td["nof_ch_symbols"], td["tb_bytes"], td["harq_cb_index"], td["llr_offset"], td["tb_offset"] = nllr // MOD, tb_bytes, idx * ncb, idx * stride, idx * tb_bytes
            ce_p = torch.zeros(m * nl * NPT * nsc * 2, device="cuda", dtype=torch.float32)
            llr_p = torch.zeros(m * stride, dtype=torch.int8, device="cuda")
            h = (soft, msgs, crc, out, res)
            keep.append((nl, res, out, tb, m))

            def fused(pdus=pdus, grid_p=grid_p, h=h, scp=scp):
                ctx.pusch_process_layers_batch(pdus, grid_p, *h, scp)

            def est(cj=cj, grid_p=grid_p, ce_p=ce_p, scp=scp):
                ctx.dmrs_pusch_estimate_layers_batch(cj, grid_p, ce_p, scp)

            def dem(dj=dj, grid_p=grid_p, ce_p=ce_p, scp=scp, llr_p=llr_p):
                ctx.pusch_demodulate_layers_batch(dj, grid_p, ce_p, scp, llr_p)

            def dec(td=td, llr_p=llr_p, h=h):
                ctx.pusch_decode_batch(td, llr_p, *h)

            bits = m * tb_bytes * 8
            legs += [("process_L%d_P4_fused" % nl, fused, m, bits), ("process_L%d_P4_stage_estimate" % nl, est, m, 0),
                     ("process_L%d_P4_stage_demodulate" % nl, dem, m, 0), ("process_L%d_P4_stage_decode" % nl, dec, m, bits)]

    for _, run, _, _ in legs:
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    for nl, res, out, tb, m in keep:
        ok = int((res.cpu().numpy().view(miphy.PuschResult)["tb_crc_ok"] != 0).sum())
        print(json.dumps({"processor_layers": nl, "transport_blocks": m, "tb_crc_ok": ok, "tb_bytes": int(tb.size),
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
    for name, _, slots, bits in legs:
        t = sorted(ms[name])
        med = t[len(t) // 2]
        rec = {"leg": name, "slots": slots, "ms_per_call_median": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4),
               "slots_per_s": round(slots / (med * 1e-3))}
        if bits:
            rec["info_gbit_per_s"] = round(bits / (med * 1e-3) / 1e9, 3)
        print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
