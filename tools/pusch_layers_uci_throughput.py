#!/usr/bin/env python3
"""What UCI placeholders and the EVM cost above one layer (csrc/pusch_demod.hip: the EX instances of pusch_demod_kernel, which take the exact
demapper; csrc/pusch_proc.hip: miphy_pusch_process_layers_batch_ex).

Demodulator legs: L = 2 and 4 on four ports, 273 PRB x 14 symbols (DM-RS on symbol 2, two CDM groups without data), 256QAM, the compact estimate,
`--jobs` device-resident jobs per launch with a grid of random samples each: miphy_pusch_demodulate_layers_batch (plain), and _ex with the EVM sums
only, with the placeholders of a one-bit HARQ-ACK only (20 resource elements, 40 reserved), and with both.

Processor legs: one transport block on L = 2 and 4 (256QAM, four ports, `--snr` dB), its grid copied `--slots` times so that every PDU reads a grid and
HARQ buffers of its own: miphy_pusch_process_layers_batch on the transmission of tests/pusch_layers_estimator_cases.py against _ex with a four-bit
HARQ-ACK on 40 resource elements and the EVM on the transmission of tests/pusch_layers_uci_cases.py (same transport block size, same channel), with
the number of transport blocks whose CRC passed.

HIP events around `--iters` back-to-back calls after a warm-up of every leg; the legs are timed in turn `--rounds` times; median, fastest and slowest
round are printed, and the ratio of every leg to the plain leg of its group.
Run on the MI355X:  python tools/pusch_layers_uci_throughput.py [--jobs 1024] [--slots 1024] [--iters 20] [--rounds 5]
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
    ap.add_argument("--slots", type=int, default=1024)
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
    nre = nsc * 13
    legs = []  # (group, name, run)

    # ---- demodulator
    n = args.jobs
    gen = torch.Generator(device="cuda").manual_seed(0)
    grid = torch.randn(n * NPT * 14 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)
    ce = torch.randn(n * 16 * nsc * 2, generator=gen, device="cuda", dtype=torch.float32)
    sc = torch.full((5 * n,), 0.01, dtype=torch.float32, device="cuda")
    llr = torch.zeros(n * nre * 4 * MOD + 64, dtype=torch.int8, device="cuda")
    sums = torch.zeros(14 * n, dtype=torch.float32, device="cuda")
    for nl in (2, 4):
        x = np.zeros(1, dtype=miphy.UlschDemuxJob)[0]
        x["mod"], x["nof_layers"], x["start_symbol"], x["nof_symbols"], x["dmrs_type"], x["nof_cdm_groups_without_data"] = MOD, nl, 0, 14, 1, 2
        x["dmrs_symbols_mask"], x["nof_prb"], x["nof_harq_ack_rvd"], x["nof_enc_harq_ack_bits"], x["nof_harq_ack_bits"] = 1 << 2, NPRB, 40 * nl * MOD, 20 * nl * MOD, 1
        ph = miphy.ulsch_placeholders(x)
        assert ph.size == 20
        ph_d = torch.from_numpy(ph.view(np.int16)).cuda()
        jobs = {}
        for with_ph in (False, True):
            lj = np.zeros(n, dtype=miphy.PuschDemodLayersJob)
            j = lj["base"]
            j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = 0x4601, 900, MOD, NPT, 0, 14
            j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 1, 2, 14, 1
            j["rx_ports"] = [0, 1, 2, 3]
            j["dmrs_symbols_mask"], j["grid_nof_prb"] = 1 << 2, NPRB
            mask_all(j)
            idx = np.arange(n, dtype=np.uint64)
            j["grid_offset"], j["ce_offset"], j["scalars_offset"] = idx * (NPT * 14 * nsc), idx * (16 * nsc), idx * 5
            j["llr_offset"], j["nof_llr"], j["evm_offset"] = idx * (nre * 4 * MOD), nre * nl * MOD, idx * 14
            j["nof_placeholders"] = ph.size if with_ph else 0
            lj["nof_tx_layers"] = nl
            jobs[with_ph] = torch.from_numpy(lj.view(np.uint8).copy()).cuda()
        g = "demodulate_L%d_P4" % nl
        legs += [(g, g + "_plain", lambda d=jobs[False]: ctx.pusch_demodulate_layers_batch(d, grid, ce, sc, llr)),
                 (g, g + "_evm", lambda d=jobs[False]: ctx.pusch_demodulate_layers_batch_ex(d, grid, ce, sc, llr, None, sums)),
                 (g, g + "_placeholders", lambda d=jobs[True], p=ph_d: ctx.pusch_demodulate_layers_batch_ex(d, grid, ce, sc, llr, p, None)),
                 (g, g + "_placeholders_evm", lambda d=jobs[True], p=ph_d: ctx.pusch_demodulate_layers_batch_ex(d, grid, ce, sc, llr, p, sums))]

    # ---- processor
    keep = []
    if not args.no_processor:
        import pusch_layers_cases as PL
        import pusch_layers_estimator_cases as E
        import pusch_layers_uci_cases as U
        m = args.slots
        for nl in (2, 4):
            tb_bytes = tb_size(args.tb_bytes * nl)
            ncb = miphy.sch_segmentation(tb_bytes, 1).nof_cbs
            c, tb0, g0, _ = E.chain_tx(nl, NPT, MOD, tb_bytes, args.snr, (2,), nprb=NPRB)
            t = U.build("probe", dict(nl=nl, npt=NPT, mod=MOD, tb_bytes=tb_bytes, snr_db=args.snr, O=(4, 0, 0), G_re=(40, 0, 0), rvd_re=0, nprb=NPRB, dmrs=(2,)))
            g1 = U.chain_tx(t["c"], t["scr"], args.snr)[0]
            rb, dm = PL.masks(c)
            pdus = np.zeros(m, dtype=miphy.PuschLayersPdu)
            p = pdus["base"]
            p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, E.SLOT, c["rnti"], c["n_id"], E.SCR
            p["tb_bytes"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb_bytes, MOD, NPT, 0, 14
            p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = 1, 0, 1, [0, 1, 2, 3], 1, 6
            p["dmrs_symbols_mask"], p["grid_nof_prb"] = 1 << 2, NPRB
            mask_all(p)
            idx = np.arange(m, dtype=np.uint64)
            p["harq_cb_index"], p["grid_offset"], p["tb_offset"] = idx * ncb, idx * g0.size, idx * tb_bytes
            pdus["nof_tx_layers"] = nl
            G = t["mc"][9][0]
            uci = np.zeros(m, dtype=miphy.PuschUci)
            uci["nof_harq_ack_bits"], uci["nof_enc_harq_ack_bits"], uci["has_codeword"], uci["harq_ack_offset"] = 4, G, 1, idx * G
            uci["csi_part1_offset"] = uci["csi_part2_offset"] = uci["harq_ack_offset"] + np.uint64(G)
            soft = torch.zeros(m * ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
            msgs = torch.zeros(m * ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
            crc = torch.zeros(m * ncb, dtype=torch.uint8, device="cuda")
            scp = torch.zeros(80 * m, dtype=torch.float32, device="cuda")
            uci_llr = torch.zeros(m * G + 16, dtype=torch.int8, device="cuda")
            evm = torch.zeros(m, dtype=torch.float32, device="cuda")
            run = {}
            for name, g_host, tb in (("plain", g0, tb0), ("uci_evm", g1, t["tb"])):
                grid_p = torch.from_numpy(np.nan_to_num(g_host).reshape(-1)).cuda().repeat(m)
                out = torch.zeros(m * tb_bytes, dtype=torch.uint8, device="cuda")
                res = torch.zeros(m * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
                h = (soft, msgs, crc, out, res)
                keep.append((nl, name, res, out, tb, m))
                if name == "plain":
                    run[name] = lambda grid_p=grid_p, h=h, pdus=pdus, scp=scp: ctx.pusch_process_layers_batch(pdus, grid_p, *h, scp)
                else:
                    run[name] = lambda grid_p=grid_p, h=h, pdus=pdus, scp=scp, uci=uci, uci_llr=uci_llr, evm=evm: ctx.pusch_process_layers_batch_ex(
                        pdus, uci, grid_p, *h, scp, uci_llr, evm)
            g = "process_L%d_P4" % nl
            legs += [(g, g + "_plain", run["plain"]), (g, g + "_harq_ack_4_bits_evm", run["uci_evm"])]

    for _, _, run in legs:
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    for nl, name, res, out, tb, m in keep:
        ok = int((res.cpu().numpy().view(miphy.PuschResult)["tb_crc_ok"] != 0).sum())
        print(json.dumps({"processor_layers": nl, "transmission": name, "transport_blocks": m, "tb_crc_ok": ok, "tb_bytes": int(tb.size),
                          "first_block_equal": bool(np.array_equal(out[:tb.size].cpu().numpy(), tb))}))
    ms = {name: [] for _, name, _ in legs}
    for _ in range(args.rounds):
        for _, name, run in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                run()
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.iters)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    for group, name, _ in legs:
        v = sorted(ms[name])
        print(json.dumps({"leg": name, "calls_of": args.slots if group.startswith("process") else n, "ms_per_call_median": round(med[name], 4),
                          "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4), "ratio_to_plain": round(med[name] / med[group + "_plain"], 3)}))
    ctx.close()


if __name__ == "__main__":
    main()
