#!/usr/bin/env python3
"""SHA-256 of what the four DM-RS estimator entry points (csrc/chest.hip) write, per case, for an A-B of two builds of the library: a change that
is not meant to move a bit must give the same list. The cases come from the tests' own builders (tests/chest_batch.py, tests/test_chest_gpu.py,
tests/pusch_layers_estimator_cases.py, tests/test_chest_tp_gpu.py): host and device-resident jobs, compact and full estimates, 1-4 layers, 1-4
DM-RS symbols, a scattered and a full allocation on 275 PRB, hopping jobs with the caller's pilots, and per entry point one batch small enough for
the split time-alignment workgroup and one too large for it.
  MIPHY_LIBRARY=tools/_ab/parent/libmiphy.so python tools/chest_digests.py --out a.jsonl ; python tools/chest_digests.py --out b.jsonl
  python tools/chest_digests.py --compare a.jsonl b.jsonl      (exit status 1 when a case differs or is missing)
  python tools/chest_digests.py --time-tp 3                    (the transform-precoding entry under load: the one leg of chest_kernel<true> no probe has)
Run on the MI355X."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def batch_cases():
    """(name, entry, cases, keywords of chest_batch.run) for the two entry points that generate their pilots."""
    import chest_batch as B
    import pusch_layers_estimator_cases as E
    import test_chest_gpu as T
    rng = np.random.default_rng(2024)
    one = [T.make_case(rng, 52, slice(3, 33), 2, 1, [2], delay=3.0), T.make_case(rng, 106, slice(10, 60), 2, 2, [2, 11], scaling=0.7071, delay=-12.0),
           T.make_case(rng, 25, slice(0, 25), 4, 4, [2, 3, 10, 11], numerology=0, slot=9, delay=-30.0),
           T.make_case(rng, 24, slice(2, 22), 3, 3, [2, 7, 11], first=1, nof=12, delay=5.0)]
    wide = [T.make_case(rng, 275, B.SCATTERED, 2, 2, [2, 11], numerology=3, slot=79), T.make_case(rng, 275, slice(0, 275), 1, 1, [2, 7, 11], delay=4.0)]
    lay = [E.make_case(rng, 24, slice(2, 2 + 3 * nl), npt, nl, dsyms, delay=float(nl - 1), slot=nl, first=first, nof=nof)[0]
           for nl, npt, dsyms, first, nof in ((1, 2, [2, 11], 0, 14), (2, 2, [2, 7, 11], 0, 14), (3, 4, [3], 2, 10), (4, 4, [2, 5, 8, 11], 0, 14), (1, 1, [2, 7, 11], 1, 12))]
    lay_wide = [E.make_case(rng, 275, B.SCATTERED, 2, 2, [2, 7, 11], numerology=3, slot=79, delay=1.0)[0],
                E.make_case(rng, 275, slice(0, 275), 4, 4, [2], delay=2.0)[0], E.make_case(rng, 275, [274], 3, 3, [2, 11], delay=0.0)[0]]
    out = []
    for entry, tag, small, widest in (("dmrs_pusch_estimate_batch", "one", one, wide), ("dmrs_pusch_estimate_layers_batch", "layers", lay, lay_wide)):
        for compact in (False, True):
            for device in (None, "nohint", "hint"):
                out.append(("%s/%s/%s" % (tag, "compact" if compact else "full", device or "host"), entry, small, dict(compact=compact, device=device, room_4x4=True)))
        out.append((tag + "/275-prb", entry, widest, dict(compact=True)))
        out.append((tag + "/fills-the-chip", entry, small * 40, dict()))  # at least 200 jobs x 4 ports: more workgroups than half the CUs
    return out


def port_estimator(ctx, torch, miphy, device):
    """miphy_port_channel_estimate_batch as tests/test_chest_gpu.py drives it: the pilots the PUSCH estimator would generate, without and with hopping."""
    import test_chest_gpu as T
    rng = np.random.default_rng(2718)
    digests = []
    for nl, hop, alloc1, alloc2, dsyms in ((1, 0, slice(4, 34), None, [2, 11]), (1, 7, slice(2, 22), slice(28, 48), [2, 9]), (2, 6, slice(0, 25), slice(27, 52), [2, 4, 8, 11])):
        nprb, slot, scr, scaling = 52, 5, 321, 1.4125
        first, nof = (0, 14) if nl == 1 else (1, 12)
        hops = [(first, first + nof, alloc1)] if not hop else [(first, hop, alloc1), (hop, first + nof, alloc2)]
        g, per_hop = np.zeros((1, 14, nprb * 12), np.complex64), []
        for a, b, alloc in hops:
            ds = [l for l in dsyms if a <= l < b]
            case = T.make_case(rng, nprb, alloc, 1, nl, ds, slot=slot, scr=scr, scaling=scaling, delay=5.0)
            g[:, a:b, :] = case[-1][:, a:b, :]
            per_hop.append((ds, case[7]))
        j = np.zeros(1, dtype=miphy.PuschChestJob)
        j[0]["numerology"], j[0]["scaling"], j[0]["nof_tx_layers"], j[0]["nof_rx_ports"] = 1, scaling, nl, 1
        j[0]["first_symbol"], j[0]["nof_symbols"], j[0]["rx_ports"], j[0]["grid_nof_prb"] = first, nof, [0, 1, 2, 3], nprb
        j[0]["symbols_mask"], j[0]["hop_symbol"] = sum(1 << l for l in dsyms), hop
        for key, (ds, rb) in zip(("rb_mask", "rb_mask2"), per_hop):
            m = [0] * 5
            for r in np.nonzero(rb)[0]:
                m[r >> 6] |= 1 << (int(r) & 63)
            j[0][key] = m
        j[0]["re_odd_mask"] = sum(((ly // 2) % 2) << ly for ly in range(nl))
        pil = np.concatenate([np.stack([T._pilots(rb, l, slot, scr, 0, nl) for l in ds], axis=1) for ds, rb in per_hop], axis=1)
        g_d, p_d = torch.from_numpy(g.reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(pil).reshape(-1)).cuda()
        ce_d = torch.ones(nl * (first + nof) * nprb * 12, dtype=torch.complex64, device="cuda")
        sc_d = torch.full((5 * nl,), -77.0, dtype=torch.float32, device="cuda")
        ctx.port_channel_estimate_batch(torch.from_numpy(j.view(np.uint8)).cuda() if device else j, g_d, p_d, ce_d, sc_d)
        torch.cuda.synchronize()
        digests.append(("port/%dl-hop%d/%s" % (nl, hop, "device" if device else "host"), sha(ce_d.cpu().numpy()), sha(sc_d.cpu().numpy())))
    return digests


def tp_estimator(ctx, torch, miphy, device, repeat):
    """miphy_dmrs_pusch_estimate_tp_batch on the jobs of tests/test_chest_tp_gpu.py, `repeat` times in one batch."""
    import test_chest_tp_gpu as P
    rng = np.random.default_rng(31)
    cases = [(24, 3, 2, 1, 0, 1, (2, 11)), (24, 7, 5, 2, 1, 0, P.DSYMS), (24, 11, 6, 4, 2, 1, (2, 11)), (24, 9, 12, 3, 2, 0, P.DSYMS), (273, 2, 270, 2, 1, 1, P.DSYMS)] * repeat
    jobs, grids, goff, coff = [], [], 0, 0
    for k, (gprb, first, nprb, ports, hopping, compact, dsyms) in enumerate(cases):
        nsc = gprb * 12
        grids.append((rng.standard_normal((4, 14, nsc)) + 1j * rng.standard_normal((4, 14, nsc))).astype(np.complex64))
        jobs.append(P._job(miphy, gprb, first, nprb, ports, 19 - k % 20, 100 + 200 * (k % 5), hopping, compact, dsyms, 0, goff, coff, 20 * k))
        goff += grids[-1].size
        coff += ports * (1 if compact else 14) * nsc
    ja = np.array(jobs, dtype=miphy.PuschChestTpJob)
    g = torch.from_numpy(np.concatenate([x.reshape(-1) for x in grids])).cuda()
    ce = torch.full((coff,), 5 + 5j, dtype=torch.complex64, device="cuda")
    sc = torch.full((20 * len(cases),), -5.0, dtype=torch.float32, device="cuda")
    if device:
        ctx.dmrs_pusch_estimate_tp_batch(torch.from_numpy(ja.view(np.uint8)).cuda(), g, ce, sc, max_ports=4)
    else:
        ctx.dmrs_pusch_estimate_tp_batch(ja, g, ce, sc)
    torch.cuda.synchronize()
    return ("tp/x%d/%s" % (repeat, "device" if device else "host"), sha(ce.cpu().numpy()), sha(sc.cpu().numpy()))


def time_tp_estimator(ctx, torch, miphy, jobs_n, iters, rounds):
    """chest_kernel<true> under load, which no other probe times: HIP events around `iters` back-to-back calls of miphy_dmrs_pusch_estimate_tp_batch on
    `jobs_n` device-resident jobs (270 of 273 PRB, two ports, three DM-RS symbols, compact estimate, one grid of random samples for all); its pilot
    kernel is part of the call. -> JSON record: median, fastest and slowest round in ms per call."""
    import test_chest_tp_gpu as P
    nsc = 273 * 12
    ja = np.array([P._job(miphy, 273, 2, 270, 2, k % 20, 100 + k % 900, k % 3, 1, P.DSYMS, 0, 0, 2 * nsc * k, 20 * k) for k in range(jobs_n)], dtype=miphy.PuschChestTpJob)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    g = torch.view_as_complex(torch.randn(4 * 14 * nsc, 2, device="cuda", generator=gen))
    ce, sc = torch.zeros(2 * nsc * jobs_n, dtype=torch.complex64, device="cuda"), torch.zeros(20 * jobs_n, dtype=torch.float32, device="cuda")
    jd = torch.from_numpy(ja.view(np.uint8)).cuda()
    call = lambda: ctx.dmrs_pusch_estimate_tp_batch(jd, g, ce, sc, max_ports=2)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    ms.sort()
    return {"leg": "estimate_tp_270prb_P2", "jobs": jobs_n, "ms_per_call_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def compare(a, b):
    la, lb = ([json.loads(l) for l in open(f) if l.startswith("{")] for f in (a, b))
    da, db = ({r["case"]: (r["ce_sha256"], r["scalars_sha256"]) for r in l} for l in (la, lb))
    bad = [c for c in sorted(set(da) | set(db)) if da.get(c) != db.get(c)]
    print("%d cases in %s, %d in %s, %d differ or are missing: %s" % (len(da), a, len(db), b, len(bad), bad))
    return 1 if bad or not da else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write one JSON line per case to this file (and to the standard output)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time-tp", type=int, metavar="ROUNDS", help="no digests: time miphy_dmrs_pusch_estimate_tp_batch (1024 jobs, 20 calls per round)")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    import miphy
    import chest_batch as B
    assert torch.cuda.is_available(), "the digests are of what the GPU writes"
    ctx = miphy.Context(0)
    if args.time_tp:
        print(json.dumps(time_tp_estimator(ctx, torch, miphy, 1024, 20, args.time_tp)))
        ctx.close()
        return
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    digests = []
    for name, entry, cases, kw in batch_cases():
        if name.endswith("fills-the-chip"):
            assert len(cases) * 2 > cus, "too few jobs for the unsplit form"
        elif "275" not in name:
            assert len(cases) * 16 * 2 <= cus, "too many jobs for the split form"
        res = B.run(ctx, cases, entry, None, check=False, **kw)
        digests.append((name, sha(*[ce for ce, _ in res]), sha(*[sc for _, sc in res])))
    for device in (False, True):
        digests += port_estimator(ctx, torch, miphy, device)
        digests += [tp_estimator(ctx, torch, miphy, device, 1), tp_estimator(ctx, torch, miphy, device, 60)]
    ctx.close()
    lib = os.environ.get("MIPHY_LIBRARY", "in-tree")
    lines = [json.dumps({"tool": "chest_digests", "library": lib, "case": n, "ce_sha256": c, "scalars_sha256": s}) for n, c, s in digests]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
