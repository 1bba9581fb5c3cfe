#!/usr/bin/env python3
"""SHA-256 of what the entry points built on the low-PAPR sequences and on the PUCCH per-port measurements write, per case, for an A-B of two builds
of the library: a change that is not meant to move a bit must give the same list. PUCCH formats 0 to 4 (csrc/pucch.hip, pucch_f34.hip, pucch_f0.hip),
SRS pilots and estimates (csrc/srs.hip), the DM-RS of transform-precoded PUSCH (csrc/transform_precoding.hip, pilots and estimator entry) and the host
function miphy_low_papr_sequence. The cases come from the tests' own builders (tests/pucch_tx.py, pucch_long_tx.py, pucch_f34_tx.py, pucch_f0_cases.py,
srs_tx.py, test_chest_tp_gpu.py) at the smallest shapes that reach each branch; every case is one call, or one call per entry point.
  MIPHY_LIBRARY=tools/_ab/parent/libmiphy.so python tools/sequence_digests.py --out a.jsonl ; python tools/sequence_digests.py --out b.jsonl
  python tools/sequence_digests.py --compare a.jsonl b.jsonl      (exit status 1 when a case differs or is missing; prints each list folded to one
                                                                   SHA-256 per entry-point group, the form profiles/ keeps, and the verdict)
  python tools/sequence_digests.py --compare-dumps DIR_A DIR_B    (the .npy arrays of two `bench.py --dump-outputs` runs, byte for byte)
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


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def named(names, arrays):
    return {n: sha(a) for n, a in zip(names, arrays)}


def format1(ctx, torch, miphy):
    """4 and 14 symbols, with and without hopping, 1 and 4 ports, 0 (SR alone), 1 and 2 HARQ-ACK bits: one PDU on a 4-PRB grid of its own per call."""
    import pucch_long_tx as LT
    import pucch_tx as T
    import test_pucch_long_gpu as PL
    out, i = [], 0
    for nsym in (4, 14):
        for hop in (0, 1):
            for nports in (1, 4):
                for nharq in (0, 1, 2):
                    c = LT.f2_cfg(0, nsym, 14 - nsym, 1, 4, nports, 0, (411, 1023)[i % 2], 0, slot=(7, 19)[hop])
                    c[T.H_FMT], c[T.H_HOP], c[T.H_PRB2], c[T.H_OCC], c[T.H_ICS], c[T.H_NHARQ], c[T.H_NSR] = 1, hop, 3, nsym == 14, (5 * i) % 12, nharq, nharq == 0
                    bits = [(i >> k) & 1 for k in range(max(nharq, 1))] if nharq else [0]
                    grid = LT.build_grid(900 + i, nports, 4, 0.1, [c], [bits], [True])
                    jobs = np.array([PL.job_of(c, (nharq, int(nharq == 0), 0), 0, 3, 1)], miphy.PucchJob)
                    res = PL.run(ctx, jobs, torch.from_numpy(grid.ravel()).cuda(), 24, 64)
                    out.append(("f1/%dsym-hop%d-%dport-%dharq" % (nsym, hop, nports, nharq), named(("payload", "records", "llr"), res)))
                    i += 1
    return out


def format2(ctx, torch, miphy):
    """1 and 16 PRB, 1 and 2 symbols, 3, 11 and 12 bits where the allocation carries them, list sizes 1 and 8 through miphy_pucch_process_batch_ex (12 bits
    with and without llr_out) and the short ones through miphy_pucch_process_batch as well."""
    import pucch_long_tx as LT
    import test_pucch_long_gpu as PL
    import uci_polar as U
    out, i = [], 0
    for nprb in (1, 16):
        for nsym in (1, 2):
            for K in (3, 11, 12):
                E = 16 * nprb * nsym
                if K > 11 and U.info(K, E) is None:
                    continue
                c = LT.f2_cfg(nprb, nsym, 14 - nsym - i % 3, 2, 20, (1, 2, 4)[i % 3], 4660 + i, (29, 777)[i % 2], 100 + i, slot=(0, 19)[i % 2])
                bits = np.random.default_rng(i).integers(0, 2, K).astype(np.uint8)
                grid_d = torch.from_numpy(LT.build_grid(950 + i, int(c[3]), 20, 0.3, [c], [bits], [True]).ravel()).cuda()
                counts = (min(K, 2), int(K > 3), K - min(K, 2) - int(K > 3))
                jobs = np.array([PL.job_of(c, counts, 0, 3, 1)], miphy.PucchJob)
                tag = "f2/%dprb-%dsym-%dbits" % (nprb, nsym, K)
                for L in (1, 8):
                    for with_llr in (True, False) if K > 11 else (True,):
                        res = PL.run(ctx, jobs, grid_d, K + 16, E + 16, L, with_llr=with_llr)
                        out.append(("%s/list%d%s" % (tag, L, "" if with_llr else "-no-llr-out"), named(("payload", "records", "llr"), res)))
                if K <= 11:
                    out.append((tag + "/short-entry", named(("payload", "records", "llr"), PL.run(ctx, jobs, grid_d, K + 16, E + 16))))
                i += 1
    return out


def formats34(ctx, torch, miphy):
    """Format 3 on 1 PRB (the table), 3 PRB (the first Zadoff-Chu length) and 16 PRB, format 4 with two and four sequences, each with four shapes that
    vary hopping, additional DM-RS, pi/2-BPSK and 11 or 12 bits (the nearest payload the allocation carries), est_out and llr_out both on and both off,
    and each alone."""
    import pucch_f34_cases as G
    import pucch_f34_tx as X
    import test_pucch_f34_gpu as PF
    out, i = [], 0
    for fmt, nprb, nsf in ((3, 1, 0), (3, 3, 0), (3, 16, 0), (4, 1, 2), (4, 1, 4)):
        for nsym, hop, add, pi2, K in ((4, 1, 0, 0, 11), (14, 0, 1, 1, 12), (10, 1, 1, 0, 12), (5, 0, 0, 1, 11)):
            p = X.pdu(fmt, nsym, nprb, hop, add, pi2, nsf, (i + 1) % nsf if nsf else 0, nports=(1, 2, 4)[i % 3], prb=1, prb2=17, grid_nprb=G.GRID_NPRB,
                      nid_hop=(0, 29, 513, 1023)[i % 4], nid_scr=77 + i, rnti=4660 + i, slot=(0, 19, 7)[i % 3])
            K = next(k for k in (K, 23 - K, 3) if G.feasible(p, k))
            item = G.item(p, K, 0.05, 31000 + i)
            pre = PF.prepare([item])
            tag = "f%d/%dprb-occ%d/%dsym-hop%d-add%d-pi2bpsk%d-%dbits-%dport" % (fmt, nprb, nsf, nsym, hop, add, pi2, K, p["nports"])
            for llr, est in ((True, True), (False, False), (True, False), (False, True)):
                res = PF.run(ctx, pre, 4, with_llr=llr, with_est=est)
                out.append(("%s/llr%d-est%d" % (tag, llr, est), named(("payload", "records", "llr", "est"), res)))
            i += 1
    return out


def format0(ctx, torch, miphy):
    """The mixed set of tests/pucch_f0_cases.py (1 and 2 symbols, hopping, 1 to 4 ports, every (HARQ-ACK, SR) and so every hypothesis count) with host
    and with device jobs, the batch and every PDU alone."""
    import pucch_f0_cases as G
    import test_pucch_f0_gpu as P0
    items = G.mixed_items()
    assert {(d["pdu"]["nharq"], d["pdu"]["nsr"]) for d in items} == set(G.UCI) and {d["pdu"]["nports"] for d in items} == {1, 2, 3, 4}
    pre = P0.prepare(items)
    jobs = P0.with_thresholds(pre["jobs"])
    out = []
    for dev in (False, True):
        side = "device" if dev else "host"
        out.append(("f0/mixed/" + side, named(("payload", "records", "energy"), P0.run(ctx, pre, jobs=jobs, on_device=dev))))
        for k, d in enumerate(items):
            p = d["pdu"]
            res = P0.run(ctx, pre, jobs=jobs[k:k + 1], on_device=dev)
            out.append(("f0/%dsym-hop%d-%dport-%dharq-%dsr/%s" % (p["nsym"], p["hop"], p["nports"], p["nharq"], p["nsr"], side), named(("payload", "records", "energy"), res)))
    return out


def srs(ctx, torch, miphy):
    """4 PRB on comb 4 (M = 12) and 12 PRB on comb 2 (M = 72, sequence hopping draws v), hopping 0, 1, 2, one, two and four transmit ports on one comb and
    four on two, host and device jobs, pilots and estimate."""
    import srs_tx as X
    import test_srs_gpu as PS
    out, i = [], 0
    for nprb, K in ((4, 4), (12, 2)):
        for hopping in (0, 1, 2):
            for nap, ncs in ((1, 0), (2, 3), (4, 1), (4, K * 2 + 1)):  # the last at or above n_cs_max / 2: the four ports split over two combs
                p = X.ue(R=(1, 4)[i % 2], nap=nap, start=(13, 12, 10)[i % 3], nsym=(1, 2, 4)[i % 3], K=K, kbar=i % K, ncs=ncs, nid=(0, 29, 513, 1023)[i % 4],
                         hopping=hopping, prg=4, prb=i % 3, nprb=nprb, slot=(0, 19)[i % 2], numerology=1)
                rng = np.random.default_rng(700 + i)
                grid = X.build_grid(800 + i, p["R"], p["grid_nprb"], 0.1, [(p, X.prg_channel(rng, p), 0.002 * (i % 5 - 2))])
                assert X.derive(p)["M"] == (12 if K == 4 else 72) and X.derive(p)["P"] == (2 if ncs > 4 else nap)
                pre = PS.prepare([dict(p=p, grid=grid)])
                for dev in (False, True):
                    pil = torch.full((pre["npil"],), complex(PS.HS), dtype=torch.complex64, device="cuda")
                    j = torch.from_numpy(pre["jobs"].view(np.uint8).copy()).cuda() if dev else pre["jobs"]
                    ctx.srs_pilots_batch(j, pil, jobs_on_device=dev)
                    h, rec = PS.run(ctx, pre, on_device=dev)
                    tag = "srs/%dprb-comb%d-hopping%d-%dtx-ncs%d/%s" % (nprb, K, hopping, nap, ncs, "device" if dev else "host")
                    out.append((tag, named(("pilots", "h", "records"), (pil.cpu().numpy(), h, rec))))
                i += 1
    return out


def tp_dmrs(ctx, torch, miphy):
    """miphy_dmrs_pusch_tp_pilots_batch on 2, 5, 6 and 12 PRB (lengths 12, 30, 36, 72), hopping 0, 1, 2, host and device jobs;
    miphy_dmrs_pusch_estimate_tp_batch on 2 and 12 PRB."""
    import test_chest_tp_gpu as P
    out = []
    for nprb in (2, 5, 6, 12):
        for hopping in (0, 1, 2):
            n_id = (37 * nprb + 500 * hopping + 907) % 1008
            ja = np.array([P._job(miphy, 24, 3, nprb, 1, 19, n_id, hopping)], dtype=miphy.PuschChestTpJob)
            for dev in (False, True):
                pil = torch.full((3 * 6 * nprb + 2,), 7 + 7j, dtype=torch.complex64, device="cuda")
                ctx.dmrs_pusch_tp_pilots_batch(torch.from_numpy(ja.view(np.uint8)).cuda() if dev else ja, pil)
                torch.cuda.synchronize()
                out.append(("tp-pilots/%dprb-hopping%d/%s" % (nprb, hopping, "device" if dev else "host"), {"pilots": sha(pil.cpu().numpy())}))
    rng = np.random.default_rng(31)
    for nprb, hopping, ports, compact in ((2, 1, 2, 1), (12, 2, 4, 0), (2, 0, 1, 0), (12, 1, 1, 1)):
        g = torch.from_numpy((rng.standard_normal(4 * 14 * 288) + 1j * rng.standard_normal(4 * 14 * 288)).astype(np.complex64)).cuda()
        ja = np.array([P._job(miphy, 24, 5, nprb, ports, 11, 100 + 200 * hopping, hopping, compact)], dtype=miphy.PuschChestTpJob)
        ce = torch.full((ports * (1 if compact else 14) * 288,), 5 + 5j, dtype=torch.complex64, device="cuda")
        sc = torch.full((20,), -5.0, dtype=torch.float32, device="cuda")
        ctx.dmrs_pusch_estimate_tp_batch(ja, g, ce, sc)
        torch.cuda.synchronize()
        out.append(("tp-estimate/%dprb-hopping%d-%dport" % (nprb, hopping, ports), named(("ce", "scalars"), (ce.cpu().numpy(), sc.cpu().numpy()))))
    return out


def host_sequences(miphy):
    """miphy_low_papr_sequence at every accepted length up to 96, u in {0, 29}, v in {0, 1}."""
    return [("host-sequence/len%d-u%d-v%d" % (n, u, v), {"r": sha(miphy.low_papr_sequence(u, v, n))})
            for n in [12, 30] + list(range(36, 97, 6)) for u in (0, 29) for v in (0, 1)]


def load(f):
    return {r["case"]: r["sha256"] for r in (json.loads(l) for l in open(f) if l.startswith("{")) if r.get("tool") == "sequence_digests"}


def folded(d):
    """A list folded per entry-point group (the case name up to its first slash): the SHA-256 over its 'case array digest' lines in case order."""
    groups = {}
    for case, arrays in d.items():
        g = groups.setdefault(case.split("/")[0], dict(cases=0, arrays=0, h=hashlib.sha256()))
        g["cases"] += 1
        for name, digest in arrays.items():
            g["arrays"] += 1
            g["h"].update(("%s %s %s\n" % (case, name, digest)).encode())
    return {k: dict(cases=g["cases"], arrays=g["arrays"], sha256=g["h"].hexdigest()) for k, g in groups.items()}


def compare(a, b):
    da, db = load(a), load(b)
    bad = [c for c in sorted(set(da) | set(db)) if da.get(c) != db.get(c)]
    for f, d in ((a, da), (b, db)):
        print(json.dumps({"tool": "sequence_digests", "list": f, "groups": folded(d)}))
    print(json.dumps({"tool": "sequence_digests", "compare": [a, b], "cases": [len(da), len(db)], "differ_or_missing": bad, "equal": not bad and bool(da)}))
    return 1 if bad or not da else 0


def compare_dumps(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = [n for n in names if not (os.path.exists(os.path.join(a, n)) and os.path.exists(os.path.join(b, n)) and
                                    open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read())]
    print(json.dumps({"tool": "sequence_digests", "bench_dump_outputs": names, "differ_or_missing": bad, "byte_identical": not bad and bool(names)}))
    return 1 if bad or not names else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write one JSON line per case to this file (and to the standard output)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--compare-dumps", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.compare_dumps:
        sys.exit(compare_dumps(*args.compare_dumps))
    import torch
    import miphy
    assert torch.cuda.is_available(), "the digests are of what the GPU writes"
    ctx = miphy.Context(0)
    digests = host_sequences(miphy)
    for part in (format1, format2, formats34, format0, srs, tp_dmrs):
        digests += part(ctx, torch, miphy)
    ctx.close()
    assert len({n for n, _ in digests}) == len(digests), "case names repeat"
    lib = os.environ.get("MIPHY_LIBRARY", "in-tree")
    lines = [json.dumps({"tool": "sequence_digests", "library": lib, "case": n, "sha256": d}) for n, d in digests]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
