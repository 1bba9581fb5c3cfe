#!/usr/bin/env python3
"""Records tests/golden/pucch_processor.npz: the reference's own PUCCH processor (create_pucch_processor_factory_sw, driven by
tools/gen_pucch_golden.cpp) on grids that tests/pucch_tx.py builds from a seed, for formats 1 and 2:
- format 1: every symbol count and start, hopping on and off, cyclic shifts 0..11, every valid OCC, SR-only and 1-2 HARQ-ACK bits,
  and groups of 2..12 users sharing one PRB with different shift / OCC pairs (one case per user, one grid per group);
- format 2: 1..2 symbols at every start, 1..16 PRBs, 3..11 payload bits split across HARQ-ACK / SR / CSI part 1;
- both: n_id and slot over numerologies 0 and 1, 1..4 receive ports, BWP start != 0, SNR from clean down to noise only (DTX).
The grids themselves are not stored: per group, the seed, the channel parameters and the SHA-256 of the grid bytes the reference saw.
Needs the reference library build() compiles (oracle/_ref/libsrsran_ref.a) and its sources.
Run:  python tools/gen_pucch_golden.py
"""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pucch_tx as T  # noqa: E402

rng = np.random.default_rng(20261017)
NOISE = (0.0, 0.003, 0.03, 0.1, 0.3, 0.7, 1.5, 4.0)


def build_driver():
    exe = os.path.join(ROOT, "oracle", "_ref", "gen_pucch_golden")
    lib = os.path.join(ROOT, "oracle", "_ref", "libsrsran_ref.a")
    inc = ["-I%s/include" % REF, "-I%s/external/fmt/include" % REF, "-I%s/external" % REF, "-I%s" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-w", "-mavx", "-mavx2", "-mfma", "-DHAVE_SSE", "-DHAVE_AVX", "-DHAVE_AVX2",
                           "-DHAVE_FMA"] + inc + [os.path.join(ROOT, "tools", "gen_pucch_golden.cpp"), lib, "-lpthread", "-o", exe])
    return exe


def f1_max_occ(nsym, hop):
    _, data = T.f1_layout(nsym, hop)
    return min(len(d) for d in data if d) - 1  # the detector's w* asserts i < N for every hop


def common(num, nports):
    """Slot, ports and BWP of one group."""
    slot = int(rng.integers(0, 10 << num))
    bwp_start = int(rng.choice([0, 0, 1, 3, 7, 20]))
    bwp_size = int(rng.integers(16, 33))
    return slot, bwp_start, bwp_size


def f1_cfg(num, slot, nports, bwp_start, bwp_size, start, nsym, hop, prb, prb2, nid, ics, occ, nharq):
    c = np.zeros(T.NHDR, np.int32)
    c[[T.H_FMT, T.H_NUM, T.H_SLOT, T.H_NPORTS, T.H_START, T.H_NSYM, T.H_BWP_START, T.H_BWP_SIZE, T.H_PRB, T.H_HOP, T.H_PRB2, T.H_NID,
       T.H_ICS, T.H_OCC, T.H_NHARQ, T.H_GRID_NPRB]] = [1, num, slot, nports, start, nsym, bwp_start, bwp_size, prb, hop, prb2, nid, ics,
                                                        occ, nharq, bwp_start + bwp_size]
    return c


def cases():
    """Groups: (seed, nports, grid_nprb, noise, [(cfg, bits, tx_on)])."""
    groups = []
    # Format 1, one user per grid: every (nsym, hop) with every start, the shifts and OCCs spread over them.
    k = 0
    for nsym in range(4, 15):
        for hop in (0, 1):
            for start in range(0, 15 - nsym):
                for rep in range(2 if nsym < 12 else 4):
                    num = k % 2
                    nports = 1 + (k % 4)
                    slot, bwp_start, bwp_size = common(num, nports)
                    prb = int(rng.integers(0, bwp_size))
                    prb2 = int(rng.integers(0, bwp_size))
                    nid = int(rng.integers(0, 1024))
                    occ = int(rng.integers(0, f1_max_occ(nsym, hop) + 1))
                    nharq = int(rng.integers(0, 3))
                    noise = NOISE[k % len(NOISE)]
                    on = (k % 11) != 5
                    bits = [int(b) for b in rng.integers(0, 2, nharq)] if nharq else [0]
                    c = f1_cfg(num, slot, nports, bwp_start, bwp_size, start, nsym, hop, prb, prb2, nid, k % 12, occ, nharq)
                    groups.append((int(rng.integers(1, 2**62)), nports, bwp_start + bwp_size, noise, [(c, bits, on)]))
                    k += 1
    # Format 1, 2..12 users on one PRB (same symbols, hopping, n_id), separated by cyclic shift and OCC.
    for g in range(40):
        num = g % 2
        nports = 1 + (g % 4)
        slot, bwp_start, bwp_size = common(num, nports)
        nsym = int(rng.choice([4, 8, 10, 14, 14]))
        hop = int(g % 3 == 0)
        start = int(rng.integers(0, 15 - nsym))
        prb, prb2 = int(rng.integers(0, bwp_size)), int(rng.integers(0, bwp_size))
        nid = int(rng.integers(0, 1024))
        nocc = f1_max_occ(nsym, hop) + 1
        pairs = [(ics, occ) for occ in range(nocc) for ics in range(0, 12, 2)]
        nue = min(2 + g % 11, len(pairs))
        sel = rng.choice(len(pairs), nue, replace=False)
        users = []
        for j in sel:
            ics, occ = pairs[j]
            nharq = int(rng.integers(0, 3))
            bits = [int(b) for b in rng.integers(0, 2, nharq)] if nharq else [0]
            users.append((f1_cfg(num, slot, nports, bwp_start, bwp_size, start, nsym, hop, prb, prb2, nid, ics, occ, nharq), bits,
                          bool(rng.random() > 0.15)))
        groups.append((int(rng.integers(1, 2**62)), nports, bwp_start + bwp_size, float(rng.choice(NOISE[:6])), users))
    # Format 2.
    k = 0
    for nsym in (1, 2):
        for start in range(0, 15 - nsym):
            for nprb in list(range(1, 17)) + [int(x) for x in rng.integers(1, 17, 4)]:
                num = k % 2
                nports = 1 + (k % 4)
                slot, bwp_start, bwp_size = common(num, nports)
                bwp_size = max(bwp_size, nprb)
                prb = int(rng.integers(0, bwp_size - nprb + 1))
                K = 3 + (k % 9)
                nharq = int(rng.integers(0, K + 1))
                nsr = int(rng.integers(0, min(K - nharq, 4) + 1))
                c = np.zeros(T.NHDR, np.int32)
                c[[T.H_FMT, T.H_NUM, T.H_SLOT, T.H_NPORTS, T.H_START, T.H_NSYM, T.H_BWP_START, T.H_BWP_SIZE, T.H_PRB, T.H_NPRB, T.H_NID,
                   T.H_NID0, T.H_RNTI, T.H_NHARQ, T.H_NSR, T.H_NCSI1, T.H_GRID_NPRB]] = [
                       2, num, slot, nports, start, nsym, bwp_start, bwp_size, prb, nprb, int(rng.integers(0, 1024)),
                       int(rng.integers(0, 65536)), int(rng.integers(1, 65520)), nharq, nsr, K - nharq - nsr, bwp_start + bwp_size]
                noise = NOISE[(k * 5) % len(NOISE)]
                on = (k % 13) != 7
                groups.append((int(rng.integers(1, 2**62)), nports, bwp_start + bwp_size, noise,
                               [(c, [int(b) for b in rng.integers(0, 2, K)], on)]))
                k += 1
    return groups


def main():
    exe = build_driver()
    groups = cases()
    cfg, grp, bits, nbits, on = [], [], [], [], []
    g_seed, g_nports, g_nprb, g_noise, g_hash = [], [], [], [], []
    stdin = [struct.pack("<I", sum(len(g[4]) for g in groups))]
    for gi, (seed, nports, gnprb, noise, users) in enumerate(groups):
        grid = T.build_grid(seed, nports, gnprb, noise, [u[0] for u in users], [u[1] for u in users], [u[2] for u in users])
        g_seed.append(seed), g_nports.append(nports), g_nprb.append(gnprb), g_noise.append(noise), g_hash.append(T.grid_hash(grid))
        for c, b, o in users:
            cfg.append(c), grp.append(gi), on.append(o), nbits.append(len(b))
            bits.append(np.pad(np.asarray(b, np.uint8), (0, 11 - len(b))))
            stdin.append(c.astype("<i4").tobytes() + grid.astype(np.complex64).tobytes())
    out = subprocess.run([exe], input=b"".join(stdin), stdout=subprocess.PIPE, check=True).stdout
    lp = np.frombuffer(out[:30 * 12 * 12 * 8], np.complex64).reshape(30, 12, 12)
    pos = 30 * 12 * 12 * 8
    n = len(cfg)
    status = np.zeros(n, np.uint8)
    pay = np.zeros((n, 11), np.uint8)
    pay_n = np.zeros(n, np.uint8)
    fl = np.zeros((n, 5), np.float32)
    llr, llr_off = [], np.zeros(n + 1, np.int64)
    for i in range(n):
        status[i], pay_n[i] = out[pos], out[pos + 1]
        m = int(pay_n[i])
        pos += 2
        pay[i, :m] = np.frombuffer(out[pos:pos + m], np.uint8)
        pos += m
        fl[i] = np.frombuffer(out[pos:pos + 20], np.float32)
        pos += 20
        (nl,) = struct.unpack("<I", out[pos:pos + 4])
        pos += 4
        llr.append(np.frombuffer(out[pos:pos + nl], np.int8))
        pos += nl
        llr_off[i + 1] = llr_off[i] + nl
    assert pos == len(out)
    cfg = np.stack(cfg)
    path = os.path.join(ROOT, "tests", "golden", "pucch_processor.npz")
    np.savez_compressed(path, cfg=cfg, group=np.asarray(grp, np.int32), tx_bits=np.stack(bits), tx_nbits=np.asarray(nbits, np.uint8),
                        tx_on=np.asarray(on, np.uint8), g_seed=np.asarray(g_seed, np.uint64), g_nports=np.asarray(g_nports, np.int32),
                        g_grid_nprb=np.asarray(g_nprb, np.int32), g_noise=np.asarray(g_noise, np.float64),
                        g_sha256=np.asarray(g_hash), status=status, payload=pay, payload_len=pay_n, metric=fl[:, 0], epre_db=fl[:, 1],
                        rsrp_db=fl[:, 2], sinr_db=fl[:, 3], ta_s=fl[:, 4], llr=np.concatenate(llr), llr_offset=llr_off, low_papr=lp)
    f1 = cfg[:, T.H_FMT] == 1
    print("%s: %d format-1 cases, %d format-2 cases, %d groups, %d bytes" % (path, f1.sum(), (~f1).sum(), len(groups),
                                                                            os.path.getsize(path)))
    for f in (1, 2):
        m = cfg[:, T.H_FMT] == f
        print("format %d status counts:" % f, np.bincount(status[m], minlength=3))


if __name__ == "__main__":
    main()
