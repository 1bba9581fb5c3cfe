#!/usr/bin/env python3
"""Records tests/golden/short_block_detector.npz: the reference's own short-block detector (create_short_block_detector_factory_sw,
driven by tools/gen_short_block_golden.cpp) on seeded stimuli for every message length K = 1..11 and modulation order Qm in
{1, 2, 4, 6, 8}: minimum, odd, non-multiple-of-32 and long (>= 2000) soft-bit counts; clean +-k, AWGN from noise-only to clean
(both GLRT verdicts for every K >= 3), +-127 inputs, opposite infinities in one accumulator, sums that clamp and recover, all-zero
input and exact correlation ties. Needs the reference library build() compiles (oracle/_ref/libsrsran_ref.a) and its sources.
Run:  python tools/gen_short_block_golden.py
"""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uci_short_block as U  # noqa: E402  (encoder and rate matcher for the stimuli only; the verdicts come from the reference)

rng = np.random.default_rng(20261016)
MODS = (1, 2, 4, 6, 8)


def build_driver():
    exe = os.path.join(ROOT, "oracle", "_ref", "gen_short_block_golden")
    lib = os.path.join(ROOT, "oracle", "_ref", "libsrsran_ref.a")
    inc = ["-I%s/include" % REF, "-I%s/external/fmt/include" % REF, "-I%s/external" % REF, "-I%s" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-w", "-mavx", "-mavx2", "-mfma"] + inc +
                          [os.path.join(ROOT, "tools", "gen_short_block_golden.cpp"), lib, "-lpthread", "-o", exe])
    return exe


def lengths(K, m):
    if K == 1:
        return [m, m + 1, 7 * m, 37, 2001]
    if K == 2:
        return [3 * m, 3 * m + 1, 12 * m, 101, 2003]
    return [K + 1, 31, 45, 97, 2049]


def quant(y, scale):
    return np.clip(np.round(scale * y), -U.LLR_MAX, U.LLR_MAX).astype(np.int64)


def stimuli():
    """(K, Qm, llr) records."""
    out = []
    for K in range(1, 12):
        for m in MODS:
            for E in lengths(K, m):
                long = E >= 2000
                msg = rng.integers(0, 2, K, dtype=np.uint8)
                s = 1.0 - 2.0 * U.rate_match(U.encode(msg, m), E)
                out.append((K, m, quant(s, rng.integers(1, 121))))  # clean +-k
                # AWGN: noise only, then from below to above the detection threshold (long blocks: fewer draws)
                for sigma in ((None, 1.0) if long else (None, 8.0, 4.0, 2.5, 1.6, 1.0, 0.5)):
                    for _ in range(1 if long else 3):
                        msg = rng.integers(0, 2, K, dtype=np.uint8)
                        s = 1.0 - 2.0 * U.rate_match(U.encode(msg, m), E)
                        y = rng.standard_normal(E) if sigma is None else s + sigma * rng.standard_normal(E)
                        out.append((K, m, quant(y, rng.choice([4.0, 12.0, 30.0]))))
                if long:
                    continue
                # +-127 among finite values
                x = rng.integers(-120, 121, E)
                inf = rng.random(E) < 0.15
                x[inf] = 127 * rng.choice([-1, 1], int(inf.sum()))
                out.append((K, m, x))
                # small integers: many exact correlation ties and zero accumulators
                out.append((K, m, rng.integers(-2, 3, E)))
            # all-zero input; both infinities into one accumulator (then further values); clamp and recover
            L = m if K == 1 else (3 * m if K == 2 else 32)
            E = max(lengths(K, m)[0], 3 * L)
            out.append((K, m, np.zeros(E, np.int64)))
            x = rng.integers(-30, 31, E)
            x[:L] = 127 * rng.choice([-1, 1], L)
            x[L:2 * L] = -x[:L]
            out.append((K, m, x))
            x = rng.integers(-10, 11, 5 * L)
            x[:L], x[L:2 * L], x[2 * L:3 * L] = 100, 100, -100  # 100 + 100 clamps to 120, - 100 leaves 20 (not 100)
            x[3 * L:4 * L] = rng.choice([-1, 1], L) * 119
            out.append((K, m, x))
    # exact ties between two codewords for K >= 3: x = a c_p + b c_q with |corr| equal
    for K in range(3, 12):
        for m in MODS:
            for _ in range(4):
                ncw = 1 << (K - 1)
                p, q = sorted(rng.choice(ncw, 2, replace=False))
                sgn = rng.choice([-1, 1])
                x = 5 * (U.SIGNS[p] + sgn * U.SIGNS[q])
                out.append((K, m, np.concatenate([x, np.zeros(int(rng.integers(0, 3)) * 32, np.int64)])))
    return out


def main():
    exe = build_driver()
    recs = stimuli()
    blob = [struct.pack("<I", len(recs))]
    for K, m, x in recs:
        assert np.all((np.abs(x) <= U.LLR_MAX) | (np.abs(x) == U.LLR_INFTY))
        blob.append(struct.pack("<III", K, m, len(x)) + x.astype(np.int8).tobytes())
    res = subprocess.run([exe], input=b"".join(blob), stdout=subprocess.PIPE, check=True).stdout
    K = np.array([r[0] for r in recs], np.uint8)
    mod = np.array([r[1] for r in recs], np.uint8)
    E = np.array([len(r[2]) for r in recs], np.uint32)
    off = np.concatenate([[0], np.cumsum(E.astype(np.uint64))[:-1]]).astype(np.uint64)
    llr = np.concatenate([r[2] for r in recs]).astype(np.int8)
    poff = np.concatenate([[0], np.cumsum(K.astype(np.uint64))[:-1]]).astype(np.uint64)
    payload = np.zeros(int(K.sum()), np.uint8)
    status = np.zeros(len(recs), np.uint8)
    pos = 0
    for i, k in enumerate(K.tolist()):
        payload[poff[i]:poff[i] + k] = np.frombuffer(res[pos:pos + k], np.uint8)
        status[i] = U.STATUS_VALID if res[pos + k] else U.STATUS_INVALID
        pos += k + 1
    assert pos == len(res)
    for k in range(3, 12):
        v = status[K == k]
        assert (v == U.STATUS_VALID).any() and (v == U.STATUS_INVALID).any(), ("both verdicts", k)
    path = os.path.join(ROOT, "tests", "golden", "short_block_detector.npz")
    np.savez_compressed(path, K=K, mod=mod, E=E, llr_offset=off, llr=llr, payload_offset=poff, payload=payload, status=status)
    print("%d fields, %d soft bits, %.1f KiB" % (len(recs), llr.size, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
