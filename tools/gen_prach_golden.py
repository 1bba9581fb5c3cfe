#!/usr/bin/env python3
"""Records tests/golden/prach_detector.npz: the reference's own PRACH detector (create_prach_detector_factory_simple with the generic
IDFT of size 1536, driven by tools/gen_prach_golden.cpp) on symbols that tests/prach_ref.py builds from a seed:
- every format the reference serves (0..3, and A1..C2 with the A/B pairs at RA subcarrier spacings 15 and 30 kHz), every
  zeroCorrelationZoneConfig 0..15, root sequence indices including ones whose preamble range runs past the end of the root table;
- the full range of 64 preamble indices, partial ranges and empty ones;
- 0..4 transmitted preambles per occasion (two of them on one root with different shifts where the zone allows), with integer and
  fractional delays inside the detection window, beyond it and negative, from noise-free down to noise only, and all-zero symbols.
Per case: what detect() returned. Per case and requested preamble: peak index, peak power and metric of the driver's replay of the
detector's steps. The symbols themselves are not stored: per case, the seed, the transmitter parameters and the SHA-256 of the symbol
bytes the reference saw.
The generator part: eight samples of every logical root at shift 0 (838 long, 138 short), from which tools/gen_prach_tables.py reads
the root order back, and eight complete sequences of each length with non-zero shifts.
Needs the reference library build() compiles (oracle/_ref/libsrsran_ref.a) and its sources.
Run:  python tools/gen_prach_golden.py [--time]
"""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prach_ref as P  # noqa: E402
from gen_prach_tables import recover_root_order  # noqa: E402

rng = np.random.default_rng(20261018)
NOISE = (0.0, 0.01, 0.1, 0.3, 1.0, 3.0)
POS_LONG = np.array([0, 1, 2, 3, 57, 419, 700, 838])
POS_SHORT = np.array([0, 1, 2, 3, 29, 69, 100, 138])
FORMATS = [(f, 0) for f in range(4)] + [(f, s) for f in range(4, 14) for s in (0, 1)]


def build_driver():
    exe = os.path.join(ROOT, "oracle", "_ref", "gen_prach_golden")
    lib = os.path.join(ROOT, "oracle", "_ref", "libsrsran_ref.a")
    inc = ["-I%s/include" % REF, "-I%s/external/fmt/include" % REF, "-I%s/external" % REF, "-I%s" % REF]
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-mavx", "-mavx2", "-mfma", "-DHAVE_SSE", "-DHAVE_AVX", "-DHAVE_AVX2",
                           "-DHAVE_FMA"] + inc + [os.path.join(ROOT, "tools", "gen_prach_golden.cpp"), lib, "-lpthread", "-o", exe])
    return exe


def generate(exe, reqs):
    """reqs: (format, root_sequence_index, zero_correlation_zone, preamble_index) -> list of complex64 sequences."""
    inp = struct.pack("<II", 0, len(reqs)) + b"".join(struct.pack("<4I", *r) for r in reqs)
    out = subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout
    seqs, pos = [], 0
    for _ in reqs:
        (L,) = struct.unpack("<I", out[pos:pos + 4])
        seqs.append(np.frombuffer(out[pos + 4:pos + 4 + 8 * L], np.complex64))
        pos += 4 + 8 * L
    assert pos == len(out)
    return seqs


def cases():
    """(cfg, seed, noise, tx_idx, tx_delay, tx_amp) per occasion."""
    out = []
    for i in range(252):
        fmt, scs = FORMATS[i % len(FORMATS)]
        zcz = (i * 7 + i // 16) % 16
        d = P.derive(fmt, scs, zcz)
        L, n_cs, dmax = d["L"], d["n_cs"], d["delay_n_maximum"]
        per_root = L // n_cs if n_cs else 1
        root = int(rng.integers(0, L - 1))
        if i % 7 == 3:
            root = L - 2 - int(rng.integers(0, 2))  # the preamble range runs past the last logical root
        kind = i % 10
        if kind < 6:
            start, nof = 0, 64
        elif kind < 9:
            start = int(rng.integers(0, 64))
            nof = int(rng.integers(1, 65 - start))
        else:
            start, nof = int(rng.integers(0, 65)), 0
        ntx = (i // 3) % 5
        noise = NOISE[(i * 5 + i // 6) % len(NOISE)]
        if i in (41, 127, 203):
            ntx, noise = 0, 0.0  # all-zero symbols
        lo, hi = (start, start + nof) if nof else (0, 64)
        idx = []
        if ntx >= 2 and per_root >= 2:
            a = int(rng.integers(lo, hi))
            a -= (a % per_root == per_root - 1)
            if a >= 0 and a + 1 < 64:
                idx = [a, a + 1]  # one root, neighbouring shifts
        while len(idx) < ntx:
            a = int(rng.integers(lo, hi)) if rng.random() < 0.85 else int(rng.integers(0, 64))
            if a not in idx:
                idx.append(a)
        delay = []
        for k in range(ntx):
            what = (i + 2 * k) % 6
            if what == 0:
                v = 0.0
            elif what == 1:
                v = float(rng.integers(0, max(1, min(dmax, 768))))
            elif what in (2, 5):
                v = float(rng.uniform(0, max(1, min(dmax, 768)) - 1))
            elif what == 3:
                v = float(min(dmax + int(rng.integers(0, 4)), 760))
            else:
                v = -float(rng.integers(1, 6)) if k % 2 == 0 else -float(rng.uniform(0.6, 5))
            delay.append(v)
        amp = [float(rng.uniform(0.5, 1.5)) for _ in range(ntx)]
        out.append((np.array([fmt, scs, root, zcz, start, nof], np.int32), int(rng.integers(1, 2**62)), noise, idx, delay, amp))
    return out


def main():
    exe = build_driver()
    if "--time" in sys.argv:
        subprocess.check_call([exe, "--time"])
        return
    # Generator part first: it yields the root order the transmitter needs.
    roots_long = generate(exe, [(0, r, 0, 0) for r in range(838)])
    roots_short = generate(exe, [(4, r, 0, 0) for r in range(138)])
    gen_roots_long = np.stack([s[POS_LONG] for s in roots_long])
    gen_roots_short = np.stack([s[POS_SHORT] for s in roots_short])
    tables = P.Tables(recover_root_order(839, POS_LONG, gen_roots_long))
    assert (recover_root_order(139, POS_SHORT, gen_roots_short) == tables.order[139]).all()

    def shifted(formats, L):
        """(format, root, zone, preamble index) with a non-zero cyclic shift."""
        out = []
        while len(out) < 8:
            f, r, z, k = int(rng.choice(formats)), int(rng.integers(0, L - 1)), int(rng.integers(1, 16)), int(rng.integers(1, 64))
            if P.root_and_shift(f, r, z, k, tables)[2] != 0:
                out.append((f, r, z, k))
        return out

    full_long, full_short = shifted(range(4), 839), shifted(range(4, 14), 139)
    gen_full_long = np.stack(generate(exe, full_long))
    gen_full_short = np.stack(generate(exe, full_short))

    cs = cases()
    n = len(cs)
    cfg = np.stack([c[0] for c in cs])
    tx_n = np.array([len(c[3]) for c in cs], np.int32)
    tx_idx = np.zeros((n, P.MAX_TX), np.int32)
    tx_delay = np.zeros((n, P.MAX_TX), np.float64)
    tx_amp = np.zeros((n, P.MAX_TX), np.float64)
    sha, stdin = [], [struct.pack("<II", 1, n)]
    for i, (c, seed, noise, idx, delay, amp) in enumerate(cs):
        tx_idx[i, :len(idx)], tx_delay[i, :len(idx)], tx_amp[i, :len(idx)] = idx, delay, amp
        sym = P.build_symbol(seed, c, noise, idx, delay, amp, tables)
        sha.append(P.symbol_hash(sym))
        stdin.append(struct.pack("<7I", *[int(v) for v in c], len(sym)) + sym.tobytes())
    out = subprocess.run([exe], input=b"".join(stdin), stdout=subprocess.PIPE, check=True).stdout

    rssi_db, rssi_lin = np.zeros(n, np.float32), np.zeros(n, np.float32)
    t_res, ta_max = np.zeros(n, np.int64), np.zeros(n, np.int64)
    det_off, pk_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    det_idx, det_ta, det_pow, pk_idx, pk_pow, pk_met = [], [], [], [], [], []
    pos = 0
    for i in range(n):
        rssi_db[i], rssi_lin[i], t_res[i], ta_max[i], nd = struct.unpack("<ffqqI", out[pos:pos + 28])
        pos += 28
        for _ in range(nd):
            a, b, c = struct.unpack("<Iqf", out[pos:pos + 16])
            det_idx.append(a), det_ta.append(b), det_pow.append(c)
            pos += 16
        for _ in range(int(cfg[i, P.C_NOF])):
            a, b, c = struct.unpack("<Iff", out[pos:pos + 12])
            pk_idx.append(a), pk_pow.append(b), pk_met.append(c)
            pos += 12
        det_off[i + 1], pk_off[i + 1] = len(det_idx), len(pk_idx)
    assert pos == len(out)
    path = os.path.join(ROOT, "tests", "golden", "prach_detector.npz")
    np.savez_compressed(
        path, cfg=cfg, seed=np.array([c[1] for c in cs], np.uint64), noise=np.array([c[2] for c in cs], np.float64), tx_n=tx_n, tx_idx=tx_idx,
        tx_delay=tx_delay, tx_amp=tx_amp, sha256=np.asarray(sha), rssi_db=rssi_db, rssi=rssi_lin, time_resolution_tc=t_res,
        time_advance_max_tc=ta_max, det_offset=det_off, det_index=np.asarray(det_idx, np.int32), det_time_advance_tc=np.asarray(det_ta, np.int64),
        det_power_db=np.asarray(det_pow, np.float32), peak_offset=pk_off, peak_index=np.asarray(pk_idx, np.int32),
        peak_power=np.asarray(pk_pow, np.float32), peak_metric=np.asarray(pk_met, np.float32), gen_positions_long=POS_LONG,
        gen_positions_short=POS_SHORT, gen_roots_long=gen_roots_long, gen_roots_short=gen_roots_short,
        gen_full_long_cfg=np.asarray(full_long, np.int32), gen_full_short_cfg=np.asarray(full_short, np.int32), gen_full_long=gen_full_long,
        gen_full_short=gen_full_short)
    print("%s: %d occasions, %d (occasion, preamble) pairs, %d detections, %d bytes" % (path, n, len(pk_idx), len(det_idx), os.path.getsize(path)))


if __name__ == "__main__":
    main()
