#!/usr/bin/env python3
"""Records tests/golden/prach_demod.npz: the reference's own OFDM PRACH demodulator (create_ofdm_prach_demodulator_factory_sw over the
generic DFT, driven by tools/gen_prach_demod_golden.cpp with a sentinel-filled prach_buffer_impl) on windows that
tests/prach_demod_ref.py builds from a seed:
- every format (0..3 with few cases, their outputs being the large ones; A1..C2 and the A/B pairs);
- PUSCH subcarrier spacings 15 / 30 / 60 kHz wherever the frequency mapping is not reserved and the geometry fits;
- sampling rates 7.68, 15.36, 23.04, 30.72 and 61.44 MHz;
- 1..4 frequency-domain occasions, with the sequences in the lower half of the PRACH grid, in the upper half and across its middle;
- several time-domain occasions, among them one that starts exactly at 0.5 ms, ones that span it and one that ends exactly on it, and
  A/B pairs with two and more occasions (the last one takes the B cyclic prefix).
Per case: the configuration row (sampling rate first), the seed, the SHA-256 of the window's bytes and the reference's complete
output [td][fd][symbol][L], flattened. The windows themselves are not stored. Prints the largest distance between the reference and the
float64 restatement (max |difference| / rms of the expected).
Needs the reference library build() compiles (oracle/_ref/libsrsran_ref.a) and its sources.
Run:  python tools/gen_prach_demod_golden.py [--time]
"""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prach_demod_ref as D  # noqa: E402

rng = np.random.default_rng(20261018)
LOW, UPPER, ACROSS = range(3)


def build_driver():
    exe = os.path.join(ROOT, "oracle", "_ref", "gen_prach_demod_golden")
    lib = os.path.join(ROOT, "oracle", "_ref", "libsrsran_ref.a")
    inc = ["-I%s/include" % REF, "-I%s/external/fmt/include" % REF, "-I%s/external" % REF, "-I%s" % REF]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-mavx", "-mavx2", "-mfma", "-DHAVE_SSE", "-DHAVE_AVX", "-DHAVE_AVX2",
                           "-DHAVE_FMA"] + inc + [os.path.join(ROOT, "tools", "gen_prach_demod_golden.cpp"), lib, "-lpthread", "-o", exe])
    return exe


def config(srate, fmt, mu, ntd, nfd, start, where, extra=0):
    """A configuration row with the sequences of its frequency-domain occasions placed `where` in the grid, or None if the reference
    would assert on it."""
    if fmt < 4:
        scs_hz = 5000 if fmt == 3 else 1250
        L = 839
    else:
        scs_hz, L = 15000 << mu, 139
    if (scs_hz, mu) not in D.FREQ_MAP or srate % scs_hz:
        return None
    N, K = srate // scs_hz, (15000 << mu) // scs_hz
    nof_rb_ra, k_bar = D.FREQ_MAP[(scs_hz, mu)]
    nprb = min((N - 1) // (K * 12), (106, 51, 24, 12)[mu] * max(1, srate // 30720000))
    span_rb = nof_rb_ra * nfd
    if where == LOW:
        rb = 0
    elif where == UPPER:
        rb = nprb - span_rb - 1
    else:  # the middle of the grid falls inside the first occasion's sequence
        rb = (nprb * K * 6 - k_bar - L // 2) // (K * 12)
    if rb < 0:
        return None
    c = np.array([srate, fmt, mu, ntd, nfd, start, rb, nprb, 1 << 30], np.int64)
    try:
        g = D.geometry(c)
    except ValueError:
        return None
    half = g["grid"] // 2
    k0, k1 = g["k_start"][0], g["k_start"][-1]
    if (where == LOW and k1 + L > half) or (where == UPPER and k0 < half) or (where == ACROSS and not k0 < half < k0 + L):
        return None
    last = max(o + cp + g["nof_symbols"] * N for o, cp in zip(g["td_sample_offset"], g["td_cp_samples"]))
    c[D.C_NSAMPLES] = max(g["window_samples"], last) + extra
    return c


def cases():
    out = []

    def add(*a, **k):
        c = config(*a, **k)
        assert c is not None, a
        out.append(c)

    # long formats: few cases, every sampling rate, every four-step size they reach and the single-pass sizes of format 3
    add(30720000, 0, 0, 1, 1, 0, LOW)
    add(30720000, 0, 1, 1, 4, 0, ACROSS)
    add(61440000, 0, 0, 1, 2, 0, ACROSS, extra=5)
    add(7680000, 0, 0, 1, 1, 2, UPPER)
    add(15360000, 0, 2, 1, 1, 0, ACROSS)
    add(23040000, 0, 1, 1, 2, 0, LOW)
    add(30720000, 1, 0, 1, 1, 0, UPPER)
    add(15360000, 2, 0, 1, 1, 0, ACROSS)
    add(30720000, 3, 0, 1, 1, 9, ACROSS)
    add(7680000, 3, 1, 1, 1, 0, ACROSS)   # N = 1536: the sequence is wider than half the grid
    add(23040000, 3, 2, 1, 1, 1, UPPER)
    # short formats: occasions at, across and up to 0.5 ms
    add(30720000, 4, 0, 1, 1, 7, LOW)        # A1 at 15 kHz starts exactly at 0.5 ms
    add(30720000, 4, 0, 4, 2, 1, ACROSS)     # ... as its fourth occasion
    add(30720000, 5, 0, 2, 1, 4, UPPER)      # A2: the first occasion spans 0.5 ms
    add(30720000, 4, 1, 1, 1, 12, ACROSS)    # A1 at 30 kHz ends exactly on 0.5 ms
    add(30720000, 4, 0, 3, 1, 5, LOW)        # A1 x 3 from symbol 5
    add(30720000, 11, 0, 3, 2, 0, ACROSS)    # A1/B1 x 3
    add(15360000, 12, 1, 3, 1, 2, UPPER)     # A2/B2 x 3
    add(23040000, 13, 0, 2, 2, 0, ACROSS)    # A3/B3 x 2
    add(61440000, 11, 1, 2, 4, 1, LOW)
    add(30720000, 9, 0, 2, 1, 0, ACROSS)     # C0 x 2
    add(7680000, 9, 1, 1, 1, 0, ACROSS)      # N = 256
    add(15360000, 8, 0, 1, 1, 0, ACROSS)     # B4, N = 1024
    add(30720000, 8, 1, 1, 1, 2, UPPER)
    # the rest: every short format at every spacing and sampling rate the geometry allows, parameters drawn
    for fmt in range(4, 14):
        duration = D.SHORT[fmt - 4][3]
        for mu in (0, 1, 2):
            for srate in D.SRATES:
                if srate == 46080000 or (fmt + mu + srate // 7680000) % 3:
                    continue
                for _ in range(8):
                    start = int(rng.integers(0, 14 - duration + 1))
                    ntd = int(rng.integers(1, min(D.MAX_TD, (14 - start) // duration) + 1))
                    c = config(srate, fmt, mu, ntd, int(rng.integers(1, 5)), start, int(rng.integers(0, 3)), extra=int(rng.integers(0, 8)))
                    if c is not None and c[D.C_NTD] * c[D.C_NFD] * D.SHORT[fmt - 4][0] <= 10:
                        out.append(c)
                        break
    return out


def main():
    exe = build_driver()
    if "--time" in sys.argv:
        subprocess.check_call([exe, "--time"])
        return
    cs = cases()
    seeds = [int(rng.integers(1, 2**62)) for _ in cs]
    stdin, sha, windows = [struct.pack("<I", len(cs))], [], []
    for c, seed in zip(cs, seeds):
        x = D.fixture_window(seed, c)
        windows.append(x)
        sha.append(D.window_hash(x))
        stdin.append(struct.pack("<9I", *[int(v) for v in c]) + x.tobytes())
    out = subprocess.run([exe], input=b"".join(stdin), stdout=subprocess.PIPE, check=True).stdout
    pos, offs, data, worst = 0, [0], [], 0.0
    for c, x in zip(cs, windows):
        ntd, nfd, nsym, L = struct.unpack("<4I", out[pos:pos + 16])
        pos += 16
        m = ntd * nfd * nsym * L
        y = np.frombuffer(out[pos:pos + 8 * m], np.complex64)
        pos += 8 * m
        ref = D.demodulate(x, c)
        assert ref.shape == (ntd, nfd, nsym, L), (c, ref.shape, (ntd, nfd, nsym, L))
        worst = max(worst, D.rel_err(y, ref))
        data.append(y)
        offs.append(offs[-1] + m)
    assert pos == len(out)
    path = os.path.join(ROOT, "tests", "golden", "prach_demod.npz")
    np.savez_compressed(path, cfg=np.stack(cs), seed=np.array(seeds, np.uint64), sha256=np.asarray(sha), out_offset=np.array(offs, np.int64),
                        out=np.concatenate(data))
    print("%s: %d cases, %d output samples, %d bytes; largest distance reference - restatement %.2e" %
          (path, len(cs), offs[-1], os.path.getsize(path), worst))


if __name__ == "__main__":
    main()
