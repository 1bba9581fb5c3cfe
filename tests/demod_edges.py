"""Crafted inputs for the soft demapper (csrc/demod_device.h, csrc/pusch_demod.hip), on the host in numpy float32: no device, no reference.

Random symbols never land on the places where the three device forms of the demapper (packed, fast, exact) could part: a scaled value exactly at
n + 0.5, one ulp either side of the clip, a symbol on an interval boundary, a reciprocal noise variance that is subnormal or infinite. This module
makes such inputs on purpose, per modulation order, as real components x with the class each belongs to:

  boundary   every interior boundary k * width of the interval grids of tables/nr_demod_tables.h (64-QAM: 8 and 4 intervals, 256-QAM: 16 and 8),
             the nearest float32 and two neighbours on either side
  threshold  +- the 16-QAM threshold and its neighbours
  zero       0 and its neighbours (the two smallest subnormals of either sign)
  beyond     +-(count / 2 + 1) * width, +-8, +-1e6: the interval index clamps
  tie        the scaled value (l * rcp * scale in float32, operations in the order of demod_device.h) is exactly n + 0.5: found by solving for x and
             scanning +-64 ulps; even and odd n, both signs, for every soft-bit function of the modulation
  clip       scaled value 119.5, the float below 120, 120, the float above 120, 120.5, 1e6 (pi/2-BPSK: the clip of the LLR at +-24 likewise)
  tiny       +-0, +-the smallest subnormal, +-FLT_MIN
  nonfinite  +-Inf and NaN in re only, in im only and in both, +-FLT_MAX, crossed with one representative of every finite class

Every element carries the noise variance it wants: nv = base * 4^-k, which an estimate h = 2^k delivers exactly (z = y 2^-k, nv = noise_var 2^-2k).
The noise classes (reciprocal subnormal, reciprocal infinite with a zero component, h = 0, |h|^2 subnormal) ride on ordinary symbols.
lay() puts a set of elements into a resource grid and an estimate for an allocation and returns the oracle's arguments with them."""
import os
import re

import numpy as np

F = np.float32
MODS = (1, 2, 4, 6, 8)
TIE_NVS = ((1.0, 0), (1.0, 1), (0.1, 0), (0.037, 0))  # (base, k): nv = 1, 0.25, 0.1, 0.037
CLIP_NVS = TIE_NVS + ((0.037, 1), (0.037, 3))  # the innermost tables reach +-120 only under a small variance: 0.00925, 0.000578
TIE_N = (0, 1, 2, 3, 6, 7, 20, 21, 58, 59, 118, 119)
CLIP_TARGETS = (F(119.5), np.nextafter(F(120), F(0)), F(120), np.nextafter(F(120), F(np.inf)), F(120.5), F(1e6))
FLT_MAX, FLT_MIN, DENORM = np.finfo(F).max, np.finfo(F).tiny, F(1e-45)
H_POW2, H_ZERO, H_SUB_REAL, H_SUB_COMPLEX = 0, 1, 2, 3  # the estimate of an element: 2^k, 0, 2^-64 (|h|^2 subnormal, its reciprocal infinite), 2^-64 (1 + i)


def _tables():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "srsran_project_23.5_amd", "csrc", "tables", "nr_demod_tables.h")
    txt = open(path).read()
    num = lambda s: F(float.fromhex(s.strip().rstrip("f")))  # noqa: E731
    t = {m.group(1): num(m.group(2)) for m in re.finditer(r"#define NR_DEMOD_(\w+) (-?0x[0-9a-fp.+-]+f)", txt)}
    for m in re.finditer(r"NR_DEMOD_(\w+)\[\d+\] = \{([^}]*)\}", txt):
        t[m.group(1)] = np.array([num(v) for v in m.group(2).split(",")], F)
    return t


T = _tables()
FUNCS = {1: ("bpsk",), 2: ("qpsk",), 4: ("first", "second", "l23"), 6: ("B0", "B1", "B2"), 8: ("B0", "B1", "B2", "B3")}
GRIDS = {6: (("B0", 8), ("B2", 4)), 8: (("B0", 16), ("B3", 8))}  # the interval grids a modulation indexes: (table that names the width, count)


def nv_of(base, k):
    """The variance the equaliser hands to the demapper for noise_var = base and h = 2^k: rcpd * noise_var, rcpd = 2^-2k."""
    return F(2.0 ** (-2 * k)) * F(base)


def interval_idx(mod, name, x):
    f = np.floor(x * T["QAM%d_%s_RCP_WIDTH" % (2 ** mod, name)])
    count = T["QAM%d_%s_SLOPE" % (2 ** mod, name)].size
    return np.clip(f.astype(np.int64) + count // 2, 0, count - 1)


def scaled(mod, fn, x, nv):
    """The value the quantiser clips and rounds (float32, one rounding per operation, order of demod_device.h); NaN where fn does not apply to x."""
    x = np.asarray(x, F)
    nv = F(nv)
    with np.errstate(all="ignore"):
        if mod == 1:  # v = gain * (a + b) / nvar with the other component 0; the LLR is clipped at +-24 before this scale
            return T["QPSK_GAIN"] * x / nv / F(24) * F(120)
        rcp = F(1) / nv
        if mod == 2:
            return T["QPSK_GAIN"] * x * rcp * F(5)
        if mod == 4:
            first = T["QAM16_GAIN"] * x
            outer = np.abs(x) > T["QAM16_THRESHOLD"]
            if fn == "first":
                return np.where(outer, F(np.nan), first * rcp * F(6))
            if fn == "second":
                return np.where(outer, (F(2) * first - np.copysign(F(0.8), x)) * rcp * F(6), F(np.nan))
            return (F(0.8) - np.abs(first)) * rcp * F(6)
        q = "QAM%d_%s_" % (2 ** mod, fn)
        i = interval_idx(mod, fn, x)
        return (T[q + "SLOPE"][i] * x + T[q + "INTERCEPT"][i]) * rcp * F(6)


def _pieces(mod, fn):
    """The linear pieces (slope, intercept, lo, hi) of a soft-bit function before the noise and the scale, in float64."""
    inf = np.inf
    if mod <= 2:
        return [(float(T["QPSK_GAIN"]), 0.0, -inf, inf)]
    if mod == 4:
        g, th = float(T["QAM16_GAIN"]), float(T["QAM16_THRESHOLD"])
        return {"first": [(g, 0.0, -th, th)], "second": [(2 * g, 0.8, -inf, -th), (2 * g, -0.8, th, inf)], "l23": [(g, 0.8, -inf, 0.0), (-g, 0.8, 0.0, inf)]}[fn]
    q = "QAM%d_%s_" % (2 ** mod, fn)
    s, c, w = T[q + "SLOPE"].astype(float), T[q + "INTERCEPT"].astype(float), float(T[q + "WIDTH"])
    n = s.size
    return [(s[i], c[i], -inf if i == 0 else (i - n // 2) * w, inf if i == n - 1 else (i + 1 - n // 2) * w) for i in range(n)]


def _around(x, n):
    """x and its n float32 neighbours on either side."""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.array(sorted(out), F)


def _solve(mod, fn, nv, target, exact=True):
    """Inputs x (one per linear piece at most) whose scaled value is `target`: bit-exactly, or else (exact=False) as near as +-64 ulps allow."""
    out = []
    gain = (120.0 / 24.0 if mod <= 2 else 6.0) / float(nv)
    for pc, (a, b, lo, hi) in enumerate(_pieces(mod, fn)):
        x0 = (float(target) / gain - b) / a
        if not (lo <= x0 < hi) or abs(x0) > 1e30:
            continue
        cand = _around(x0, 64)
        s = scaled(mod, fn, cand, nv)
        hit = np.nonzero(s == F(target))[0]
        if hit.size:
            out.append((pc, cand[hit[hit.size // 2]], True))
        elif not exact:  # the nearest scaled value on the same side of the clip as the target
            side = np.isfinite(s) & ((np.abs(s) < 120) == (abs(target) < 120)) & ((np.abs(s) > 120) == (abs(target) > 120))
            if side.any():
                out.append((pc, cand[side][np.argmin(np.abs(s[side].astype(float) - float(target)))], False))
    return out


def components(mod):
    """[(x, base, k, class)]: the crafted real components of a modulation, each with the noise variance nv_of(base, k) it is meant for."""
    out = []
    nvs = TIE_NVS
    # ---- ties: at most two per (function, piece, sign, parity of n), from different noise variances where there are several
    for fn in FUNCS[mod]:
        kept = {}
        for n in TIE_N:
            for sign in (1, -1):
                for base, k in nvs:
                    for pc, x, _ in _solve(mod, fn, nv_of(base, k), sign * (n + 0.5)):
                        key = (pc, sign, n & 1)
                        if kept.setdefault(key, 0) < 2:
                            kept[key] += 1
                            out.append((x, base, k, "tie:%s:%s:%s" % (fn, "+" if sign > 0 else "-", "odd" if n & 1 else "even")))
        for sign in "+-":
            for par in ("even", "odd"):
                assert any(c == "tie:%s:%s:%s" % (fn, sign, par) for _, _, _, c in out), "no tie for modulation %d, %s, %s, n %s" % (mod, fn, sign, par)
    # ---- clip: the first exact solution per (function, target, sign); the nearest one where +-64 ulps hold no exact one
    for fn in FUNCS[mod]:
        for t in CLIP_TARGETS:
            for sign in (1, -1):
                found = [(x, base, k, ex) for base, k in CLIP_NVS for _, x, ex in _solve(mod, fn, nv_of(base, k), sign * t, exact=False)]
                found.sort(key=lambda f: not f[3])
                for x, base, k, ex in found[:1]:
                    out.append((x, base, k, "clip:%s:%s%s" % (fn, "+" if sign > 0 else "-", "%.9g" % t if ex else "near%.9g" % t)))
    # ---- boundaries, threshold, zero, beyond: on the ordinary noise variances in turn
    plain = []
    for name, count in GRIDS.get(mod, ()):
        w = float(T["QAM%d_%s_WIDTH" % (2 ** mod, name)])
        for kk in range(-(count // 2 - 1), count // 2):
            if kk:
                plain += [(x, "boundary:%s:%d" % (name, kk)) for x in _around(kk * w, 2)]
        plain += [(F(s * (count // 2 + 1) * w), "beyond:%s" % name) for s in (1, -1)]
    if mod == 4:
        plain += [(x, "threshold") for s in (1, -1) for x in _around(s * T["QAM16_THRESHOLD"], 2)]
    plain += [(x, "zero") for x in _around(0.0, 2)]
    plain += [(F(v), "beyond") for v in (8, -8, 1e6, -1e6)]
    plain += [(F(v), "tiny") for v in (0.0, -0.0, DENORM, -DENORM, FLT_MIN, -FLT_MIN)]
    out += [(x, nvs[i % len(nvs)][0], nvs[i % len(nvs)][1], c) for i, (x, c) in enumerate(plain)]
    return out


ELEM = np.dtype([("re", F), ("im", F), ("base", F), ("k", np.int32), ("hmode", np.int32), ("cre", np.int32), ("cim", np.int32)])
NONFINITE = (F(np.inf), F(-np.inf), F(np.nan))
# noise classes: (name, base, k, hmode). nv = base 4^-k: 3 * 2^126 has a subnormal reciprocal, 0.037 * 2^-126 is subnormal and its reciprocal infinite.
NOISE_CLASSES = (("noise:rcp_subnormal", 3.0, -63, H_POW2), ("noise:rcp_infinite", 0.037, 63, H_POW2), ("noise:h_zero", 1.0, 0, H_ZERO),
                 ("noise:h2_subnormal", 1.0, 0, H_SUB_REAL), ("noise:h2_subnormal_complex", 0.037, 0, H_SUB_COMPLEX))
NOISE_SYMBOLS = ((0.0, 0.5), (0.5, 0.0), (0.0, 0.0), (-0.75, 0.25), (1.5, -1e-30), (1.0, -1.0))
NOISE_SYMBOLS_LARGE = NOISE_SYMBOLS[:4] + ((1e30, -3e37), (3e38, 1.0))  # under the largest variance only large symbols give a soft bit other than 0
_cache = {}


def elements(mod):
    """(elements, class names): the crafted symbols of a modulation as ELEM records; cre / cim index the class names."""
    if mod in _cache:
        return _cache[mod]
    comp = components(mod)
    names = sorted({c for _, _, _, c in comp}) + ["filler", "nonfinite"] + [n for n, _, _, _ in NOISE_CLASSES]
    ci = {n: i for i, n in enumerate(names)}
    rows = []
    groups = {}
    for x, base, k, c in comp:
        groups.setdefault((base, k), []).append((x, ci[c]))
    for (base, k), g in sorted(groups.items()):
        m = len(g)
        for i, (x, c) in enumerate(g):
            if mod == 1:  # the soft bit is a function of re + im (or im - re): the crafted component beside a zero, in re and in im in turn
                rows.append((x, 0, base, k, H_POW2, c, ci["zero"]) if i % 2 == 0 else (0, x, base, k, H_POW2, ci["zero"], c))
            else:  # a fixed permutation pairs the list with itself: every component is once the real and once the imaginary part
                y, cy = g[(i + m // 3 + 1) % m]
                rows.append((x, y, base, k, H_POW2, c, cy))
    # ---- non-finite values: with each other, and with one representative of every finite class (the first of the class, on its own noise variance)
    nf = ci["nonfinite"]
    for a in NONFINITE:
        for b in NONFINITE:
            rows.append((a, b, 1.0, 0, H_POW2, nf, nf))
    reps = {}
    for x, base, k, c in comp:
        reps.setdefault(c.split(":")[0] + ":" + (c.split(":")[1] if c.startswith(("tie", "clip")) else ""), (x, base, k, ci[c]))
    for x, base, k, c in reps.values():
        big = F(FLT_MAX * 4.0 ** -max(k, 0))  # (the largest value that passes the equaliser on h = 2^k: the sum y conj(h) must stay finite)
        for a in NONFINITE + (big, -big):
            z = ci["zero"]
            if mod == 1:
                rows += [(a, 0, base, k, H_POW2, nf, z), (0, a, base, k, H_POW2, z, nf)]
            rows += [(a, x, base, k, H_POW2, nf, c), (x, a, base, k, H_POW2, c, nf)]
    rows += [(FLT_MAX, -FLT_MAX, 1.0, 0, H_POW2, nf, nf), (-FLT_MAX, FLT_MAX, 0.037, 0, H_POW2, nf, nf)]
    # ---- noise classes
    for name, base, k, hmode in NOISE_CLASSES:
        rows += [(a, b, base, k, hmode, ci[name], ci[name]) for a, b in (NOISE_SYMBOLS_LARGE if k < 0 else NOISE_SYMBOLS)]
    el = np.array(rows, dtype=ELEM)
    _cache[mod] = (el, names)
    return _cache[mod]


def is_noise_class(el):
    """Elements that need an estimate of their own on every resource element (only the 14-symbol estimate can carry them)."""
    return (el["hmode"] != H_POW2) | (np.abs(el["k"]) > 8)


def delivered_exactly(el):
    """Finite symbol on a normal power-of-two estimate: the equaliser must hand symbol and variance to the demapper bit for bit (a -0 component
    arrives as +0: the equaliser's sums start at +0)."""
    return np.isfinite(el["re"]) & np.isfinite(el["im"]) & (el["hmode"] == H_POW2)


def nv_direct(el):
    """The variance of each element as the standalone demapper takes it (one per symbol): what the equaliser would have produced."""
    nv = np.array([nv_of(b, k) for b, k in zip(el["base"], el["k"])], F)
    nv[el["hmode"] != H_POW2] = np.inf  # a dead or subnormal estimate: infinite variance ...
    m = el["hmode"] == H_SUB_COMPLEX
    nv[m] = F(2.0 ** 127) * el["base"][m]  # ... but |h|^2 = 2^-127 has a finite reciprocal
    return nv


ABNORMAL_NOISE_VARS = (0.0, -1.0, np.inf, np.nan, 1e-40)  # job noise variances: zero, negative, infinite, NaN, subnormal


def fixture_inputs(mod):
    """Symbols and per-symbol variances for the standalone demapper: every crafted element, then the ordinary ones of nv = 1 again under each
    abnormal variance, padded with fillers to a multiple of 32 symbols."""
    el, _ = elements(mod)
    sym = np.empty(el.size, np.complex64)
    sym.real, sym.imag = el["re"], el["im"]  # (keeps NaN / Inf parts apart)
    nv = nv_direct(el)
    plain = (el["base"] == 1.0) & (el["k"] == 0) & (el["hmode"] == H_POW2)
    syms, nvs = [sym], [nv]
    for v in ABNORMAL_NOISE_VARS:
        syms.append(sym[plain])
        nvs.append(np.full(int(plain.sum()), v, F))
    sym, nv = np.concatenate(syms), np.concatenate(nvs)
    pad = -sym.size % 32
    return np.concatenate([sym, np.full(pad, 0.25 - 0.125j, np.complex64)]), np.concatenate([nv, np.ones(pad, F)])


def reference_comparable(nv, mod):
    """Per LLR: whether the reference's value binds the oracle. Left out, one class: a positive variance below 2^-100 (the subnormal variances 1e-40
    and 0.037 * 2^-126). Its reciprocal is infinite, so a soft bit is +-120 or 0 (0 * inf) according to whether the interval function is exactly
    zero, where the reference's build contracts slope * x + intercept into one rounding and the oracle rounds twice; and the reference's scalar code
    divides by the variance instead (a subnormal symbol then gives 0 where its vector body gives +-120)."""
    nv = np.asarray(nv, F)
    return np.repeat(~((nv > 0) & (nv < F(2.0 ** -100))), mod)


def compare_with_reference(mod, nv, oracle_llr, ref_llr):
    """(largest |oracle - reference| over the LLRs that bind, share of exact matches among them)."""
    keep = reference_comparable(nv, mod)
    diff = np.abs(oracle_llr.astype(int) - ref_llr.astype(int))[keep]
    return int(diff.max()), float((diff == 0).mean())


# ------------------------------------------------------------------------------------------------ delivery through a resource grid
FILLER = (F(0.25), F(-0.125))


def data_positions(rb, dm, start, nof, cdm):
    """(symbol, subcarrier) of every data element in codeword order (DM-RS type 1)."""
    sub = np.nonzero(np.repeat(rb, 12))[0]
    data = sub[(sub % 12) % 2 >= cdm]
    sy, sc = [], []
    for s in range(start, start + nof):
        keep = data if dm[s] else sub
        sy.append(np.full(keep.size, s))
        sc.append(keep)
    return np.concatenate(sy), np.concatenate(sc)


def lay(mod, el, noise_var, compact, ports=1, layers=1, nprb_grid=25, prbs=tuple(range(1, 12)) + tuple(range(13, 24)), start=1, nof=13, dmrs=(3,), cdm=1,
        rnti=0x4601, n_id=77):
    """The elements `el` (one noise base, the job's noise_var; with a compact estimate no noise classes) on the data elements of an allocation.
    One layer: element e sits at codeword position slot[e]; `layers` > 1: codeword symbol slot[e] = layers * resource element + layer, through a
    diagonal channel. compact: one estimate row, so the elements of a subcarrier share k; subcarriers are filled group by group.
    Returns dict(grid [4 or ports][14][nsc], ce [ports][rows][nsc] (layers > 1: [layers][ports][rows][nsc]), slot, n_re, rb, dm, args=the oracle's
    arguments (one layer), and the allocation)."""
    rb = np.zeros(nprb_grid, np.uint8)
    rb[list(prbs)] = 1
    dm = np.zeros(14, np.uint8)
    dm[list(dmrs)] = 1
    sy, sc = data_positions(rb, dm, start, nof, cdm)
    n_re, nsc, L = sy.size, nprb_grid * 12, layers
    rows = 1 if compact else 14
    z = np.empty(n_re * L, np.complex64)
    z.real, z.imag = FILLER
    kk = np.zeros(n_re * L, np.int64)
    hm = np.full(n_re * L, H_POW2)
    slot = np.full(el.size, -1)
    if compact:
        assert not is_noise_class(el).any()
        cols = {}
        for i, c in enumerate(sc):
            cols.setdefault(int(c), []).extend(range(i * L, i * L + L))
        col_iter = iter(sorted(cols))
        for k in sorted(set(el["k"].tolist())):
            todo = list(np.nonzero(el["k"] == k)[0])
            while todo:
                for s in cols[next(col_iter)]:  # (StopIteration: the allocation is too small for the set)
                    kk[s] = k
                    if todo:
                        slot[todo.pop(0)] = s
    else:
        assert el.size <= n_re * L
        slot[:] = np.arange(el.size)
        kk[slot], hm[slot] = el["k"], el["hmode"]
    z.real[slot], z.imag[slot] = el["re"], el["im"]
    with np.errstate(all="ignore"):
        h = np.where(hm == H_ZERO, 0, np.where(hm == H_POW2, 2.0 ** kk, 2.0 ** -64)).astype(np.complex64)
        h[hm == H_SUB_COMPLEX] *= np.complex64(1 + 1j)
        y = np.empty_like(z)
        g = np.where(hm == H_ZERO, 1, h.real).astype(F)
        y.real, y.imag = z.real * g, z.imag * g  # (h real on every exact element; elsewhere any sample does)
    z, y, h = z.reshape(n_re, L), y.reshape(n_re, L), h.reshape(n_re, L)
    nan = np.complex64(np.nan + 1j * np.nan)
    if L == 1:
        grid = np.full((ports, 14, nsc), nan, np.complex64)
        ce = np.ones((ports, rows, nsc), np.complex64)
        grid[0, sy, sc], ce[0, 0 if compact else sy, sc] = y[:, 0], h[:, 0]
        grid[1:, sy, sc], ce[1:] = np.complex64(0.5 - 0.25j), 0  # further ports: a finite sample on a zero estimate adds exactly nothing
        args = (rnti, n_id, mod, start, nof, dm, 0, cdm, rb, grid, np.repeat(ce, 14, axis=1) if compact else ce, noise_var)
    else:
        assert ports == L
        grid = np.full((4, 14, nsc), nan, np.complex64)
        ce = np.zeros((L, ports, rows, nsc), np.complex64)
        for l in range(L):
            grid[l, sy, sc], ce[l, l, 0 if compact else sy, sc] = y[:, l], h[:, l]
        args = None
    return dict(mod=mod, grid=grid, ce=ce, slot=slot, n_re=n_re, rb=rb, dm=dm, args=args, noise_var=noise_var, compact=compact, ports=ports, layers=L,
                start=start, nof=nof, cdm=cdm, rnti=rnti, n_id=n_id, el=el, prbs=tuple(prbs), dmrs=tuple(dmrs), nprb_grid=nprb_grid)


def bases(mod, with_noise_classes):
    """The job noise variances the crafted set of a modulation needs, and the elements of each."""
    el, _ = elements(mod)
    if not with_noise_classes:
        el = el[~is_noise_class(el)]
    return [(float(b), el[el["base"] == b]) for b in sorted(set(el["base"].tolist()))]
