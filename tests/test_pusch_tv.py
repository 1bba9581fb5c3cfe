"""CPU: the float64 restatement of the estimator that follows a channel through the slot (tests/pusch_tv_cases.py) against what it can be held to
without a device: (a) the time weights; (b) noise free it returns the offset and, on every symbol, a channel that changes linearly in time; (c) with
one DM-RS symbol it is the CFO restatement; (d) the chain transmissions under two-ray gains decode through it where the CFO chain does not; (e)
exports, record size and header text."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pusch_cfo_cases as F
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import pusch_tv_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = E.CHAIN_CASES + [E.ONE_LAYER_CASE]
DMRS_SETS = ([2, 11], [2, 7, 11], [2, 5, 8, 11])
# (d) measured on the CPU, two_ray_gains(fd) with its default seed, every case at its listed SNR (all five decode through the new restatement with
# constant gains, fd = 0, so no SNR is raised). Decoded (1) or not (0) per case 0..4, "CFO chain / INTERPOLATE / LINE":
#   fd  100: 0/1/1 0/1/1 1/1/1 0/1/1 1/1/1      fd  600: 0/1/1 0/0/0 0/1/1 0/1/0 1/1/1      fd 1100: 0/0/0 0/0/0 0/0/0 0/0/0 0/1/0
#   fd  200: 0/1/1 0/1/1 1/1/1 0/1/1 1/1/1      fd  700: 0/1/1 0/0/0 0/1/1 0/0/0 1/1/1      fd 1200: 0/0/0 0/0/0 0/0/0 0/0/0 0/1/0
#   fd  300: 0/1/1 0/1/1 0/1/1 0/1/1 1/1/1      fd  800: 0/0/0 0/0/0 0/1/1 0/0/0 1/1/1      fd 1300 .. 1500: nothing decodes
#   fd  400: 0/1/1 0/1/1 0/1/1 0/1/1 1/1/1      fd  900: 0/0/0 0/0/0 0/1/1 0/0/0 1/1/1
#   fd  500: 0/1/1 0/0/0 0/1/1 0/1/1 1/1/1      fd 1000: 0/0/0 0/0/0 0/1/0 0/0/0 0/1/1
# FD_HZ is the smallest of 100, 200, ... 1500 Hz at which the CFO chain no longer decodes every case (every case has at least two DM-RS symbols): at
# 100 Hz it fails cases 0, 1 and 3. Margin of INTERPOLATE per case, the largest fd up to which it decodes without a gap: 700, 400, 1000, 600, 1200 Hz
# (the two cases on DM-RS symbols 2 and 11 only have two points for their polygon; case 1 carries 256-QAM on them). The CFO chain fails ALL five
# only from 1000 Hz on, where the phase between the two rays turns 4 rad between symbols 2 and 11 and no polygon through two or three points follows.
FD_HZ = 100.0
CFO_CHAIN_FAILS = (0, 1, 3)


# ------------------------------------------------------------------------------------------------ (a) weights
@pytest.mark.parametrize("mu,slot", ((0, 0), (1, 3), (2, 1)))
@pytest.mark.parametrize("dsyms", ([3], [2, 11], [2, 7, 11], [2, 5, 8, 11], [0, 5, 13]), ids=lambda d: "dmrs" + "_".join(map(str, d)))
def test_weights(mu, slot, dsyms):
    """(a) Rows sum to 1; INTERPOLATE is the identity at the DM-RS symbols and has at most two weights per row; the modes agree at two DM-RS symbols;
    LINE (and INTERPOLATE between and beyond two DM-RS symbols) reproduces a linear function of tau exactly."""
    tau = F.symbol_times(mu, slot)
    wi, wl = T.weights(mu, slot, dsyms, T.INTERPOLATE), T.weights(mu, slot, dsyms, T.LINE)
    assert wi.shape == wl.shape == (14, len(dsyms))
    assert np.allclose(wi.sum(1), 1.0, atol=1e-13) and np.allclose(wl.sum(1), 1.0, atol=1e-13)
    assert np.array_equal(wi[dsyms], np.eye(len(dsyms)))
    assert np.all((wi != 0).sum(1) <= 2)
    if len(dsyms) <= 2:
        assert np.allclose(wi, wl, atol=1e-13)
    lin = 0.7 - 900.0 * tau  # any linear function of the symbol time
    assert np.allclose(wl @ lin[dsyms], lin if len(dsyms) > 1 else lin[dsyms[0]], atol=1e-12)
    assert np.allclose(wi @ lin[dsyms], lin if len(dsyms) > 1 else lin[dsyms[0]], atol=1e-12)
    if len(dsyms) > 2:  # a polygon follows a kink at a DM-RS symbol, a line does not
        kink = np.abs(tau - tau[dsyms[1]])
        assert np.allclose((wi @ kink[dsyms])[dsyms[0]:dsyms[-1] + 1], kink[dsyms[0]:dsyms[-1] + 1], atol=1e-12)
        assert not np.allclose(wl @ kink[dsyms], kink, atol=1e-6)


# ------------------------------------------------------------------------------------------------ (b) noise free
@pytest.mark.parametrize("mode", T.MODES, ids=("interpolate", "line"))
@pytest.mark.parametrize("dsyms", DMRS_SETS, ids=lambda d: "dmrs" + "_".join(map(str, d)))
@pytest.mark.parametrize("nl,npt", PL.TOPOLOGIES)
def test_noise_free_linear_channel(nl, npt, dsyms, mode):
    """(b) One tap at delay 0, no noise, float64: real gains that change linearly in time with a slope of their own per port, times an offset. The
    offset within 1e-6 Hz; H_l = h gain_p[l] exp(j phi_l) within 1e-5 of max |h| on every symbol, the extrapolated ones included (the bound of the CFO
    test); var > 0. With constant gains var < 1e-12."""
    rng = np.random.default_rng(100 * nl + npt + len(dsyms))
    case, h = E.make_case(rng, 24, slice(3, 15), npt, nl, dsyms, delay=0.0, taps=1, background=0.0)
    mu, slot, rb = case[0], case[1], case[7]
    g = np.zeros((npt, 14, 24 * 12), np.complex128)
    E.add_dmrs(g, h, rb, dsyms, nl, slot, case[3], case[4], float(E.BETA))
    mask = np.repeat(rb.astype(bool), 12)
    tau = F.symbol_times(mu, slot)
    gains = T.linear_gains(mu, slot, [600.0, -900.0, 1200.0, -300.0][:npt])  # +-0.25 ms around the middle: the gains stay within 0.7 .. 1.3
    assert gains.min() > 0.5
    args = case[:5] + (float(E.BETA),) + case[6:-1]
    for f in F.OFFSETS_HZ:
        ce, sc, fh, rho, var = T.estimate(mode, *args, F.apply_cfo(T.apply_gains(g, gains), mu, slot, f, phase0=0.3))
        assert abs(fh - f) <= 1e-6, (f, fh)
        want = h[:, :, None, :] * (gains * np.exp(1j * (0.3 + 2 * np.pi * f * tau))[None, :])[None, :, :, None]
        assert np.abs(ce[..., mask] - want[..., mask]).max() < 1e-5 * np.abs(h).max(), f
        assert np.isnan(ce[..., ~mask]).all()
        assert np.all(var > 0), var
        var0 = T.estimate(mode, *args, F.apply_cfo(g, mu, slot, f, phase0=0.3))[4]
        assert np.all(var0 < 1e-12), var0


# ------------------------------------------------------------------------------------------------ (c) one DM-RS symbol
@pytest.mark.parametrize("mode", T.MODES, ids=("interpolate", "line"))
@pytest.mark.parametrize("nl,npt", ((1, 2), (2, 2), (3, 4)))
def test_one_dmrs_symbol(nl, npt, mode):
    """(c) Nothing to interpolate: estimate, scalars (noise_var = 0.001 epre) and offset are those of the CFO restatement; var = 0."""
    case, _ = E.make_case(np.random.default_rng(9), 24, slice(3, 15), npt, nl, [3], delay=2.0)
    g = T.apply_gains(case[-1], T.two_ray_gains(400.0, case[0], case[1], npt))
    ce, sc, f, rho, var = T.estimate(mode, *case[:-1], g)
    ece, esc, ef, erho = F.estimate(*case[:-1], g)
    assert f == ef == 0.0 and rho == erho == 0.0 and np.all(var == 0.0)
    assert np.allclose(ce, ece, rtol=1e-13, atol=0, equal_nan=True) and np.allclose(sc, esc, rtol=1e-12, atol=0)


def test_two_dmrs_symbols_give_one_estimate_in_both_modes():
    """Two DM-RS symbols: a line and a polygon are the same thing, the noise divisor too (R = 2)."""
    case, _ = E.make_case(np.random.default_rng(10), 24, slice(3, 15), 3, 3, [2, 11], delay=2.0)
    g = T.apply_gains(case[-1], T.two_ray_gains(300.0, case[0], case[1], 3))
    a, b = T.estimate(T.INTERPOLATE, *case[:-1], g), T.estimate(T.LINE, *case[:-1], g)
    assert np.allclose(a[0], b[0], rtol=1e-12, atol=1e-15, equal_nan=True) and np.allclose(a[1], b[1], rtol=1e-12) and np.allclose(a[4], b[4], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ (d) the chain
_chain = {}


def decode(case, c, tb, llr):
    nl, npt, mod, tb_bytes = case[:4]
    ok, out, _ = O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes).decode(llr, 0, True, 6, True)
    return bool(ok) and np.array_equal(out, tb)


def chain_run(k, fd):
    """Chain case k under two_ray_gains(fd), once: dict(cfo, interpolate, line: decoded or not; var; c, tb, grid, est)."""
    if (k, fd) not in _chain:
        c, tb, grid, est = T.chain_tx(CHAIN[k], fd)
        li, _, _, var = T.host_llr(T.INTERPOLATE, c, grid, est)
        _chain[(k, fd)] = dict(cfo=decode(CHAIN[k], c, tb, F.host_llr(c, grid, est)[0]), interpolate=decode(CHAIN[k], c, tb, li),
                               line=decode(CHAIN[k], c, tb, T.host_llr(T.LINE, c, grid, est)[0]), var=var, c=c, tb=tb, grid=grid, est=est)
    return _chain[(k, fd)]


@pytest.mark.parametrize("k", range(len(CHAIN)))
def test_chain_cases_decode_with_constant_gains(k):
    """(d) fd = 0 at the listed SNR: per-symbol fits cost estimation noise, but no case needs a higher SNR for it."""
    r = chain_run(k, 0.0)
    assert r["interpolate"] and r["cfo"]


@pytest.mark.parametrize("k", range(len(CHAIN)))
def test_chain_cases_decode_under_two_ray_gains(k):
    """(d) At FD_HZ = 100 Hz every case decodes in INTERPOLATE mode (6 iterations) at its listed SNR (20, 30, 16, 24, 20 dB: none was raised, all five
    decode with constant gains); LINE is reported (it decodes all five too). Measured: the CFO chain fails cases 0, 1 and 3 at 100 Hz; INTERPOLATE keeps
    decoding up to 700, 400, 1000, 600 and 1200 Hz per case (table at the top of this file)."""
    r = chain_run(k, FD_HZ)
    print("case %d at fd %g Hz: CFO chain %d, INTERPOLATE %d, LINE %d, largest var %.3f" % (k, FD_HZ, r["cfo"], r["interpolate"], r["line"], r["var"].max()))
    assert r["interpolate"]


def test_the_cfo_chain_fails_at_fd_and_not_below():
    """(d) Why the entry point exists: the CFO chain -- one averaged estimate, rotated per symbol -- on the same grids does not decode cases 0, 1 and 3
    at FD_HZ, the smallest value of the 100 Hz raster (below it, constant gains: everything decodes)."""
    assert FD_HZ == 100.0  # (the raster's first value: the step below is fd = 0)
    assert tuple(k for k in range(len(CHAIN)) if not chain_run(k, FD_HZ)["cfo"]) == CFO_CHAIN_FAILS
    assert all(chain_run(k, 0.0)["cfo"] for k in range(len(CHAIN)))
    assert all(len(case[5]) >= 2 for case in CHAIN)


# ------------------------------------------------------------------------------------------------ (e) exports
def test_exports_record_and_header():
    """(e) Both entry points are in the library; PuschChestTvJob is miphy_pusch_chest_cfo_job, var_offset, time_mode, seven reserved bytes: 176."""
    import miphy
    lib = ctypes.CDLL(miphy.lib_path)
    for name in ("miphy_dmrs_pusch_estimate_tv_batch", "miphy_pusch_process_layers_tv_batch"):
        assert hasattr(lib, name), name
    d = miphy.PuschChestTvJob
    assert d.itemsize == 176 and d.fields["base"][0] == miphy.PuschChestCfoJob and d.fields["base"][1] == 0
    assert d.fields["var_offset"][1] == 160 and d.fields["time_mode"][1] == 168 and d.fields["reserved"][1] == 169
    assert (miphy.TIME_INTERPOLATE, miphy.TIME_LINE) == (T.INTERPOLATE, T.LINE) == (1, 2)
    assert hasattr(miphy.Context, "dmrs_pusch_estimate_tv_batch") and hasattr(miphy.Context, "pusch_process_layers_tv_batch")
    hdr = open(os.path.join(ROOT, "include", "miphy.h")).read()
    assert re.search(r"#define\s+MIPHY_TIME_INTERPOLATE\s+1\b", hdr) and re.search(r"#define\s+MIPHY_TIME_LINE\s+2\b", hdr)
    assert re.search(r"miphy_pusch_chest_cfo_job\s+base;.*\n\s*uint64_t\s+var_offset;.*\n\s*uint8_t\s+time_mode;.*\n\s*uint8_t\s+reserved\[7\];.*\n\}\s*miphy_pusch_chest_tv_job;",
                     hdr)
    for text in ("w[l][j] = 1 - u", "noise_var = sum |e|^2 / nprb / (6 nds - nlay R)", "var = sum_m sum_d |S_d[m] - mean_d S[m]|^2 / sum_m sum_d |S_d[m]|^2"):
        assert text in hdr, text
    cfo_out = hdr[hdr.index("typedef struct {\n  miphy_pusch_chest_job base;   /* ce_compact must be 0; nof_tx_layers 1..4") - 400:]
    assert "Out: time interpolation of the channel magnitude" not in hdr and "miphy_dmrs_pusch_estimate_tv_batch below" in cfo_out[:400]
