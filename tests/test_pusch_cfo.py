"""CPU: the float64 restatement of the estimator that estimates and compensates a carrier frequency offset (tests/pusch_cfo_cases.py) against what
it can be held to without a device: (a) noise free it returns the applied offset and the per-symbol channel; (b) the transmissions of the GPU
processor test decode through it at 0, 150, 400 and -1000 Hz, with the offset found, while the chain without it fails at -1000 Hz; (c) its symbol
times are those of the OFDM oracle; (d) with one DM-RS symbol it is the layered restatement; (e) exports and record size."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pusch_cfo_cases as F
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = E.CHAIN_CASES + [E.ONE_LAYER_CASE]


@pytest.mark.parametrize("dsyms", ([2, 11], [2, 7, 11], [2, 5, 8, 11]), ids=lambda d: "dmrs" + "_".join(map(str, d)))
@pytest.mark.parametrize("nl,npt", PL.TOPOLOGIES)
def test_noise_free_offset_and_channel(nl, npt, dsyms):
    """(a) One tap at delay 0, no noise, grid and rotation in float64: the offset within 1e-6 Hz, the per-symbol channel h exp(j phi_l) within 1e-5 of
    max |h| (the bound of the flat-channel test of the layered restatement), rho = 1."""
    rng = np.random.default_rng(100 * nl + npt + len(dsyms))
    case, h = E.make_case(rng, 24, slice(3, 15), npt, nl, dsyms, delay=0.0, taps=1, background=0.0)
    mu, slot, rb = case[0], case[1], case[7]
    g = np.zeros((npt, 14, 24 * 12), np.complex128)
    E.add_dmrs(g, h, rb, dsyms, nl, slot, case[3], case[4], float(E.BETA))  # (the case's own grid is rounded to float32)
    mask = np.repeat(rb.astype(bool), 12)
    tau = F.symbol_times(mu, slot)
    for f in F.OFFSETS_HZ:
        ce, sc, fh, rho = F.estimate(*case[:5], float(E.BETA), *case[6:-1], F.apply_cfo(g, mu, slot, f, phase0=0.3))
        assert abs(fh - f) <= 1e-6, (f, fh)
        assert abs(rho - 1) < 1e-9, rho
        # the phase of the first DM-RS symbol belongs to the channel: the estimator cannot tell it from h
        want = h[:, :, None, :] * np.exp(1j * (0.3 + 2 * np.pi * f * tau))[None, None, :, None]
        assert np.abs(ce[..., mask] - want[..., mask]).max() < 1e-5 * np.abs(h).max(), f
        assert np.isnan(ce[..., ~mask]).all()


_chain = {}


def _chain_run(k, f):
    """The chain case k at offset f through the restatement and the oracle decoder, once: (decoded, cfo_hz, rho, c, tb, grid, est)."""
    if (k, f) not in _chain:
        nl, npt, mod, tb_bytes = CHAIN[k][:4]
        c, tb, grid, est = F.chain_tx(CHAIN[k], f)
        llr, fh, rho = F.host_llr(c, grid, est)
        ok, out, _ = O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes).decode(llr, 0, True, 6, True)
        _chain[(k, f)] = (bool(ok) and np.array_equal(out, tb), fh, rho, c, tb, grid, est)
    return _chain[(k, f)]


@pytest.mark.parametrize("f", F.OFFSETS_HZ)
@pytest.mark.parametrize("k", range(len(CHAIN)))
def test_chain_cases_decode_with_an_offset(k, f):
    """(b) All twenty decode through the restatement (6 iterations); |cfo_hz - f| <= 10 Hz (measured <= 3.6 Hz), rho >= 0.9 (measured >= 0.958)."""
    ok, fh, rho = _chain_run(k, f)[:3]
    print("case %d at %g Hz: cfo_hz %.3f, rho %.4f, decoded %s" % (k, f, fh, rho, ok))
    assert ok
    assert abs(fh - f) <= 10.0, (fh, f)
    assert rho >= 0.9, rho


@pytest.mark.parametrize("k", range(len(CHAIN)))
def test_the_chain_without_compensation_fails_at_minus_1000_hz(k):
    """(b) Why the entry point exists: host_llr() of the existing chain -- one averaged estimate for every symbol -- on the same grid does not decode."""
    nl, npt, mod, tb_bytes = CHAIN[k][:4]
    c, tb, grid, est = _chain_run(k, -1000.0)[3:]
    ok, out, _ = O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes).decode(E.host_llr(c, grid, est), 0, True, 6, True)
    assert not (ok and np.array_equal(out, tb))


# Residual of the common phase against 2 pi f (tau_l - tau_0), measured on the CPU with the cases below: at most 6.8e-9 rad (numerology 1). The
# inter-carrier interference of a 400 Hz offset has relative amplitude about f / scs = 0.027 (15 kHz) from each neighbour; over the 288 subcarriers of
# independent QPSK it turns the sum by the order of 0.027 / sqrt(288) = 1.6e-3 rad -- but the grid carries the same row on every symbol, so the term is
# the same on every symbol and leaves the differences; what remains is the rounding of the float32 samples. Bound: 1e-6 rad, 150 times the measured
# value. A symbol-time rule off by ONE sample of the 16 * 2^mu that distinguish a long prefix would show as 2 pi 400 / 61.44e6 = 4.1e-5 rad at
# numerology 2 (more below), forty times the bound.
SYMBOL_PHASE_BOUND = 1e-6


@pytest.mark.parametrize("mu,slot", ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)))
def test_symbol_times_against_the_ofdm_oracle(mu, slot):
    """(c) A slot modulated by the oracle, multiplied by exp(j 2 pi f t), f = 400 Hz, demodulated by the oracle: the common phase of symbol l relative
    to symbol 0 is 2 pi f (tau_l - tau_0). Slot 0 (symbol 0 long) at numerology 0, 1, 2; numerology 2, slot 1: no long symbol; slot 2: symbol 0 long
    again. (At numerology 0 and 1 symbol 0 of every slot is long: 14 slot is a multiple of 7 * 2^mu.)"""
    f, nprb, n = 400.0, 24, 1024
    cfg = O.OfdmCfg(mu, nprb, n, 0, 1.0, 3.5e9)
    rng = np.random.default_rng(5)
    row = ((1 - 2 * rng.integers(0, 2, nprb * 12)) + 1j * (1 - 2 * rng.integers(0, 2, nprb * 12))) / np.sqrt(2)
    grid = np.tile(row, (14, 1)).astype(np.complex64)
    x = O.o_ofdm_mod_slot(cfg, slot, grid).astype(np.complex128)
    t = np.arange(x.size) / (n * 15000.0 * (1 << mu))
    y = O.o_ofdm_demod_slot(cfg, slot, (x * np.exp(2j * np.pi * f * t)).astype(np.complex64))
    common = (y.astype(np.complex128) * grid.conj()).sum(1)
    tau = F.symbol_times(mu, slot)
    resid = np.angle(common * common[0].conj() * np.exp(-2j * np.pi * f * (tau - tau[0])))
    print("numerology %d slot %d: residual %.3g rad" % (mu, slot, np.abs(resid).max()))
    assert np.abs(resid).max() < SYMBOL_PHASE_BOUND
    long0 = (14 * slot) % (7 << mu) == 0
    assert long0 == (mu < 2 or slot % 2 == 0)
    assert np.isclose(tau[0] * n * 15000.0 * (1 << mu), (144 + (16 << mu if long0 else 0)) * n / 2048)


@pytest.mark.parametrize("nl,npt", ((1, 2), (2, 2), (3, 4)))
def test_one_dmrs_symbol(nl, npt):
    """(d) Nothing to correlate: cfo_hz = 0, rho = 0, the estimate is estimate() of the layered restatement on every symbol."""
    case, _ = E.make_case(np.random.default_rng(9), 24, slice(3, 15), npt, nl, [3], delay=2.0)
    g = F.apply_cfo(case[-1], case[0], case[1], 400.0)
    ce, sc, f, rho = F.estimate(*case[:-1], g)
    ece, esc = E.estimate(*case[:-1], g)
    assert f == 0.0 and rho == 0.0
    assert np.array_equal(ce, ece, equal_nan=True) and np.array_equal(sc, esc)


def test_exports_and_record_size():
    """(e) Both entry points are in the library; PuschChestCfoJob is miphy_pusch_chest_job plus the offset of {cfo_hz, rho}."""
    import miphy
    lib = ctypes.CDLL(miphy.lib_path)
    for name in ("miphy_dmrs_pusch_estimate_cfo_batch", "miphy_pusch_process_layers_cfo_batch"):
        assert hasattr(lib, name), name
    assert miphy.PuschChestCfoJob.itemsize == miphy.PuschChestJob.itemsize + 8 == 160
    assert miphy.PuschChestCfoJob.fields["base"][0] == miphy.PuschChestJob and miphy.PuschChestCfoJob.fields["cfo_offset"][1] == miphy.PuschChestJob.itemsize
    hdr = open(os.path.join(ROOT, "include", "miphy.h")).read()
    assert re.search(r"miphy_pusch_chest_job\s+base;.*\n\s*uint64_t\s+cfo_offset;.*\n\}\s*miphy_pusch_chest_cfo_job;", hdr)
    assert hasattr(miphy.Context, "dmrs_pusch_estimate_cfo_batch") and hasattr(miphy.Context, "pusch_process_layers_cfo_batch")
