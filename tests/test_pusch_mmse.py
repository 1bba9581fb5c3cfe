"""CPU: the MMSE-IRC contract of tests/pusch_mmse_cases.py -- the float32 restatement of csrc/mmse_device.h against numpy.linalg in float64, the
formula against zero forcing where the two must agree, the covariance against the estimator's own noise variance, the transmissions that zero
forcing loses to an interferer and MMSE-IRC decodes, and what can be seen of the library's new entry points without a GPU."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import pusch_mmse_cases as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "srsran_project_23.5_amd", "libmiphy.so")

# Largest |x_single - x_double| / (2^-24 cond(A) cond(C) |x|) (norms over the layers of an element) that mmse_single showed over seeds 0..4 at
# 2 000 elements per topology, and for the noise variances |nv_single - nv_double| / (2^-24 cond(A) cond(C) nv): see test_mmse_single_against_double.
MMSE_BOUND = 13.5


def _mmse_ratios(nl, npt, seed, n=2000):
    """20 covariance matrices of 100 elements each: sigma^2 (I + sum rho_k a_k a_k^H), one interferer on the even matrices, two on the odd ones,
    rho uniform in (0, 100]; the last two matrices at rho = 100."""
    rng = np.random.default_rng(1000 * seed + 10 * nl + npt)
    h, _ = PL.channels(rng, nl, npt, n)
    xs = (rng.standard_normal((nl, n)) + 1j * rng.standard_normal((nl, n))).astype(np.complex64)
    tx, sigma2, per = 0.8, 0.05, 100
    cov = []
    for k in range(n // per):
        rhos = rng.uniform(0, 100, 1 + k % 2)
        if k >= n // per - 2:
            rhos[:] = 100.0
        cov.append(MM.coloured(rng, npt, sigma2, rhos))
    cov = np.stack(cov).astype(np.complex64)
    idx = np.arange(n) // per
    lc = np.linalg.cholesky(cov.astype(np.complex128))
    noise = np.einsum("npq,qn->pn", lc[idx], (rng.standard_normal((npt, n)) + 1j * rng.standard_normal((npt, n))) / np.sqrt(2))
    y = (tx * np.einsum("lpn,ln->pn", h.astype(np.complex128), xs.astype(np.complex128)) + noise).astype(np.complex64)
    xd, vd = MM.mmse_double(y, h, cov, tx, per)
    x1, v1 = MM.mmse_single(y, h, cov, tx, per)
    assert np.all(np.isfinite(v1))
    c128 = cov.astype(np.complex128)
    cond_c = np.linalg.cond(c128)[idx]
    hh = h.astype(np.complex128).transpose(2, 1, 0)
    a = tx * tx * (hh.conj().transpose(0, 2, 1) @ np.linalg.inv(c128)[idx] @ hh) + np.eye(nl)
    cond = np.linalg.cond(a) * cond_c
    eps = 2.0 ** -24
    ex = np.linalg.norm(x1 - xd, axis=0) / (eps * cond * np.linalg.norm(xd, axis=0))
    ev = np.abs(v1 - vd).max(axis=0) / (eps * cond * np.abs(vd).max(axis=0))
    return float(ex.max()), float(ev.max())


@pytest.mark.parametrize("nl,npt", PL.TOPOLOGIES)
def test_mmse_single_against_double(nl, npt):
    """The float32 restatement against numpy.linalg in float64, all topologies, coloured noise with one and two interferers up to 20 dB above
    the white part: error <= MMSE_BOUND * 2^-24 * cond(A) * cond(C) * |x|, likewise for the noise variances. Measured with this
    very function (never with the kernel): the largest ratio over seeds 0..4 and all topologies was 6.73 for the symbols (1 x 2; 4 x 4: 0.22) and
    5.51 for the noise variances (1 x 1); MMSE_BOUND is the larger one doubled, because the seeds are few. gamma is taken as (B T)_ll, not as
    1 - B_ll: no topology needs a larger bound where an interferer pushes the SINR down."""
    worst = [_mmse_ratios(nl, npt, seed) for seed in range(5)]
    ex, ev = max(w[0] for w in worst), max(w[1] for w in worst)
    print("mmse_single vs mmse_double %dx%d: symbols %.2f, noise variances %.2f (units of 2^-24 cond(A) cond(C) |x|)" % (nl, npt, ex, ev))
    assert ex <= MMSE_BOUND and ev <= MMSE_BOUND


@pytest.mark.parametrize("npt", [1, 2, 3, 4])
def test_one_layer_in_white_noise_is_maximum_ratio_combining(npt):
    """L = 1, C = sigma^2 I: the unbiased MMSE symbol and its variance are those of zero forcing (MRC), whatever sigma^2."""
    rng = np.random.default_rng(40 + npt)
    h, _ = PL.channels(rng, 1, npt, 500)
    y = (rng.standard_normal((npt, 500)) + 1j * rng.standard_normal((npt, 500)))
    for sigma2, tx in ((0.3, 1.0), (2.5, 0.7)):
        x, v = MM.mmse_double(y, h, sigma2 * np.eye(npt), tx)
        xz, vz = PL.zf_double(y, h, sigma2, tx)
        assert np.abs(x - xz).max() <= 1e-12 * np.abs(xz).max() and np.abs(v - vz).max() <= 1e-12 * np.abs(vz).max()


@pytest.mark.parametrize("nl,npt", PL.TOPOLOGIES)
def test_white_noise_limit_is_zero_forcing(nl, npt):
    """C = sigma^2 I, sigma^2 -> 1e-9: symbols and variances approach the pseudo-inverse's to 1e-6."""
    rng = np.random.default_rng(50 + 10 * nl + npt)
    h, _ = PL.channels(rng, nl, npt, 500)
    y = (rng.standard_normal((npt, 500)) + 1j * rng.standard_normal((npt, 500)))
    x, v = MM.mmse_double(y, h, 1e-9 * np.eye(npt), 0.9)
    xz, vz = PL.zf_double(y, h, 1e-9, 0.9)
    assert np.abs(x - xz).max() <= 1e-6 * np.abs(xz).max() and np.abs(v - vz).max() <= 1e-6 * np.abs(vz).max()


# ------------------------------------------------------------------------------------------------ covariance()
@pytest.mark.parametrize("nl,npt", [(1, 2), (2, 4)])
def test_covariance_diagonal_is_the_estimators_noise_variance(nl, npt):
    rng = np.random.default_rng(60 + nl)
    case, _ = E.make_case(rng, 24, slice(3, 14), npt, nl, [2, 7, 11])
    _, sc = E.estimate(*case)
    cov = MM.covariance(case)
    assert cov.shape == (1, npt, npt)
    for p in range(npt):
        assert abs(cov[0, p, p].real - sc[p, 0, 2]) <= 1e-12 * sc[p, 0, 2] and cov[0, p, p].imag == 0
    assert np.array_equal(cov[0], cov[0].conj().T)


def test_covariance_loading_grows_the_diagonal_only():
    rng = np.random.default_rng(63)
    case, _ = E.make_case(rng, 24, slice(3, 14), 3, 2, [2, 11])
    c0, c1 = MM.covariance(case, 4), MM.covariance(case, 4, 0.1)
    assert c0.shape == (3, 3, 3)
    for j in range(3):
        add = 0.1 * np.real(np.trace(c0[j])) / 3
        assert np.allclose(c1[j] - c0[j], add * np.eye(3), rtol=0, atol=1e-15 * add)
        off = ~np.eye(3, dtype=bool)
        assert np.array_equal(c1[j][off], c0[j][off])


def _only_prbs(case, keep):
    """The case with its allocation cut down to the PRBs `keep`."""
    rb = np.zeros_like(case[7])
    rb[keep] = 1
    return case[:7] + (rb,) + case[8:]


def test_covariance_prg_edges():
    """5 allocated PRBs at prg_size 2: three matrices, the last from one PRB -- each the whole-allocation matrix of its PRBs alone (the residuals
    of a PRB depend on that PRB only)."""
    rng = np.random.default_rng(64)
    case, _ = E.make_case(rng, 24, slice(6, 11), 2, 2, [2, 7, 11])
    cov = MM.covariance(case, 2)
    assert cov.shape == (3, 2, 2)
    for j, keep in enumerate(([6, 7], [8, 9], [10])):
        assert np.allclose(cov[j], MM.covariance(_only_prbs(case, keep))[0], rtol=1e-12, atol=0)


def test_covariance_counts_prgs_over_the_allocated_rank():
    """PRBs 3, 4 and 9 at prg_size 2: PRG 0 = {3, 4}, PRG 1 = {9} -- not {3}, {4}, {9 / 2}."""
    rng = np.random.default_rng(65)
    case, _ = E.make_case(rng, 24, [3, 4, 9], 2, 1, [2, 11])
    cov = MM.covariance(case, 2)
    assert cov.shape == (2, 2, 2)
    assert np.allclose(cov[0], MM.covariance(_only_prbs(case, [3, 4]))[0], rtol=1e-12, atol=0)
    assert np.allclose(cov[1], MM.covariance(_only_prbs(case, [9]))[0], rtol=1e-12, atol=0)
    c = PL.case("x", 1, 2, 2, prbs=(3, 4, 9), start=0, nof=14, dmrs=(2, 11))
    idx = MM.re_prg_index(c, 2)
    _, sc = PL.data_positions(c)
    assert np.array_equal(idx, np.where(sc // 12 == 9, 1, 0))


# ------------------------------------------------------------------------------------------------ the library without a GPU
NEW_SYMBOLS = ("miphy_pusch_noise_covariance_batch", "miphy_pusch_noise_covariance_nof_prg", "miphy_channel_equalize_mmse_batch",
               "miphy_pusch_demodulate_layers_mmse_batch", "miphy_pusch_demodulate_layers_mmse_batch_ex", "miphy_pusch_process_layers_mmse_batch")


def test_new_symbols_are_exported_and_bound():
    import miphy
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = set(re.findall(r" T (miphy_[a-z0-9_]+)", out))
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    for name in ("PuschNcovJob", "EqualizerMmseJob", "PuschDemodMmseJob", "PuschMmsePdu", "pusch_noise_covariance_nof_prg"):
        assert hasattr(miphy, name) and name in miphy.__all__
    for name in ("pusch_noise_covariance_batch", "channel_equalize_mmse_batch", "pusch_demodulate_layers_mmse_batch", "pusch_demodulate_layers_mmse_batch_ex",
                 "pusch_process_layers_mmse_batch"):
        assert callable(getattr(miphy.Context, name))


def test_record_sizes_match_the_header():
    import miphy
    src = '#include "miphy.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(miphy_pusch_ncov_job), sizeof(miphy_equalizer_mmse_job), sizeof(miphy_pusch_demod_mmse_job), sizeof(miphy_pusch_mmse_pdu)); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert sizes == [miphy.PuschNcovJob.itemsize, miphy.EqualizerMmseJob.itemsize, miphy.PuschDemodMmseJob.itemsize, miphy.PuschMmsePdu.itemsize] == [168, 64, 144, 128]


def test_nof_prg_on_valid_and_invalid_jobs():
    import miphy
    rng = np.random.default_rng(66)
    five = E.make_case(rng, 24, slice(6, 11), 2, 2, [2, 11])[0]
    split = E.make_case(rng, 24, [3, 4, 9], 2, 1, [2, 11])[0]
    for case, prg, want in ((five, 0, 1), (five, 1, 5), (five, 2, 3), (five, 4, 2), (five, 5, 1), (five, 64, 1), (split, 2, 2)):
        assert miphy.pusch_noise_covariance_nof_prg(MM.ncov_job(miphy, case, prg)) == want == MM.covariance(case, prg).shape[0]
    for field, value in (("loading", -1.0), ("loading", float("nan")), ("loading", float("inf")), ("hop_symbol", 7), ("nof_rx_ports", 5), ("nof_tx_layers", 0),
                         ("symbols_mask", 0), ("scaling", 0.0), ("rb_mask", 0)):
        a = np.array([MM.ncov_job(miphy, five, 2)], dtype=miphy.PuschNcovJob)
        (a if field == "loading" else a["base"])[field] = value
        assert miphy.pusch_noise_covariance_nof_prg(a[0]) == 0, field


# ------------------------------------------------------------------------------------------------ the reason the feature exists
def _decodes(c, tb, llr, tb_bytes):
    ok, out, _ = O.OraclePuschDecoder(1, c["mod"], 0, c["nl"], PL.nof_re(c) * c["nl"], tb_bytes).decode(llr, 0, True, 6, True)
    return bool(ok) and np.array_equal(out, tb)


@pytest.mark.parametrize("case", MM.IRC_CASES)
@pytest.mark.parametrize("prg", [0, 4])
def test_irc_decodes_what_zero_forcing_loses(case, prg):
    """A neighbour cell's user on the same PRBs at INR +5 dB: the zero-forcing host chain (E.host_llr) loses the transport block, the IRC host
    chain (covariance -> mmse_single -> compose_llr, float32 where the device is) returns it, oracle decoder at 6 iterations. Sweep of the INR
    with these very functions (seed 3; 1 = the transport block came back; IRC alike at prg_size 0, 4 and 1):
                                          INR dB:  none  -10   -5    0   +5  +10  +15
      2 layers, 4 ports, DM-RS (2, 7, 11)   ZF       1    1    0    0    0    0    0      IRC   1 at every step
      2 layers, 4 ports, DM-RS (2, 11)      ZF       1    0    0    0    0    0    0      IRC   1 at every step
      1 layer,  2 ports, DM-RS (2, 7, 11)   ZF       1    1    0    0    0    0    0      IRC   1 at every step
    so at +5 dB every case has zero forcing failing 5 dB below and IRC decoding 5 dB above. (With two DM-RS symbols zero forcing fails from
    -10 dB on: the estimator's forced noise variance, 0.001 EPRE, makes its soft bits over-confident.)"""
    nl, npt, mod, tb_bytes, snr_db, dmrs = case
    c, tb, grid, est = MM.interfered_tx(nl, npt, mod, tb_bytes, snr_db, dmrs, MM.INR_DB)
    assert not _decodes(c, tb, E.host_llr(c, grid, est), tb_bytes)
    assert _decodes(c, tb, MM.irc_llr(c, grid, est, prg), tb_bytes)
