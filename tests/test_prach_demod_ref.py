"""CPU: the float64 restatement of the OFDM PRACH demodulator (tests/prach_demod_ref.py) against the reference's output recorded in
tests/golden/prach_demod.npz, and the library's host-only miphy_prach_demod_info against the restatement's geometry."""
import re

import numpy as np
import pytest

import miphy
import prach_demod_ref as D

TOL = 4e-6  # the project's DFT tolerance (tests/test_ofdm_gpu.py), same metric


def test_fixture_covers_what_it_claims():
    cfg = np.stack([c["cfg"] for c in D.fixture()])
    assert set(cfg[:, D.C_FMT]) == set(range(14))
    assert set(cfg[:, D.C_SRATE]) == {7680000, 15360000, 23040000, 30720000, 61440000}
    assert set(cfg[:, D.C_SCS]) == {0, 1, 2} and set(cfg[:, D.C_NFD]) == {1, 2, 3, 4}
    assert (cfg[:, D.C_NTD] >= 3).sum() >= 5
    assert ((cfg[:, D.C_FMT] >= 11) & (cfg[:, D.C_NTD] >= 2)).sum() >= 4  # A/B pairs whose last occasion differs
    where = set()
    for c in D.fixture():
        g = c["geometry"]
        for k in g["k_start"]:
            where.add("low" if k + g["L"] <= g["grid"] // 2 else ("upper" if k >= g["grid"] // 2 else "across"))
    assert where == {"low", "upper", "across"}


def test_regenerated_windows_match_the_recorded_hashes():
    for i, c in enumerate(D.fixture()):
        assert D.window_hash(c["window"]) == c["sha256"], i


def test_restatement_matches_the_reference_on_every_case():
    worst = 0.0
    for i, c in enumerate(D.fixture()):
        e = D.rel_err(D.demodulate(c["window"], c["cfg"]), c["expected"])
        worst = max(worst, e)
        assert e < TOL, (i, list(c["cfg"]), e)
    print("largest distance restatement - reference: %.2e" % worst)


def info(cfg, **kw):
    job = np.zeros(1, miphy.PrachDemodJob)
    job[0] = D.job_of(cfg, **kw)
    return miphy.prach_demod_info(int(cfg[D.C_SRATE]), job[0])


def assert_same_geometry(cfg, g):
    o = info(cfg, g=g)
    for k in ("L", "ra_scs_hz", "dft_size", "nof_symbols", "K", "k_bar", "nof_rb_ra", "window_samples"):
        assert int(o[k]) == g[k], (list(cfg), k, int(o[k]), g[k])
    ntd, nfd = int(cfg[D.C_NTD]), int(cfg[D.C_NFD])
    assert list(o["td_sample_offset"][:ntd]) == g["td_sample_offset"], list(cfg)
    assert list(o["td_cp_samples"][:ntd]) == g["td_cp_samples"], list(cfg)
    assert list(o["k_start"][:nfd]) == g["k_start"], list(cfg)


def test_info_equals_the_restated_geometry_on_the_fixture():
    for c in D.fixture():
        assert_same_geometry(c["cfg"], c["geometry"])


def error_of(cfg, **kw):
    """(code, message) of miphy_prach_demod_info on a configuration row; (0, "") where it accepts."""
    job = np.zeros(1, miphy.PrachDemodJob)
    job[0] = D.job_of(cfg, **kw)
    try:
        miphy.prach_demod_info(int(cfg[D.C_SRATE]), job[0])
    except RuntimeError as e:
        m = re.match(r"miphy error (-?\d+): (.*)", str(e), re.S)
        return int(m.group(1)), m.group(2)
    return 0, ""


def error_code(cfg, **kw):
    return error_of(cfg, **kw)[0]


def test_info_equals_the_restated_geometry_on_a_sweep():
    """Every (format, PUSCH spacing, sampling rate, start symbol 0..13): where the restatement accepts, the same numbers; where it
    rejects, MIPHY_EINVAL. Short formats with as many time-domain occasions as the slot holds. 2.25 and 5.76 MHz are there for the
    times that are not whole numbers of samples (16 kappa is 1.17 and 3 samples); 11.52, 17.28 and 92.16 MHz are rates of the GPU tests
    (tests/test_prach_demod_gpu.py) outside prach_demod_ref.SRATES."""
    accepted = 0
    for fmt in range(14):
        for mu in range(4):
            for srate in D.SRATES + (122880000, 2250000, 5760000, 11520000, 17280000, 92160000):
                for start in range(14):
                    duration = 0 if fmt < 4 else D.SHORT[fmt - 4][3]
                    ntd = 1 if fmt < 4 else min(D.MAX_TD, max(1, (14 - start) // duration))
                    nprb = (106, 51, 24, 12)[mu] if srate >= 7680000 else 12
                    cfg = np.array([srate, fmt, mu, ntd, 1, start, 0, nprb, 1 << 30], np.int64)
                    try:
                        g = D.geometry(cfg)
                    except D.Rejected:
                        assert error_code(cfg, max_nof_symbols=12) == -1, list(cfg)
                        continue
                    except D.Unsupported:
                        assert error_code(cfg, max_nof_symbols=12) == -4, list(cfg)
                        continue
                    assert_same_geometry(cfg, g)
                    accepted += 1
    assert accepted > 1000


# One job per rule of miphy_prach_demod_info, each a single change to a valid one.
LONG_OK = np.array([30720000, 0, 0, 1, 1, 0, 0, 106, 30720], np.int64)
SHORT_OK = np.array([30720000, 4, 1, 2, 1, 0, 0, 51, 0], np.int64)
SHORT_OK[D.C_NSAMPLES] = D.window_samples(SHORT_OK)


def changed(base, **kw):
    c = base.copy()
    for k, v in kw.items():
        c[getattr(D, "C_" + k)] = v
    return c


def test_the_valid_jobs_are_valid():
    assert error_code(LONG_OK) == 0 and error_code(SHORT_OK) == 0


C0_OK = np.array([30720000, 9, 1, 1, 1, 0, 0, 51, 0], np.int64)  # C0 reads 1660 samples (cyclic prefix + one symbol) of a window of 2200
C0_OK[D.C_NSAMPLES] = D.window_samples(C0_OK)
# A1 at 2.25 MHz / 15 kHz, 12 PRB: valid in every other respect (grid 144 above 2 + 139, DFT size 150), its cyclic prefix of 304 kappa is
# 22.27 samples
NOT_WHOLE = np.array([2250000, 4, 0, 1, 1, 0, 0, 12, 1 << 20], np.int64)


def test_the_jobs_the_rules_start_from_are_valid():
    assert error_of(C0_OK, max_nof_symbols=1) == (0, "")
    g = D.geometry(C0_OK)
    assert g["td_sample_offset"][0] + g["td_cp_samples"][0] + g["dft_size"] < g["window_samples"] - 1


# The message pins the rule: every MIPHY_EINVAL shares the code.
@pytest.mark.parametrize("name,cfg,kw,code,message", [
    ("not a PRACH format", changed(LONG_OK, FMT=14), dict(max_nof_symbols=1), -1, "is not a PRACH format"),
    ("long format with two time-domain occasions", changed(LONG_OK, NTD=2), dict(max_nof_symbols=1), -1, "long preambles only support one occasion"),
    ("no time-domain occasion", changed(SHORT_OK, NTD=0), dict(max_nof_symbols=2), -1, "must be greater than 0"),
    ("no frequency-domain occasion", changed(SHORT_OK, NFD=0), dict(max_nof_symbols=2, max_nof_fd_occasions=1), -1, "must be greater than 0"),
    ("time-domain occasions beyond the maximum", changed(SHORT_OK, NTD=8, NSAMPLES=1 << 20), dict(max_nof_symbols=2), -1, "occasions exceed the maxima"),
    ("frequency-domain occasions beyond the maximum", changed(LONG_OK, NFD=9), dict(max_nof_symbols=1, max_nof_fd_occasions=9), -1,
     "occasions exceed the maxima"),
    ("frequency-domain occasions beyond the buffer's", changed(LONG_OK, NFD=2), dict(max_nof_symbols=1, max_nof_fd_occasions=1), -1,
     "occasions exceed the maxima"),
    ("symbols beyond the buffer's", SHORT_OK, dict(max_nof_symbols=1), -1, "symbols exceed the buffer's"),
    ("strides beyond the interface's bound", LONG_OK, dict(max_nof_symbols=65536), -1, "buffer strides"),
    ("reserved spacing pair", changed(LONG_OK, SCS=3, NPRB=1), dict(max_nof_symbols=1), -1, "combination is reserved"),
    ("DFT size not above the grid", changed(LONG_OK, NPRB=171), dict(max_nof_symbols=1), -1, "is not sufficient for"),
    ("sequence beyond the grid", changed(LONG_OK, RB=101), dict(max_nof_symbols=1), -1, "exceeds PRACH grid size"),
    ("grid that wraps in 32 bits", changed(LONG_OK, NPRB=(1 << 32) // 144 + 7), dict(max_nof_symbols=1), -1, "is not sufficient for"),
    ("offset that wraps in 32 bits", changed(LONG_OK, RB=(1 << 32) // 144 + 1), dict(max_nof_symbols=1), -1, "exceeds PRACH grid size"),
    ("start symbol that wraps in 32 bits", changed(SHORT_OK, START=(1 << 32) - 2), dict(max_nof_symbols=2), -1, "of a window of"),
    ("time that is not a whole number of samples", NOT_WHOLE, dict(max_nof_symbols=2), -1, "not a whole number of samples"),
    ("sampling rate the RA spacing does not divide", changed(SHORT_OK, SRATE=30730000), dict(max_nof_symbols=2), -1, "is not a multiple of the RA"),
    ("long window shorter than what is read", changed(LONG_OK, NSAMPLES=3168 + 24576 - 1), dict(max_nof_symbols=1), -1, "of a window of"),
    ("short window shorter than what an occasion reads", changed(SHORT_OK, NSAMPLES=int(SHORT_OK[D.C_NSAMPLES]) - 1), dict(max_nof_symbols=2), -1,
     "of a window of"),
    ("short window between what is read and the window duration", changed(C0_OK, NSAMPLES=int(C0_OK[D.C_NSAMPLES]) - 1), dict(max_nof_symbols=1), -1,
     "equal to or greater than the PRACH window"),
    ("DFT size the device does not transform", changed(LONG_OK, SRATE=122880000, NSAMPLES=122880), dict(max_nof_symbols=1), -4, "not supported"),
])
def test_info_rejects_what_the_reference_asserts_on(name, cfg, kw, code, message):
    got, text = error_of(cfg, **kw)
    assert got == code and message in text, (name, got, text)


def test_restatement_rejects_the_same_two_rules():
    """The restatement's own to_samples and window-duration branches, on the jobs that pin them in the library."""
    with pytest.raises(D.Rejected, match="not a whole number of samples"):
        D.geometry(NOT_WHOLE)
    with pytest.raises(D.Rejected, match="fewer input samples than the PRACH window"):
        D.geometry(changed(C0_OK, NSAMPLES=int(C0_OK[D.C_NSAMPLES]) - 1))
