"""CPU: the contract of miphy_precoding_weights_batch. The 23.5 reference computes no precoding, so the specification is the numpy restatement of
tests/precoding_weights_ref.py; here its float32 form (the kernel's operation order, which the GPU test holds the kernel to byte for byte) is held to
float64 numpy.linalg.eigh and numpy.linalg.solve, the case builder to what it promises, and miphy_precoding_weights_info to every rule.

Bounds. EIG = 1e-5 on the invariants of the decomposition, relative to |R|: ten times the 1.0e-6 a float32 Jacobi of five sweeps reaches.
Subspaces: a residual of EIG |R| against a gap of at least 3/64 |R| (the cases' eigenvalues are 1, 1/4, 1/16, 1/64 of the largest, so the smallest gap
between a served and an unserved direction is 1/16 - 1/64) turns an eigenvector by at most EIG x 64 / 3 = 2.2e-4: SUB. Final columns: that, times the
bound 2.34 x 8 = 19 of the cases on the condition of the zero forcing: COL = 4.1e-3 of the amplitude, divided by the share of the column's norm on port
0 (at least 2^-10), which is what the phase is taken from."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import miphy
import precoding_weights_cases as G
import precoding_weights_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG = 1e-5
SUB = EIG * 64 / 3
COL = SUB * 2.34 * 8


@pytest.fixture(scope="module")
def solved():
    """Every case with its float32 and float64 results, computed once."""
    with np.errstate(all="ignore"):
        return [(j, R.weights32(j), R.weights64(j)) for j in G.all_jobs()]


def random_grams(rng, count=300):
    """A in 2..4, U in 1..4, scales 1e-2..1e2, a third of them rank deficient."""
    out = {2: [], 3: [], 4: []}
    for n in range(count):
        A, U = int(rng.integers(2, 5)), int(rng.integers(1, 5))
        h = (rng.standard_normal((A, U)) + 1j * rng.standard_normal((A, U))) * 10 ** rng.uniform(-1, 1)
        if n % 3 == 0:
            h[:, U // 2:] = 0 if U > 1 else h[:, U // 2:]
        out[A].append((h.conj() @ h.T).astype(np.complex64))
    return out


def test_the_float32_jacobi_against_eigh():
    worst = dict(res=0.0, orth=0.0, lam=0.0)
    for A, grams in random_grams(np.random.default_rng(11)).items():
        Rm = np.array(grams)
        lam, V = R.eig32(Rm)
        assert np.isfinite(lam).all() and np.isfinite(V.view(np.float32)).all()
        assert (np.diff(lam, axis=1) <= 0).all(), "eigenvalues descending"
        for n in range(len(Rm)):
            R64, V64, L64 = Rm[n].astype(complex), V[n].astype(complex), np.diag(lam[n].astype(float))
            scale = np.abs(R64).sum(axis=1).max()
            worst["res"] = max(worst["res"], np.abs(R64 @ V64 - V64 @ L64).sum(axis=1).max() / scale)
            worst["orth"] = max(worst["orth"], np.abs(V64.conj().T @ V64 - np.eye(A)).max())
            worst["lam"] = max(worst["lam"], np.abs(lam[n] - R.eig64(R64)[0]).max() / scale)
    print("worst: residual %.3g, orthonormality %.3g, eigenvalues %.3g" % (worst["res"], worst["orth"], worst["lam"]))
    assert worst["res"] <= EIG and worst["orth"] <= EIG and worst["lam"] <= EIG, worst


def test_no_nan_from_zero_subnormal_or_deficient_matrices():
    tiny = np.float32(1e-30)
    mats = [np.zeros((4, 4)), np.full((4, 4), 1e-42), np.full((4, 4), tiny), np.diag([1, 0, 0, 0]), np.ones((4, 4)), np.diag([1e-45, 1, 0, 1e38]),
            np.array([[1, 1e-25, 0, 0], [1e-25, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])]
    lam, V = R.eig32(np.array(mats, np.complex64))
    assert np.isfinite(lam).all() and np.isfinite(V.view(np.float32)).all()
    assert lam[0].tolist() == [0, 0, 0, 0] and lam[3].tolist() == [1, 0, 0, 0]
    assert abs(lam[4][0] - 4) <= 4 * EIG and np.abs(lam[4][1:]).max() <= 4 * EIG


def test_the_cases_are_what_they_promise():
    """Gaps of at least 2 between a served eigenvalue and the next, and cond(G W) <= 100 at reg = 0, by construction: nothing is discarded."""
    kinds = set()
    for j in G.single_ue_jobs() + G.multi_ue_jobs() + G.geometry_jobs():
        for p in range(j["nof_prg"]):
            for ue in j["ues"]:
                lam = R.eig64(R.gram64(ue, j["S"], p))[0]
                if ue["l"] < min(ue["U"], j["A"]):
                    assert lam[ue["l"] - 1] >= 2 * lam[ue["l"]], (j["A"], ue["U"], ue["l"])
                assert lam[ue["l"] - 1] > 1e-3 * lam[0]
            W, Gm = R.solve64(dict(j, reg=0.0), p)[:2]
            assert np.linalg.cond(Gm @ W) <= 100
        L = sum(u["l"] for u in j["ues"])
        kinds.add((len(j["ues"]), L == j["A"], j["reg"] > 0))
    assert {(k, full, reg) for k in (2, 3) for full in (False, True) for reg in (False, True)} <= kinds
    assert {(4, True, False), (4, True, True)} <= kinds
    singles = {(j["A"], j["ues"][0]["U"], j["ues"][0]["l"]) for j in G.single_ue_jobs()}
    assert singles == {(A, U, l) for A in range(1, 5) for U in (1, 2, 4) for l in range(1, min(U, A) + 1)}
    geo = G.geometry_jobs()
    assert sorted(w for _, w in R.srs_weights(geo[0]["ues"][0], 4, 2)[0]) == [1, 3] and R.srs_range(geo[0]["ues"][0], 4, 0)[2:] == (0, 0)
    assert R.srs_range(geo[0]["ues"][0], 4, 4) == (1, 1, 0, 0), "above the band: its last SRS PRG"
    assert [R.max_count(j) for j in geo[2:]] == [1, 72, 12, 8, 9] and [R.wave_form(j) for j in geo[2:]] == [False, True, True, False, True]
    assert geo[2]["nof_prg"] == 65


def test_subspaces_against_eigh():
    """The projector onto each UE's l strongest directions, float32 Jacobi against eigh, on the Gram matrices of every case."""
    worst = 0.0
    for j in G.single_ue_jobs() + G.multi_ue_jobs() + G.geometry_jobs():
        for ue in j["ues"]:
            grams = np.array([R.gram64(ue, j["S"], p) for p in range(j["nof_prg"])])
            V32 = R.eig32(grams.astype(np.complex64))[1].astype(complex)
            for p in range(len(grams)):
                V64 = R.eig64(grams[p])[1]
                a, b = V32[p][:, :ue["l"]], V64[:, :ue["l"]]
                worst = max(worst, np.linalg.norm(a @ a.conj().T - b @ b.conj().T, 2))
    print("worst projector difference %.3g" % worst)
    assert worst <= SUB


def test_final_columns_and_metrics_against_float64(solved):
    worst = 0.0
    for j, got, want in solved:
        if "exact" in j:
            continue
        for (W32, M32), (W64, M64) in zip(got, want):
            share = np.maximum(np.abs(W64[:, :1, :]) / j["amplitude"], 2.0 ** -10)
            e = (np.abs(W32 - W64) * share).max() / j["amplitude"]
            worst = max(worst, e)
            assert e <= COL, (j["A"], [u["l"] for u in j["ues"]], e)
            assert np.abs(np.linalg.norm(W32.astype(complex), axis=1) - j["amplitude"]).max() <= 2e-6 * j["amplitude"], "columns of 2-norm amplitude (32 roundings of 2^-24)"
            assert (W32[:, 0, :].imag == 0).all() and (W32[:, 0, :].real >= 0).all(), "port 0 real and not negative"
            assert np.abs(M32 - M64).max() <= 2 * COL * M64.max()
    print("worst column difference (weighted by the share on port 0) %.3g of the amplitude" % worst)


def test_one_ue_is_plain_eigen_beamforming(solved):
    n = 0
    for j, got, _ in solved:
        if len(j["ues"]) != 1 or "exact" in j:
            continue
        ue, (W32, M32) = j["ues"][0], got[0]
        for p in range(j["nof_prg"]):
            lam, V = R.eig64(R.gram64(ue, j["S"], p))
            for i in range(ue["l"]):
                w = W32[p, :, i].astype(complex) / j["amplitude"]
                assert abs(abs(np.vdot(V[:, i], w)) - 1) <= SUB, "column i is eigenvector i up to its phase"
                assert abs(M32[p, i, 0] - lam[i]) <= EIG * lam[0]
                assert abs(M32[p, i, 1] - lam[i] * j["amplitude"] ** 2) <= 2 * SUB * lam[0] * j["amplitude"] ** 2, "sig = lambda amplitude^2"
        n += 1
    assert n >= 21


def test_zero_forcing_leaves_no_leak_at_reg_zero(solved):
    n = 0
    for j, got, _ in solved:
        if len(j["ues"]) < 2 or j["reg"] != 0 or "exact" in j:
            continue
        for W32, M32 in got:
            assert (M32[..., 2] <= 1e-5 * M32[..., 1]).all(), (j["A"], [u["l"] for u in j["ues"]], (M32[..., 2] / M32[..., 1]).max())
            assert (M32[..., 1] > 0).all()
        n += 1
    assert n >= 9


def test_rank_deficiency_gives_zeros(solved):
    n = 0
    for j, got, _ in solved:
        if "exact" not in j:
            continue
        for W32, M32 in got:
            assert np.isfinite(W32.view(np.float32)).all() and np.isfinite(M32).all()
            if j["exact"]:
                zero = j.get("zero_prgs", range(j["nof_prg"]))
                served = [p for p in range(j["nof_prg"]) if p not in zero]
                assert not W32[list(zero)].any() and not M32[list(zero)][..., 1:].any(), "zero weights, sig and leak"
                assert all(W32[p].any() for p in served), "nothing else is affected"
        n += 1
    assert n == 6


# ------------------------------------------------------------------------------------------------ miphy_precoding_weights_info
def record(**changes):
    """A valid job of two UEs (A = 4), with fields replaced: ue0_xxx / ue1_xxx name a UE's field."""
    rec = G.records(miphy, [G.job(1, 4, [dict(U=2, l=2, start=3, nprb=12, s=4), dict(U=4, l=1, start=0, nprb=8, s=2)], S=2, nof_prg=9, reg=0.1)])[0]
    for k, v in changes.items():
        if k.startswith("ue"):
            rec["ue"][0, int(k[2])][k[4:]] = v
        else:
            rec[k] = v
    return rec[0]


def refused(text, **changes):
    with pytest.raises(Exception) as e:
        miphy.precoding_weights_info(record(**changes))
    assert "error -1" in str(e.value) and text in str(e.value), str(e.value)
    assert text in miphy.lib().miphy_last_error().decode()


def test_info_reports_sizes_and_form():
    got = miphy.precoding_weights_info(record())
    assert int(got["nof_layers"]) == 3 and list(got["nof_weights"]) == [9 * 4 * 2, 9 * 4 * 1, 0, 0] and list(got["nof_metrics"]) == [54, 27, 0, 0]
    assert int(got["max_srs_prg"]) == 2 and int(got["wave_form"]) == 0  # PRBs 6 and 7 of output PRG 3 lie in two SRS PRGs of 4 from PRB 3
    got = miphy.precoding_weights_info(record(prg_size=275, nof_prg=1))
    assert int(got["max_srs_prg"]) == 4 and int(got["wave_form"]) == 0
    got = miphy.precoding_weights_info(record(prg_size=275, nof_prg=1, ue1_nof_prb=20, ue1_prg_size=1))
    assert int(got["max_srs_prg"]) == 20 and int(got["wave_form"]) == 1


def test_info_counts_the_srs_prgs_as_looking_at_every_output_prg_does():
    n = 0
    for start, nprb, s, S in itertools.product((0, 1, 2, 3, 5, 30), (4, 8, 12, 40), (1, 2, 4), (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 275)):
        for nof_prg in (1, 2, 3, 7, 11, 64):
            j = dict(A=1, S=S, nof_prg=nof_prg, ues=[dict(start=start, nprb=nprb, s=s, U=1, l=1)])
            got = miphy.precoding_weights_info(record(nof_ues=1, nof_ports=1, prg_size=S, nof_prg=nof_prg, ue0_start_prb=start, ue0_nof_prb=nprb,
                                                      ue0_prg_size=s, ue0_nof_ue_ports=1, ue0_nof_layers=1))
            assert int(got["max_srs_prg"]) == R.max_count(j) and int(got["wave_form"]) == R.wave_form(j), (start, nprb, s, S, nof_prg)
            n += 1
    assert n > 5000


def test_the_rules():
    miphy.precoding_weights_info(record())
    refused("nof_ues is 1..4", nof_ues=0)
    refused("nof_ues is 1..4", nof_ues=5)
    refused("nof_ports is 1..4", nof_ports=0)
    refused("nof_ports is 1..4", nof_ports=5)
    refused("prg_size and nof_prg are at least 1", prg_size=0)
    refused("prg_size and nof_prg are at least 1", nof_prg=0)
    refused("reg is finite and not negative", reg=-1e-3)
    refused("reg is finite and not negative", reg=np.inf)
    refused("reg is finite and not negative", reg=np.nan)
    miphy.precoding_weights_info(record(reg=0.0))
    refused("amplitude is a positive normal number", amplitude=0.0)
    refused("amplitude is a positive normal number", amplitude=-1.0)
    refused("amplitude is a positive normal number", amplitude=1e-42)
    refused("amplitude is a positive normal number", amplitude=np.inf)
    refused("SRS prg_size of a UE is 1, 2 or 4", ue1_prg_size=3)
    refused("SRS prg_size of a UE is 1, 2 or 4", ue0_prg_size=0)
    refused("the sounded band of a UE", ue0_nof_prb=0)
    refused("the sounded band of a UE", ue0_nof_prb=10)
    refused("the sounded band of a UE", ue1_nof_prb=276)
    refused("the sounded band of a UE", ue1_start_prb=268)  # 268 + 8 > 275
    miphy.precoding_weights_info(record(ue1_start_prb=267))
    refused("nof_ue_ports of a UE is 1, 2 or 4", ue0_nof_ue_ports=3)
    refused("nof_ue_ports of a UE is 1, 2 or 4", ue1_nof_ue_ports=0)
    refused("nof_layers of a UE is 1..nof_ue_ports", ue0_nof_layers=3)
    refused("nof_layers of a UE is 1..nof_ue_ports", ue1_nof_layers=0)
    refused("at most 4 and at most nof_ports", ue1_nof_layers=3)  # 2 + 3 layers
    refused("at most 4 and at most nof_ports", nof_ports=2)  # 3 layers on 2 ports
    miphy.precoding_weights_info(record(nof_ports=3))
    miphy.precoding_weights_info(record(nof_ues=1, ue1_nof_ue_ports=3))  # entries from nof_ues on are not read
    with pytest.raises(Exception, match="null argument"):
        miphy.binding.check(miphy.lib().miphy_precoding_weights_info(None, None))


def test_exports_and_record_layouts_against_the_header():
    out = subprocess.check_output(["nm", "-D", "--defined-only", miphy.lib_path], text=True)
    assert " T miphy_precoding_weights_info" in out and " T miphy_precoding_weights_batch" in out
    names = (("miphy_precoding_weights_ue", miphy.PrecodingWeightsUe), ("miphy_precoding_weights_job", miphy.PrecodingWeightsJob),
             ("miphy_precoding_weights_info_t", miphy.PrecodingWeightsInfo))
    lines = ['printf("%%zu\\n", sizeof(%s));' % n for n, _ in names]
    for n, dt in names:
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (n, f) for f in dt.names]
    src = '#include "miphy.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    want = [dt.itemsize for _, dt in names] + [dt.fields[f][1] for _, dt in names for f in dt.names]
    assert got == want, (got, want)
    assert got[:3] == [24, 112, 44]
