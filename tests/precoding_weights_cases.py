"""Cases for miphy_precoding_weights_batch (tests/test_precoding_weights.py on the CPU, tests/test_precoding_weights_gpu.py and the chain test on the GPU).

Channels have prescribed singular values, so that what the tests compare is well defined by construction and no case is ever discarded:
 - UE k's downlink channel on SRS PRG g is  e^(j phi_g) c_g  Q_g  diag(sigma)  V_k^H  (U x A): the right singular vectors V_k are common to the PRGs,
   the left ones Q_g (random unitaries), the phase phi_g (the delay's ramp) and the real gain c_g in 0.8 .. 1.25 change from PRG to PRG. The Gram
   matrix of any average is V_k diag(mean c_g^2 sigma^2) V_k^H: eigenvalues sigma^2 SIGMA^2 with sigma_i = 2^-i, a gap of 4 >= 2 between neighbours.
 - The UEs of a job take their dominant directions from one random unitary Q, each turned by a Cayley rotation within EPS = 0.2 of the identity:
   the L x A matrix D of the served directions is within sqrt(L) EPS of orthonormal rows, its singular values within 1 -+ 0.4. At reg = 0, G W is
   diagonal with entries amplitude sigma_r / |row r of pinv(D)|, so cond(G W) <= (1.4 / 0.6) (sigma_max / sigma_min) <= 2.34 x 8 < 100.
What the SRS estimator writes is H[g][a][u] = the transpose of that channel."""
import numpy as np

EPS = 0.2
SIGMA = [1.0, 0.5, 0.25, 0.125]


def unitary(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def near_identity(rng, n, eps=EPS):
    """A unitary within eps of the identity (2-norm): the Cayley transform of a Hermitian matrix of 2-norm eps / 2."""
    k = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    k = k + k.conj().T
    k *= 0.5 * eps / np.linalg.norm(k, 2)
    return np.linalg.solve(np.eye(n) - 1j * k, np.eye(n) + 1j * k)


def ue_channel(rng, V, U, G, scale=1.0, sigma=None):
    """H complex64 [G][A][U] of one UE with right singular vectors V (A x A) and singular values scale x sigma (default SIGMA, min(U, A) of them)."""
    A = V.shape[0]
    r = min(U, A)
    sigma = np.asarray(SIGMA[:r] if sigma is None else sigma, float) * scale
    H = np.zeros((G, A, U), np.complex128)
    for g in range(G):
        c = rng.uniform(0.8, 1.25) * np.exp(2j * np.pi * rng.uniform())
        S = np.zeros((U, A))
        S[:r, :r] = np.diag(sigma)
        H[g] = (c * unitary(rng, U) @ S @ V.conj().T).T
    return H.astype(np.complex64)


def job(seed, A, ues, S=2, nof_prg=4, reg=0.0, amplitude=1.0, scale=1.0):
    """ues: per UE a dict with U, l and optionally start, nprb, s, sigma. The UEs' served directions are distinct columns of one unitary, each UE turned
    by its own rotation near the identity."""
    rng = np.random.default_rng(seed)
    Q = unitary(rng, A)
    out, first = [], 0
    for k, u in enumerate(ues):
        start, nprb, s = u.get("start", 0), u.get("nprb", 8), u.get("s", 2)
        order = [(first + i) % A for i in range(A)]  # this UE's strongest directions: the columns of Q no other UE serves
        V = (near_identity(rng, A) if len(ues) > 1 else np.eye(A)) @ Q[:, order]
        H = ue_channel(rng, V, u["U"], nprb // s, scale * u.get("scale", 1.0), u.get("sigma"))
        out.append(dict(H=H, start=start, nprb=nprb, s=s, U=u["U"], l=u["l"]))
        first += u["l"]
    return dict(A=A, S=S, nof_prg=nof_prg, reg=reg, amplitude=amplitude, ues=out)


def single_ue_jobs():
    """Every A in 1..4 x U in {1, 2, 4} x l in 1..min(U, A); scales 0.1, 1, 10 in turn."""
    out = []
    for A in range(1, 5):
        for U in (1, 2, 4):
            for l in range(1, min(U, A) + 1):
                n = len(out)
                out.append(job(100 + n, A, [dict(U=U, l=l)], S=(1, 2, 4)[n % 3], nof_prg=(8, 4, 2)[n % 3], amplitude=(1.0, 0.5, 2.0)[n % 3],
                               scale=(0.1, 1.0, 10.0)[n % 3]))
    return out


# (A, layers per UE): 2, 3 and 4 UEs with L = A and (2 and 3 UEs; four UEs of one layer fill the four ports) with L < A, and two layers for one of them
MU_TOPOLOGIES = [(2, (1, 1)), (4, (1, 1)), (3, (1, 1, 1)), (4, (1, 1, 1)), (4, (1, 1, 1, 1)), (4, (2, 1, 1)), (4, (2, 2)), (3, (2, 1)), (4, (2, 1))]


def multi_ue_jobs():
    """Every topology at reg = 0 and at reg = 0.05 (in units of |h|^2; the strongest eigenvalue is about 1)."""
    out = []
    for n, (A, layers) in enumerate(MU_TOPOLOGIES):
        for reg in (0.0, 0.05):
            ues = [dict(U=(2, 4)[k % 2] if l == 2 else (1, 2)[k % 2], l=l, s=(1, 2, 4)[(n + k) % 3]) for k, l in enumerate(layers)]
            out.append(job(200 + n, A, ues, S=2, nof_prg=4, reg=reg, amplitude=0.5 if n % 2 else 1.0))
    return out


def geometry_jobs():
    """Band edges and launch geometry."""
    out = []
    # the band starts at PRB 5: output PRGs of 4 PRB share 3 and 1 PRBs with the SRS PRGs; PRG 0 lies below the band and PRG 4 above it
    out.append(job(300, 4, [dict(U=2, l=2, start=5, nprb=8, s=4)], S=4, nof_prg=5))
    out.append(job(301, 3, [dict(U=2, l=1, start=5, nprb=8, s=4), dict(U=1, l=1, start=6, nprb=12, s=2)], S=4, nof_prg=6, reg=0.01))
    # 65 output PRGs: the lane form crosses a wavefront
    out.append(job(302, 2, [dict(U=2, l=2, start=0, nprb=260, s=4)], S=4, nof_prg=65))
    # one wideband PRG over 72 SRS PRGs: the wave form crosses 64 lanes
    out.append(job(303, 4, [dict(U=4, l=2, start=3, nprb=72, s=1)], S=275, nof_prg=1))
    # six PRGs of twelve SRS PRGs each (the wave form, more wavefronts than one workgroup), two UEs
    out.append(job(304, 4, [dict(U=2, l=1, start=0, nprb=72, s=1), dict(U=2, l=2, start=4, nprb=64, s=2)], S=12, nof_prg=6, reg=0.02))
    # eight SRS PRGs under a PRG: still the lane form; nine: the wave form
    out.append(job(305, 2, [dict(U=1, l=1, start=0, nprb=16, s=1)], S=8, nof_prg=2))
    out.append(job(306, 2, [dict(U=1, l=1, start=0, nprb=20, s=1)], S=9, nof_prg=2))
    return out


def deficient_jobs():
    """Zero and rank-deficient channels. `exact`: the missing eigenvalue is exactly 0 in any arithmetic (ports 2 and 3 see nothing, or nothing at all is
    seen), so at reg = 0 the abnormal rule must fire; the others are deficient up to rounding and only have to come out finite."""
    out = []
    j = job(400, 4, [dict(U=4, l=3)], S=2, nof_prg=4)
    j["ues"][0]["H"][:, 2:, :] = 0
    out.append(dict(j, exact=True))
    j = job(401, 3, [dict(U=2, l=1)], S=2, nof_prg=4, reg=0.1)
    j["ues"][0]["H"][:] = 0
    out.append(dict(j, exact=True))
    j = job(402, 2, [dict(U=1, l=1), dict(U=1, l=1)], S=2, nof_prg=4)
    j["ues"][1]["H"][2:] = 0  # the second UE's channel vanishes on the upper half of the band: those PRGs are zero for both UEs, the others are served
    out.append(dict(j, exact=True, zero_prgs=[2, 3]))
    j = job(403, 2, [dict(U=1, l=1)], S=2, nof_prg=4)
    j["ues"][0]["H"][:] *= np.complex64(1e-23)  # |h|^2 about 1e-46: below the subnormals, the Gram matrix is 0
    out.append(dict(j, exact=True))
    out.append(dict(job(404, 4, [dict(U=4, l=3, sigma=[1.0, 0.5, 0.0, 0.0])], S=2, nof_prg=4), exact=False))
    out.append(dict(job(405, 4, [dict(U=2, l=2, sigma=[1.0, 0.0]), dict(U=1, l=1)], S=2, nof_prg=4, reg=0.05), exact=False))
    return out


def all_jobs():
    return single_ue_jobs() + multi_ue_jobs() + geometry_jobs() + deficient_jobs()


def records(miphy, jobs, gap_h=3, gap_w=5, gap_m=2):
    """(PrecodingWeightsJob array, h complex64, layout): the jobs' channels concatenated with gap_h unused elements between the blocks; layout[i][k] =
    (weights_offset, nof_weights, metrics_offset, nof_metrics) of UE k of job i, with gaps between the blocks; layout.nw / .nm: the buffer sizes."""
    rec = np.zeros(len(jobs), miphy.PrecodingWeightsJob)
    hs, ho, wo, mo, layout = [], 1, 4, 3, []
    hs.append(np.zeros(1, np.complex64))
    for i, j in enumerate(jobs):
        r = rec[i]
        r["nof_ues"], r["nof_ports"], r["prg_size"], r["nof_prg"], r["reg"], r["amplitude"] = len(j["ues"]), j["A"], j["S"], j["nof_prg"], j["reg"], j["amplitude"]
        lay = []
        for k, u in enumerate(j["ues"]):
            e = r["ue"][k]
            nw, nm = j["nof_prg"] * j["A"] * u["l"], 3 * j["nof_prg"] * u["l"]
            e["h_offset"], e["weights_offset"], e["metrics_offset"] = ho, wo, mo
            e["start_prb"], e["nof_prb"], e["prg_size"], e["nof_ue_ports"], e["nof_layers"] = u["start"], u["nprb"], u["s"], u["U"], u["l"]
            hs += [u["H"].ravel(), np.zeros(gap_h, np.complex64)]
            lay.append((wo, nw, mo, nm))
            ho, wo, mo = ho + u["H"].size + gap_h, wo + nw + gap_w, mo + nm + gap_m
        layout.append(lay)
    return rec, np.concatenate(hs), dict(ues=layout, nw=wo + 8, nm=mo + 8)
