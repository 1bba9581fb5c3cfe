"""The contract of miphy_precoding_weights_batch in numpy: the 23.5 reference computes no precoding, so this restatement is the specification.
Two forms: `weights64` in float64 through numpy.linalg.eigh and numpy.linalg.solve, and `weights32` in float32 in the operation order of
csrc/precoding_weights.hip and csrc/jacobi_device.h (every product, sum, quotient and square root one float32 operation), which the kernel is held to
byte for byte. tests/test_precoding_weights.py holds the second to the first.

A job is a dict: A (antenna ports), S (PRBs per output PRG), nof_prg, reg, amplitude and ues, a list of dicts with H (complex64 [G][A][U], as
miphy_srs_estimate_batch writes it), start, nprb, s (the sounding's PRG size), U and l (layers)."""
import numpy as np

from pusch_layers_cases import F, _add, _cm, _mul, _mulc, _norm
from pusch_mmse_cases import _ldl, _lower_mul, _pos_normal

SWEEPS = 5
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
LANE_MAX = 8


# ------------------------------------------------------------------------------------------------ the SRS PRGs under an output PRG
def srs_range(ue, S, j):
    """(i0, i1, lo, hi): the SRS PRGs under output PRG j and the PRBs [lo, hi) they share with it; hi == lo: none is met, the nearest alone."""
    b0, b1, s = ue["start"], ue["start"] + ue["nprb"], ue["s"]
    lo, hi = max(j * S, b0), min((j + 1) * S, b1)
    if hi > lo:
        return (lo - b0) // s, (hi - 1 - b0) // s, lo, hi
    i = 0 if (j + 1) * S <= b0 else ue["nprb"] // s - 1
    return i, i, 0, 0


def srs_weights(ue, S, j):
    """[(i, w_i)] and their sum."""
    i0, i1, lo, hi = srs_range(ue, S, j)
    if hi == lo:
        return [(i0, 1)], 1
    b0, s = ue["start"], ue["s"]
    return [(i, min(b0 + (i + 1) * s, hi) - max(b0 + i * s, lo)) for i in range(i0, i1 + 1)], hi - lo


def max_count(job):
    """The largest number of SRS PRGs of one UE under one output PRG, by looking at every one."""
    return max(len(srs_weights(ue, job["S"], j)[0]) for ue in job["ues"] for j in range(job["nof_prg"]))


def wave_form(job):
    return max_count(job) > LANE_MAX


def row_slices(job):
    out, r = [], 0
    for ue in job["ues"]:
        out.append(slice(r, r + ue["l"]))
        r += ue["l"]
    return out


# ------------------------------------------------------------------------------------------------ float64
def gram64(ue, S, j):
    iw, wt = srs_weights(ue, S, j)
    H = ue["H"].astype(np.complex128)
    return sum(w * (H[i].conj() @ H[i].T) for i, w in iw) / wt


def eig64(R):
    """Eigenvalues descending (stable) with their eigenvectors by column."""
    lam, V = np.linalg.eigh(R)
    order = np.argsort(-lam, kind="stable")
    return lam[order], V[:, order]


def fix_columns(W, amplitude):
    with np.errstate(all="ignore"):  # (a zero column of a channel that is deficient up to rounding: the caller does not compare it)
        W = W * (amplitude / np.linalg.norm(W, axis=0))
    for c in range(W.shape[1]):
        if abs(W[0, c]) >= amplitude * 2.0 ** -10:
            W[:, c] *= np.conj(W[0, c]) / abs(W[0, c])
    return W


def solve64(job, j):
    """(W [A][L], G [L][A], lam [L], sig [L], leak [L], ok) of output PRG j."""
    A, rows = job["A"], []
    lam = []
    for ue in job["ues"]:
        ev, V = eig64(gram64(ue, job["S"], j))
        for i in range(ue["l"]):
            lam.append(max(ev[i], 0.0))
            rows.append(np.sqrt(lam[-1]) * V[:, i].conj())
    G = np.array(rows).reshape(len(rows), A)
    B = G @ G.conj().T + job["reg"] * np.eye(len(rows))
    ok = np.linalg.matrix_rank(B, tol=1e-9 * max(np.abs(B).max(), 1e-300)) == len(rows)
    if not ok:
        z = np.zeros(len(rows))
        return np.zeros((A, len(rows)), complex), G, np.array(lam), z, z, False
    W = fix_columns(np.linalg.solve(B, G).conj().T, job["amplitude"])
    D = np.abs(G @ W) ** 2
    return W, G, np.array(lam), np.diag(D).copy(), D.sum(axis=1) - np.diag(D), True


def weights64(job):
    """Per UE (W [nof_prg][A][l], metrics [nof_prg][l][3])."""
    per_prg = [solve64(job, j) for j in range(job["nof_prg"])]
    out = []
    for sl in row_slices(job):
        W = np.array([p[0][:, sl] for p in per_prg])
        M = np.array([np.stack([p[2][sl], p[3][sl], p[4][sl]], axis=-1) for p in per_prg])
        out.append((W, M))
    return out


# ------------------------------------------------------------------------------------------------ float32, the kernel's operations
def gram32(ue, A, S, j, wave):
    """Step 1 for one UE and output PRG: (d[a], o[a][b] for a > b) as float32 scalars."""
    i0, i1, lo, hi = srs_range(ue, S, j)
    iw = dict(srs_weights(ue, S, j)[0])
    U, H = ue["U"], ue["H"]
    lanes = 64 if wave else 1
    zero = np.zeros(lanes, F)
    d = [zero.copy() for _ in range(A)]
    o = [[(zero.copy(), zero.copy()) for _ in range(a)] for a in range(A)]
    for t in range(lanes):
        for i in range(i0 + t, i1 + 1, lanes):
            w = F(iw[i])
            h = [[(F(H[i, a, u].real), F(H[i, a, u].imag)) for u in range(U)] for a in range(A)]
            for a in range(A):
                for b in range(a + 1):
                    if a == b:
                        acc = _norm(h[a][0])
                        for u in range(1, U):
                            acc = acc + _norm(h[a][u])
                        d[a][t] = d[a][t] + w * acc
                    else:
                        acc = _cm(h[a][0], h[b][0])
                        for u in range(1, U):
                            acc = _add(acc, _cm(h[a][u], h[b][u]))
                        o[a][b][0][t] = o[a][b][0][t] + w * acc[0]
                        o[a][b][1][t] = o[a][b][1][t] + w * acc[1]
    if wave:
        lane = np.arange(64)
        off = 32
        while off >= 1:
            d = [x + x[lane ^ off] for x in d]
            o = [[(x + x[lane ^ off], y + y[lane ^ off]) for x, y in row] for row in o]
            off >>= 1
    wt = F(hi - lo if hi > lo else 1)
    return [x[0] / wt for x in d], [[(x[0] / wt, y[0] / wt) for x, y in row] for row in o]


def jacobi32(ar, ai, n):
    """csrc/jacobi_device.h on float32 arrays ar[p][q], ai[p][q] (one entry per problem), order n: (eigenvalues [n], vr, vi)."""
    N = ar[0][0].shape
    ar = [[x.copy() for x in row] for row in ar]
    ai = [[x.copy() for x in row] for row in ai]
    vr = [[np.full(N, 1 if i == k else 0, F) for k in range(n)] for i in range(n)]
    vi = [[np.zeros(N, F) for k in range(n)] for i in range(n)]
    one = F(1)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                if q >= n:
                    continue
                bx, by = ar[p][q], ai[p][q]
                g2 = bx * bx + by * by
                do = _pos_normal(g2)
                g = np.sqrt(g2)
                e = (bx / g, by / g)
                tau = (ar[q][q] - ar[p][p]) / (g + g)
                ta = one / (np.abs(tau) + np.sqrt(one + tau * tau))
                t = np.where(tau < 0, -ta, ta)
                c = one / np.sqrt(one + t * t)
                s = t * c
                z = (s * e[0], s * e[1])

                def cols(xr, xi, k):
                    xp, xq = (xr[k][p], xi[k][p]), (xr[k][q], xi[k][q])
                    u, w = _mulc(xq, z), _mul(xp, z)
                    new = (c * xp[0] - u[0], c * xp[1] - u[1], w[0] + c * xq[0], w[1] + c * xq[1])
                    xr[k][p], xi[k][p] = np.where(do, new[0], xp[0]), np.where(do, new[1], xp[1])
                    xr[k][q], xi[k][q] = np.where(do, new[2], xq[0]), np.where(do, new[3], xq[1])

                for k in range(n):
                    cols(ar, ai, k)
                    cols(vr, vi, k)
                for k in range(n):
                    xp, xq = (ar[p][k], ai[p][k]), (ar[q][k], ai[q][k])
                    u, w = _mul(z, xq), _cm(z, xp)
                    new = (c * xp[0] - u[0], c * xp[1] - u[1], w[0] + c * xq[0], w[1] + c * xq[1])
                    ar[p][k], ai[p][k] = np.where(do, new[0], xp[0]), np.where(do, new[1], xp[1])
                    ar[q][k], ai[q][k] = np.where(do, new[2], xq[0]), np.where(do, new[3], xq[1])
                zero = np.zeros(N, F)
                for (i, k) in ((p, q), (q, p)):
                    ar[i][k], ai[i][k] = np.where(do, zero, ar[i][k]), np.where(do, zero, ai[i][k])
                ai[p][p], ai[q][q] = np.where(do, zero, ai[p][p]), np.where(do, zero, ai[q][q])
    return [ar[c][c] for c in range(n)], vr, vi


def eig32(R):
    """Jacobi of complex64 matrices R [N][n][n] in float32: (lam [N][n] descending, V [N][n][n] by column), as the kernel orders them."""
    R = np.asarray(R, np.complex64)
    n = R.shape[-1]
    ar = [[R[:, p, q].real.astype(F) for q in range(n)] for p in range(n)]
    ai = [[R[:, p, q].imag.astype(F) for q in range(n)] for p in range(n)]
    ev, vr, vi = jacobi32(ar, ai, n)
    rank = _ranks(ev)
    lam = np.zeros(R.shape[:2], F)
    V = np.zeros(R.shape, np.complex64)
    for i in range(n):
        for c in range(n):
            m = rank[c] == i
            lam[m, i] = ev[c][m]
            for a in range(n):
                V.real[m, a, i], V.imag[m, a, i] = vr[a][c][m], vi[a][c][m]
    return lam, V


def _ranks(ev):
    n = len(ev)
    rank = []
    for c in range(n):
        r = np.zeros(ev[0].shape, np.int64)
        for c2 in range(n):
            if c2 != c:
                r = r + ((ev[c2] > ev[c]) | ((ev[c2] == ev[c]) & (c2 < c)))
        rank.append(r)
    return rank


def weights32(job):
    """Per UE (W complex64 [nof_prg][A][l], metrics float32 [nof_prg][l][3]): the bytes the kernel writes, in the form the job takes."""
    A, S, P = job["A"], job["S"], job["nof_prg"]
    wave = wave_form(job)
    reg, amp = F(job["reg"]), F(job["amplitude"])
    zero = np.zeros(P, F)
    G, lam = [], []  # G[r][a] pairs, lam[r]
    with np.errstate(all="ignore"):
        for ue in job["ues"]:
            grams = [gram32(ue, A, S, j, wave) for j in range(P)]
            ar = [[None] * A for _ in range(A)]
            ai = [[None] * A for _ in range(A)]
            for a in range(A):
                ar[a][a], ai[a][a] = np.array([g[0][a] for g in grams], F), zero.copy()
                for b in range(a):
                    ar[a][b], ai[a][b] = np.array([g[1][a][b][0] for g in grams], F), np.array([g[1][a][b][1] for g in grams], F)
                    ar[b][a], ai[b][a] = ar[a][b].copy(), -ai[a][b]
            ev, vr, vi = jacobi32(ar, ai, A)
            rank = _ranks(ev)
            for i in range(ue["l"]):
                l = zero.copy()
                col = [(zero.copy(), zero.copy()) for _ in range(A)]
                for c in range(A):
                    m = rank[c] == i
                    l = np.where(m, ev[c], l)
                    col = [(np.where(m, vr[a][c], col[a][0]), np.where(m, vi[a][c], col[a][1])) for a in range(A)]
                l = np.where(l > 0, l, zero)
                q = np.sqrt(l)
                lam.append(l)
                G.append([(q * col[a][0], -(q * col[a][1])) for a in range(A)])
        L = len(G)
        B = [[None] * L for _ in range(L)]
        for i in range(L):
            for c in range(i + 1):
                if i == c:
                    t = _norm(G[i][0])
                    for a in range(1, A):
                        t = t + _norm(G[i][a])
                    B[i][i] = (t + reg, None)
                else:
                    t = _mulc(G[i][0], G[c][0])
                    for a in range(1, A):
                        t = _add(t, _mulc(G[i][a], G[c][a]))
                    B[i][c] = t
        ok, rp, N = _ldl(B, L)
        ok = ok & np.ones(P, bool)
        W = [[None] * L for _ in range(A)]
        for a in range(A):
            T = _lower_mul(N, [G[i][a] for i in range(L)])
            Z = [(T[i][0] * rp[i], T[i][1] * rp[i]) for i in range(L)]
            for i in range(L):
                acc = Z[i]
                for k in range(i + 1, L):
                    acc = _add(acc, _cm(N[k][i], Z[k]))
                W[a][i] = (acc[0], -acc[1])
        floor_ = amp * F(2.0 ** -10)
        for i in range(L):
            n2 = _norm(W[0][i])
            for a in range(1, A):
                n2 = n2 + _norm(W[a][i])
            ok = ok & _pos_normal(n2)
            f = amp / np.sqrt(n2)
            for a in range(A):
                W[a][i] = (f * W[a][i][0], f * W[a][i][1])
            p = W[0][i]
            m2 = _norm(p)
            m = np.sqrt(m2)
            turn = _pos_normal(m2) & (m >= floor_)
            e = (p[0] / m, -(p[1] / m))
            for a in range(1, A):
                t = _mul(W[a][i], e)
                W[a][i] = (np.where(turn, t[0], W[a][i][0]), np.where(turn, t[1], W[a][i][1]))
            W[0][i] = (np.where(turn, m, p[0]), np.where(turn, zero, p[1]))
        sig, leak = [None] * L, [zero.copy() for _ in range(L)]
        for r in range(L):
            for c in range(L):
                dd = _mul(G[r][0], W[0][c])
                for a in range(1, A):
                    dd = _add(dd, _mul(G[r][a], W[a][c]))
                e = _norm(dd)
                if c == r:
                    sig[r] = e
                else:
                    leak[r] = leak[r] + e
    out = []
    for sl in row_slices(job):
        rows = range(sl.start, sl.stop)
        Wk = np.zeros((P, A, len(rows)), np.complex64)
        Mk = np.zeros((P, len(rows), 3), F)
        for i, r in enumerate(rows):
            for a in range(A):
                Wk.real[:, a, i], Wk.imag[:, a, i] = np.where(ok, W[a][r][0], zero), np.where(ok, W[a][r][1], zero)  # keeps the sign of a zero
            Mk[:, i, 0], Mk[:, i, 1], Mk[:, i, 2] = lam[r], np.where(ok, sig[r], zero), np.where(ok, leak[r], zero)
        out.append((Wk, Mk))
    return out
