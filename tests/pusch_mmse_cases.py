"""MMSE-IRC for PUSCH on 1..4 layers, on the host: what miphy_pusch_noise_covariance_batch and miphy_channel_equalize_mmse_batch are held to.
The 23.5 reference has no MMSE equaliser ("MMSE equalizer is not implemented yet"), so the contract is restated here:

  mmse_double()     float64 through numpy.linalg: W = C^-1, A = t^2 H^H W H + I, B = A^-1, x~ = t B H^H W y, gamma_l = 1 - B_ll,
                    x_l = x~_l / gamma_l, nvar_l = B_ll / gamma_l
  mmse_single()     numpy float32 in the operation order of csrc/mmse_device.h (what the device must reproduce bit for bit)
  covariance()      float64: the DM-RS residuals of pusch_layers_estimator_cases.estimate() as a P x P matrix per PRG
  coloured()        C = sigma^2 (I + sum_k rho_k a_k a_k^H): white noise plus rank-one interferers
  interfered_tx()   pusch_layers_estimator_cases.chain_tx() plus a rank-one interferer on every element of the allocation, DM-RS included
  irc_llr()         the host chain in front of the decoder: estimate() -> covariance() -> mmse_single() -> compose_llr()
"""
import numpy as np

import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
from pusch_layers_cases import F, _add, _cm, _dot, _mul, _mulc, _norm

TINY = PL.TINY


# ------------------------------------------------------------------------------------------------ float64 model
def _cov_per_element(cov, npt, n, re_per_cov):
    """cov [matrices][P][P] (or [P][P]) -> [n][P][P]."""
    cov = np.asarray(cov).reshape(-1, npt, npt)
    idx = np.arange(n) // re_per_cov if re_per_cov else np.zeros(n, int)
    return cov[idx]


def mmse_double(y, h, cov, tx, re_per_cov=0):
    """y [P][n], h [L][P][n], cov [matrices][P][P] -> (x complex128 [L][n], nvar float64 [L][n])."""
    nl, npt, n = h.shape
    hh = np.asarray(h).astype(np.complex128).transpose(2, 1, 0)  # [n][P][L]
    yy = np.asarray(y).astype(np.complex128).T[:, :, None]
    c = _cov_per_element(np.asarray(cov).astype(np.complex128), npt, n, re_per_cov)
    low = np.tril(np.ones((npt, npt), bool), -1)
    c = np.where(low, c, 0) + np.where(low, c, 0).conj().transpose(0, 2, 1) + np.real(np.einsum("npp->np", c))[:, :, None] * np.eye(npt)  # lower triangle only
    w = np.linalg.inv(c)
    hw = hh.conj().transpose(0, 2, 1) @ w
    a = tx * tx * (hw @ hh) + np.eye(nl)
    b = np.linalg.inv(a)
    xt = tx * (b @ (hw @ yy))[:, :, 0]
    bll = np.real(np.einsum("nll->nl", b))
    gamma = 1.0 - bll
    return (xt / gamma).T, (bll / gamma).T


def coloured(rng, npt, sigma2, rhos):
    """C = sigma2 (I + sum_k rho_k a_k a_k^H), a_k ~ CN(0, 1) per port: complex128 [P][P]."""
    c = np.eye(npt, dtype=np.complex128)
    for rho in rhos:
        a = (rng.standard_normal(npt) + 1j * rng.standard_normal(npt)) / np.sqrt(2)
        c = c + rho * np.outer(a, a.conj())
    return sigma2 * c


# ------------------------------------------------------------------------------------------------ float32 restatement of csrc/mmse_device.h
def _pos_normal(x):
    return (x >= TINY) & (x < np.inf)


def _ldl(a, n):
    """mmse_ldl: a[i][j] (i >= j) pairs of float32 arrays -> (ok, r[j], m[i][j] for i > j)."""
    one = F(1)
    w = [[None] * n for _ in range(n)]
    lf = [[None] * n for _ in range(n)]
    m = [[None] * n for _ in range(n)]
    r = [None] * n
    ok = True
    for j in range(n):
        for i in range(j, n):
            acc = (a[j][j][0], None) if i == j else a[i][j]
            for k in range(j):
                t = _mulc(w[i][k], lf[j][k])
                acc = (acc[0] - t[0], None) if i == j else (acc[0] - t[0], acc[1] - t[1])
            w[i][j] = acc
        d = w[j][j][0]
        r[j] = one / d
        ok = ok & _pos_normal(d)
        for i in range(j + 1, n):
            lf[i][j] = (w[i][j][0] * r[j], w[i][j][1] * r[j])
    for j in range(n):
        for i in range(j + 1, n):
            acc = lf[i][j]
            for k in range(j + 1, i):
                acc = _add(acc, _mul(lf[i][k], m[k][j]))
            m[i][j] = (-acc[0], -acc[1])
    return ok, r, m


def _lower_mul(nm, y):
    v = []
    for p in range(len(y)):
        acc = y[p]
        for k in range(p):
            acc = _add(acc, _mul(nm[p][k], y[k]))
        v.append(acc)
    return v


def mmse_single(y, h, cov, tx, re_per_cov=0):
    """y complex64 [P][n], h complex64 [L][P][n], cov complex64 [matrices][P][P] -> (x complex64 [L][n], nvar float32 [L][n]);
    csrc/mmse_device.h, operation for operation."""
    y = np.asarray(y, np.complex64)
    h = np.asarray(h, np.complex64)
    nl, npt, n = h.shape
    c = _cov_per_element(np.asarray(cov, np.complex64), npt, n, re_per_cov)
    H = [[(np.ascontiguousarray(h[l, p].real), np.ascontiguousarray(h[l, p].imag)) for p in range(npt)] for l in range(nl)]
    Y = [(np.ascontiguousarray(y[p].real), np.ascontiguousarray(y[p].imag)) for p in range(npt)]
    Cm = [[(np.ascontiguousarray(c[:, p, q].real), np.ascontiguousarray(c[:, p, q].imag)) for q in range(npt)] for p in range(npt)]
    tx = F(tx)
    one = F(1)
    with np.errstate(all="ignore"):
        okc, rc, N = _ldl(Cm, npt)  # mmse_factor
        # mmse_prepare
        U = [_lower_mul(N, H[a]) for a in range(nl)]
        UW = [[(U[a][p][0] * rc[p], U[a][p][1] * rc[p]) for p in range(npt)] for a in range(nl)]
        t2 = tx * tx
        T = [[None] * nl for _ in range(nl)]
        A = [[None] * nl for _ in range(nl)]
        for j in range(nl):
            s = _norm(U[j][0]) * rc[0]
            for p in range(1, npt):
                s = s + _norm(U[j][p]) * rc[p]
            T[j][j] = (t2 * s, None)
            A[j][j] = (T[j][j][0] + one, None)
            for i in range(j + 1, nl):
                sij = _dot(U[i], UW[j])
                T[i][j] = A[i][j] = (t2 * sij[0], t2 * sij[1])
        oka, ra, M = _ldl(A, nl)
        ok = oka & okc
        B = [[None] * nl for _ in range(nl)]
        for a in range(nl):
            for b in range(a + 1):
                if a == b:
                    acc = ra[a]
                    for k in range(a + 1, nl):
                        acc = acc + _norm(M[k][a]) * ra[k]
                    B[a][a] = (acc, None)
                else:
                    acc = (M[a][b][0] * ra[a], M[a][b][1] * ra[a])
                    for k in range(a + 1, nl):
                        t = _cm(M[k][a], M[k][b])
                        acc = (acc[0] + t[0] * ra[k], acc[1] + t[1] * ra[k])
                    B[a][b] = acc
        sc, nv = [], []
        for a in range(nl):
            g = None
            for k in range(nl):
                hi, lo = max(k, a), min(k, a)
                t = B[a][a][0] * T[a][a][0] if k == a else B[hi][lo][0] * T[hi][lo][0] + B[hi][lo][1] * T[hi][lo][1]
                g = t if k == 0 else g + t
            ok = ok & _pos_normal(g)
            rg = one / g
            sc.append(tx * rg)
            nv.append(B[a][a][0] * rg)
        # mmse_apply
        V = _lower_mul(N, Y)
        m = [_dot(UW[a], V) for a in range(nl)]
        z = []
        for i in range(nl):
            acc = m[i]
            for j in range(i):
                acc = _add(acc, _mul(M[i][j], m[j]))
            z.append((acc[0] * ra[i], acc[1] * ra[i]))
        xo = np.zeros((nl, n), np.complex64)
        no = np.zeros((nl, n), F)
        ok = np.broadcast_to(ok, (n,))
        for a in range(nl):
            acc = z[a]
            for k in range(a + 1, nl):
                acc = _add(acc, _cm(M[k][a], z[k]))
            xo[a].real = np.where(ok, acc[0] * sc[a], F(0))
            xo[a].imag = np.where(ok, acc[1] * sc[a], F(0))
            no[a] = np.where(ok, nv[a], F(np.inf))
    return xo, no


# ------------------------------------------------------------------------------------------------ covariance from the DM-RS residuals
def nof_prg(nprb, prg):
    return -(-nprb // prg) if prg else 1


def covariance(est_case, prg=0, loading=0.0):
    """The estimator case of pusch_layers_estimator_cases (estimate(*est_case)) -> complex128 [PRG][P][P]: include/miphy.h above
    miphy_pusch_noise_covariance_batch. PRGs are counted over the allocated PRBs in ascending order."""
    mu, slot, type2, scr, nscid, scaling, sm, rb, first, nof, nl, g = est_case
    assert not type2
    g = np.asarray(g).astype(np.complex128)
    nports = g.shape[0]
    beta = float(scaling)
    prbs = np.nonzero(rb)[0]
    nprb, npil = prbs.size, prbs.size * 6
    dsyms = [l for l in range(first, first + nof) if sm[l]]
    nds = len(dsyms)
    gp = (prbs[:, None] * 6 + np.arange(6)[None, :]).reshape(-1)
    r = np.stack([E.gold_pilots(rb.size, slot, l, scr, nscid)[gp] for l in dsyms])  # [nds][np]
    par = np.where(np.arange(npil) % 2, -1.0, 1.0)
    per = prg if prg else nprb
    ng = nof_prg(nprb, prg)
    prg_of_pilot = (np.arange(npil) // 6) // per
    acc = np.zeros((ng, nports, nports), np.complex128)
    fitted_sum = 0
    for grp in range((nl + 1) // 2):
        pair = 2 * grp + 1 < nl
        sub = (prbs[:, None] * 12 + 2 * np.arange(6)[None, :] + grp).reshape(-1)
        resid = []
        for p in range(nports):
            x = np.stack([g[p, l, sub] for l in dsyms])
            z = (x * r.conj()).sum(0) / (nds * beta)
            if pair:
                s = [(z[0::2] + z[1::2]) / 2, (z[0::2] - z[1::2]) / 2]
                ma, mb = (np.repeat(v.reshape(nprb, 3).mean(1), 6) for v in s)
                resid.append(x - beta * r * (ma + par * mb)[None, :])
            else:
                resid.append(x - beta * r * np.repeat(z.reshape(nprb, 6).mean(1), 6)[None, :])
        resid = np.stack(resid)  # [P][nds][np]
        fitted_sum += 6 * nds - (2 if pair else 1)
        for j in range(ng):
            e = resid[:, :, prg_of_pilot == j].reshape(nports, -1)
            acc[j] += e @ e.conj().T
    for j in range(ng):
        n_j = min(per, nprb - j * per)
        low = np.tril(acc[j], -1)
        acc[j] = (low + low.conj().T + np.diag(np.real(np.diag(acc[j])))) / (n_j * fitted_sum)  # Hermitian to the bit, as the device writes it
        acc[j] +=loading * np.real(np.trace(acc[j])) / nports * np.eye(nports)
    return acc


def re_prg_index(c, prg):
    """PRG of every data element of the allocation c (codeword order): rank of its PRB among the allocated ones / prg."""
    _, sc = PL.data_positions(c)
    if not prg:
        return np.zeros(sc.size, int)
    rank = np.cumsum(PL.masks(c)[0]) - 1
    return rank[sc // 12] // prg


# ------------------------------------------------------------------------------------------------ interference
def interfered_tx(nl, npt, mod, tb_bytes, snr_db, dmrs, inr_db, seed=3):
    """chain_tx() plus a neighbour cell's user on the same PRBs: port signature a[p] ~ CN(0, 1) times the one-tap profile at delay 5, random QPSK
    on every element of all 14 symbols (DM-RS included), amplitude 10^(inr_db / 20). inr_db None: no interferer. -> chain_tx()'s tuple."""
    c, tb, grid, est = E.chain_tx(nl, npt, mod, tb_bytes, snr_db, dmrs, seed=seed)
    if inr_db is None:
        return c, tb, grid, est
    rng = np.random.default_rng(seed + 77)
    nsc = grid.shape[2]
    a = (rng.standard_normal(npt) + 1j * rng.standard_normal(npt)) / np.sqrt(2)
    q = ((1 - 2.0 * rng.integers(0, 2, (14, nsc))) + 1j * (1 - 2.0 * rng.integers(0, 2, (14, nsc)))) / np.sqrt(2)
    itf = 10 ** (inr_db / 20) * a[:, None, None] * E.profile(nsc, 5.0, taps=1)[None, None, :] * q[None, :, :]
    grid = grid.copy()
    grid[:npt] = (grid[:npt].astype(np.complex128) + itf).astype(np.complex64)
    est = est[:-1] + (grid[:npt],)
    return c, tb, grid, est


def mmse_on_allocation(c, grid, ce, cov, prg):
    """PL.extract() through mmse_single() at tx_scaling 1, every data element with the matrix of its PRG: cov complex64 [PRG][P][P].
    -> (x complex64 [L][n], nvar float32 [L][n])."""
    y, h = PL.extract(c, grid, ce)
    idx = re_prg_index(c, prg)
    x = np.zeros((c["nl"], y.shape[1]), np.complex64)
    nv = np.zeros((c["nl"], y.shape[1]), F)
    for j in np.unique(idx):
        sel = idx == j
        x[:, sel], nv[:, sel] = mmse_single(y[:, sel], h[:, :, sel], cov[j], 1.0)
    return x, nv


def irc_llr(c, grid, est, prg=0, loading=0.0):
    """The IRC host chain in front of the decoder, float32 where the device is: estimate() -> compact estimate, covariance() -> mmse_single()
    per PRG -> compose_llr()."""
    ce, _ = E.estimate(*est)
    cov = covariance(est, prg, loading).astype(np.complex64)
    c = dict(c, compact=True)
    return PL.compose_llr(c, *mmse_on_allocation(c, grid, ce[:, :, :1].astype(np.complex64), cov, prg))


# ------------------------------------------------------------------------------------------------ jobs of the library
def ncov_job(miphy, est_case, prg=0, loading=0.0, grid_off=0, cov_off=0, rx_ports=(0, 1, 2, 3)):
    """A PuschNcovJob record for an estimator case (the grid's ports in order unless rx_ports names others)."""
    mu, slot, t2, scr, nscid, scaling, sm, rb, first, nof, nl, g = est_case
    arr = np.zeros(1, dtype=miphy.PuschNcovJob)
    nj, j = arr[0], arr["base"]
    j["numerology"], j["slot_in_frame"], j["scrambling_id"], j["scaling"] = mu, slot, scr, scaling
    j["n_scid"], j["nof_tx_layers"], j["nof_rx_ports"], j["first_symbol"], j["nof_symbols"] = nscid, nl, g.shape[0], first, nof
    j["rx_ports"] = list(rx_ports)
    j["symbols_mask"] = sum(int(b) << l for l, b in enumerate(sm))
    j["grid_nof_prb"] = rb.size
    j["rb_mask"] = PL.mask_words(rb)
    j["grid_offset"] = grid_off
    nj["cov_offset"], nj["loading"], nj["prg_size"] = cov_off, loading, prg
    return nj


def equalizer_mmse_job(miphy, nre, npt, nl, tx, re_per_cov, y_off=0, h_off=0, c_off=0, z_off=0, nv_off=0):
    arr = np.zeros(1, dtype=miphy.EqualizerMmseJob)
    arr["base"][0] = PL.equalizer_job(miphy, nre, npt, nl, 0.0, tx, y_off, h_off, z_off, nv_off)
    arr[0]["cov_offset"], arr[0]["re_per_cov"] = c_off, re_per_cov
    return arr[0]


def demod_mmse_job(miphy, c, prg, grid_off=0, ce_off=0, cov_off=0, llr_off=0):
    arr = np.zeros(1, dtype=miphy.PuschDemodMmseJob)
    arr["base"][0] = PL.demod_job(miphy, c, grid_off, ce_off, 0, llr_off)
    arr[0]["cov_offset"], arr[0]["prg_size"] = cov_off, prg
    return arr[0]


# ------------------------------------------------------------------------------------------------ grid to bytes
INR_DB = 5.0
IRC_CASES = [  # (layers, ports, modulation, transport block bytes, SNR dB, DM-RS symbols): 24 PRB, interfered_tx() at INR_DB, seed 3
    (2, 4, 4, 1497, 20.0, (2, 7, 11)),
    (2, 4, 4, 1497, 20.0, (2, 11)),
    (1, 2, 4, 745, 20.0, (2, 7, 11)),
]
