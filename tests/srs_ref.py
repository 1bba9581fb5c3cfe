"""The SRS channel estimator of csrc/srs.hip restated in numpy float64: what miphy_srs_estimate_batch is compared with. No device code is involved.

Per comb c in use (one, or two when four ports split), n_ref the cyclic shift of its lowest port, P the ports on it, Q the comb elements per PRG:
  z_(r,l,c)[n] = y_r[l, 12 prb + c + K n] conj(r_(u_l,v_l)(n)) e^(-j 2 pi n_ref n / n_cs_max)
  C = sum_(r,l,c) sum_(n < M - P) z[n + P] conj(z[n]),  phi = atan2(Im C, Re C),  theta = phi / (K P),  time alignment = -theta / (2 pi delta_f)
  w[n] = z[n] e^(-j theta K n);  d_i = (n_cs,i - n_ref) mod n_cs_max;  PRG g holds the elements g Q .. (g + 1) Q - 1
  hhat_(r,i,g) = (1 / (L Q)) sum_l sum_n w[n] e^(-j 2 pi d_i n / n_cs_max);  H[g][r][i] = hhat e^(+j theta K (g Q + (Q - 1) / 2));  H_wb = mean_g hhat
  e[n] = w[n] - sum_(i on the comb) hhat_(r,i,g(n)) e^(+j 2 pi d_i n / n_cs_max);  noise_var = sum |e|^2 / (R |combs| (L M - G P))
  EPRE = mean |y|^2 over the SRS elements;  rsrp_i = mean_(r,g) |hhat|^2;  sinr = mean_i rsrp_i / noise_var."""
import numpy as np

import pusch_tp_ref as TP
import srs_tx as X


def max_delay(p):
    """The estimate is unambiguous for |delay| below this: 1 / (2 delta_f K P)."""
    return 1.0 / (2 * 15e3 * 2 ** p["numerology"] * p["K"] * X.derive(p)["P"])


def receive(p, grid):
    """grid: [port][14][12 grid_nprb] (any complex type; taken to complex128)."""
    d = X.derive(p)
    M, Q, P, G, K, R, L, nmax = d["M"], d["Q"], d["P"], d["G"], p["K"], p["R"], p["nsym"], d["ncs_max"]
    assert Q % P == 0 and M != 24
    n = np.arange(M)
    base = np.array([TP.low_papr(*X.uv(p, p["start"] + l), M) for l in range(L)])  # [l][n]
    y = np.asarray(grid, np.complex128)[:R, p["start"]:p["start"] + L]
    zs, C, epre = [], 0.0, 0.0
    for ports in d["combs"]:
        yc = y[:, :, X.subcarriers(p, ports[0])]  # [r][l][n]
        z = yc * np.conj(base)[None] * np.exp(-2j * np.pi * ((d["cs"][ports[0]] * n) % nmax) / nmax)
        zs.append(z)
        C = C + (z[:, :, P:] * np.conj(z[:, :, :-P])).sum()
        epre += (np.abs(yc) ** 2).sum()
    phi = float(np.angle(C)) if C != 0 else 0.0
    thetaK = phi / P  # theta K: rad per comb element
    hhat = np.zeros((G, R, p["nap"]), np.complex128)
    noise = 0.0
    for ports, z in zip(d["combs"], zs):
        w = (z * np.exp(-1j * thetaK * n)).reshape(R, L, G, Q)
        fit = np.zeros_like(w)
        for i in ports:
            rot = np.exp(2j * np.pi * ((((d["cs"][i] - d["cs"][ports[0]]) % nmax) * n) % nmax) / nmax).reshape(G, Q)
            hhat[:, :, i] = (w * np.conj(rot)[None, None]).mean(axis=(1, 3)).T
            fit += hhat[:, :, i].T[:, None, :, None] * rot[None, None]
        noise += (np.abs(w - fit) ** 2).sum()
    ncombs = len(d["combs"])
    noise_var = noise / (R * ncombs * (L * M - G * P))
    H = hhat * np.exp(1j * thetaK * (np.arange(G) * Q + (Q - 1) / 2))[:, None, None]
    rsrp = (np.abs(hhat) ** 2).mean(axis=(0, 1))
    h_wb = np.zeros((4, 4), np.complex128)
    h_wb[:R, :p["nap"]] = hhat.mean(axis=0)
    return dict(H=H, h_wb=h_wb, noise_var=noise_var, epre=epre / (R * ncombs * L * M), rsrp=rsrp, sinr=rsrp.mean() / noise_var if noise_var > 0 else np.inf,
                phi=phi, time_alignment_s=-(phi / (K * P)) / (2 * np.pi * 15e3 * 2 ** p["numerology"]))
