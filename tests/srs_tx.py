"""The sounding reference signal of TS 38.211 6.4.1.4.2-3 (normal cyclic prefix), restated in numpy float64: sequence group and number with group and
sequence hopping, cyclic shifts and comb offsets per transmit port, the mapping to the comb, and a transmitter that puts one or several UEs through a
per-PRG channel with a delay into one grid with noise. The 23.5 reference has no SRS code, so this file and tests/srs_ref.py -- not a reference build --
are what miphy_srs_pilots_batch and miphy_srs_estimate_batch are compared with. No device code is involved.

A UE (and the job that receives it) is a dict: R receive ports, nap transmit ports, start / nsym symbols of the slot, comb K with offset kbar, cyclic
shift ncs, nid, hopping (0 neither, 1 group, 2 sequence), prg PRBs per estimate, prb / nprb the allocation in grid numbering, slot, numerology and the
grid width grid_nprb."""
import numpy as np

import pucch_tx as T
import pusch_tp_ref as TP


def ue(R=1, nap=1, start=13, nsym=1, K=2, kbar=0, ncs=0, nid=0, hopping=0, prg=4, prb=0, nprb=4, slot=0, numerology=0, grid_nprb=None):
    return dict(R=R, nap=nap, start=start, nsym=nsym, K=K, kbar=kbar, ncs=ncs, nid=nid, hopping=hopping, prg=prg, prb=prb, nprb=nprb, slot=slot,
                numerology=numerology, grid_nprb=prb + nprb if grid_nprb is None else grid_nprb)


def derive(p):
    """What follows from a UE's parameters: M, Q, P, G, n_cs_max, per port the cyclic shift and the comb offset, and the combs in use as lists of
    ports (the lowest port first)."""
    K, nap = p["K"], p["nap"]
    ncs_max = 8 if K == 2 else 12
    split = nap == 4 and p["ncs"] >= ncs_max // 2
    cs = [(p["ncs"] + ncs_max * i // nap) % ncs_max for i in range(nap)]
    assert all((ncs_max * i) % nap == 0 for i in range(nap))
    off = [(p["kbar"] + K // 2) % K if split and i in (1, 3) else p["kbar"] for i in range(nap)]
    combs = [[0, 2], [1, 3]] if split else [list(range(nap))]
    return dict(M=12 * p["nprb"] // K, Q=12 * p["prg"] // K, P=len(combs[0]), G=p["nprb"] // p["prg"], ncs_max=ncs_max, cs=cs, off=off, combs=combs)


def uv(p, l_abs):
    """(u, v) of the symbol l_abs of the slot: c_init = n_id in both hopping modes."""
    M, base = derive(p)["M"], 14 * p["slot"] + l_abs
    f_gh = v = 0
    if p["hopping"] == 1:
        c = T.gold(p["nid"], 8 * base + 8)
        f_gh = sum(int(c[8 * base + m]) << m for m in range(8)) % 30
    elif p["hopping"] == 2 and M >= 72:
        v = int(T.gold(p["nid"], base + 1)[base])
    return (f_gh + p["nid"]) % 30, v


def port_sequence(p, l, i):
    """r_(u,v)(n) e^(j 2 pi n_cs,i n / n_cs_max), n < M, of symbol l of the resource and transmit port i; the shift's phase reduced in integers."""
    d = derive(p)
    n = np.arange(d["M"])
    return TP.low_papr(*uv(p, p["start"] + l), d["M"]) * np.exp(2j * np.pi * ((d["cs"][i] * n) % d["ncs_max"]) / d["ncs_max"])


def pilots(p):
    """[symbol][tx port][M] complex128: what miphy_srs_pilots_batch writes."""
    return np.array([[port_sequence(p, l, i) for i in range(p["nap"])] for l in range(p["nsym"])])


def subcarriers(p, i):
    """Grid subcarriers of the M elements of transmit port i."""
    d = derive(p)
    return 12 * p["prb"] + d["off"][i] + p["K"] * np.arange(d["M"])


def prg_channel(rng, p, spread=0.3):
    """[G][R][nap] complex128: one random matrix, scaled per PRG by a real gain in 1 +- spread. The channel is flat on every PRG and differs between
    them, and the products of neighbouring elements across a PRG border keep the phase of the delay alone, so a noise-free delay estimate is exact."""
    d = derive(p)
    h0 = (rng.standard_normal((p["R"], p["nap"])) + 1j * rng.standard_normal((p["R"], p["nap"]))) / np.sqrt(2)
    return (1 + spread * rng.uniform(-1, 1, d["G"]))[:, None, None] * h0[None]


def theta_of_delay(p, tau):
    """Phase slope in rad per subcarrier of a delay of tau seconds."""
    return -2 * np.pi * 15e3 * 2 ** p["numerology"] * tau


def add_ue(grid, p, Hg, theta=0.0):
    """Adds the UE's signal to grid [port][14][12 grid_nprb] (complex128): port i's element n through Hg[PRG of n][r][i] and the phase
    theta (k - 12 prb) of a delay at subcarrier k."""
    d = derive(p)
    for i in range(p["nap"]):
        k = subcarriers(p, i)
        g = np.arange(d["M"]) // d["Q"]
        for l in range(p["nsym"]):
            x = port_sequence(p, l, i) * np.exp(1j * theta * (k - 12 * p["prb"]))
            for r in range(p["R"]):
                grid[r, p["start"] + l, k] += Hg[g, r, i] * x


def centre_channel(p, Hg, theta):
    """[G][R][nap]: the channel at the centre of every PRG's elements on the port's comb, what the estimator's H approaches."""
    d = derive(p)
    out = np.array(Hg, np.complex128)
    for i in range(p["nap"]):
        kc = d["off"][i] + p["K"] * (np.arange(d["G"]) * d["Q"] + (d["Q"] - 1) / 2)
        out[:, :, i] *= np.exp(1j * theta * kc)[:, None]
    return out


def build_grid(seed, nports, grid_nprb, noise_std, ues, dtype=np.complex64):
    """Grid [port][14][12 grid_nprb] (complex64, as the device reads it): the UEs (p, Hg, theta) and complex noise of standard deviation noise_std per
    element."""
    rng = np.random.default_rng(seed)
    grid = np.zeros((nports, 14, 12 * grid_nprb), np.complex128)
    for p, Hg, theta in ues:
        assert p["R"] <= nports and p["prb"] + p["nprb"] <= grid_nprb
        add_ue(grid, p, Hg, theta)
    if noise_std:
        grid += noise_std * (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) / np.sqrt(2)
    return grid.astype(dtype)


def job_of(p, grid_offset=0, h_offset=0, pilots_offset=0):
    import miphy
    j = np.zeros(1, miphy.SrsJob)[0]
    j["numerology"], j["nof_rx_ports"], j["slot"], j["nof_tx_ports"], j["start_symbol"], j["nof_symbols"] = p["numerology"], p["R"], p["slot"], p["nap"], p["start"], p["nsym"]
    j["comb_size"], j["comb_offset"], j["cyclic_shift"], j["hopping"], j["prg_size"] = p["K"], p["kbar"], p["ncs"], p["hopping"], p["prg"]
    j["start_prb"], j["nof_prb"], j["n_id"], j["grid_nprb"] = p["prb"], p["nprb"], p["nid"], p["grid_nprb"]
    j["grid_offset"], j["h_offset"], j["pilots_offset"] = grid_offset, h_offset, pilots_offset
    return j
