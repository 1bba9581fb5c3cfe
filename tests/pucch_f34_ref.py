"""Receiver of PUCCH formats 3 and 4 restated in numpy float64, step by step as the issue of the device processor states it: per receive
port and hop a least-squares estimate over the hop's DM-RS symbols (all 12 REs of a PRB are DM-RS: averaging window 12, no interpolation),
for format 4 averaged over aligned blocks of occ_len subcarriers, EPRE, RSRP, noise against the per-PRB mean (forced to EPRE / 1000 with
fewer than three DM-RS symbols or with hopping), time alignment from the +-144 taps of the 4096-point IDFT; zero forcing 1 x N with the
noise variance of the first port, the de-precoding IDFT, format-4 despreading, soft demapping (QPSK, pi/2-BPSK) with the quantisation of
the PUSCH demodulator, descrambling; the short-block detector of tests/uci_short_block.py or the polar restatements. It looks at no device
code. PDUs are the dicts of tests/pucch_f34_tx.py."""
import numpy as np

import pucch_f34_tx as X
import uci_polar as UP
import uci_polar_list as UL
import uci_short_block as SB

DFT, HALF_CP = 4096, 144
QPSK_GAIN = 2 * np.sqrt(2)


def time_alignment_taps(h):
    """estimate_time_alignment: the first maximum of |IDFT_4096| over taps [0, 144) against the first over the last 144 taps."""
    t = np.abs(np.fft.ifft(h, DFT)) ** 2
    d, a = t[:HALF_CP], t[DFT - HALF_CP:]
    if d.max() >= a.max():
        return float(np.argmax(d))
    return -float(HALF_CP - np.argmax(a))


def estimate(p, grid):
    """(h [port][hop][M] complex128, noise variance [port], dict of the CSI: epre_db, rsrp_db, sinr_db, time_alignment_s)."""
    grid = np.asarray(grid, np.complex128)
    M, nports, nh = 12 * p["nprb"], p["nports"], 2 if p["hop"] else 1
    dmrs, _ = X.layout(p["nsym"], p["hop"], p["add"])
    ndm_all = len(dmrs[0]) + len(dmrs[1])
    prb = X.hop_prbs(p)
    occ = p["occ_len"] if p["fmt"] == 4 else 1
    h = np.zeros((nports, nh, M), np.complex128)
    nvar, sums = np.zeros(nports), np.zeros(4)
    for port in range(nports):
        epre = rsrp = noise = ta = 0.0
        for hop in range(nh):
            sc = 12 * prb[hop] + np.arange(M)
            x = np.array([grid[port, p["start"] + o, sc] for o in dmrs[hop]])
            r = np.array([X.dmrs_sequence(p, p["start"] + o) for o in dmrs[hop]])
            s = (x * r.conj()).sum(axis=0)
            epre += (np.abs(x) ** 2).sum()
            if occ > 1:
                s = np.repeat(s.reshape(-1, occ).mean(axis=1), occ)
            rsrp += (np.abs(s) ** 2).sum() / len(x)
            h[port, hop] = s / len(x)
            avg = np.repeat(h[port, hop].reshape(-1, 12).mean(axis=1), 12)
            noise += sum((np.abs(x[i] - avg * r[i]) ** 2).sum() / M * 12 for i in range(len(x)))
            ta += time_alignment_taps(h[port, hop])
        epre, rsrp = epre / (M * ndm_all), rsrp / (M * ndm_all)
        noise /= 12 * ndm_all - 1
        if ndm_all < 3 or p["hop"]:
            noise = 0.001 * epre
        nvar[port] = noise
        ta = (ta / nh) / (DFT * (15 << p["numerology"]) * 1000.0)
        sums += (epre, rsrp, rsrp / noise if noise != 0 else 1000.0, ta)
    sums /= nports
    return h, nvar, dict(epre_db=10 * np.log10(sums[0]), rsrp_db=10 * np.log10(sums[1]), sinr_db=10 * np.log10(sums[2]), time_alignment_s=sums[3])


def despread(y, p):
    """The 12 / occ_len symbols of one de-precoded format-4 symbol: d(j) = (((t_0 + t_1) + t_2) + t_3) / occ_len. Keeps the dtype of y."""
    nsf, per = p["occ_len"], 12 // p["occ_len"]
    w = X.occ_w(nsf, p["occ_idx"]).conj().astype(y.dtype)
    d = w[:per] * y[:per]
    for q in range(1, nsf):
        d = d + w[q * per:(q + 1) * per] * y[q * per:(q + 1) * per]
    return d / y.real.dtype.type(nsf)


def equalised_symbols(p, grid, h, noise0):
    """(modulation symbols in transmission order, one noise variance per symbol)."""
    grid = np.asarray(grid, np.complex128)
    M = 12 * p["nprb"]
    _, data = X.layout(p["nsym"], p["hop"], p["add"])
    prb = X.hop_prbs(p)
    syms, var = [], []
    for o in range(p["nsym"]):
        hop = int(o in data[1])
        if o not in data[hop]:
            continue
        y = grid[:p["nports"], p["start"] + o, 12 * prb[hop]:12 * prb[hop] + M]
        hh = h[:, hop]
        den = (np.abs(hh) ** 2).sum(axis=0)
        z = np.fft.ifft((y * hh.conj()).sum(axis=0) / den) * np.sqrt(M)
        v = (noise0 / den).mean()
        if p["fmt"] == 4:
            z, v = despread(z, p), v / p["occ_len"]
        syms.append(z)
        var.append(np.full(z.size, v))
    return np.concatenate(syms), np.concatenate(var)


def demap(sym, var, pi2):
    """int8 soft bits: the max-log LLR in the range +-24 quantised to +-120 (round to nearest even; pi/2-BPSK: half away from zero)."""
    if pi2:
        odd = np.arange(sym.size) % 2 == 1
        a, b = np.where(odd, sym.imag, sym.real), np.where(odd, -sym.real, sym.imag)
        v = np.clip(QPSK_GAIN * (a + b) / var, -24, 24) / 24 * 120
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int8)
    v = np.empty(2 * sym.size)
    v[0::2], v[1::2] = QPSK_GAIN * sym.real / var, QPSK_GAIN * sym.imag / var
    return np.rint(np.clip(v * 5, -120, 120)).astype(np.int8)


def soft_bits(p, grid, h, noise0):
    sym, var = equalised_symbols(p, grid, h, noise0)
    llr = demap(sym, var, p["pi2"]).astype(np.int16)
    return (llr * (1 - 2 * X.scrambling(p, llr.size).astype(np.int16))).astype(np.int8)


def decode(p, K, llr, list_size=1):
    """(payload bits, status) of the soft bits of a K-bit PDU: the short-block restatement, or the polar ones at the list size."""
    if K <= 11:
        bits, status = SB.detect(np.asarray(llr, np.int8), K, 1 if p["pi2"] else 2)
        return np.asarray(bits, np.uint8), int(status)
    bits, valid = UP.decode(K, len(llr), llr) if list_size == 1 else UL.decode(K, len(llr), llr, list_size)
    return bits, UP.STATUS_VALID if valid else UP.STATUS_INVALID


def receive(p, grid, K, list_size=1):
    """dict(h, noise, csi, llr, bits, status) of one PDU on its grid [port][14][12 grid_nprb]."""
    h, nvar, csi = estimate(p, grid)
    llr = soft_bits(p, grid, h, nvar[0])
    bits, status = decode(p, K, llr, list_size)
    return dict(h=h, noise=nvar, csi=csi, llr=llr, bits=bits, status=status)
