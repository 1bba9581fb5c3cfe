"""PUSCH with transform precoding (DFT-s-OFDM), restated in numpy float64 from TS 38.211: the low-PAPR sequences of 5.2.2, the DM-RS
sequence and its group / sequence hopping of 6.4.1.1.1.2, and a receiver (least-squares DM-RS estimate, MRC, the de-precoding IDFT of
6.3.1.4 read backwards, one noise variance per symbol) in front of the oracle's soft demapper, demultiplexer and decoder. The 23.5 reference
has no transform precoding, so this file -- not a reference build -- is what the device blocks are compared with. No device code is involved."""
import numpy as np

import oracle_lib as O
import pucch_tx

DMRS_BETA = 10 ** (3 / 20)  # two CDM groups without data: the DM-RS is 3 dB above the data


def tp_sizes():
    """The PRB counts transform precoding allows up to 270: 2^a 3^b 5^c (TS 38.211 6.3.1.4). 53 of them."""
    out = []
    for n in range(1, 271):
        m = n
        for f in (2, 3, 5):
            while m % f == 0:
                m //= f
        if m == 1:
            out.append(n)
    return out


def largest_prime_below(n):
    for c in range(n - 1, 1, -1):
        if all(c % d for d in range(2, int(c ** 0.5) + 1)):
            return c
    raise ValueError(n)


def low_papr(u, v, length):
    """r_{u,v}(n), alpha = 0, n < length (TS 38.211 5.2.2), complex128. Lengths 12, 30 and 6 N >= 36; 6, 18 and 24 need tables this
    repository does not hold."""
    u, v, length = int(u), int(v), int(length)
    assert 0 <= u < 30 and v in (0, 1)
    if length == 12:  # (no v below length 36)
        return np.exp(1j * np.pi * pucch_tx.PHI12[u].astype(np.float64) / 4)
    if length == 30:
        n = np.arange(30)
        return np.exp(-1j * np.pi * (((u + 1) * (n + 1) * (n + 2)) % 62) / 31)
    assert length >= 36 and length % 6 == 0, length
    nzc = largest_prime_below(length)
    q = (2 * nzc * (u + 1) + 31) // 62 + v * (-1) ** ((2 * nzc * (u + 1)) // 31)
    m = np.arange(length, dtype=np.int64) % nzc
    return np.exp(-1j * np.pi * ((q * m * (m + 1)) % (2 * nzc)) / nzc)  # the phase reduced in integers: q m (m+1) reaches 4e9


def dmrs_uv(n_id_rs, hopping, slot, l, length):
    """(u, v) of DM-RS symbol l of slot `slot` of the frame (TS 38.211 6.4.1.1.1.2). hopping: 0 neither, 1 group, 2 sequence."""
    f_gh = v = 0
    if hopping == 1:
        c = pucch_tx.gold(n_id_rs // 30, 8 * (14 * slot + l) + 8)
        f_gh = int(sum(int(c[8 * (14 * slot + l) + m]) << m for m in range(8))) % 30
    elif hopping == 2 and length >= 72:
        v = int(pucch_tx.gold(n_id_rs, 14 * slot + l + 1)[14 * slot + l])
    return (f_gh + n_id_rs) % 30, v


def dmrs_pilots(n_id_rs, hopping, slot, dmrs_symbols, nprb):
    """[DM-RS symbol][6 nprb] complex128."""
    return np.array([low_papr(*dmrs_uv(n_id_rs, hopping, slot, l, 6 * nprb), 6 * nprb) for l in dmrs_symbols])


def deprecode(x, v):
    """One symbol: x [M] equalised elements, v [M] their noise variances. y[n] = (1 / sqrt(M)) sum_k x[k] e^(+j 2 pi k n / M) with the elements
    that are not normal (variance not positive and finite) entered as 0, and the mean variance of the normal ones (+inf when there is none)."""
    x = np.asarray(x, np.complex128)
    v = np.asarray(v, np.float64)
    normal = np.isfinite(v) & (v > 0)
    y = np.fft.ifft(np.where(normal, x, 0)) * np.sqrt(x.size)
    return y, (v[normal].mean() if normal.any() else np.inf)


def receive(case, grid, rb, dm, uci=None):
    """The receiver on the ports case["ports"] of grid [4][14][nsc]. uci: None, or (demultiplexer case tuple, placeholders) of tests/oracle_lib.
    Returns dict(llr, ok, tb, streams)."""
    c = case
    g = np.asarray(grid, np.complex128)[list(c["ports"])]
    sub = np.nonzero(np.repeat(rb, 12))[0]
    nprb, M = int(rb.sum()), int(rb.sum()) * 12
    dsyms = [l for l in range(c["start"], c["start"] + c["nof"]) if dm[l]]
    data = [l for l in range(c["start"], c["start"] + c["nof"]) if not dm[l]]
    r = dmrs_pilots(c["scr"], c["hopping"], c["slot"], dsyms, nprb)
    # least squares on the even subcarriers, averaged over the DM-RS symbols, smoothed over three pilots for the noise, interpolated in between
    ls = np.stack([g[:, l, sub[0::2]] * np.conj(r[i]) / DMRS_BETA for i, l in enumerate(dsyms)], axis=1)  # [port][DM-RS symbol][6 nprb]
    h_p = ls.mean(axis=1)
    pad = np.concatenate([h_p[:, :1], h_p, h_p[:, -1:]], axis=1)
    smooth = (pad[:, :-2] + pad[:, 1:-1] + pad[:, 2:]) / 3
    nv = float(np.mean(np.abs(ls - smooth[:, None, :]) ** 2) * DMRS_BETA ** 2) * 1.5 + 1e-9  # (the smoothing removes a third of the noise power)
    k = np.arange(M)
    h = np.stack([np.interp(k, k[0::2], h_p[p].real) + 1j * np.interp(k, k[0::2], h_p[p].imag) for p in range(g.shape[0])])
    den = (np.abs(h) ** 2).sum(axis=0)
    ys, vs = [], []
    for l in data:
        y, v = deprecode((np.conj(h) * g[:, l, sub]).sum(axis=0) / den, nv / den)
        ys.append(y)
        vs.append(np.full(M, v))
    llr = O.o_demodulate_soft(c["mod"], np.concatenate(ys), np.concatenate(vs)).astype(np.int16)
    chips = O.o_gold((c["rnti"] << 15) + c["n_id"], 0, llr.size).astype(np.int16)
    sign = 1 - 2 * chips
    streams = None
    nof_sch = llr.size
    if uci is not None:
        ucase, ph = uci
        for re in ph:  # TS 38.211 6.3.1.1: y carries the chip of the bit before it, the x bits are not scrambled
            sign[re * c["mod"] + 1] = sign[re * c["mod"]]
            sign[re * c["mod"] + 2:(re + 1) * c["mod"]] = 1
    llr = (llr * sign).astype(np.int8)
    sch = llr
    if uci is not None:
        _, nof_sch, streams, _ = O.o_ulsch_demultiplex(*ucase, llr=llr)
        sch = streams[0]
    dec = O.OraclePuschDecoder(c["bg"], c["mod"], 0, 1, nof_sch // c["mod"], c["tbs"] // 8)
    ok, tb, _ = dec.decode(sch, 0, True, 6, True)
    return dict(llr=llr, ok=ok, tb=tb, streams=streams)
