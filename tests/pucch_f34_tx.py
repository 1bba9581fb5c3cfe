"""PUCCH formats 3 and 4 transmitter and channel, restated in numpy float64 from TS 38.211 6.3.2.6 (scrambling, QPSK or pi/2-BPSK,
block-wise spreading, transform precoding, mapping) and 6.4.1.3.3 (DM-RS), normal cyclic prefix, no group or sequence hopping, with the
payload coding of tests/uci_short_block.py (3..11 bits) and tests/uci_polar.py (12 bits and more). The 23.5 reference neither sends nor
receives these formats; miphy_pucch_process_f34_batch is checked against this transmitter composed with tests/pucch_f34_ref.py.

A PDU is a dict: fmt (3 / 4), numerology, slot, nports, start, nsym, hop (0 / 1), bwp_start, bwp_size, prb, prb2, nprb, pi2 (0 / 1),
add (additional DM-RS, 0 / 1), occ_len, occ_idx, nid_hop, nid_scr, rnti, grid_nprb. Bits are in pucch_uci_message order."""
import cmath
import math

import numpy as np

import pucch_tx as T
import pusch_tp_ref as TP
import uci_polar as UP
import uci_short_block as SB

# TS 38.211 Table 6.4.1.3.3.2-1: DM-RS symbols relative to the first symbol of the PUCCH, by PUCCH length.
DMRS = {4: (1,), 5: (0, 3), 6: (1, 4), 7: (1, 4), 8: (1, 5), 9: (1, 6), 10: (2, 7), 11: (2, 7), 12: (2, 8), 13: (2, 9), 14: (3, 10)}
DMRS_LENGTH4_HOPPING = (0, 2)
DMRS_ADDITIONAL = {10: (1, 3, 6, 8), 11: (1, 3, 6, 9), 12: (1, 4, 7, 10), 13: (1, 4, 7, 11), 14: (1, 5, 8, 12)}
F3_NPRB = (1, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16)  # 2 PRBs need the length-24 sequences, which this repository does not hold
M0 = {2: (0, 6), 4: (0, 6, 3, 9)}  # cyclic shift of the DM-RS of format 4 by orthogonal sequence index (Table 6.4.1.3.3.1-1)


def dmrs_offsets(nsym, hop, add):
    if nsym == 4:
        return DMRS_LENGTH4_HOPPING if hop else DMRS[4]
    return DMRS_ADDITIONAL[nsym] if add and nsym >= 10 else DMRS[nsym]


def layout(nsym, hop, add):
    """(DM-RS offsets per hop, data offsets per hop); the second hop is empty without hopping."""
    dm = dmrs_offsets(nsym, hop, add)
    split = nsym // 2 if hop else nsym
    dmrs = [[o for o in dm if o < split], [o for o in dm if o >= split]]
    data = [[o for o in range(nsym) if o not in dm and o < split], [o for o in range(nsym) if o not in dm and o >= split]]
    return dmrs, data


def occ_w(nsf, n):
    """w_n(k), k < 12, of the block-wise spreading of format 4 (Tables 6.3.2.6.3-1 and -2)."""
    g = {2: (1, -1), 4: (1, -1j, -1, 1j)}[nsf][n]
    return np.array([g ** (k * nsf // 12) for k in range(12)], np.complex128)


def per_symbol(p):
    """Modulation symbols of one data OFDM symbol."""
    return 12 // p["occ_len"] if p["fmt"] == 4 else 12 * p["nprb"]


def nof_soft_bits(p):
    _, data = layout(p["nsym"], p["hop"], p["add"])
    return (1 if p["pi2"] else 2) * per_symbol(p) * (len(data[0]) + len(data[1]))


def scrambling(p, E):
    return T.gold(p["rnti"] * 2 ** 15 + p["nid_scr"], E)


def coded_bits(p, bits):
    """The E scrambled bits of one PDU, as they are modulated."""
    E, K = nof_soft_bits(p), len(bits)
    b = np.asarray(bits, np.uint8)
    cw = SB.rate_match(SB.encode(b, 1 if p["pi2"] else 2), E) if K <= 11 else UP.encode(K, E, b)
    return cw ^ scrambling(p, E)


def modulate(b, pi2):
    b = np.asarray(b, np.float64)
    if pi2:  # TS 38.211 5.1.1
        i = np.arange(b.size)
        return np.exp(0.5j * np.pi * (i % 2)) * ((1 - 2 * b) + 1j * (1 - 2 * b)) / np.sqrt(2)
    return ((1 - 2 * b[0::2]) + 1j * (1 - 2 * b[1::2])) / np.sqrt(2)


def dmrs_sequence(p, l):
    """r(n), n < 12 nof_prb, of the DM-RS on symbol l of the slot."""
    M = 12 * p["nprb"]
    m0 = M0[p["occ_len"]][p["occ_idx"]] if p["fmt"] == 4 else 0
    a = T.alpha_index(p["nid_hop"], p["slot"], l, m0)
    return np.exp(2j * np.pi * a * np.arange(M) / 12) * TP.low_papr(p["nid_hop"] % 30, 0, M)


def hop_prbs(p):
    return [p["bwp_start"] + p["prb"], p["bwp_start"] + (p["prb2"] if p["hop"] else p["prb"])]


def pdu_symbols(p, bits):
    """Transmitted REs of one PDU: list of (symbol, subcarrier array, values)."""
    M = 12 * p["nprb"]
    dmrs, data = layout(p["nsym"], p["hop"], p["add"])
    d = modulate(coded_bits(p, bits), p["pi2"])
    per = per_symbol(p)
    prb = hop_prbs(p)
    out, r = [], 0
    for o in range(p["nsym"]):
        h = int(o in dmrs[1] or o in data[1])
        sc = 12 * prb[h] + np.arange(M)
        if o in dmrs[h]:
            out.append((p["start"] + o, sc, dmrs_sequence(p, p["start"] + o)))
            continue
        y = d[r * per:(r + 1) * per]
        if p["fmt"] == 4:
            y = occ_w(p["occ_len"], p["occ_idx"]) * y[np.arange(12) % per]
        out.append((p["start"] + o, sc, np.fft.fft(y) / np.sqrt(M)))
        r += 1
    return out


def build_grid(seed, nports, grid_nprb, noise_std, pdus, bits, tx_on=None):
    """The received grid of PDUs that share a slot, as pucch_tx.build_grid makes it: every transmitting PDU goes through its own complex
    gain per port and delay ramp, then AWGN of standard deviation noise_std. Deterministic in `seed` (numpy PCG64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nsc = 12 * grid_nprb
    grid = np.zeros((nports, 14, nsc), np.complex128)
    for i, (p, b) in enumerate(zip(pdus, bits)):
        gain = (rng.standard_normal(nports) + 1j * rng.standard_normal(nports)) / np.sqrt(2)
        delay = rng.uniform(-0.004, 0.004)  # cycles per subcarrier: up to about +-16 taps of the 4096-point IDFT
        if tx_on is not None and not tx_on[i]:
            continue
        h = gain[:, None] * np.array([cmath.exp(-2j * math.pi * delay * kk) for kk in range(nsc)])[None, :]
        for l, sc, v in pdu_symbols(p, b):
            grid[:, l, sc] += h[:, sc] * v[None, :]
    noise = (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * (noise_std / np.sqrt(2))
    return (grid + noise).astype(np.complex64)


def pdu(fmt, nsym, nprb=1, hop=0, add=0, pi2=0, occ_len=0, occ_idx=0, nports=1, start=None, prb=0, prb2=None, grid_nprb=52, slot=3, numerology=1,
        nid_hop=0, nid_scr=0, rnti=1):
    """A PDU whose BWP is the whole grid; without `start` the allocation ends with the slot."""
    return dict(fmt=fmt, numerology=numerology, slot=slot, nports=nports, start=14 - nsym if start is None else start, nsym=nsym, hop=hop,
                bwp_start=0, bwp_size=grid_nprb, prb=prb, prb2=prb if prb2 is None else prb2, nprb=nprb, pi2=pi2, add=add, occ_len=occ_len,
                occ_idx=occ_idx, nid_hop=nid_hop, nid_scr=nid_scr, rnti=rnti, grid_nprb=grid_nprb)


def split_counts(K):
    """(HARQ-ACK, SR, CSI part 1) bit counts of a K-bit payload."""
    return (min(K, 2), 1 if K > 3 else 0, K - min(K, 2) - (1 if K > 3 else 0))


def job_of(p, K, grid_offset=0, payload_offset=0, llr_offset=0, est_offset=0):
    """The miphy.PucchF34Job record of a PDU carrying K bits."""
    import miphy
    j = np.zeros(1, miphy.PucchF34Job)[0]
    j["format"], j["numerology"], j["slot"], j["nof_ports"] = p["fmt"], p["numerology"], p["slot"], p["nports"]
    j["start_symbol"], j["nof_symbols"], j["intra_slot_hopping"] = p["start"], p["nsym"], p["hop"]
    j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"], j["second_hop_prb"] = p["bwp_start"], p["bwp_size"], p["prb"], p["prb2"]
    j["nof_prb"], j["pi2_bpsk"], j["additional_dmrs"], j["occ_length"], j["occ_index"] = p["nprb"], p["pi2"], p["add"], p["occ_len"], p["occ_idx"]
    j["nof_harq_ack"], j["nof_sr"], j["nof_csi_part1"] = split_counts(K)
    j["n_id_hopping"], j["n_id_scrambling"], j["rnti"], j["grid_nprb"] = p["nid_hop"], p["nid_scr"], p["rnti"], p["grid_nprb"]
    j["grid_offset"], j["payload_offset"], j["llr_offset"], j["est_offset"] = grid_offset, payload_offset, llr_offset, est_offset
    return j
