"""Restatement of the framing of polar-coded UCI fields (TS 38.212 5.2.1, 5.3.1, 6.3.1.2-6.3.1.5, 6.3.2) around the oracle's polar
chains (o_polar_encode_chain / o_polar_decode_chain, nMax = 10, ibil = 1) and its CRC (o_crc_bits with CRC6 / CRC11). The 23.5
reference decodes no UCI field above 11 bits; the kernel of csrc/uci_polar.hip is checked against this composition."""
import numpy as np

import oracle_lib as ol

MIN_BITS, MAX_BITS, E_MAX = 12, 1706, 8192
STATUS_VALID, STATUS_INVALID = 1, 2  # srsran::uci_status


def _ceil_log2(x):
    return int(x - 1).bit_length()


def info(A, E):
    """dict(C, L, K_r, E_r, n, nPC) plus A_seg and pad of a field of A bits in E soft bits, or None where a rule refuses it."""
    if A < MIN_BITS or A > MAX_BITS:
        return None
    C = 2 if (A >= 360 and E >= 1088) or A >= 1013 else 1
    L = 6 if A <= 19 else 11
    A_seg = -(-A // C)
    K_r, E_r = A_seg + L, E // C
    nPC = 3 if K_r <= 25 else 0
    if not K_r + nPC < E_r or E_r > E_MAX:
        return None
    # TS 38.212 5.3.1: n = max(min(n1, n2, nMax), 5)
    e = _ceil_log2(E_r)
    n1 = e - 1 if (8 * E_r <= 9 * 2 ** (e - 1) and 16 * K_r < 9 * E_r) else e
    n = max(min(n1, _ceil_log2(K_r) + 3, 10), 5)
    return dict(C=C, L=L, K_r=K_r, E_r=E_r, n=n, nPC=nPC, A_seg=A_seg, pad=A_seg * C - A)


def _crc(L, bits):
    v = ol.o_crc_bits(ol.CRC6 if L == 6 else ol.CRC11, bits)
    return np.array([(v >> (L - 1 - i)) & 1 for i in range(L)], np.uint8)


def encode(A, E, bits):
    """The E rate-matched bits of a field (an unowned last bit is zero)."""
    f = info(A, E)
    assert f is not None
    a = np.concatenate([np.zeros(f["pad"], np.uint8), np.asarray(bits, np.uint8)])
    out = np.zeros(E, np.uint8)
    for r in range(f["C"]):
        seg = a[r * f["A_seg"]:(r + 1) * f["A_seg"]]
        cw = ol.o_polar_encode_chain(f["K_r"], f["E_r"], 10, 1, np.concatenate([seg, _crc(f["L"], seg)]))[0]
        out[r * f["E_r"]:(r + 1) * f["E_r"]] = cw
    return out


def decode(A, E, llr):
    """(payload bits (uint8, A), valid) of E soft bits; the payload is what the decoder found whatever the verdict."""
    f = info(A, E)
    assert f is not None and len(llr) == E
    llr = np.asarray(llr, np.int8)
    segs, valid = [], True
    for r in range(f["C"]):
        msg = ol.o_polar_decode_chain(f["K_r"], f["E_r"], 10, 1, llr[r * f["E_r"]:(r + 1) * f["E_r"]])[0]
        seg = msg[:f["A_seg"]]
        valid = valid and bool(np.array_equal(_crc(f["L"], seg), msg[f["A_seg"]:]))
        segs.append(seg)
    return np.concatenate(segs)[f["pad"]:].astype(np.uint8), valid


def min_E(A):
    """The smallest accepted number of soft bits of a field of A bits."""
    C = 2 if A >= 1013 else 1  # below 1013 bits the second segment needs E >= 1088, more than one segment's minimum
    L = 6 if A <= 19 else 11
    E = C * (-(-A // C) + L + (3 if A <= 19 else 0) + 1)
    assert info(A, E) is not None and info(A, E - 1) is None, (A, E)
    return E
