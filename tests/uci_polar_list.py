"""Restatement of CRC-aided list decoding of polar-coded UCI fields (miphy_uci_polar_decode_list_batch): the framing of
tests/uci_polar.py, the survivors of tests/polar_scl_ref.py (pinned to the oracle's list decoder) on the oracle's dematched soft bits,
and the selection rule of include/miphy.h: per segment the survivor with the smallest (metric, slot) whose CRC11 checks, or the
smallest (metric, slot) overall where none does; the field is valid when every segment has a passing survivor. List size 1 and
fields of 12..19 bits are uci_polar.decode, the SSC chain."""
import functools

import numpy as np

import oracle_lib as ol
import polar_scl_ref as R
import uci_polar as U


@functools.lru_cache(maxsize=None)
def k_set(K, E):
    """The N information-set flags of the code (K, E, nMax = 10, ibil = 1): the allocation of an all-ones message."""
    return ol.o_polar_encode_chain(K, E, 10, 1, np.ones(K, np.uint8))[1].astype(bool)


def segment_survivors(K, E, llr, L):
    """[(metric, K bits in K-set order)] in slot order for the E soft bits of one segment."""
    ks = k_set(K, E)
    ch = ol.o_polar_decode_chain(K, E, 10, 1, llr)[1]
    return [(m, u[ks]) for m, u in R.survivors(ks, ch, L)]


def crc11_ok(bits):
    v = ol.o_crc_bits(ol.CRC11, bits[:-11])
    return all(int(bits[len(bits) - 11 + i]) == (v >> (10 - i)) & 1 for i in range(11))


def select(surv):
    """(slot of the chosen survivor, whether any survivor passes CRC11)."""
    ok = [q for q, (m, b) in enumerate(surv) if crc11_ok(b)]
    pool = ok if ok else range(len(surv))
    return min(pool, key=lambda q: (surv[q][0], q)), bool(ok)


def decode_ex(A, E, llr, L):
    """(payload, valid, per segment: True where the chosen survivor is not the best-metric one)."""
    f = U.info(A, E)
    assert f is not None and len(llr) == E and L in (1, 2, 4, 8)
    if L == 1 or A <= 19:
        payload, valid = U.decode(A, E, llr)
        return payload, valid, [False] * f["C"]
    assert f["L"] == 11 and f["nPC"] == 0
    llr = np.asarray(llr, np.int8)
    segs, valid, off_best = [], True, []
    for r in range(f["C"]):
        surv = segment_survivors(f["K_r"], f["E_r"], llr[r * f["E_r"]:(r + 1) * f["E_r"]], L)
        q, ok = select(surv)
        best = min(range(len(surv)), key=lambda p: (surv[p][0], p))
        off_best.append(q != best)
        valid = valid and ok
        segs.append(surv[q][1][:f["A_seg"]])
    return np.concatenate(segs)[f["pad"]:].astype(np.uint8), valid, off_best


def decode(A, E, llr, L):
    """(payload bits (uint8, A), valid) of E soft bits at list size L."""
    return decode_ex(A, E, llr, L)[:2]
