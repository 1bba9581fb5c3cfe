"""Numpy restatement of the UCI short-block code of TS 38.212 (encoder 5.3.3.3, rate matching 5.4.3) and of the reference's
short-block detector (srsran::short_block_detector::detect, lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp:58-199):
the golden fixture pins it against the reference (tests/test_uci_short_block.py), the kernel of csrc/uci.hip is checked against it."""
import numpy as np

LLR_MAX, LLR_INFTY = 120, 127
# Detection thresholds of the GLRT, per number of message bits K = 1..11 (compared with a strict >).
THRESHOLDS = (0, 0, 12, 14, 16, 18, 20, 22, 24, 26, 29)
STATUS_VALID, STATUS_INVALID = 1, 2  # srsran::uci_status

# TS 38.212 Table 5.3.3.3-1: basis sequences M_{i,n} of the (32, K) code, one row per output bit i, columns n = 0..10.
_TS_TABLE = """
11000000001 11100000011 10010010111 10110000101 11110001001 11001011101 10101010111 10011001101 11011001011 10111010011 10100111011
11100110101 10010101111 11010101011 10001101001 11001111011 11101110010 10011100100 11011111000 10000110000 10100010001 11010000011
10001001101 11101000111 11111011110 11000111001 10110100110 11110101110 10101110100 10111111100 11111111111 10000000000
""".split()
BASIS = np.array([[int(ch) for ch in row] for row in _TS_TABLE], np.uint8)  # [32][11]
assert BASIS.shape == (32, 11)


def encode(msg, mod):
    """TS 38.212 5.3.3: K = 1..11 message bits -> N bits (N = Qm, 3 Qm or 32). Placeholders of the 1- / 2-bit codes are sent as
    the value they stand for at the modulator ('y' = repeat the previous bit, 'x' = 1); only the detector-relevant positions matter."""
    msg = np.asarray(msg, np.uint8)
    K = msg.size
    if K == 1:
        out = np.ones(mod, np.uint8)
        out[0] = msg[0]
        if mod > 1:
            out[1] = msg[0]
        return out
    if K == 2:
        c0, c1 = int(msg[0]), int(msg[1])
        c2 = c0 ^ c1
        if mod == 1:
            return np.array([c0, c1, c2], np.uint8)
        out = np.ones(3 * mod, np.uint8)
        out[0], out[1] = c0, c1
        out[mod], out[mod + 1] = c2, c0
        out[2 * mod], out[2 * mod + 1] = c1, c2
        return out
    return (BASIS[:, :K].astype(np.int64) @ msg.astype(np.int64) % 2).astype(np.uint8)


def rate_match(cw, E):
    """TS 38.212 5.4.3: e_k = d_{k mod N}."""
    return np.asarray(cw, np.uint8)[np.arange(E) % len(cw)]


def llr_add(a, b):
    """Saturating LLR sum (lib/phy/upper/log_likelihood_ratio.cpp:38-70): a == -b gives 0 (+inf + -inf included), +-127 is sticky,
    otherwise the sum is clamped to +-120."""
    if a == -b:
        return 0
    if abs(a) == LLR_INFTY:
        return a
    if abs(b) == LLR_INFTY:
        return b
    return max(-LLR_MAX, min(LLR_MAX, a + b))


def rate_dematch(llr, L):
    """tmp[i % L] += llr[i] for i = 0..E-1, in increasing i (the saturating sum is not associative)."""
    llr = np.asarray(llr, np.int64)
    tmp = [0] * L
    for i, v in enumerate(llr.tolist()):
        tmp[i % L] = llr_add(tmp[i % L], v)
    return np.array(tmp, np.int64)


def _codeword_masks():
    """Bit i of mask[idx] = bit i of the codeword of the even message 2 idx (message bit k = bit k of 2 idx)."""
    col = np.zeros(11, np.int64)
    for n in range(11):
        col[n] = sum(int(BASIS[i, n]) << i for i in range(32))
    masks = np.zeros(1024, np.int64)
    for idx in range(1024):
        m = 0
        for n in range(1, 11):
            if (2 * idx >> n) & 1:
                m ^= int(col[n])
        masks[idx] = m
    return masks


MASKS = _codeword_masks()
SIGNS = 1 - 2 * ((MASKS[:, None] >> np.arange(32)[None, :]) & 1)  # [1024][32], +1 / -1


def detect(llr, K, mod):
    """Returns (payload bits (uint8, K), status 1 = valid / 2 = invalid). Preconditions as the reference (validate_spans)."""
    E = len(llr)
    assert 1 <= K <= 11
    assert (E > K) if K > 2 else (E >= (mod if K == 1 else 3 * mod))
    if K == 1:
        t = rate_dematch(llr, mod)
        return np.array([0 if t[0] > 0 else 1], np.uint8), STATUS_VALID  # metric 1 > threshold 0
    if K == 2:
        t = rate_dematch(llr, 3 * mod)
        if mod == 1:
            x = t
        else:
            s = mod - 2  # in_size / 3 - 2
            x = np.array([t[0] + t[s + 3], t[1] + t[2 * s + 4], t[s + 2] + t[2 * s + 5]], np.int64)
        table = ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))
        best, idx = 0, 0  # the reference starts at DBL_MIN: an integer correlation wins only when >= 1
        for c in range(4):
            m = int(np.dot(x, table[c]))
            if m > best:
                best, idx = m, c
        norm = int(np.dot(x, x))
        metric = _div(2.0 * best * best, 3.0 * norm - best * best)
        bits = np.array([idx & 1, (idx >> 1) & 1], np.uint8)
    else:
        x = rate_dematch(llr, 32)
        corr = SIGNS[:1 << (K - 1)] @ x
        a = np.abs(corr)
        idx = int(np.argmax(a))  # first maximum
        best = int(a[idx])
        if best == 0:
            idx = 0
        bit0 = 1 if corr[idx] < 0 else 0
        v = 2 * idx + bit0
        bits = np.array([(v >> k) & 1 for k in range(K)], np.uint8)
        norm = int(np.dot(x, x))
        metric = _div(31.0 * best * best, 32.0 * norm - best * best)
    return bits, (STATUS_VALID if metric > THRESHOLDS[K - 1] else STATUS_INVALID)


def _div(num, den):
    """IEEE double division (0/0 = NaN, x/0 = inf) without numpy warnings."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(num) / np.float64(den))


def _llr_add_v(a, b):
    """llr_add on arrays."""
    s = np.clip(a + b, -LLR_MAX, LLR_MAX)
    s = np.where(np.abs(b) == LLR_INFTY, b, s)
    s = np.where(np.abs(a) == LLR_INFTY, a, s)
    return np.where(a == -b, 0, s)


def detect_batch(llr, K, mod, E, off):
    """detect() of many fields at once: field i reads llr[off[i] : off[i] + E[i]]. Returns (list of payload arrays, status array).
    Same arithmetic as detect(); the in-order fold runs over all fields of a dematching length together."""
    llr = np.asarray(llr, np.int64)
    K, mod, E, off = (np.asarray(v, np.int64) for v in (K, mod, E, off))
    n = K.size
    L = np.where(K == 1, mod, np.where(K == 2, 3 * mod, 32))
    bits = [None] * n
    status = np.zeros(n, np.uint8)
    for Lv in np.unique(L):
        sel = np.nonzero(L == Lv)[0]
        acc = np.zeros((sel.size, Lv), np.int64)
        lane = np.arange(Lv)
        for p in range(int((E[sel].max() + Lv - 1) // Lv)):
            pos = p * Lv + lane[None, :]
            live = pos < E[sel][:, None]
            v = llr[np.where(live, off[sel][:, None] + pos, 0)]
            acc = np.where(live, _llr_add_v(acc, v), acc)
        for j, i in enumerate(sel):
            t = acc[j]
            if K[i] <= 2:  # the dematched values are a valid input of length L, which dematches to itself
                bits[i], status[i] = detect(t, int(K[i]), int(mod[i]))
        big = sel[K[sel] >= 3]
        if big.size:
            X = acc[np.searchsorted(sel, big)]
            corr = X @ SIGNS.T  # [fields][1024]
            norm = (X * X).sum(axis=1)
            for j, i in enumerate(big):
                c = corr[j, :1 << (int(K[i]) - 1)]
                a = np.abs(c)
                idx = int(np.argmax(a))
                best = int(a[idx])
                if best == 0:
                    idx = 0
                v = 2 * idx + (1 if c[idx] < 0 else 0)
                bits[i] = ((v >> np.arange(int(K[i]))) & 1).astype(np.uint8)
                metric = _div(31.0 * best * best, 32.0 * int(norm[j]) - best * best)
                status[i] = STATUS_VALID if metric > THRESHOLDS[int(K[i]) - 1] else STATUS_INVALID
    return bits, status

