"""Restatement of the oracle's list decoder (orc_polar_scl_decode, oracle/phy_oracle.c) that returns EVERY survivor, which the oracle
does not: the oracle hands back one path, chosen by CRC24C or by metric, so it cannot say what a CRC11 selection among the survivors
must give. This module repeats its recursion on dematched soft bits and is pinned to it in tests/test_uci_polar_list.py: the best
survivor in CRC mode 0, and the oracle's pick among the survivors in CRC modes 1 and 2 (which is not always the best-metric one).

The rate-0 rule is the oracle's: an aligned all-frozen block [i, i + 2^r) is handled at stage r and costs the sum of its negative
stage-r soft bits. Under the saturating addition this is NOT the leaf-by-leaf sum (x = y = -100 costs 200 at the block's stage, and
0 + |sat(-200)| = 120 leaf by leaf), so the block rule is part of what is restated."""
import numpy as np

LLR_MAX = 120


def llr_add(a, b):
    """log_likelihood_ratio::operator+ as the oracle states it (llr_add): the right operand's special cases first."""
    t = np.clip(a + b, -LLR_MAX, LLR_MAX)
    t = np.where(np.abs(a) > LLR_MAX, a, t)
    t = np.where(np.abs(b) > LLR_MAX, b, t)
    return np.where(b == -a, 0, t)


def soft_xor(x, y):
    m = np.minimum(np.abs(x), np.abs(y))
    return np.where(x * y < 0, -m, m)


def rate0_exponents(k_set):
    """Per position the exponent r of the largest aligned all-frozen block [i, i + 2^r) starting there (0 at an information bit)."""
    N = len(k_set)
    n = N.bit_length() - 1
    out = np.zeros(N, np.int64)
    for i in range(N):
        r = 0
        if not k_set[i]:
            while r < n and i % (2 << r) == 0 and not k_set[i:i + (2 << r)].any():
                r += 1
        out[i] = r
    return out


def survivors(k_set, ch, L):
    """k_set: N flags (information and parity-check positions), ch: the N dematched soft bits, L: 1, 2, 4 or 8.
    Returns [(metric, u)] in slot order, u the N decisions of the path (take u[k_set != 0] for the bits in K-set order)."""
    k_set = np.asarray(k_set).astype(bool)
    N = k_set.size
    n = N.bit_length() - 1
    assert 1 << n == N and L in (1, 2, 4, 8)
    ch = np.asarray(ch, np.int64)
    rexp = rate0_exponents(k_set)
    # per path: llr (stage s at offset 2^s, s < n), bl (left partial sums of stage s at offset 2^s), u
    llr = np.zeros((1, N), np.int64)
    bl = np.zeros((1, N), np.int64)
    u = np.zeros((1, N), np.int64)
    pm = np.zeros(1, np.int64)
    i = 0
    while i < N:
        r = int(rexp[i])
        B = 1 << r
        t = n
        if i:
            t = (i & -i).bit_length() - 1
            sz = 1 << t
            up = np.broadcast_to(ch, (llr.shape[0], N)) if t + 1 == n else llr[:, 2 * sz:4 * sz]
            x, y = up[:, :sz], up[:, sz:2 * sz]
            llr[:, sz:2 * sz] = np.where(bl[:, sz:2 * sz] != 0, llr_add(y, -x), llr_add(y, x))
        for s in range(t - 1, r - 1, -1):
            sz = 1 << s
            up = np.broadcast_to(ch, (llr.shape[0], N)) if s + 1 == n else llr[:, 2 * sz:4 * sz]
            llr[:, sz:2 * sz] = soft_xor(up[:, :sz], up[:, sz:2 * sz])
        if not k_set[i]:
            v = np.broadcast_to(ch, (llr.shape[0], N)) if r == n else llr[:, B:2 * B]
            u[:, i:i + B] = 0
            pm = pm + np.where(v < 0, -v, 0).sum(axis=1)
        else:
            active = llr.shape[0]
            keep = min(2 * active, L)
            l0 = llr[:, 1]
            hard = (l0 <= 0).astype(np.int64)
            met = np.empty(2 * active, np.int64)
            bit = np.empty(2 * active, np.int64)
            met[0::2], bit[0::2] = pm, hard
            met[1::2], bit[1::2] = pm + np.abs(l0), 1 - hard
            order = np.argsort(met, kind="stable")[:keep]  # rank: smaller metric first, ties to the lower candidate index
            parent = order >> 1
            llr, bl, u = llr[parent].copy(), bl[parent].copy(), u[parent].copy()
            u[:, i] = bit[order]
            pm = met[order]
        if r < n:
            if not (i >> r) & 1:
                bl[:, B:2 * B] = u[:, i:i + B]
            else:
                cur = u[:, i:i + B].copy()
                sz, s = B, r
                while s < n and (i >> s) & 1:
                    cur = np.concatenate([cur ^ bl[:, sz:2 * sz], cur], axis=1)
                    sz, s = 2 * sz, s + 1
                if s < n:
                    bl[:, sz:2 * sz] = cur
        i += B
    return [(int(pm[q]), u[q].astype(np.uint8)) for q in range(llr.shape[0])]
