"""Which (wavefront, layer) pairs of the packed LDPC decoder have saturated rows, from soft bits at iteration boundaries (the oracle's,
o_ldpc_decode with want_soft). Shared by tests/test_ldpc_saturated_rows*.py and tools/ldpc_saturation_profile.py; BG1 and even Z only.
Lane l of a codeblock owns check rows l and l + Z / 2 of every layer, wavefront w the lanes 64 w .. 64 w + 63; row r reads, on an edge
with shift s and column c, the soft bit ((r + s) mod Z) + c Z."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_BASE = (2, 3, 5, 7, 9, 11, 13, 15)  # TS 38.212 Table 5.3.2-1: Z = a * 2^j


@functools.lru_cache(maxsize=None)
def bg1_tables():
    """(row_start, column per edge, shift[set][edge]) of base graph 1, read from the generated table header of the library."""
    txt = open(os.path.join(ROOT, "srsran_project_23.5_amd", "csrc", "tables", "nr_ldpc_tables.h")).read()

    def array(name):
        body = re.search(r"\b%s(?:\[\d+\])+ = \{(.*?)\};" % name, txt, re.S).group(1)
        return np.array([int(v) for v in re.findall(r"\d+", body)])

    rs, col = array("NR_LDPC_BG1_ROW_START"), array("NR_LDPC_BG1_COL")
    return rs, col, array("NR_LDPC_BG1_SHIFT").reshape(8, col.size)


def lifting_set(Z):
    return max(i for i, a in enumerate(SET_BASE) if Z % a == 0 and ((Z // a) & (Z // a - 1)) == 0)


def infinite(soft):
    return np.abs(soft.astype(np.int32)) > 120


@functools.lru_cache(maxsize=None)
def row_reads(Z, layers):
    """Per layer the soft-bit positions its check rows read, [row, edge]."""
    rs, col, shift = bg1_tables()
    out = []
    for m in range(layers):
        e = np.arange(rs[m], rs[m + 1])
        sh, c = shift[lifting_set(Z)][e] % Z, col[e]
        out.append((np.arange(Z)[:, None] + sh[None, :]) % Z + c[None, :] * Z)
    return out


def nof_waves(Z):
    return (Z // 2 + 63) // 64


def wave_rows(Z, w):
    assert Z % 2 == 0
    lanes = np.arange(64 * w, min(64 * w + 64, Z // 2))
    return np.concatenate([lanes, lanes + Z // 2])


def saturated_from(snaps, Z, layers):
    """snaps[k] = the 68 Z soft bits at the START of iteration k (k = 0: two zero columns, then the decoder's input) ->
    {(wavefront, layer): first k whose snapshot shows only infinite soft bits on the pair's rows, or None}. The pair is saturated at its
    visit of iteration k at the latest (the layers before it in iteration k - 1 may have finished the job) and left out from k + 1 on."""
    reads, out = row_reads(Z, layers), {}
    for w in range(nof_waves(Z)):
        for m in range(layers):
            pos = reads[m][wave_rows(Z, w)].ravel()
            k0 = [k for k, s in enumerate(snaps) if infinite(s[pos]).all()]
            out[(w, m)] = k0[0] if k0 else None
    return out


def left_out(sat, max_iter):
    """{pair: visits left out at least} of saturated_from's result for a decode of max_iter iterations."""
    return {p: (max_iter - 1 - k if k is not None else 0) for p, k in sat.items()}


def dead_below_live(sat, max_iter):
    """Iterations (< max_iter) in which some wavefront leaves out a layer and runs a HIGHER one behind it -- the address-table instance
    then requests quads across a set bit -- as [(iteration, wavefront, dead layer, live layer)]; from the lower bounds of saturated_from,
    so a pair counts as dead in iteration k only if it was saturated by the start of k - 1, and as live only if not saturated at the start of k
    AND not of any later iteration before the end (it runs to the last iteration for certain)."""
    out = []
    for k in range(1, max_iter):
        for (w, m), km in sat.items():
            if km is None or km + 1 > k:
                continue
            for (w2, m2), k2 in sat.items():
                if w2 == w and m2 > m and k2 is None:
                    out.append((k, w, m, m2))
    return out
