"""The soft-bit address table of the LDPC decoder (miphy_ldpc_address_table, include/miphy.h) against the addresses written down from the
base graph tables: lane l of a codeblock owns check rows l and l + ceil(Z / 2) of every layer, and the soft bit of row r on an edge with
cyclic shift s and column c lies at LDS byte ((r + s) mod Z) + c Z. Host code only: no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_BASE = (2, 3, 5, 7, 9, 11, 13, 15)  # TS 38.212 Table 5.3.2-1: Z = a * 2^j


def graph_tables():
    """{bg: (row_start, column per edge, shift[set][edge])} read from the generated table header of the library."""
    txt = open(os.path.join(ROOT, "srsran_project_23.5_amd", "csrc", "tables", "nr_ldpc_tables.h")).read()

    def array(name):
        body = re.search(r"\b%s(?:\[\d+\])+ = \{(.*?)\};" % name, txt, re.S).group(1)
        return np.array([int(v) for v in re.findall(r"\d+", body)])

    out = {}
    for bg in (1, 2):
        rs, col = array("NR_LDPC_BG%d_ROW_START" % bg), array("NR_LDPC_BG%d_COL" % bg)
        out[bg] = (rs, col, array("NR_LDPC_BG%d_SHIFT" % bg).reshape(8, col.size))
    return out


def lifting_set(Z):
    return max(i for i, a in enumerate(SET_BASE) if Z % a == 0 and ((Z // a) & (Z // a - 1)) == 0)


@pytest.fixture(scope="module")
def tables():
    return graph_tables()


@pytest.mark.parametrize("layers", [4, 6])
@pytest.mark.parametrize("Z", [128, 208, 256, 352, 384])
@pytest.mark.parametrize("bg", [1, 2])
def test_address_table_against_the_graph(tables, bg, Z, layers):
    import miphy
    lib = miphy.lib()
    rs, col, shift = tables[bg]
    H = (Z + 1) // 2
    lanes = 64 * ((H + 63) // 64)
    quads = [(int(rs[m + 1] - rs[m]) + 3) // 4 for m in range(layers)]
    words = lib.miphy_ldpc_address_table(bg, Z, layers, None)
    assert words == sum(quads) * lanes * 4
    buf = np.full(words + 8, 0xDEADBEEF, dtype=np.uint32)
    assert lib.miphy_ldpc_address_table(bg, Z, layers, buf.ctypes.data_as(C.c_void_p)) == words
    assert (buf[words:] == 0xDEADBEEF).all()  # nothing written behind the table
    got = buf[:words].reshape(sum(quads), lanes, 4)
    rows = np.arange(H)
    q0 = 0
    for m in range(layers):
        d = int(rs[m + 1] - rs[m])
        for j in range(4 * quads[m]):
            e = int(rs[m]) + min(j, d - 1)  # a pad entry repeats the last edge
            sh, c = int(shift[lifting_set(Z)][e]) % Z, int(col[e])
            a = (rows + sh) % Z + c * Z
            b = (rows + H + sh) % Z + c * Z
            w = got[q0 + j // 4, :, j % 4]
            assert np.array_equal(w[:H] & 0xffff, a), (m, j)
            assert np.array_equal(w[:H] >> 16, b), (m, j)
            assert (w[H:] == 0).all(), (m, j)  # lanes without rows
        q0 += quads[m]


def test_address_table_of_an_odd_lifting_size(tables):
    """Z = 15: the last lane owns row 7 twice (no row 15 exists)."""
    import miphy
    lib = miphy.lib()
    rs, col, shift = tables[2]
    Z, H = 15, 8
    words = lib.miphy_ldpc_address_table(2, Z, 4, None)
    buf = np.zeros(words, dtype=np.uint32)
    assert lib.miphy_ldpc_address_table(2, Z, 4, buf.ctypes.data_as(C.c_void_p)) == words
    got = buf.reshape(-1, 64, 4)
    sh, c = int(shift[lifting_set(Z)][0]) % Z, int(col[0])
    w = got[0, :H, 0]
    assert np.array_equal(w & 0xffff, (np.arange(H) + sh) % Z + c * Z)
    assert np.array_equal(w[:H - 1] >> 16, (np.arange(H - 1) + H + sh) % Z + c * Z)
    assert w[H - 1] >> 16 == w[H - 1] & 0xffff


def test_address_table_refuses_what_is_no_code():
    import miphy
    lib = miphy.lib()
    assert lib.miphy_ldpc_address_table(3, 384, 4, None) < 0
    assert lib.miphy_ldpc_address_table(1, 385, 4, None) < 0
    assert lib.miphy_ldpc_address_table(1, 384, 0, None) < 0
    assert lib.miphy_ldpc_address_table(2, 384, 43, None) < 0
