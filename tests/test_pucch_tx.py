"""CPU: the PUCCH transmitter of tests/pucch_tx.py rebuilds every grid of tests/golden/pucch_processor.npz bit for bit, and the
low-PAPR table the kernel compiles in (csrc/tables/nr_low_papr_tables.h) equals the reference's recorded table."""
import os
import re

import numpy as np
import pytest

import pucch_tx as T

HERE = os.path.dirname(os.path.abspath(__file__))
FX = os.path.join(HERE, "golden", "pucch_processor.npz")
HDR = os.path.join(HERE, "..", "srsran_project_23.5_amd", "csrc", "tables", "nr_low_papr_tables.h")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FX))


def test_fixture_coverage(fx):
    cfg = fx["cfg"]
    f1, f2 = cfg[cfg[:, T.H_FMT] == 1], cfg[cfg[:, T.H_FMT] == 2]
    assert len(f1) >= 500 and len(f2) >= 500
    assert set(f1[:, T.H_NSYM]) == set(range(4, 15)) and set(f1[:, T.H_HOP]) == {0, 1}
    assert set(f1[:, T.H_ICS]) == set(range(12)) and set(f1[:, T.H_OCC]) == set(range(7))
    assert set(f2[:, T.H_NPRB]) == set(range(1, 17)) and set(f2[:, T.H_NSYM]) == {1, 2}
    k2 = f2[:, T.H_NHARQ] + f2[:, T.H_NSR] + f2[:, T.H_NCSI1]
    assert set(k2) == set(range(3, 12))
    assert set(cfg[:, T.H_NPORTS]) == {1, 2, 3, 4} and set(cfg[:, T.H_NUM]) == {0, 1} and (cfg[:, T.H_BWP_START] > 0).any()
    sizes = np.bincount(fx["group"])
    assert sizes.max() >= 12 and (sizes >= 2).sum() >= 30  # format-1 users sharing a PRB
    assert (fx["tx_on"] == 0).any() and (fx["g_noise"] == 0).any()
    for f in (1, 2):
        st = fx["status"][cfg[:, T.H_FMT] == f]
        assert (st == 1).any() and (st == 2).any()


def test_grids_rebuild_bit_exact(fx):
    grids = T.fixture_grids(fx)
    bad = [g for g, grid in enumerate(grids) if T.grid_hash(grid) != str(fx["g_sha256"][g])]
    assert not bad, "grids of groups %s differ from the ones the reference saw" % bad[:10]


def test_low_papr_table_matches_reference(fx):
    txt = open(HDR).read()
    body = txt[txt.index("NR_LOW_PAPR12"):]
    vals = np.array([float(v) for v in re.findall(r"[-+]?\d*\.?\d+(?:[eE][-+]?\d+)?(?=f)", body)], np.float64)
    assert vals.size == 30 * 12 * 12 * 2
    tab = (vals[0::2] + 1j * vals[1::2]).reshape(30, 12, 12)
    assert np.abs(tab - fx["low_papr"].astype(np.complex128)).max() < 1e-6
    assert np.abs(T.low_papr_table() - fx["low_papr"]).max() < 1e-6


def test_binding_layout_matches_header(tmp_path):
    """Every field offset of miphy.PucchJob / miphy.PucchResult against include/miphy.h, compiled with gcc."""
    import subprocess

    import miphy
    fields = [("miphy_pucch_job", miphy.PucchJob), ("miphy_pucch_result", miphy.PucchResult)]
    body = "".join('  printf("%%zu\\n", sizeof(%s));\n' % t + "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (t, f) for f in dt.names)
                   for t, dt in fields)
    src = tmp_path / "l.c"
    src.write_text('#include "miphy.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-I", os.path.join(HERE, "..", "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, dt in fields:
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert got == want
