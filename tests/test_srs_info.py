"""CPU: miphy_srs_info through the binding, no device. What the library derives from an SRS job -- M, Q, P, G, cyclic shift and comb offset per transmit
port, the size of the estimate and the unambiguous delay range -- must equal the numpy restatement of tests/srs_tx.py, and every rule of the C ABI
must refuse with its code and its message. The record sizes are checked against include/miphy.h with a C program."""
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import miphy
import srs_ref as R
import srs_tx as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPP = -1, -4


def info_of(p, **changes):
    j = X.job_of(p)
    for k, v in changes.items():
        j[k] = v
    return miphy.srs_info(j)


def refused(code, text, p, **changes):
    with pytest.raises(Exception) as e:
        info_of(p, **changes)
    assert "error %d" % code in str(e.value) and text in str(e.value), str(e.value)
    assert text in miphy.lib().miphy_last_error().decode()


def test_every_accepted_combination_equals_the_numpy_restatement():
    n = refused_q = unsupp = 0
    for K, nap, prg, nprb, R_ in itertools.product((2, 4), (1, 2, 4), (1, 2, 4), (4, 8, 12, 52, 272), (1, 3)):
        for ncs in range(8 if K == 2 else 12):
            p = X.ue(R=R_, nap=nap, start=n % 11, nsym=(1, 2, 4)[n % 3], K=K, kbar=n % K, ncs=ncs, nid=(37 * n) % 1024, hopping=n % 3, prg=prg, prb=n % 3, nprb=nprb,
                     slot=n % 20, numerology=1)
            n += 1
            d = X.derive(p)
            if d["M"] == 24:
                refused(EUNSUPP, "Table 5.2.2.2-4", p)
                unsupp += 1
                continue
            if d["Q"] % d["P"]:
                refused(EINVAL, "not a multiple of the ports that share the comb", p)
                refused_q += 1
                continue
            got = info_of(p)
            assert [int(got[k]) for k in ("M", "Q", "P", "G", "nof_combs")] == [d["M"], d["Q"], d["P"], d["G"], len(d["combs"])], p
            assert list(got["cyclic_shifts"][:nap]) == d["cs"] and list(got["comb_offsets"][:nap]) == d["off"], p
            assert not got["cyclic_shifts"][nap:].any() and not got["comb_offsets"][nap:].any()
            assert int(got["nof_h"]) == d["G"] * R_ * nap
            assert abs(float(got["max_delay_s"]) - R.max_delay(p)) <= 1e-6 * R.max_delay(p)
    assert refused_q > 0 and unsupp > 0 and n - refused_q - unsupp > 500


def test_a_handful_of_jobs():
    got = info_of(X.ue(R=2, nap=4, K=2, ncs=5, nprb=8, prg=2))  # four ports split over both combs
    assert [int(got[k]) for k in ("M", "Q", "P", "G", "nof_combs", "nof_h")] == [48, 12, 2, 4, 2, 32]
    assert list(got["cyclic_shifts"]) == [5, 7, 1, 3] and list(got["comb_offsets"]) == [0, 1, 0, 1]
    assert abs(float(got["max_delay_s"]) - 1 / (2 * 15e3 * 2 * 2)) < 1e-11
    got = info_of(X.ue(R=4, nap=4, K=4, kbar=3, ncs=5, nprb=272, prg=4, numerology=1))  # four ports on one comb
    assert [int(got[k]) for k in ("M", "Q", "P", "G", "nof_combs", "nof_h")] == [816, 12, 4, 68, 1, 1088]
    assert list(got["cyclic_shifts"]) == [5, 8, 11, 2] and list(got["comb_offsets"]) == [3, 3, 3, 3]
    assert abs(float(got["max_delay_s"]) - 1 / (2 * 30e3 * 4 * 4)) < 1e-11
    got = info_of(X.ue(R=1, nap=4, K=4, kbar=3, ncs=6, nprb=12, prg=2))  # split: the other comb wraps to offset 1
    assert list(got["cyclic_shifts"]) == [6, 9, 0, 3] and list(got["comb_offsets"]) == [3, 1, 3, 1] and int(got["P"]) == 2
    got = info_of(X.ue(nap=1, K=2, nprb=272, prg=1, ncs=7))  # the longest sequence
    assert [int(got[k]) for k in ("M", "Q", "P", "G")] == [1632, 6, 1, 272]
    got = info_of(X.ue(nap=2, K=4, nprb=4, prg=2, ncs=11))  # the shortest
    assert [int(got[k]) for k in ("M", "Q", "P", "G")] == [12, 6, 2, 2] and list(got["cyclic_shifts"]) == [11, 5, 0, 0]


def test_the_rules():
    p = X.ue(R=2, nap=2, start=10, nsym=4, K=2, kbar=1, ncs=7, nid=1023, hopping=2, prg=2, prb=3, nprb=8, slot=19, numerology=1, grid_nprb=11)
    info_of(p)
    refused(EINVAL, "outside the frame", p, slot=20)
    refused(EINVAL, "outside the frame", p, numerology=5)
    refused(EINVAL, "invalid number of receive ports", p, nof_rx_ports=0)
    refused(EINVAL, "invalid number of receive ports", p, nof_rx_ports=5)
    refused(EINVAL, "invalid number of transmit ports", p, nof_tx_ports=3)
    refused(EINVAL, "invalid number of transmit ports", p, nof_tx_ports=0)
    refused(EINVAL, "invalid symbol range", p, nof_symbols=3)
    refused(EINVAL, "invalid symbol range", p, nof_symbols=0)
    refused(EINVAL, "invalid symbol range", p, start_symbol=11)  # four symbols from 11 leave the slot
    refused(EINVAL, "invalid symbol range", p, start_symbol=14, nof_symbols=1)
    refused(EINVAL, "comb_size is 2 or 4", p, comb_size=3)
    refused(EINVAL, "comb_size is 2 or 4", p, comb_size=0)
    refused(EINVAL, "comb_offset below it", p, comb_offset=2)
    refused(EINVAL, "comb_offset below it", p, comb_size=4, comb_offset=4)
    refused(EINVAL, "cyclic_shift is below 8", p, cyclic_shift=8)
    refused(EINVAL, "cyclic_shift is below 8", p, comb_size=4, cyclic_shift=12)
    info_of(p, comb_size=4, cyclic_shift=11, nof_prb=12, grid_nprb=15)
    refused(EINVAL, "n_id is 0..1023", p, n_id=1024)
    refused(EINVAL, "hopping is 0", p, hopping=3)
    refused(EINVAL, "prg_size is 1, 2 or 4", p, prg_size=3)
    refused(EINVAL, "prg_size is 1, 2 or 4", p, prg_size=0)
    refused(EINVAL, "nof_prb is a multiple of 4", p, nof_prb=6, grid_nprb=20)
    refused(EINVAL, "nof_prb is a multiple of 4", p, nof_prb=0)
    refused(EINVAL, "nof_prb is a multiple of 4", p, nof_prb=276, start_prb=0, grid_nprb=276)
    refused(EINVAL, "leaves the grid window", p, grid_nprb=10)  # a window too narrow
    refused(EINVAL, "leaves the grid window", p, grid_nprb=276)
    refused(EINVAL, "leaves the grid window", p, grid_nprb=0)
    refused(EUNSUPP, "Table 5.2.2.2-4", p, nof_prb=4)  # M = 24 at comb 2
    refused(EUNSUPP, "Table 5.2.2.2-4", p, comb_size=4, nof_prb=8)  # and at comb 4
    refused(EINVAL, "not a multiple of the ports that share the comb", p, nof_tx_ports=4, cyclic_shift=0, prg_size=1)  # K = 2, four ports on one comb, Q = 6
    info_of(p, nof_tx_ports=4, cyclic_shift=4, prg_size=1)  # the same ports on two combs: P = 2
    refused(EINVAL, "not a multiple of the ports that share the comb", p, comb_size=4, nof_prb=12, grid_nprb=15, prg_size=1)  # Q = 3, P = 2
    with pytest.raises(Exception, match="null argument"):
        miphy.binding.check(miphy.lib().miphy_srs_info(None, None))


def test_record_sizes_and_offsets_against_the_header():
    names = (("miphy_srs_job", miphy.SrsJob), ("miphy_srs_info_t", miphy.SrsInfo), ("miphy_srs_result", miphy.SrsResult))
    lines = ['printf("%%zu\\n", sizeof(%s));' % n for n, _ in names]
    for n, dt in names:
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (n, f) for f in dt.names]
    src = '#include "miphy.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    want = [dt.itemsize for _, dt in names] + [dt.fields[f][1] for _, dt in names for f in dt.names]
    assert got == want, (got, want)
    assert got[:3] == [48, 36, 168] and all(s % 8 == 0 for s in (got[0], got[2]))
