"""CPU: PUSCH with transform precoding (DFT-s-OFDM). The numpy restatement of TS 38.211 (tests/pusch_tp_ref.py) is held to the properties the
standard gives its sequences, the library's host function miphy_low_papr_sequence to the restatement, the records of the new entry points to
include/miphy.h, and the slots of tests/pusch_tp_tx.py -- what tests/test_pusch_proc_tp_gpu.py sends through the device -- are shown to be
decodable by the restated receiver alone."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pucch_tx
import pusch_tp_ref as R
import pusch_tp_tx as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "srsran_project_23.5_amd", "libmiphy.so")
MIPHY_EINVAL, MIPHY_EUNSUPP = -1, -4
LENGTHS = (12, 30, 36, 72, 1500, 1620)


def test_the_transform_precoding_sizes():
    s = R.tp_sizes()
    assert len(s) == 53 and s[0] == 1 and s[-1] == 270 and 7 not in s and 25 in s
    assert sum(1 for n in s if n % 5 == 0) == 25  # the sizes that need a radix-5 pass


@pytest.mark.parametrize("length", LENGTHS + (150, 600))
def test_low_papr_restatement(length):
    """Unit modulus; the table of PUCCH formats 0 and 1 at length 12; r(n + N_ZC) = r(n) from length 36 on (the base sequence is the cyclic
    extension of a Zadoff-Chu sequence of prime length); u and v give different sequences."""
    seen = set()
    for u in range(30):
        for v in ((0, 1) if length >= 72 else (0,)):
            r = R.low_papr(u, v, length)
            assert r.shape == (length,) and np.abs(np.abs(r) - 1).max() < 1e-12
            if length == 12:
                assert np.abs(r - pucch_tx.low_papr_table()[u, 0]).max() < 1e-6
            if length >= 36:
                nzc = R.largest_prime_below(length)
                assert nzc < length and np.abs(r[nzc:] - r[:length - nzc]).max() < 1e-9
                # a Zadoff-Chu sequence of prime length has a flat spectrum
                assert np.abs(np.abs(np.fft.fft(r[:nzc])) - np.sqrt(nzc)).max() < 1e-6
            seen.add(np.round(r, 6).tobytes())
    assert len(seen) == 30 * (2 if length >= 72 else 1)


def test_hopping_restatement():
    """Neither: u = n_ID mod 30, v = 0. Group hopping moves u with the symbol and the slot and leaves v; sequence hopping leaves u and draws v,
    below length 72 never."""
    assert R.dmrs_uv(777, 0, 19, 11, 150) == (777 % 30, 0)
    us = {R.dmrs_uv(777, 1, s, l, 150) for s in (0, 19) for l in (2, 7, 11)}
    assert len(us) > 2 and all(v == 0 and 0 <= u < 30 for u, v in us)
    vs = [R.dmrs_uv(500, 2, s, l, 150) for s in range(20) for l in (2, 11)]
    assert {u for u, _ in vs} == {500 % 30} and {v for _, v in vs} == {0, 1}
    assert all(R.dmrs_uv(500, 2, s, 2, 36) == (500 % 30, 0) for s in range(20))


def _lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import torch  # noqa: F401  (brings the HIP runtime the library links against)
    lib = ctypes.CDLL(LIB)
    lib.miphy_low_papr_sequence.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def test_host_low_papr_sequence_matches_restatement():
    """Within 1e-6 absolute: the argument of the sine and cosine is a fraction below 2 of pi, rounded to single precision at worst (3.7e-7 rad),
    plus two units in the last place of the functions. Every u and both v, at the lengths of 2, 5, 6, 12, 250 and 270 PRB."""
    lib = _lib()
    worst = 0.0
    for length in LENGTHS:
        for u in range(30):
            for v in (0, 1):
                out = np.full(length + 2, 7 + 7j, np.complex64)
                rc = lib.miphy_low_papr_sequence(u, v, length, out.ctypes.data_as(ctypes.c_void_p))
                assert rc == 0, (u, v, length)
                assert np.all(out[length:] == 7 + 7j)
                d = np.abs(out[:length].astype(np.complex128) - R.low_papr(u, v, length)).max()
                worst = max(worst, d)
                assert d <= 1e-6, (u, v, length, d)
    print("worst distance of miphy_low_papr_sequence from the restatement: %.3g" % worst)


def test_host_low_papr_sequence_refusals():
    lib = _lib()
    out = np.zeros(2000, np.complex64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for length in (6, 18, 24):  # Tables 5.2.2.2-1, -3, -4 are not in the library
        assert lib.miphy_low_papr_sequence(0, 0, length, p) == MIPHY_EUNSUPP
    for u, v, length in ((30, 0, 36), (0, 2, 72), (0, 0, 0), (0, 0, 35), (0, 0, 40), (0, 0, 1626), (0, 0, 13)):
        assert lib.miphy_low_papr_sequence(u, v, length, p) == MIPHY_EINVAL, (u, v, length)
    assert lib.miphy_low_papr_sequence(0, 0, 36, None) == MIPHY_EINVAL
    assert not out.any()


def test_binding_record_sizes_match_header():
    import miphy
    src = r'''
#include "miphy.h"
#include <stddef.h>
#include <stdio.h>
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(miphy_transform_deprecode_job), sizeof(miphy_pusch_chest_tp_job), offsetof(miphy_pusch_chest_tp_job, hopping),
         sizeof(miphy_pusch_tp_pdu), offsetof(miphy_pusch_tp_pdu, hopping));
  printf("%zu %zu\n", offsetof(miphy_transform_deprecode_job, eq_symbols_offset), offsetof(miphy_transform_deprecode_job, out_noise_var_offset));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    mine = [miphy.TransformDeprecodeJob.itemsize, miphy.PuschChestTpJob.itemsize, miphy.PuschChestTpJob.fields["hopping"][1], miphy.PuschTpPdu.itemsize,
            miphy.PuschTpPdu.fields["hopping"][1], miphy.TransformDeprecodeJob.fields["eq_symbols_offset"][1],
            miphy.TransformDeprecodeJob.fields["out_noise_var_offset"][1]]
    assert sizes == mine, (sizes, mine)


def test_deprecoder_restatement_inverts_the_precoder():
    rng = np.random.default_rng(5)
    for nprb in (1, 5, 270):
        M = 12 * nprb
        x = rng.standard_normal(M) + 1j * rng.standard_normal(M)
        y, v = R.deprecode(np.fft.fft(x) / np.sqrt(M), np.full(M, 0.25))
        assert np.abs(y - x).max() < 1e-10 and abs(v - 0.25) < 1e-15
    y, v = R.deprecode(np.ones(12), np.array([0.5, np.inf] + [1.5] * 10))
    assert abs(v - (0.5 + 15) / 11) < 1e-15 and abs(y[0] - 11 / np.sqrt(12)) < 1e-12  # the abnormal element counts as 0 and is left out of the mean
    assert R.deprecode(np.ones(12), np.full(12, np.inf))[1] == np.inf


@pytest.mark.parametrize("name", [c["name"] for c in T.TP_CASES])
def test_restated_receiver_recovers_every_transport_block(name):
    """Every slot of the device test decodes in the restated receiver: the cases are decodable by the restatement of the standard alone."""
    import uci_short_block as U
    c, tb, grid, rb, dm, uci, ucase, ph = T.build(name)
    r = R.receive(c, grid, rb, dm, (ucase, ph) if uci else None)
    assert r["ok"] and np.array_equal(r["tb"], tb)
    if uci:
        for f, (o, m) in enumerate(zip(uci["O"], uci["msgs"])):
            if o:
                bits, status = U.detect(r["streams"][1 + f], o, c["mod"])
                assert np.array_equal(bits, m), f
