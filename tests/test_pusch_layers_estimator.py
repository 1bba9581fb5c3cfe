"""CPU: the float64 restatement of the layered DM-RS estimator (tests/pusch_layers_estimator_cases.py) against what it can be held to without a
device: (a) it returns a flat noise-free channel, where the reference-style estimate of a layer that shares its CDM group is off by the other
layer; (b) where a layer is alone in its group it is the oracle's estimator; (c) the transmissions of the GPU processor test decode through it on
the host; (d) the library exports both entry points and the binding's records match the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nl,npt", PL.LAYERED)
def test_flat_channel_is_returned_and_the_one_layer_fit_is_not_enough(nl, npt):
    """(a) One tap at delay 0, no noise: float64 on an exactly representable model -> 1e-5 of max |h|, compact (one row) and full. The oracle's
    estimator on the same grid misses every layer that shares its group by more than 0.1 max |h|: why the entry point exists."""
    rng = np.random.default_rng(100 * nl + npt)
    case, h = E.make_case(rng, 24, slice(3, 15), npt, nl, [2, 11], delay=0.0, taps=1, background=0.0)
    ce, sc = E.estimate(*case)
    mask = np.repeat(case[7].astype(bool), 12)
    hmax = np.abs(h).max()
    want = np.broadcast_to(h[:, :, None, :], ce.shape)
    assert np.abs(ce[..., mask] - want[..., mask]).max() < 1e-5 * hmax            # full: every symbol of the allocation
    assert np.abs(ce[:, :, :1][..., mask] - h[:, :, None, :][..., mask]).max() < 1e-5 * hmax  # compact: the one row a compact job holds
    assert np.isnan(ce[..., ~mask]).all()
    oce, _ = O.o_dmrs_pusch_estimate(*case)
    for ly in range(nl):
        shares = (ly ^ 1) < nl
        miss = np.abs(oce[ly][..., mask] - want[ly][..., mask]).max() / hmax
        assert (miss > 0.1) if shares else (miss < 1e-4), (ly, miss)


def _assert_like_chest_gpu(got_ce, got_sc, exp_ce, exp_sc, mask, mu):
    err = np.abs(got_ce[..., mask] - exp_ce[..., mask]).max() / np.abs(exp_ce[..., mask]).max()
    assert err < 1e-4, err
    for k in range(4):
        rel = np.abs(got_sc[..., k] - exp_sc[..., k]) / (np.abs(exp_sc[..., k]) + 1e-30)
        assert rel.max() < 1e-4, (k, got_sc[..., k], exp_sc[..., k])
    tap = 1.0 / (4096 * 15000.0 * (1 << mu))
    assert np.abs(got_sc[..., 4] - exp_sc[..., 4]).max() <= 1.01 * tap


@pytest.mark.parametrize("dsyms", ([2], [2, 11], [2, 7, 11], [2, 5, 8, 11]))
def test_solo_layers_are_the_oracles(dsyms):
    """(b) L = 1, and layer 2 of three: the tolerances of tests/test_chest_gpu.py."""
    rng = np.random.default_rng(len(dsyms))
    prbs = [0, 1, 2, 10, 11, 30, 31, 32, 33, 51]
    case, _ = E.make_case(rng, 52, prbs, 2, 1, dsyms, delay=3.0, first=1, nof=13)
    mask = np.repeat(case[7].astype(bool), 12)
    ce, sc = E.estimate(*case)
    oce, osc = O.o_dmrs_pusch_estimate(*case)
    _assert_like_chest_gpu(ce[:, :, 1:], sc, oce[:, :, 1:], osc, mask, 1)
    case, _ = E.make_case(rng, 52, prbs, 3, 3, dsyms, delay=1.0, numerology=0, slot=9)
    ce, sc = E.estimate(*case)
    oce, osc = O.o_dmrs_pusch_estimate(*case)
    _assert_like_chest_gpu(ce[2:], sc[:, 2:], oce[2:], osc[:, 2:], mask, 0)


@pytest.mark.parametrize("nl,npt,mod,tb_bytes,snr_db,dmrs", E.CHAIN_CASES + [E.ONE_LAYER_CASE])
def test_chain_cases_decode_on_the_host(nl, npt, mod, tb_bytes, snr_db, dmrs):
    """(c) restatement -> expected_llr with that estimate and its noise variance -> the oracle decoder, 6 iterations."""
    c, tb, grid, est = E.chain_tx(nl, npt, mod, tb_bytes, snr_db, dmrs)
    llr = E.host_llr(c, grid, est)
    ok, out, _ = O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes).decode(llr, 0, True, 6, True)
    assert ok and np.array_equal(out, tb)


def test_retransmission_case_needs_its_second_transmission():
    """The retransmission of the GPU processor test: rv 0 alone fails in the host chain, rv 2 combined with it decodes."""
    nl, npt, mod, tb_bytes, snr_db, dmrs = E.RETX_CASE
    dec = None
    for rv, want in ((0, False), (2, True)):
        c, tb, grid, est = E.chain_tx(nl, npt, mod, tb_bytes, snr_db, dmrs, rv=rv)
        dec = dec or O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes)
        ok, out, _ = dec.decode(E.host_llr(c, grid, est), rv, rv == 0, 6, True)
        assert ok == want, rv
    assert np.array_equal(out, tb)


def test_exports_and_layouts():
    """(d) Both entry points are in the library; PuschLayersPdu is miphy_pusch_pdu plus eight bytes, the layer count first."""
    import miphy
    lib = ctypes.CDLL(miphy.lib_path)
    for name in ("miphy_dmrs_pusch_estimate_layers_batch", "miphy_pusch_process_layers_batch"):
        assert hasattr(lib, name), name
    assert miphy.PuschLayersPdu.itemsize == miphy.PuschPdu.itemsize + 8
    assert miphy.PuschLayersPdu.fields["nof_tx_layers"][1] == miphy.PuschPdu.itemsize
    assert miphy.PuschLayersPdu.fields["base"][0] == miphy.PuschPdu
    hdr = open(os.path.join(ROOT, "include", "miphy.h")).read()
    assert re.search(r"miphy_pusch_pdu\s+base;\s*uint8_t\s+nof_tx_layers;[^}]*uint8_t\s+reserved\[7\];\s*\}\s*miphy_pusch_layers_pdu;", hdr)
    assert hasattr(miphy.Context, "dmrs_pusch_estimate_layers_batch") and hasattr(miphy.Context, "pusch_process_layers_batch")
