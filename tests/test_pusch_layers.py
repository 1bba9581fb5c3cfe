"""CPU: the host restatement of PUSCH on 1..4 layers (tests/pusch_layers_cases.py) against the oracle where the oracle has a say, and against
itself elsewhere; and the library's new entry points as far as they can be seen without a GPU (exports, the LLR count)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL

MODS = (1, 2, 4, 6, 8)
# Largest |x_single - x_double| / (2^-24 cond(G) |x|) (norms over the layers of an element) that zf_single showed over seeds 0..4 at 2 000 elements
# per topology, and for the noise variances |nv_single - nv_double| / (2^-24 cond(G) nv): see test_zf_single_against_double.
ZF_BOUND = 10.2


@pytest.mark.parametrize("nl,npt", [(1, 1), (1, 2), (1, 3), (1, 4), (2, 2)])
def test_zf_single_is_the_oracle_where_the_oracle_goes(nl, npt):
    rng = np.random.default_rng(10 * nl + npt)
    y, h, nvar, _ = O.equalizer_case(rng, 1500, npt, nl, dead=(3, 700))
    for tx in (1.0, 0.7):
        z, nv = O.o_channel_equalize(y, h, nvar, tx)
        x, v = PL.zf_single(y, h, nvar, tx)
        assert np.array_equal(x.view(np.uint32), z.view(np.uint32))
        assert np.array_equal(v.view(np.uint32), nv.view(np.uint32))
        assert np.all(np.isinf(v[:, [3, 700]])) and np.all(x[:, [3, 700]] == 0)


def _zf_ratios(nl, npt, seed, n=2000):
    rng = np.random.default_rng(1000 * seed + 10 * nl + npt)
    h, cond = PL.channels(rng, nl, npt, n)
    assert cond.max() <= 16.0 * (1 + 1e-5)  # s in [0.5, 2] by construction (the rounding of H to single precision moves it by 1e-7)
    xs = (rng.standard_normal((nl, n)) + 1j * rng.standard_normal((nl, n))).astype(np.complex64)
    y = np.einsum("lpn,ln->pn", h.astype(np.complex128), xs.astype(np.complex128)).astype(np.complex64)
    tx, nvar = 0.8, 0.05
    xd, vd = PL.zf_double(y, h, nvar, tx)
    x1, v1 = PL.zf_single(y, h, nvar, tx)
    assert np.all(np.isfinite(v1))
    eps = 2.0 ** -24
    ex = np.linalg.norm(x1 - xd, axis=0) / (eps * cond * np.linalg.norm(xd, axis=0))
    ev = np.abs(v1 - vd).max(axis=0) / (eps * cond * np.abs(vd).max(axis=0))
    return float(ex.max()), float(ev.max())


@pytest.mark.parametrize("nl,npt", PL.TOPOLOGIES)
def test_zf_single_against_double(nl, npt):
    """The float32 restatement against the float64 pseudo-inverse, all topologies: error <= ZF_BOUND * 2^-24 * cond(G) * |x|. Measured with this
    very function (never with the kernel): the largest ratio over seeds 0..4 and all topologies was 5.06 for the symbols (1 x 3; 4 x 4: 2.65) and
    4.56 for the noise variances (2 x 2); ZF_BOUND is the larger one doubled, because the seeds are few."""
    worst = [_zf_ratios(nl, npt, seed) for seed in range(5)]
    ex, ev = max(w[0] for w in worst), max(w[1] for w in worst)
    print("zf_single vs zf_double %dx%d: symbols %.2f, noise variances %.2f (units of 2^-24 cond |x|)" % (nl, npt, ex, ev))
    assert ex <= ZF_BOUND and ev <= ZF_BOUND


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("npt,compact,type2,cdm", [(1, True, 0, 2), (2, False, 0, 1), (4, True, 1, 2)])
def test_expected_llr_on_one_layer_is_the_oracle_demodulator(mod, npt, compact, type2, cdm):
    """Pins the extraction, the order and the descrambling of the helper: at L = 1 it is orc_pusch_demodulate bit for bit."""
    c = PL.case("one", 1, npt, mod, compact=compact, type2=type2, cdm=cdm, rx_ports=(3, 0, 2, 1), seed=mod + npt)
    grid, ce = PL.random_slot(c)
    ce[0, 0, 0, 2 * 12 + 5] = 0  # a dead coefficient
    rb, dm = PL.masks(c)
    g = np.ascontiguousarray(grid[list(c["rx_ports"][:npt])])
    h = np.repeat(ce[0], 14, axis=1) if compact else ce[0]
    ref = O.o_pusch_demodulate(c["rnti"], c["n_id"], mod, c["start"], c["nof"], dm, type2, cdm, rb, g, h, c["noise_var"])[0]
    got = PL.expected_llr(c, grid, ce)
    assert got.size == ref.size == PL.nof_re(c) * mod
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("nl,npt", [(1, 1), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4)])
def test_noise_free_signs_are_the_transmitted_bits(nl, npt, mod):
    """Pins the layer order: without noise the sign of every expected LLR is the bit that the transmitter put there."""
    c = PL.case("signs", nl, npt, mod, seed=100 * nl + 10 * npt + mod)
    rng = np.random.default_rng(c["seed"])
    bits = rng.integers(0, 2, PL.nof_re(c) * nl * mod, dtype=np.uint8)
    grid, ce, _ = PL.transmit(c, bits=bits, rng=rng)
    llr = PL.expected_llr(c, grid, ce)
    assert np.all(llr != 0)
    assert np.array_equal((llr < 0).astype(np.uint8), bits)


@pytest.mark.parametrize("nl,npt,mod,tb_bytes,snr_db", PL.CHAIN_CASES)
def test_chain_cases_decode_on_the_cpu(nl, npt, mod, tb_bytes, snr_db):
    """The transmissions of tests/test_pusch_layers_chain_gpu.py decode in the host chain alone: expected_llr -> orc_pusch_decode(nof_layers)."""
    c, tb, grid, ce = PL.chain_transmission(nl, npt, mod, tb_bytes, snr_db)
    llr = PL.expected_llr(c, grid, ce)
    dec = O.OraclePuschDecoder(1, mod, 0, nl, PL.nof_re(c) * nl, tb_bytes)
    assert dec.seg.nof_cbs >= 2
    ok, out, _ = dec.decode(llr, 0, True, 6, True)
    assert ok and np.array_equal(out, tb)


def test_library_exports_and_llr_count():
    """Fails without the feature: the three new symbols of libmiphy.so, and miphy_pusch_demod_layers_nof_llr against the helper's count."""
    import miphy
    lib = ctypes.CDLL(miphy.lib_path)
    for name in ("miphy_channel_equalize_layers_batch", "miphy_pusch_demodulate_layers_batch", "miphy_pusch_demod_layers_nof_llr"):
        assert hasattr(lib, name), name
    assert miphy.PuschDemodLayersJob.itemsize == 128
    for nl, npt in PL.TOPOLOGIES:
        for mod, type2, cdm in ((1, 0, 2), (4, 0, 1), (6, 1, 2), (8, 1, 3)):
            c = PL.case("count", nl, npt, mod, type2=type2, cdm=cdm)
            j = PL.demod_job(miphy, c)
            assert miphy.pusch_demod_layers_nof_llr(j) == PL.nof_re(c) * nl * mod == j["base"]["nof_llr"]
    j = PL.demod_job(miphy, PL.case("count", 2, 2, 4))
    for bad in (0, 3, 5):  # no layers, more layers than ports, more than four
        j["nof_tx_layers"] = bad
        assert miphy.pusch_demod_layers_nof_llr(j) == 0
