"""CPU: the host side of PUSCH with multiplexed UCI and EVM above one layer. The new entry points exist in the library and the binding; the
restatements of tests/pusch_layers_uci_cases.py (placeholder descrambling, EVM terms) are the oracle's at one layer, where it has a say; noise free
they return the multiplexed bits on 2, 3 and 4 layers; and the four transmissions the device tests receive decode in the host chain (true channel as
the estimate, zf_single, the oracle's demultiplexer, the field decoders, the oracle's transport block decoder)."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL
import pusch_layers_uci_cases as U


def test_entry_points_exist():
    import miphy
    lib = ctypes.CDLL(miphy.lib_path)
    for name in ("miphy_pusch_demodulate_layers_batch_ex", "miphy_pusch_process_layers_batch_ex"):
        assert hasattr(lib, name), name
    for name in ("pusch_demodulate_layers_batch_ex", "pusch_process_layers_batch_ex"):
        assert callable(getattr(miphy.Context, name, None)), name


@pytest.mark.parametrize("mod", [2, 4, 6, 8])
def test_restatement_is_the_oracle_on_one_layer(mod):
    """One layer, two ports, a one-bit HARQ-ACK on reserved elements: the oracle's equalised symbols through compose_llr with the placeholder chips
    are the bytes of orc_pusch_demodulate_ex with that list, and the restated EVM is its EVM (float32 against float64 accumulation: 1e-6)."""
    c = U.allocation(1, 2, mod, noise_var=0.02, seed=40 + mod)
    grid, ce = PL.random_slot(c)
    mc = U.mux_case(c, (1, 0, 0), (20, 0, 0), 40)
    ph = O.o_ulsch_demultiplex(*mc)[3]
    assert ph.size == 20
    rb, dm = PL.masks(c)
    args = (c["rnti"], c["n_id"], mod, 0, 14, dm, 0, 2, rb, grid[:2], np.repeat(ce[0], 14, axis=1), c["noise_var"])
    _, eq, nv = O.o_pusch_demodulate(*args)
    llr, evm = O.o_pusch_demodulate_ex(*args, placeholders=ph)
    assert np.array_equal(U.compose_llr(c, eq[None, :], nv[None, :], ph), llr)
    assert not np.array_equal(U.compose_llr(c, eq[None, :], nv[None, :]), llr)
    terms = U.evm_terms(c, eq[None, :], nv[None, :])
    mine = np.sqrt(terms.astype(np.float64).sum() / terms.size)
    assert abs(mine - evm) <= 1e-6 * evm, (mine, evm)


def test_pi2_bpsk_evm_is_the_oracle_on_one_layer():
    c = U.allocation(1, 1, 1, noise_var=0.02, seed=3)
    grid, ce = PL.random_slot(c)
    rb, dm = PL.masks(c)
    args = (c["rnti"], c["n_id"], 1, 0, 14, dm, 0, 2, rb, grid[:1], np.repeat(ce[0], 14, axis=1), c["noise_var"])
    _, eq, nv = O.o_pusch_demodulate(*args)
    _, evm = O.o_pusch_demodulate_ex(*args)
    terms = U.evm_terms(c, eq[None, :], nv[None, :])
    mine = np.sqrt(terms.astype(np.float64).sum() / terms.size)
    assert abs(mine - evm) <= 1e-6 * evm, (mine, evm)


@pytest.mark.parametrize("nl,npt,mod", [(2, 2, 2), (2, 3, 8), (3, 3, 6), (3, 4, 4), (4, 4, 8), (4, 4, 2)])
def test_noise_free_soft_bits_carry_the_multiplexed_bits(nl, npt, mod):
    """Two one-bit fields (placeholders in both) and a CSI part 2: outside the x positions the sign of every restated LLR is the multiplexed bit."""
    t = U.build("n", dict(nl=nl, npt=npt, mod=mod, tb_bytes=None, snr_db=30.0, O=(1, 1, 5), G_re=(20, 30, 12), rvd_re=40))
    c = t["c"]
    assert t["ph"].size == 50
    grid, ce = U.transmit_true(c, t["scr"])
    y, h = PL.extract(c, grid, ce)
    x, nv = PL.zf_single(y, h, 1e-3, 1.0)
    llr = U.compose_llr(c, x, nv, t["ph"])
    look = ~U.x_positions(llr.size, t["ph"], nl, mod)
    assert np.all(llr[look] != 0) and np.array_equal((llr[look] < 0).astype(np.uint8), t["cw"][look])
    # and the plain descrambler gets the y bits of the placeholder symbols wrong where the chips of bits 0 and 1 differ
    plain = PL.compose_llr(c, x, nv)
    assert np.any((plain[look] < 0).astype(np.uint8) != t["cw"][look])


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_cases_decode_in_the_host_chain(name):
    t = U.build(name)
    c = t["c"]
    assert t["ph"].size == {"A": 20, "B": 0, "C": 0, "D": 50}[name]
    grid, ce = U.transmit_true(c, t["scr"], snr_db=t["snr_db"])
    y, h = PL.extract(c, grid, ce)
    x, nv = PL.zf_single(y, h, c["noise_var"], 1.0)
    fields, tb = U.receive(t, U.compose_llr(c, x, nv, t["ph"]))
    for k, f in enumerate(fields):
        if t["O"][k]:
            assert f[1] and np.array_equal(f[0], t["payloads"][k]), (name, k)
    if t["tb"] is not None:
        assert tb[0] and np.array_equal(tb[1], t["tb"]), name
