"""PUSCH slots with multiplexed UCI on the host, for the receive-chain tests that decode the UCI fields behind the PUSCH processor: one
layer, one receive port, DM-RS type 1 in symbol 2, the whole grid allocated. tests/pusch_tx.py places a transport block only; here the
encoded UCI fields are multiplexed with the map read off the oracle's demultiplexer (the reference has a demultiplexer only: the gNB
receives), as tests/test_pusch_uci_gpu.py does for random field bits. No device code is involved."""
import numpy as np

import oracle_lib as O
from pusch_tx import CHEST_SCALING, DMRS_AMPLITUDE, port_channel

TBS_BITS = {2: 2976, 4: 6016, 6: 9736, 8: 14600}


def mux_map(case, n_in):
    """Per output stream (UL-SCH, HARQ-ACK, CSI part 1, CSI part 2): the input index of every position (-1: punctured, no source).
    Three 'digits' of the input index go through the oracle's demultiplexer."""
    idx = np.arange(n_in)
    digs = [O.o_ulsch_demultiplex(*case, llr=((idx // (100 ** d)) % 100 + 1).astype(np.int8))[2] for d in range(3)]
    maps = []
    for k in range(4):
        a = [digs[d][k].astype(np.int64) for d in range(3)]
        src = (a[0] - 1) + 100 * (a[1] - 1) + 10000 * (a[2] - 1)
        src[a[0] == 0] = -1
        maps.append(src)
    return maps


def pusch_uci_slot(rng, nprb, mod, O_bits, G_re, rvd_re, field_bits, with_tb, slot=5, rnti=0x3311, n_id=411, scr=17, sigma=0.02):
    """One slot. O_bits: information bits of (HARQ-ACK, CSI part 1, CSI part 2); G_re: resource elements of each; field_bits: the
    encoded, rate-matched bits of each field (G_re[k] * mod of them, empty for an absent field). Returns a dict: grid [1][14][nsc]
    complex64, G, n_sch, tb (bytes, or None), bg, dm, rb, nof_harq_ack_rvd."""
    nsc = nprb * 12
    dm = np.zeros(14, np.uint8)
    dm[2] = 1
    rb = np.ones(nprb, np.uint8)
    G = tuple(g * mod for g in G_re)
    case = (mod, 1, nprb, 0, 14, rvd_re * mod, 1, 1 << 2, 2, G, tuple(O_bits))
    info = O.o_ulsch_demultiplex(*case)
    assert info is not None
    n_in, n_sch, _, ph = info
    assert n_in == nprb * 156 * mod
    tbs_bits = TBS_BITS[mod]
    bg = 1 if tbs_bits > 3824 else 2
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8) if with_tb else None
    sch_bits = O.o_pdsch_encode(bg, 0, mod, 0, 1, n_sch // mod, tb) if with_tb else rng.integers(0, 2, n_sch, dtype=np.uint8)
    cw = np.zeros(n_in, np.uint8)
    maps = mux_map(case, n_in)
    for k, bits in enumerate([sch_bits] + [np.asarray(b, np.uint8) for b in field_bits]):
        m = maps[k]
        assert m.size == bits.size, (k, m.size, bits.size)
        cw[m[m >= 0]] = bits[m >= 0]
    sc_bits = cw ^ O.o_gold((rnti << 15) + n_id, 0, n_in)
    for re in ph:  # TS 38.211 6.3.1.1: y repeats the previous scrambled bit, x is 1
        sc_bits[re * mod + 1] = sc_bits[re * mod]
        sc_bits[re * mod + 2:re * mod + mod] = 1
    sym = O.nr_modulate(sc_bits, mod)
    h = port_channel(0, nsc, 2.0).astype(np.complex64)
    grid = np.zeros((1, 14, nsc), np.complex64)
    data_syms = [l for l in range(14) if l != 2]
    for i, l in enumerate(data_syms):
        grid[0, l] = sym[i * nsc:(i + 1) * nsc] * h
    g3 = np.zeros((1, 14, nsc), np.complex64)
    O.o_dmrs_pdsch_map(slot, 0, 0, scr, 0, DMRS_AMPLITUDE, dm, rb, [0], g3)
    grid[0, 2] = g3[0, 2] * h
    grid += ((rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * sigma).astype(np.complex64)
    return dict(grid=grid, G=G, n_sch=n_sch, tb=tb, bg=bg, dm=dm, rb=rb, nof_harq_ack_rvd=rvd_re * mod, mod=mod, nprb=nprb, slot=slot, rnti=rnti,
                n_id=n_id, scr=scr, O=tuple(O_bits), scaling=CHEST_SCALING)
