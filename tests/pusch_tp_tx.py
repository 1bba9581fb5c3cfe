"""PUSCH transmitter with transform precoding (DFT-s-OFDM) on the host: the transmitter of tests/pusch_tx.py with the precoding DFT of
TS 38.211 6.3.1.4 on every data symbol and the low-PAPR DM-RS of 6.4.1.1.1.2 (tests/pusch_tp_ref.py) in place of the Gold-sequence one;
one layer, DM-RS type 1 on the even subcarriers with two CDM groups without data, a contiguous allocation. Multiplexed UCI as in
tests/pusch_uci_tx.py (the multiplexing happens in front of the precoder, in codeword order). No device code is involved.

TP_CASES are the slots of tests/test_pusch_proc_tp_gpu.py; tests/test_pusch_tp.py shows on the CPU that the restated receiver recovers
every transport block."""
import functools

import numpy as np

import oracle_lib as O
import pusch_tp_ref as R
import uci_short_block as U
from pusch_tx import NOF_GRID_PORTS, base_graph, port_channel
from pusch_uci_tx import mux_map


def tp_slot(rng, case, tb, uci=None):
    """One slot of `case`. uci: None or dict(O=(ack, csi1, csi2) information bits, G_re=(..) resource elements each, rvd_re, msgs=[bits ..]).
    Returns (grid [4][14][nsc] complex64, rb, dm, ucase, placeholders): ucase / placeholders of the demultiplexer (None without UCI)."""
    c = case
    nsc = c["nprb_grid"] * 12
    rb = np.zeros(c["nprb_grid"], np.uint8)
    rb[c["first"]:c["first"] + c["nprb"]] = 1
    dm = np.zeros(14, np.uint8)
    dm[[l for l in c["dmrs"] if c["start"] <= l < c["start"] + c["nof"]]] = 1
    data = [l for l in range(c["start"], c["start"] + c["nof"]) if not dm[l]]
    dsyms = [l for l in range(c["start"], c["start"] + c["nof"]) if dm[l]]
    M, mod = 12 * c["nprb"], c["mod"]
    nre = len(data) * M
    sub = np.arange(c["first"] * 12, c["first"] * 12 + M)
    ucase = ph = None
    if uci is None:
        cw = O.o_pdsch_encode(c["bg"], 0, mod, 0, 1, nre, tb)
    else:
        G = tuple(g * mod for g in uci["G_re"])
        ucase = (mod, 1, c["nprb"], c["start"], c["nof"], uci["rvd_re"] * mod, 1, sum(1 << l for l in dsyms), 2, G, tuple(uci["O"]))
        n_in, n_sch, _, ph = O.o_ulsch_demultiplex(*ucase)
        assert n_in == nre * mod
        fields = [U.rate_match(U.encode(m, mod), g) if o else np.zeros(0, np.uint8) for m, o, g in zip(uci["msgs"], uci["O"], G)]
        cw = np.zeros(n_in, np.uint8)
        for m, bits in zip(mux_map(ucase, n_in), [O.o_pdsch_encode(c["bg"], 0, mod, 0, 1, n_sch // mod, tb)] + fields):
            cw[m[m >= 0]] = bits[m >= 0]
    bits = cw ^ O.o_gold((c["rnti"] << 15) + c["n_id"], 0, cw.size)
    for re in (ph if ph is not None else ()):  # TS 38.211 6.3.1.1: y repeats the previous scrambled bit, x is 1
        bits[re * mod + 1] = bits[re * mod]
        bits[re * mod + 2:re * mod + mod] = 1
    sym = O.nr_modulate(bits, mod).astype(np.complex128)
    tx = np.zeros((14, nsc), np.complex128)
    for i, l in enumerate(data):  # TS 38.211 6.3.1.4: y[k] = (1 / sqrt(M)) sum_i x[i] e^(-j 2 pi i k / M)
        tx[l, sub] = np.fft.fft(sym[i * M:(i + 1) * M]) / np.sqrt(M)
    pilots = R.dmrs_pilots(c["scr"], c["hopping"], c["slot"], dsyms, c["nprb"])
    for i, l in enumerate(dsyms):
        tx[l, sub[0::2]] = R.DMRS_BETA * pilots[i]
    grid = np.full((NOF_GRID_PORTS, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    sigma = 10 ** (-c["snr_db"] / 20) * np.sqrt(0.5)
    for p, d in zip(c["ports"], c["delay"]):
        noise = (rng.standard_normal((14, nsc)) + 1j * rng.standard_normal((14, nsc))) * sigma
        grid[p] = (tx * port_channel(p, nsc, d) + noise).astype(np.complex64)
    return grid, rb, dm, ucase, ph


def _case(name, nprb_grid, first, nprb, ports, mod, tbs, dmrs, slot, scr, hopping, snr_db, delay, rnti=0x4601, n_id=900, uci=None):
    nre = nprb * 12 * (14 - len(dmrs))
    return dict(name=name, nprb_grid=nprb_grid, first=first, nprb=nprb, ports=tuple(ports), mod=mod, tbs=tbs, start=0, nof=14, dmrs=tuple(dmrs), mu=1,
                slot=slot, scr=scr, hopping=hopping, snr_db=snr_db, delay=tuple(delay), rnti=rnti, n_id=n_id, uci=uci, bg=base_graph(tbs, tbs / (nre * mod)))


# 2, 5, 6 and 25 PRB in QPSK and 64QAM, 2 and 6 PRB in pi/2-BPSK as well; one and two ports; lengths 12, 30, 36 and 150 of the DM-RS; one slot with
# HARQ-ACK and CSI part 1 multiplexed, one with group hopping, one with sequence hopping at a length that has v = 1.
TP_CASES = [
    _case("prb2_qpsk", 24, 3, 2, (1,), 2, 208, (2, 11), 3, 17, 0, 14.0, (2.0,)),
    _case("prb2_qam64", 24, 5, 2, (0, 2), 6, 672, (2, 7, 11), 4, 1007, 0, 27.0, (1.0, -2.0)),
    _case("prb2_bpsk", 24, 20, 2, (3,), 1, 104, (2, 11), 5, 0, 0, 10.0, (0.0,)),
    _case("prb5_qpsk", 24, 1, 5, (2, 1), 2, 552, (2, 11), 6, 451, 0, 12.0, (3.0, -1.0)),
    _case("prb5_qam64", 24, 19, 5, (0,), 6, 1800, (2, 7, 11), 7, 30, 0, 29.0, (2.0,)),
    _case("prb6_qpsk_uci", 24, 7, 6, (1,), 2, 552, (2, 11), 8, 123, 0, 14.0, (1.5,), uci=dict(O=(4, 5, 0), G_re=(30, 40, 0), rvd_re=0)),
    _case("prb6_qam64_group_hopping", 24, 2, 6, (3, 0), 6, 2088, (2, 7, 11), 19, 777, 1, 27.0, (0.0, 4.0)),
    _case("prb6_bpsk", 24, 18, 6, (0, 1), 1, 320, (2, 11), 9, 64, 0, 7.0, (1.0, 2.0)),
    _case("prb25_qpsk", 52, 11, 25, (2,), 2, 2976, (2, 11), 10, 999, 0, 12.0, (5.0,)),
    _case("prb25_qam64_sequence_hopping", 52, 27, 25, (1, 3), 6, 9736, (2, 7, 11), 0, 500, 2, 27.0, (-3.0, 6.0)),
]


def transport_block(case):
    return np.random.default_rng(sum(case["name"].encode())).integers(0, 256, case["tbs"] // 8, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def build(name):
    """(case, tb, grid, rb, dm, uci, ucase, placeholders) of a named case, built once per process; uci carries the sent field bits (msgs)."""
    c = dict(next(x for x in TP_CASES if x["name"] == name))
    tb = transport_block(c)
    rng = np.random.default_rng(77 + sum(name.encode()))
    uci = None
    if c["uci"]:
        uci = dict(c["uci"])
        uci["msgs"] = [rng.integers(0, 2, o, dtype=np.uint8) for o in uci["O"]]
    grid, rb, dm, ucase, ph = tp_slot(rng, c, tb, uci)
    for a in (tb, grid, rb, dm):
        a.setflags(write=False)
    return c, tb, grid, rb, dm, uci, ucase, ph
