"""PUSCH transmitter and channel on the host, for the receive-chain tests: one layer, DM-RS type 1 with two CDM groups without data (what
the PUSCH processor of this library receives), built from the oracle's encoder and DM-RS mapper and the numpy mapper of oracle_lib. No
device code is involved, so a slot built here pins the device receive chain to the oracle and not to the device's own transmit chain.

Grid layout: [4 ports][14][grid_nprb * 12] complex64. The selected grid ports carry the slot, each through a channel of its own; the
other ports are NaN, so a receiver that reads a port it was not given cannot produce a finite result.

PROC_CASES / HARQ_CASE are the slots of tests/test_pusch_proc_gpu.py; tests/test_pusch_tx.py shows on the CPU that every one of them
gives its stated verdict in the oracle chain alone. oracle_receive() is that chain."""
import functools

import numpy as np

import oracle_lib as O

NOF_GRID_PORTS = 4
DMRS_AMPLITUDE = 10 ** (3 / 20)  # pusch_processor_impl.cpp:150: two CDM groups without data -> +3 dB
CHEST_SCALING = np.float32(10.0) ** np.float32(3.0 / 20.0)


def base_graph(tbs_bits, rate):
    """TS 38.212 6.2.2."""
    return 2 if (tbs_bits <= 292 or (tbs_bits <= 3824 and rate <= 0.67) or rate <= 0.25) else 1


def port_channel(port, nsc, delay):
    """Frequency response of grid port `port`: a gain of its own and a linear phase of `delay` taps of a 4096-point IDFT."""
    gain = (0.75 + 0.1 * port) * np.exp(1j * (0.4 + 1.3 * port))
    return gain * np.exp(-2j * np.pi * np.arange(nsc) * delay / 4096)


def pusch_slot(rng, nprb_grid, prbs, ports, mod, tb, rv=0, Nref=0, start=0, nof=14, dmrs=(2,), slot=0, scr=0, n_scid=0, snr_db=30.0, delay=0.0,
               rnti=1, n_id=0, bg=1):
    """One PUSCH transmission on the grid ports `ports` (distinct, < 4). delay: taps per selected port (a scalar serves all).
    Returns (grid [4][14][nsc] complex64, rb_mask uint8 [nprb_grid], dmrs_mask uint8 [14])."""
    ports = list(ports)
    assert len(set(ports)) == len(ports) and all(0 <= p < NOF_GRID_PORTS for p in ports)
    delays = list(delay) if np.ndim(delay) else [float(delay)] * len(ports)
    assert len(delays) == len(ports)
    nsc = nprb_grid * 12
    rb = np.zeros(nprb_grid, np.uint8)
    rb[list(prbs)] = 1
    dm = np.zeros(14, np.uint8)
    dm[[l for l in dmrs if start <= l < start + nof]] = 1
    data_syms = [l for l in range(start, start + nof) if not dm[l]]
    sub = np.nonzero(np.repeat(rb, 12))[0]
    nre = len(data_syms) * sub.size
    cw = O.o_pdsch_encode(bg, rv, mod, Nref, 1, nre, tb)
    sym = O.nr_modulate(cw ^ O.o_gold((rnti << 15) + n_id, 0, cw.size), mod)
    tx = np.zeros((1, 14, nsc), np.complex64)
    O.o_dmrs_pdsch_map(slot, 0, 0, scr, n_scid, DMRS_AMPLITUDE, dm, rb, [0], tx)
    for i, l in enumerate(data_syms):  # symbol-major over the allocated subcarriers
        tx[0, l, sub] = sym[i * sub.size:(i + 1) * sub.size]
    grid = np.full((NOF_GRID_PORTS, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    sigma = 10 ** (-snr_db / 20) * np.sqrt(0.5)
    for p, d in zip(ports, delays):
        noise = (rng.standard_normal((14, nsc)) + 1j * rng.standard_normal((14, nsc))) * sigma
        grid[p] = (tx[0] * port_channel(p, nsc, d) + noise).astype(np.complex64)
    return grid, rb, dm


def nof_data_re(rb, dm, start, nof):
    return int(rb.sum()) * 12 * sum(1 for l in range(start, start + nof) if not dm[l])


def oracle_receive(case, grid, rb, dm, rv=0, new_data=True, decoder=None, ce_row=None, noise_var=None, want_evm=False):
    """The oracle chain estimator -> demodulator -> decoder on the selected ports of `grid`. With ce_row ([ports][nsc], an estimate from
    elsewhere) and noise_var the estimator is skipped and the row serves every symbol. Returns a dict (ce, sc, llr, evm, ok, tb, iters,
    decoder); the decoder keeps the HARQ state and is handed back in for a retransmission."""
    c = case
    g = np.ascontiguousarray(grid[list(c["ports"])])
    ce = sc = None
    if ce_row is None:
        ce, sc = O.o_dmrs_pusch_estimate(c["mu"], c["slot"], 0, c["scr"], c["n_scid"], CHEST_SCALING, dm, rb,
                                         c["start"], c["nof"], 1, g)
        h, nv = ce[0], float(sc[0, 0, 2])
    else:
        h, nv = np.repeat(np.asarray(ce_row, np.complex64)[:, None, :], c["start"] + c["nof"], axis=1), float(noise_var)
    args = (c["rnti"], c["n_id"], c["mod"], c["start"], c["nof"], dm, 0, 2, rb, g, h, nv)
    evm = None
    if want_evm:
        llr, evm = O.o_pusch_demodulate_ex(*args)
    else:
        llr = O.o_pusch_demodulate(*args)[0]
    if decoder is None:
        decoder = O.OraclePuschDecoder(c["bg"], c["mod"], c["Nref"], 1, nof_data_re(rb, dm, c["start"], c["nof"]), c["tbs"] // 8)
    ok, tb, iters = decoder.decode(llr, rv, new_data, 6, True)
    return dict(ce=ce, sc=sc, llr=llr, evm=evm, ok=ok, tb=tb, iters=iters, decoder=decoder)


def _case(name, nprb_grid, prbs, ports, mod, tbs, start, nof, dmrs, mu, slot, scr, n_scid, snr_db, delay, ok, Nref=0, rnti=0x4601, n_id=900, margin=True):
    prbs = list(prbs)
    nre = len(prbs) * 12 * (nof - len([l for l in dmrs if start <= l < start + nof]))
    return dict(name=name, nprb_grid=nprb_grid, prbs=prbs, ports=tuple(ports), mod=mod, tbs=tbs, start=start, nof=nof, dmrs=tuple(dmrs), mu=mu,
                slot=slot, scr=scr, n_scid=n_scid, snr_db=snr_db, delay=delay, ok=ok, Nref=Nref, rnti=rnti, n_id=n_id, margin=margin,
                bg=base_graph(tbs, tbs / (nre * mod)))


SCATTERED = [63, 64, 65, 127, 128, 191, 192, 255, 256, 274]  # crosses every 64-bit word of rb_mask
# ok: the verdict of the oracle chain (asserted in tests/test_pusch_tx.py). margin: the SNR is far enough from the decoding threshold for the
# verdict to survive the 1e-4 difference between the device's estimate and the oracle's.
PROC_CASES = [
    _case("two_ports_partial_slot", 52, range(5, 35), (3, 1), 4, 6016, 2, 12, (3, 10), 0, 9, 1000, 1, 18.0, (6.0, -4.0), True, Nref=12000),
    _case("four_ports_scattered", 52, [0, 1, 2, 10, 11, 30, 31, 32, 33, 51], (2, 0, 3, 1), 6, 3848, 0, 14, (2, 7, 11), 1, 7, 65535, 0, 12.0, 0.0, True,
          rnti=0xFFFF, n_id=1023),
    _case("three_ports_bg2", 25, range(25), (1, 3, 0), 2, 2976, 0, 13, (2, 11), 2, 39, 77, 0, 6.0, (3.0, -5.0, 8.0), True, rnti=0x1234, n_id=77),
    _case("one_port_widest_grid", 275, SCATTERED, (1,), 8, 4480, 1, 13, (2,), 3, 79, 40, 0, 30.0, 0.0, True, rnti=1, n_id=0),
    _case("one_port_crc_fails", 24, range(2, 22), (2,), 6, 9736, 0, 14, (2,), 1, 3, 9, 0, 4.0, 5.0, False, rnti=0x3311, n_id=411),
]
# rv 0, 2, 3, 1 in consecutive slots: fails twice, decodes at the third transmission (the same verdicts at 4.5 and 5.5 dB). Three DM-RS symbols:
# with fewer the estimator reports EPRE / 1000 as the noise variance, the LLRs saturate and combining does not help.
HARQ_CASE = _case("two_ports_harq", 24, range(2, 22), (3, 1), 6, 9736, 0, 14, (2, 7, 11), 1, 3, 9, 0, 5.0, (5.0, -3.0), True, rnti=0x1234, n_id=77)
HARQ_SEQUENCE = ((3, 0), (4, 2), (5, 3), (6, 1))  # (slot, rv)


def transport_block(case):
    return np.random.default_rng(sum(case["name"].encode())).integers(0, 256, case["tbs"] // 8, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def build(name, slot=None, rv=0):
    """(case, tb, grid, rb, dm) of a named case, built once per process. slot / rv: the transmission of a HARQ sequence."""
    c = dict(next(x for x in PROC_CASES + [HARQ_CASE] if x["name"] == name))
    if slot is not None:
        c["slot"] = slot
    tb = transport_block(c)
    rng = np.random.default_rng(1000 * c["slot"] + rv + sum(name.encode()))
    grid, rb, dm = pusch_slot(rng, c["nprb_grid"], c["prbs"], c["ports"], c["mod"], tb, rv, c["Nref"], c["start"], c["nof"], c["dmrs"], c["slot"],
                              c["scr"], c["n_scid"], c["snr_db"], c["delay"], c["rnti"], c["n_id"], c["bg"])
    for a in (tb, grid, rb, dm):
        a.setflags(write=False)
    return c, tb, grid, rb, dm
