"""CPU: the host PUSCH transmitter of tests/pusch_tx.py, received by the oracle chain alone (estimator -> demodulator -> decoder). Every slot
that tests/test_pusch_proc_gpu.py feeds to the device gives its stated verdict here, without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import pusch_tx as T


@pytest.mark.parametrize("name", [c["name"] for c in T.PROC_CASES])
def test_processor_slots_give_their_verdict_in_the_oracle(name):
    c, tb, grid, rb, dm = T.build(name)
    unsel = [p for p in range(4) if p not in c["ports"]]
    assert np.isfinite(grid[list(c["ports"])]).all() and np.isnan(grid[unsel]).all()
    r = T.oracle_receive(c, grid, rb, dm)
    assert r["ok"] == c["ok"], (name, r["iters"])
    if c["ok"]:
        assert np.array_equal(r["tb"], tb)
        assert r["iters"][1] <= 2, (name, r["iters"])  # margin: far from the six iterations allowed
    else:
        assert r["iters"] == (6, 6) and not np.array_equal(r["tb"], tb)
    # every selected port went through its own channel: RSRP (of the DM-RS, +3 dB) and the delay, per logical port
    delays = list(c["delay"]) if np.ndim(c["delay"]) else [c["delay"]] * len(c["ports"])
    tap = 1.0 / (4096 * 15000.0 * (1 << c["mu"]))
    for k, (p, d) in enumerate(zip(c["ports"], delays)):
        want = abs(T.port_channel(p, 1, 0.0)[0]) ** 2 * T.DMRS_AMPLITUDE ** 2
        assert abs(r["sc"][k, 0, 0] / want - 1) < 0.05 + 10 ** (-c["snr_db"] / 10), (name, k, r["sc"][k, 0, 0], want)
        assert abs(r["sc"][k, 0, 4] - d * tap) <= 1.01 * tap, (name, k, r["sc"][k, 0, 4], d * tap)


def test_harq_sequence_fails_then_decodes_in_the_oracle():
    dec, oks = None, []
    for t, (slot, rv) in enumerate(T.HARQ_SEQUENCE):
        c, tb, grid, rb, dm = T.build(T.HARQ_CASE["name"], slot, rv)
        r = T.oracle_receive(c, grid, rb, dm, rv, t == 0, dec)
        dec = r["decoder"]
        oks.append(r["ok"])
        if r["ok"]:
            assert np.array_equal(r["tb"], tb)
            break
    assert oks == [False, False, True], oks


@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_noiseless_slot_demodulates_to_the_codeword(mod):
    """The mapping itself, without the estimator: a slot without noise, equalised with the channel it went through, gives back the encoder's bits."""
    rng = np.random.default_rng(mod)
    nprb, prbs, ports, start, nof, dmrs = 12, [1, 2, 3, 7, 11], (2, 0), 1, 11, (3, 9, 13)  # DM-RS symbol 13 lies outside the allocation
    tb = rng.integers(0, 256, 40, dtype=np.uint8)
    grid, rb, dm = T.pusch_slot(rng, nprb, prbs, ports, mod, tb, 2, 0, start, nof, dmrs, 5, 33, 1, 200.0, (4.0, -2.0), 0x77, 5, 2)
    assert list(np.nonzero(dm)[0]) == [3, 9] and list(np.nonzero(rb)[0]) == prbs
    nre = T.nof_data_re(rb, dm, start, nof)
    assert nre == 5 * 12 * 9
    h = np.stack([np.tile(T.port_channel(p, nprb * 12, d), (14, 1)) for p, d in zip(ports, (4.0, -2.0))]).astype(np.complex64)
    llr = O.o_pusch_demodulate(0x77, 5, mod, start, nof, dm, 0, 2, rb, grid[list(ports)], h, 0.01)[0]
    assert np.array_equal((llr < 0).astype(np.uint8), O.o_pdsch_encode(2, 2, mod, 0, 1, nre, tb))
    # the DM-RS the estimator expects, through the same channel: the estimate at the pilots' subcarriers (between them it interpolates over the
    # concatenated PRBs, which a delay across a gap of the allocation does not survive)
    ce, sc = O.o_dmrs_pusch_estimate(1, 5, 0, 33, 1, T.CHEST_SCALING, dm, rb, start, nof, 1, grid[list(ports)])
    m = np.repeat(rb.astype(bool), 12) & (np.arange(nprb * 12) % 2 == 0)
    assert np.abs(ce[0][:, start:, m] - h[:, start:start + nof, m]).max() < 2e-3
