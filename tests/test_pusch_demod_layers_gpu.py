"""GPU: miphy_pusch_demodulate_layers_batch, one codeword on 1..4 transmit layers. The LLRs must be those of the composition that
tests/pusch_layers_cases.py states (extraction, L x P zero forcing, layer demapping, the oracle's soft demapper and Gold sequence), with the
equalised symbols taken from miphy_channel_equalize_layers_batch on the extracted elements -- the device composition: both kernels call one
function, so they must agree to the bit. Where the oracle has an equaliser of its own (one layer, 2 x 2) the LLRs must also be those of the
composition through orc_channel_equalize."""
import numpy as np
import pytest

import oracle_lib as O
import pusch_layers_cases as PL

pytestmark = pytest.mark.gpu
SENTINEL = 99
PAD = 8


def device_equalize(ctx):
    """An `equalize` for PL.expected_llr that runs miphy_channel_equalize_layers_batch."""
    import torch
    import miphy

    def run(y, h, noise_var, tx):
        nl, npt, n = h.shape
        job = np.array([PL.equalizer_job(miphy, n, npt, nl, noise_var, tx)], dtype=miphy.EqualizerJob)
        z = torch.zeros(nl * n, dtype=torch.complex64, device="cuda")
        v = torch.zeros(nl * n, dtype=torch.float32, device="cuda")
        ctx.channel_equalize_layers_batch(job, torch.from_numpy(y.reshape(-1)).cuda(), torch.from_numpy(h.reshape(-1)).cuda(), z, v)
        torch.cuda.synchronize()
        return z.cpu().numpy().reshape(nl, n), v.cpu().numpy().reshape(nl, n)
    return run


def oracle_equalize(y, h, noise_var, tx):
    return O.o_channel_equalize(y, h, noise_var, tx)


def run_batch(ctx, slots, device_jobs=False, first_llr=0, entry="layers", jobs_edit=None):
    """slots: list of (case, grid, ce). One batch; every codeword has PAD sentinel bytes in front of it and behind it.
    Returns the codewords, and checks the sentinels."""
    import torch
    import miphy
    jobs, grids, ces, spans = [], [], [], []
    go = co = 0
    lo = first_llr
    for i, (c, grid, ce) in enumerate(slots):
        lo += PAD
        j = PL.demod_job(miphy, c, go, co, 5 * i, lo)
        jobs.append(j)
        spans.append((lo, int(j["base"]["nof_llr"])))
        grids.append(grid.reshape(-1))
        ces.append(ce.reshape(-1))
        go += grid.size
        co += ce.size
        lo += int(j["base"]["nof_llr"])
    lo += PAD
    jobs = np.array(jobs, dtype=miphy.PuschDemodLayersJob)
    if jobs_edit:
        jobs_edit(jobs)
    sc = np.zeros(5 * len(slots), np.float32)
    sc[2::5] = [c["noise_var"] for c, _, _ in slots]
    out = torch.full((lo,), SENTINEL, dtype=torch.int8, device="cuda")
    g_d, h_d, s_d = torch.from_numpy(np.concatenate(grids)).cuda(), torch.from_numpy(np.concatenate(ces)).cuda(), torch.from_numpy(sc).cuda()
    if entry == "layers":
        ctx.pusch_demodulate_layers_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if device_jobs else jobs, g_d, h_d, s_d, out)
    else:  # the one-layer entry point on the base jobs
        ctx.pusch_demodulate_batch(np.ascontiguousarray(jobs["base"]), g_d, h_d, s_d, out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    keep = np.ones(out.size, bool)
    for o, n in spans:
        keep[o:o + n] = False
    assert np.all(out[keep] == SENTINEL), "bytes outside the codewords were written"
    return [out[o:o + n] for o, n in spans]


def check(ctx, slots, got):
    eq = device_equalize(ctx)
    for (c, grid, ce), llr in zip(slots, got):
        exp = PL.expected_llr(c, grid, ce, eq)
        assert llr.size == exp.size
        bad = np.nonzero(llr != exp)[0]
        assert bad.size == 0, (c["name"], c["nl"], c["npt"], c["mod"], bad.size, bad[:8], llr[bad[:8]], exp[bad[:8]])
        if c["nl"] == 1 or (c["nl"], c["npt"]) == (2, 2):
            assert np.array_equal(llr, PL.expected_llr(c, grid, ce, oracle_equalize)), ("oracle", c["name"])


@pytest.mark.parametrize("device_jobs,first_llr", [(False, 0), (True, 0), (False, 1)])
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_every_modulation_on_every_layered_topology(ctx, mod, device_jobs, first_llr):
    """24 PRB grid, PRBs 2-9 and 14-17, symbols 2..13 with DM-RS on 2 and 11; the six layered topologies in one batch, alternating the compact and
    the per-symbol estimate and one and two CDM groups without data, receive ports in the order 3, 0, 2, 1. first_llr = 1 moves
    every codeword by one byte: those that were aligned to their stores take the byte path and the other way round."""
    slots = []
    for k, (nl, npt) in enumerate(PL.LAYERED):
        c = PL.case("t%d%d" % (nl, npt), nl, npt, mod, compact=(k + mod // 2) % 2 == 0, cdm=1 + (k // 2 + mod // 4) % 2, rx_ports=(3, 0, 2, 1), seed=31 * mod + k,
                    rnti=0x1000 + k, n_id=100 + mod)
        slots.append((c, *PL.random_slot(c)))
    check(ctx, slots, run_batch(ctx, slots, device_jobs, first_llr))


@pytest.mark.parametrize("nl,npt,mod,compact", [(2, 3, 6, True), (3, 3, 4, False), (4, 4, 8, True), (2, 2, 1, False)])
def test_dmrs_type_2(ctx, nl, npt, mod, compact):
    c = PL.case("type2", nl, npt, mod, type2=1, cdm=2, compact=compact, dmrs=(2,), seed=nl + mod)
    slots = [(c, *PL.random_slot(c))]
    check(ctx, slots, run_batch(ctx, slots))


def test_sequence_longer_than_one_piece(ctx):
    """80 PRB x 14 symbols, four layers, 256QAM: 399 360 sequence bits, more than one piece and more than the one-layer table."""
    c = PL.case("long", 4, 4, 8, nprb_grid=80, prbs=range(80), start=0, nof=14, dmrs=(2,), seed=3)
    assert PL.nof_re(c) * 4 * 8 == 399360
    slots = [(c, *PL.random_slot(c))]
    check(ctx, slots, run_batch(ctx, slots))


def test_widest_grid_once(ctx):
    c = PL.case("widest", 4, 4, 8, nprb_grid=273, prbs=range(273), start=0, nof=14, dmrs=(2,), seed=4, rnti=0xFFFF, n_id=1023)
    slots = [(c, *PL.random_slot(c))]
    check(ctx, slots, run_batch(ctx, slots, device_jobs=True))


def test_mixed_batch_equals_each_job_alone_and_the_one_layer_entry_point(ctx):
    slots = []
    for k, (nl, npt, mod, compact) in enumerate([(1, 1, 8, True), (3, 4, 6, False), (1, 4, 6, False), (2, 2, 4, True), (4, 4, 2, True), (1, 2, 1, True),
                                                 (2, 4, 8, False)]):
        c = PL.case("mix%d" % k, nl, npt, mod, compact=compact, seed=50 + k, n_id=k)
        slots.append((c, *PL.random_slot(c)))
    for device_jobs in (False, True):
        got = run_batch(ctx, slots, device_jobs)
        check(ctx, slots, got)
        for s, llr in zip(slots, got):
            assert np.array_equal(llr, run_batch(ctx, [s])[0]), s[0]["name"]
            if s[0]["nl"] == 1:
                assert np.array_equal(llr, run_batch(ctx, [s], entry="one_layer")[0]), s[0]["name"]


@pytest.mark.parametrize("nl,npt,mod,compact", [(2, 2, 4, True), (3, 4, 8, False), (4, 4, 6, True)])
def test_dead_column_and_non_finite_samples(ctx, nl, npt, mod, compact):
    """A zero channel column: LLR 0 on ALL layers of those elements; one +inf and one NaN grid sample: what the composition gives."""
    c = PL.case("dead", nl, npt, mod, compact=compact, seed=70 + nl)
    grid, ce = PL.random_slot(c)
    sc_dead = 3 * 12 + 4
    ce[nl - 1, :, :, sc_dead] = 0
    grid[c["rx_ports"][0], 5, 4 * 12 + 1] = np.inf
    grid[c["rx_ports"][npt - 1], 6, 15 * 12 + 7] = np.nan
    slots = [(c, grid, ce)]
    got = run_batch(ctx, slots)
    check(ctx, slots, got)
    sy, sc = PL.data_positions(c)
    dead = np.nonzero(sc == sc_dead)[0]
    assert dead.size == 10  # every symbol without DM-RS
    llr = got[0].reshape(-1, nl * mod)
    assert np.all(llr[dead] == 0) and np.any(llr[np.setdiff1d(np.arange(sy.size), dead)] != 0)


def _set(field, value, base=True):
    def edit(jobs):
        (jobs["base"] if base else jobs)[field][1] = value
    return edit


def _two_ports(jobs):
    jobs["base"]["nof_rx_ports"][1] = 2  # three layers on two ports


REJECTIONS = [
    ("layers_0", _set("nof_tx_layers", 0, False)), ("layers_5", _set("nof_tx_layers", 5, False)), ("layers_above_ports", _two_ports),
    ("ports_5", _set("nof_rx_ports", 5)), ("mod_3", _set("mod", 3)), ("time", _set("nof_symbols", 13)), ("estimate_short", _set("ce_nof_symbols", 13)),
    ("dmrs_type", _set("dmrs_type", 3)), ("cdm_groups", _set("nof_cdm_groups_without_data", 3)), ("grid_width", _set("grid_nof_prb", 276)),
    ("n_id", _set("n_id", 1024)), ("rnti", _set("rnti", 65536)), ("placeholders", _set("nof_placeholders", 1)), ("nof_llr", _set("nof_llr", 8)),
]


@pytest.mark.parametrize("name,edit", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ctx, name, edit):
    """One job per rule between two good ones: from the host MIPHY_EINVAL and nothing written; on the device it is skipped, its neighbours intact."""
    slots = []
    for k in range(3):
        c = PL.case("r%d" % k, 3, 3, 4, compact=False, prbs=range(2, 6), seed=90 + k)
        slots.append((c, *PL.random_slot(c)))
    good = run_batch(ctx, slots)
    with pytest.raises(RuntimeError):
        run_batch(ctx, slots, jobs_edit=edit)
    import torch
    torch.cuda.synchronize()
    # (run_batch raised before it looked at the output: look at the device-resident form, where the output comes back)
    got = run_batch(ctx, slots, device_jobs=True, jobs_edit=edit)
    assert np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2])
    assert np.all(got[1] == SENTINEL)


def test_host_rejection_writes_nothing(ctx):
    import torch
    import miphy
    c = PL.case("r", 2, 2, 4, prbs=range(2, 6))
    grid, ce = PL.random_slot(c)
    jobs = np.array([PL.demod_job(miphy, c), PL.demod_job(miphy, c)], dtype=miphy.PuschDemodLayersJob)
    jobs["nof_tx_layers"][1] = 3
    out = torch.full((int(jobs["base"]["nof_llr"][0]) + 8,), SENTINEL, dtype=torch.int8, device="cuda")
    sc = torch.full((5,), 0.05, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):
        ctx.pusch_demodulate_layers_batch(jobs, torch.from_numpy(grid.reshape(-1)).cuda(), torch.from_numpy(ce.reshape(-1)).cuda(), sc, out)
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
