"""GPU: miphy_pusch_demodulate_layers_mmse_batch[_ex], one codeword on 1..4 layers through MMSE-IRC. The LLRs must be the bytes of the composition
extraction (pusch_layers_cases.extract) -> mmse_single per PRG (pusch_mmse_cases, the float32 restatement of csrc/mmse_device.h) -> the oracle's
soft demapper -> descrambling; with placeholders and EVM, of the composition restated in tests/pusch_layers_uci_cases.py. The scalars pointer is
NULL throughout: the scalar noise variance is not read."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_uci_cases as U
import pusch_mmse_cases as MM
from test_pusch_demod_layers_uci_gpu import additions, one_bit_ack

pytestmark = pytest.mark.gpu
SENTINEL, PAD = 99, 8
EVM_SENTINEL, EVM_PAD, PH_FRONT = -5.0, 3, 5
U24 = 2.0 ** -24
PRGS = (0, 1, 4)


def slot(c, prg, seed=None):
    """(case, grid, estimate, covariance matrices [PRG][P][P], prg_size): a random slot and white noise 0.02 plus interferers up to 20 dB above it."""
    rng = np.random.default_rng(1000 + (c["seed"] if seed is None else seed))
    grid, ce = PL.random_slot(c)
    cov = np.stack([MM.coloured(rng, c["npt"], 0.02, rng.uniform(0, 100, 1 + k % 2)) for k in range(MM.nof_prg(len(c["prbs"]), prg))]).astype(np.complex64)
    return c, grid, ce, cov, prg


def run(ctx, slots, phs=None, evm=False, device_jobs=False, first_llr=0, ex=False, jobs_edit=None, repeat=1):
    """One batch; repeat: the one slot that many times on one grid. Every codeword sits between PAD sentinel bytes, every job's 14 sums between
    EVM_PAD sentinel floats. -> (codewords, sums [n][14] or None)."""
    import torch
    import miphy
    if repeat > 1:
        slots, phs = slots * repeat, (phs * repeat if phs else None)
    n = len(slots)
    phs = phs or [None] * n
    jobs, grids, ces, covs, spans = [], [], [], [], []
    ph_all = [np.full(PH_FRONT, 7, np.uint16)]
    go = co = vo = 0
    lo, po = first_llr, PH_FRONT
    for i, (c, grid, ce, cov, prg) in enumerate(slots):
        lo += PAD
        j = MM.demod_mmse_job(miphy, c, prg, go, co, vo, lo)
        j["base"]["base"]["evm_offset"] = EVM_PAD + i * (14 + EVM_PAD)
        if phs[i] is not None:
            j["base"]["base"]["placeholders_offset"], j["base"]["base"]["nof_placeholders"] = po, phs[i].size
            ph_all.append(phs[i])
            po += phs[i].size
        jobs.append(j)
        nllr = int(j["base"]["base"]["nof_llr"])
        spans.append((lo, nllr))
        if repeat == 1 or i == 0:
            grids.append(grid.reshape(-1))
            ces.append(ce.reshape(-1))
            covs.append(cov.reshape(-1))
        if repeat == 1:
            go, co, vo = go + grid.size, co + ce.size, vo + cov.size
        lo += nllr
    lo += PAD
    jobs = np.array(jobs, dtype=miphy.PuschDemodMmseJob)
    if jobs_edit:
        jobs_edit(jobs)
    out = torch.full((lo,), SENTINEL, dtype=torch.int8, device="cuda")
    sums = torch.full((EVM_PAD + n * (14 + EVM_PAD),), EVM_SENTINEL, dtype=torch.float32, device="cuda") if evm else None
    ph_d = torch.from_numpy(np.concatenate(ph_all).view(np.int16)).cuda() if ex else None
    g_d, h_d, c_d = (torch.from_numpy(np.concatenate(a)).cuda() for a in (grids, ces, covs))
    jd = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if device_jobs else jobs
    try:
        if ex or evm:
            ctx.pusch_demodulate_layers_mmse_batch_ex(jd, g_d, h_d, c_d, out, ph_d, sums)
        else:
            ctx.pusch_demodulate_layers_mmse_batch(jd, g_d, h_d, c_d, out)
    finally:
        torch.cuda.synchronize()
        run.last_out = out.cpu().numpy()
    out = run.last_out
    keep = np.ones(out.size, bool)
    for o, m in spans:
        keep[o:o + m] = False
    assert np.all(out[keep] == SENTINEL), "bytes outside the codewords were written"
    got_sums = None
    if evm:
        s = sums.cpu().numpy()
        body = s[EVM_PAD:].reshape(n, 14 + EVM_PAD)
        assert np.all(s[:EVM_PAD] == EVM_SENTINEL) and np.all(body[:, 14:] == EVM_SENTINEL), "floats outside the 14 sums of a job were written"
        got_sums = body[:, :14].copy()
    return [out[o:o + m] for o, m in spans], got_sums


def check(slots, llrs, phs=None, sums=None):
    phs = phs or [None] * len(slots)
    for i, ((c, grid, ce, cov, prg), llr) in enumerate(zip(slots, llrs)):
        x, nv = MM.mmse_on_allocation(c, grid, ce, cov, prg)
        exp = U.compose_llr(c, x, nv, () if phs[i] is None else phs[i])
        if phs[i] is None:
            assert np.array_equal(exp, PL.compose_llr(c, x, nv))
        assert llr.size == exp.size
        bad = np.nonzero(llr != exp)[0]
        assert bad.size == 0, (c["name"], c["nl"], c["npt"], c["mod"], prg, bad.size, bad[:8], llr[bad[:8]], exp[bad[:8]])
        if sums is not None:
            ref = U.evm_symbol_sums(c, U.evm_terms(c, x, nv))
            tol = (additions(c) + 2) * U24
            rel = np.abs(sums[i].astype(np.float64) - ref) / np.where(ref > 0, ref, 1.0)
            assert np.all(sums[i][ref == 0] == 0) and np.all(rel <= tol), (c["name"], rel.max(), tol)


def topology_slots(mod):
    """The ten topologies, one layer included: PRBs 2-9 and 14-17 of 24, symbols 2..13, DM-RS on 2 and 11, alternating the compact and the per-symbol
    estimate, one and two CDM groups without data, DM-RS type 2 on every third job, receive ports in the order 3, 0, 2, 1, prg_size 0, 1 and 4 in turn."""
    slots = []
    for k, (nl, npt) in enumerate(PL.TOPOLOGIES):
        c = PL.case("t%d%d" % (nl, npt), nl, npt, mod, compact=(k + mod // 2) % 2 == 0, cdm=1 + (k // 2 + mod // 4) % 2, type2=int(k % 3 == 2), rx_ports=(3, 0, 2, 1),
                    seed=37 * mod + k, rnti=0x2000 + k, n_id=200 + mod)
        slots.append(slot(c, PRGS[(k + mod) % 3]))
    return slots


@pytest.mark.parametrize("device_jobs,first_llr", [(False, 0), (True, 0), (False, 1)])
@pytest.mark.parametrize("mod", [1, 2, 4, 6, 8])
def test_every_modulation_on_every_topology(ctx, mod, device_jobs, first_llr):
    """first_llr = 1 moves every codeword by one byte: those that were aligned to their stores take the byte path and the other way round."""
    slots = topology_slots(mod)
    assert {s[4] for s in slots} == set(PRGS) and {s[0]["compact"] for s in slots} == {True, False} and {s[0]["type2"] for s in slots} == {0, 1}
    check(slots, run(ctx, slots, device_jobs=device_jobs, first_llr=first_llr)[0])


def test_mixed_batch_equals_each_job_alone(ctx):
    slots = []
    for k, (nl, npt, mod, compact, prg) in enumerate([(1, 2, 8, True, 4), (3, 4, 6, False, 0), (1, 4, 6, False, 1), (2, 2, 4, True, 1), (4, 4, 2, True, 4),
                                                      (1, 1, 1, True, 0), (2, 4, 8, False, 4)]):
        slots.append(slot(PL.case("mix%d" % k, nl, npt, mod, compact=compact, seed=150 + k, n_id=k), prg))
    for device_jobs in (False, True):
        got = run(ctx, slots, device_jobs=device_jobs)[0]
        check(slots, got)
        for s, llr in zip(slots, got):
            assert np.array_equal(llr, run(ctx, [s])[0][0]), s[0]["name"]


def test_widest_grid_once(ctx):
    """273 PRBs (thirteen chunks), four layers on four ports, 256QAM, a matrix for every four PRBs (69 of them); and one layer on two ports."""
    for nl, npt, prg in ((4, 4, 4), (1, 2, 0)):
        c = PL.case("widest", nl, npt, 8, nprb_grid=273, prbs=range(273), start=0, nof=14, dmrs=(2,), seed=4, rnti=0xFFFF, n_id=1023)
        slots = [slot(c, prg)]
        check(slots, run(ctx, slots, device_jobs=True)[0])


@pytest.mark.parametrize("nl,npt,mod,compact,prg", [(2, 4, 6, True, 4), (1, 2, 4, False, 1)])
def test_placeholders_and_evm(ctx, nl, npt, mod, compact, prg):
    """The placeholders of a one-bit HARQ-ACK and the EVM sums against the composition: each per-symbol sum within (A + 2) 2^-24 relative of the
    float64 sum of the restated float32 terms (A = additions(c), tests/test_pusch_demod_layers_uci_gpu.py). Requesting EVM changes no LLR; the job
    alone (its walk is cut into four parts of the OFDM symbols) and 130 times in one batch (one part) gives the same LLRs and the same sums, bit for bit."""
    import miphy
    c = PL.case("ex", nl, npt, mod, compact=compact, prbs=range(2, 10), seed=5 + nl)
    s = slot(c, prg)
    ph = one_bit_ack(miphy, c)
    llr1, sums1 = run(ctx, [s], [ph], evm=True, ex=True)
    check([s], llr1, [ph], sums1)
    assert np.array_equal(run(ctx, [s], [ph], evm=False, ex=True)[0][0], llr1[0])
    llrs, sums = run(ctx, [s], [ph], evm=True, ex=True, repeat=130)
    assert all(np.array_equal(l, llr1[0]) for l in llrs)
    assert all(x.tobytes() == sums1[0].tobytes() for x in sums)
    plain = run(ctx, [s])[0][0]  # no placeholders, no EVM: the plain entry point and _ex with both pointers NULL agree
    assert np.array_equal(plain, run(ctx, [s], evm=True)[0][0])


def test_dead_column_and_singular_matrix(ctx):
    """A zero channel column and a PRG whose matrix is singular (all ones: a pivot is exactly 0): LLR 0 on ALL layers of those elements."""
    c = PL.case("dead", 3, 4, 4, compact=True, seed=77)
    s = slot(c, 4)
    sc_dead = 3 * 12 + 4  # (PRB 3: PRG 0)
    s[2][c["nl"] - 1, :, :, sc_dead] = 0
    s[3][2] = 0.25  # PRG 2: allocated PRBs 8 .. 11 = PRBs 14 .. 17
    got = run(ctx, [s])[0]
    check([s], got)
    sy, sc = PL.data_positions(c)
    dead = (sc == sc_dead) | (sc // 12 >= 14)
    llr = got[0].reshape(-1, c["nl"] * c["mod"])
    assert np.all(llr[dead] == 0) and np.any(llr[~dead] != 0)


def _set(field, value, depth):
    def edit(jobs):
        rec = jobs
        for _ in range(depth):
            rec = rec["base"]
        rec[field][1] = value
    return edit


REJECTIONS = [("layers_0", _set("nof_tx_layers", 0, 1)), ("layers_5", _set("nof_tx_layers", 5, 1)), ("layers_above_ports", _set("nof_rx_ports", 2, 2)),
              ("mod_3", _set("mod", 3, 2)), ("nof_llr", _set("nof_llr", 8, 2)), ("placeholders_without_list", _set("nof_placeholders", 1, 2))]


@pytest.mark.parametrize("name,edit", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_rejections(ctx, name, edit):
    """One job per rule between two good ones: from the host MIPHY_EINVAL and nothing written; on the device it is skipped, its neighbours intact."""
    slots = [slot(PL.case("r%d" % k, 3, 3, 4, compact=False, prbs=range(2, 6), seed=190 + k), 1) for k in range(3)]
    good = run(ctx, slots)[0]
    with pytest.raises(RuntimeError, match="miphy error -1"):
        run(ctx, slots, jobs_edit=edit)
    assert np.all(run.last_out == SENTINEL), "a refused batch writes nothing"
    got = run(ctx, slots, device_jobs=True, jobs_edit=edit)[0]
    assert np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2])
    assert np.all(got[1] == SENTINEL)
