"""GPU: miphy_pusch_demodulate_layers_batch_ex -- UCI repetition placeholders and the EVM sums above one layer. LLRs are bit-equal to the composition
through the device equaliser (miphy_channel_equalize_layers_batch) with the descrambling restated in tests/pusch_layers_uci_cases.py; the per-symbol EVM
sums are the restated float32 terms added in float64, within the rounding of the kernel's own additions; requesting EVM changes no LLR; without
placeholders and EVM the bytes are those of the plain entry point; the split of a job over the OFDM symbols changes neither LLRs nor sums; a one-layer job
gives the bytes and sums of miphy_pusch_demodulate_batch_ex."""
import numpy as np
import pytest

import pusch_layers_cases as PL
import pusch_layers_uci_cases as U

pytestmark = pytest.mark.gpu
SENTINEL, PAD = 99, 8
EVM_SENTINEL, EVM_PAD, PH_FRONT = -5.0, 3, 5
U24 = 2.0 ** -24


def equalize(ctx, c, grid, ce):
    """The data elements of a slot through miphy_channel_equalize_layers_batch: (x [L][n], nvar [L][n])."""
    import torch
    import miphy
    y, h = PL.extract(c, grid, ce)
    nl, npt, n = h.shape
    job = np.array([PL.equalizer_job(miphy, n, npt, nl, c["noise_var"], 1.0)], dtype=miphy.EqualizerJob)
    z = torch.zeros(nl * n, dtype=torch.complex64, device="cuda")
    v = torch.zeros(nl * n, dtype=torch.float32, device="cuda")
    ctx.channel_equalize_layers_batch(job, torch.from_numpy(y.reshape(-1)).cuda(), torch.from_numpy(h.reshape(-1)).cuda(), z, v)
    torch.cuda.synchronize()
    return z.cpu().numpy().reshape(nl, n), v.cpu().numpy().reshape(nl, n)


def one_bit_ack(miphy, c, g_re=20, rvd_re=40):
    """The placeholder list of a one-bit HARQ-ACK on allocation c, from miphy_ulsch_placeholders at the job's layer count."""
    rb, dm = PL.masks(c)
    k = c["nl"] * c["mod"]
    j = np.zeros(1, dtype=miphy.UlschDemuxJob)[0]
    j["mod"], j["nof_layers"], j["start_symbol"], j["nof_symbols"], j["dmrs_type"] = c["mod"], c["nl"], c["start"], c["nof"], 2 if c["type2"] else 1
    j["nof_cdm_groups_without_data"], j["dmrs_symbols_mask"], j["nof_prb"] = c["cdm"], sum(1 << int(s) for s in np.nonzero(dm)[0]), int(rb.sum())
    j["nof_harq_ack_rvd"], j["nof_enc_harq_ack_bits"], j["nof_harq_ack_bits"] = rvd_re * k, g_re * k, 1
    ph = miphy.ulsch_placeholders(j)
    assert ph.size == g_re and np.all(np.diff(ph.astype(int)) > 0)
    return ph


def run(ctx, slots, phs=None, evm=True, device_jobs=False, first_llr=0, entry="ex", pass_ph=True, jobs_edit=None, repeat_grid=False):
    """One batch. phs: per job a uint16 list or None, packed behind PH_FRONT foreign entries. Every codeword sits between PAD sentinel bytes, every job's
    14 sums between EVM_PAD sentinel floats. repeat_grid: every job reads the first slot's grid and estimate. -> (codewords, sums [n][14] or None)."""
    import torch
    import miphy
    n = len(slots)
    phs = phs or [None] * n
    jobs, grids, ces, spans = [], [], [], []
    ph_all = [np.full(PH_FRONT, 7, np.uint16)]
    go = co = 0
    lo, po = first_llr, PH_FRONT
    for i, (c, grid, ce) in enumerate(slots):
        lo += PAD
        j = PL.demod_job(miphy, c, go, co, 5 * i, lo)
        j["base"]["evm_offset"] = EVM_PAD + i * (14 + EVM_PAD)
        if phs[i] is not None:
            j["base"]["placeholders_offset"], j["base"]["nof_placeholders"] = po, phs[i].size
            ph_all.append(phs[i])
            po += phs[i].size
        jobs.append(j)
        spans.append((lo, int(j["base"]["nof_llr"])))
        if not (repeat_grid and i):
            grids.append(grid.reshape(-1))
            ces.append(ce.reshape(-1))
            go += grid.size
            co += ce.size
        if repeat_grid:
            go = co = 0
        lo += int(j["base"]["nof_llr"])
    lo += PAD
    jobs = np.array(jobs, dtype=miphy.PuschDemodLayersJob)
    if jobs_edit:
        jobs_edit(jobs)
    sc = np.zeros(5 * n, np.float32)
    sc[2::5] = [c["noise_var"] for c, _, _ in slots]
    out = torch.full((lo,), SENTINEL, dtype=torch.int8, device="cuda")
    sums = torch.full((EVM_PAD + n * (14 + EVM_PAD),), EVM_SENTINEL, dtype=torch.float32, device="cuda") if evm else None
    ph_d = torch.from_numpy(np.concatenate(ph_all).view(np.int16)).cuda() if pass_ph else None
    g_d, h_d, s_d = torch.from_numpy(np.concatenate(grids)).cuda(), torch.from_numpy(np.concatenate(ces)).cuda(), torch.from_numpy(sc).cuda()
    jd = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if device_jobs else jobs
    try:
        if entry == "ex":
            ctx.pusch_demodulate_layers_batch_ex(jd, g_d, h_d, s_d, out, ph_d, sums)
        elif entry == "plain":
            ctx.pusch_demodulate_layers_batch(jd, g_d, h_d, s_d, out)
        else:  # the one-layer entry point on the base jobs
            ctx.pusch_demodulate_batch_ex(np.ascontiguousarray(jobs["base"]), g_d, h_d, s_d, out, ph_d, sums)
    finally:
        torch.cuda.synchronize()
        run.last_out = out.cpu().numpy()
        run.last_sums = sums.cpu().numpy() if evm else None
    out = run.last_out
    keep = np.ones(out.size, bool)
    for o, m in spans:
        keep[o:o + m] = False
    assert np.all(out[keep] == SENTINEL), "bytes outside the codewords were written"
    got_sums = None
    if evm:
        s = run.last_sums
        body = s[EVM_PAD:].reshape(n, 14 + EVM_PAD)
        assert np.all(s[:EVM_PAD] == EVM_SENTINEL) and np.all(body[:, 14:] == EVM_SENTINEL), "floats outside the 14 sums of a job were written"
        got_sums = body[:, :14].copy()
    return [out[o:o + m] for o, m in spans], got_sums


def additions(c):
    """A: float32 additions on the longest path from a term to the stored sum of an OFDM symbol (csrc/pusch_demod.hip): L - 1 over the layers of an
    element, 6 in the wavefront shuffle tree, 3 over the four wavefronts, chunks - 1 in pusch_evm_reduce_kernel (its sum starts from 0)."""
    chunks = -(-len(c["prbs"]) * 12 // 256)
    return (c["nl"] - 1) + 6 + 3 + (chunks - 1)


def check(ctx, slots, phs, llrs, sums):
    for i, ((c, grid, ce), llr) in enumerate(zip(slots, llrs)):
        x, nv = equalize(ctx, c, grid, ce)
        exp = U.compose_llr(c, x, nv, () if phs[i] is None else phs[i])
        bad = np.nonzero(llr != exp)[0]
        assert bad.size == 0, (c["name"], c["nl"], c["npt"], c["mod"], bad.size, bad[:8], llr[bad[:8]], exp[bad[:8]])
        if sums is not None:
            ref = U.evm_symbol_sums(c, U.evm_terms(c, x, nv))
            tol = (additions(c) + 2) * U24
            rel = np.abs(sums[i].astype(np.float64) - ref) / np.where(ref > 0, ref, 1.0)
            print("EVM sums %s L=%d mod=%d: max relative error %.3g, bound %.3g" % (c["name"], c["nl"], c["mod"], rel.max(), tol))
            assert np.all(sums[i][ref == 0] == 0) and np.count_nonzero(ref) == c["nof"] - (len(c["dmrs"]) if c["cdm"] == 2 and not c["type2"] else 0)
            assert np.all(rel <= tol), (c["name"], rel.max(), tol)


def layered_slots(mod):
    """The geometry of test_every_modulation_on_every_layered_topology (tests/test_pusch_demod_layers_gpu.py)."""
    slots = []
    for k, (nl, npt) in enumerate(PL.LAYERED):
        c = PL.case("t%d%d" % (nl, npt), nl, npt, mod, compact=(k + mod // 2) % 2 == 0, cdm=1 + (k // 2 + mod // 4) % 2, rx_ports=(3, 0, 2, 1), seed=31 * mod + k,
                    rnti=0x1000 + k, n_id=100 + mod)
        slots.append((c, *PL.random_slot(c)))
    return slots


@pytest.mark.parametrize("device_jobs,first_llr", [(False, 0), (True, 0), (False, 1)])
@pytest.mark.parametrize("mod", [2, 4, 6, 8])
def test_placeholders_and_evm_on_every_layered_topology(ctx, mod, device_jobs, first_llr):
    """PRBs 2-9 and 14-17 of 24, symbols 2..13, the six layered topologies in one batch, every job with the placeholders of a one-bit HARQ-ACK.
    EVM: each per-symbol sum within (A + 2) 2^-24 relative of the float64 sum of the restated float32 terms, A = additions(c) = (L - 1) + 6 + 3 + 0
    float32 additions here (one chunk): 10 on two layers, 12 on four; the 2 covers a contracted product-sum."""
    import miphy
    slots = layered_slots(mod)
    phs = [one_bit_ack(miphy, c) for c, _, _ in slots]
    llrs, sums = run(ctx, slots, phs, evm=True, device_jobs=device_jobs, first_llr=first_llr)
    check(ctx, slots, phs, llrs, sums)
    without, _ = run(ctx, slots, phs, evm=False, device_jobs=device_jobs, first_llr=first_llr)
    assert all(np.array_equal(a, b) for a, b in zip(llrs, without)), "the LLRs do not depend on whether EVM is requested"


def test_evm_of_pi2_bpsk_and_the_plain_bytes(ctx):
    """mod 1 (no placeholders possible) with EVM; and for every modulation: no placeholders, both pointers NULL -> the bytes of the plain entry point."""
    slots = layered_slots(1)
    none = [None] * len(slots)
    llrs, sums = run(ctx, slots, evm=True)
    check(ctx, slots, none, llrs, sums)
    for mod in (1, 2, 4, 6, 8):
        slots = layered_slots(mod)
        a, _ = run(ctx, slots, evm=False, pass_ph=False)
        b, _ = run(ctx, slots, evm=False, entry="plain")
        c, _ = run(ctx, slots, evm=True)
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c)), mod


def test_symbol_parts_give_the_same_sums(ctx):
    """One job alone (the walk is cut into four parts of the OFDM symbols) and the same job 130 times on one grid (one part): identical LLRs and sums."""
    import miphy
    c = PL.case("parts", 3, 4, 6, prbs=range(2, 10), seed=5)
    slot = (c, *PL.random_slot(c))
    ph = one_bit_ack(miphy, c)
    llr1, sums1 = run(ctx, [slot], [ph])
    check(ctx, [slot], [ph], llr1, sums1)
    llrs, sums = run(ctx, [slot] * 130, [ph] * 130, repeat_grid=True)
    assert all(np.array_equal(l, llr1[0]) for l in llrs)
    assert all(s.tobytes() == sums1[0].tobytes() for s in sums)


def test_one_layer_job_in_a_mixed_batch(ctx):
    """LLRs and the 14 sums of a one-layer job are those of miphy_pusch_demodulate_batch_ex on its base record, byte for byte."""
    import miphy
    slots = []
    for k, (nl, npt, mod, compact) in enumerate([(2, 2, 4, True), (1, 2, 6, False), (4, 4, 8, True), (1, 4, 2, True), (1, 1, 1, True)]):
        c = PL.case("mix%d" % k, nl, npt, mod, compact=compact, seed=60 + k, n_id=k)
        slots.append((c, *PL.random_slot(c)))
    phs = [one_bit_ack(miphy, c) if c["mod"] >= 2 else None for c, _, _ in slots]
    for device_jobs in (False, True):
        llrs, sums = run(ctx, slots, phs, device_jobs=device_jobs)
        check(ctx, slots, phs, llrs, sums)
        for i, s in enumerate(slots):
            if s[0]["nl"] == 1:
                l1, s1 = run(ctx, [s], [phs[i]], entry="one_layer")
                assert np.array_equal(llrs[i], l1[0]) and sums[i].tobytes() == s1[0].tobytes(), s[0]["name"]


@pytest.mark.parametrize("what", ["null_list", "mod_1"])
def test_rejections(ctx, what):
    """nof_placeholders != 0 without a list, or at mod 1: from the host RuntimeError and nothing written; device-resident: skipped, neighbours intact."""
    mod = 1 if what == "mod_1" else 4
    slots = []
    for k in range(3):
        c = PL.case("r%d" % k, 3, 3, mod, compact=False, prbs=range(2, 6), seed=90 + k)
        slots.append((c, *PL.random_slot(c)))
    pass_ph = what != "null_list"

    def edit(jobs):
        jobs["base"]["nof_placeholders"][1], jobs["base"]["placeholders_offset"][1] = 2, 1

    good_llr, good_sums = run(ctx, slots, pass_ph=pass_ph)
    with pytest.raises(RuntimeError, match="placeholders need the list and a modulation order of at least 2"):
        run(ctx, slots, pass_ph=pass_ph, jobs_edit=edit)
    assert np.all(run.last_out == SENTINEL) and np.all(run.last_sums == EVM_SENTINEL)
    llr, sums = run(ctx, slots, pass_ph=pass_ph, jobs_edit=edit, device_jobs=True)
    assert np.array_equal(llr[0], good_llr[0]) and np.array_equal(llr[2], good_llr[2]) and np.all(llr[1] == SENTINEL)
    assert sums[0].tobytes() == good_sums[0].tobytes() and sums[2].tobytes() == good_sums[2].tobytes() and np.all(sums[1] == EVM_SENTINEL)
