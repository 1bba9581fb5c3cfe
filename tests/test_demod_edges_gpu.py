"""GPU: the soft demapper of the PUSCH demodulator on the crafted edges of tests/demod_edges.py -- interval boundaries, rounding ties, the clip,
zeros and subnormals, non-finite symbols and abnormal noise variances -- through every choice of form (packed, fast, exact) the kernels make:
per element (finite symbol, finite reciprocal variance), per OFDM symbol (alignment of the LLR pointer) and per job (compact estimate, ports, EVM,
placeholders, pi/2-BPSK, one layer or several). Every case: all LLRs equal to the oracle's, and every byte outside the codewords untouched.
tests/test_demod_edges.py holds the generator to its census and shows that the crafted symbols and variances arrive at the demapper bit for bit."""
import functools

import numpy as np
import pytest

import demod_edges as DE
import oracle_lib as O
import pusch_layers_cases as PL

pytestmark = pytest.mark.gpu
SENTINEL = 99
QAM = (2, 4, 6, 8)


@functools.lru_cache(maxsize=None)
def _lays(mod, kind, noise_override=None):
    """The crafted set of a modulation as jobs, one per noise base. kind: 'deep' compact estimate on one port, 'compact2' compact estimate on two
    ports (the second estimate is 0), 'full' 14-symbol estimate carrying the noise classes too. noise_override: the job noise variance instead of
    the base. Each with its oracle LLRs (shared by the tests; never modified)."""
    out = []
    for n, (base, el) in enumerate(DE.bases(mod, with_noise_classes=(kind == "full"))):
        lay = DE.lay(mod, el, base if noise_override is None else noise_override, kind != "full", ports=2 if kind == "compact2" else 1, rnti=0x4601 + n,
                     n_id=77 + mod)
        lay["exp"] = O.o_pusch_demodulate(*lay["args"])[0]
        lay["exp"].setflags(write=False)
        out.append(lay)
    return out


def _offsets(sizes, odd):
    """Codeword starts with at least eight guard bytes in between: multiples of 8, or (odd) 1, 3, 5, 7 past one in turn."""
    offs, cur = [], 8
    for n, sz in enumerate(sizes):
        cur = (cur + 7) // 8 * 8 + (2 * (n % 4) + 1 if odd else 0)
        offs.append(cur)
        cur += sz + 8
    return offs, cur


def _run(ctx, lays, odd, device_jobs, placeholders=None, evm=False):
    """One batch of the jobs `lays`; returns the LLR buffer. placeholders: per job a sorted uint16 list (then, or with evm, the _ex entry point)."""
    import torch
    import miphy
    offs, total = _offsets([lay["exp"].size for lay in lays], odd)
    jobs = np.zeros(len(lays), dtype=miphy.PuschDemodJob)
    go = co = po = 0
    for i, (lay, lo) in enumerate(zip(lays, offs)):
        j = jobs[i]
        j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = lay["rnti"], lay["n_id"], lay["mod"], lay["ports"], lay["start"], lay["nof"]
        j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 1, lay["cdm"], 14, int(lay["compact"])
        j["rx_ports"] = [0, 1, 2, 3]
        j["dmrs_symbols_mask"] = sum(1 << int(s) for s in np.nonzero(lay["dm"])[0])
        j["grid_nof_prb"] = lay["rb"].size
        j["rb_mask"] = PL.mask_words(lay["rb"])
        j["grid_offset"], j["ce_offset"], j["scalars_offset"], j["llr_offset"] = go, co, 5 * i, lo
        j["nof_llr"] = lay["n_re"] * lay["mod"]
        if placeholders is not None:
            j["placeholders_offset"], j["nof_placeholders"] = po, placeholders[i].size
            po += placeholders[i].size
        j["evm_offset"] = 14 * i
        go += lay["grid"].size
        co += lay["ce"].size
    sc = np.zeros(5 * len(lays), np.float32)
    sc[2::5] = [lay["noise_var"] for lay in lays]
    g = torch.from_numpy(np.concatenate([lay["grid"].reshape(-1) for lay in lays])).cuda()
    h = torch.from_numpy(np.concatenate([lay["ce"].reshape(-1) for lay in lays])).cuda()
    out = torch.full((total,), SENTINEL, dtype=torch.int8, device="cuda")
    recs = torch.from_numpy(jobs.view(np.uint8)).cuda() if device_jobs else jobs
    if placeholders is None and not evm:
        ctx.pusch_demodulate_batch(recs, g, h, torch.from_numpy(sc).cuda(), out)
    else:
        ph_d = torch.from_numpy(np.concatenate(list(placeholders) + [np.zeros(1, np.uint16)]).view(np.int16)).cuda() if placeholders is not None else None
        evm_d = torch.zeros(14 * len(lays), dtype=torch.float32, device="cuda") if evm else None
        ctx.pusch_demodulate_batch_ex(recs, g, h, torch.from_numpy(sc).cuda(), out, ph_d, evm_d)
    torch.cuda.synchronize()
    return out.cpu().numpy(), offs


def _check(out, offs, expected, what=""):
    used = np.zeros(out.size, bool)
    for n, (lo, exp) in enumerate(zip(offs, expected)):
        used[lo:lo + exp.size] = True
        got = out[lo:lo + exp.size]
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (what, "job", n, "LLRs that differ", bad.size, "first at", bad[:8], "got", got[bad[:8]], "oracle", exp[bad[:8]])
    assert np.all(out[~used] == SENTINEL), (what, "bytes outside the codewords were written")


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("mod", QAM)
def test_deep_walk(ctx, mod, odd, device_jobs):
    """Compact estimate, one port, no EVM, no placeholders: aligned codewords take the packed store, odd ones the byte path through the fast and the
    exact form."""
    lays = _lays(mod, "deep")
    out, offs = _run(ctx, lays, odd, device_jobs)
    _check(out, offs, [lay["exp"] for lay in lays])


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("kind", ["compact2", "full"])
@pytest.mark.parametrize("mod", QAM)
def test_general_walk(ctx, mod, kind, device_jobs):
    """The general walk: the compact estimate on two ports (the second estimate is 0: the values still pass exactly), and the 14-symbol estimate,
    where 2^k and so the variance change from element to element and every noise class rides along. Aligned and odd codewords in one batch."""
    lays = _lays(mod, kind)
    for odd in (False, True):
        out, offs = _run(ctx, lays, odd, device_jobs)
        _check(out, offs, [lay["exp"] for lay in lays], odd)


@functools.lru_cache(maxsize=None)
def _placeholder_case(mod, kind):
    lays = _lays(mod, kind)
    phs = [np.arange(3, lay["n_re"], 7, dtype=np.uint16) for lay in lays]
    exp = [O.o_pusch_demodulate_ex(*lay["args"], placeholders=ph, want_evm=False)[0] for lay, ph in zip(lays, phs)]
    return lays, phs, exp


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("kind", ["deep", "full"])
@pytest.mark.parametrize("mod", QAM)
def test_evm_and_placeholders_leave_the_packed_form(ctx, mod, kind, device_jobs):
    """The same grids with the EVM requested, and with a placeholder list on every seventh element: both leave the packed form for the fast and exact
    ones. LLRs only (placeholders: against o_pusch_demodulate_ex); the EVM value is not looked at."""
    lays = _lays(mod, kind)
    out, offs = _run(ctx, lays, False, device_jobs, evm=True)
    _check(out, offs, [lay["exp"] for lay in lays], "EVM")
    lays, phs, exp = _placeholder_case(mod, kind)
    out, offs = _run(ctx, lays, True, device_jobs, placeholders=phs)
    _check(out, offs, exp, "placeholders")


@pytest.mark.parametrize("device_jobs", [False, True])
def test_bpsk(ctx, device_jobs):
    """pi/2-BPSK: its own ties (round half away from zero) and the clip of the LLR at +-24, on the compact and on the 14-symbol estimate."""
    lays = _lays(1, "deep") + _lays(1, "full")
    for odd in (False, True):
        out, offs = _run(ctx, lays, odd, device_jobs)
        _check(out, offs, [lay["exp"] for lay in lays], odd)


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("mod", DE.MODS)
def test_abnormal_job_noise_variances(ctx, mod, device_jobs):
    """Job noise variances 0, negative, +Inf, NaN and subnormal, one job each on the compact estimate (every walk's common case but for the variance)
    and one on the 14-symbol estimate: the crafted symbols of noise base 1, whose estimates are 2^k with k up to 3, 0 and 2^-64."""
    lays = []
    for v in DE.ABNORMAL_NOISE_VARS:
        lays += [_lays(mod, "deep", v)[-1], _lays(mod, "full", v)[-2]]  # (bases ascend: 1.0 is the last of the compact set, 3.0 follows it in the full one)
    assert all(np.all(lay["el"]["base"] == 1.0) for lay in lays)
    out, offs = _run(ctx, lays, False, device_jobs)
    _check(out, offs, [lay["exp"] for lay in lays])


# ------------------------------------------------------------------------------------------------ several layers
@functools.lru_cache(maxsize=None)
def _layered(mod, nl):
    """The finite crafted elements (no noise classes) as codeword symbols of nl layers on nl ports through diagonal channels 2^k, one job per noise
    base. Returns [(case, grid, ce, expected LLRs)] and, from zf_single alone, how many components of each class reach the demapper unchanged."""
    slots, arrived = [], {}
    _, names = DE.elements(mod)
    for n, (base, el) in enumerate(DE.bases(mod, with_noise_classes=False)):
        el = el[np.isfinite(el["re"]) & np.isfinite(el["im"])]
        lay = DE.lay(mod, el, base, True, ports=nl, layers=nl)
        c = PL.case("edges", nl, nl, mod, nprb_grid=lay["nprb_grid"], prbs=lay["prbs"], start=lay["start"], nof=lay["nof"], dmrs=lay["dmrs"], cdm=lay["cdm"],
                    compact=True, rnti=0x5000 + n, n_id=500 + mod, noise_var=base)
        assert PL.nof_re(c) == lay["n_re"]
        x, nv = PL.zf_single(*PL.extract(c, lay["grid"], lay["ce"]), base, 1.0)
        x, nv = np.ascontiguousarray(x.T).reshape(-1)[lay["slot"]], np.ascontiguousarray(nv.T).reshape(-1)[lay["slot"]]  # [element][layer] = codeword order
        nv_ok = nv.view(np.uint32) == np.array([DE.nv_of(b, k) for b, k in zip(el["base"], el["k"])], np.float32).view(np.uint32)
        for got, part, cls in ((x.real, "re", "cre"), (x.imag, "im", "cim")):
            same = nv_ok & (np.ascontiguousarray(got).view(np.uint32) == (el[part] + np.float32(0)).view(np.uint32))
            for ci in el[cls][same]:
                arrived[names[ci]] = arrived.get(names[ci], 0) + 1
        exp = PL.expected_llr(c, lay["grid"], lay["ce"])
        exp.setflags(write=False)
        slots.append((c, lay["grid"], lay["ce"], exp))
    # one more job for the variance whose reciprocal is infinite: layer 0 through 2^62, the others through 1, noise variance 0.037. Layer 0 then has
    # the subnormal variance 0.037 * 2^-124 on symbols with a zero component (0 * inf), and its symbols must still arrive unchanged.
    c = PL.case("tiny", nl, nl, mod, nprb_grid=25, prbs=(1, 2), start=1, nof=13, dmrs=(3,), cdm=1, compact=True, rnti=0x5100, n_id=600 + mod, noise_var=0.037)
    sy, sc = PL.data_positions(c)
    z = np.array([complex(*DE.NOISE_SYMBOLS[i % len(DE.NOISE_SYMBOLS)]) for i in range(sy.size)], np.complex64)
    grid = np.full((4, 14, 25 * 12), np.nan + 1j * np.nan, np.complex64)
    ce = np.zeros((nl, nl, 1, 25 * 12), np.complex64)
    for l in range(nl):
        ce[l, l, 0, :] = 1
        grid[l, sy, sc] = np.complex64(complex(*DE.FILLER))
    ce[0, 0, 0, :] = np.float32(2.0 ** 62)
    grid[0, sy, sc] = z * np.float32(2.0 ** 62)
    x, nv = PL.zf_single(*PL.extract(c, grid, ce), 0.037, 1.0)
    arrived["noise:rcp_infinite"] = int(np.sum((nv[0] > 0) & (nv[0] < DE.FLT_MIN) & (x[0] == z) & ((z.real == 0) | (z.imag == 0))))
    exp = PL.expected_llr(c, grid, ce)
    exp.setflags(write=False)
    slots.append((c, grid, ce, exp))
    return slots, arrived


@pytest.mark.parametrize("device_jobs", [False, True])
@pytest.mark.parametrize("nl", [2, 4])
@pytest.mark.parametrize("mod", DE.MODS)
def test_layers(ctx, mod, nl, device_jobs):
    """miphy_pusch_demodulate_layers_batch on 2 x 2 and 4 x 4 diagonal power-of-two channels: the zero forcing of csrc/equalize_device.h (restated
    in pusch_layers_cases.zf_single) must leave the crafted values as they are -- at least one component of every boundary, tie and clip class, counted
    from zf_single alone, and of the variance whose reciprocal is infinite, beside a zero component -- and the LLRs are those of
    pusch_layers_cases.expected_llr. Aligned and odd codewords."""
    import torch
    import miphy
    slots, arrived = _layered(mod, nl)
    _, names = DE.elements(mod)
    for n in names:
        if n.startswith(("boundary", "tie", "clip", "threshold")) or n == "noise:rcp_infinite":
            assert arrived.get(n, 0) >= 1, ("class does not reach the demapper unchanged", n)
    for odd in (False, True):
        offs, total = _offsets([s[3].size for s in slots], odd)
        jobs, go, co = [], 0, 0
        for i, ((c, grid, ce, exp), lo) in enumerate(zip(slots, offs)):
            jobs.append(PL.demod_job(miphy, c, go, co, 5 * i, lo))
            go += grid.size
            co += ce.size
        jobs = np.array(jobs, dtype=miphy.PuschDemodLayersJob)
        sc = np.zeros(5 * len(slots), np.float32)
        sc[2::5] = [s[0]["noise_var"] for s in slots]
        out = torch.full((total,), SENTINEL, dtype=torch.int8, device="cuda")
        ctx.pusch_demodulate_layers_batch(torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if device_jobs else jobs,
                                          torch.from_numpy(np.concatenate([s[1].reshape(-1) for s in slots])).cuda(),
                                          torch.from_numpy(np.concatenate([s[2].reshape(-1) for s in slots])).cuda(), torch.from_numpy(sc).cuda(), out)
        torch.cuda.synchronize()
        _check(out.cpu().numpy(), offs, [s[3] for s in slots], odd)
