"""GPU parity for the batched DFT and the OFDM slot (de)modulator vs the double-precision oracle.

Tolerance (floating point): max |err| <= 4e-6 * rms(output) -- the reference's own float radix-2 DFT sits at ~1.1e-6 * rms
from the exact transform (measured in tests/test_oracle_vs_ref.py); the reference's vector tests allow 1e-4 absolute at
unit scale (ofdm_demodulator_vectortest.cpp:29-83) and MSE < 1e-6 (dft_processor_test.cpp:40-42)."""
import numpy as np
import pytest

from oracle_lib import OfdmCfg, o_dft, o_ofdm_demod_slot, o_ofdm_mod_slot, o_ofdm_slot_size

pytestmark = pytest.mark.gpu
TOL = 4e-6


def rel_err(a, b):
    return float(np.abs(a - b).max() / np.sqrt(np.mean(np.abs(b) ** 2)))


@pytest.mark.parametrize("N", [128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096])
def test_dft_sizes(ctx, N):
    import torch
    rng = np.random.default_rng(N)
    n = 5
    x = (rng.uniform(-1, 1, (n, N)) + 1j * rng.uniform(-1, 1, (n, N))).astype(np.complex64)
    x_d = torch.from_numpy(x).cuda()
    for inv in (False, True):
        out_d = torch.zeros_like(x_d)
        ctx.dft_batch(N, inv, n, x_d, out_d)
        torch.cuda.synchronize()
        out = out_d.cpu().numpy()
        for i in range(n):
            assert rel_err(out[i], o_dft(x[i], inv)) < TOL, (N, inv, i)


@pytest.mark.parametrize("N", [4608, 6144, 9216, 12288, 18432, 24576, 36864, 49152])
def test_dft_large_sizes_four_step(ctx, N):
    """The remaining sizes of the reference's list (dft_processor_generic_impl.cpp:193-210) go through the four-step path.
    Checked against numpy's double-precision FFT (the O(N^2) oracle is too slow here) with the same tolerance."""
    import torch
    rng = np.random.default_rng(N)
    n = 3
    x = (rng.uniform(-1, 1, (n, N)) + 1j * rng.uniform(-1, 1, (n, N))).astype(np.complex64)
    x_d = torch.from_numpy(x).cuda()
    for inv in (False, True):
        out_d = torch.zeros_like(x_d)
        ctx.dft_batch(N, inv, n, x_d, out_d)
        torch.cuda.synchronize()
        out = out_d.cpu().numpy()
        ref = (np.fft.ifft(x.astype(np.complex128), axis=1) * N) if inv else np.fft.fft(x.astype(np.complex128), axis=1)
        for i in range(n):
            assert rel_err(out[i], ref[i]) < TOL, (N, inv, i, rel_err(out[i], ref[i]))
    # small-case cross-check of numpy against the oracle so that the substitution above is itself pinned
    y = x[0, :384]
    assert rel_err(np.fft.fft(y.astype(np.complex128)).astype(np.complex64), o_dft(y, False)) < 1e-6


# Every size the in-LDS transform serves, from the rule in include/miphy.h (2^a * 3^b, 8 <= N <= 4096), not from the kernel.
SINGLE_PASS = sorted(2 ** a * 3 ** b for a in range(13) for b in range(8) if 8 <= 2 ** a * 3 ** b <= 4096)
PAD = 16
SENTINEL = np.complex64(12345.0 - 54321.0j)


def test_single_pass_size_list():
    assert len(SINGLE_PASS) == 51 and len(set(SINGLE_PASS)) == 51
    assert SINGLE_PASS[0] == 8 and SINGLE_PASS[-1] == 4096
    assert {9, 27, 81, 243, 729, 2187, 1152, 2304, 3456, 3888} <= set(SINGLE_PASS)


@pytest.mark.parametrize("N", SINGLE_PASS)
def test_dft_every_single_pass_size(ctx, N):
    """All 51 sizes of the single-pass kernel, both directions, three distinct transforms per call (the per-transform offset), against the
    double-precision DFT by definition. The ten sizes of test_dft_sizes have at most one factor 3, so there the radix-3 pass runs last and
    without twiddles; here it runs up to seven times (2187), with non-power-of-two strides and workgroups, and on sizes with fewer
    butterflies than lanes. 16 sentinel elements behind the n * N results must stay: a scatter past the end would change them.
    A single-precision restatement of the pass structure (running twiddle product, float tables) measured on the CPU stays within
    8.5e-7 * rms of the exact transform at every one of the sizes, so TOL has a fourfold margin."""
    import torch
    rng = np.random.default_rng(N)
    n = 3
    x = (rng.uniform(-1, 1, (n, N)) + 1j * rng.uniform(-1, 1, (n, N))).astype(np.complex64)
    x_d = torch.from_numpy(x.reshape(-1)).cuda()
    worst = 0.0
    for inv in (False, True):
        out_d = torch.full((n * N + PAD,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
        ctx.dft_batch(N, inv, n, x_d, out_d)
        torch.cuda.synchronize()
        out = out_d.cpu().numpy()
        assert (out[n * N:].view(np.uint64) == np.array([SENTINEL]).view(np.uint64)[0]).all(), (N, inv, "written past the end")
        errs = [rel_err(out[i * N:(i + 1) * N], o_dft(x[i], inv)) for i in range(n)]
        worst = max(worst, max(errs))
        for i in range(n):
            assert errs[i] < TOL, (N, inv, i, errs[i])
    print("N = %d: largest distance %.2e" % (N, worst))


def test_dft_unsupported_size(ctx):
    """Below 8 (4, 6), a foreign prime factor (640 = 128 * 5; 4104 = 2^3 * 3^3 * 19, also above 4096), 5000: rejected, nothing written."""
    import torch
    for N in (4, 6, 640, 4104, 5000):
        assert N not in SINGLE_PASS
        x = torch.zeros(N, dtype=torch.complex64, device="cuda")
        out = torch.full((N,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
        with pytest.raises(RuntimeError, match="not supported"):
            ctx.dft_batch(N, False, 1, x, out)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint64) == np.array([SENTINEL]).view(np.uint64)[0]).all(), N


CASES = [(1, 273, 4096, 144, 3.5e9), (1, 273, 4096, 0, 3.5e9), (1, 106, 2048, 72, 3.5e9), (0, 52, 1024, 10, 2.6e9),
         (1, 51, 1536, 0, 3.45e9), (2, 66, 1024, 36, 28e9),
         # sizes with 3^2 and 3^3 (radix-3 passes with twiddles, workgroups of 192, 320 and 448 threads):
         (2, 90, 1152, 20, 28e9),    # four slots, long CP on symbols 0 and 28; the CP of 81 samples is odd: 16- and 8-byte loads alternate
         (0, 190, 2304, 7, 2.6e9),   # odd window offset: every symbol on the unaligned path, phase ramp active
         (1, 273, 3456, 0, 3.5e9)]   # the widest grid


@pytest.mark.parametrize("mu,rb,N,wo,fc", CASES)
def test_ofdm_demodulate_and_modulate(ctx, mu, rb, N, wo, fc):
    import torch
    import miphy
    rng = np.random.default_rng(N + rb)
    nslots = 1 << mu
    cfg = miphy.OfdmConfig(mu, rb, N, wo, 0.5, 0.0, fc)
    ocfg = OfdmCfg(mu, rb, N, wo, 0.5, fc)
    sizes = [cfg.slot_size(s) for s in range(nslots)]
    assert sizes == [o_ofdm_slot_size(ocfg, s) for s in range(nslots)]
    nports = 2
    jobs = np.zeros(nslots * nports, dtype=miphy.OfdmJob)
    xs, off = [], 0
    for s in range(nslots):
        for p in range(nports):
            x = ((rng.standard_normal(sizes[s]) + 1j * rng.standard_normal(sizes[s])) * 0.7).astype(np.complex64)
            jobs[s * nports + p] = (off, (s * nports + p) * 14 * rb * 12, s, 0)
            xs.append(x)
            off += sizes[s]
    x_d = torch.from_numpy(np.concatenate(xs)).cuda()
    grid_d = torch.zeros(nslots * nports * 14 * rb * 12, dtype=torch.complex64, device="cuda")
    ctx.ofdm_demodulate_slots(cfg, jobs, x_d, grid_d)
    torch.cuda.synchronize()
    grid = grid_d.cpu().numpy().reshape(nslots * nports, 14, rb * 12)
    for j in range(nslots * nports):
        exp = o_ofdm_demod_slot(ocfg, j // nports, xs[j])
        assert rel_err(grid[j], exp) < TOL, (j, rel_err(grid[j], exp))
    # modulator: grid -> time, then the round trip mod -> demod recovers the grid up to the scale product
    mcfg = miphy.OfdmConfig(mu, rb, N, 0, 0.01, 0.0, fc)
    mocfg = OfdmCfg(mu, rb, N, 0, 0.01, fc)
    g = (rng.standard_normal((nslots * nports, 14, rb * 12)) + 1j * rng.standard_normal((nslots * nports, 14, rb * 12))).astype(np.complex64)
    g_d = torch.from_numpy(g.reshape(-1)).cuda()
    y_d = torch.zeros_like(x_d)
    jobs["grid_empty"][-1] = 1
    ctx.ofdm_modulate_slots(mcfg, jobs, g_d, y_d)
    torch.cuda.synchronize()
    y = y_d.cpu().numpy()
    for j in range(nslots * nports):
        o0 = int(jobs[j]["samples_offset"])
        got = y[o0:o0 + sizes[j // nports]]
        if j == nslots * nports - 1:
            assert not got.any()
            continue
        exp = o_ofdm_mod_slot(mocfg, j // nports, g[j])
        assert rel_err(got, exp) < TOL, (j, rel_err(got, exp))
    # round trip (size independent property): demod(mod(grid)) == grid * N * scale_tx * scale_rx when both use offset 0
    jobs["grid_empty"][-1] = 0
    rcfg = miphy.OfdmConfig(mu, rb, N, 0, 1.0 / (N * 0.01), 0.0, fc)
    ctx.ofdm_modulate_slots(mcfg, jobs, g_d, y_d)
    g2_d = torch.zeros_like(g_d)
    ctx.ofdm_demodulate_slots(rcfg, jobs, y_d, g2_d)
    torch.cuda.synchronize()
    g2 = g2_d.cpu().numpy().reshape(g.shape)
    assert rel_err(g2, g) < 2e-5


@pytest.mark.parametrize("mu,rb,N,wo,fc", [CASES[0], CASES[2], CASES[5], CASES[7]])
def test_ofdm_symbol_entry_points_equal_the_slot_ones(ctx, mu, rb, N, wo, fc):
    """miphy_ofdm_{de}modulate_symbols (ofdm_symbol_demodulator / _modulator, ofdm_demodulator.h:55-74): one job per OFDM symbol, in any
    order, must give the rows / samples the slot entry points give for the same subframe -- bit-identical, it is the same transform."""
    import torch
    import miphy
    rng = np.random.default_rng(N * 3 + rb)
    nslots = 1 << mu
    nsc = rb * 12
    cfg = miphy.OfdmConfig(mu, rb, N, wo, 0.5, 0.0, fc)
    sizes = [cfg.slot_size(s) for s in range(nslots)]
    sym = [miphy.ofdm_symbol_size(cfg, i) for i in range(14 * nslots)]
    assert [sum(sym[14 * s:14 * s + 14]) for s in range(nslots)] == sizes
    x = ((rng.standard_normal(sum(sizes)) + 1j * rng.standard_normal(sum(sizes))) * 0.7).astype(np.complex64)
    x_d = torch.from_numpy(x).cuda()
    sj = np.zeros(nslots, dtype=miphy.OfdmJob)
    off = 0
    for s in range(nslots):
        sj[s] = (off, s * 14 * nsc, s, 0)
        off += sizes[s]
    g_slot = torch.zeros(nslots * 14 * nsc, dtype=torch.complex64, device="cuda")
    ctx.ofdm_demodulate_slots(cfg, sj, x_d, g_slot)
    order = rng.permutation(14 * nslots)
    starts = np.concatenate([[0], np.cumsum(sym)[:-1]])
    yj = np.zeros(14 * nslots, dtype=miphy.OfdmJob)
    for k, i in enumerate(order):
        yj[k] = (int(starts[i]), int(i) * nsc, int(i), 0)
    g_sym = torch.zeros_like(g_slot)
    ctx.ofdm_demodulate_symbols(cfg, yj, x_d, g_sym)
    torch.cuda.synchronize()
    assert torch.equal(g_slot, g_sym)
    # modulator
    mcfg = miphy.OfdmConfig(mu, rb, N, 0, 0.01, 0.0, fc)
    g = (rng.standard_normal(nslots * 14 * nsc) + 1j * rng.standard_normal(nslots * 14 * nsc)).astype(np.complex64)
    g_d = torch.from_numpy(g).cuda()
    y_slot, y_sym = torch.zeros_like(x_d), torch.zeros_like(x_d)
    ctx.ofdm_modulate_slots(mcfg, sj, g_d, y_slot)
    ctx.ofdm_modulate_symbols(mcfg, yj, g_d, y_sym)
    torch.cuda.synchronize()
    assert torch.equal(y_slot, y_sym)


@pytest.mark.parametrize("mu,rb,N,wo,fc", [CASES[6], CASES[2]])
def test_ofdm_device_resident_jobs(ctx, mu, rb, N, wo, fc):
    """The four entry points with their jobs in device memory (a uint8 tensor of the same bytes; the library then skips its host check of
    slot_index and reads the table in place): bit-identical to the same call with host jobs."""
    import torch
    import miphy
    rng = np.random.default_rng(N * 5 + rb)
    nslots = 1 << mu
    nsc = rb * 12
    cfg = miphy.OfdmConfig(mu, rb, N, wo, 0.5, 0.0, fc)
    mcfg = miphy.OfdmConfig(mu, rb, N, 0, 0.01, 0.0, fc)
    sizes = [cfg.slot_size(s) for s in range(nslots)]
    sym = [miphy.ofdm_symbol_size(cfg, i) for i in range(14 * nslots)]
    sj = np.zeros(nslots, dtype=miphy.OfdmJob)
    for k, s in enumerate(rng.permutation(nslots)):  # slots in any order in the table, each where the subframe puts it
        sj[k] = (int(np.sum(sizes[:s])), int(s) * 14 * nsc, int(s), 0)
    starts = np.concatenate([[0], np.cumsum(sym)[:-1]])
    yj = np.zeros(14 * nslots, dtype=miphy.OfdmJob)
    for k, i in enumerate(rng.permutation(14 * nslots)):
        yj[k] = (int(starts[i]), int(i) * nsc, int(i), 0)
    sj["grid_empty"][-1] = 1
    yj["grid_empty"][3] = 1
    x_d = torch.from_numpy(((rng.standard_normal(sum(sizes)) + 1j * rng.standard_normal(sum(sizes))) * 0.7).astype(np.complex64)).cuda()
    g_d = torch.from_numpy((rng.standard_normal(nslots * 14 * nsc) + 1j * rng.standard_normal(nslots * 14 * nsc)).astype(np.complex64)).cuda()
    for jobs, demod, mod in ((sj, ctx.ofdm_demodulate_slots, ctx.ofdm_modulate_slots), (yj, ctx.ofdm_demodulate_symbols, ctx.ofdm_modulate_symbols)):
        jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        assert jobs_d.is_cuda and jobs_d.numel() == jobs.size * miphy.OfdmJob.itemsize
        grid_h, grid_dv = torch.zeros_like(g_d), torch.zeros_like(g_d)
        demod(cfg, jobs, x_d, grid_h)
        demod(cfg, jobs_d, x_d, grid_dv)
        y_h, y_dv = torch.full_like(x_d, 7.0), torch.full_like(x_d, 7.0)
        mod(mcfg, jobs, g_d, y_h)
        mod(mcfg, jobs_d, g_d, y_dv)
        torch.cuda.synchronize()
        bits = lambda t: torch.view_as_real(t).view(torch.int32)
        assert (grid_h != 0).all() and torch.equal(bits(grid_h), bits(grid_dv))
        assert (y_h != 7.0).all() and torch.equal(bits(y_h), bits(y_dv))


@pytest.mark.parametrize("mu,rb,N", [(0, 6, 128), (1, 51, 1536)])
def test_ofdm_demodulate_more_symbols_than_one_wave_of_workgroups(ctx, mu, rb, N):
    """ofdm_demodulate starts min(symbols, CUs * per_cu) workgroups, each looping over its share of the symbols with a barrier between two of
    them (the LDS buffer is rewritten). per_cu = min(8, 160 KiB / (fft_lds_bytes(N) + 512)) -- 8 for both sizes here -- so the loop makes a
    second trip only beyond CUs * 8 symbols: 147 slots on a 256-CU chip, far more than any other test demodulates. Five distinct slots, repeated:
    every output slot is bit-identical to the same slot demodulated in a batch of five (one trip), which is within TOL of the oracle.
    This pins the second trip's indexing and results. It does not catch a missing barrier at the end of the loop body: a build without it passed
    (a wavefront reaches its next LDS write only after a round trip to HBM, long after the others have read their outputs)."""
    import torch
    import miphy
    wo = 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fft_lds_bytes = (N + (N >> 3) + 16) * 8                         # fft_device.h
    per_cu = max(1, min(8, (160 * 1024) // (fft_lds_bytes + 512)))  # ofdm_demodulate
    assert per_cu == 8
    n_slots = (cus * per_cu) // 14 + 40
    assert 14 * n_slots > cus * per_cu
    rng = np.random.default_rng(N + 7)
    cfg, ocfg = miphy.OfdmConfig(mu, rb, N, wo, 0.5, 0.0, 3.5e9), OfdmCfg(mu, rb, N, wo, 0.5, 3.5e9)
    slot_of = [k % (1 << mu) for k in range(5)]
    xs = [((rng.standard_normal(cfg.slot_size(s)) + 1j * rng.standard_normal(cfg.slot_size(s))) * 0.7).astype(np.complex64) for s in slot_of]
    starts = np.concatenate([[0], np.cumsum([x.size for x in xs])[:-1]])
    x_d = torch.from_numpy(np.concatenate(xs)).cuda()
    gsz = 14 * rb * 12
    jobs = np.zeros(n_slots, dtype=miphy.OfdmJob)
    for i in range(n_slots):
        jobs[i] = (int(starts[i % 5]), i * gsz, slot_of[i % 5], 0)
    few_d = torch.zeros(5 * gsz, dtype=torch.complex64, device="cuda")
    many_d = torch.zeros(n_slots * gsz, dtype=torch.complex64, device="cuda")
    ctx.ofdm_demodulate_slots(cfg, jobs[:5].copy(), x_d, few_d)
    ctx.ofdm_demodulate_slots(cfg, jobs, x_d, many_d)
    torch.cuda.synchronize()
    few, many = few_d.cpu().numpy().reshape(5, 14, rb * 12), many_d.cpu().numpy().reshape(n_slots, 14, rb * 12)
    for k in range(5):
        exp = o_ofdm_demod_slot(ocfg, slot_of[k], xs[k])
        assert rel_err(few[k], exp) < TOL, (k, rel_err(few[k], exp))
    bad = [i for i in range(n_slots) if not np.array_equal(many[i].view(np.uint32), few[i % 5].view(np.uint32))]
    assert not bad, (len(bad), bad[:8])
