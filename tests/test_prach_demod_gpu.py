"""GPU: miphy_prach_demodulate_batch (csrc/prach_demod.hip) against the float64 restatement of tests/prach_demod_ref.py, which
test_prach_demod_ref.py holds against the reference's recorded output on the CPU. TOL is the project's DFT tolerance with the metric
of tests/test_ofdm_gpu.py. A call has one sampling rate, so "one batch" of the fixture is one call per sampling rate with every case
of that rate."""
import re

import numpy as np
import pytest

import miphy
import prach_demod_ref as D
import prach_ref as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 4e-6
SENT = np.complex64(12345.0 - 54321.0j)


def layout(cfgs, max_fd=None, max_sym=None, gap=0):
    """Jobs of the configuration rows with their windows back to back and their buffers back to back (`gap` cf_t of slack in front of
    each buffer; max_fd / max_sym: strides above what is used, per job or one for all)."""
    jobs = np.zeros(len(cfgs), miphy.PrachDemodJob)
    geo, s_off, b_off = [], 0, 0
    for n, c in enumerate(cfgs):
        g = D.geometry(c)
        mf = int(c[D.C_NFD]) if max_fd is None else int(np.broadcast_to(max_fd, len(cfgs))[n])
        ms = g["nof_symbols"] if max_sym is None else int(np.broadcast_to(max_sym, len(cfgs))[n])
        b_off += gap
        jobs[n] = D.job_of(c, s_off, b_off, mf, ms, g=g)
        geo.append(g)
        s_off += int(c[D.C_NSAMPLES])
        b_off += int(c[D.C_NTD]) * mf * ms * g["L"]
    return jobs, geo, s_off, b_off + gap


def rows(buf, job, g):
    """[td][fd][symbol][L] of a job out of the host copy of the buffer."""
    ntd, nfd, mf, ms, L = int(job["nof_td_occasions"]), int(job["nof_fd_occasions"]), int(job["max_nof_fd_occasions"]), int(job["max_nof_symbols"]), g["L"]
    o = int(job["buffer_offset"])
    return buf[o:o + ntd * mf * ms * L].reshape(ntd, mf, ms, L)[:, :nfd, :g["nof_symbols"]]


def run(ctx, cfgs, windows, **kw):
    """Outputs per job, the whole buffer (host copy) and the jobs of one call."""
    jobs, geo, ns, nb = layout(cfgs, **kw)
    x = torch.from_numpy(np.concatenate(windows)).cuda()
    buf = torch.full((nb,), complex(SENT), dtype=torch.complex64, device="cuda")
    ctx.prach_demodulate_batch(int(cfgs[0][D.C_SRATE]), jobs, x, buf)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return [rows(h, j, g) for j, g in zip(jobs, geo)], h, jobs, geo


_restated = {}


def restated(i):
    """The float64 restatement of fixture case i, computed once."""
    if i not in _restated:
        c = D.fixture()[i]
        _restated[i] = D.demodulate(c["window"], c["cfg"], c["geometry"])
    return _restated[i]


@pytest.mark.parametrize("srate", [7680000, 15360000, 23040000, 30720000, 61440000])
def test_fixture_cases_in_one_batch_and_alone(ctx, srate):
    fx = D.fixture()
    idx = [i for i, c in enumerate(fx) if int(c["cfg"][D.C_SRATE]) == srate]
    assert idx
    batch, _, _, _ = run(ctx, [fx[i]["cfg"] for i in idx], [fx[i]["window"] for i in idx])
    worst = 0.0
    for n, i in enumerate(idx):
        e = D.rel_err(batch[n], restated(i))
        worst = max(worst, e)
        assert e < TOL, (i, list(fx[i]["cfg"]), e)
        alone, _, _, _ = run(ctx, [fx[i]["cfg"]], [fx[i]["window"]])
        assert np.array_equal(alone[0].view(np.uint32), batch[n].view(np.uint32)), (i, "the batch differs from the case alone")
    print("%d Hz: %d cases, largest distance %.2e" % (srate, len(idx), worst))


def straddling(srate, fmt, mu, nfd, start=0, ntd=1):
    """A configuration whose first frequency-domain occasion has the middle of the PRACH grid (DFT bin 0) inside its sequence."""
    scs_hz = (5000 if fmt == 3 else 1250) if fmt < 4 else 15000 << mu
    L = 839 if fmt < 4 else 139
    N, K = srate // scs_hz, (15000 << mu) // scs_hz
    nprb = min((N - 1) // (K * 12), 275)
    rb = (nprb * K * 6 - D.FREQ_MAP[(scs_hz, mu)][1] - L // 2) // (K * 12)
    c = np.array([srate, fmt, mu, ntd, nfd, start, rb, nprb, 1 << 30], np.int64)
    g = D.geometry(c)
    assert g["k_start"][0] < g["grid"] // 2 < g["k_start"][0] + L and g["dft_size"] == N
    c[D.C_NSAMPLES] = max(g["window_samples"], max(o + p + g["nof_symbols"] * N for o, p in zip(g["td_sample_offset"], g["td_cp_samples"])))
    return c


def noise(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("fmt,srate,N", [(0, 7680000, 6144), (0, 15360000, 12288), (0, 23040000, 18432), (0, 30720000, 24576), (0, 46080000, 36864),
                                         (0, 61440000, 49152), (3, 23040000, 4608), (3, 46080000, 9216)])
def test_every_four_step_size(ctx, fmt, srate, N):
    """One window each: two frequency-domain occasions, the first straddling bin 0 (the k2 range of the pruned step wraps modulo N2)."""
    c = straddling(srate, fmt, 0, 2)
    x = noise(N, int(c[D.C_NSAMPLES]))
    g = D.geometry(c)
    assert g["dft_size"] == N
    b = D.bins(g, 0)
    assert b[0] > b[-1]  # wraps from bin N - 1 to bin 0
    got, _, _, _ = run(ctx, [c], [x])
    e = D.rel_err(got[0], D.demodulate(x, c, g))
    print("N = %d: distance %.2e" % (N, e))
    assert e < TOL, e


@pytest.mark.parametrize("fmt,srate,mu,N,nsym", [(9, 7680000, 1, 256, 1), (8, 15360000, 0, 1024, 12)])
def test_smallest_single_pass_shapes(ctx, fmt, srate, mu, N, nsym):
    c = straddling(srate, fmt, mu, 1)
    g = D.geometry(c)
    assert (g["dft_size"], g["nof_symbols"]) == (N, nsym)
    x = noise(N + 1, int(c[D.C_NSAMPLES]))
    got, _, _, _ = run(ctx, [c], [x])
    e = D.rel_err(got[0], D.demodulate(x, c, g))
    assert e < TOL, e


@pytest.mark.parametrize("srate,fmt,mu,nfd,N", [
    (5760000, 3, 0, 1, 1152),    # single-pass kernel, two radix-3 passes (the second pass's twiddles), 192 threads
    (11520000, 3, 1, 1, 2304),   # single-pass kernel, 320 threads
    (17280000, 3, 0, 1, 3456),   # single-pass kernel, three radix-3 passes, 448 threads
    (17280000, 4, 0, 1, 1152),   # short format, two symbols
    (46080000, 4, 0, 2, 3072),   # a short format at 46.08 MHz
    (92160000, 3, 0, 2, 18432),  # four-step at 92.16 MHz
])
def test_sizes_and_rates_beyond_the_fixture(ctx, srate, fmt, mu, nfd, N):
    """Sampling rates the recorded fixture does not hold, among them the three whose format 3 transform has a factor 9 or 27 (no other
    test of the single-pass kernel here has one). One window of noise each, the first occasion straddling bin 0."""
    c = straddling(srate, fmt, mu, nfd)
    g = D.geometry(c)
    assert g["dft_size"] == N
    b = D.bins(g, 0)
    assert b[0] > b[-1]  # wraps from bin N - 1 to bin 0
    x = noise(srate // 1000 + fmt, int(c[D.C_NSAMPLES]))
    got, _, _, _ = run(ctx, [c], [x])
    e = D.rel_err(got[0], D.demodulate(x, c, g))
    print("%d Hz, format %d, N = %d: distance %.2e" % (srate, fmt, N, e))
    assert e < TOL, e


def test_buffer_strides_and_bounds(ctx):
    """Strides above what is used, slack around every job's buffer, two ports of one configuration through two jobs, a single-pass and a
    four-step configuration in one call: every row lands where the strides put it and nothing else changes."""
    short = straddling(30720000, 4, 0, 2, start=1, ntd=3)  # A1 x 3 x 2, N = 2048
    long_ = straddling(30720000, 0, 0, 2)                  # N = 24576
    cfgs = [short, long_, short, long_]
    windows = [noise(10 + n, int(c[D.C_NSAMPLES])) for n, c in enumerate(cfgs)]
    got, h, jobs, geo = run(ctx, cfgs, windows, max_fd=[3, 4, 3, 4], max_sym=[4, 2, 4, 2], gap=1000)
    assert jobs[2]["buffer_offset"] > jobs[0]["buffer_offset"]
    written = np.zeros(len(h), bool)
    for n, (c, x, j, g) in enumerate(zip(cfgs, windows, jobs, geo)):
        assert D.rel_err(got[n], D.demodulate(x, c, g)) < TOL, n
        L, ms, mf = g["L"], int(j["max_nof_symbols"]), int(j["max_nof_fd_occasions"])
        for td in range(int(c[D.C_NTD])):
            for fd in range(int(c[D.C_NFD])):
                for s in range(g["nof_symbols"]):
                    o = int(j["buffer_offset"]) + ((td * mf + fd) * ms + s) * L
                    written[o:o + L] = True
    assert written.sum() == sum(r.size for r in got)
    assert (h[~written].view(np.uint64) == np.array([SENT]).view(np.uint64)[0]).all(), "a sample outside the jobs' rows was written"
    assert not (h[written].view(np.uint64) == np.array([SENT]).view(np.uint64)[0]).any(), "a row keeps a sentinel"


@pytest.mark.parametrize("fmt,srate,mu,njobs", [(0, 30720000, 0, 343), (8, 15360000, 0, 1367)])
def test_calls_larger_than_one_piece(ctx, fmt, srate, mu, njobs):
    """The task table is staged and launched in pieces (1 MiB of tasks = 16384; 341 symbols of 24576 points for the four-step scratch):
    one more job than a piece holds, every job reading the same window into rows of its own, all equal to the first job's."""
    c = straddling(srate, fmt, mu, 1)
    g = D.geometry(c)
    x = noise(77, int(c[D.C_NSAMPLES]))
    jobs, _, _, nb = layout([c] * njobs)
    jobs["samples_offset"] = 0
    assert njobs * g["nof_symbols"] > (16384 if g["dft_size"] <= 4096 else (64 << 20) // (8 * g["dft_size"]))
    buf = torch.full((nb,), complex(SENT), dtype=torch.complex64, device="cuda")
    ctx.prach_demodulate_batch(srate, jobs, torch.from_numpy(x).cuda(), buf)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().reshape(njobs, -1)
    assert D.rel_err(h[0], D.demodulate(x, c, g)) < TOL
    assert (h.view(np.uint64) == h[0].view(np.uint64)).all()


# (format, PUSCH spacing, occasions td x fd, zone, root sequence index, [(td, fd, preamble index, delay_n)]): delays in samples of the
# detector's 1536-point grid, at least two taps inside its window (delay_n_maximum) and away from zero's wrap.
COMPOSED = [
    (0, 0, 1, 2, 9, 22, [(0, 0, 5, 12), (0, 1, 40, 3)]),
    (8, 1, 1, 1, 11, 60, [(0, 0, 17, 6)]),
    (11, 0, 2, 2, 8, 3, [(0, 0, 0, 6), (0, 1, 20, 12), (1, 1, 33, 3), (1, 0, 63, 9)]),
]


def composed_inputs(srate, idft):
    """Configurations, windows (noise of standard deviation 0.3 per DFT bin under unit-power preambles) and (format, spacing, zone,
    root) per configuration."""
    tables = P.header_tables()
    cfgs, windows, occasions = [], [], []
    for n, (fmt, mu, ntd, nfd, zcz, root, txs) in enumerate(COMPOSED):
        c = straddling(srate, fmt, mu, nfd, ntd=ntd)
        g = D.geometry(c)
        d = P.derive(fmt, mu, zcz, idft)
        tx = []
        for td, fd, idx, delay_n in txs:
            assert 2 <= delay_n <= d["delay_n_maximum"] - 3
            assert (delay_n * g["dft_size"]) % idft == 0
            _, u, cv = P.root_and_shift(fmt, root, zcz, idx, tables)
            tx.append((td, fd, u, cv, delay_n * g["dft_size"] // idft, 1.0))
        cfgs.append(c)
        windows.append(D.build_window(1000 + n, c, 0.3 / np.sqrt(g["dft_size"]), tx))
        occasions.append((fmt, mu, zcz, root))
    return cfgs, windows, occasions


def test_demodulate_then_detect_on_one_stream(ctx):
    """prach_demodulate_batch then prach_detect_batch on the same stream, symbol_offset pointing at symbol 0 of every (td, fd) occasion
    of the demodulator's output, no host copy in between: the detected preamble indices and delay_n of prach_detect_batch on the
    restated symbols."""
    srate, idft = 30720000, 1536
    cfgs, windows, occasions = composed_inputs(srate, idft)
    jobs, geo, ns, nb = layout(cfgs, max_fd=3, max_sym=[g_ + 1 for g_ in [D.geometry(c)["nof_symbols"] for c in cfgs]])
    # detector jobs over the demodulator's buffer, and the same over the restated symbols laid out identically
    pj = []
    ref_buf = np.zeros(nb, np.complex64)
    for c, x, j, g, (fmt, mu, zcz, root) in zip(cfgs, windows, jobs, geo, occasions):
        ref = D.demodulate(x, c, g)
        for td in range(int(c[D.C_NTD])):
            for fd in range(int(c[D.C_NFD])):
                o = int(j["buffer_offset"]) + ((td * int(j["max_nof_fd_occasions"]) + fd) * int(j["max_nof_symbols"])) * g["L"]
                ref_buf[o:o + g["L"]] = ref[td, fd, 0]
                pj.append((fmt, mu, root, zcz, 0, 0, 64, idft, o, 64 * len(pj)))
    pjobs = np.zeros(len(pj), miphy.PrachJob)
    for n, r in enumerate(pj):
        pjobs[n] = r
    REC = miphy.PrachPreambleResult.itemsize

    def detect(symbols, stream):
        res = torch.zeros(len(pjobs) * miphy.PrachResult.itemsize, dtype=torch.uint8, device="cuda")
        pre = torch.zeros(64 * len(pjobs) * REC, dtype=torch.uint8, device="cuda")
        ctx.prach_detect_batch(pjobs, symbols, res, pre, stream=stream)
        return pre

    x_d = torch.from_numpy(np.concatenate(windows)).cuda()
    buf = torch.zeros(nb, dtype=torch.complex64, device="cuda")
    ref_d = torch.from_numpy(ref_buf).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx.prach_demodulate_batch(srate, jobs, x_d, buf, stream=s)
        got_d = detect(buf, s)
        exp_d = detect(ref_d, s)
    s.synchronize()
    got = got_d.cpu().numpy().view(miphy.PrachPreambleResult)
    exp = exp_d.cpu().numpy().view(miphy.PrachPreambleResult)
    assert (np.abs(exp["metric"] - 0.07) > 0.007).all(), "a metric within 10 % of the threshold: choose another seed"
    assert np.array_equal(got["detected"], exp["detected"])
    det = exp["detected"] == 1
    assert np.array_equal(got["delay_n"][det], exp["delay_n"][det])
    # and the transmitted ones are among them (the preamble one cyclic shift below sees the same peak at a negative delay)
    want, n0 = set(), 0
    for c, (fmt, mu, ntd, nfd, zcz, root, txs) in zip(cfgs, COMPOSED):
        for td, fd, idx, delay_n in txs:
            want.add((n0 + td * nfd + fd, idx, delay_n))
        n0 += ntd * nfd
    found = {(int(i) // 64, int(i) % 64, int(exp["delay_n"][i])) for i in np.flatnonzero(det)}
    assert want <= found, (sorted(found), sorted(want))


def code_of(fn, message):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert message in str(e.value), str(e.value)
    return int(re.match(r"miphy error (-?\d+):", str(e.value)).group(1))


def test_rejection_and_no_ops(ctx):
    good = straddling(30720000, 9, 0, 1)  # C0: its window (4400 samples) is longer than what its occasion reads (3304)
    jobs, geo, ns, nb = layout([good, good])
    assert geo[1]["td_sample_offset"][0] + geo[1]["td_cp_samples"][0] + geo[1]["dft_size"] < jobs[1]["nof_samples"] - 1
    jobs[1]["nof_samples"] -= 1  # the second job's window is shorter than the window duration: nothing of the first is written either
    x = torch.from_numpy(noise(5, ns)).cuda()
    buf = torch.full((max(nb, 839),), complex(SENT), dtype=torch.complex64, device="cuda")
    assert code_of(lambda: ctx.prach_demodulate_batch(30720000, jobs, x, buf), "equal to or greater than the PRACH window") == -1
    ctx.prach_demodulate_batch(30720000, jobs[:0], x, buf)  # n == 0
    big = np.zeros(1, miphy.PrachDemodJob)
    big[0] = (0, 0, 1, 1, 0, 0, 106, 122880, 0, 0, 1, 1)  # format 0 at 122.88 MHz: 98304 points
    zeros = torch.zeros(122880, dtype=torch.complex64, device="cuda")
    assert code_of(lambda: ctx.prach_demodulate_batch(122880000, big, zeros, buf), "not supported") == -4
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint64) == np.array([SENT]).view(np.uint64)[0]).all(), "a rejected call wrote to the buffer"
