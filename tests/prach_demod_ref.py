"""OFDM PRACH demodulator restated in numpy float64 from TS 38.211 5.3.2 / 6.3.3 and from the behaviour of the reference's
ofdm_prach_demodulator_impl, get_prach_preamble_long_info / _short_info, get_prach_window_duration and prach_frequency_mapping_get,
plus a seeded transmitter that gives it (and the detector behind it) something to find.

- geometry(): what the demodulator derives before it looks at a sample. Times are kept in T_c like the reference's phy_time_unit and
  0.5 ms comes from prach_ref.from_seconds, so the comparisons around 0 and 0.5 ms are the reference's own. Raises Rejected where
  the reference asserts.
- demodulate(): per time-domain occasion and symbol one np.fft.fft of dft_size samples after the cyclic prefix; per frequency-domain
  occasion the L bins from k_start, the lower half of the PRACH grid being the last grid/2 bins of the spectrum. complex128
  [td][fd][symbol][L].
- build_window(): noise over the whole window and, per (td, fd) occasion that transmits, a preamble of prach_ref.sequence on the
  occasion's bins, taken to the time domain in float64, repeated over the symbols behind its cyclic prefix and delayed by a whole
  number of samples. Deterministic in the seed (numpy PCG64); complex64.

Configuration rows (int64): see the C_* indices. Formats and PUSCH subcarrier spacings are numbered as in prach_ref / the reference
(formats 0..13; pusch_scs 0..3 = 15..120 kHz, which short formats use as RA spacing too).
"""
import hashlib

import numpy as np

import prach_ref as P

(C_SRATE, C_FMT, C_SCS, C_NTD, C_NFD, C_START, C_RB, C_NPRB, C_NSAMPLES) = range(9)
KAPPA = 64
TC_PER_S = 480000 * 4096
MAX_TD, MAX_FD = 7, 8
SRATES = (7680000, 15360000, 23040000, 30720000, 46080000, 61440000)
SERVED_SIZES = (4608, 6144, 9216, 12288, 18432, 24576, 36864, 49152)

# get_prach_preamble_long_info: symbol length and cyclic prefix in kappa, RA spacing in Hz
LONG = ((24576, 3168, 1250), (2 * 24576, 21024, 1250), (4 * 24576, 4688, 1250), (4 * 6144, 3168, 5000))
# get_prach_preamble_short_info at 15 kHz (>> numerology): symbol length / 2048 kappa, cyclic prefix, cyclic prefix of the last occasion;
# get_preamble_duration in PUSCH symbols. A1 A2 A3 B1 B4 C0 C2 A1/B1 A2/B2 A3/B3
SHORT = ((2, 288, 288, 2), (4, 576, 576, 4), (6, 864, 864, 6), (2, 216, 216, 2), (12, 936, 936, 12), (1, 1240, 1240, 2), (4, 2048, 2048, 6),
         (2, 288, 216, 2), (4, 576, 360, 4), (6, 864, 504, 6))
# prach_frequency_mapping_get: (RA spacing Hz, PUSCH spacing index) -> (nof_rb_ra, k_bar); anything else is reserved
FREQ_MAP = {(1250, 0): (6, 7), (1250, 1): (3, 1), (1250, 2): (2, 133), (5000, 0): (24, 12), (5000, 1): (12, 10), (5000, 2): (6, 7),
            (15000, 0): (12, 2), (15000, 1): (6, 2), (15000, 2): (3, 2), (30000, 0): (24, 2), (30000, 1): (12, 2), (30000, 2): (6, 2),
            (60000, 2): (12, 2), (60000, 3): (6, 2), (120000, 2): (24, 2), (120000, 3): (12, 2)}


class Rejected(ValueError):
    """The reference asserts on this configuration."""


class Unsupported(ValueError):
    """Valid for the reference, a DFT size the device does not transform."""


def _to_samples(tc, srate):
    if (tc * srate) % TC_PER_S:
        raise Rejected("%d T_c is not a whole number of samples at %d Hz" % (tc, srate))
    return (tc * srate) // TC_PER_S


def size_served(n):
    if n in SERVED_SIZES:
        return True
    if n < 8 or n > 4096:
        return False
    while n % 2 == 0:
        n //= 2
    while n % 3 == 0:
        n //= 3
    return n == 1


def geometry(cfg, max_nof_fd_occasions=MAX_FD, max_nof_symbols=12):
    """dict(L, ra_scs_hz, dft_size, nof_symbols, K, k_bar, nof_rb_ra, window_samples, td_sample_offset[], td_cp_samples[], k_start[],
    grid) of a configuration row."""
    srate, fmt, mu, ntd, nfd, start, rb, nprb, nsamples = (int(v) for v in cfg)
    sixteen = 16 * KAPPA
    zero, half_ms = P.from_seconds(0.0), P.from_seconds(0.5e-3)
    if not 0 <= fmt <= 13 or not 0 <= mu <= 3:
        raise Rejected("format or PUSCH subcarrier spacing")
    is_long = fmt < 4
    if is_long and ntd != 1:
        raise Rejected("long preambles only support one occasion")
    if ntd < 1 or nfd < 1 or ntd > MAX_TD or nfd > MAX_FD or nfd > max_nof_fd_occasions:
        raise Rejected("number of occasions")
    pusch_symbol = ((144 + 2048) >> mu) * KAPPA
    if is_long:
        sym_tc, cp_first, scs_hz = LONG[fmt][0] * KAPPA, LONG[fmt][1] * KAPPA, LONG[fmt][2]
        cp_last, duration, L = cp_first, 0, 839
    else:
        x, cp_a, cp_b, duration = SHORT[fmt - 4]
        sym_tc, cp_first, cp_last, scs_hz, L = ((x * 2048) >> mu) * KAPPA, (cp_a >> mu) * KAPPA, (cp_b >> mu) * KAPPA, 15000 << mu, 139
    if (scs_hz, mu) not in FREQ_MAP:
        raise Rejected("reserved subcarrier spacing combination")
    nof_rb_ra, k_bar = FREQ_MAP[(scs_hz, mu)]
    if srate <= 0 or srate % scs_hz:
        raise Rejected("the RA subcarrier spacing does not divide the sampling rate")
    dft_size = srate // scs_hz
    nof_symbols = _to_samples(sym_tc, scs_hz)
    if nof_symbols > max_nof_symbols:
        raise Rejected("symbols exceed the buffer")
    K = (15000 << mu) // scs_hz
    grid = nprb * K * 12
    if dft_size <= grid:
        raise Rejected("DFT size not sufficient for the grid")
    k_start = [K * 12 * (rb + nof_rb_ra * fd) + k_bar for fd in range(nfd)]
    if any(k + L >= grid for k in k_start):
        raise Rejected("start subcarrier plus sequence length exceeds the grid")

    def start_of(t):
        if t > zero:
            t += sixteen
        if t > half_ms:
            t += sixteen
        return t

    td_off, td_cp = [], []
    for td in range(ntd):
        cp = cp_last if td == ntd - 1 else cp_first
        t_start = start_of(pusch_symbol * (start + duration * td))
        t_end = t_start + cp + sym_tc
        if not is_long:
            if t_start <= zero and t_end >= zero:
                cp += sixteen
            if t_start <= half_ms and t_end >= half_ms:
                cp += sixteen
        off, cps, total = _to_samples(t_start, srate), _to_samples(cp, srate), _to_samples(cp + sym_tc, srate)
        if off + total > nsamples:
            raise Rejected("the window is shorter than what occasion %d reads" % td)
        td_off.append(off), td_cp.append(cps)
    # get_prach_window_duration
    w_start = start_of((pusch_symbol if not is_long else (144 + 2048) * KAPPA) * start)
    if is_long:
        w_end = P.from_seconds(1e-3 * np.ceil((w_start + cp_first + sym_tc) / TC_PER_S * 1e3))
        window = (w_end * srate) // TC_PER_S
    else:
        w_end = w_start + pusch_symbol * duration * ntd
        if w_start <= zero and w_end >= zero:
            w_end += sixteen
        if w_start <= half_ms and w_end > half_ms:
            w_end += sixteen
        window = _to_samples(w_end, srate)
        if nsamples < window:
            raise Rejected("fewer input samples than the PRACH window")
    if not size_served(dft_size):
        raise Unsupported("DFT size %d" % dft_size)
    return dict(L=L, ra_scs_hz=scs_hz, dft_size=dft_size, nof_symbols=nof_symbols, K=K, k_bar=k_bar, nof_rb_ra=nof_rb_ra, window_samples=window,
                td_sample_offset=td_off, td_cp_samples=td_cp, k_start=k_start, grid=grid)


def window_samples(cfg):
    """The window length of a configuration whose own nof_samples is not known yet."""
    c = np.array(cfg, np.int64)
    c[C_NSAMPLES] = 1 << 30
    return int(geometry(c)["window_samples"])


def bins(g, fd):
    """DFT bins of the L sequence elements of a frequency-domain occasion."""
    return (g["k_start"][fd] - g["grid"] // 2 + np.arange(g["L"])) % g["dft_size"]


def demodulate(x, cfg, g=None):
    g = g or geometry(cfg)
    ntd, nfd, N = int(cfg[C_NTD]), int(cfg[C_NFD]), g["dft_size"]
    out = np.zeros((ntd, nfd, g["nof_symbols"], g["L"]), np.complex128)
    x = np.asarray(x, np.complex128)
    for td in range(ntd):
        first = g["td_sample_offset"][td] + g["td_cp_samples"][td]
        for s in range(g["nof_symbols"]):
            X = np.fft.fft(x[first + s * N:first + (s + 1) * N])
            for fd in range(nfd):
                out[td, fd, s] = X[bins(g, fd)]
    return out


def build_window(seed, cfg, noise_std=0.1, tx=()):
    """tx: (td, fd, u, cv, delay_samples, amplitude) per transmitted preamble, u the physical root and cv the cyclic shift of
    prach_ref.sequence. A preamble has unit power per subcarrier times amplitude^2 after the demodulator (whose DFT is unnormalised:
    the time-domain signal is scaled by 1 / dft_size). Noise: standard deviation noise_std per sample and dimension-pair."""
    g = geometry(cfg)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    n, N, L = int(cfg[C_NSAMPLES]), g["dft_size"], g["L"]
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (noise_std / np.sqrt(2))
    tables = P.header_tables()
    for td, fd, u, cv, delay, amp in tx:
        X = np.zeros(N, np.complex128)
        X[bins(g, fd)] = P.sequence(L, int(u), int(cv), tables) / np.sqrt(L) * amp * np.exp(1j * rng.uniform(0, 2 * np.pi))
        t = np.fft.ifft(X)  # one period; the demodulator's unnormalised DFT returns X
        cp, total = g["td_cp_samples"][td], g["td_cp_samples"][td] + g["nof_symbols"] * N
        idx = (np.arange(total) - cp - int(delay)) % N  # cyclic prefix and repetitions: the period continued both ways
        x[g["td_sample_offset"][td]:g["td_sample_offset"][td] + total] += t[idx]
    return x.astype(np.complex64)


def window_hash(x):
    return hashlib.sha256(np.ascontiguousarray(x, np.complex64).tobytes()).hexdigest()


def rel_err(got, ref):
    """The metric of tests/test_ofdm_gpu.py: max |difference| over the rms of the expected."""
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    return float(np.abs(got - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2)))


def fixture_tx(seed, cfg):
    """The transmissions of a fixture case, a function of its seed: one preamble per (td, fd) occasion with a random root, no cyclic
    shift, a delay inside the first half of the cyclic prefix and an amplitude around one."""
    g = geometry(cfg)
    rng = np.random.Generator(np.random.PCG64(int(seed) ^ 0x5DEECE66D))
    return [(td, fd, int(rng.integers(1, g["L"])), 0, int(rng.integers(0, g["td_cp_samples"][td] // 2 + 1)), float(rng.uniform(0.5, 1.5)))
            for td in range(int(cfg[C_NTD])) for fd in range(int(cfg[C_NFD]))]


def fixture_window(seed, cfg):
    return build_window(seed, cfg, 0.1, fixture_tx(seed, cfg))


_fixture = None


def fixture():
    """tests/golden/prach_demod.npz with its windows rebuilt, once per process: a list of dict(cfg, seed, sha256, window, expected) with
    expected the reference's output [td][fd][symbol][L] (complex64). Treat it as read-only."""
    global _fixture
    if _fixture is None:
        import os
        fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prach_demod.npz"))
        _fixture = []
        for i, cfg in enumerate(fx["cfg"]):
            g = geometry(cfg)
            exp = fx["out"][fx["out_offset"][i]:fx["out_offset"][i + 1]].reshape(int(cfg[C_NTD]), int(cfg[C_NFD]), g["nof_symbols"], g["L"])
            _fixture.append(dict(cfg=cfg, seed=int(fx["seed"][i]), sha256=str(fx["sha256"][i]), window=fixture_window(int(fx["seed"][i]), cfg),
                                 expected=exp, geometry=g))
    return _fixture


def job_of(cfg, samples_offset=0, buffer_offset=0, max_nof_fd_occasions=None, max_nof_symbols=None, g=None):
    """The PrachDemodJob fields of a configuration row as a tuple in the order of the record."""
    srate, fmt, mu, ntd, nfd, start, rb, nprb, nsamples = (int(v) for v in cfg)
    if max_nof_symbols is None:
        max_nof_symbols = (g or geometry(cfg))["nof_symbols"]
    return (fmt, mu, ntd, nfd, start, rb, nprb, nsamples, samples_offset, buffer_offset, nfd if max_nof_fd_occasions is None else max_nof_fd_occasions,
            max_nof_symbols)
