"""PUSCH on 1..4 transmit layers, on the host: what the layered equaliser and demodulator of the library are held to. The 23.5 reference stops
at one layer (its demodulator asserts it) and at 1 x N / 2 x 2 in the equaliser, so beyond those the contract is restated here:

  channels()        H = U diag(s) V^H per subcarrier with s in [0.5, 2]: cond(H^H H) <= 16 by construction, no element needs excluding
  zf_double()       float64 pseudo-inverse: x = pinv(H) y / tx, nvar_l = noise_var [(H^H H)^-1]_ll / tx^2
  zf_single()       numpy float32 in the operation order of csrc/equalize_device.h (what the device must reproduce bit for bit)
  extract()         the data resource elements of an allocation, symbol-major, subcarrier ascending, and the estimate at each
  expected_llr()    equalised symbols and variances interleaved [element][layer] (TS 38.211 6.3.1.3), the oracle's soft demapper, sign flip
                    with the oracle's Gold sequence: c_init = rnti * 2^15 + n_id
  transmit()        the oracle's encoder on L layers, scrambling, the oracle's mapper, layer mapping, H and noise: a grid to receive

test_pusch_layers.py pins these to the oracle where it has a say (one layer, 2 x 2) and to each other elsewhere."""
import numpy as np

import oracle_lib as O

F = np.float32
TINY = np.finfo(np.float32).tiny
TOPOLOGIES = [(l, p) for l in range(1, 5) for p in range(l, 5)]  # (layers, ports); the nine beyond one layer plus 1 x N
LAYERED = [(l, p) for (l, p) in TOPOLOGIES if l >= 2]


# ------------------------------------------------------------------------------------------------ channels
def channels(rng, nl, npt, n, smin=0.5, smax=2.0):
    """complex64 [layer][port][n] and the float64 condition number of H^H H per element."""
    a = rng.standard_normal((n, npt, nl)) + 1j * rng.standard_normal((n, npt, nl))
    u = np.linalg.qr(a)[0]  # [n][P][L], orthonormal columns
    b = rng.standard_normal((n, nl, nl)) + 1j * rng.standard_normal((n, nl, nl))
    v = np.linalg.qr(b)[0]
    s = rng.uniform(smin, smax, (n, nl))
    h = np.einsum("npl,nl,nkl->npk", u, s, v.conj())  # U diag(s) V^H
    h = np.ascontiguousarray(h.transpose(2, 1, 0)).astype(np.complex64)
    return h, cond_g(h)


def cond_g(h):
    hh = h.astype(np.complex128).transpose(2, 1, 0)  # [n][P][L]
    sv = np.linalg.svd(hh, compute_uv=False)
    return (sv[:, 0] / sv[:, -1]) ** 2


# ------------------------------------------------------------------------------------------------ zero forcing
def zf_double(y, h, noise_var, tx):
    hh = h.astype(np.complex128).transpose(2, 1, 0)  # [n][P][L]
    yy = y.astype(np.complex128).T[:, :, None]
    x = (np.linalg.pinv(hh) @ yy)[:, :, 0] / tx
    gi = np.linalg.inv(hh.conj().transpose(0, 2, 1) @ hh)
    nv = noise_var * np.real(np.einsum("nll->nl", gi)) / tx ** 2
    return x.T, nv.T


def _cm(a, b):  # conj(a) b
    return (a[0] * b[0] + a[1] * b[1], a[0] * b[1] - a[1] * b[0])


def _mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _mulc(a, b):  # a conj(b)
    return (a[0] * b[0] + a[1] * b[1], a[1] * b[0] - a[0] * b[1])


def _norm(a):
    return a[0] * a[0] + a[1] * a[1]


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def _dot(a, b, from_zero=False):
    s = _cm(a[0], b[0])
    if from_zero:
        s = (F(0) + s[0], F(0) + s[1])
    for p in range(1, len(a)):
        s = _add(s, _cm(a[p], b[p]))
    return s


def _col_norm(a):
    s = _norm(a[0])
    for p in range(1, len(a)):
        s = s + _norm(a[p])
    return s


def _normal(x):
    a = np.abs(x)
    return (a >= TINY) & (a < np.inf)


def zf_single(y, h, noise_var, tx):
    """y complex64 [P][n], h complex64 [L][P][n] -> (x complex64 [L][n], nvar float32 [L][n]); csrc/equalize_device.h, operation for operation."""
    y = np.asarray(y, np.complex64)
    h = np.asarray(h, np.complex64)
    nl, npt, n = h.shape
    H = [[(np.ascontiguousarray(h[l, p].real), np.ascontiguousarray(h[l, p].imag)) for p in range(npt)] for l in range(nl)]
    Y = [(np.ascontiguousarray(y[p].real), np.ascontiguousarray(y[p].imag)) for p in range(npt)]
    nvar, tx = F(noise_var), F(tx)
    nv_ok = bool(_normal(nvar)) and bool(nvar > 0)
    one = F(1)
    with np.errstate(all="ignore"):
        m = [_dot(H[l], Y, from_zero=(nl == 1)) for l in range(nl)]
        if nl == 1:
            d = tx * (F(0) + _col_norm(H[0]))
            ok = _normal(d) & nv_ok
            r = one / d
            x = [(m[0][0] * r, m[0][1] * r)]
            nv = [r * (nvar / tx)]
        elif nl == 2:
            n0, n1 = _col_norm(H[0]), _col_norm(H[1])
            xr, xi = _dot(H[0], H[1])
            xm = xr * xr + xi * xi
            d_pinv = tx * ((n0 * n1) - xm)
            d_nvars = tx * d_pinv
            ok = _normal(d_pinv) & nv_ok
            rp, rn = one / d_pinv, one / d_nvars
            x = [((n1 * m[0][0] - (xr * m[1][0] - xi * m[1][1])) * rp, (n1 * m[0][1] - (xr * m[1][1] + xi * m[1][0])) * rp),
                 ((n0 * m[1][0] - (xr * m[0][0] + xi * m[0][1])) * rp, (n0 * m[1][1] - (xr * m[0][1] - xi * m[0][0])) * rp)]
            nv = [nvar * n1 * rn, nvar * n0 * rn]
        else:
            w = [[None] * nl for _ in range(nl)]
            lf = [[None] * nl for _ in range(nl)]
            r = [None] * nl
            ok = np.full(n, nv_ok)
            zero = np.zeros(n, F)
            for j in range(nl):
                for i in range(j, nl):
                    acc = (_col_norm(H[j]), zero) if i == j else _dot(H[i], H[j])
                    for k in range(j):
                        t = _mulc(w[i][k], lf[j][k])
                        acc = (acc[0] - t[0], zero) if i == j else (acc[0] - t[0], acc[1] - t[1])
                    w[i][j] = acc
                dj = w[j][j][0]
                rd = one / dj
                for i in range(j + 1, nl):
                    lf[i][j] = (w[i][j][0] * rd, w[i][j][1] * rd)
                dt = tx * dj
                r[j] = one / dt
                ok = ok & _normal(dj) & _normal(dt)
            M = [[None] * nl for _ in range(nl)]
            for j in range(nl):
                for i in range(j + 1, nl):
                    acc = lf[i][j]
                    for k in range(j + 1, i):
                        acc = _add(acc, _mul(lf[i][k], M[k][j]))
                    M[i][j] = (-acc[0], -acc[1])
            s = nvar / tx
            nv = []
            for a in range(nl):
                acc = r[a]
                for k in range(a + 1, nl):
                    acc = acc + _norm(M[k][a]) * r[k]
                nv.append(acc * s)
            z = []
            for i in range(nl):
                acc = m[i]
                for j in range(i):
                    acc = _add(acc, _mul(M[i][j], m[j]))
                z.append((acc[0] * r[i], acc[1] * r[i]))
            x = []
            for a in range(nl):
                acc = z[a]
                for k in range(a + 1, nl):
                    acc = _add(acc, _cm(M[k][a], z[k]))
                x.append(acc)
        xo = np.zeros((nl, n), np.complex64)
        no = np.zeros((nl, n), F)
        for l in range(nl):
            xo[l].real = np.where(ok, x[l][0], F(0))
            xo[l].imag = np.where(ok, x[l][1], F(0))
            no[l] = np.where(ok, nv[l], F(np.inf))
    return xo, no


# ------------------------------------------------------------------------------------------------ allocations
def case(name, nl, npt, mod, nprb_grid=24, prbs=tuple(range(2, 10)) + tuple(range(14, 18)), start=2, nof=12, dmrs=(2, 11), type2=0, cdm=2, compact=True,
         rx_ports=(0, 1, 2, 3), rnti=0x4601, n_id=900, noise_var=0.02, seed=0):
    return dict(name=name, nl=nl, npt=npt, mod=mod, nprb_grid=nprb_grid, prbs=tuple(prbs), start=start, nof=nof, dmrs=tuple(dmrs), type2=type2, cdm=cdm,
                compact=compact, rx_ports=tuple(rx_ports), rnti=rnti, n_id=n_id, noise_var=noise_var, seed=seed)


def masks(c):
    rb = np.zeros(c["nprb_grid"], np.uint8)
    rb[list(c["prbs"])] = 1
    dm = np.zeros(14, np.uint8)
    dm[[s for s in c["dmrs"] if c["start"] <= s < c["start"] + c["nof"]]] = 1
    return rb, dm


def data_positions(c):
    """(symbol, subcarrier) of every data element, in codeword order."""
    rb, dm = masks(c)
    sub = np.nonzero(np.repeat(rb, 12))[0]
    k = sub % 12
    is_dmrs = (k % 6 < 2 * c["cdm"]) if c["type2"] else (k % 2 < c["cdm"])
    sy, sc = [], []
    for s in range(c["start"], c["start"] + c["nof"]):
        keep = sub[~is_dmrs] if dm[s] else sub
        sy.append(np.full(keep.size, s))
        sc.append(keep)
    return np.concatenate(sy), np.concatenate(sc)


def nof_re(c):
    return data_positions(c)[0].size


def extract(c, grid, ce):
    """grid [4][14][nsc], ce [L][P][ce_syms or 1][nsc] -> y [P][n], h [L][P][n] at the data elements."""
    sy, sc = data_positions(c)
    y = np.stack([grid[c["rx_ports"][p], sy, sc] for p in range(c["npt"])]).astype(np.complex64)
    row = np.zeros_like(sy) if c["compact"] else sy
    h = np.stack([np.stack([ce[l, p, row, sc] for p in range(c["npt"])]) for l in range(c["nl"])]).astype(np.complex64)
    return y, h


def compose_llr(c, x, nv):
    """Equalised symbols x [L][n] and variances nv [L][n] -> the descrambled codeword."""
    sym = np.ascontiguousarray(x.T).reshape(-1)  # [element][layer]
    var = np.ascontiguousarray(nv.T).reshape(-1)
    llr = O.o_demodulate_soft(c["mod"], sym, var)
    chips = O.o_gold((c["rnti"] << 15) + c["n_id"], 0, llr.size)
    return np.where(chips != 0, -llr.astype(np.int16), llr.astype(np.int16)).astype(np.int8)


def expected_llr(c, grid, ce, equalize=zf_single):
    y, h = extract(c, grid, ce)
    x, nv = equalize(y, h, c["noise_var"], 1.0)
    return compose_llr(c, x, nv)


# ------------------------------------------------------------------------------------------------ transmitter
def random_slot(c, rng=None):
    """A grid of random samples and an estimate from channels(): what the demodulator tests feed (no transport block behind it).
    Returns (grid [4][14][nsc], ce [L][P][rows][nsc])."""
    rng = rng or np.random.default_rng(c["seed"])
    nsc = c["nprb_grid"] * 12
    rows = 1 if c["compact"] else 14
    h, _ = channels(rng, c["nl"], c["npt"], rows * nsc)
    ce = h.reshape(c["nl"], c["npt"], rows, nsc)
    grid = (rng.standard_normal((4, 14, nsc)) + 1j * rng.standard_normal((4, 14, nsc))).astype(np.complex64)
    return grid, np.ascontiguousarray(ce)


def transmit(c, bits=None, tb=None, bg=1, snr_db=None, rng=None):
    """Codeword (given as `bits`, or encoded from the transport block `tb` by the oracle on nl layers) -> scrambled, mapped by the oracle,
    layer-mapped, through a compact channel from channels() plus noise. snr_db None: noise free. Returns (grid, ce, codeword bits)."""
    rng = rng or np.random.default_rng(c["seed"])
    nl, npt, mod = c["nl"], c["npt"], c["mod"]
    sy, sc = data_positions(c)
    n = sy.size
    if bits is None:
        bits = O.o_pdsch_encode(bg, 0, mod, 0, nl, n * nl, tb)
    assert bits.size == n * nl * mod
    scr = bits ^ O.o_gold((c["rnti"] << 15) + c["n_id"], 0, bits.size)
    x = O.o_modulate(mod, scr).reshape(n, nl).T  # layer ly carries symbols ly, L + ly, ...
    nsc = c["nprb_grid"] * 12
    h, _ = channels(rng, nl, npt, nsc)
    grid = np.full((4, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    for p in range(npt):
        g = (rng.standard_normal((14, nsc)) + 1j * rng.standard_normal((14, nsc))).astype(np.complex64)  # DM-RS and unallocated elements: anything
        rx = np.einsum("ln,ln->n", h[:, p, sc].astype(np.complex128), x.astype(np.complex128))
        if snr_db is not None:
            rx = rx + 10 ** (-snr_db / 20) * np.sqrt(0.5) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        g[sy, sc] = rx.astype(np.complex64)
        grid[c["rx_ports"][p]] = g
    ce = np.ascontiguousarray(h.reshape(nl, npt, 1, nsc))
    if not c["compact"]:
        ce = np.ascontiguousarray(np.repeat(ce, 14, axis=2))
    return grid, ce, bits


# ------------------------------------------------------------------------------------------------ grid to bytes
CHAIN_CASES = [  # (layers, ports, modulation, transport block bytes (TS 38.214 sizes of 2 and 6 codeblocks), SNR dB): 24 PRB
    (2, 2, 4, 1497, 16.0),
    (4, 4, 8, 5997, 30.0),
]


def chain_case(nl, npt, mod):
    return case("chain", nl, npt, mod, prbs=range(24), start=0, nof=14, dmrs=(2, 11), noise_var=None, seed=7 * nl + mod)


def chain_transmission(nl, npt, mod, tb_bytes, snr_db):
    c = chain_case(nl, npt, mod)
    c["noise_var"] = float(10 ** (-snr_db / 10))
    rng = np.random.default_rng(c["seed"])
    tb = rng.integers(0, 256, tb_bytes, dtype=np.uint8)
    grid, ce, cw = transmit(c, tb=tb, bg=1, snr_db=snr_db, rng=rng)
    return c, tb, grid, ce


# ------------------------------------------------------------------------------------------------ jobs of the library
def mask_words(rb):
    w = np.zeros(5, dtype=np.uint64)
    for r in np.nonzero(rb)[0]:
        w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def demod_job(miphy, c, grid_off=0, ce_off=0, sc_off=0, llr_off=0):
    rb, dm = masks(c)
    arr = np.zeros(1, dtype=miphy.PuschDemodLayersJob)
    lj, j = arr[0], arr["base"]  # (views of the one record)
    j["rnti"], j["n_id"], j["mod"], j["nof_rx_ports"], j["start_symbol"], j["nof_symbols"] = c["rnti"], c["n_id"], c["mod"], c["npt"], c["start"], c["nof"]
    j["dmrs_type"], j["nof_cdm_groups_without_data"], j["ce_nof_symbols"], j["ce_compact"] = 2 if c["type2"] else 1, c["cdm"], 14, int(c["compact"])
    j["rx_ports"] = list(c["rx_ports"])
    j["dmrs_symbols_mask"] = sum(1 << int(s) for s in np.nonzero(dm)[0])
    j["grid_nof_prb"] = rb.size
    j["rb_mask"] = mask_words(rb)
    j["grid_offset"], j["ce_offset"], j["scalars_offset"], j["llr_offset"] = grid_off, ce_off, sc_off, llr_off
    lj["nof_tx_layers"] = c["nl"]
    j["nof_llr"] = nof_re(c) * c["nl"] * c["mod"]
    return lj


def equalizer_job(miphy, nre, npt, nl, noise_var, tx, y_off=0, h_off=0, z_off=0, nv_off=0):
    j = np.zeros(1, dtype=miphy.EqualizerJob)[0]
    j["nof_re"], j["nof_rx_ports"], j["nof_tx_layers"], j["noise_var"], j["tx_scaling"] = nre, npt, nl, noise_var, tx
    j["ch_symbols_offset"], j["ch_estimates_offset"], j["eq_symbols_offset"], j["eq_noise_vars_offset"] = y_off, h_off, z_off, nv_off
    return j
