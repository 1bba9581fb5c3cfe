"""The numerical contract of precoding (CPU only: numpy + oracle_lib), shared by tests/test_pdsch_precoded.py, which checks the statements below against
a brute-force loop over REs, and the GPU tests of the precoded entry points (tests/test_precoder_gpu.py, tests/test_pdsch_precoded_gpu.py).

The contract is y_a = sum_ly W[prg][a][ly] x_ly in float64, of the exact float32 layer symbols (pdsch_layers_cases.layer_symbols(c, exact=True)) or of
the oracle's DM-RS (o_dmrs_pdsch_map of the L DM-RS ports onto a zeroed L-port staging grid), with float32 weights from a seeded generator whose parts
lie in +-[0.25, 1]. PRG g covers the grid PRBs [g prg_size, (g + 1) prg_size): the PRG of an RE follows its PRB's place in the grid.

Tolerance, derived and not measured: each real and each imaginary part of y is a dot product of n = 2 L real terms. Evaluated in float32, in any order
and with or without fused multiply-adds, it errs by at most gamma_n sum |a_i b_i| with gamma_n ~ n 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 3.1). A part must therefore lie within 2 x 2 L x 2^-24 x A of the float64 value, A being the sum of the absolute values of its 2 L real
products -- the factor 2 is margin over a bound that is already the worst case -- and where A = 0 the device value must be +-0. The float64 reference
is itself exact to 2^-53 A, far inside that."""
import zlib

import numpy as np

import dl_grid as D
import oracle_lib as O
import pdsch_layers_cases as PC

GUARD = PC.GUARD
EPS = 2.0 ** -24


def weights(tag, shape):
    """complex64 array of `shape` whose real and imaginary parts lie in +-[0.25, 1], from a generator seeded by the tag."""
    rng = np.random.default_rng(zlib.crc32(("weights " + tag).encode()))
    part = lambda: ((0.25 + 0.75 * rng.random(shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    return (part() + 1j * part()).astype(np.complex64)


def precode_ref(W, x):
    """The contract for n REs: W [n][P][L] (the matrix of each RE) or [P][L] (one matrix), x [L][n] complex64. Returns (y, A): y [P][n] complex128 in
    float64 arithmetic, A [P][n][2] the sum of the absolute values of the 2 L real products of the real and of the imaginary part."""
    W = np.asarray(W)
    x = np.asarray(x)
    if W.ndim == 2:
        W = np.broadcast_to(W, (x.shape[1],) + W.shape)
    wr, wi = W.real.astype(np.float64), W.imag.astype(np.float64)  # [n][P][L]
    xr, xi = x.real.astype(np.float64).T[:, None, :], x.imag.astype(np.float64).T[:, None, :]  # [n][1][L]
    y = (wr * xr - wi * xi).sum(axis=2) + 1j * (wr * xi + wi * xr).sum(axis=2)
    A = np.stack([(np.abs(wr * xr) + np.abs(wi * xi)).sum(axis=2), (np.abs(wr * xi) + np.abs(wi * xr)).sum(axis=2)], axis=-1)
    return np.ascontiguousarray(y.T), np.ascontiguousarray(A.transpose(1, 0, 2))


def excess(got, y, A, L):
    """got [P][n] complex64 against precode_ref's (y, A) for L layers: the largest error in units of the tolerance 2 x 2 L x 2^-24 x A over the parts with
    A > 0 (at most 1 passes), and the number of parts with A = 0 that are not +-0."""
    got = np.asarray(got)
    err = np.stack([np.abs(got.real.astype(np.float64) - y.real), np.abs(got.imag.astype(np.float64) - y.imag)], axis=-1)
    tol = 2.0 * 2 * L * EPS * A
    pos = A > 0
    worst = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    if not np.isfinite(err).all():
        worst = float("inf")
    return worst, int((err[~pos] != 0).sum())


def assert_within(got, y, A, L, what=""):
    worst, nonzero = excess(got, y, A, L)
    print("%s: largest error %.3f of the tolerance (2 x %d x 2^-24 x A); %d parts with A = 0 are not zero" % (what, worst, 2 * L, nonzero))
    assert worst <= 1.0 and nonzero == 0, what


# ---------------------------------------------------------------------------------------------------- PDSCH data
def precoded(c, P, prg_size, ports=None, grid_ports=None, nof_prg=None, tag=""):
    """A modulator case c of pdsch_layers_cases / pdsch_mapped_cases behind a precoding onto P antenna ports (grid port ports[a], default a) with PRGs of
    prg_size PRBs: a dict with the case, the geometry and W [nof_prg][P][L]."""
    ports = list(range(P)) if ports is None else list(ports)
    assert len(ports) == P
    nof_prg = -(-c["nprb_grid"] // prg_size) if nof_prg is None else nof_prg
    name = "%s_P%d_prg%d%s" % (c["name"], P, prg_size, tag)
    return dict(name=name, c=c, L=c["L"], P=P, prg_size=prg_size, nof_prg=nof_prg, ports=ports, grid_ports=max(ports) + 1 if grid_ports is None else grid_ports,
                W=weights(name, (nof_prg, P, c["L"])))


def grid_shape(pc):
    return (pc["grid_ports"], 14, pc["c"]["nprb_grid"] * 12)


def background(pc):
    return D.background(grid_shape(pc), np.random.default_rng(zlib.crc32(pc["name"].encode()) ^ 0xA5A5))


def data_positions(c):
    """(symbol, subcarrier) of the data REs in mapping order: symbol by symbol, within a symbol PRB by PRB in the order of c["prbs"] (ascending for the
    cases of pdsch_layers_cases, the list for those of pdsch_mapped_cases), subcarriers ascending inside a PRB."""
    dm = PC.data_mask(c).reshape(14, c["nprb_grid"], 12)
    prbs = c["prbs"].astype(int)
    sy_all, col_all = [], []
    for sy in range(c["start"], c["start"] + c["nof"]):
        pi, k = np.nonzero(dm[sy][prbs])
        sy_all.append(np.full(pi.size, sy))
        col_all.append(prbs[pi] * 12 + k)
    return np.concatenate(sy_all), np.concatenate(col_all)


def data_statement(pc):
    """(sy, col, y, A): the data RE of rank i sits at (sy[i], col[i]) and carries y[a][i] on antenna port a (precode_ref of the matrix of the PRG of its
    grid PRB col[i] // 12 and of x^(ly)(i))."""
    sy, col = data_positions(pc["c"])
    y, A = precode_ref(pc["W"][(col // 12) // pc["prg_size"]], PC.layer_symbols(pc["c"], exact=True))
    return sy, col, y, A


def data_statement_brute_force(pc):
    """data_statement by a loop over symbols, PRBs of the list, subcarriers, antenna ports and layers in Python floats (float64)."""
    c, W = pc["c"], pc["W"]
    x = PC.layer_symbols(c, exact=True)
    dm = PC.data_mask(c)
    sy_o, col_o, y, A, i = [], [], [], [], 0
    for sy in range(c["start"], c["start"] + c["nof"]):
        for rb in c["prbs"].astype(int):
            for k in range(12):
                if not dm[sy, rb * 12 + k]:
                    continue
                g = rb // pc["prg_size"]
                ya, Aa = [], []
                for a in range(pc["P"]):
                    re = im = are = aim = 0.0
                    for ly in range(c["L"]):
                        w, v = complex(W[g, a, ly]), complex(x[ly, i])
                        re += w.real * v.real - w.imag * v.imag
                        im += w.real * v.imag + w.imag * v.real
                        are += abs(w.real * v.real) + abs(w.imag * v.imag)
                        aim += abs(w.real * v.imag) + abs(w.imag * v.real)
                    ya.append(complex(re, im))
                    Aa.append((are, aim))
                sy_o.append(sy), col_o.append(rb * 12 + k), y.append(ya), A.append(Aa)
                i += 1
    assert i == x.shape[1]
    return np.array(sy_o), np.array(col_o), np.array(y).T, np.array(A).transpose(1, 0, 2)


def owned_mask(pc, sy, col):
    """Boolean [grid_ports][14][nsc]: the REs (sy, col) on the grid ports of the antenna ports -- what a precoded job may write."""
    m = np.zeros(grid_shape(pc), bool)
    m[np.asarray(pc["ports"])[:, None], sy[None, :], col[None, :]] = True
    return m


def check_grid(pc, got, bg, sy, col, y, A, what=None):
    """got, bg [grid_ports][14][nsc]: the owned REs of every antenna port are within the tolerance of (y, A), everything else holds the bits of bg."""
    owned = owned_mask(pc, sy, col)
    keep = ~np.repeat(owned[..., None], 2, axis=-1)
    stray = int((D.bits(got).reshape(keep.shape)[keep] != D.bits(bg).reshape(keep.shape)[keep]).sum())
    print("%s: %d words outside the job's REs differ from the background" % (what or pc["name"], stray))
    assert stray == 0
    assert_within(got[np.asarray(pc["ports"])[:, None], sy[None, :], col[None, :]], y, A, pc["L"], what or pc["name"])


# ---------------------------------------------------------------------------------------------------- PDSCH DM-RS
def dmrs_case(name, L, type2, symbols, nprb_grid, prbs, ref_point, P, prg_size, ports=None, grid_ports=None):
    """A precoded DM-RS job: DM-RS ports 1000 .. 1000 + L - 1 of type 1 / 2 in `symbols` on the PRBs `prbs`, onto P antenna ports."""
    ports = list(range(P)) if ports is None else list(ports)
    crc = zlib.crc32(name.encode())
    nof_prg = -(-nprb_grid // prg_size)
    rb = np.zeros(nprb_grid, np.uint8)
    rb[list(prbs)] = 1
    return dict(name=name, L=L, type2=type2, symbols=tuple(symbols), nprb_grid=nprb_grid, rb=rb, ref_point=ref_point, P=P, prg_size=prg_size, nof_prg=nof_prg,
                ports=ports, grid_ports=max(ports) + 1 if grid_ports is None else grid_ports, slot=crc % 20, scr=(crc >> 5) % 65536, n_scid=(crc >> 3) & 1,
                amplitude=float(np.float32(0.5 + (crc % 7) / 4.0)), W=weights(name, (nof_prg, P, L)))


def dmrs_staging(dc):
    """The oracle's DM-RS of the L DM-RS ports on a zeroed grid [L][14][nsc], DM-RS port ly on staging port ly: r_ly, and zero where port ly has none."""
    sm = np.zeros(14, np.uint8)
    sm[list(dc["symbols"])] = 1
    g = np.zeros((dc["L"], 14, dc["nprb_grid"] * 12), np.complex64)
    O.o_dmrs_pdsch_map(dc["slot"], dc["ref_point"], dc["type2"], dc["scr"], dc["n_scid"], dc["amplitude"], sm, dc["rb"], list(range(dc["L"])), g)
    return g


def dmrs_statement(dc):
    """(sy, col, y, A): the REs on which at least one of the L DM-RS ports has a value (the union of the oracle's per-layer masks: a DM-RS value is never
    zero), and on antenna port a the sum of W[prg][a][ly] r_ly over the layers -- a layer of another CDM group has r_ly = 0 there and adds nothing."""
    st = dmrs_staging(dc)
    sy, col = np.nonzero((st != 0).any(axis=0))
    y, A = precode_ref(dc["W"][(col // 12) // dc["prg_size"]], st[:, sy, col])
    return sy, col, y, A


def dmrs_statement_brute_force(dc):
    st = dmrs_staging(dc)
    sy_o, col_o, y, A = [], [], [], []
    for sy in range(14):
        for col in range(st.shape[2]):
            if not any(st[ly, sy, col] != 0 for ly in range(dc["L"])):
                continue
            g = (col // 12) // dc["prg_size"]
            ya, Aa = [], []
            for a in range(dc["P"]):
                re = im = are = aim = 0.0
                for ly in range(dc["L"]):
                    w, v = complex(dc["W"][g, a, ly]), complex(st[ly, sy, col])
                    re += w.real * v.real - w.imag * v.imag
                    im += w.real * v.imag + w.imag * v.real
                    are += abs(w.real * v.real) + abs(w.imag * v.imag)
                    aim += abs(w.real * v.imag) + abs(w.imag * v.real)
                ya.append(complex(re, im))
                Aa.append((are, aim))
            sy_o.append(sy), col_o.append(col), y.append(ya), A.append(Aa)
    return np.array(sy_o), np.array(col_o), np.array(y).T, np.array(A).transpose(1, 0, 2)


def dmrs_cases():
    """L = 1..4 of type 1 and L = 2, 4 of type 2; single and double symbols; a reference point above PRB 0 (PRBs below it carry nothing) and an allocation
    with a gap; P = L and P = 8; PRGs of 2 and 4 PRBs that the allocation straddles."""
    out = []
    prbs = [1, 2, 3, 6, 7, 9]
    for type2, Ls in ((0, (1, 2, 3, 4)), (1, (2, 4))):
        for L in Ls:
            for P in (L, 8):
                double = P == L
                out.append(dmrs_case("dmrs_type%d_L%d_P%d" % (type2 + 1, L, P), L, type2, (2, 3, 11) if double else (2, 11), 10, prbs, 2 if L % 2 else 0, P,
                                     2 if P == L else 4, ports=None if P == L else (5, 0, 9, 2, 1, 7, 3, 8), grid_ports=P if P == L else 10))
    assert len({d["name"] for d in out}) == len(out)
    return out
