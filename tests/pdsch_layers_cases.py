"""Cases of the PDSCH modulator on one codeword and 1..4 layers (CPU only: numpy + oracle_lib), shared by tests/test_pdsch_layers.py, which
checks with the oracle alone that the fixture states the layer mapping of TS 38.211 7.3.1.3, and tests/test_pdsch_layers_gpu.py, which holds
the device against it. A case is a plain dict; codewords and grids derive from its name, so both files see the same bits."""
import zlib

import numpy as np

import dl_grid as D
import oracle_lib as O

GUARD = 64  # elements in front of and behind every grid that no job may touch
SCATTERED = [63, 64, 65, 127, 128, 191, 192, 255, 256, 274]  # a PRB on either side of every 64-bit word of the allocation mask


def _case(name, L, mod, nprb_grid, prbs, start=0, nof=1, dmrs=(), type2=0, cdm=1, bwp=None, reserved=(), ports=None, grid_ports=None, scaling=1.4125375,
          cw_pad=0):
    ports = list(range(L)) if ports is None else list(ports)
    prbs = np.asarray(list(prbs), dtype=np.uint16)
    res = []
    for (rprbs, re_mask, symbols) in reserved:
        pm = np.zeros(nprb_grid, np.uint8)
        pm[list(rprbs)] = 1
        res.append((pm, re_mask, symbols))
    return dict(name=name, L=L, mod=mod, nprb_grid=nprb_grid, prbs=prbs, start=start, nof=nof, dmrs=tuple(dmrs), type2=type2, cdm=cdm,
                bwp=(0, nprb_grid) if bwp is None else bwp, reserved=res, ports=ports, grid_ports=max(ports) + 1 if grid_ports is None else grid_ports,
                scaling=scaling, cw_pad=cw_pad, rnti=1 + zlib.crc32(name.encode()) % 65535, n_id=zlib.crc32(name.encode()[::-1]) % 1024)


def cases():
    out = []
    # base sweep: every number of layers with every modulation; three PRBs of a six-PRB grid over three symbols, DM-RS in the middle one
    for L in (1, 2, 3, 4):
        for mod in (1, 2, 4, 6, 8):
            out.append(_case("sweep_L%d_mod%d" % (L, mod), L, mod, 6, [1, 2, 4], start=1, nof=3, dmrs=(2,), cdm=1))
    # (a) pi/2-BPSK: the parity of the codeword symbol runs across the layers of one element
    out.append(_case("a_bpsk_L4", 4, 1, 1, [0]))
    # (b) 18 and 24 bits per element: the scrambling window straddles a sequence word at most elements
    out += [_case("b_L3_mod%d" % mod, 3, mod, 24, range(2, 22), nof=2) for mod in (6, 8)]
    # (c) 32 bits per element: the window at shift 0 of every word
    out.append(_case("c_L4_mod8", 4, 8, 12, range(1, 11), nof=2))
    # (d) an odd codeword byte offset forces the general path, its aligned twin takes the wide loads
    for L, mod, pad in ((2, 4, 1), (3, 4, 3), (2, 8, 1), (3, 8, 5)):
        out += [_case("d_L%d_mod%d_%s" % (L, mod, tag), L, mod, 12, range(0, 11), nof=2, dmrs=(1,), cdm=2, cw_pad=p) for tag, p in (("odd", pad), ("aligned", 0))]
    # (e) 275 PRBs in one symbol: every iteration of the per-thread loop, on the wide-load path and on the general one
    out += [_case("e_275prb_L2_mod%d" % mod, 2, mod, 275, range(275)) for mod in (8, 6)]
    # (f) PRBs on either side of every word of the allocation mask
    out.append(_case("f_scattered_L3_mod4", 3, 4, 275, SCATTERED, start=5, nof=2, dmrs=(6,), cdm=2))
    # (g) layers on ports that are not in order
    out.append(_case("g_ports_2031_L4_mod2", 4, 2, 8, range(1, 7), nof=2, ports=(2, 0, 3, 1), grid_ports=4))
    # (h) start symbol 2, 11 symbols, DM-RS on symbols 3 and 10, a BWP above PRB 0 that some allocated PRBs lie outside of, two reserved patterns
    # of which the first covers a DM-RS symbol
    res = [(range(6, 14), 0x0F3, (1 << 3) | (1 << 7)), (range(10, 25), 0x801, 1 << 12)]
    for tag, L, mod, type2, cdm in (("type1_cdm1", 2, 6, 0, 1), ("type1_cdm2", 3, 4, 0, 2), ("type2_cdm3", 2, 8, 1, 3)):
        out.append(_case("h_%s_L%d_mod%d" % (tag, L, mod), L, mod, 30, range(2, 23), start=2, nof=11, dmrs=(3, 10), type2=type2, cdm=cdm, bwp=(4, 24), reserved=res,
                         ports=(1, 3, 0)[:L], grid_ports=4))
    # (i) a scaling that is not a normal number is not applied
    out += [_case("i_scaling_%s" % tag, 2, 4, 6, [0, 3, 5], nof=2, scaling=s) for tag, s in (("zero", 0.0), ("nan", float("nan")))]
    # (j) scrambling sequences longer than the 185 344 bits one workgroup generates: six pieces on the wide-load path (the whole slot of 273 PRBs),
    # two on the general path; every later piece starts from a jump of both shift registers
    out.append(_case("j_273prb_14sym_L3_mod8", 3, 8, 273, range(273), nof=14, dmrs=(2,), cdm=2))
    out.append(_case("j_275prb_6sym_L2_mod6", 2, 6, 275, range(275), start=4, nof=6))
    # (k) the paths the one-layer and the layered entry point share, on the grid of (d). The 16QAM / 256QAM path at L = 1 with an odd codeword
    # offset, an aligned one, and at 256QAM one that is a multiple of 4 bytes but not of 8
    for mod, pad in ((4, 1), (4, 0), (8, 3), (8, 0), (8, 4)):
        out.append(_case("k_L1_mod%d_pad%d" % (mod, pad), 1, mod, 12, range(0, 11), nof=2, dmrs=(1,), cdm=2, cw_pad=pad))
    # ... the wide gathers of QPSK and 64QAM in the general loop at one and two layers, and QPSK on three, where the layers of one element start
    # at different alignments
    for L, mod, pad in ((1, 2, 1), (1, 2, 0), (2, 2, 1), (2, 2, 0), (1, 6, 3), (1, 6, 0), (2, 6, 1), (2, 6, 0), (3, 2, 1)):
        out.append(_case("k_L%d_mod%d_pad%d" % (L, mod, pad), L, mod, 12, range(0, 11), nof=2, dmrs=(1,), cdm=2, cw_pad=pad))
    assert len({c["name"] for c in out}) == len(out)
    return out


def dmrs_mask(c):
    dm = np.zeros(14, np.uint8)
    dm[list(c["dmrs"])] = 1
    return dm


def nof_re(c):
    """Data REs per layer, counted in numpy from the descriptor (O.pdsch_nof_re: brute force over symbols, PRBs and subcarriers)."""
    if "nof_re" not in c:  # (computed once per case)
        c["nof_re"] = O.pdsch_nof_re(c["prbs"], c["start"], c["nof"], dmrs_mask(c), c["type2"], c["cdm"], c["bwp"][0], c["bwp"][1], c["reserved"])
    return c["nof_re"]


def codeword(c):
    """REs x L x mod bits, one per byte; the upper bits of some bytes are set: only bit 0 of a byte is the bit."""
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    cw = rng.integers(0, 2, nof_re(c) * c["L"] * c["mod"], dtype=np.uint8)
    return cw | (rng.integers(0, 2, cw.size, dtype=np.uint8) << 1)


def grid_shape(c):
    return (c["grid_ports"], 14, c["nprb_grid"] * 12)


def background(c):
    return D.background(grid_shape(c), np.random.default_rng(zlib.crc32(c["name"].encode()) ^ 0x5A5A))


def oracle_modulate(c, grid, cw=None):
    """o_pdsch_modulate of the case on grid [ports][14][nsc] in place; returns what the oracle returns (REs per layer, or -1).

    One to three layers: the codeword as it is. Four layers: orc_pdsch_modulate takes them in the form of its reference, as TWO codeword arguments
    of two layers each (nof_cw = nof_layers >= 4 ? 2 : 1: layers 0, 1 carry symbols 2 i + ly of the first argument scrambled with c_init, layers
    2, 3 symbols 2 i + ly - 2 of the second scrambled with c_init + 2^14), and returns -1 when given one. The ONE codeword of TS 38.211 Table
    7.3.1.3-1 is therefore handed over as its two halves by layer pair, each bit pre-scrambled with the XOR of the sequence bit the oracle will
    apply and the one 7.3.1.1 applies to that bit of the one codeword (position (4 i + ly) mod + t of c_init's sequence), so that the oracle's
    own scrambling leaves exactly cw ^ c; the parity of 4 i + ly is that of 2 i + (ly mod 2), so pi/2-BPSK turns alike. That this call states
    x^(ly)(i) = d(4 i + ly), like the plain call for fewer layers, is what tests/test_pdsch_layers.py checks against numpy for every case."""
    cw = (codeword(c) if cw is None else cw) & 1
    cws, mod = [cw], c["mod"]
    if c["L"] == 4:
        c_init, n = (c["rnti"] << 15) + c["n_id"], cw.size // (4 * mod)
        bits, seq = cw.reshape(n, 4, mod), O.o_gold(c_init, 0, cw.size).reshape(n, 4, mod)
        cws = [np.ascontiguousarray((bits[:, 2 * q:2 * q + 2] ^ seq[:, 2 * q:2 * q + 2] ^ O.o_gold(c_init + (q << 14), 0, n * 2 * mod).reshape(n, 2, mod)).reshape(-1))
               for q in (0, 1)]
    return O.o_pdsch_modulate(c["rnti"], c["n_id"], c["scaling"], c["L"], [mod] * len(cws), cws, c["start"], c["nof"], dmrs_mask(c), c["type2"], c["cdm"], c["bwp"][0],
                              c["bwp"][1], c["prbs"], c["reserved"], c["ports"], c["nprb_grid"], grid)


def data_mask(c):
    """Boolean [14][nsc]: the data REs of the allocation (the same on every layer), in mapping order when flattened."""
    nprb, (bs, bz) = c["nprb_grid"], c["bwp"]
    k, r = np.arange(12), np.arange(nprb)
    dpat = ((k % 2) < c["cdm"]) if not c["type2"] else ((k % 6) < 2 * c["cdm"])
    ex = np.zeros((14, nprb, 12), bool)
    for s in c["dmrs"]:
        ex[s] |= ((r >= bs) & (r < bs + bz))[:, None] & dpat[None, :]
    for (pm, rm, sm) in c["reserved"]:
        ex |= (((sm >> np.arange(14)) & 1) == 1)[:, None, None] & (np.asarray(pm) != 0)[None, :, None] & (((rm >> k) & 1) == 1)[None, None, :]
    alloc = np.zeros((14, nprb, 12), bool)
    alloc[c["start"]:c["start"] + c["nof"], c["prbs"].astype(int), :] = True
    return (alloc & ~ex).reshape(14, nprb * 12)


def _scaled(d, scaling):
    s = np.float32(scaling)
    if np.isfinite(s) and abs(s) >= np.finfo(np.float32).tiny:  # std::isnormal
        d = (d.real * s + 1j * (d.imag * s)).astype(np.complex64)
    return d


def codeword_symbols(c, cw=None, exact=True):
    """TS 38.211 7.3.1.1-7.3.1.2 from the oracle's primitives: d(0 .. REs x L - 1) = O.nr_modulate(cw ^ O.o_gold(c_init, 0, nof_bits), mod) times
    the scaling when it is a normal number. O.nr_modulate divides the integer level by sqrt(average power) in double precision and rounds once;
    the mapper of the reference (modulation_mapper_impl.cpp:31-146, restated by the oracle and the device) multiplies the level by the single
    precision sqrtf(1 / average power), which differs in the last bit for some levels. exact = True recovers the integer levels from
    O.nr_modulate and forms that single-precision product, so that a comparison can be on the bits."""
    cw = (codeword(c) if cw is None else cw) & 1
    mod = c["mod"]
    d = O.nr_modulate(cw ^ O.o_gold((c["rnti"] << 15) + c["n_id"], 0, cw.size), mod)
    if exact:
        avg = {1: 2.0, 2: 2.0, 4: 10.0, 6: 42.0, 8: 170.0}[mod]
        sc = np.float32(np.sqrt(0.5)) if mod == 1 else np.sqrt(np.float32(1.0) / np.float32(avg), dtype=np.float32)
        lr, li = np.rint(d.real.astype(np.float64) * np.sqrt(avg)), np.rint(d.imag.astype(np.float64) * np.sqrt(avg))
        assert np.abs(lr * lr + li * li).max() <= 2 * (2 ** (mod // 2 if mod > 1 else 1) - 1) ** 2 and (lr % 2 != 0).all() and (li % 2 != 0).all()
        d = (lr.astype(np.float32) * sc + 1j * (li.astype(np.float32) * sc)).astype(np.complex64)
    return _scaled(d, c["scaling"])


def layer_symbols(c, cw=None, exact=True):
    """The layer mapping of TS 38.211 7.3.1.3 on codeword_symbols: row ly of the result [L][REs] is x^(ly)(i) = d(L i + ly)."""
    return np.ascontiguousarray(codeword_symbols(c, cw, exact).reshape(-1, c["L"]).T)


def grid_from_layer_symbols(c, bg, cw=None):
    """Copy of the background bg with x^(ly)(i) on the i-th data RE (symbol by symbol, ascending subcarrier) of port ports[ly]."""
    out = bg.copy()
    sy, k = np.nonzero(data_mask(c))
    out[np.asarray(c["ports"])[:, None], sy[None, :], k[None, :]] = layer_symbols(c, cw)
    return out
