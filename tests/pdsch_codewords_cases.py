"""Cases of the PDSCH modulator on two codewords and 5..8 layers (CPU only: numpy + oracle_lib), shared by tests/test_pdsch_codewords.py, which
checks with the oracle alone that o_pdsch_modulate with two codeword arguments states TS 38.211 7.3.1.1-7.3.1.3 and Table 7.3.1.3-1, and
tests/test_pdsch_codewords_gpu.py, which holds the device against it. The cases build on pdsch_layers_cases: a case is a case of that table (L = all
the layers, eight ports) plus mods = (mod0, mod1) and cw_pads = (pad0, pad1); codeword(c, q) of a case IS the case of that table on the layers,
modulation and ports of codeword q, so that its helpers (codeword, layer_symbols, grid_from_layer_symbols) serve each codeword as they are."""
import zlib

import numpy as np

import oracle_lib as O
import pdsch_layers_cases as PC
import pdsch_mapped_cases as MC

GUARD = PC.GUARD
SCATTERED = PC.SCATTERED
OUT_OF_ORDER = (7, 1, 3, 0, 2, 6, 5, 4)
ON_SIXTEEN = (15, 0, 9, 4, 12, 7, 2, 10)  # eight ports scattered over a 16-port grid


def _case(name, L, mods, nprb_grid, prbs, cw_pads=(0, 0), ports=None, **kw):
    assert 5 <= L <= 8
    ports = tuple(range(8)) if ports is None else tuple(ports)
    c = PC._case(name, L, mods[0], nprb_grid, prbs, ports=ports[:L], grid_ports=kw.pop("grid_ports", max(ports) + 1), **kw)
    c["mods"], c["cw_pads"], c["ports8"] = tuple(mods), tuple(cw_pads), ports
    return c


def split(L):
    """Layers of codeword 0 and of codeword 1 (TS 38.211 Table 7.3.1.3-1); (L, 0) up to four layers."""
    return (L // 2, L - L // 2) if L > 4 else (L, 0)


def cases():
    out = []
    # sweep: every number of layers with modulation pairs that put each order on either codeword; three PRBs of a six-PRB grid over three symbols,
    # DM-RS in the middle one
    for L in (5, 6, 7, 8):
        for mods in ((1, 8), (2, 1), (4, 8), (8, 4), (6, 2), (8, 8)):
            out.append(_case("sweep_L%d_mod%d_%d" % (L, *mods), L, mods, 6, [1, 2, 4], start=1, nof=3, dmrs=(2,), cdm=1))
    # (a) elements of 16 / 24 / 32 bits (2, 3, 4 layers of 256QAM) and 12 / 18 (64QAM): the scrambling window of each codeword straddles words differently
    for L in (5, 7):
        out += [_case("a_L%d_mod%d_%d" % (L, *mods), L, mods, 24, range(2, 22), nof=2) for mods in ((8, 8), (6, 8))]
    # (b) one codeword on the wide-load path and the other on the general loop: by modulation, and by an odd byte offset of either codeword
    for L in (6, 8):
        out += [_case("b_L%d_mod%d_%d" % (L, *mods), L, mods, 12, range(0, 11), nof=2, dmrs=(1,), cdm=2) for mods in ((4, 6), (8, 2))]
        out.append(_case("b_L%d_odd_cw0" % L, L, (8, 4), 12, range(0, 11), nof=2, dmrs=(1,), cdm=2, cw_pads=(1, 0)))
        out.append(_case("b_L%d_odd_cw1" % L, L, (4, 8), 12, range(0, 11), nof=2, dmrs=(1,), cdm=2, cw_pads=(0, 3)))
    # (c) 275 PRBs in one symbol: every iteration of the per-thread loop, both codewords on the wide-load path / one on each
    out += [_case("c_275prb_L8_mod%d_%d" % mods, 8, mods, 275, range(275)) for mods in ((8, 8), (6, 4))]
    # (d) PRBs on either side of every word of the allocation mask
    out.append(_case("d_scattered_L7", 7, (4, 6), 275, SCATTERED, start=5, nof=2, dmrs=(6,), cdm=2))
    # (e) layers on ports that are not in order, and on a grid of sixteen
    out.append(_case("e_ports_out_of_order_L8", 8, (2, 4), 8, range(1, 7), nof=2, ports=OUT_OF_ORDER))
    out.append(_case("e_ports_on_sixteen_L8", 8, (8, 6), 8, range(1, 7), nof=2, ports=ON_SIXTEEN, grid_ports=16))
    # (f) the "h" cases of the layered table: start symbol 2, 11 symbols, DM-RS on 3 and 10, a BWP above PRB 0, two reserved patterns
    res = [(range(6, 14), 0x0F3, (1 << 3) | (1 << 7)), (range(10, 25), 0x801, 1 << 12)]
    for tag, L, mods, type2, cdm in (("type1_cdm1", 5, (6, 4), 0, 1), ("type1_cdm2", 6, (4, 8), 0, 2), ("type2_cdm3", 8, (8, 6), 1, 3)):
        out.append(_case("f_%s_L%d" % (tag, L), L, mods, 30, range(2, 23), start=2, nof=11, dmrs=(3, 10), type2=type2, cdm=cdm, bwp=(4, 24), reserved=res,
                         ports=OUT_OF_ORDER))
    # (g) a scaling that is not a normal number is not applied, to either codeword
    out += [_case("g_scaling_%s" % tag, 6, (4, 2), 6, [0, 3, 5], nof=2, scaling=s) for tag, s in (("zero", 0.0), ("nan", float("nan")))]
    # (h) the whole slot of 273 PRBs: both scrambling sequences in several pieces of 185 344 bits
    out.append(_case("h_273prb_14sym_L8_mod8_8", 8, (8, 8), 273, range(273), nof=14, dmrs=(2,), cdm=2))
    # (i) a list in the order of the interleaved VRB-to-PRB mapping, bundles of 2 (what miphy_vrb_to_prb_list gives: tests/test_pdsch_codewords.py)
    for L, mods in ((5, (8, 4)), (8, (6, 8))):
        c = _case("i_interleaved_L%d" % L, L, mods, 30, MC.vrb_to_prb(2, 5, 19, 5)[[0, 1, 6, 7, 8, 15, 18]], start=2, nof=11, dmrs=(3, 10), cdm=2, bwp=(5, 19))
        c["vmap"], c["vrbs"] = (2, 5, 19, 5), (0, 1, 6, 7, 8, 15, 18)
        out.append(c)
    assert len({c["name"] for c in out}) == len(out)
    return out


def small(cs):
    """The cases of a few PRBs: what a mixed batch holds next to one large case."""
    return [c for c in cs if c["nprb_grid"] <= 48]


def codeword_case(c, q):
    """Codeword q of case c as a case of pdsch_layers_cases: its L_q layers on its slice of the ports, its modulation, c_init + q 2^14 (stated through
    n_id, which pdsch_layers_cases adds to rnti 2^15), bits of its own."""
    L0, L1 = split(c["L"])
    first, Lq = (0, L0) if q == 0 else (L0, L1)
    s = dict(c, name="%s/cw%d" % (c["name"], q), L=Lq, mod=c["mods"][q], ports=list(c["ports8"][first:first + Lq]), n_id=c["n_id"] + (q << 14),
             cw_pad=c["cw_pads"][q])
    s["nof_re"] = PC.nof_re(c)
    return s


def codewords(c):
    """The two codewords of the case, one bit per byte (upper bits of some bytes set)."""
    return [PC.codeword(codeword_case(c, q)) for q in (0, 1)]


def oracle_modulate(c, grid, cws=None):
    """o_pdsch_modulate with two codeword arguments on grid [ports][14][nsc] in place; returns what the oracle returns (REs per layer, or -1)."""
    cws = codewords(c) if cws is None else cws
    return O.o_pdsch_modulate(c["rnti"], c["n_id"], c["scaling"], c["L"], list(c["mods"]), [cw & 1 for cw in cws], c["start"], c["nof"], PC.dmrs_mask(c), c["type2"],
                              c["cdm"], c["bwp"][0], c["bwp"][1], c["prbs"], c["reserved"], list(c["ports8"][:c["L"]]), c["nprb_grid"], grid)


def data_res_in_list_order(c):
    """(symbol, subcarrier) of the data REs in mapping order: symbol by symbol, within a symbol PRB by PRB in the order of the list."""
    m = PC.data_mask(c).reshape(14, c["nprb_grid"], 12)
    sy, k = [], []
    for s in range(14):
        for rb in c["prbs"].astype(int):
            kk = np.nonzero(m[s, rb])[0]
            sy.append(np.full(kk.size, s))
            k.append(rb * 12 + kk)
    return np.concatenate(sy), np.concatenate(k)


def grid_from_38211(c, bg, cws=None):
    """The numpy statement: copy of bg in which codeword q has gone through PC.layer_symbols on its own layer count with c_init + q 2^14, layer ly of it
    onto the data REs (in list order) of port ports[first_q + ly]."""
    out = bg.copy()
    sy, k = data_res_in_list_order(c)
    for q in (0, 1):
        s = codeword_case(c, q)
        out[np.asarray(s["ports"])[:, None], sy[None, :], k[None, :]] = PC.layer_symbols(s, None if cws is None else cws[q])
    return out


def background(c):
    return PC.background(c)
