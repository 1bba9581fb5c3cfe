"""Cases of the PDSCH modulator with the PRBs of a job in mapping order (CPU only: numpy + oracle_lib), shared by tests/test_pdsch_mapped.py, which
checks with the oracle alone that the fixture states "the i-th data RE in list order carries x^(ly)(i)", and tests/test_pdsch_mapped_gpu.py, which
holds the device against it. The cases are those of pdsch_layers_cases in form (PC._case), and its helpers serve them as they are: c["prbs"] is the
list in mapping order, the allocation mask is its set. vrb_to_prb() states the mapping of TS 38.211 7.3.1.6 in numpy; every case is the smallest
shape that exercises its path."""
import numpy as np

import pdsch_layers_cases as PC

GUARD = PC.GUARD


def vrb_to_prb(L, align, N, first_prb=0):
    """TS 38.211 7.3.1.6: the PRB of every VRB 0 .. N - 1 of a region whose PRB 0 is grid PRB first_prb, bundles of L on a raster aligned to RB
    number `align` (L = 0: non-interleaved). Resource-block bundles: N_bundle = ceil((N + align mod L) / L); bundle 0 holds L - align mod L resource
    blocks, the last one what is left, every other one L. VRB bundle N_bundle - 1 is mapped to PRB bundle N_bundle - 1; VRB bundle j = c R + r
    (r = 0 .. R - 1, c = 0 .. C - 1, R = 2, C = floor(N_bundle / 2)) of the others to PRB bundle f(j) = r C + c."""
    n = np.arange(N)
    if L == 0:
        return first_prb + n
    s = align % L
    nb = -(-(N + s) // L)
    R, C = 2, nb // 2
    f = np.arange(nb)
    for c in range(C):
        for r in range(R):
            if c * R + r < nb - 1:
                f[c * R + r] = r * C + c
    bundle, pos = (n + s) // L, (n + s) % L  # bundle b holds the resource blocks b L - s .. b L - s + L - 1 of the region that exist
    return first_prb + f[bundle] * L + pos - s


def _mapped(name, L, mod, nprb_grid, vrbs, vmap, **kw):
    """A case whose list is the PRBs of the VRBs `vrbs` (ascending) under vmap = (bundle size, align, region size, first PRB)."""
    vrbs = np.asarray(sorted(vrbs))
    c = PC._case(name, L, mod, nprb_grid, vrb_to_prb(*vmap)[vrbs], **kw)
    c["vrbs"], c["vmap"] = vrbs, vmap
    return c


def cases():
    out = []
    # base sweep: the first size at which the mapping is no identity, [0 1 4 5 2 3 6 7]; symbols 1..3, DM-RS on 2: the general loop and both wide-load paths
    for L in (1, 2, 4):
        for mod in (2, 4, 6, 8):
            out.append(_mapped("sweep_L%d_mod%d" % (L, mod), L, mod, 8, range(8), (2, 0, 8, 0), start=1, nof=3, dmrs=(2,), cdm=1))
    # partial bundles: BWP (5, 19) with L_i = 4 -- a first bundle of 3 PRBs, a last one of 4; VRBs 3..13; the time allocation, reserved patterns and
    # ports of case (h) of pdsch_layers_cases
    res = [(range(6, 14), 0x0F3, (1 << 3) | (1 << 7)), (range(10, 25), 0x801, 1 << 12)]
    h = dict(start=2, nof=11, dmrs=(3, 10), cdm=2, bwp=(5, 19), reserved=res, grid_ports=4)
    for L, mod in ((3, 4), (2, 8)):
        out.append(_mapped("partial_bundles_L%d_mod%d" % (L, mod), L, mod, 30, range(3, 14), (4, 5, 19, 5), ports=(1, 3, 0)[:L], **h))
    # a type-0 allocation (a VRB bitmap) and interleaved, L_i = 2, same BWP
    for L, mod in ((1, 6), (2, 4)):
        out.append(_mapped("type0_L%d_mod%d" % (L, mod), L, mod, 30, (0, 1, 6, 7, 8, 15, 18), (2, 5, 19, 5), ports=(1, 3, 0)[:L], **h))
    # DCI 1_0 in a common search space: N = N_BWP,init = 24 from the CORESET's first PRB 7 of a BWP that starts at 10, raster aligned to 10 + 7
    out.append(_mapped("css_L1_mod2", 1, 2, 48, range(2, 22), (2, 17, 24, 17), nof=2, dmrs=(1,), cdm=2, bwp=(10, 38)))
    # 275 PRBs in one symbol: every iteration of the per-thread loops, lists that cross every 64-bit word of the mask
    out += [_mapped("e_275prb_L2_mod%d" % mod, 2, mod, 275, range(275), (2, 0, 275, 0)) for mod in (8, 6)]
    # an order no formula gives: the list itself is honoured (the grid of case (d), odd and aligned codeword offset)
    for tag, pad in (("odd", 1), ("aligned", 0)):
        c = PC._case("reversed_L2_mod4_%s" % tag, 2, 4, 12, range(10, -1, -1), nof=2, dmrs=(1,), cdm=2, cw_pad=pad)
        c["vrbs"], c["vmap"] = None, None
        out.append(c)
    # scrambling sequences of several pieces (case (j)), L_i = 4
    out.append(_mapped("j_273prb_14sym_L3_mod8", 3, 8, 273, range(273), (4, 0, 273, 0), nof=14, dmrs=(2,), cdm=2))
    assert len({c["name"] for c in out}) == len(out)
    return out


def small(cs):
    """The cases of a few PRBs: what a mixed batch holds."""
    return [c for c in cs if c["nprb_grid"] <= 48]


def ascending(c):
    """The case with its PRBs in ascending order (same name: same codeword, same grid)."""
    a = dict(c)
    a["prbs"] = np.sort(c["prbs"])
    return a


def grid_in_list_order(c, bg):
    """Copy of the background bg with x^(ly)(i) on the i-th data RE of port ports[ly], the data REs taken symbol by symbol, within a symbol PRB by
    PRB in the order of the list, subcarriers ascending inside a PRB."""
    out = bg.copy()
    dm = PC.data_mask(c).reshape(14, c["nprb_grid"], 12)
    prbs = c["prbs"].astype(int)
    sy_all, col_all = [], []
    for sy in range(c["start"], c["start"] + c["nof"]):
        pi, k = np.nonzero(dm[sy][prbs])  # row-major: list position first, then subcarrier
        sy_all.append(np.full(pi.size, sy))
        col_all.append(prbs[pi] * 12 + k)
    sy, col = np.concatenate(sy_all), np.concatenate(col_all)
    out[np.asarray(c["ports"])[:, None], sy[None, :], col[None, :]] = PC.layer_symbols(c)
    return out
