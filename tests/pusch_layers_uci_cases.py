"""PUSCH on 2..4 layers with multiplexed UCI and the EVM, on the host: what miphy_pusch_demodulate_layers_batch_ex and
miphy_pusch_process_layers_batch_ex are held to. The 23.5 reference asserts one layer in its demodulator, so above one layer the contract is
restated here from TS 38.211 6.3.1.1 and TS 38.212 6.3.2 (no device code):

  CASES / build()   four transmissions: UCI fields encoded (uci_short_block, uci_polar), multiplexed with the UL-SCH bits through the map read off the
                    oracle's demultiplexer at nof_layers = L (pusch_uci_tx.mux_map), scrambled with the per-symbol placeholder rule
  scramble()        a listed resource element i carries the pattern [c0 y x ..] in EACH of its L codeword symbols L i + ly: y repeats the scrambled
                    bit in front of it, x is 1
  compose_llr()     pusch_layers_cases.compose_llr with the placeholder chips: in such a symbol bit 0 takes its own chip c((L i + ly) mod), bit 1
                    that same chip, the bits behind them none
  evm_terms()       per codeword symbol |ideal - equalised|^2 in float32 (two subtractions, two products, one sum), the ideal point from the hard
                    decision on the soft bits before descrambling (l <= 0 -> bit 1), pi/2-BPSK rotated by the parity of L i + ly
  transmit_true()   layers and channel as pusch_layers_cases.transmit (the true channel is the estimate)
  chain_tx()        as pusch_layers_estimator_cases.chain_tx (DM-RS of every layer, smooth channel): what the fused processor receives

test_pusch_layers_uci.py pins the restatements to the oracle at one layer and shows that the four cases decode in the host chain."""
import numpy as np

import oracle_lib as O
import pusch_layers_cases as PL
import pusch_layers_estimator_cases as E
import uci_polar as UP
import uci_short_block as SB
from pusch_uci_tx import mux_map

F = np.float32
NPRB, DMRS = 24, (2, 7, 11)
# layers, ports, modulation, transport block bytes (None: UCI only), SNR dB, O = information bits of (HARQ-ACK, CSI part 1, CSI part 2),
# G and reserved HARQ-ACK elements in resource elements (x L x mod bits)
CASES = {
    "A": dict(nl=2, npt=2, mod=4, tb_bytes=1497, snr_db=16.0, O=(1, 4, 0), G_re=(20, 30, 0), rvd_re=40),   # 20 placeholder REs, punctured UL-SCH
    "B": dict(nl=4, npt=4, mod=8, tb_bytes=5997, snr_db=30.0, O=(20, 11, 7), G_re=(10, 30, 25), rvd_re=0),  # polar HARQ-ACK (E = 320), CSI part 2
    "C": dict(nl=2, npt=4, mod=2, tb_bytes=None, snr_db=10.0, O=(2, 6, 0), G_re=(24, 30, 0), rvd_re=40),   # UCI only
    "D": dict(nl=3, npt=3, mod=6, tb_bytes=None, snr_db=25.0, O=(1, 1, 0), G_re=(20, 30, 0), rvd_re=40),   # 50 placeholder REs in two fields, odd L
}


def allocation(nl, npt, mod, seed=None, nprb=NPRB, dmrs=DMRS, **kw):
    """24 PRB, symbols 0..13, type 1, two CDM groups without data, DM-RS on symbols 2, 7 and 11, as pusch_layers_cases.case()."""
    kw.setdefault("noise_var", None)
    return PL.case("uci", nl, npt, mod, nprb_grid=nprb, prbs=range(nprb), start=0, nof=14, dmrs=dmrs, seed=7 * nl + mod if seed is None else seed, **kw)


def mux_case(c, O_bits, G_re, rvd_re):
    """The arguments of oracle_lib.o_ulsch_demultiplex for allocation c."""
    rb, dm = PL.masks(c)
    k = c["nl"] * c["mod"]
    return (c["mod"], c["nl"], int(rb.sum()), c["start"], c["nof"], rvd_re * k, 2 if c["type2"] else 1, sum(1 << int(s) for s in np.nonzero(dm)[0]), c["cdm"],
            tuple(g * k for g in G_re), tuple(O_bits))


def c_init(c):
    return (c["rnti"] << 15) + c["n_id"]


def wide_mux_map(mc, n_in):
    """pusch_uci_tx.mux_map, whose three digits end at 10^6 soft bits, with a fourth one (tools/pusch_layers_uci_throughput.py: 273 PRB on four layers)."""
    if n_in <= 100 ** 3:
        return mux_map(mc, n_in)
    idx = np.arange(n_in)
    digs = [O.o_ulsch_demultiplex(*mc, llr=((idx // (100 ** d)) % 100 + 1).astype(np.int8))[2] for d in range(4)]
    maps = []
    for k in range(4):
        a = [digs[d][k].astype(np.int64) for d in range(4)]
        src = sum((a[d] - 1) * 100 ** d for d in range(4))
        src[a[0] == 0] = -1
        maps.append(src)
    return maps


# ------------------------------------------------------------------------------------------------ fields
def encode_field(nof_bits, E_bits, mod, payload):
    if nof_bits <= 11:
        return SB.rate_match(SB.encode(payload, mod), E_bits)
    return UP.encode(nof_bits, E_bits, payload)


def decode_field(nof_bits, mod, llr):
    """-> (payload bits, valid)."""
    if nof_bits <= 11:
        bits, status = SB.detect(np.asarray(llr, np.int8), nof_bits, mod)
        return bits, status == SB.STATUS_VALID
    return UP.decode(nof_bits, len(llr), llr)


# ------------------------------------------------------------------------------------------------ scrambling with placeholders
def placeholder_symbols(ph, nl):
    """Codeword symbols of the listed resource elements: L i + ly."""
    ph = np.asarray(ph, np.int64)
    return (ph[:, None] * nl + np.arange(nl)[None, :]).reshape(-1)


def x_positions(nbits, ph, nl, mod):
    """The bits that carry an x placeholder (never descrambled, their value says nothing)."""
    m = np.zeros(nbits, bool)
    for s in placeholder_symbols(ph, nl):
        m[s * mod + 2:(s + 1) * mod] = True
    return m


def scramble(c, cw, ph):
    s = cw ^ O.o_gold(c_init(c), 0, cw.size)
    mod = c["mod"]
    for q in placeholder_symbols(ph, c["nl"]):
        s[q * mod + 1] = s[q * mod]
        s[q * mod + 2:(q + 1) * mod] = 1
    return s


def chips(c, nbits, ph):
    """(chip of every soft bit, 0 where it is not descrambled)."""
    ch = O.o_gold(c_init(c), 0, nbits).copy()
    mod = c["mod"]
    for q in placeholder_symbols(ph, c["nl"]):
        ch[q * mod + 1] = ch[q * mod]
        ch[q * mod + 2:(q + 1) * mod] = 0
    return ch


def soft_bits(c, x, nv):
    """Equalised symbols x [L][n] and variances nv [L][n] -> (symbols, quantised soft bits before descrambling), [element][layer]."""
    sym = np.ascontiguousarray(x.T).reshape(-1)
    var = np.ascontiguousarray(nv.T).reshape(-1)
    return sym, O.o_demodulate_soft(c["mod"], sym, var)


def compose_llr(c, x, nv, ph=()):
    _, llr = soft_bits(c, x, nv)
    ch = chips(c, llr.size, ph)
    return np.where(ch != 0, -llr.astype(np.int16), llr.astype(np.int16)).astype(np.int8)


# ------------------------------------------------------------------------------------------------ EVM
def ideal_points(mod, hard, first=0):
    """csrc/mod_device.h map_symbol: hard [n][mod] bits -> (re, im) float32; the constellation scale is one float32 constant per modulation."""
    hard = np.asarray(hard, np.int64).reshape(-1, mod)
    n = hard.shape[0]
    if mod == 1:
        v = F(0.70710678118654752440)
        s = np.where(hard[:, 0] != 0, -v, v).astype(F)
        odd = ((np.arange(n) + first) & 1) != 0
        return np.where(odd, -s, s).astype(F), s
    h = mod // 2
    lr, li = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(h - 1, -1, -1):
        w = 1 << (h - 1 - j)
        lr = (1 - 2 * hard[:, 2 * j]) * (w - lr)
        li = (1 - 2 * hard[:, 2 * j + 1]) * (w - li)
    sc = np.sqrt(F(1) / F({2: 2, 4: 10, 6: 42, 8: 170}[mod]))
    assert sc.dtype == F
    return lr.astype(F) * sc, li.astype(F) * sc


def evm_terms(c, x, nv):
    """float32 [n L]: the term of codeword symbol L i + ly."""
    sym, llr = soft_bits(c, x, nv)
    ir, ii = ideal_points(c["mod"], llr.reshape(-1, c["mod"]) <= 0)
    er, ei = ir - sym.real.astype(F), ii - sym.imag.astype(F)
    with np.errstate(all="ignore"):
        return (er * er + ei * ei).astype(F)


def evm_symbol_sums(c, terms):
    """float64 [14]: the terms of every OFDM symbol (all elements, all layers) added in double precision."""
    sy, _ = PL.data_positions(c)
    out = np.zeros(14)
    np.add.at(out, np.repeat(sy, c["nl"]), terms.astype(np.float64))
    return out


# ------------------------------------------------------------------------------------------------ transmissions
def build(name, case=None):
    """case: a record as those of CASES (optional keys nprb, dmrs). -> dict: c (allocation), mc (mux case), n_in, n_sch, ph, tb (or None), payloads (three arrays), cw (multiplexed bits), scr (scrambled bits),
    maps (per stream the codeword index of every position, -1: punctured)."""
    k = dict(case or CASES[name])
    c = allocation(k["nl"], k["npt"], k["mod"], nprb=k.get("nprb", NPRB), dmrs=k.get("dmrs", DMRS), noise_var=float(10 ** (-k["snr_db"] / 10)))
    rng = np.random.default_rng(1000 + c["seed"])
    mc = mux_case(c, k["O"], k["G_re"], k["rvd_re"])
    info = O.o_ulsch_demultiplex(*mc)
    assert info is not None
    n_in, n_sch, _, ph = info
    assert n_in == PL.nof_re(c) * k["nl"] * k["mod"]
    tb = rng.integers(0, 256, k["tb_bytes"], dtype=np.uint8) if k["tb_bytes"] else None
    sch = O.o_pdsch_encode(1, 0, k["mod"], 0, k["nl"], n_sch // k["mod"], tb) if tb is not None else rng.integers(0, 2, n_sch, dtype=np.uint8)
    payloads = [rng.integers(0, 2, o, dtype=np.uint8) for o in k["O"]]
    fields = [encode_field(o, g, k["mod"], p) if o else np.zeros(0, np.uint8) for o, g, p in zip(k["O"], mc[9], payloads)]
    maps = wide_mux_map(mc, n_in)
    cw = np.zeros(n_in, np.uint8)
    for m, bits in zip(maps, [sch] + fields):
        assert m.size == bits.size, (m.size, bits.size)
        cw[m[m >= 0]] = bits[m >= 0]
    return dict(k, name=name, c=c, mc=mc, n_in=n_in, n_sch=n_sch, ph=np.asarray(ph, np.uint16), tb=tb, payloads=payloads, cw=cw, scr=scramble(c, cw, ph), maps=maps)


def layer_symbols(c, scr):
    n = PL.nof_re(c)
    return O.o_modulate(c["mod"], scr).reshape(n, c["nl"]).T.astype(np.complex128)  # layer ly carries symbols ly, L + ly, ...


def transmit_true(c, scr, snr_db=None, rng=None):
    """As pusch_layers_cases.transmit behind the scrambler: -> (grid [4][14][nsc], ce [L][P][1][nsc], the true channel)."""
    rng = rng or np.random.default_rng(c["seed"])
    nl, npt = c["nl"], c["npt"]
    sy, sc = PL.data_positions(c)
    x = layer_symbols(c, scr)
    nsc = c["nprb_grid"] * 12
    h, _ = PL.channels(rng, nl, npt, nsc)
    grid = np.full((4, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    for p in range(npt):
        g = (rng.standard_normal((14, nsc)) + 1j * rng.standard_normal((14, nsc))).astype(np.complex64)
        rx = np.einsum("ln,ln->n", h[:, p, sc].astype(np.complex128), x)
        if snr_db is not None:
            rx = rx + 10 ** (-snr_db / 20) * np.sqrt(0.5) * (rng.standard_normal(sy.size) + 1j * rng.standard_normal(sy.size))
        g[sy, sc] = rx.astype(np.complex64)
        grid[c["rx_ports"][p]] = g
    return grid, np.ascontiguousarray(h.reshape(nl, npt, 1, nsc))


def chain_tx(c, scr, snr_db, delay=2.0):
    """As pusch_layers_estimator_cases.chain_tx behind the scrambler: -> (grid complex64 [4][14][nsc], the estimator case on its first npt ports)."""
    nl, npt = c["nl"], c["npt"]
    rng = np.random.default_rng(c["seed"] + 5000)
    sy, scx = PL.data_positions(c)
    x = layer_symbols(c, scr)
    nsc = c["nprb_grid"] * 12
    hm = PL.channels(np.random.default_rng(c["seed"]), nl, npt, 1)[0][:, :, 0].astype(np.complex128)
    h = hm[:, :, None] * E.profile(nsc, delay)[None, None, :]
    g = np.zeros((npt, 14, nsc), np.complex128)
    for p in range(npt):
        g[p, sy, scx] = np.einsum("ln,ln->n", h[:, p, scx], x)
    rb, dm = PL.masks(c)
    E.add_dmrs(g, h, rb, list(c["dmrs"]), nl, E.SLOT, E.SCR, 0, E.BETA)
    g += 10 ** (-snr_db / 20) * np.sqrt(0.5) * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape))
    grid = np.full((4, 14, nsc), np.nan + 1j * np.nan, np.complex64)
    grid[:npt] = g.astype(np.complex64)
    return grid, (1, E.SLOT, False, E.SCR, 0, np.float32(E.BETA), dm, rb, 0, 14, nl, grid[:npt])


def receive(t, llr):
    """The host chain behind the demodulator: the oracle's demultiplexer, the field decoders, the oracle's transport block decoder.
    -> (fields: list of (payload, valid) or None per field, (crc ok, transport block) or None)."""
    _, _, streams, _ = O.o_ulsch_demultiplex(*t["mc"], llr=llr)
    fields = [decode_field(o, t["mod"], streams[1 + k]) if o else None for k, o in enumerate(t["O"])]
    tb = None
    if t["tb"] is not None:
        ok, out, _ = O.OraclePuschDecoder(1, t["mod"], 0, t["nl"], t["n_sch"] // t["mod"], t["tb"].size).decode(streams[0], 0, True, 6, True)
        tb = (ok, out)
    return fields, tb
