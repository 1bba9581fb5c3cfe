"""CPU: the helper the background-grid tests of the downlink kernels stand on (tests/dl_grid.py). Conditions on its inputs, checked with the
oracle alone: the background has no zero and all the special patterns; the channels of a composed slot own disjoint elements, their order does
not matter, the PDSCH reserved patterns cover the SS/PBCH block and the CSI-RS. With oracle/_ref built, the composed 52-PRB slot is also
produced channel by channel by the reference itself."""
import numpy as np
import pytest

import dl_grid as D
import oracle_lib as O


def test_background_has_no_zero_and_all_special_patterns():
    rng = np.random.default_rng(11)
    for shape in ((3, 14, 360), (2, 40), 13, 5, 3, 7):
        g = D.background(shape, rng)
        u = D.bits(g).reshape(-1, g.shape[-1], 2)
        assert g.dtype == np.complex64 and (u != 0).all() and not (g == 0).any()
        for row in u:
            special = np.isin(row, D.SPECIAL_BITS)
            assert special.sum() == min(8, g.shape[-1]) and special.sum(axis=1).max() == 1
            assert len(set(row[special].tolist())) == special.sum()  # each pattern at most once per row, all eight where the row is long enough
            rest = row[~special].view(np.float32)
            assert ((np.abs(rest) >= 0.5) & (np.abs(rest) < 2.0)).all()
    nan = D.SPECIAL_BITS[2:].view(np.float32)
    assert np.isnan(nan).all() and (D.SPECIAL_BITS[2:] & 0x00400000).all() and len(set(D.SPECIAL_BITS.tolist())) == 8
    assert D.SPECIAL_BITS[:2].view(np.float32).tolist() == [0.0, np.inf] and np.signbit(D.SPECIAL_BITS[:1].view(np.float32))[0]
    f = D.finite_copy(g)
    assert np.isfinite(f.real).all() and np.isfinite(f.imag).all() and ((f == g) | ~np.isfinite(g.real) | ~np.isfinite(g.imag)).all()


def test_written_mask_sees_stores_and_refuses_accumulation():
    rng = np.random.default_rng(12)

    def store(g):
        g[1, 2, 5:9] = 0  # a stored zero is a store
        g[0, 0, 0] = 1 + 2j
    m = D.written_mask(store, (2, 3, 20), rng)
    assert m.sum() == 5 and m[1, 2, 5:9].all() and m[0, 0, 0]

    def accumulate(g):
        g[0, 1, :] += 1
    with pytest.raises(AssertionError):
        D.written_mask(accumulate, (2, 3, 20), rng)


@pytest.fixture(scope="module", params=[52, 275])
def slot(request):
    return D.compose_slot(np.random.default_rng(20 + request.param), request.param, 4)


def test_composed_slot_contents(slot):
    s = slot
    assert s.ssb[0]["k0"] % 12 == 0 and s.ssb[0]["ports"] == [0, 2]
    assert [(p["AL"], p["dur"], p["start"], p["port"]) for p in s.pdcch] == [(4, 1, 0, 0), (2, 2, 0, 1), (8, 3, 1, 0)]
    assert s.csi[0]["row"] == 1 and s.csi[0]["dens"] == 3 and s.csi[1]["cdm"] != 0
    assert all(c["ports"] != list(range(len(c["ports"]))) for c in s.csi)
    assert [(p["mod"], p["bg"], p["rv"], p["port"]) for p in s.pdsch] == [(2, 2, 0, 0), (6, 1, 2, 1), (8, 1, 3, 3)]
    assert s.pdsch[0]["bwp"][0] > 0 and s.pdsch[0]["ref_point_prb0"] == 1 and s.pdsch[1]["start"] == 3
    assert len(s.pdsch[2]["dmrs_symbols"]) == 3 and s.pdsch[2]["cdm"] == 1
    assert all(1 <= len(p["reserved"]) <= 4 for p in s.pdsch)


def test_written_masks_are_pairwise_disjoint_and_cover_what_changed(slot):
    s = slot
    names = list(s.masks)
    assert len(names) == 9
    union = np.zeros(s.shape, bool)
    for n in names:
        assert s.masks[n].any(), n
        assert not (union & s.masks[n]).any(), n
        union |= s.masks[n]
    same = (D.bits(s.expected) == D.bits(s.background)).reshape(s.shape + (2,)).all(axis=-1)
    assert (same | union).all()  # outside the union the expected grid is the background
    assert not same[union].all()
    # PDCCH symbols: only [start, start + duration) of the PDU's port
    for i, p in enumerate(s.pdcch):
        m = s.masks["pdcch%d" % i]
        assert m.sum() == 72 * p["AL"] and m[p["port"], p["start"]:p["start"] + p["dur"]].sum() == m.sum()
    assert s.masks["ssb"].sum() == 2 * (432 + 144 + 2 * 127)


def test_order_of_the_channels_does_not_matter(slot):
    s = slot
    n = len(s.channels)
    rng = np.random.default_rng(31)
    for order in (list(range(n))[::-1], list(rng.permutation(n))):
        g = D.apply_channels(s, s.background.copy(), order)
        assert np.array_equal(D.bits(g), D.bits(s.expected)), order


def test_pdsch_nof_re_three_ways(slot):
    s = slot
    for i, p in enumerate(s.pdsch):
        dm, pl = D.pdsch_alloc(p)
        nre = O.pdsch_nof_re(pl, p["start"], p["nof"], dm, 0, p["cdm"], p["bwp"][0], p["bwp"][1], p["reserved"])
        data = D.written_mask(lambda g: D.o_pdsch_process(p, g, parts=("data",)), s.shape, np.random.default_rng(40 + i))
        assert p["nof_re"] == nre == int(data.sum()) == int(D.pdsch_data_mask(p).sum()) and p["cw"].size == nre * p["mod"]
        assert np.array_equal(data[p["port"]], D.pdsch_data_mask(p)) and data.sum() == data[p["port"]].sum()
        dmrs = D.written_mask(lambda g: D.o_pdsch_process(p, g, parts=("dmrs",)), s.shape, np.random.default_rng(50 + i))
        assert not (dmrs & data).any() and np.array_equal(dmrs | data, s.masks["pdsch%d" % i])
        ref_pt = p["bwp"][0] if p["ref_point_prb0"] else 0
        assert dmrs.sum() == 6 * len(p["dmrs_symbols"]) * int(p["rb"][ref_pt:].sum())


def test_reserved_patterns_cover_block_and_csi_rs(slot):
    """Inside every PDSCH allocation (on any port: a PDU reserves what the other ports carry too) the reserved elements are exactly the
    SS/PBCH block's PRBs and symbols plus the CSI-RS elements of all ports."""
    s = slot
    block = np.zeros(s.shape[1:], bool)
    k0, l0 = s.ssb[0]["k0"], s.ssb[0]["l0"]
    block[l0:l0 + 4, k0:k0 + 240] = True
    assert (s.masks["ssb"].any(axis=0) <= block).all()
    csi = (s.masks["csi0"] | s.masks["csi1"]).any(axis=0)
    hit = 0
    for i, p in enumerate(s.pdsch):
        alloc = np.zeros((14, s.nprb, 12), bool)
        alloc[p["start"]:p["start"] + p["nof"], p["rb"] != 0] = True
        alloc = alloc.reshape(14, -1)
        unreserved = D.pdsch_data_mask(dict(p, reserved=[]))
        reserved = alloc & unreserved & ~D.pdsch_data_mask(p)
        dmrs = alloc & ~unreserved
        assert np.array_equal(reserved, alloc & (block | csi) & ~dmrs), i
        assert not (dmrs & (block | csi)).any(), i  # the DM-RS symbols stay clear of both
        hit += int((reserved & block).any()) + 2 * int((reserved & csi).any())
    assert hit >= 4  # the block and the CSI-RS are really inside some allocation


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")
def test_composed_slot_channel_by_channel_from_the_reference():
    """Every channel of a composed 52-PRB slot produced by the reference on a zero grid equals the oracle composition wherever the channel's
    written mask is set (and is zero elsewhere: the reference maps nothing else)."""
    s = D.compose_slot(np.random.default_rng(61), 52, 4)
    nprb, want = s.nprb, D.bits(s.expected).reshape(s.shape + (2,))

    def check(name, ref_grid):
        m, u = s.masks[name], D.bits(ref_grid).reshape(s.shape + (2,))
        assert np.array_equal(u[m], want[m]), name
        assert not ref_grid[~m].any(), name
    # SS/PBCH block
    p = s.ssb[0]
    r = p["ref"]
    rc, g, l0, k0 = O.r_ssb_process(r["numerology"], p["sfn"], r["slot"], p["N_id"], p["beta"], p["ssb_idx"], p["L_max"], r["scs_khz"], p["k_ssb"], r["offset_to_pointA"],
                                    r["case"], p["payload"], nprb)
    assert rc == 0 and (l0, k0) == (p["l0"], p["k0"])
    full = np.zeros(s.shape, np.complex64)
    for port in p["ports"]:
        full[port] = g
    check("ssb", full)
    # PDCCH: the reference's own CCE-to-PRB mapping gives the PRBs of the descriptor
    for i, p in enumerate(s.pdcch):
        c = p["coreset"]
        g, rb = O.r_pdcch_process(c["mapping"], c["bwp_start"], c["bwp_size"], p["start"], p["dur"], c["fr"], c["reg_bundle"], c["interleaver"], c["shift"], 1, p["slot"],
                                  p["rnti"], p["n_id_dmrs"], p["n_id_data"], p["n_rnti"], c["cce"], p["AL"], p["dmrs_dB"], p["data_dB"], p["payload"], nprb)
        assert np.array_equal(rb, p["rb"]), i
        full = np.zeros(s.shape, np.complex64)
        full[p["port"]] = g
        check("pdcch%d" % i, full)
    # CSI-RS: the pattern of the fixture is what the reference derives from the case, the ports of the job are a relabelling
    for i, p in enumerate(s.csi):
        g, bes, rm, sm = O.r_csi_rs_map(1, p["slot"], p["start_rb"], p["nof_rb"], p["row"], p["k_ref"], p["l0"], 0, p["cdm"], p["dens"], p["scr"], p["amp"], p["nports"], nprb)
        assert tuple(bes) == p["bes"] and np.array_equal(rm[:p["nports"]], p["rm"]) and np.array_equal(sm[:p["nports"]], p["sm"])
        full = np.zeros(s.shape, np.complex64)
        for k, port in enumerate(p["ports"]):
            full[port] = g[k]
        check("csi%d" % i, full)
    # PDSCH: encoder, modulator (contiguous allocation in the BWP) and DM-RS processor
    for i, p in enumerate(s.pdsch):
        dm, pl = D.pdsch_alloc(p)
        bs, bz = p["bwp"]
        vrb = p["rb"][bs:bs + bz]
        assert vrb.sum() == p["rb"].sum() and np.array_equal(O.r_prb_indices(bs, bz, vrb, 0), pl)
        cw = O.r_pdsch_encode(p["bg"], p["rv"], p["mod"], p["lbrm_bytes"] * 8, 1, p["nof_re"], p["tb"])
        assert np.array_equal(cw, p["cw"])
        g, _ = O.r_pdsch_modulate(p["rnti"], p["n_id"], D.db_to_amplitude(-p["data_dB"]), 1, [p["mod"]], [cw], p["start"], p["nof"], dm, 0, p["cdm"], bs, bz, vrb, 0,
                                  p["reserved"], [p["port"]], nprb, s.nports)
        d = O.r_dmrs_pdsch_map(1, p["slot"], bs if p["ref_point_prb0"] else 0, 0, p["scr"], p["n_scid"], D.db_to_amplitude(-p["dmrs_dB"]), dm, p["rb"], [p["port"]], s.nports)
        assert not (g != 0)[d != 0].any()
        check("pdsch%d" % i, np.where(d != 0, d, g))
