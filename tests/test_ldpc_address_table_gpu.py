"""GPU: the packed LDPC decoder instance that reads its soft-bit addresses from a table (csrc/ldpc_pk_device.h, pk_table_addresses;
high-rate BG1 codeblocks that are dematched while they load) against the CPU oracle chain, next to the same plan with the table switched
off (miphy_debug_force_ldpc_kernel | 0x200, every launch computes its addresses). Both runs must give the oracle's hard bits, codeblock
CRC flags, iteration counts and transport blocks, and leave the oracle's HARQ soft images.

Shapes: one codeblock per wavefront count of the instance (Z = 384, 256, 128: three, two, one), four layers reached, and one shape of the
six-layer bucket, which keeps computing its addresses. Three codeblocks per batch, received at three noise levels: one passes its CRC after
two iterations, one after about four, one never. Iteration limits 1, 2 and 6, CRC early stop on and off. Then a batch larger than the
resident grid (a persistent workgroup takes a second codeblock: the table request in front of its load phase), an all-zero codeblock
inside a batch (the codeblock is left before its first layer), and a batch that mixes a table class with one that computes."""
import functools

import numpy as np
import pytest

from oracle_lib import OraclePuschDecoder, o_pdsch_encode, o_segmentation

pytestmark = pytest.mark.gpu

THROUGHPUT, NO_TABLE = 4, 0x200  # miphy_debug_force_ldpc_kernel: class-sorted launches in the geometry of a full chip; flag: no address table
BG, MOD = 1, 8
# name: TB bits, channel symbols, lifting size, codeblocks, layers reached, takes the table
SHAPES = {
    "z384": (25224, 3420, 384, 3, 4, True),
    "z256": (5608, 768, 256, 1, 4, True),
    "z128": (2800, 384, 128, 1, 4, True),
    "z352": (15416, 2112, 352, 2, 4, True),
    "z384_six_layers": (25248, 3744, 384, 3, 6, False),
}
SIGMAS = {4: (0.30, 0.40, 0.47), 6: (0.35, 0.45, 0.60)}  # per bucket (code rate 0.92 / 0.85): two, about four, more than six iterations


def layers_reached(seg, c):
    """Layers the decoder sizes a first transmission by: the E rate-matched bits and the fillers, in whole columns, at least four."""
    cols = -(-(seg.E[c] + seg.nof_filler_bits) // seg.Z)
    return max(4, min(max(cols, 24), seg.N // seg.Z) + 2 - 22)


@functools.lru_cache(maxsize=None)
def transport_block(shape, sigmas, seed, zero_cb=-1):
    """(TB bytes, LLRs): codeblock c of the codeword received with noise sigmas[c % len]; codeblock zero_cb not received at all."""
    tbs_bits, nsym, Z, ncb, lay, _ = SHAPES[shape]
    seg = o_segmentation(tbs_bits, BG, MOD, 1, nsym)
    assert (seg.Z, seg.nof_cbs) == (Z, ncb) and all(layers_reached(seg, c) == lay for c in range(ncb)), shape
    rng = np.random.default_rng(seed)
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
    cw = o_pdsch_encode(BG, 0, MOD, 0, 1, nsym, tb)
    sig = np.concatenate([np.full(seg.E[c], sigmas[c % len(sigmas)]) for c in range(ncb)])
    llr = np.round(np.clip(4 * ((1.0 - 2.0 * (cw & 1)) + sig * rng.standard_normal(cw.size)), -20, 20) / 20 * 120).astype(np.int8)
    if zero_cb >= 0:
        llr[seg.cw_offset[zero_cb]:seg.cw_offset[zero_cb] + seg.E[zero_cb]] = 0
    tb.setflags(write=False)
    llr.setflags(write=False)
    return tb, llr


@functools.lru_cache(maxsize=None)
def oracle_of(shape, sigmas, seed, zero_cb, max_iter, early_stop):
    tbs_bits, nsym = SHAPES[shape][:2]
    od = OraclePuschDecoder(BG, MOD, 0, 1, nsym, tbs_bits // 8)
    od.softbuf[:] = 33
    ok, tbo, mm = od.decode(transport_block(shape, sigmas, seed, zero_cb)[1], 0, True, max_iter, early_stop)
    return ok, tbo, mm, od.cb_crc.copy(), od.cb_msgs.reshape(od.seg.nof_cbs, -1).copy(), od.softbuf.reshape(od.seg.nof_cbs, -1).copy()


def run_plan(ctx, tbs, max_iter, early_stop, mode):
    """tbs: [(shape, sigmas, seed, zero_cb)] -> per TB (result record, TB bytes, CRC flags, hard bits, soft images) and the number of
    decoder launches that read the table."""
    import torch
    import miphy
    lib = miphy.lib()
    d = np.zeros(len(tbs), dtype=miphy.PuschTbDesc)
    llrs, slot, llr_off, tb_off, where = [], 0, 0, 0, []
    for i, t in enumerate(tbs):
        tbs_bits, nsym, Z, ncb = SHAPES[t[0]][:4]
        llr = transport_block(*t)[1]
        d[i] = (BG, 0, MOD, 1, 1, int(early_stop), max_iter, 0, nsym, tbs_bits // 8, slot, llr_off, tb_off)
        where.append((slot, ncb, tb_off, tbs_bits // 8, 66 * Z, (22 * Z + 7) // 8))
        llrs.append(llr)
        slot, llr_off, tb_off = slot + ncb, llr_off + llr.size, tb_off + tbs_bits // 8
    soft_d = torch.full((slot * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(slot, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(len(tbs) * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    tb_d = torch.full((tb_off,), 0xEE, dtype=torch.uint8, device="cuda")
    lib.miphy_debug_force_ldpc_kernel(mode)
    plan = None
    try:
        plan = ctx.pusch_decode_plan(d)
        lib.miphy_debug_ldpc_address_table_launches(1)
        plan.run(torch.from_numpy(np.concatenate(llrs)).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        table_launches = int(lib.miphy_debug_ldpc_address_table_launches(1))
    finally:
        lib.miphy_debug_force_ldpc_kernel(0)
        if plan is not None:
            plan.close()
    res, tb_out, crc = res_d.cpu().numpy().view(miphy.PuschResult), tb_d.cpu().numpy(), crc_d.cpu().numpy()
    soft, msgs = soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE), msgs_d.cpu().numpy().reshape(slot, miphy.HARQ_MSG_STRIDE)
    out = [(res[i], tb_out[o:o + nb], crc[s:s + n], msgs[s:s + n, :kb], soft[s:s + n, :N]) for i, (s, n, o, nb, N, kb) in enumerate(where)]
    return out, table_launches


def check_against_oracle(tbs, got, max_iter, early_stop, what):
    for i, (t, (res, tb_out, crc, msgs, soft)) in enumerate(zip(tbs, got)):
        ok, tbo, mm, e_crc, e_msgs, e_soft = oracle_of(*t, max_iter, early_stop)
        key = (what, i, t[0], ok, mm)
        assert bool(res["tb_crc_ok"]) == ok and res["nof_codeblocks_total"] == len(e_crc), (key, res)
        assert (int(res["iters_min"]), int(res["iters_max"])) == mm, (key, res)
        assert np.array_equal(crc, e_crc), (key, crc, e_crc)
        assert np.array_equal(msgs, e_msgs), (key, int(np.sum(msgs != e_msgs)))
        assert np.array_equal(soft, e_soft), key
        if ok:
            assert np.array_equal(tb_out, tbo) and np.array_equal(tb_out, transport_block(*t)[0]), key


def check_both(ctx, tbs, max_iter, early_stop, base_mode, expect_table_launches):
    on, n_on = run_plan(ctx, tbs, max_iter, early_stop, base_mode)
    off, n_off = run_plan(ctx, tbs, max_iter, early_stop, base_mode | NO_TABLE)
    assert (n_on, n_off) == (expect_table_launches, 0), (n_on, n_off)
    check_against_oracle(tbs, on, max_iter, early_stop, "table")
    check_against_oracle(tbs, off, max_iter, early_stop, "computed")
    for a, b in zip(on, off):  # (what the oracle comparison covers, said directly: the two runs leave the same bytes)
        assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    return on


def batch_of_three(shape):
    """Three codeblocks at the three noise levels of the shape's bucket: one transport block of three, or three of one."""
    ncb, lay = SHAPES[shape][3], SHAPES[shape][4]
    if ncb == 3:
        return ((shape, SIGMAS[lay], 100, -1),)
    return tuple((shape, (s,), 200 + k, -1) for k, s in enumerate(SIGMAS[lay]))


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("max_iter", [1, 2, 6])
@pytest.mark.parametrize("shape", ["z384", "z256", "z128", "z384_six_layers"])
def test_three_codeblocks(ctx, shape, max_iter, early_stop):
    tbs = batch_of_three(shape)
    got = check_both(ctx, tbs, max_iter, early_stop, THROUGHPUT, 1 if SHAPES[shape][5] else 0)
    if max_iter == 6 and early_stop:  # the inputs are what the docstring says: codeblocks that pass early, late and never
        flags = np.concatenate([g[2] for g in got])
        its = [int(g[0][k]) for g in got for k in ("iters_min", "iters_max")]
        assert flags.tolist() == [1, 1, 0] and min(its) == 2 and max(its) == 6, (flags, its)


def test_batch_larger_than_the_resident_grid(ctx):
    """434 transport blocks of three codeblocks of Z = 384 (1302 codeblocks; 256 CUs hold 1024): the automatic choice is the throughput
    form, and every persistent workgroup that takes a second codeblock requests its first table rows in front of the load phase."""
    kinds = [("z384", (0.30, 0.40, 0.47), 300, -1), ("z384", (0.40, 0.30, 0.35), 301, -1), ("z384", (0.47, 0.35, 0.40), 302, -1), ("z384", (0.25, 0.47, 0.30), 303, -1)]
    tbs = tuple(kinds[(7 * i) % 4] for i in range(434))
    check_both(ctx, tbs, 6, True, 0, 1)


def test_all_zero_codeblock_inside_a_batch(ctx):
    """Nothing received of the middle codeblock of the middle transport block: the decoder leaves it before its first layer, with the
    table rows of layer 1 requested and never used, and goes on with the next codeblock."""
    tbs = (("z384", (0.30, 0.40, 0.35), 400, -1), ("z384", (0.30, 0.40, 0.35), 401, 1), ("z384", (0.35, 0.30, 0.40), 402, -1))
    got = check_both(ctx, tbs, 6, True, THROUGHPUT, 1)
    assert got[1][2].tolist() == [1, 0, 1] and not got[1][0]["tb_crc_ok"] and got[0][0]["tb_crc_ok"] and got[2][0]["tb_crc_ok"]


def test_table_class_next_to_a_class_that_computes(ctx):
    """Two launch classes in one plan: four layers at two lifting sizes of one workgroup size (one launch, a table per lifting size) and
    the six-layer bucket (computed addresses)."""
    tbs = (("z384", SIGMAS[4], 500, -1), ("z384_six_layers", SIGMAS[6], 501, -1), ("z352", (0.40, 0.30), 502, -1), ("z384", (0.40, 0.47, 0.30), 503, -1))
    check_both(ctx, tbs, 6, True, THROUGHPUT, 1)
