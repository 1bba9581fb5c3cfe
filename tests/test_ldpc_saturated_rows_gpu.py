"""GPU: the packed LDPC decoder with and without its skip of saturated rows (csrc/ldpc_decode_pk.hip: a wavefront leaves out its visits of
a layer once every soft bit its rows read there is infinite; miphy_debug_force_ldpc_kernel | 0x400 switches that off) against the CPU
oracle chain. Every case runs four ways -- skip on / off, soft-bit addresses from the table / computed (| 0x200) -- in the class-sorted
throughput geometry (mode 4), and all four must give the oracle's hard bits, codeblock CRC flags, iteration counts / result records and
transport blocks, and leave the oracle's HARQ soft images. A case that is there for the skip asserts with the oracle's soft bits
(tests/test_ldpc_saturated_rows.py, sticky_skips) that visits ARE left out, and where it says so that every reached soft bit is +-127 two
iterations before the end.

Shapes and LLR formula: tests/test_ldpc_address_table_gpu.py, received at sigma 0.10 (LLRs around +-24: a clean codeblock saturates
within four to five iterations, its layers and wavefronts one after another, so that visits that run and visits that are left out
follow each other both ways round). z384_six_layers and the low rate never saturate completely: some (wavefront, layer) pairs die,
others live to the end."""
import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import o_ldpc_decode, o_ldpc_encode
from ldpc_saturation_model import dead_below_live, infinite
from test_ldpc_saturated_rows import BG, MOD, SHAPES, SIGMA, STUCK, oracle_of, saturation, soft_after, sticky_skips, transport_block

pytestmark = pytest.mark.gpu

THROUGHPUT, NO_TABLE, NO_SKIP = 4, 0x200, 0x400
WAYS = [THROUGHPUT, THROUGHPUT | NO_SKIP, THROUGHPUT | NO_TABLE, THROUGHPUT | NO_TABLE | NO_SKIP]
KERNEL_GMSG, KERNEL_SPLIT = 8, 32
ROWSKIP = 1 << 16  # (this file's own bit: a launch took the instance that leaves visits out, miphy_debug_ldpc_row_skip_launches)


def run_plan(ctx, tbs, max_iter, early_stop, mode):
    """tbs: [(shape, sigma, seed, flip_cb)] -> per TB (result record, TB bytes, CRC flags, hard bits, soft images), table launches, kernels used."""
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
        lib.miphy_debug_ldpc_kernels_used(1)
        lib.miphy_debug_ldpc_row_skip_launches(1)
        plan.run(torch.from_numpy(np.concatenate(llrs)).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        table_launches, used = int(lib.miphy_debug_ldpc_address_table_launches(1)), int(lib.miphy_debug_ldpc_kernels_used(1))
        used |= ROWSKIP if lib.miphy_debug_ldpc_row_skip_launches(1) else 0
    finally:
        lib.miphy_debug_force_ldpc_kernel(0)
        if plan is not None:
            plan.close()
    res, tb_out, crc = res_d.cpu().numpy().view(miphy.PuschResult), tb_d.cpu().numpy(), crc_d.cpu().numpy()
    soft, msgs = soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE), msgs_d.cpu().numpy().reshape(slot, miphy.HARQ_MSG_STRIDE)
    out = [(res[i], tb_out[o:o + nb], crc[s:s + n], msgs[s:s + n, :kb], soft[s:s + n, :N]) for i, (s, n, o, nb, N, kb) in enumerate(where)]
    return out, table_launches, used


def check_against_oracle(tbs, got, max_iter, early_stop, what):
    for i, (t, (res, tb_out, crc, msgs, soft)) in enumerate(zip(tbs, got)):
        ok, tbo, mm, e_crc, e_msgs, e_soft = oracle_of(*t, max_iter, early_stop)
        key = (what, i, t, ok, mm)
        assert bool(res["tb_crc_ok"]) == ok and res["nof_codeblocks_total"] == len(e_crc), (key, res)
        assert (int(res["iters_min"]), int(res["iters_max"])) == mm, (key, res)
        assert np.array_equal(crc, e_crc), (key, crc, e_crc)
        assert np.array_equal(msgs, e_msgs), (key, int(np.sum(msgs != e_msgs)))
        assert np.array_equal(soft, e_soft), key
        if ok:
            assert np.array_equal(tb_out, tbo) and np.array_equal(tb_out, transport_block(*t)[0]), key


def check_four_ways(ctx, tbs, max_iter, early_stop, table, gmsg=False):
    """-> the kernels the run with the skip used. table: the plan has a launch that reads its addresses from the table (unless switched off).
    The launch planner takes the instance that leaves visits out only where codeblocks run all their iterations with their messages in LDS;
    with 0x400, with the early stop or with messages in global memory the launch runs the instance without it."""
    first, used0 = None, 0
    for mode in WAYS:
        got, n_table, used = run_plan(ctx, tbs, max_iter, early_stop, mode)
        assert n_table == (1 if table and not (mode & NO_TABLE) else 0), (mode, n_table)
        assert bool(used & KERNEL_GMSG) == gmsg, (hex(mode), used)
        assert bool(used & ROWSKIP) == (not (mode & NO_SKIP) and not early_stop and not gmsg), (hex(mode), used)
        check_against_oracle(tbs, got, max_iter, early_stop, hex(mode))
        if first is None:
            first, used0 = got, used
        for a, b in zip(first, got):  # (what the oracle comparison covers, said directly: the runs leave the same bytes)
            assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), hex(mode)
    return first, used0


def all_reached_saturated(t, k):
    """Per codeblock: every soft bit of the reached columns is +-127 after k iterations (the oracle's)."""
    Z, lay = SHAPES[t[0]][2], SHAPES[t[0]][4]
    return [bool((np.abs(soft[:(22 + lay) * Z].astype(np.int32)) == 127).all()) for _, soft in soft_after(*t, k)]


@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("max_iter", [6, 8])
@pytest.mark.parametrize("shape", ["z384", "z352", "z128", "z256", "z384_six_layers"])
def test_clean_saturation(ctx, shape, max_iter, early_stop):
    """(z384 with six iterations saturates after five: at most one visit per pair is left out there, none for most -- the case is the skip
    arriving in the last iteration, not a precondition met.)"""
    t = (shape, SIGMA, 100, -1)
    skips = sticky_skips(*t, max_iter)
    if shape == "z384_six_layers":  # the mixed case: in every codeblock pairs that die and pairs that live to the end
        assert all(min(p.values()) == 0 and max(p.values()) > 0 for p in skips), skips
        assert not any(all_reached_saturated(t, max_iter - 2))
    else:  # every (wavefront, layer) pair of every codeblock leaves visits out -- not all from the same iteration on
        assert all(min(p.values()) > 0 for p in skips) or (shape, max_iter) == ("z384", 6), skips
        assert all(max(p.values()) > min(p.values()) for p in skips), skips
        # (Z = 384 saturates after five iterations: with six, its last soft bits are still finite two iterations before the end)
        assert all_reached_saturated(t, max_iter - 2) == [(shape, max_iter) != ("z384", 6)] * SHAPES[shape][3]
    # (six layers: the throughput geometry moves the messages to global memory, and the planner keeps such a launch on the instance that runs every visit)
    got, _ = check_four_ways(ctx, (t,), max_iter, early_stop, shape != "z384_six_layers", gmsg=shape == "z384_six_layers")
    assert got[0][0]["tb_crc_ok"] and got[0][2].all()
    if not early_stop:  # (with the early stop the codeblocks leave after their second iteration: nothing is left out, nothing may differ)
        assert (int(got[0][0]["iters_min"]), int(got[0][0]["iters_max"])) == (max_iter, max_iter)


@pytest.mark.parametrize("early_stop", [False, True])
def test_live_throughout_next_to_clean_codeblocks(ctx, early_stop):
    """60 LLRs of the middle codeblock are +-120 with the wrong sign: it never saturates and fails its CRC; its neighbours saturate."""
    t = ("z384", SIGMA, 100, 1)
    skips = sticky_skips(*t, 8)
    assert max(skips[1].values()) == 0 and min(skips[0].values()) > 0 and min(skips[2].values()) > 0, skips
    assert all_reached_saturated(t, 6) == [True, False, True]
    got, _ = check_four_ways(ctx, (t,), 8, early_stop, True)
    assert got[0][2].tolist() == [1, 0, 1] and not got[0][0]["tb_crc_ok"]


def test_batch_larger_than_the_resident_grid(ctx):
    """434 transport blocks of three codeblocks of Z = 384 (1302 codeblocks; 256 CUs hold 1024): every persistent workgroup that takes a
    second codeblock starts it with a cleared mask -- saturating codeblocks and the live one of every other transport block follow each
    other on the same workgroups."""
    kinds = [("z384", SIGMA, 300, -1), ("z384", SIGMA, 301, 1)]
    for t, live in zip(kinds, (-1, 1)):
        skips = sticky_skips(*t, 8)
        assert all((max(p.values()) == 0) == (c == live) for c, p in enumerate(skips)), skips
    tbs = tuple(kinds[i % 2] for i in range(434))
    got, _ = check_four_ways(ctx, tbs, 8, False, True)
    assert [bool(g[0]["tb_crc_ok"]) for g in got] == [i % 2 == 0 for i in range(434)]


def test_messages_in_global_memory(ctx):
    """Rate 1/3 at Z = 384 reaches all 46 layers: the throughput geometry keeps its messages in global memory, and the planner keeps such a
    launch on the instance that runs every visit (the parity columns with one check each stay finite: few rows saturate)."""
    t = ("z384_rate_one_third", SIGMA, 100, -1)
    skips = sticky_skips(*t, 6)
    assert min(skips[0].values()) == 0 and max(skips[0].values()) > 0
    for early_stop in (False, True):
        got, used = check_four_ways(ctx, (t,), 6, early_stop, False, gmsg=True)
        assert used & KERNEL_GMSG, used
        assert got[0][0]["tb_crc_ok"]


@pytest.mark.parametrize("Z", [384, 128])
def test_saturation_onto_a_wrong_word(ctx, Z):
    """A codeword of a message WITHOUT a valid CRC, received at +-120 through the codeblock-level entry point: every row goes dead, the
    checksum fails in every iteration, the iteration count is 0 and the hard bits are the oracle's (the message that was sent)."""
    import torch
    import miphy
    from miphy.ldpc import make_dec_descs
    lib = miphy.lib()
    rng = np.random.default_rng(7)
    K, in_len, n, max_iter = 22 * Z, 24 * Z, 3, 6
    copies = 100  # 300 codeblocks: more than one per CU, so the automatic geometry is the throughput form, and few enough that their messages stay in LDS
    llrs, exp = [], []
    for _ in range(n):
        msg = rng.integers(0, 2, K, dtype=np.uint8)
        assert O.o_crc_bits(O.CRC24B, msg) != 0
        llr = (120 * (1 - 2 * o_ldpc_encode(BG, Z, msg, 66 * Z)[:in_len].astype(np.int32))).astype(np.int8)
        it, hard, soft = o_ldpc_decode(BG, Z, llr, 0, -1, max_iter - 2, want_soft=True)
        assert infinite(soft[:26 * Z]).all() and (np.abs(soft[:26 * Z].astype(np.int32)) == 127).all()  # the rows are dead two iterations before the end
        e_it, e_hard = o_ldpc_decode(BG, Z, llr, 0, O.CRC24B, max_iter)
        assert e_it == 0 and np.array_equal(np.unpackbits(e_hard)[:K], msg)
        llrs.append(llr)
        exp.append(e_hard)
    llr_d = torch.from_numpy(np.concatenate(llrs * copies)).cuda()
    n, exp = n * copies, exp * copies
    for mode in (3, 3 | NO_SKIP):  # class-sorted launches, geometry by the size of the batch (the plain kernel has no address table)
        out_d = torch.full((n * K // 8,), 0xEE, dtype=torch.uint8, device="cuda")
        it_d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        lib.miphy_debug_force_ldpc_kernel(mode)
        try:
            descs = make_dec_descs(n, BG, Z, in_len, miphy.CRC24B, max_iter)
            descs["flags"] = 1  # the CRC behind the last iteration only: the codeblocks run all iterations, the launch may leave visits out
            lib.miphy_debug_ldpc_kernels_used(1)
            lib.miphy_debug_ldpc_row_skip_launches(1)
            ctx.ldpc_decode_batch(descs, llr_d, out_d, it_d)
            torch.cuda.synchronize()
        finally:
            lib.miphy_debug_force_ldpc_kernel(0)
        assert not lib.miphy_debug_ldpc_kernels_used(1) & (KERNEL_GMSG | KERNEL_SPLIT), hex(mode)
        assert bool(lib.miphy_debug_ldpc_row_skip_launches(1)) == (not (mode & NO_SKIP)), hex(mode)
        assert it_d.cpu().tolist() == [0] * n, (hex(mode), it_d.cpu().tolist())
        assert np.array_equal(out_d.cpu().numpy().reshape(n, -1), np.stack(exp)), hex(mode)


def test_address_requests_across_set_bits(ctx):
    """The table instance with dead layers between live ones, both ways round (STUCK, tests/test_ldpc_saturated_rows.py): wavefront 0 runs
    layers 0, 2, 3 and leaves out layer 1 between them (the request of layer 0 names layer 2), wavefront 2 runs layer 3 alone (its request
    wraps over layers 0, 1, 2). The stuck bits are held on the right side by the rows that stay alive; the codeblock decodes. Next to it a
    second transport block of the same kind received clean."""
    t = ("z384", None, 100, STUCK)
    sat = saturation(*t, 8)[0]
    assert {(0, 1, 2), (2, 0, 3), (2, 2, 3)} <= {(w, dead, live) for _, w, dead, live in dead_below_live(sat, 8)}
    got, _ = check_four_ways(ctx, (t, ("z384", SIGMA, 100, -1)), 8, False, True)
    assert got[0][0]["tb_crc_ok"] and got[1][0]["tb_crc_ok"]
