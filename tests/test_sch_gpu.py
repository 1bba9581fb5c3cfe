"""GPU parity for the transport-block level entry points (pusch_decoder::decode with HARQ, pdsch_encoder::encode) vs the
CPU oracle: TB bytes, CRC verdicts and LDPC iteration statistics must be identical."""
import numpy as np
import pytest

from oracle_lib import OraclePuschDecoder, o_pdsch_encode, o_segmentation

pytestmark = pytest.mark.gpu


def noisy(cw, sigma, rng):
    y = (1.0 - 2.0 * (cw & 1)) + sigma * rng.standard_normal(cw.size)
    return np.round(np.clip(4 * y, -20, 20) / 20 * 120).astype(np.int8)


CASES = [  # bg, mod, nof_layers, nprb, tbs bits, sigmas
    (2, 2, 1, 106, 3848, (0.75, 1.3)),
    (1, 4, 1, 106, 42016, (0.45, 0.62)),
    (1, 6, 1, 106, 83976, (0.3, 0.62)),
    (1, 8, 1, 273, 319784, (0.3, 0.45)),
    (2, 2, 1, 273, 9984, (0.75, 1.3)),
    (1, 4, 2, 50, 40976, (0.45, 0.62)),
    (2, 2, 1, 4, 320, (0.5, 1.0)),
    (2, 2, 1, 2, 24, (0.5, 1.1)),
]


def test_pdsch_encode_batch(ctx):
    import torch
    import miphy
    rng = np.random.default_rng(51)
    tbs, descs, cw_off, tb_off, tb_list = [], [], 0, 0, []
    for bg, mod, nl, nprb, tbs_bits, _ in CASES:
        nsym = nprb * 156 * nl
        for rv, Nref in ((0, 0), (2, 0), (3, 20000 if bg == 1 else 0)):
            tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
            descs.append((bg, rv, mod, nl, Nref, nsym, tb.size, tb_off, cw_off))
            tb_list.append(tb)
            tb_off += (tb.size + 15) // 16 * 16
            cw_off += nsym * mod
    d = np.zeros(len(descs), dtype=miphy.PdschTbDesc)
    tb_all = np.zeros(tb_off + 16, dtype=np.uint8)
    for i, x in enumerate(descs):
        d[i] = x
        tb_all[x[7]:x[7] + tb_list[i].size] = tb_list[i]
    cw_d = torch.full((cw_off,), 9, dtype=torch.uint8, device="cuda")
    ctx.pdsch_encode_batch(d, torch.from_numpy(tb_all).cuda(), cw_d)
    torch.cuda.synchronize()
    cw = cw_d.cpu().numpy()
    for i, (bg, rv, mod, nl, Nref, nsym, nb, to, co) in enumerate(descs):
        exp = o_pdsch_encode(bg, rv, mod, Nref, nl, nsym, tb_list[i])
        assert np.array_equal(cw[co:co + nsym * mod], exp), descs[i]


def test_pdsch_encode_packed_kernel_lifting_sizes(ctx):
    """The bit-packed codeblock kernel (one wavefront per codeblock, lifting sizes that are multiples of 32) against the oracle for
    every such lifting size of both base graphs, every PDSCH modulation, all redundancy versions, limited buffers, repetition
    (E beyond the circular buffer: the selected bits wrap) and puncturing; a codeword too long for its LDS buffer (E > 65536) must
    take the one-lane-per-bit kernel, as must every other lifting size. The test asserts which kernel encoded how many codeblocks."""
    import ctypes as C
    import torch
    import miphy
    rng = np.random.default_rng(77)
    want = {(bg, Z) for bg in (1, 2) for Z in range(32, 385, 32)}
    found = {}
    for bg in (1, 2):  # transport-block sizes (bytes) that segment into each lifting size
        for nbytes in list(range(8, 1100, 2)) + list(range(1100, 12000, 40)):
            seg = o_segmentation(nbytes * 8, bg, 2, 1, 10000)
            key = (bg, seg.Z)
            if key in want and key not in found:
                found[key] = nbytes
    assert set(found) == want, sorted(want - set(found))
    descs, tb_list, cw_off, tb_off, npk, ncb = [], [], 0, 0, 0, 0
    sizes = sorted(found.items())
    # several codeblocks per transport block: TS 38.214 sizes (byte-aligned codeblock payloads: packed kernel) and sizes the standard cannot
    # produce (payloads that are not whole bytes: those codeblocks must go to the one-lane-per-bit kernel)
    for bg, nbytes in ((1, 42016 // 8), (1, 83976 // 8), (2, 9984 // 8), (1, 5000), (2, 1500)):
        seg = o_segmentation(nbytes * 8, bg, 2, 1, 10000)
        assert seg.nof_cbs > 1 and seg.Z % 32 == 0, (bg, nbytes, seg.nof_cbs, seg.Z)
        sizes.append(((bg, seg.Z), nbytes))

    def packed(seg, e_bits):  # miphy_pdsch_cb_packed_ok for every codeblock of a transport block
        last = seg.cb_info_bits - seg.nof_tb_crc_bits - seg.zero_pad
        return (seg.Z % 32 == 0 and seg.cb_info_bits % 8 == 0 and last % 8 == 0 and seg.zero_pad % 8 == 0 and e_bits <= 65536)
    for (bg, Z), nbytes in sizes:
        seg = o_segmentation(nbytes * 8, bg, 2, 1, 10000)
        N = seg.N * seg.nof_cbs
        for mod, rv, Nref, ratio in ((2, 0, 0, 0.5), (4, 1, 0, 0.9), (6, 2, 0, 1.7), (8, 3, (seg.N * 2) // 3, 0.4), (8, 0, 0, 2.6), (4, 3, 0, 1.0)):
            nsym = max(seg.nof_cbs, int(N * ratio / mod)) // seg.nof_cbs * seg.nof_cbs  # every codeblock the same number of symbols
            tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
            descs.append((bg, rv, mod, 1, Nref, nsym, tb.size, tb_off, cw_off))
            tb_list.append(tb)
            tb_off += (tb.size + 15) // 16 * 16
            cw_off += nsym * mod
            ncb += seg.nof_cbs
            npk += seg.nof_cbs if packed(seg, nsym * mod // seg.nof_cbs) else 0
    # one codeblock repeated beyond the packed kernel's buffer, and lifting sizes it does not take
    for bg, nbytes, mod, nsym in ((1, found[(1, 128)], 8, 9000), (2, 40, 2, 300), (1, 100, 4, 400)):
        seg = o_segmentation(nbytes * 8, bg, mod, 1, nsym)
        assert seg.Z % 32 != 0 or nsym * mod // seg.nof_cbs > 65536
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        descs.append((bg, 0, mod, 1, 0, nsym, tb.size, tb_off, cw_off))
        tb_list.append(tb)
        tb_off += (tb.size + 15) // 16 * 16
        cw_off += nsym * mod
        ncb += seg.nof_cbs
    d = np.zeros(len(descs), dtype=miphy.PdschTbDesc)
    tb_all = np.zeros(tb_off + 16, dtype=np.uint8)
    for i, x in enumerate(descs):
        d[i] = x
        tb_all[x[7]:x[7] + tb_list[i].size] = tb_list[i]
    cw_d = torch.full((cw_off,), 9, dtype=torch.uint8, device="cuda")
    cnt = (C.c_uint * 2)()
    miphy.lib().miphy_debug_pdsch_cb_counts(cnt, 1)
    ctx.pdsch_encode_batch(d, torch.from_numpy(tb_all).cuda(), cw_d)
    torch.cuda.synchronize()
    miphy.lib().miphy_debug_pdsch_cb_counts(cnt, 1)
    assert (cnt[0], cnt[1]) == (npk, ncb), (cnt[0], cnt[1], npk, ncb)
    cw = cw_d.cpu().numpy()
    for i, (bg, rv, mod, nl, Nref, nsym, nb, to, co) in enumerate(descs):
        exp = o_pdsch_encode(bg, rv, mod, Nref, nl, nsym, tb_list[i])
        assert np.array_equal(cw[co:co + nsym * mod], exp), descs[i]


@pytest.mark.parametrize("early_stop,max_iter", [(1, 6), (0, 2), (1, 2)])
def test_pusch_decode_batch_with_harq(ctx, early_stop, max_iter):
    import torch
    import miphy
    rng = np.random.default_rng(52 + max_iter + early_stop)
    rvs = [0, 2, 3, 1]
    tbs = []
    slot = 0
    for bg, mod, nl, nprb, tbs_bits, sigmas in CASES:
        for sigma in sigmas:
            nsym = nprb * 156 * nl
            tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
            seg = o_segmentation(tbs_bits, bg, mod, nl, nsym)
            llrs = [noisy(o_pdsch_encode(bg, rv, mod, 0, nl, nsym, tb), sigma, rng) for rv in rvs]
            od = OraclePuschDecoder(bg, mod, 0, nl, nsym, tbs_bits // 8)
            od.softbuf[:] = 33  # the same stale garbage as the device buffers
            tbs.append(dict(bg=bg, mod=mod, nl=nl, nsym=nsym, tb=tb, llrs=llrs, slot=slot, ncb=seg.nof_cbs, od=od))
            slot += seg.nof_cbs
    n = len(tbs)
    soft_d = torch.full((slot * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")  # stale garbage, new_data must cope
    msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(slot, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    for t, rv in enumerate(rvs):
        d = np.zeros(n, dtype=miphy.PuschTbDesc)
        llr_off, tb_off, chunks = 0, 0, []
        for i, x in enumerate(tbs):
            d[i] = (x["bg"], rv, x["mod"], x["nl"], 1 if t == 0 else 0, early_stop, max_iter, 0, x["nsym"], x["tb"].size, x["slot"], llr_off, tb_off)
            chunks.append(x["llrs"][t])
            llr_off += x["llrs"][t].size
            tb_off += x["tb"].size
        tb_d = torch.full((tb_off,), 0xEE, dtype=torch.uint8, device="cuda")
        ctx.pusch_decode_batch(d, torch.from_numpy(np.concatenate(chunks)).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        res = res_d.cpu().numpy().view(miphy.PuschResult)
        tb_out = tb_d.cpu().numpy()
        soft = soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE)
        for i, x in enumerate(tbs):
            ok, tbo, mm = x["od"].decode(x["llrs"][t], rv, t == 0, max_iter, bool(early_stop))
            r = res[i]
            key = (i, t, x["bg"], x["mod"], x["tb"].size * 8)
            assert bool(r["tb_crc_ok"]) == ok, key
            assert r["nof_codeblocks_total"] == x["ncb"], key
            assert (int(r["iters_min"]), int(r["iters_max"])) == mm, (key, r, mm)
            o0 = int(d[i]["tb_offset"])
            got = tb_out[o0:o0 + x["tb"].size]
            if ok:
                assert np.array_equal(got, tbo) and np.array_equal(got, x["tb"]), key
            elif not np.all(x["od"].cb_crc):
                assert np.all(got == 0xEE), key  # untouched unless every codeblock passed
            # the HARQ soft buffers hold what the reference's dematcher leaves there, whichever launch class dematched the codeblock
            # (inside the packed decoder for first transmissions with Z >= 128, the dematcher kernel for the rest)
            N = x["od"].softbuf.size // x["ncb"]
            exp_soft = x["od"].softbuf.reshape(x["ncb"], N)
            for c in range(x["ncb"]):
                assert np.array_equal(soft[x["slot"] + c, :N], exp_soft[c]), (key, c)


FUSABLE = [  # bg, mod, nof_layers, nprb, tbs bits, sigma: every codeblock Z >= 128 (a multiple of 16), rv 0 fits the circular buffer
    (2, 1, 1, 100, 3848, 0.9),
    (2, 2, 1, 60, 3848, 0.75),
    (1, 4, 1, 106, 42016, 0.45),
    (1, 6, 1, 106, 83976, 0.62),
    (1, 8, 1, 273, 319784, 0.3),
    (2, 2, 1, 100, 9984, 1.3),
    (1, 4, 2, 50, 40976, 0.45),
    (1, 2, 1, 81, 8400, 0.8),  # one codeblock, rate 1/3: E = N - fillers... (full circular buffer)
]


@pytest.mark.parametrize("form", ["auto", "throughput"])
@pytest.mark.parametrize("early_stop", [0, 1])
def test_first_transmission_dematched_by_the_decoder(ctx, early_stop, form):
    """A batch of first transmissions (rv 0, new data) takes the path where the LDPC decoder rate-dematches while it loads its
    codeblock: the HARQ soft buffers must hold exactly what the reference's dematcher leaves there (oracle, pinned against the
    reference), results and transport blocks as the oracle; a retransmission (separate dematcher launch, combining into those
    buffers) then also matches."""
    import torch
    import miphy
    # "throughput": the launch geometry of a batch that fills the chip (these few transport blocks would otherwise all take the latency
    # form of the packed kernel with its messages in LDS)
    miphy.lib().miphy_debug_force_ldpc_kernel(4 if form == "throughput" else 0)
    rng = np.random.default_rng(77 + early_stop)
    tbs, slot = [], 0
    for bg, mod, nl, nprb, tbs_bits, sigma in FUSABLE:
        nsym = nprb * 156 * nl
        tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
        seg = o_segmentation(tbs_bits, bg, mod, nl, nsym)
        assert seg.Z >= 128 and seg.Z % 16 == 0
        llrs = [noisy(o_pdsch_encode(bg, rv, mod, 0, nl, nsym, tb), sigma, rng) for rv in (0, 2)]
        od = OraclePuschDecoder(bg, mod, 0, nl, nsym, tbs_bits // 8)
        od.softbuf[:] = 33
        tbs.append(dict(bg=bg, mod=mod, nl=nl, nsym=nsym, tb=tb, llrs=llrs, slot=slot, ncb=seg.nof_cbs, N=seg.N, od=od))
        slot += seg.nof_cbs
    n = len(tbs)
    soft_d = torch.full((slot * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(slot, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    for t, rv in enumerate((0, 2)):
        d = np.zeros(n, dtype=miphy.PuschTbDesc)
        llr_off, tb_off, chunks = 0, 0, []
        for i, x in enumerate(tbs):
            d[i] = (x["bg"], rv, x["mod"], x["nl"], 1 if t == 0 else 0, early_stop, 6, 0, x["nsym"], x["tb"].size, x["slot"], llr_off + 3, tb_off)
            chunks.append(x["llrs"][t])
            llr_off += x["llrs"][t].size
            tb_off += x["tb"].size
        tb_d = torch.full((tb_off,), 0xEE, dtype=torch.uint8, device="cuda")
        llr_all = np.concatenate([np.zeros(3, np.int8)] + chunks)  # every codeword starts at an odd offset
        miphy.lib().miphy_debug_ldpc_kernels_used(1)
        ctx.pusch_decode_batch(d, torch.from_numpy(llr_all).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        used = int(miphy.lib().miphy_debug_ldpc_kernels_used(1))
        # first transmissions: the packed kernel (2) dematches while it loads (FUSED, 4); the retransmission runs the dematcher as a launch of
        # its own. Throughput form: messages in LDS for the high-rate classes, in global memory (GMSG, 8) for the others. Automatic
        # choice: these few codeblocks take the latency form (32) with the messages in LDS -- except the rate-1/3 codeblock, whose LDS
        # image with messages and exchange slots exceeds a CU.
        if form == "throughput":
            assert used == ((2 | 4 | 8) if t == 0 else (2 | 8)), used
        else:
            assert used == ((2 | 4 | 32) if t == 0 else (2 | 32)), used
        res = res_d.cpu().numpy().view(miphy.PuschResult)
        tb_out = tb_d.cpu().numpy()
        soft = soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE)
        for i, x in enumerate(tbs):
            ok, tbo, mm = x["od"].decode(x["llrs"][t], rv, t == 0, 6, bool(early_stop))
            r = res[i]
            key = (i, t, x["bg"], x["mod"], x["tb"].size * 8)
            assert bool(r["tb_crc_ok"]) == ok and (int(r["iters_min"]), int(r["iters_max"])) == mm, (key, r, mm)
            exp_soft = x["od"].softbuf.reshape(x["ncb"], x["N"])
            for c in range(x["ncb"]):
                bad = np.nonzero(soft[x["slot"] + c, :x["N"]] != exp_soft[c])[0]
                assert bad.size == 0, (key, c, bad[:8], soft[x["slot"] + c, bad[:8]], exp_soft[c, bad[:8]])
            if ok:
                o0 = int(d[i]["tb_offset"])
                assert np.array_equal(tb_out[o0:o0 + x["tb"].size], x["tb"]), key
    miphy.lib().miphy_debug_force_ldpc_kernel(0)
    assert any(bool(r["tb_crc_ok"]) for r in res)


@pytest.mark.parametrize("form", ["auto", "throughput"])
def test_mixed_class_plan_replays_as_a_hip_graph(form):
    """A prepared PUSCH decode plan whose codeblocks fall into several launch classes (wave kernel, packed kernel with one and three wavefronts,
    small classes forked to side streams and joined with events) is captured in a HIP graph on its first run and replayed on new LLRs, after a
    larger per-call decode on the same context has grown its workspaces: the results equal the plain runs' and the oracle's verdicts. The
    throughput form keeps decoder messages in global memory, the plan's own scratch. A context of its own: the session's may hold large
    workspaces already."""
    import torch
    import miphy
    ctx = miphy.Context(0)
    miphy.lib().miphy_debug_force_ldpc_kernel({"auto": 0, "throughput": 4}[form])
    try:
        rng = np.random.default_rng(91)
        cases = [(2, 2, 1, 4, 144), (2, 2, 1, 8, 768), (1, 6, 1, 40, 31752), (1, 8, 1, 90, 104496), (2, 4, 1, 16, 3752)]
        tbs, slot = [], 0
        for rep in range(3):
            for bg, mod, nl, nprb, tbs_bits in cases:
                nsym = nprb * 156 * nl
                tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
                seg = o_segmentation(tbs_bits, bg, mod, nl, nsym)
                cw = o_pdsch_encode(bg, 0, mod, 0, nl, nsym, tb)
                tbs.append(dict(bg=bg, mod=mod, nl=nl, nsym=nsym, tb=tb, cw=cw, slot=slot, ncb=seg.nof_cbs))
                slot += seg.nof_cbs
        n = len(tbs)
        d = np.zeros(n, dtype=miphy.PuschTbDesc)
        llr_off, tb_off = 0, 0
        for i, x in enumerate(tbs):
            d[i] = (x["bg"], 0, x["mod"], x["nl"], 1, 1, 6, 0, x["nsym"], x["tb"].size, x["slot"], llr_off, tb_off)
            x["llr_off"], x["tb_off"] = llr_off, tb_off
            llr_off += (x["cw"].size + 15) // 16 * 16
            tb_off += (x["tb"].size + 15) // 16 * 16
        plan = ctx.pusch_decode_plan(d)
        assert plan.nof_launches() >= 4
        soft_d = torch.zeros(slot * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
        msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        crc_d = torch.zeros(slot, dtype=torch.uint8, device="cuda")
        res_d = torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        tb_d = torch.zeros(tb_off, dtype=torch.uint8, device="cuda")
        llr_d = torch.zeros(llr_off, dtype=torch.int8, device="cuda")

        def fill(sigma):
            h = np.zeros(llr_off, np.int8)
            for x in tbs:
                h[x["llr_off"]:x["llr_off"] + x["cw"].size] = noisy(x["cw"], sigma, rng)
            llr_d.copy_(torch.from_numpy(h))
            return h

        h = fill(0.3)
        torch.cuda.synchronize()
        miphy.lib().miphy_debug_ldpc_kernels_used(1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # the plan's first run: its scratch and side streams exist from plan_create
            plan.run(llr_d, soft_d, msgs_d, crc_d, tb_d, res_d, torch.cuda.current_stream())
        used = int(miphy.lib().miphy_debug_ldpc_kernels_used(1))
        if form == "throughput":
            assert used & 8, used  # MIPHY_LDPC_KERNEL_GMSG
        # a larger per-call decode of the same transport blocks, four times over, into buffers of its own: the context's workspaces grow
        reps = 4
        big = np.concatenate([d] * reps)
        for k in range(reps):
            big[k * n:(k + 1) * n]["harq_cb_index"] += k * slot
            big[k * n:(k + 1) * n]["llr_offset"] += k * llr_off
            big[k * n:(k + 1) * n]["tb_offset"] += k * tb_off
        tb_big = torch.zeros(reps * tb_off, dtype=torch.uint8, device="cuda")
        res_big = torch.zeros(reps * n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        ctx.pusch_decode_batch(big, llr_d.repeat(reps), torch.zeros(reps * slot * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda"),
                               torch.zeros(reps * slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda"),
                               torch.zeros(reps * slot, dtype=torch.uint8, device="cuda"), tb_big, res_big)
        torch.cuda.synchronize()
        res_b = res_big.cpu().numpy().view(miphy.PuschResult).reshape(reps, n)
        for i, x in enumerate(tbs):
            od = OraclePuschDecoder(x["bg"], x["mod"], 0, x["nl"], x["nsym"], x["tb"].size)
            ok, tbo, mm = od.decode(h[x["llr_off"]:x["llr_off"] + x["cw"].size], 0, True, 6, True)
            for k in range(reps):
                assert bool(res_b[k, i]["tb_crc_ok"]) == ok and (int(res_b[k, i]["iters_min"]), int(res_b[k, i]["iters_max"])) == mm, (i, k)
        for sigma in (0.25, 0.5):
            h = fill(sigma)
            tb_d.zero_()
            g.replay()
            torch.cuda.synchronize()
            res = res_d.cpu().numpy().view(miphy.PuschResult).copy()
            got = tb_d.cpu().numpy().copy()
            tb_d.zero_()
            plan.run(llr_d, soft_d, msgs_d, crc_d, tb_d, res_d)
            torch.cuda.synchronize()
            assert np.array_equal(res_d.cpu().numpy().view(miphy.PuschResult), res)
            assert np.array_equal(tb_d.cpu().numpy(), got)
            for i, x in enumerate(tbs):
                od = OraclePuschDecoder(x["bg"], x["mod"], 0, x["nl"], x["nsym"], x["tb"].size)
                ok, tbo, mm = od.decode(h[x["llr_off"]:x["llr_off"] + x["cw"].size], 0, True, 6, True)
                assert bool(res[i]["tb_crc_ok"]) == ok and (int(res[i]["iters_min"]), int(res[i]["iters_max"])) == mm, (i, sigma)
                if ok:
                    assert np.array_equal(got[x["tb_off"]:x["tb_off"] + x["tb"].size], x["tb"]), (i, sigma)
        del g
        plan.close()
    finally:
        miphy.lib().miphy_debug_force_ldpc_kernel(0)
        torch.cuda.synchronize()
        ctx.close()


def test_smallest_full_image_and_creates_that_fail(ctx):
    """The smallest PUSCH batch in which every array of the decode's device image is non-empty: two new transmissions of one codeblock each, one
    on base graph 1 with Z = 384 (a packed class that dematches while it loads), one on base graph 2 with Z = 24 (a wave class: a bundle, and a
    dematcher descriptor of its own). Per call and as a plan: bits, iteration counts and result records as the oracle's. Then every create
    function -- PUSCH decode plan, LDPC decode plan, PDSCH process plan and the prepared PDSCH encode inside it -- refuses a batch with one
    invalid entry with MIPHY_EINVAL, and a valid create and run on the same context afterwards still gives the oracle's results."""
    import torch
    import miphy
    import dl_grid as D
    import oracle_lib as O
    from miphy.ldpc import make_dec_descs
    from test_pdsch_mod_gpu import _words
    rng = np.random.default_rng(2024)

    def refused(what, make):
        with pytest.raises(RuntimeError, match=r"miphy error -1: .*" + what):
            make()

    # ---- PUSCH decode
    tbs, slot, llr_off, tb_off = [], 0, 0, 0
    for bg, nbytes, nprb, Z, sigma in [(1, 1000, 52, 384, 0.6), (2, 16, 2, 24, 0.6)]:
        seg = miphy.sch_segmentation(nbytes, bg)
        assert (seg.nof_cbs, seg.Z) == (1, Z)
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        nsym = nprb * 156
        llr = noisy(o_pdsch_encode(bg, 0, 2, 0, 1, nsym, tb), sigma, rng)
        tbs.append(dict(bg=bg, nsym=nsym, tb=tb, llr=llr, slot=slot, llr_off=llr_off, tb_off=tb_off))
        slot, llr_off, tb_off = slot + 1, llr_off + (llr.size + 15) // 16 * 16, tb_off + (nbytes + 15) // 16 * 16
    n = len(tbs)
    d = np.zeros(n, dtype=miphy.PuschTbDesc)
    llr_h = np.zeros(llr_off, np.int8)
    for i, x in enumerate(tbs):
        d[i] = (x["bg"], 0, 2, 1, 1, 1, 6, 0, x["nsym"], x["tb"].size, x["slot"], x["llr_off"], x["tb_off"])
        llr_h[x["llr_off"]:x["llr_off"] + x["llr"].size] = x["llr"]
        od = OraclePuschDecoder(x["bg"], 2, 0, 1, x["nsym"], x["tb"].size)
        x["ok"], x["tbo"], x["mm"] = od.decode(x["llr"], 0, True, 6, True)
        x["soft"] = od.softbuf.copy()
    assert all(x["ok"] for x in tbs)
    llr_d = torch.from_numpy(llr_h).cuda()

    def decode_and_check(run):
        soft_d = torch.full((slot * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
        msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        crc_d = torch.ones(slot, dtype=torch.uint8, device="cuda")
        res_d = torch.zeros(n * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
        tb_d = torch.full((tb_off,), 0xEE, dtype=torch.uint8, device="cuda")
        run(llr_d, soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        res, got, soft = res_d.cpu().numpy().view(miphy.PuschResult), tb_d.cpu().numpy(), soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE)
        for i, x in enumerate(tbs):
            r = res[i]
            assert bool(r["tb_crc_ok"]) and int(r["nof_codeblocks_total"]) == 1 and int(r["nof_decoded"]) == 1, (i, r)
            assert (int(r["iters_min"]), int(r["iters_max"])) == x["mm"] and float(r["iters_mean"]) == float(x["mm"][0]), (i, r, x["mm"])
            assert np.array_equal(got[x["tb_off"]:x["tb_off"] + x["tb"].size], x["tb"]) and np.array_equal(x["tbo"], x["tb"]), i
            assert np.array_equal(soft[x["slot"], :x["soft"].size], x["soft"]), i
        return res.copy(), got

    miphy.lib().miphy_debug_ldpc_kernels_used(1)
    res_call, tb_call = decode_and_check(lambda *a: ctx.pusch_decode_batch(d, *a))
    used = int(miphy.lib().miphy_debug_ldpc_kernels_used(1))
    assert used & 2 and used & 4 and used & 16, used  # packed + dematching while it loads, and the wave kernel (MIPHY_LDPC_KERNEL_WAVE)
    bad = d.copy()
    bad[1]["mod"] = 3
    refused("invalid modulation", lambda: ctx.pusch_decode_plan(bad))
    plan = ctx.pusch_decode_plan(d)
    assert plan.info()[0] == 2 and plan.nof_launches() == 2
    for _ in range(2):
        res_plan, tb_plan = decode_and_check(plan.run)
        assert np.array_equal(res_plan, res_call) and np.array_equal(tb_plan, tb_call)
    plan.close()

    # ---- LDPC decode plan: two BG1 / Z = 384 codeblocks as in smoke(), the second descriptor of the refused batch with no iterations
    bg, Z, nf, mod, E, ncb = 1, 384, 8, 8, 8968, 2
    K, N = 22 * Z, 66 * Z
    sb, exp = np.zeros((ncb, N), np.int8), []
    for i in range(ncb):
        msg = rng.integers(0, 2, K, dtype=np.uint8)
        c = O.o_crc_bits(O.CRC24B, msg[:K - nf - 24])
        msg[K - nf - 24:K - nf] = [(c >> (23 - j)) & 1 for j in range(24)]
        msg[K - nf:] = 254
        rm = O.o_rate_match(0, mod, 0, nf, O.o_ldpc_encode(bg, Z, msg, N), E)
        sb[i] = O.o_rate_dematch(0, mod, 0, nf, 1, noisy(rm, 0.25, rng), np.zeros(N, np.int8))
        exp.append(O.o_ldpc_decode(bg, Z, sb[i], nf, O.CRC24B, 6))
    descs = make_dec_descs(ncb, bg, Z, N, miphy.CRC24B, 6, nf)
    bad = descs.copy()
    bad[1]["max_iter"] = 0
    refused("max_iter", lambda: miphy.LdpcDecodePlan(ctx, bad))
    lplan = miphy.LdpcDecodePlan(ctx, descs)
    out_d = torch.zeros(ncb * K // 8, dtype=torch.uint8, device="cuda")
    it_d = torch.zeros(ncb, dtype=torch.int32, device="cuda")
    lplan.run(torch.from_numpy(sb.reshape(-1)).cuda(), out_d, it_d)
    torch.cuda.synchronize()
    for i in range(ncb):
        assert int(it_d[i].item()) == exp[i][0] and exp[i][0] > 0, i
        assert np.array_equal(out_d.cpu().numpy().reshape(ncb, K // 8)[i], exp[i][1]), i
    lplan.close()

    # ---- PDSCH process plan: one PDU refused by the processor's own rules, one by the prepared encoder underneath it
    nprb, dsyms = 25, (2,)
    rb = np.zeros(nprb, np.uint8)
    rb[3:7] = 1
    pdus = np.zeros(2, dtype=miphy.PdschPdu)
    want, ptbs = [], []
    for i, nbytes in enumerate((40, 24)):
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        p = pdus[i]
        p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"], p["tbs_lbrm_bytes"], p["tb_bytes"] = 3 + i, 0x1234 + i, 77, 99, 400, nbytes
        p["bg"], p["rv"], p["mod"], p["port"], p["start_symbol"], p["nof_symbols"] = 2, 0, 2, 0, 0, 14
        p["nof_cdm_groups_without_data"], p["n_scid"], p["ref_point_prb0"], p["nof_reserved"] = 1, 0, 0, 0
        p["dmrs_symbols_mask"], p["grid_nof_prb"], p["bwp_start_rb"], p["bwp_size_rb"], p["rb_mask"] = 1 << 2, nprb, 0, nprb, _words(rb)
        p["tb_offset"], p["grid_offset"] = 64 * i, i * 14 * nprb * 12
        g = np.zeros((1, 14, nprb * 12), dtype=np.complex64)
        D.o_pdsch_process(dict(bg=2, rv=0, mod=2, lbrm_bytes=400, tb=tb, rnti=0x1234 + i, n_id=77, slot=3 + i, scr=99, n_scid=0, start=0, nof=14, dmrs_symbols=dsyms,
                               cdm=1, bwp=(0, nprb), rb=rb, reserved=[], port=0, ref_point_prb0=0, dmrs_dB=0.0, data_dB=0.0), g)
        want.append(g.reshape(-1))
        ptbs.append(tb)
    bad = pdus.copy()
    bad[1]["nof_cdm_groups_without_data"] = 3
    refused("CDM groups", lambda: miphy.PdschProcessPlan(ctx, bad))
    bad = pdus.copy()
    bad[1]["tb_bytes"] = 0
    refused("sch: transport block size 0 bytes", lambda: miphy.PdschProcessPlan(ctx, bad))
    pplan = miphy.PdschProcessPlan(ctx, pdus)
    tb_all = np.zeros(128, np.uint8)
    tb_all[0:40], tb_all[64:88] = ptbs[0], ptbs[1]
    gd = torch.zeros(2 * 14 * nprb * 12, dtype=torch.complex64, device="cuda")
    pplan.run(torch.from_numpy(tb_all).cuda(), gd)
    torch.cuda.synchronize()
    assert np.array_equal(gd.cpu().numpy().view(np.uint32), np.concatenate(want).view(np.uint32))
    pplan.close()
