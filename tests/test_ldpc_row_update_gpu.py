"""GPU parity of two places of the packed row update (csrc/ldpc_pk_device.h) where a cheaper instruction sequence is tempting and a
wrong one is quiet: the 0.8 scaling of the two row minima (floor(x * 52428 / 65536); a 16-bit form such as floor(x * 409 / 512) equals it
on 0 ... 160 only, and 408 or 410 in its place are off by one at some minima) and the split of a row pair's soft-bit addresses, which
adds the column offset in one of two forms (pk_edge_addresses, FOLD). Expected values always come from the CPU oracle, bit for bit; the
compared outputs are hard bits, CRC verdict and iteration count.

Scaling: a minimum off by one must reach a hard decision or an iteration count, so the inputs are random (every soft bit matters,
nothing converges by a wide margin) next to noisy codewords (the CRC stops them at an iteration that depends on the messages), at
iteration limits 1, 2 and 6. The magnitude bands |s| <= 4, 16, 64, 120 (each mixed with exact zeros and +-127) spread the minima over
the range; the plateau codeblocks make the coverage certain: in plateau m no soft bit is smaller than m and a third of them equal m, so
that in the first visit of a layer min1 = m wherever a row holds such a soft bit and min2 = m wherever it holds two (rows with hundreds
of instances per codeblock), for every m = 0 ... 120.

Addresses: full-length inputs reach all 46 / 42 layers and the largest column offsets (column 67 of BG1 at Z = 384 starts at byte 25 728),
in every launch form the suite names, with the kernel that ran asserted from miphy_debug_ldpc_kernels_used."""
import functools

import numpy as np
import pytest

from oracle_lib import (BG_K, BG_NS, CRC16, CRC24B, CRC_ORDER, OraclePuschDecoder, o_crc_bits, o_ldpc_decode, o_ldpc_encode, o_pdsch_encode,
                        o_segmentation)

pytestmark = pytest.mark.gpu

SCALAR, PACKED, FUSED, GMSG, WAVE, SPLIT, GMSG_PART = 1, 2, 4, 8, 16, 32, 64  # MIPHY_LDPC_KERNEL_* (include/miphy.h)
# miphy_debug_force_ldpc_kernel: class-sorted launches in the geometry of a full chip; automatic (few codeblocks: latency form in four
# parts); the same in two parts; the packed kernel as one launch for the whole batch
FORMS = {"throughput": 4, "latency4": 0, "latency2": 6, "single": 2}
LATENCY_ALL = 5  # the latency form in two parts on every packed class, however many codeblocks it has
ALL_GMSG = 0x100
BANDS = (4, 16, 64, 120)


def force_kernel(mode):
    import miphy
    miphy.lib().miphy_debug_force_ldpc_kernel(mode)
    miphy.lib().miphy_debug_ldpc_kernels_used(1)


def kernels_used():
    import miphy
    return int(miphy.lib().miphy_debug_ldpc_kernels_used(1))


def crc_of(bg, Z):
    return CRC24B if BG_K[bg] * Z > 60 else CRC16


def codeword_bits(bg, Z, rng, poly):
    K, nb = BG_K[bg] * Z, CRC_ORDER[poly]
    msg = rng.integers(0, 2, K, dtype=np.uint8)
    c = o_crc_bits(poly, msg[:K - nb])
    msg[K - nb:] = [(c >> (nb - 1 - i)) & 1 for i in range(nb)]
    return o_ldpc_encode(bg, Z, msg, BG_NS[bg] * Z) & 1


def sprinkle(llr, rng, sign):
    """Exact zeros and +-127 (an infinite soft bit: no iteration changes its sign, so the sign is given) over a few percent of the soft bits each."""
    u = rng.random(llr.size)
    llr[u < 0.04] = 0
    hit = u > 0.96
    llr[hit] = (127 * sign[hit]).astype(np.int8)
    return llr


def band_inputs(bg, Z, rng):
    """Per band: soft bits uniform in [-band, band], and a codeword received at an amplitude of half the band with noise, clipped to the band."""
    n, out = BG_NS[bg] * Z, []
    for band in BANDS:
        out.append(sprinkle(rng.integers(-band, band + 1, n).astype(np.int8), rng, 1 - 2 * rng.integers(0, 2, n)))
        tx = 1 - 2 * codeword_bits(bg, Z, rng, crc_of(bg, Z)).astype(np.int64)
        out.append(sprinkle(np.clip(np.round((tx + 0.7 * rng.standard_normal(n)) * band / 2.0), -band, band).astype(np.int8), rng, tx))
    return out


def plateau_inputs(bg, Z, rng):
    """Plateau m = 0 ... 120: magnitudes >= m, a third of them exactly m, signs of a codeword with 1 to 4 in 64 flipped (some plateaus
    pass their CRC after a few iterations, some never)."""
    n, out = BG_NS[bg] * Z, []
    for m in range(121):
        mag = np.where(rng.random(n) < 1.0 / 3, m, rng.integers(m, 121, n))
        sign = 1 - 2 * (codeword_bits(bg, Z, rng, crc_of(bg, Z)).astype(np.int64) ^ (rng.random(n) < (1 + m % 4) / 64.0))
        out.append((sign * mag).astype(np.int8))
    return out


def make_cases(inputs_by_graph, Z, max_iter):
    cases = []
    for bg, inputs in inputs_by_graph:
        K = BG_K[bg] * Z
        for llr in inputs:
            for crc in (crc_of(bg, Z), -1):
                c = dict(bg=bg, Z=Z, llr=llr, nf=0, crc=crc, flags=0, max_iter=max_iter)
                its, bits = o_ldpc_decode(bg, Z, llr, 0, crc, max_iter, out_init=np.full((K + 7) // 8, 0x5A, dtype=np.uint8))
                bits.setflags(write=False)
                c["exp"] = (its, bits)
                cases.append(c)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def scaling_cases(Z, max_iter):
    """Both base graphs, with and without CRC early stop; the plateaus at the sizes where 121 codeblocks are small."""
    rng = np.random.default_rng(7000 + Z)  # (the inputs of a size are the same at every iteration limit)
    by_graph = []
    for bg in (1, 2):
        inputs = band_inputs(bg, Z, rng)
        if Z <= 144:
            inputs += plateau_inputs(bg, Z, rng)
        by_graph.append((bg, inputs))
    return make_cases(by_graph, Z, max_iter)


def decode(ctx, cases, repeat=1):
    """One call for `cases`, each `repeat` times (host descriptors) -> [(iterations, hard bits)] in that order."""
    import torch
    import miphy
    n = len(cases) * repeat
    descs = np.zeros(n, dtype=miphy.LdpcDecDesc)
    llr_off, out_off, first = [], 0, 0
    for c in cases:
        llr_off.append(first)
        first += c["llr"].size
    for i in range(n):
        c = cases[i % len(cases)]
        descs[i] = (c["bg"], c["crc"] if c["crc"] >= 0 else miphy.CRC_NONE, c["Z"], c["max_iter"], c["nf"], c["llr"].size, c["flags"], llr_off[i % len(cases)], out_off)
        out_off += (BG_K[c["bg"]] * c["Z"] + 7) // 8
    llr_d = torch.from_numpy(np.concatenate([c["llr"] for c in cases])).cuda()
    out_d = torch.full((out_off,), 0x5A, dtype=torch.uint8, device="cuda")
    it_d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctx.ldpc_decode_batch(descs, llr_d, out_d, it_d)
    torch.cuda.synchronize()
    out, its = out_d.cpu().numpy(), it_d.cpu().numpy()
    return [(int(its[i]), out[int(descs[i]["out_offset"]):int(descs[i]["out_offset"]) + (BG_K[descs[i]["bg"]] * int(descs[i]["Z"]) + 7) // 8]) for i in range(n)]


def mismatches(cases, got):
    bad = []
    for i, g in enumerate(got):
        c = cases[i % len(cases)]
        e = c["exp"]
        if g[0] != e[0] or not np.array_equal(g[1], e[1]):
            bad.append((i, c["bg"], c["Z"], c["crc"], c["max_iter"], "iterations %d, oracle %d" % (g[0], e[0]), "%d hard bytes differ" % int(np.sum(e[1] != g[1]))))
    return bad


# the wave kernel (6, 36), the packed kernel with one and two wavefronts per codeblock (72, 144) and with three (384)
@pytest.mark.parametrize("max_iter", [1, 2, 6])
@pytest.mark.parametrize("Z", [6, 36, 72, 144, 384])
def test_scaled_minima(ctx, Z, max_iter):
    cases = scaling_cases(Z, max_iter)
    try:
        # the throughput form, and the latency form, whose parts merge their minima before they are scaled (the wave kernel has one form)
        for mode in (FORMS["throughput"], LATENCY_ALL) if Z > 64 else (FORMS["throughput"],):
            force_kernel(mode)
            got = decode(ctx, cases)
            used = kernels_used()
            if Z <= 64:
                assert used & WAVE and not used & (SCALAR | PACKED | SPLIT), (mode, used)
            else:
                assert used & PACKED and not used & (SCALAR | WAVE) and bool(used & SPLIT) == (mode == LATENCY_ALL), (mode, used)
            bad = mismatches(cases, got)
            assert not bad, (mode, len(bad), bad[:8])
    finally:
        force_kernel(0)


ADDRESS_SIZES = (3, 15, 64, 128, 256, 288, 384)


@functools.lru_cache(maxsize=None)
def address_cases(bg, Z):
    """Six full-length codeblocks: codewords from clean to beyond what six iterations repair, and two of random soft bits."""
    rng = np.random.default_rng(9000 + 10 * Z + bg)
    n, inputs = BG_NS[bg] * Z, []
    for sigma in (0.5, 0.8, 1.0, 1.2):
        y = (1.0 - 2.0 * codeword_bits(bg, Z, rng, crc_of(bg, Z))) + sigma * rng.standard_normal(n)
        inputs.append(np.round(np.clip(4 * y, -20, 20) / 20 * 120).astype(np.int8))
    for band in (16, 120):
        inputs.append(rng.integers(-band, band + 1, n).astype(np.int8))
    cases = make_cases([(bg, inputs)], Z, 6)
    return tuple(c for c in cases if c["crc"] >= 0 or c["llr"] is inputs[1] or c["llr"] is inputs[5])  # (all with the CRC, two without as well)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("Z", ADDRESS_SIZES)
@pytest.mark.parametrize("bg", [1, 2])
def test_soft_bit_addresses_of_full_length_codeblocks(ctx, bg, Z, form):
    cases = address_cases(bg, Z)
    assert 2 <= len(cases) <= 8 and all(c["llr"].size == BG_NS[bg] * Z for c in cases)
    try:
        force_kernel(FORMS[form])
        got = decode(ctx, cases)
        used = kernels_used()
        if form == "single":
            assert used & PACKED and not used & (SCALAR | WAVE | SPLIT), used
        elif Z <= 64:
            # bundles of min(codeblocks that share CRC and limits, floor(64 / ceil(Z / 2))) codeblocks per wavefront: the groups behind
            # the first have a non-zero base
            assert used & WAVE and not used & (SCALAR | PACKED | SPLIT), used
        else:
            assert used & PACKED and not used & (SCALAR | WAVE), used
            # BG1 at Z = 384 with all 46 layers: 157 504 B of soft bits and messages, and the exchange slots of four parts (9 216 B) do
            # not fit the 160 KiB of a CU beside them, those of two parts (4 608 B) do
            split = form == "latency2" or (form == "latency4" and not (bg == 1 and Z == 384))
            assert bool(used & SPLIT) == split, used
        bad = mismatches(cases, got)
        assert not bad, (len(bad), bad[:8])
    finally:
        force_kernel(0)


@pytest.mark.parametrize("bg,nodes", [(1, 68), (2, 52), (1, 37)])
def test_soft_bit_addresses_with_messages_in_global_memory(ctx, bg, nodes):
    """A batch that fills the chip (640 codeblocks at Z = 384, eight distinct inputs) moves messages to global memory: full length with
    every message there, and BG1 at 15 layers, where the automatic choice keeps the first layers' messages in LDS (the split placement)
    and mode | 0x100 switches that off."""
    Z = 384
    cases = tuple(dict(c, llr=c["llr"][:(nodes - 2) * Z]) for c in address_cases(bg, Z))
    if nodes != BG_NS[bg] + 2:
        K = BG_K[bg] * Z
        for c in cases:
            c["exp"] = o_ldpc_decode(bg, Z, c["llr"], 0, c["crc"], 6, out_init=np.full((K + 7) // 8, 0x5A, dtype=np.uint8))
    try:
        for mode in (0, ALL_GMSG):
            force_kernel(mode)
            got = decode(ctx, cases, repeat=640 // len(cases))
            used = kernels_used()
            assert used & PACKED and used & GMSG and not used & (SPLIT | SCALAR | WAVE), (mode, used)
            if nodes == 37:
                assert bool(used & GMSG_PART) == (mode == 0), (mode, used)
            bad = mismatches(cases, got)
            assert not bad, (mode, len(bad), bad[:8])
    finally:
        force_kernel(0)


# base graph: modulation, PRBs, TB bits, noise of the two TBs. Two codeblocks of Z = 384 per TB; E + fillers stays just below the
# buffer length (what the decoder needs to dematch while it loads) and reaches into its last column, so that every layer is visited.
FUSED_TBS = {1: (4, 79, 16008, (0.9, 1.25)), 2: (2, 121, 7000, (1.0, 1.35))}


@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("form", ["auto", "throughput"])
def test_soft_bit_addresses_in_the_decoder_that_dematches(ctx, form, bg):
    """First transmissions through a prepared plan (latency form for so few codeblocks, throughput form when forced), all layers reached:
    transport blocks, CRC flags, iteration counts and soft buffers as the oracle chain."""
    import torch
    import miphy
    rng = np.random.default_rng(9500 + bg)
    mod, nprb, tbs_bits, sigmas = FUSED_TBS[bg]
    nsym, max_iter = nprb * 156, 6
    seg = o_segmentation(tbs_bits, bg, mod, 1, nsym)
    ncb, N = seg.nof_cbs, seg.N
    assert seg.Z == 384 and ncb == 2 and N == BG_NS[bg] * 384
    tbs = [rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8) for _ in sigmas]
    cws = [o_pdsch_encode(bg, 0, mod, 0, 1, nsym, tb) for tb in tbs]
    E = cws[0].size
    assert (BG_NS[bg] - 1) * 384 < E // ncb + seg.nof_filler_bits <= N  # the last soft bit received lies in the last column
    llrs = [np.round(np.clip(4 * ((1.0 - 2.0 * (cw & 1)) + s * rng.standard_normal(E)), -20, 20) / 20 * 120).astype(np.int8) for cw, s in zip(cws, sigmas)]
    d = np.zeros(2, dtype=miphy.PuschTbDesc)
    for i in range(2):
        d[i] = (bg, 0, mod, 1, 1, 1, max_iter, 0, nsym, tbs_bits // 8, i * ncb, i * E, i * (tbs_bits // 8))
    soft_d = torch.full((2 * ncb * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(2 * ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(2 * ncb, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(2 * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    tb_d = torch.full((2 * (tbs_bits // 8),), 0xEE, dtype=torch.uint8, device="cuda")
    force_kernel(FORMS["throughput"] if form == "throughput" else 0)
    plan = None
    try:
        plan = ctx.pusch_decode_plan(d)
        plan.run(torch.from_numpy(np.concatenate(llrs)).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        used = kernels_used()
        # (BG1 with all its layers has no room for the exchange slots of four parts: see the test of the forms above)
        split = form == "auto" and bg == 2
        assert used == (PACKED | FUSED | (SPLIT if split else 0) | (used & (GMSG | GMSG_PART))), used
        res, tb_out = res_d.cpu().numpy().view(miphy.PuschResult), tb_d.cpu().numpy().reshape(2, -1)
        crc, soft = crc_d.cpu().numpy(), soft_d.cpu().numpy().reshape(2 * ncb, miphy.HARQ_CB_STRIDE)[:, :N]
        for i in range(2):
            od = OraclePuschDecoder(bg, mod, 0, 1, nsym, tbs_bits // 8)
            od.softbuf[:] = 33
            ok, tbo, mm = od.decode(llrs[i], 0, True, max_iter, True)
            key = (i, ok, mm)
            assert bool(res[i]["tb_crc_ok"]) == ok and res[i]["nof_codeblocks_total"] == ncb, (key, res[i])
            assert (int(res[i]["iters_min"]), int(res[i]["iters_max"])) == mm, (key, res[i])
            assert np.array_equal(crc[i * ncb:(i + 1) * ncb], od.cb_crc), (key, crc)
            assert np.array_equal(soft[i * ncb:(i + 1) * ncb], od.softbuf.reshape(ncb, N)), key
            if ok:
                assert np.array_equal(tb_out[i], tbo) and np.array_equal(tb_out[i], tbs[i]), key
    finally:
        force_kernel(0)
        if plan is not None:
            plan.close()
