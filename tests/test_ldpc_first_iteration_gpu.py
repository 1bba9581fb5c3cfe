"""GPU parity of the LDPC decoders' first iteration, which does not visit layer 0 and runs layers 1 and 2 in a form that knows one of
their inputs to be zero (the punctured columns; update_rows_pk_zero in csrc/ldpc_pk_device.h): hard bits and iteration counts against
the CPU oracle, and against the one-row-per-lane kernel (which visits every layer in full) on the same batch. The corners where the
shortcut can go wrong: iteration limits 1 (layer 0 is never visited), 2 (its first visit is in iteration 1) and more; soft bits so small
that the scaled minima are zero; raw inputs of magnitude 121 ... 127, which the skipped stores would have rewritten to 127; whole columns
of zeros; fillers; both message homes and their split; the variant that dematches while it loads."""
import functools

import numpy as np
import pytest

from oracle_lib import (BG_K, BG_NS, CRC16, CRC24B, CRC_ORDER, OraclePuschDecoder, o_crc_bits, o_ldpc_decode, o_ldpc_encode, o_pdsch_encode,
                        o_segmentation)

pytestmark = pytest.mark.gpu

MODES = {"auto": 0, "scalar": 1, "packed": 2, "throughput": 4, "latency2": 6}  # miphy_debug_force_ldpc_kernel
SCALAR, PACKED, FUSED, GMSG, WAVE, SPLIT, GMSG_PART = 1, 2, 4, 8, 16, 32, 64  # MIPHY_LDPC_KERNEL_* (include/miphy.h)
# odd Z, the wave kernel (Z <= 64), one-, two- and three-wavefront workgroups of the packed kernel
SIZES = (3, 15, 64, 72, 208, 384)
# a column of each base graph that, among layers 0 ... 3, only layers 1 and 2 read: nothing general touches it before iteration 1
COLUMN_OF_LAYERS_1_2 = {1: 24, 2: 12}
FINAL_ONLY = 1  # descriptor flag: CRC checked once, after the last iteration


def force_kernel(mode):
    import miphy
    miphy.lib().miphy_debug_force_ldpc_kernel(mode)
    miphy.lib().miphy_debug_ldpc_kernels_used(1)


def kernels_used():
    import miphy
    return int(miphy.lib().miphy_debug_ldpc_kernels_used(1))


def codeword_llrs(bg, Z, rng, nf, poly, length, sigma):
    """A codeword with its checksum (and nf fillers, received as +127) through a noisy channel, the first `length` soft bits."""
    K, nb = BG_K[bg] * Z, CRC_ORDER[poly]
    msg = rng.integers(0, 2, K, dtype=np.uint8)
    c = o_crc_bits(poly, msg[:K - nf - nb])
    msg[K - nf - nb:K - nf] = [(c >> (nb - 1 - i)) & 1 for i in range(nb)]
    if nf:
        msg[K - nf:] = 254
    cw = o_ldpc_encode(bg, Z, msg, BG_NS[bg] * Z)[:length]
    y = (1.0 - 2.0 * (cw & 1)) + sigma * rng.standard_normal(length)
    llr = np.round(np.clip(4 * y, -20, 20) / 20 * 120).astype(np.int8)
    if nf:
        llr[K - 2 * Z - nf:K - 2 * Z] = 127
    return llr


def input_kinds(bg, Z, rng, length):
    """The inputs of one (base graph, lifting size, length): (soft bits, fillers). Soft bit i belongs to column 2 + i // Z."""
    K = BG_K[bg] * Z
    poly = CRC24B if K > 60 else CRC16
    col = (COLUMN_OF_LAYERS_1_2[bg] - 2) * Z
    out = [(codeword_llrs(bg, Z, rng, 0, poly, length, 0.55), 0)]
    # {-2 ... 2}: floor(0.8 min) is 0 or 1, column 0 stays zero into layer 2 for many rows
    out.append((rng.integers(-2, 3, length).astype(np.int8), 0))
    # raw magnitudes 121 ... 126 and 127 over a tenth of the soft bits and over the whole column that only layers 1 and 2 read
    big = codeword_llrs(bg, Z, rng, 0, poly, length, 0.7)
    hit = rng.random(length) < 0.1
    hit[col:col + Z] = True
    mags = rng.integers(121, 128, length)
    big[hit] = (np.where(big < 0, -mags, mags)[hit]).astype(np.int8)
    big[rng.random(length) < 0.02] = -127  # some of them wrong-signed
    out.append((big, 0))
    # whole columns of zeros (column 2, column 5, the column of layers 1 and 2) and fillers at +127
    nf = Z // 4
    zc = codeword_llrs(bg, Z, rng, nf, poly, length, 0.5)
    for c0 in (0, 3 * Z, col):
        zc[c0:c0 + Z] = 0
    out.append((zc, nf))
    return poly, out


@functools.lru_cache(maxsize=None)
def batch(max_iter):
    """Every case of one iteration limit with what the oracle decodes from it (computed once, shared by the kernel modes): both base
    graphs, every size, input lengths K + 2 Z (four layers) and full, each input with CRC early stop, without a CRC and with the CRC after
    the last iteration only."""
    rng = np.random.default_rng(100 + max_iter)
    cases = []
    for bg in (1, 2):
        for Z in SIZES:
            K = BG_K[bg] * Z
            for length in (K + 2 * Z, BG_NS[bg] * Z):
                poly, kinds = input_kinds(bg, Z, rng, length)
                for llr, nf in kinds:
                    for crc, flags in ((poly, 0), (-1, 0), (poly, FINAL_ONLY)):
                        cases.append(dict(bg=bg, Z=Z, llr=llr, nf=nf, crc=crc, flags=flags, max_iter=max_iter))
    for c in cases:
        K = BG_K[c["bg"]] * c["Z"]
        init = np.full((K + 7) // 8, 0x5A, dtype=np.uint8)
        if c["flags"] & FINAL_ONLY:  # pusch_decoder_impl.cpp:105-118
            _, bits = o_ldpc_decode(c["bg"], c["Z"], c["llr"], c["nf"], -1, max_iter, out_init=init)
            its = max_iter if o_crc_bits(c["crc"], np.unpackbits(bits)[:K - c["nf"]]) == 0 else 0
        else:
            its, bits = o_ldpc_decode(c["bg"], c["Z"], c["llr"], c["nf"], c["crc"], max_iter, out_init=init)
        bits.setflags(write=False)
        c["exp"] = (its, bits)
    return tuple(cases)


def decode(ctx, cases):
    """One call for `cases` (host descriptors) -> [(iterations, hard bits)]."""
    import torch
    import miphy
    descs = np.zeros(len(cases), dtype=miphy.LdpcDecDesc)
    llr_off, out_off = 0, 0
    for i, c in enumerate(cases):
        descs[i] = (c["bg"], c["crc"] if c["crc"] >= 0 else miphy.CRC_NONE, c["Z"], c["max_iter"], c["nf"], c["llr"].size, c["flags"], llr_off, out_off)
        llr_off += c["llr"].size
        out_off += (BG_K[c["bg"]] * c["Z"] + 7) // 8
    llr_d = torch.from_numpy(np.concatenate([c["llr"] for c in cases])).cuda()
    out_d = torch.full((out_off,), 0x5A, dtype=torch.uint8, device="cuda")
    it_d = torch.full((len(cases),), -7, dtype=torch.int32, device="cuda")
    ctx.ldpc_decode_batch(descs, llr_d, out_d, it_d)
    torch.cuda.synchronize()
    out, its = out_d.cpu().numpy(), it_d.cpu().numpy()
    return [(int(its[i]), out[int(descs[i]["out_offset"]):int(descs[i]["out_offset"]) + (BG_K[c["bg"]] * c["Z"] + 7) // 8]) for i, c in enumerate(cases)]


def mismatches(cases, got, exp):
    return [(i, c["bg"], c["Z"], c["llr"].size, c["crc"], c["flags"], c["nf"], e[0], g[0], int(np.sum(e[1] != g[1])))
            for i, (c, g, e) in enumerate(zip(cases, got, exp)) if g[0] != e[0] or not np.array_equal(g[1], e[1])]


@pytest.mark.parametrize("max_iter", [1, 2, 3, 6])
@pytest.mark.parametrize("mode", list(MODES))
def test_first_iteration_corners(ctx, mode, max_iter):
    """Every case as ONE heterogeneous batch and as one batch per (base graph, lifting size) -- the geometry of that size: wavefronts
    per codeblock, message home -- against the oracle and against the one-row-per-lane kernel run on the same batch."""
    cases = batch(max_iter)
    exp = [c["exp"] for c in cases]
    try:
        force_kernel(MODES["scalar"])
        by_row = decode(ctx, cases)
        assert kernels_used() == SCALAR
        force_kernel(MODES[mode])
        got = decode(ctx, cases)
        used = kernels_used()
        assert (used == SCALAR) if mode == "scalar" else (used & PACKED and not used & SCALAR), used
        if mode in ("auto", "throughput", "latency2"):
            assert used & WAVE, used
        if mode == "throughput":
            assert not used & SPLIT, used
        bad = mismatches(cases, got, exp)
        assert not bad, bad[:10]
        bad = mismatches(cases, got, by_row)
        assert not bad, bad[:10]
        for key in sorted({(c["bg"], c["Z"]) for c in cases}):
            idx = [i for i, c in enumerate(cases) if (c["bg"], c["Z"]) == key]
            sub = [cases[i] for i in idx]
            bad = mismatches(sub, decode(ctx, sub), [exp[i] for i in idx])
            assert not bad, (key, bad[:10])
    finally:
        force_kernel(0)


@pytest.mark.parametrize("max_iter", [1, 2, 5])
def test_first_iteration_with_messages_split_between_lds_and_global_memory(ctx, max_iter):
    """A batch that fills the chip, at a code rate where the launcher keeps the first layers' messages in LDS and moves the others to
    global memory (640 codeblocks of BG1 / Z = 384 at 15 layers, eight distinct inputs): layer 0's slots are not written in iteration 0 in
    either home; the same with every message in global memory (mode | 0x100)."""
    import torch
    import miphy
    rng = np.random.default_rng(300 + max_iter)
    bg, Z, nodes = 1, 384, 37
    K = BG_K[bg] * Z
    nb = K // 8
    poly, kinds = input_kinds(bg, Z, rng, nodes * Z)
    _, more = input_kinds(bg, Z, rng, nodes * Z)
    base = [k for k in kinds + more if k[1] == 0][:6] + [kinds[3], more[3]]  # (the two with fillers last)
    n = 640
    descs = np.zeros(n, dtype=miphy.LdpcDecDesc)
    for i in range(n):
        descs[i] = (bg, miphy.CRC24B, Z, max_iter, base[i % 8][1], nodes * Z, 0, (i % 8) * nodes * Z, i * nb)
    llr_d = torch.from_numpy(np.concatenate([b[0] for b in base])).cuda()
    exp = [o_ldpc_decode(bg, Z, llr, nf, CRC24B, max_iter, out_init=np.full(nb, 0x5A, dtype=np.uint8)) for llr, nf in base]
    try:
        for mode in (0, 0x100):
            force_kernel(mode)
            out_d = torch.full((n * nb,), 0x5A, dtype=torch.uint8, device="cuda")
            it_d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            ctx.ldpc_decode_batch(descs, llr_d, out_d, it_d)
            torch.cuda.synchronize()
            used = kernels_used()
            assert used & PACKED and used & GMSG and not used & (SPLIT | SCALAR | WAVE), (mode, used)
            assert bool(used & GMSG_PART) == (mode == 0), (mode, used)
            out, its = out_d.cpu().numpy().reshape(n, nb), it_d.cpu().numpy()
            for i in range(n):
                assert its[i] == exp[i % 8][0] and np.array_equal(out[i], exp[i % 8][1]), (mode, i, int(its[i]), exp[i % 8][0])
    finally:
        force_kernel(0)


PLAN_TBS = {1: (4, 106, 42016, (0.45, 0.6)), 2: (2, 100, 9984, (0.75, 1.2))}  # base graph: modulation, PRBs, TB bits, noise of the two TBs


@pytest.mark.parametrize("max_iter", [2, 6])
@pytest.mark.parametrize("bg", [1, 2])
@pytest.mark.parametrize("form", ["auto", "throughput"])
def test_first_iteration_in_a_prepared_pusch_plan(ctx, form, bg, max_iter):
    """Two first transmissions of a few codeblocks each through a prepared plan, where the packed kernel dematches while it loads (latency
    form for so few codeblocks, throughput form when forced): transport blocks, CRC flags, result records and soft buffers as the oracle
    chain; the same plan run on other soft bits and then on the first ones again gives the first results again -- nothing depends on
    message memory a previous codeblock left behind."""
    import torch
    import miphy
    rng = np.random.default_rng(400 + 10 * bg + max_iter)
    mod, nprb, tbs_bits, sigmas = PLAN_TBS[bg]
    nsym = nprb * 156
    seg = o_segmentation(tbs_bits, bg, mod, 1, nsym)
    assert seg.Z >= 128 and seg.Z % 16 == 0 and 2 <= seg.nof_cbs <= 8
    tbs = [rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8) for _ in sigmas]
    cws = [o_pdsch_encode(bg, 0, mod, 0, 1, nsym, tb) for tb in tbs]
    ncb, N, E = seg.nof_cbs, seg.N, cws[0].size

    def noisy(scale):
        return [np.round(np.clip(4 * ((1.0 - 2.0 * (cw & 1)) + scale * s * rng.standard_normal(E)), -20, 20) / 20 * 120).astype(np.int8)
                for cw, s in zip(cws, sigmas)]

    first, other = noisy(1.0), noisy(1.3)
    d = np.zeros(2, dtype=miphy.PuschTbDesc)
    for i in range(2):
        d[i] = (bg, 0, mod, 1, 1, 1, max_iter, 0, nsym, tbs_bits // 8, i * ncb, i * E, i * (tbs_bits // 8))
    soft_d = torch.full((2 * ncb * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(2 * ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(2 * ncb, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(2 * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    tb_d = torch.zeros(2 * (tbs_bits // 8), dtype=torch.uint8, device="cuda")
    force_kernel(MODES[form])
    plan = None
    try:
        plan = ctx.pusch_decode_plan(d)

        def run(llrs):
            tb_d.fill_(0xEE)
            plan.run(torch.from_numpy(np.concatenate(llrs)).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
            torch.cuda.synchronize()
            return (res_d.cpu().numpy().view(miphy.PuschResult).copy(), tb_d.cpu().numpy().reshape(2, -1).copy(), crc_d.cpu().numpy().copy(),
                    soft_d.cpu().numpy().reshape(2 * ncb, miphy.HARQ_CB_STRIDE)[:, :N].copy())

        res, tb_out, crc, soft = run(first)
        used = kernels_used()
        assert used == (PACKED | FUSED | (SPLIT if form == "auto" else 0) | (used & (GMSG | GMSG_PART))), used
        for i in range(2):
            od = OraclePuschDecoder(bg, mod, 0, 1, nsym, tbs_bits // 8)
            od.softbuf[:] = 33
            ok, tbo, mm = od.decode(first[i], 0, True, max_iter, True)
            key = (i, ok, mm)
            assert bool(res[i]["tb_crc_ok"]) == ok and res[i]["nof_codeblocks_total"] == ncb, (key, res[i])
            assert (int(res[i]["iters_min"]), int(res[i]["iters_max"])) == mm, (key, res[i])
            assert np.array_equal(crc[i * ncb:(i + 1) * ncb], od.cb_crc), (key, crc)
            assert np.array_equal(soft[i * ncb:(i + 1) * ncb], od.softbuf.reshape(ncb, N)), key
            if ok:
                assert np.array_equal(tb_out[i], tbo) and np.array_equal(tb_out[i], tbs[i]), key
            elif not np.all(od.cb_crc):
                assert np.all(tb_out[i] == 0xEE), key
        run(other)
        again = run(first)
        for a, b in zip((res, tb_out, crc, soft), again):
            assert np.array_equal(a, b)
    finally:
        force_kernel(0)
        if plan is not None:
            plan.close()
