"""GPU: the phases of an LDPC decode around the layer loop -- the load that dematches (csrc/rdm_device.h stage_vector, csrc/ldpc_decode_pk.hip
pk_fused_load), the HARQ image and the search for the last non-zero soft bit (pk_fused_image_out), the hard decision shared by the checksum
and the output (csrc/ldpc_pk_device.h hard_word, crc_zmask_partial, store_hard_words / store_kept_words) -- against the CPU oracle.

Hard bits and checksum: codeblocks of plain soft bits through miphy_ldpc_decode_batch, one, two and three wavefronts per codeblock of the
packed kernel (Z = 72 / 88 on base graph 1 and 104 on base graph 2 have a K that is no multiple of 32), the wave kernel at Z = 64 (two
codeblocks per wavefront: the second one sits at a non-zero group base), and the one-row-per-lane kernel; fillers that put the message length
L = K - F at L mod 32 = 0, 1, 8 and 31; no checksum, CRC16, CRC24A, CRC24B (masks) and CRC24C (division); the verdict taken every
iteration, after the last one only, and never; outputs that start 0, 1, 2 and 3 bytes past a dword; inputs whose soft bits end at exactly 0
(hard bit 1) and at +-127.

Fused load: transport blocks of two or three codeblocks through a PUSCH decode plan, the only way into the instances that dematch while
they load, in the throughput form (with and without the early stop: the instances that keep the checksum's words) and in the latency form.
Modulation orders 1, 2, 4, 6 and 8; E no multiple of 16; a second codeblock that starts 1, 2 and 3 bytes past a dword; even and odd
Kq = E / MOD; fillers with a symbol pair of a bit plane split by the filler gap and not split; the last k soft bits of a codeblock's image
zero for k = 1, 15, 16, 17 and for a k that crosses a multiple of Z (one layer less); an all-zero codeblock. Compared: HARQ soft images
byte for byte, hard bits, CRC flags, iteration counts, transport blocks."""
import functools

import numpy as np
import pytest

from oracle_lib import BG_K, CRC16, CRC24A, CRC24B, CRC24C, OraclePuschDecoder, o_crc_bits, o_ldpc_decode, o_pdsch_encode, o_segmentation
from test_ldpc_decode_gpu import FUSED, PACKED, SCALAR, SPLIT, WAVE, make_codeword, noisy_llr

pytestmark = pytest.mark.gpu

AUTO, ROW_KERNEL, THROUGHPUT = 0, 1, 4  # miphy_debug_force_ldpc_kernel (include/miphy.h)


# ------------------------------------------------------------------------------------------------ hard bits and checksum
def filler_for(K, l_mod_32):
    """The smallest F > 0 with (K - F) mod 32 = l_mod_32."""
    return (K - l_mod_32 - 1) % 32 + 1


@functools.lru_cache(maxsize=None)
def hard_bit_cases(bg, Z):
    """Codeblocks of one lifting size: every filler tail with the mask checksums and the division, every verdict timing, received clean
    (passes at once), noisy (passes late or never), and two inputs that leave soft bits at exactly 0 and at +-127."""
    rng = np.random.default_rng(1000 * bg + Z)
    K = BG_K[bg] * Z
    cases = []

    def add(poly, nf, sigma, flags, max_iter=4):
        _, cw = make_codeword(bg, Z, rng, nf, poly if poly >= 0 else CRC24B)
        llr = noisy_llr(cw[:(BG_K[bg] + 6) * Z], sigma, rng)
        if nf:
            llr[K - 2 * Z - nf:K - 2 * Z] = 127
        cases.append(dict(bg=bg, Z=Z, llr=llr, crc=poly, max_iter=max_iter, nf=nf, flags=flags))

    for k, lm in enumerate((0, 1, 8, 31)):
        nf = filler_for(K, lm)
        assert (K - nf) % 32 == lm and 0 < nf <= 32
        for poly in (CRC24B, CRC24A, CRC16, CRC24C):
            add(poly, nf, (0.25, 0.45, 0.55, 0.40)[(k + poly) % 4], flags=(k + poly) % 2)
    for poly in (CRC24B, CRC16, CRC24C):  # no fillers: the message ends where K ends (a half word for these K)
        add(poly, 0, 0.3, 0)
        add(poly, 0, 0.5, 1)
    add(-1, 0, 0.5, 0)
    add(-1, filler_for(K, 8), 0.9, 0, max_iter=2)
    # soft bits that stay at exactly 0 (two zero inputs in a row void every message of it: most columns never move) next to +-127
    for poly, flags in ((-1, 0), (CRC24B, 1), (CRC24B, 0)):
        n = (BG_K[bg] + 5) * Z
        llr = np.zeros(n, np.int8)
        pick = rng.random(n) < 0.06
        llr[pick] = rng.choice(np.array([-127, 127, -3, 5], np.int8), int(pick.sum()))
        llr[-1] = 5
        cases.append(dict(bg=bg, Z=Z, llr=llr, crc=poly, max_iter=3, nf=0, flags=flags))
    for c in cases:
        c["llr"].setflags(write=False)
        c["expect"] = expected(c)
    return tuple(cases)


def expected(c):
    """(iterations, hard bytes) of the oracle; bytes the decoder must leave alone are 0x5A."""
    K = BG_K[c["bg"]] * c["Z"]
    init = np.full((K + 7) // 8, 0x5A, np.uint8)
    if c["flags"] & 1:  # checksum once after the last iteration (pusch_decoder_impl.cpp:105-118)
        _, oo = o_ldpc_decode(c["bg"], c["Z"], c["llr"], c["nf"], -1, c["max_iter"], out_init=init)
        return (c["max_iter"] if o_crc_bits(c["crc"], np.unpackbits(oo)[:K - c["nf"]]) == 0 else 0), oo
    return o_ldpc_decode(c["bg"], c["Z"], c["llr"], c["nf"], c["crc"], c["max_iter"], out_init=init)


def run_codeblocks(ctx, cases, mode, out_shift):
    """One batch; codeblock i's output starts (out_shift + i) mod 4 bytes past a dword, between guard bytes. Returns (kernels used, mismatches)."""
    import torch
    import miphy
    lib = miphy.lib()
    n = len(cases)
    descs = np.zeros(n, dtype=miphy.LdpcDecDesc)
    llr_off, out_off, outs = 0, 0, []
    for i, c in enumerate(cases):
        nb = (BG_K[c["bg"]] * c["Z"] + 7) // 8
        out_off = (out_off + 3) // 4 * 4 + 4 + (out_shift + i) % 4
        descs[i] = (c["bg"], c["crc"] if c["crc"] >= 0 else miphy.CRC_NONE, c["Z"], c["max_iter"], c["nf"], c["llr"].size, c["flags"], llr_off, out_off)
        outs.append((out_off, nb))
        llr_off += (c["llr"].size + 15) // 16 * 16
        out_off += nb
    llr_h = np.zeros(llr_off, np.int8)
    for i, c in enumerate(cases):
        llr_h[int(descs[i]["llr_offset"]):int(descs[i]["llr_offset"]) + c["llr"].size] = c["llr"]
    out_d = torch.full((out_off + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    it_d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    lib.miphy_debug_force_ldpc_kernel(mode)
    try:
        lib.miphy_debug_ldpc_kernels_used(1)
        ctx.ldpc_decode_batch(descs, torch.from_numpy(llr_h).cuda(), out_d, it_d)
        torch.cuda.synchronize()
        used = int(lib.miphy_debug_ldpc_kernels_used(1))
    finally:
        lib.miphy_debug_force_ldpc_kernel(0)
    out, its = out_d.cpu().numpy(), it_d.cpu().numpy()
    bad, mine = [], np.zeros(out.size, bool)
    for i, (c, (o0, nb)) in enumerate(zip(cases, outs)):
        ito, oo = c["expect"]
        mine[o0:o0 + nb] = True
        if ito != its[i] or not np.array_equal(oo, out[o0:o0 + nb]):
            bad.append((i, c["bg"], c["Z"], c["crc"], c["nf"], c["flags"], o0 % 4, ito, int(its[i]), int(np.sum(oo != out[o0:o0 + nb]))))
    assert np.all(out[~mine] == 0x5A), "bytes between the outputs were written"
    return used, bad


# (base graph, Z): wavefronts per codeblock of the packed kernel 1, 1, 1, 1, 2, 3
PACKED_SIZES = [(1, 72), (1, 88), (2, 104), (1, 128), (1, 192), (1, 384)]


@pytest.mark.parametrize("mode", [THROUGHPUT, AUTO, ROW_KERNEL], ids=["throughput", "latency", "row"])
@pytest.mark.parametrize("bg,Z", PACKED_SIZES)
def test_hard_bits_and_checksum(ctx, bg, Z, mode):
    cases = hard_bit_cases(bg, Z)
    assert (BG_K[bg] * Z) % 32 != 0 or Z >= 128
    for shift in (0, 2):  # with the index of the codeblock: every output alignment meets every kind of codeblock over the two runs
        used, bad = run_codeblocks(ctx, cases, mode, shift)
        print(bg, Z, mode, "kernels used", hex(used))
        if mode == ROW_KERNEL:
            assert used == SCALAR, hex(used)
        else:
            assert used & PACKED and not used & (SCALAR | WAVE) and bool(used & SPLIT) == (mode == AUTO), hex(used)
        assert not bad, bad[:8]


def test_hard_bits_and_checksum_wave_kernel(ctx):
    """Z = 64: two codeblocks per wavefront, the second one behind a non-zero group base."""
    cases = hard_bit_cases(1, 64) + hard_bit_cases(2, 64)
    for shift in (0, 1):
        used, bad = run_codeblocks(ctx, cases, THROUGHPUT, shift)
        assert used & WAVE and not used & (SCALAR | PACKED), hex(used)
        assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------ fused load
BG = 1
# name: (modulation order, TB bits, channel symbols, Z, codeblocks, E per codeblock, fillers, a symbol pair of a plane split by the filler gap)
SHAPES = {
    "bpsk_z256_e1mod4": (1, 10600, 10754, 256, 2, 5377, 296, False),
    "bpsk_z256_e2mod4": (1, 10600, 10756, 256, 2, 5378, 296, False),
    "bpsk_z256_e3mod4": (1, 10600, 10758, 256, 2, 5379, 296, False),
    "bpsk_z384_three": (1, 23160, 24195, 384, 3, 8065, 696, False),
    "bpsk_z256_seven_layers": (1, 10600, 13000, 256, 2, 6500, 296, False),
    "qpsk_z256_odd_kq": (2, 10600, 5378, 256, 2, 5378, 296, True),
    "qpsk_z384_even_kq": (2, 23160, 12096, 384, 3, 8064, 696, False),
    "qam16_z208_odd_kq": (4, 8600, 2186, 208, 2, 4372, 240, True),
    "qam16_z384_even_kq": (4, 23160, 6054, 384, 3, 8072, 696, False),
    "qam64_z256_odd_kq": (6, 10600, 1794, 256, 2, 5382, 296, True),
    "qam64_z384_even_kq": (6, 23160, 4038, 384, 3, 8076, 696, False),
    "qam256_z208_odd_kq_split": (8, 8600, 1094, 208, 2, 4376, 240, True),
    "qam256_z256_odd_kq": (8, 10600, 1382, 256, 2, 5528, 296, False),
    "qam256_z384_odd_kq_split": (8, 23400, 3027, 384, 3, 8072, 616, True),
    "qam256_z384_even_kq": (8, 23160, 3024, 384, 3, 8064, 696, False),
    "qam256_z384_seven_layers": (8, 23160, 3495, 384, 3, 9320, 696, True),
}


def split_planes(mod, Z, E, F):
    """Bit planes in which the filler gap falls between the two symbols of a lane's pair (an odd number of symbols in front of it)."""
    Kq, f0 = E // mod, 20 * Z - F
    return [q for q in range(mod) if 0 < f0 - q * Kq < Kq and (f0 - q * Kq) % 2 == 1]


def segmentation_of(shape):
    mod, tbs_bits, nsym, Z, ncb, E, F, split = SHAPES[shape]
    seg = o_segmentation(tbs_bits, BG, mod, 1, nsym)
    assert (seg.Z, seg.nof_cbs, seg.nof_filler_bits, seg.cb_info_bits % 8) == (Z, ncb, F, 0) and all(seg.E[c] == E for c in range(ncb)), shape
    assert F > 0 and E + F <= seg.N and E >= 20 * Z - F and bool(split_planes(mod, Z, E, F)) == split, shape  # dematched by the decoder; the data crosses the fillers
    return seg


@functools.lru_cache(maxsize=None)
def transport_block(shape, seed, zero_tail=0, tail_cb=0, zero_cb=-1):
    """(TB bytes, LLRs). zero_tail: the last zero_tail soft bits of codeblock tail_cb's IMAGE are not received (bit plane q of symbol p is
    image rank q Kq + p and input byte p MOD + q); zero_cb: a codeblock that is not received at all."""
    mod, tbs_bits, nsym = SHAPES[shape][:3]
    seg = segmentation_of(shape)
    rng = np.random.default_rng(seed)
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
    cw = o_pdsch_encode(BG, 0, mod, 0, 1, nsym, tb)
    # (noise by code rate: the shapes of about 21 columns carry next to no parity; codeblocks that pass early, late and never)
    levels = (0.30, 0.42, 0.36) if seg.E[0] > 24 * seg.Z else (0.10, 0.20, 0.15)
    sig = np.concatenate([np.full(seg.E[c], levels[(c + seed) % 3]) for c in range(seg.nof_cbs)])
    llr = np.round(np.clip(4 * ((1.0 - 2.0 * (cw & 1)) + sig * rng.standard_normal(cw.size)), -20, 20) / 20 * 120).astype(np.int8)
    llr[llr == 0] = 1  # (so that the image ends where the test says it does)
    if zero_tail:
        E, Kq = seg.E[tail_cb], seg.E[tail_cb] // mod
        r = np.arange(E - zero_tail, E)
        llr[seg.cw_offset[tail_cb] + (r % Kq) * mod + r // Kq] = 0
    if zero_cb >= 0:
        llr[seg.cw_offset[zero_cb]:seg.cw_offset[zero_cb] + seg.E[zero_cb]] = 0
    tb.setflags(write=False)
    llr.setflags(write=False)
    return tb, llr


@functools.lru_cache(maxsize=None)
def oracle_of(t, max_iter, early_stop):
    mod, tbs_bits, nsym = SHAPES[t[0]][:3]
    od = OraclePuschDecoder(BG, mod, 0, 1, nsym, tbs_bits // 8)
    od.softbuf[:] = 33
    ok, tbo, mm = od.decode(transport_block(*t)[1], 0, True, max_iter, early_stop)
    return ok, tbo, mm, od.cb_crc.copy(), od.cb_msgs.reshape(od.seg.nof_cbs, -1).copy(), od.softbuf.reshape(od.seg.nof_cbs, -1).copy()


def run_plan(ctx, tbs, max_iter, early_stop, mode, llr_shift=0):
    """tbs: transport_block() argument tuples. TB i's LLRs start llr_shift + i bytes past a multiple of 16. -> kernels used, per TB (result
    record, TB bytes, CRC flags, hard bits, soft images)."""
    import torch
    import miphy
    lib = miphy.lib()
    d = np.zeros(len(tbs), dtype=miphy.PuschTbDesc)
    parts, slot, llr_off, tb_off, where = [], 0, 0, 0, []
    for i, t in enumerate(tbs):
        mod, tbs_bits, nsym, Z, ncb = SHAPES[t[0]][:5]
        llr = transport_block(*t)[1]
        llr_off = (llr_off + 15) // 16 * 16 + (llr_shift + i) % 16
        d[i] = (BG, 0, mod, 1, 1, int(early_stop), max_iter, 0, nsym, tbs_bits // 8, slot, llr_off, tb_off)
        where.append((slot, ncb, tb_off, tbs_bits // 8, 66 * Z, (22 * Z + 7) // 8))
        parts.append((llr_off, llr))
        slot, llr_off, tb_off = slot + ncb, llr_off + llr.size, tb_off + tbs_bits // 8
    llr_h = np.full(llr_off + 16, 77, np.int8)
    for o, l in parts:
        llr_h[o:o + l.size] = l
    soft_d = torch.full((slot * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(slot * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc_d = torch.ones(slot, dtype=torch.uint8, device="cuda")
    res_d = torch.zeros(len(tbs) * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    tb_d = torch.full((tb_off,), 0xEE, dtype=torch.uint8, device="cuda")
    lib.miphy_debug_force_ldpc_kernel(mode)
    plan = None
    try:
        plan = ctx.pusch_decode_plan(d)
        lib.miphy_debug_ldpc_kernels_used(1)
        plan.run(torch.from_numpy(llr_h).cuda(), soft_d, msgs_d, crc_d, tb_d, res_d)
        torch.cuda.synchronize()
        used = int(lib.miphy_debug_ldpc_kernels_used(1))
    finally:
        lib.miphy_debug_force_ldpc_kernel(0)
        if plan is not None:
            plan.close()
    res, tb_out, crc = res_d.cpu().numpy().view(miphy.PuschResult), tb_d.cpu().numpy(), crc_d.cpu().numpy()
    soft, msgs = soft_d.cpu().numpy().reshape(slot, miphy.HARQ_CB_STRIDE), msgs_d.cpu().numpy().reshape(slot, miphy.HARQ_MSG_STRIDE)
    return used, [(res[i], tb_out[o:o + nb], crc[s:s + n], msgs[s:s + n, :kb], soft[s:s + n, :N]) for i, (s, n, o, nb, N, kb) in enumerate(where)]


def check_against_oracle(tbs, got, max_iter, early_stop, what):
    for i, (t, (res, tb_out, crc, msgs, soft)) in enumerate(zip(tbs, got)):
        ok, tbo, mm, e_crc, e_msgs, e_soft = oracle_of(t, max_iter, early_stop)
        key = (what, i, t, ok, mm)
        assert np.array_equal(soft, e_soft), (key, "soft image", int(np.sum(soft != e_soft)))
        assert (int(res["iters_min"]), int(res["iters_max"])) == mm, (key, res)
        assert np.array_equal(crc, e_crc), (key, crc, e_crc)
        assert np.array_equal(msgs, e_msgs), (key, "hard bits", int(np.sum(msgs != e_msgs)))
        assert bool(res["tb_crc_ok"]) == ok and res["nof_codeblocks_total"] == len(e_crc), (key, res)
        if ok:
            assert np.array_equal(tb_out, tbo) and np.array_equal(tb_out, transport_block(*t)[0]), key


def check_forms(ctx, tbs, what, llr_shift=0):
    """The throughput form with the verdict every iteration and after the last one, and the latency form; all dematch while they load."""
    for mode, early_stop in ((THROUGHPUT, True), (THROUGHPUT, False), (AUTO, True)):
        used, got = run_plan(ctx, tbs, 4, early_stop, mode, llr_shift)
        assert used & PACKED and used & FUSED and not used & (SCALAR | WAVE) and bool(used & SPLIT) == (mode == AUTO), (what, hex(used))
        check_against_oracle(tbs, got, 4, early_stop, (what, mode, early_stop))
    return got


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_load_shapes(ctx, shape):
    """Every modulation order, odd and even Kq, E that is no multiple of 16, fillers split and not split across a symbol pair; the
    transport block twice, so that every codeblock's input meets two alignments (the second TB starts one byte further)."""
    mod, _, _, Z, ncb, E, F, _ = SHAPES[shape]
    tbs = ((shape, 7), (shape, 8))
    for shift in ((0, 2) if mod == 1 else (0,)):
        check_forms(ctx, tbs, shape, shift)


def test_fused_load_input_alignments_and_lengths():
    """What the shapes are chosen for, said by the table itself (no device)."""
    s = {k: v for k, v in SHAPES.items()}
    assert {v[0] for v in s.values()} == {1, 2, 4, 6, 8}
    assert {s[k][5] % 4 for k in ("bpsk_z256_e1mod4", "bpsk_z256_e2mod4", "bpsk_z256_e3mod4")} == {1, 2, 3}  # the second codeblock's first byte
    assert any(v[5] % 16 for v in s.values()) and any(v[5] % 16 == 0 for v in s.values())
    for mod in (2, 4, 6, 8):
        assert {(v[5] // v[0]) % 2 for v in s.values() if v[0] == mod} == {0, 1}, mod
    assert {v[7] for v in s.values() if v[0] == 8} == {True, False}
    for k in s:
        segmentation_of(k)



@pytest.mark.parametrize("shape", ["bpsk_z256_seven_layers", "qam256_z384_seven_layers"])
def test_zero_tails(ctx, shape):
    """The last k soft bits of a codeblock's image not received: k = 1, 15, 16, 17 (around a 16-byte vector) and a k that takes the end of
    the data below a multiple of Z, which lowers the number of layers; one codeblock all zero."""
    mod, _, _, Z, ncb, E, F, _ = SHAPES[shape]
    cross = (E + F) % Z + 3
    assert (E + F - cross + 2 * Z + Z - 1) // Z < (E + F + 2 * Z + Z - 1) // Z and (E + F + Z - 1) // Z > 24  # fewer variable nodes, above the minimum of four layers
    tbs = tuple((shape, 20 + k, k, i % ncb) for i, k in enumerate((1, 15, 16, 17, cross))) + ((shape, 30, 0, 0, 1),)
    got = check_forms(ctx, tbs, shape)
    assert got[-1][2].tolist()[1] == 0 and not got[-1][0]["tb_crc_ok"]
    e = oracle_of(tbs[4], 4, True)[5]
    assert not e[4 % ncb, E + F - cross:].any() and e[4 % ncb, E + F - cross - 1] != 0
