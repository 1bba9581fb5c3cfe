"""GPU: transport-block assembly (pusch_tb_assemble_kernel: codeblock payloads to their place in the transport block, TB CRC24A from
per-codeblock parts, result record, flag reset on a TB CRC failure) against the CPU oracle, bit for bit, over every lifting size
whole-byte transport blocks can reach, every class of codeblock payload length modulo 32 and codeblock count, every destination
alignment, both launch forms (1024 and 512 threads), transport blocks whose CRC fails although every codeblock CRC passes
(tests/sch_tx.py), partly decoded transport blocks over three transmissions, and the sizes the decode refuses.

Every transport block sits behind guard bytes of 0xEE in an output buffer pre-filled with 0xEE, the soft buffers start as stale 33,
the result records as 0x55 and the codeblock flags as 1. The oracle's behaviour these tests lean on is pinned to the reference in
tests/test_oracle_vs_ref.py::test_sch_chain_sizes_and_tb_crc_failure."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import o_ldpc_decode, o_pdsch_encode, o_segmentation
from sch_tx import cb_payload_range, sch_codeword

pytestmark = pytest.mark.gpu

MAX_TB_BYTES = {1: 54753, 2: 24801}  # 52 codeblocks


def noisy(cw, sigma, rng):  # as tests/test_sch_gpu.py
    y = (1.0 - 2.0 * (cw & 1)) + sigma * rng.standard_normal(cw.size)
    return np.round(np.clip(4 * y, -20, 20) / 20 * 120).astype(np.int8)


def clean(cw, amp):
    return ((1 - 2 * cw.astype(np.int16)) * amp).astype(np.int8)


def pick_nsym(ncb, tb_bytes, mod, nl):
    """About rate 1/2; with several codeblocks the symbols per layer do not divide by them (short and long segments)."""
    per_layer = (2 * (tb_bytes * 8 + 24) + mod * nl - 1) // (mod * nl)
    while ncb > 1 and per_layer % ncb == 0:
        per_layer += 1
    return per_layer * nl


class Tx:
    """One transport block on the air and the oracle's HARQ state for it. Several placements in a batch may share one Tx (same
    LLRs, HARQ slots of their own): the oracle then runs once for all of them."""

    def __init__(self, bg, mod, nl, nbytes, nsym=None):
        seg0 = o_segmentation(nbytes * 8, bg, 1, 1, 1000)
        self.bg, self.mod, self.nl, self.nbytes = bg, mod, nl, nbytes
        self.nsym = nsym if nsym else pick_nsym(seg0.nof_cbs, nbytes, mod, nl)
        self.od = O.OraclePuschDecoder(bg, mod, 0, nl, self.nsym, nbytes)
        self.od.softbuf[:] = 33  # the same stale garbage as the device buffers
        self.seg, self.ncb = self.od.seg, self.od.seg.nof_cbs
        if self.ncb > 1:
            assert (self.nsym // nl) % self.ncb != 0
        self.llr, self.exp = None, None

    def key(self):
        return (self.bg, self.nbytes, self.ncb, self.seg.Z, self.mod, self.nl)

    def oracle_step(self, rv, new_data, max_iter, early_stop):
        """orc_pusch_decode with the output pre-filled with 0xEE (so 'not written' shows), plus what the result record adds to it."""
        od, s = self.od, self.seg
        pre = np.zeros(self.ncb, np.uint8) if new_data else od.cb_crc.copy()
        tb = np.full(self.nbytes, 0xEE, np.uint8)
        mm = (C.c_int * 2)()
        ok = O.oracle().orc_pusch_decode(self.bg, rv, self.mod, C.c_uint(0), C.c_uint(self.nl), C.c_uint(self.nsym), C.c_uint(self.nbytes),
                                         int(new_data), O._p(self.llr), C.c_uint(max_iter), int(early_stop), O._p(od.softbuf), O._p(od.cb_crc),
                                         O._p(od.cb_msgs), O._p(tb), mm)
        assert ok >= 0
        decoded = np.nonzero(pre == 0)[0]
        if decoded.size == 0:
            mean = np.float32(0)
        elif mm[0] == mm[1]:
            mean = np.float32(mm[0])
        else:  # per-codeblock counts the way orc_pusch_decode takes them: the decoder on the soft buffer the dematcher left
            soft = od.softbuf.reshape(self.ncb, s.N)
            its = [o_ldpc_decode(self.bg, s.Z, soft[c], s.nof_filler_bits, s.crc_poly if early_stop else -1, max_iter)[0] for c in decoded]
            its = [it if (it and early_stop) else max_iter for it in its]
            assert (min(its), max(its)) == (mm[0], mm[1])
            mean = np.float32(sum(its)) / np.float32(len(its))
        self.exp = dict(ok=bool(ok), tb=tb, mm=(mm[0], mm[1]), nof_decoded=int(decoded.size), mean=mean, flags=od.cb_crc.copy(),
                        part=0 < int(od.cb_crc.sum()) < self.ncb)
        return self.exp


class Batch:
    """Placements of Tx objects with HARQ slots and device HARQ state that lasts over the steps of a test."""

    def __init__(self, txs, aligns=None):
        import torch
        import miphy
        self.txs = txs
        self.aligns = aligns if aligns is not None else [None] * len(txs)
        self.slots, n = [], 0
        for tx in txs:
            self.slots.append(n)
            n += tx.ncb
        self.nslots = n
        self.soft_d = torch.full((n * miphy.HARQ_CB_STRIDE,), 33, dtype=torch.int8, device="cuda")
        self.msgs_d = torch.zeros(n * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
        self.crc_d = torch.ones(n, dtype=torch.uint8, device="cuda")

    def descs(self, rv, new_data, early_stop, max_iter):
        import miphy
        d = np.zeros(len(self.txs), dtype=miphy.PuschTbDesc)
        llr_off, pos = 0, 0
        for i, tx in enumerate(self.txs):
            if self.aligns[i] is None:
                tb_off = pos + 1 + i % 3  # 1-3 guard bytes
            else:
                tb_off = pos + 1 + (self.aligns[i] - pos - 1) % 4  # 1-4 guard bytes, the offset (and the address) at the wanted residue
                assert tb_off % 4 == self.aligns[i]
            llr_off += i % 3
            d[i] = (tx.bg, rv, tx.mod, tx.nl, new_data, early_stop, max_iter, 0, tx.nsym, tx.nbytes, self.slots[i], llr_off, tb_off)
            llr_off += tx.nsym * tx.mod
            pos = tb_off + tx.nbytes
        return d, llr_off, pos + 3

    def step(self, ctx, rv, new_data, early_stop=1, max_iter=6, run_oracle=True, plan=False):
        """One decode call compared with the oracle. Returns the launch form the assembly kernel took (its threads)."""
        import torch
        import miphy
        d, llr_len, tb_len = self.descs(rv, new_data, early_stop, max_iter)
        llr = np.zeros(llr_len, np.int8)
        for i, tx in enumerate(self.txs):
            o = int(d[i]["llr_offset"])
            llr[o:o + tx.llr.size] = tx.llr
        tb_d = torch.full((tb_len,), 0xEE, dtype=torch.uint8, device="cuda")
        assert tb_d.data_ptr() % 4 == 0
        res_d = torch.full((len(self.txs) * miphy.PuschResult.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        llr_d = torch.from_numpy(llr).cuda()
        if plan:
            p = ctx.pusch_decode_plan(d)
            try:
                p.run(llr_d, self.soft_d, self.msgs_d, self.crc_d, tb_d, res_d)
                torch.cuda.synchronize()
            finally:
                p.close()
        else:
            ctx.pusch_decode_batch(d, llr_d, self.soft_d, self.msgs_d, self.crc_d, tb_d, res_d)
            torch.cuda.synchronize()
        res = res_d.cpu().numpy().view(miphy.PuschResult)
        tb_out, flags = tb_d.cpu().numpy(), self.crc_d.cpu().numpy()
        if run_oracle:
            for tx in {id(t): t for t in self.txs}.values():
                tx.oracle_step(rv, new_data, max_iter, bool(early_stop))
        exp_tb = np.full(tb_len, 0xEE, np.uint8)
        for i, tx in enumerate(self.txs):
            e, r, key = tx.exp, res[i], (i, tx.key(), rv, new_data, early_stop, max_iter)
            assert bool(r["tb_crc_ok"]) == e["ok"] and int(r["tb_crc_ok"]) in (0, 1), (key, r)
            assert r["nof_codeblocks_total"] == tx.ncb, (key, r)
            assert (int(r["iters_min"]), int(r["iters_max"])) == e["mm"], (key, r, e["mm"])
            assert int(r["nof_decoded"]) == e["nof_decoded"], (key, r, e["nof_decoded"])
            assert np.float32(r["iters_mean"]) == e["mean"], (key, r, e["mean"])
            assert np.array_equal(flags[self.slots[i]:self.slots[i] + tx.ncb], e["flags"]), (key, flags[self.slots[i]:self.slots[i] + tx.ncb], e["flags"])
            o = int(d[i]["tb_offset"])
            exp_tb[o:o + tx.nbytes] = e["tb"]
            bad = np.nonzero(tb_out[o:o + tx.nbytes] != e["tb"])[0]
            assert bad.size == 0, (key, "transport block bytes", bad[:8], tb_out[o + bad[:8]], e["tb"][bad[:8]])
        bad = np.nonzero(tb_out != exp_tb)[0]
        assert bad.size == 0, ("guard bytes", bad[:8], tb_out[bad[:8]])
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        return 1024 if len(self.txs) * 4 <= cus else 512


def reachable_lifting_sizes():
    """(base graph, lifting size) pairs of whole-byte transport blocks, from the rule (TS 38.212 5.2.2): B = 8 n + 16 up to 3824
    bits and 8 n + 24 above; one codeblock up to Kcb, else ceil(B / (Kcb - 24)) of them with 24 CRC bits each; the smallest Z with
    Kb Z >= B' / C."""
    out = set()
    for bg in (1, 2):
        kcb = 8448 if bg == 1 else 3840
        for n in range(1, MAX_TB_BYTES[bg] + 1):
            b = 8 * n + (16 if 8 * n <= 3824 else 24)
            c = 1 if b <= kcb else -(-b // (kcb - 24))
            kb = 22 if bg == 1 else (10 if b > 640 else 9 if b > 560 else 8 if b > 192 else 6)
            per_cb = -(-(b + (24 * c if c > 1 else 0)) // c)
            out.add((bg, min(z for z in O.ALL_Z if kb * z >= per_cb)))
    return out


def expect_rejected(ctx, bg, nbytes, text, nsym=None, mod=2):
    import torch
    import miphy
    d = np.zeros(1, dtype=miphy.PuschTbDesc)
    d[0] = (bg, 0, mod, 1, 1, 1, 6, 0, nsym if nsym else 8 * max(nbytes, 1), nbytes, 0, 0, 0)
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=text):
        ctx.pusch_decode_batch(d, z.view(torch.int8), z.view(torch.int8), z, z, z, z)
    with pytest.raises(RuntimeError, match=text):
        ctx.pusch_decode_plan(d)


BOUNDARY_BITS = (8, 24, 176, 184, 544, 552, 624, 632, 3816, 3824, 3832, 3840, 3848, 8416, 8424, 8440)


def test_every_reachable_lifting_size(ctx):
    """The smallest transport block of every (base graph, lifting size) whole-byte sizes can reach, and the sizes around every
    switch of the segmentation (Kb of base graph 2, CRC16 / CRC24A, one / two / three codeblocks): segmentation as the oracle's, and a
    noise-free decode equal to the oracle's in every field. Sizes whose codeblock payloads are not whole bytes are refused."""
    import miphy
    rng = np.random.default_rng(201)
    first = {}
    for bg in (1, 2):
        for n in range(1, MAX_TB_BYTES[bg] + 1):
            first.setdefault((bg, o_segmentation(n * 8, bg, 1, 1, 1000).Z), n)
    want = reachable_lifting_sizes()
    assert set(first) == want and len(want) == 97
    assert {z for z in O.ALL_Z if (1, z) not in want} == set() and {z for z in O.ALL_Z if (2, z) not in want} == {2, 3, 5, 9, 13}
    sizes = sorted((bg, n) for (bg, z), n in first.items())
    sizes += [(bg, bits // 8) for bg in (1, 2) for bits in BOUNDARY_BITS if (bg, bits // 8) not in sizes]
    txs, refused = [], []
    for i, (bg, nbytes) in enumerate(sizes):
        seg, got = o_segmentation(nbytes * 8, bg, 1, 1, 1000), miphy.sch_segmentation(nbytes, bg)
        for f in ("nof_cbs", "Z", "K", "N", "nof_filler_bits", "nof_tb_crc_bits", "nof_cb_crc_bits", "cb_info_bits", "zero_pad"):
            assert getattr(got, f) == getattr(seg, f), (bg, nbytes, f)
        if seg.nof_cbs > 1 and seg.cb_info_bits % 8:
            refused.append((bg, nbytes))
            continue
        tx = Tx(bg, (1, 2, 4, 6, 8)[i % 5], 1 + (i // 5) % 4, nbytes)
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        tx.llr = clean(o_pdsch_encode(bg, 0, tx.mod, 0, tx.nl, tx.nsym, tb), int(rng.integers(20, 101)))
        tx.tb = tb
        txs.append(tx)
    assert sorted(refused) == [(2, 3840 // 8), (2, 8416 // 8), (2, 8440 // 8)], refused
    assert {(t.bg, t.seg.Z) for t in txs} == want
    assert {(t.bg, t.ncb) for t in txs} >= {(1, 1), (1, 2), (2, 1), (2, 2), (2, 3)}
    assert {t.mod for t in txs} == {1, 2, 4, 6, 8} and {t.nl for t in txs} == {1, 2, 3, 4}
    for bg, nbytes in refused:
        expect_rejected(ctx, bg, nbytes, "not a TS 38.214")
    b = Batch(txs)
    b.step(ctx, 0, 1)
    for tx in txs:  # the oracle decodes every one of them, so the copy and the checksum ran for all
        assert tx.exp["ok"] and np.array_equal(tx.exp["tb"], tx.tb), tx.key()


def assembly_class_sizes():
    """The smallest byte-aligned multi-codeblock size of every (base graph, cb_info_bits mod 32, codeblock count range), the
    two sizes whose last codeblock is a byte short (zero_pad = 8) and the two largest sizes (52 codeblocks)."""
    cls = {}
    for bg in (1, 2):
        for n in range(1, MAX_TB_BYTES[bg] + 1):
            s = o_segmentation(n * 8, bg, 1, 1, 1000)
            if s.nof_cbs > 1 and s.cb_info_bits % 8 == 0:
                cls.setdefault((bg, s.cb_info_bits % 32, 0 if s.nof_cbs <= 8 else 1 if s.nof_cbs <= 16 else 2), n)
    assert set(cls) == {(bg, m, r) for bg in (1, 2) for m in (0, 8, 16, 24) for r in (0, 1, 2)}
    extra = [(1, 8429), (2, 3821), (1, MAX_TB_BYTES[1]), (2, MAX_TB_BYTES[2])]
    for bg, n in extra[:2]:
        s = o_segmentation(n * 8, bg, 1, 1, 1000)
        assert (s.nof_cbs, s.zero_pad) == (9, 8)
    for bg, n in extra[2:]:
        assert o_segmentation(n * 8, bg, 1, 1, 1000).nof_cbs == 52
    sizes = sorted((k[0], n) for k, n in cls.items())
    return sizes + [x for x in extra if x not in sizes], len(cls)


def test_assembly_classes_alignments_and_launch_forms(ctx):
    """Every class of last-word mask (codeblock payload bits mod 32) and codeblock count, at transport-block addresses congruent to
    0, 1, 2 and 3 modulo 4: each alignment as a batch of its own (1024 threads per transport block), one of them again through a
    prepared plan, then all of them in one batch (512 threads, up to seven turns of the eight wavefronts over 52 codeblocks)."""
    import torch
    rng = np.random.default_rng(202)
    sizes, ncls = assembly_class_sizes()
    assert ncls == 24 and len(sizes) == 26  # the two zero_pad = 8 sizes are the smallest of their classes as well
    txs = []
    for i, (bg, nbytes) in enumerate(sizes):
        tx = Tx(bg, (2, 4, 6, 8, 1)[i % 5], 1 + i % 4, nbytes)
        tx.tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        tx.llr = clean(o_pdsch_encode(bg, 0, tx.mod, 0, tx.nl, tx.nsym, tx.tb), int(rng.integers(20, 101)))
        txs.append(tx)
    assert {(t.bg, t.seg.cb_info_bits % 32) for t in txs} == {(bg, m) for bg in (1, 2) for m in (0, 8, 16, 24)}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    forms = []
    for a in range(4):
        assert len(txs) * 4 <= cus
        forms.append(Batch(txs, [a] * len(txs)).step(ctx, 0, 1, run_oracle=(a == 0)))
        if a == 0:
            for tx in txs:
                assert tx.exp["ok"] and np.array_equal(tx.exp["tb"], tx.tb), tx.key()
    forms.append(Batch(txs, [3] * len(txs)).step(ctx, 0, 1, run_oracle=False, plan=True))
    assert forms == [1024] * 5
    every, aligns = txs * 4, [a for a in range(4) for _ in txs]
    if len(every) * 4 <= cus:  # a part with more compute units: one-codeblock transport blocks until the batch takes the other form
        pad = Tx(1, 2, 1, 100)
        pad.tb = rng.integers(0, 256, 100, dtype=np.uint8)
        pad.llr = clean(o_pdsch_encode(1, 0, 2, 0, 1, pad.nsym, pad.tb), 50)
        pad.oracle_step(0, 1, 6, True)
        extra = cus // 4 + 1 - len(every)
        every, aligns = every + [pad] * extra, aligns + [None] * extra
    assert len(every) * 4 > cus
    assert Batch(every, aligns).step(ctx, 0, 1, run_oracle=False) == 512
    print("launch forms: alignment batches and plan %s, whole batch 512 (%d transport blocks, %d compute units)" % (forms, len(every), cus))


TB_CRC_SIZES = {1: ((2106, 3), (8429, 9), (16859, 17)), 2: ((954, 3), (3821, 9), (7630, 17))}


@pytest.mark.parametrize("bg", [1, 2])
def test_tb_checksum_sees_every_codeblock(ctx, bg):
    """One transport block per codeblock index with a single payload bit flipped inside that codeblock (first, middle, last bit in
    rotation) and one with only the TB CRC changed, all behind valid codeblock CRCs, between intact transport blocks of the same sizes:
    the corrupted ones report a failed TB CRC with their bytes written, all their flags cleared, every codeblock decoded; a
    retransmission decodes all of them again (the flags were reset) and fails again; new data then decodes. A single-codeblock transport
    block with a wrong CRC16 or CRC24A fails in the decoder itself and nothing is written."""
    rng = np.random.default_rng(203 + bg)
    txs, bad = [], []
    for nbytes, ncb in TB_CRC_SIZES[bg]:
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        good = Tx(bg, 4, 1, nbytes)
        assert good.ncb == ncb
        good.cws = {rv: o_pdsch_encode(bg, rv, 4, 0, 1, good.nsym, tb) for rv in (0, 2)}
        good.tb, good.amp = tb, int(rng.integers(20, 101))
        kinds = [dict(tb_crc_flip=1 << int(rng.integers(0, 24)))]
        for c in range(ncb):
            lo, hi = cb_payload_range(good.seg, c)
            kinds.append(dict(flip_bits=[(lo, (lo + hi) // 2, hi)[c % 3]]))
        for kw in kinds:
            tx = Tx(bg, 4, 1, nbytes, good.nsym)
            tx.cws = {}
            for rv in (0, 2):
                tx.cws[rv], tx.payload = sch_codeword(bg, rv, 4, 0, 1, tx.nsym, tb, **kw)
            tx.tb, tx.amp = tb, int(rng.integers(20, 101))
            txs += [tx, good]
            bad.append(tx)
    single = []
    # CRC16 and CRC24A (base graph 2 has no single codeblock above 3824 bits: its largest CRC16 size instead)
    for nbytes, flip, ncrc in ((100, 0x8001, 16), (600, 0x800001, 24) if bg == 1 else (478, 0x4, 16)):
        tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
        tx = Tx(bg, 2, 1, nbytes)
        assert tx.ncb == 1 and tx.seg.nof_tb_crc_bits == ncrc
        tx.cws = {rv: sch_codeword(bg, rv, 2, 0, 1, tx.nsym, tb, tb_crc_flip=flip)[0] for rv in (0, 2)}
        tx.tb, tx.amp = tb, 60
        txs.append(tx)
        single.append(tx)
    intact = [t for t in txs if t not in bad and t not in single]
    b = Batch(txs)
    for step, (rv, new_data) in enumerate(((0, 1), (2, 0), (0, 1))):
        for tx in set(txs):
            tx.llr = clean(tx.cws[rv] if step < 2 else o_pdsch_encode(bg, 0, tx.mod, 0, 1, tx.nsym, tx.tb), tx.amp)
        b.step(ctx, rv, new_data)
        for tx in bad:
            e = tx.exp
            if step < 2:
                assert not e["ok"] and e["nof_decoded"] == tx.ncb and not e["flags"].any() and np.array_equal(e["tb"], tx.payload), (step, tx.key())
            else:
                assert e["ok"] and e["flags"].all() and np.array_equal(e["tb"], tx.tb), (step, tx.key())
        for tx in intact:
            assert tx.exp["ok"] and tx.exp["flags"].all() and tx.exp["nof_decoded"] == (0 if step == 1 else tx.ncb), (step, tx.key())
        for tx in single:
            e = tx.exp
            if step < 2:
                assert not e["ok"] and np.all(e["tb"] == 0xEE) and e["nof_decoded"] == 1 and e["mm"] == (6, 6), (step, tx.key())
            else:
                assert e["ok"] and np.array_equal(e["tb"], tx.tb), (step, tx.key())


PARTLY_SIGMAS = {6: (0.74, 0.78, 0.82), 2: (0.58, 0.62, 0.66)}  # per nof_ldpc_iterations


@pytest.mark.parametrize("early_stop,max_iter", [(1, 6), (0, 6), (1, 2), (0, 2)])
def test_partly_decoded_transport_blocks(ctx, early_stop, max_iter):
    """Noisy first transmissions after which some codeblocks of a transport block pass and others do not, then rv 2 and rv 3: the
    codeblocks already decoded are skipped (nof_decoded < C) and the mean takes the counts of the others only."""
    rng = np.random.default_rng(204 + 10 * early_stop + max_iter)
    txs = []
    for bg, nbytes, mod in ((1, 4212, 4), (1, 8429, 6), (2, 954, 2), (2, 7630, 2), (1, 300, 2)):
        for sigma in PARTLY_SIGMAS[max_iter]:
            tx = Tx(bg, mod, 1, nbytes)
            tx.tb = rng.integers(0, 256, nbytes, dtype=np.uint8)
            tx.llrs = [noisy(o_pdsch_encode(bg, rv, mod, 0, 1, tx.nsym, tx.tb), sigma, rng) for rv in (0, 2, 3)]
            txs.append(tx)
    b = Batch(txs)
    seen = set()
    for step, rv in enumerate((0, 2, 3)):
        for tx in txs:
            tx.llr = tx.llrs[step]
        b.step(ctx, rv, int(step == 0), early_stop, max_iter)
        if step == 0:
            assert sum(tx.exp["part"] for tx in txs) >= 2, [(tx.key(), tx.exp["flags"].sum()) for tx in txs]
        else:
            seen |= {"skipped" for tx in txs if 0 < tx.exp["nof_decoded"] < tx.ncb}
        seen |= {"mean" for tx in txs if tx.exp["mm"][0] != tx.exp["mm"][1]}
        seen |= {"ok" for tx in txs if tx.exp["ok"]} | {"fail" for tx in txs if not tx.exp["ok"]}
    assert seen >= {"skipped", "ok", "fail"} and (not early_stop or "mean" in seen), seen



def test_sizes_the_decode_refuses(ctx):
    rng = np.random.default_rng(205)
    expect_rejected(ctx, 1, MAX_TB_BYTES[1] + 1, "exceed MAX_NOF_SEGMENTS")
    expect_rejected(ctx, 2, MAX_TB_BYTES[2] + 1, "exceed MAX_NOF_SEGMENTS")
    expect_rejected(ctx, 1, 5000, "not a TS 38.214")
    expect_rejected(ctx, 1, 0, "out of range")
    expect_rejected(ctx, 2, 0, "out of range")
    tx = Tx(2, 2, 1, 479)  # the context still decodes
    tx.tb = rng.integers(0, 256, 479, dtype=np.uint8)
    tx.llr = clean(o_pdsch_encode(2, 0, 2, 0, 1, tx.nsym, tx.tb), 40)
    Batch([tx]).step(ctx, 0, 1)
    assert tx.exp["ok"] and np.array_equal(tx.exp["tb"], tx.tb)
