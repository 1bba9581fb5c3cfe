"""GPU: miphy_uci_polar_decode_batch (polar-coded UCI fields of 12 to 1706 bits) against the restatement of tests/uci_polar.py, that is
the oracle's polar receive chain per segment inside the TS 38.212 framing: payload bits and verdict bit for bit on every input, the
ones whose CRC fails included (the payload is then the decoder's wrong bits)."""
import ctypes as C
import functools

import numpy as np
import pytest

import uci_polar as U

pytestmark = pytest.mark.gpu

SHAPES = [(12, 32), (13, 240), (19, 215), (19, 216), (20, 40), (20, 8192), (31, 64), (64, 128), (100, 300), (359, 2000), (360, 1087), (360, 1088),
          (361, 1089), (500, 1100), (1012, 1087), (1012, 8192), (1013, 1200), (1705, 3500), (1706, 16384), (1706, 1760)]
SIGMAS = (0.0, 0.5, 0.9, 1.3)
SENTINEL = 0xA5
LLR_SCALE = 32  # soft bit = 32 y for y = +-1 + noise, clipped to +-120


def _soft(rng, tx, sigma):
    y = 1.0 - 2.0 * tx.astype(np.float64)
    if sigma:
        y = y + sigma * rng.standard_normal(tx.size)
    return np.clip(np.rint(LLR_SCALE * y), -120, 120).astype(np.int8)


def _field(A, E, llr, sent, tag):
    payload, valid = U.decode(A, E, llr)
    return dict(A=A, E=E, llr=llr, sent=sent, payload=payload, status=U.STATUS_VALID if valid else U.STATUS_INVALID, tag=tag, f=U.info(A, E))


@functools.lru_cache(maxsize=None)
def fixed_fields():
    """The fixed shapes with a noise-free and three noisy inputs each, and the two fields with one segment sign-flipped wholesale.
    The verdicts of the restatement alone must cover both outcomes in every (L, C) class before the device is looked at."""
    out = []
    for i, (A, E) in enumerate(SHAPES):
        for j, sigma in enumerate(SIGMAS):
            rng = np.random.default_rng(9000 + 10 * i + j)
            x = rng.integers(0, 2, A).astype(np.uint8)
            out.append(_field(A, E, _soft(rng, U.encode(A, E, x), sigma), x, (A, E, sigma)))
    rng = np.random.default_rng(77)
    A, E = 500, 1100
    f = U.info(A, E)
    for seg in (1, 0):
        x = rng.integers(0, 2, A).astype(np.uint8)
        llr = _soft(rng, U.encode(A, E, x), 0.0)
        llr[seg * f["E_r"]:(seg + 1) * f["E_r"]] *= -1
        out.append(_field(A, E, llr, x, (A, E, "segment %d flipped" % seg)))
    seen = {(c["f"]["L"], c["f"]["C"], c["status"]) for c in out}
    for L, Cs in ((6, 1), (11, 1), (11, 2)):
        assert (L, Cs, U.STATUS_VALID) in seen and (L, Cs, U.STATUS_INVALID) in seen, (L, Cs, sorted(seen))
    for c in out:
        if c["tag"][2] == 0.0:
            assert c["status"] == U.STATUS_VALID and np.array_equal(c["payload"], c["sent"]), c["tag"]
    return out


def _layout(fields):
    """Odd, unaligned soft-bit offsets; payloads five sentinel bytes apart."""
    llr_off, pay_off, lo, po = [], [], 1, 3
    for c in fields:
        llr_off.append(lo)
        pay_off.append(po)
        lo += c["E"] + (2 if (lo + c["E"]) % 2 else 1)  # keeps every offset odd
        po += c["A"] + 5
    return np.array(llr_off, np.int64), np.array(pay_off, np.int64), lo + 8, po + 8


def _jobs(fields, llr_off, pay_off):
    import miphy
    jobs = np.zeros(len(fields), miphy.UciPolarJob)
    jobs["nof_bits"], jobs["nof_llr"] = [c["A"] for c in fields], [c["E"] for c in fields]
    jobs["llr_offset"], jobs["payload_offset"] = llr_off, pay_off
    return jobs


def _run(ctx, fields, unowned=None, one_by_one=False):
    """Payload and status buffers (numpy) after decoding `fields`, in one call or one call per field. unowned: the value of the last
    soft bit of a two-segment field with an odd number of soft bits."""
    import torch
    llr_off, pay_off, nl, npay = _layout(fields)
    assert all(o % 2 == 1 for o in llr_off)
    llr = np.full(nl, 55, np.int8)
    for c, o in zip(fields, llr_off):
        llr[o:o + c["E"]] = c["llr"]
        if unowned is not None and c["f"]["C"] == 2 and c["E"] % 2:
            llr[o + c["E"] - 1] = unowned
    d_llr = torch.from_numpy(llr).cuda()
    d_pay = torch.full((npay,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((len(fields) + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    jobs = _jobs(fields, llr_off, pay_off)
    if one_by_one:
        for i in range(len(fields)):
            ctx.uci_polar_decode_batch(jobs[i:i + 1], d_llr, d_pay, d_st[i:])
    else:
        ctx.uci_polar_decode_batch(jobs, d_llr, d_pay, d_st)
    torch.cuda.synchronize()
    return d_pay.cpu().numpy(), d_st.cpu().numpy(), pay_off


def _check(fields, pay, st, pay_off):
    touched = np.zeros(pay.size, bool)
    for i, (c, o) in enumerate(zip(fields, pay_off)):
        got = pay[o:o + c["A"]]
        assert np.array_equal(got, c["payload"]), (c["tag"], int((got != c["payload"]).sum()))
        assert st[i] == c["status"], (c["tag"], int(st[i]), c["status"])
        touched[o:o + c["A"]] = True
    assert np.all(pay[~touched] == SENTINEL) and np.all(st[len(fields):] == SENTINEL)


def test_fixed_shapes_in_one_call_equal_the_restatement(ctx):
    fields = fixed_fields()
    pay, st, pay_off = _run(ctx, fields)
    _check(fields, pay, st, pay_off)
    flipped = [c for c in fields if isinstance(c["tag"][2], str)]
    for c, seg in zip(flipped, (1, 0)):  # the untouched segment still carries what was sent
        assert c["status"] == U.STATUS_INVALID
        half = c["f"]["A_seg"]
        keep = slice(0, half) if seg == 1 else slice(half, 2 * half)
        assert np.array_equal(c["payload"][keep], c["sent"][keep])


def test_one_field_per_call_gives_the_same_bytes(ctx):
    fields = fixed_fields()
    pay, st, pay_off = _run(ctx, fields)
    pay1, st1, _ = _run(ctx, fields, one_by_one=True)
    assert np.array_equal(pay, pay1) and np.array_equal(st, st1)
    _check(fields, pay1, st1, pay_off)


def test_the_unowned_last_soft_bit_is_never_read(ctx):
    fields = fixed_fields()
    assert sum(1 for c in fields if c["f"]["C"] == 2 and c["E"] % 2) >= 4
    a = _run(ctx, fields, unowned=127)
    b = _run(ctx, fields, unowned=-127)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _check(fields, a[0], a[1], a[2])


def test_small_pieces_give_the_same_bytes(ctx):
    import miphy
    fields = fixed_fields()
    pay, st, pay_off = _run(ctx, fields)
    assert miphy.lib().miphy_debug_uci_polar_pieces() == 1
    try:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(40000)
        pay1, st1, _ = _run(ctx, fields)
        assert miphy.lib().miphy_debug_uci_polar_pieces() >= 5
    finally:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(0)
    assert np.array_equal(pay, pay1) and np.array_equal(st, st1)


@functools.lru_cache(maxsize=None)
def drawn_fields():
    rng = np.random.default_rng(600600)
    out = []
    while len(out) < 600:
        A = int(rng.integers(12, 120)) if rng.random() < 0.5 else int(round(np.exp(rng.uniform(np.log(12), np.log(1706)))))
        E = int(rng.integers(U.min_E(A), 6 * A + 400))
        if U.info(A, E) is None:
            continue
        x = rng.integers(0, 2, A).astype(np.uint8)
        sigma = (0.0, 0.6, 1.0)[len(out) % 3]
        out.append(_field(A, E, _soft(rng, U.encode(A, E, x), sigma), x, (A, E, sigma)))
    assert len({(c["f"]["K_r"], c["f"]["E_r"]) for c in out}) > 256
    assert {c["status"] for c in out} == {U.STATUS_VALID, U.STATUS_INVALID} and {c["f"]["C"] for c in out} == {1, 2}
    return out


def test_600_fields_of_distinct_codes_go_out_in_pieces(ctx):
    import miphy
    fields = drawn_fields()
    pay, st, pay_off = _run(ctx, fields)
    assert miphy.lib().miphy_debug_uci_polar_pieces() > 1  # more than one piece at the default piece size
    _check(fields, pay, st, pay_off)
    pay1, st1, _ = _run(ctx, fields)  # the host cache (128 codes) has turned over several times by now
    assert np.array_equal(pay, pay1) and np.array_equal(st, st1)


def _raw_call(ctx, jobs, n, d_llr, d_pay, d_st, null=None):
    import miphy
    import torch
    args = [C.c_void_p(jobs.ctypes.data), n, C.c_void_p(d_llr.data_ptr()), C.c_void_p(d_pay.data_ptr()), C.c_void_p(d_st.data_ptr())]
    if null is not None:
        args[null] = None
    return miphy.lib().miphy_uci_polar_decode_batch(ctx.h, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_rejections_leave_the_outputs_alone(ctx):
    import miphy
    import torch
    fields = fixed_fields()[:8]
    llr_off, pay_off, nl, npay = _layout(fields)
    d_llr = torch.zeros(nl + 20000, dtype=torch.int8, device="cuda")
    d_pay = torch.full((npay + 2000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    good = _jobs(fields, llr_off, pay_off)
    for A, E, rule in ((11, 64, "12 to 1706"), (1707, 4000, "12 to 1706"), (12, 19, "K_r + nPC < E_r"), (19, 28, "K_r + nPC < E_r"), (20, 8193, "exceeds 8192"),
                       (1706, 16386, "exceeds 8192")):
        jobs = good.copy()
        jobs[5]["nof_bits"], jobs[5]["nof_llr"] = A, E
        assert _raw_call(ctx, jobs, jobs.size, d_llr, d_pay, d_st) == -1
        assert rule in miphy.lib().miphy_last_error().decode() and "field 5" in miphy.lib().miphy_last_error().decode()
    for null in range(5):
        if null != 1:
            assert _raw_call(ctx, good, good.size, d_llr, d_pay, d_st, null=null) == -1
    assert _raw_call(ctx, good, (1 << 24) + 1, d_llr, d_pay, d_st) == -1
    assert _raw_call(ctx, good, 0, d_llr, d_pay, d_st) == 0
    torch.cuda.synchronize()
    assert bool((d_pay == SENTINEL).all()) and bool((d_st == SENTINEL).all())
    assert _raw_call(ctx, good, good.size, d_llr, d_pay, d_st) == 0  # and the same arrays are accepted as they are
    torch.cuda.synchronize()
    assert bool((d_st[:8] != SENTINEL).all()) and bool((d_st[8:] == SENTINEL).all())


def test_the_short_block_entry_points_still_refuse_a_12_bit_field(ctx):
    import miphy
    import torch
    jobs = np.zeros(1, miphy.UciFieldJob)
    jobs[0]["nof_bits"], jobs[0]["mod"], jobs[0]["nof_llr"] = 12, 2, 64
    d_llr = torch.zeros(64, dtype=torch.int8, device="cuda")
    d_pay = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((1,), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="miphy error -1"):
        ctx.uci_decode_batch(jobs, d_llr, d_pay, d_st)
    pdus, uci = np.zeros(1, miphy.PuschPdu), np.zeros(1, miphy.PuschUci)
    pdus[0]["mod"], uci[0]["nof_harq_ack_bits"], uci[0]["nof_enc_harq_ack_bits"] = 2, 12, 64
    with pytest.raises(RuntimeError, match="miphy error -1"):
        miphy.pusch_uci_field_jobs(pdus, uci)
    torch.cuda.synchronize()
    assert bool((d_pay == SENTINEL).all()) and bool((d_st == SENTINEL).all())


def test_two_pusch_pdus_with_long_and_short_fields_on_one_stream(ctx):
    """PDU one: a 20-bit CSI part 1 (polar) and a 2-bit HARQ-ACK (short block) next to a transport block; PDU two: a 12-bit HARQ-ACK
    (polar, CRC6, parity-check bits) and no transport block. The processor, the short-block detector and the polar decoder are
    enqueued one behind the other with no host synchronisation; the payloads are the bits that were multiplexed."""
    import miphy
    import torch
    import pusch_uci_tx as T
    import uci_short_block as S
    rng = np.random.default_rng(4242)
    ack2, csi20, ack12 = (rng.integers(0, 2, k).astype(np.uint8) for k in (2, 20, 12))
    slots = [T.pusch_uci_slot(rng, 24, 2, (2, 20, 0), (18, 60, 0), 40, [S.rate_match(S.encode(ack2, 2), 36), U.encode(20, 120, csi20), []], True),
             T.pusch_uci_slot(rng, 24, 4, (12, 0, 0), (25, 0, 0), 0, [U.encode(12, 100, ack12), [], []], False, slot=6, rnti=0x1234, n_id=77, scr=99)]
    nsc = 24 * 12
    pdus, uci = np.zeros(2, miphy.PuschPdu), np.zeros(2, miphy.PuschUci)
    pos = 5
    for i, s in enumerate(slots):
        p, u = pdus[i], uci[i]
        p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, s["slot"], s["rnti"], s["n_id"], s["scr"]
        p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = T.TBS_BITS[s["mod"]] // 8, 0, s["mod"], 1, 0, 14
        p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = s["bg"], 0, 1, [0, 1, 2, 3], 1, 6
        p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"], p["grid_offset"], p["tb_offset"] = 1 << 2, 24, [(1 << 24) - 1, 0, 0, 0, 0], i * 14 * nsc, 0
        u["nof_harq_ack_bits"], u["nof_csi_part1_bits"], u["nof_csi_part2_bits"] = s["O"]
        u["nof_enc_harq_ack_bits"], u["nof_enc_csi_part1_bits"], u["nof_enc_csi_part2_bits"] = s["G"]
        u["nof_harq_ack_rvd"], u["has_codeword"] = s["nof_harq_ack_rvd"], int(s["tb"] is not None)
        u["harq_ack_offset"], u["csi_part1_offset"], u["csi_part2_offset"] = pos, pos + s["G"][0] + 3, pos + s["G"][0] + 3 + s["G"][1] + 5
        pos += sum(s["G"]) + 3 + 5 + 7
    sj, sf, pj, pf = miphy.pusch_uci_jobs(pdus, uci)
    assert list(sf) == [0] and list(pf) == [1, 3]
    assert [int(j["payload_offset"]) for j in sj] == [0] and [int(j["payload_offset"]) for j in pj] == [2, 22]
    tb = slots[0]["tb"]
    ncb = miphy.sch_segmentation(tb.size, slots[0]["bg"]).nof_cbs
    soft = torch.zeros(ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
    msgs = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(tb.size, dtype=torch.uint8, device="cuda")
    res = torch.zeros(2 * miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    scal = torch.zeros(40, dtype=torch.float32, device="cuda")
    uci_llr = torch.full((pos + 9,), 99, dtype=torch.int8, device="cuda")
    grid = torch.from_numpy(np.concatenate([s["grid"].reshape(-1) for s in slots])).cuda()
    d_pay = torch.full((34 + 6,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st_short = torch.full((2,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st_polar = torch.full((3,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.pusch_process_batch_ex(pdus, uci, grid, soft, msgs, crc, out, res, scal, uci_llr, None)
    ctx.uci_decode_batch(sj, uci_llr, d_pay, d_st_short)
    ctx.uci_polar_decode_batch(pj, uci_llr, d_pay, d_st_polar)
    torch.cuda.synchronize()
    pay = d_pay.cpu().numpy()
    assert np.array_equal(pay[:2], ack2) and np.array_equal(pay[2:22], csi20) and np.array_equal(pay[22:34], ack12)
    assert np.all(pay[34:] == SENTINEL)
    assert list(d_st_short.cpu().numpy()) == [U.STATUS_VALID, SENTINEL] and list(d_st_polar.cpu().numpy()) == [U.STATUS_VALID, U.STATUS_VALID, SENTINEL]
    r = res.cpu().numpy().view(miphy.PuschResult)
    assert bool(r[0]["tb_crc_ok"]) and np.array_equal(out.cpu().numpy(), tb) and r[1]["nof_codeblocks_total"] == 0
