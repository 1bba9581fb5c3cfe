"""GPU: miphy_uci_polar_decode_list_batch (CRC-aided list decoding of polar-coded UCI fields) against tests/uci_polar_list.py, that is
the restatement of the oracle's list recursion (tests/polar_scl_ref.py) per segment inside the TS 38.212 framing with the CRC11
selection rule of include/miphy.h: payload bits and verdict bit for bit on every input at list sizes 2, 4 and 8, the fields whose CRC
fails included. The restatement's results are computed once per module."""
import ctypes as C
import functools

import numpy as np
import pytest

import uci_polar as U
import uci_polar_list as UL
from test_uci_polar_gpu import SENTINEL, _jobs, _layout, _soft

pytestmark = pytest.mark.gpu

LIST_SIZES = (2, 4, 8)
# (A, E): the noise levels next to one noise-free copy. The levels of the N = 1024 shapes were chosen on the CPU so that the
# restatement's verdicts meet the conditions asserted in fixed_fields(); (1706, 3500) yields no valid field from sigma = 0.8 upwards.
SHAPES = [((20, 40), (0.8,) * 8),          # the smallest CRC11 field, N = 64
          ((20, 8192), (3.0, 3.5)),        # repetition, E_r at the limit
          ((31, 64), (0.8,) * 8), ((64, 128), (0.8,) * 6), ((100, 300), (1.1,) * 4),
          ((359, 2000), (1.3, 1.4)),       # one segment, N = 1024
          ((360, 1087), (0.9, 1.0)),       # C = 1
          ((360, 1088), (1.0, 1.1)),       # C = 2
          ((361, 1089), (1.0, 1.1)),       # C = 2, odd A, odd E: the last soft bit belongs to no segment
          ((1013, 2100), (0.9, 1.0)),      # C = 2, odd A, pad bit
          ((1706, 3500), (0.6, 0.7)),
          ((12, 32), (0.7, 1.0)), ((19, 216), (1.5, 2.5))]  # CRC6: the SSC kernel at every list size


def _field(A, E, llr, sent, tag):
    ref = {1: UL.decode_ex(A, E, llr, 1)}
    for L in LIST_SIZES:
        ref[L] = UL.decode_ex(A, E, llr, L)
    return dict(A=A, E=E, llr=llr, sent=sent, tag=tag, f=U.info(A, E), ref=ref)


def _status(c, L):
    return U.STATUS_VALID if c["ref"][L][1] else U.STATUS_INVALID


@functools.lru_cache(maxsize=None)
def fixed_fields():
    out = []
    for i, ((A, E), sigmas) in enumerate(SHAPES):
        for j, sigma in enumerate((0.0,) + sigmas):
            rng = np.random.default_rng(7000 + 20 * i + j)
            x = rng.integers(0, 2, A).astype(np.uint8)
            out.append(_field(A, E, _soft(rng, U.encode(A, E, x), sigma), x, (A, E, sigma)))
    # conditions on the inputs, for the restatement alone
    for L in (1,) + LIST_SIZES:
        assert {_status(c, L) for c in out if c["A"] >= 20} == {U.STATUS_VALID, U.STATUS_INVALID}, L
        for c in out:
            if c["tag"][2] == 0.0:
                assert c["ref"][L][1] and np.array_equal(c["ref"][L][0], c["sent"]), (c["tag"], L)
    assert sum(1 for c in out if c["ref"][8][1] and not c["ref"][1][1]) >= 10
    assert sum(1 for c in out if any(any(c["ref"][L][2]) for L in LIST_SIZES)) >= 5
    assert any(c["f"]["n"] == 10 and c["f"]["C"] == 2 for c in out) and any(c["f"]["n"] == 6 for c in out)
    return out


@functools.lru_cache(maxsize=None)
def flipped_fields():
    """Two-segment fields with one segment sign-flipped wholesale, segment 1 first, then segment 0. (700, 1400) has a shortened code
    (E_r = 700 < N = 1024, 16 K_r > 7 E_r): the flipped soft bits contradict the known zeros, no survivor passes and the field is
    INVALID. (500, 1100) has a repeated code (E_r = 550 > N = 512), where the complement of a codeword is the codeword of the message
    with its last bit toggled: at list size 1 the CRC fails on that bit, from list size 2 the path with the bit toggled back is among
    the survivors, far from the best metric, and the CRC picks it."""
    rng = np.random.default_rng(78)
    out = []
    for A, E in ((700, 1400), (500, 1100)):
        f = U.info(A, E)
        assert f["C"] == 2
        for seg in (1, 0):
            x = rng.integers(0, 2, A).astype(np.uint8)
            llr = _soft(rng, U.encode(A, E, x), 0.0)
            llr[seg * f["E_r"]:(seg + 1) * f["E_r"]] *= -1
            out.append(_field(A, E, llr, x, (A, E, "segment %d flipped" % seg)))
    for c in out:
        for L in (1,) + LIST_SIZES:
            assert c["ref"][L][1] == (c["A"] == 500 and L > 1), (c["tag"], L)
    return out


def _run(ctx, fields, L, unowned=None, one_by_one=False, entry="list"):
    """Payload and status buffers (numpy) after decoding `fields` at list size L, in one call or one call per field."""
    import torch
    llr_off, pay_off, nl, npay = _layout(fields)
    llr = np.full(nl, 55, np.int8)
    for c, o in zip(fields, llr_off):
        llr[o:o + c["E"]] = c["llr"]
        if unowned is not None and c["f"]["C"] == 2 and c["E"] % 2:
            llr[o + c["E"] - 1] = unowned
    d_llr = torch.from_numpy(llr).cuda()
    d_pay = torch.full((npay,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((len(fields) + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    jobs = _jobs(fields, llr_off, pay_off)
    if entry == "ssc":
        ctx.uci_polar_decode_batch(jobs, d_llr, d_pay, d_st)
    elif one_by_one:
        for i in range(len(fields)):
            ctx.uci_polar_decode_list_batch(jobs[i:i + 1], L, d_llr, d_pay, d_st[i:])
    else:
        ctx.uci_polar_decode_list_batch(jobs, L, d_llr, d_pay, d_st)
    torch.cuda.synchronize()
    return d_pay.cpu().numpy(), d_st.cpu().numpy(), pay_off


def _check(fields, L, pay, st, pay_off):
    touched = np.zeros(pay.size, bool)
    for i, (c, o) in enumerate(zip(fields, pay_off)):
        got, want = pay[o:o + c["A"]], c["ref"][L][0]
        assert np.array_equal(got, want), (c["tag"], L, int((got != want).sum()))
        assert st[i] == _status(c, L), (c["tag"], L, int(st[i]))
        touched[o:o + c["A"]] = True
    assert np.all(pay[~touched] == SENTINEL) and np.all(st[len(fields):] == SENTINEL)


def _segments():
    import miphy
    ssc, lst = C.c_uint(0), C.c_uint(0)
    miphy.lib().miphy_debug_uci_polar_list_segments(C.byref(ssc), C.byref(lst))
    return ssc.value, lst.value


@pytest.mark.parametrize("L", LIST_SIZES)
def test_fixed_shapes_in_one_call_equal_the_restatement(ctx, L):
    fields = fixed_fields()
    pay, st, pay_off = _run(ctx, fields, L)
    # the fields of 12..19 bits went to the SSC kernel, every segment of the others to the list kernel: with the N = 1024 fields among
    # them, list size 8 is the launch with more than 48 KB of LDS
    assert _segments() == (sum(c["f"]["C"] for c in fields if c["A"] <= 19), sum(c["f"]["C"] for c in fields if c["A"] >= 20))
    assert sum(1 for c in fields if c["A"] <= 19) >= 6 and sum(1 for c in fields if c["A"] >= 20 and c["f"]["n"] == 10) >= 12
    _check(fields, L, pay, st, pay_off)


@pytest.mark.parametrize("L", LIST_SIZES)
def test_a_flipped_segment_invalidates_the_field_and_leaves_the_other_half(ctx, L):
    fields = flipped_fields()
    pay, st, pay_off = _run(ctx, fields, L)
    _check(fields, L, pay, st, pay_off)
    for i, (c, seg) in enumerate(zip(fields, (1, 0, 1, 0))):
        got = pay[pay_off[i]:pay_off[i] + c["A"]]
        if c["A"] == 700:
            assert st[i] == U.STATUS_INVALID
            half = c["f"]["A_seg"]
            keep = slice(0, half) if seg == 1 else slice(half, 2 * half)
            assert np.array_equal(got[keep], c["sent"][keep]) and not np.array_equal(got, c["sent"])
        else:  # repaired by the CRC among the survivors
            assert st[i] == U.STATUS_VALID and np.array_equal(got, c["sent"]) and any(c["ref"][L][2])


def test_one_field_per_call_and_small_pieces_give_the_same_bytes(ctx):
    import miphy
    fields = fixed_fields() + flipped_fields()
    pay, st, pay_off = _run(ctx, fields, 8)
    assert miphy.lib().miphy_debug_uci_polar_pieces() == 1
    _check(fields, 8, pay, st, pay_off)
    pay1, st1, _ = _run(ctx, fields, 8, one_by_one=True)
    assert np.array_equal(pay, pay1) and np.array_equal(st, st1)
    try:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(20000)
        pay2, st2, _ = _run(ctx, fields, 8)
        assert miphy.lib().miphy_debug_uci_polar_pieces() >= 5
    finally:
        miphy.lib().miphy_debug_set_uci_polar_piece_bytes(0)
    assert np.array_equal(pay, pay2) and np.array_equal(st, st2)


def test_the_unowned_last_soft_bit_is_never_read(ctx):
    fields = [c for c in fixed_fields() if c["f"]["C"] == 2 and c["E"] % 2]
    assert len(fields) >= 3
    a = _run(ctx, fields, 4, unowned=127)
    b = _run(ctx, fields, 4, unowned=-127)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _check(fields, 4, a[0], a[1], a[2])


def test_list_size_1_is_the_ssc_entry_point_byte_for_byte(ctx):
    fields = fixed_fields() + flipped_fields()
    a = _run(ctx, fields, 1)
    assert _segments() == (sum(c["f"]["C"] for c in fields), 0)
    b = _run(ctx, fields, 1, entry="ssc")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _check(fields, 1, a[0], a[1], a[2])


def _raw_call(ctx, jobs, n, L, d_llr, d_pay, d_st, null=None):
    import miphy
    import torch
    args = [ctx.h, C.c_void_p(jobs.ctypes.data), n, L, C.c_void_p(d_llr.data_ptr()), C.c_void_p(d_pay.data_ptr()), C.c_void_p(d_st.data_ptr())]
    if null is not None:
        args[null] = None
    return miphy.lib().miphy_uci_polar_decode_list_batch(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_rejections_leave_the_outputs_alone(ctx):
    import miphy
    import torch
    fields = [c for c in fixed_fields() if c["f"]["n"] <= 8][:8]
    llr_off, pay_off, nl, npay = _layout(fields)
    d_llr = torch.zeros(nl + 20000, dtype=torch.int8, device="cuda")
    d_pay = torch.full((npay + 2000,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    good = _jobs(fields, llr_off, pay_off)
    for L in (0, 3, 16):
        assert _raw_call(ctx, good, good.size, L, d_llr, d_pay, d_st) == -1
        assert "list size" in miphy.lib().miphy_last_error().decode()
    for null in (0, 1, 4, 5, 6):
        assert _raw_call(ctx, good, good.size, 8, d_llr, d_pay, d_st, null=null) == -1
    for A, E, rule in ((11, 64, "12 to 1706"), (1707, 4000, "12 to 1706"), (20, 31, "K_r + nPC < E_r"), (20, 8193, "exceeds 8192")):
        jobs = good.copy()
        jobs[5]["nof_bits"], jobs[5]["nof_llr"] = A, E
        assert _raw_call(ctx, jobs, jobs.size, 8, d_llr, d_pay, d_st) == -1
        assert rule in miphy.lib().miphy_last_error().decode() and "field 5" in miphy.lib().miphy_last_error().decode()
    assert _raw_call(ctx, good, 0, 8, d_llr, d_pay, d_st) == 0
    assert miphy.lib().miphy_debug_uci_polar_pieces() == 0 and _segments() == (0, 0)
    torch.cuda.synchronize()
    assert bool((d_pay == SENTINEL).all()) and bool((d_st == SENTINEL).all())
    assert _raw_call(ctx, good, good.size, 8, d_llr, d_pay, d_st) == 0  # and the same arrays are accepted as they are
    torch.cuda.synchronize()
    assert bool((d_st[:8] != SENTINEL).all()) and bool((d_st[8:] == SENTINEL).all())


def test_a_pusch_pdu_with_a_40_bit_harq_ack_and_a_7_bit_csi_field_on_one_stream(ctx):
    """One PDU with a transport block, a 40-bit HARQ-ACK (polar, CRC11: the list kernel) and a 7-bit CSI part 1 (short block). The
    processor, the short-block detector and the list decoder are enqueued one behind the other with no host synchronisation."""
    import miphy
    import torch
    import pusch_uci_tx as T
    import uci_short_block as S
    rng = np.random.default_rng(4343)
    ack40, csi7 = (rng.integers(0, 2, k).astype(np.uint8) for k in (40, 7))
    s = T.pusch_uci_slot(rng, 24, 2, (40, 7, 0), (60, 30, 0), 0, [U.encode(40, 120, ack40), S.rate_match(S.encode(csi7, 2), 60), []], True)
    nsc = 24 * 12
    pdus, uci = np.zeros(1, miphy.PuschPdu), np.zeros(1, miphy.PuschUci)
    p, u = pdus[0], uci[0]
    p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, s["slot"], s["rnti"], s["n_id"], s["scr"]
    p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = T.TBS_BITS[s["mod"]] // 8, 0, s["mod"], 1, 0, 14
    p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = s["bg"], 0, 1, [0, 1, 2, 3], 1, 6
    p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"], p["grid_offset"], p["tb_offset"] = 1 << 2, 24, [(1 << 24) - 1, 0, 0, 0, 0], 0, 0
    u["nof_harq_ack_bits"], u["nof_csi_part1_bits"], u["nof_csi_part2_bits"] = s["O"]
    u["nof_enc_harq_ack_bits"], u["nof_enc_csi_part1_bits"], u["nof_enc_csi_part2_bits"] = s["G"]
    u["nof_harq_ack_rvd"], u["has_codeword"] = s["nof_harq_ack_rvd"], 1
    u["harq_ack_offset"], u["csi_part1_offset"], u["csi_part2_offset"] = 5, 5 + s["G"][0] + 3, 5 + s["G"][0] + 3 + s["G"][1] + 5
    pos = 5 + sum(s["G"]) + 3 + 5 + 7
    sj, sf, pj, pf = miphy.pusch_uci_jobs(pdus, uci)
    assert list(sf) == [1] and list(pf) == [0]
    assert [int(j["payload_offset"]) for j in pj] == [0] and [int(j["payload_offset"]) for j in sj] == [40]
    tb = s["tb"]
    ncb = miphy.sch_segmentation(tb.size, s["bg"]).nof_cbs
    soft = torch.zeros(ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
    msgs = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(tb.size, dtype=torch.uint8, device="cuda")
    res = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    scal = torch.zeros(40, dtype=torch.float32, device="cuda")
    uci_llr = torch.full((pos + 9,), 99, dtype=torch.int8, device="cuda")
    grid = torch.from_numpy(s["grid"].reshape(-1)).cuda()
    d_pay = torch.full((47 + 6,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st_short = torch.full((2,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_st_polar = torch.full((2,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.pusch_process_batch_ex(pdus, uci, grid, soft, msgs, crc, out, res, scal, uci_llr, None)
    ctx.uci_decode_batch(sj, uci_llr, d_pay, d_st_short)
    ctx.uci_polar_decode_list_batch(pj, 8, uci_llr, d_pay, d_st_polar)
    torch.cuda.synchronize()
    assert _segments() == (0, 1)
    pay = d_pay.cpu().numpy()
    assert np.array_equal(pay[:40], ack40) and np.array_equal(pay[40:47], csi7) and np.all(pay[47:] == SENTINEL)
    assert list(d_st_short.cpu().numpy()) == [U.STATUS_VALID, SENTINEL] and list(d_st_polar.cpu().numpy()) == [U.STATUS_VALID, SENTINEL]
    r = res.cpu().numpy().view(miphy.PuschResult)
    assert bool(r[0]["tb_crc_ok"]) and np.array_equal(out.cpu().numpy(), tb)
