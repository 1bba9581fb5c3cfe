"""GPU: miphy_uci_decode_batch (the UCI short-block detector, csrc/uci.hip) against the reference's own detector
(tests/golden/short_block_detector.npz) and against the numpy restatement (tests/uci_short_block.py, pinned to the same fixture on the
CPU by tests/test_uci_short_block.py): fuzz in one launch with host and device jobs, n = 1 and 65536 fields, argument errors, and the
composed PUSCH path miphy_pusch_process_batch_ex + miphy_uci_decode_batch on one stream."""
import os

import numpy as np
import pytest

import uci_short_block as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = (1, 2, 4, 6, 8)


def _run(ctx, jobs, llr, n_payload, on_device=False, sentinel=0xAA):
    import torch
    llr_d = torch.from_numpy(np.ascontiguousarray(llr).astype(np.int8)).cuda()
    pay = torch.full((max(1, n_payload),), sentinel, dtype=torch.uint8, device="cuda")
    st = torch.full((max(1, jobs.size),), sentinel, dtype=torch.uint8, device="cuda")
    j = torch.from_numpy(jobs.view(np.uint8).copy()).cuda() if on_device else jobs
    ctx.uci_decode_batch(j, llr_d, pay, st)
    torch.cuda.synchronize()
    return pay.cpu().numpy(), st.cpu().numpy()


def _jobs(K, mod, E, llr_offset, payload_offset):
    import miphy
    jobs = np.zeros(len(K), miphy.UciFieldJob)
    jobs["nof_bits"], jobs["mod"], jobs["nof_llr"], jobs["llr_offset"], jobs["payload_offset"] = K, mod, E, llr_offset, payload_offset
    return jobs


def _fields(rng, n, long_every=50):
    """n random fields over every K, Qm and E: AWGN at random SNR, +-127 sprinkled, all-zero and tiny-integer fields; unaligned offsets."""
    K = rng.integers(1, 12, n)
    mod = rng.choice(MODS, n)
    Emin = np.where(K == 1, mod, np.where(K == 2, 3 * mod, K + 1))
    E = Emin + rng.integers(0, 120, n)
    E[::long_every] += 2000
    llrs, offs, o = [], [], 0
    for i in range(n):
        o += int(rng.integers(0, 4))  # gaps: any alignment
        msg = rng.integers(0, 2, int(K[i]), dtype=np.uint8)
        s = 1.0 - 2.0 * U.rate_match(U.encode(msg, int(mod[i])), int(E[i]))
        kind = rng.integers(0, 10)
        if kind == 0:
            x = np.zeros(int(E[i]), np.int64)
        elif kind == 1:
            x = rng.integers(-2, 3, int(E[i]))
        else:
            x = np.clip(np.round(rng.choice([4.0, 12.0, 30.0]) * (s + rng.choice([0.3, 1.0, 2.0, 4.0, 8.0]) * rng.standard_normal(int(E[i])))), -120, 120)
            x = x.astype(np.int64)
            if kind == 2:
                inf = rng.random(int(E[i])) < 0.1
                x[inf] = 127 * rng.choice([-1, 1], int(inf.sum()))
        llrs.append(x), offs.append(o)
        o += int(E[i])
    llr = np.zeros(o + 16, np.int64)
    for x, of in zip(llrs, offs):
        llr[of:of + x.size] = x
    return K, mod, E, np.array(offs, np.uint64), llr


def _check(pay, st, K, poff, bits, status):
    assert np.array_equal(st[:len(K)], status)
    for i in range(len(K)):
        assert np.array_equal(pay[int(poff[i]):int(poff[i]) + int(K[i])], bits[i]), i


def test_kernel_equals_reference_fixture(ctx):
    d = np.load(os.path.join(ROOT, "tests", "golden", "short_block_detector.npz"))
    jobs = _jobs(d["K"], d["mod"], d["E"], d["llr_offset"], d["payload_offset"])
    for on_device in (False, True):
        pay, st = _run(ctx, jobs, d["llr"], d["payload"].size, on_device)
        assert np.array_equal(st, d["status"])
        assert np.array_equal(pay, d["payload"])


def test_fuzz_one_launch_matches_restatement(ctx):
    rng = np.random.default_rng(4242)
    n = 20480
    K, mod, E, off, llr = _fields(rng, n)
    bits, status = U.detect_batch(llr, K, mod, E, off)
    assert (status == U.STATUS_VALID).any() and (status == U.STATUS_INVALID).any()
    # payloads in shuffled order, with gaps
    order = rng.permutation(n)
    poff = np.zeros(n, np.uint64)
    p = 5
    for i in order:
        poff[i] = p
        p += int(K[i]) + int(rng.integers(0, 3))
    jobs = _jobs(K, mod, E, off, poff)
    for on_device in (False, True):
        pay, st = _run(ctx, jobs, llr, p + 8, on_device)
        _check(pay, st, K, poff, bits, status)
        used = np.zeros(pay.size, bool)
        for i in range(n):
            used[int(poff[i]):int(poff[i]) + int(K[i])] = True
        assert (pay[~used] == 0xAA).all()  # nothing written outside the payloads


@pytest.mark.parametrize("n", [1, 65536])
def test_batch_sizes(ctx, n):
    rng = np.random.default_rng(n)
    K, mod, E, off, llr = _fields(rng, n, long_every=997)
    bits, status = U.detect_batch(llr, K, mod, E, off)
    poff = np.concatenate([[0], np.cumsum(K)[:-1]]).astype(np.uint64)
    pay, st = _run(ctx, _jobs(K, mod, E, off, poff), llr, int(K.sum()))
    _check(pay, st, K, poff, bits, status)
    assert (st != 0).all()


@pytest.mark.parametrize("K,mod,E", [(0, 2, 10), (12, 2, 40), (3, 2, 3), (5, 4, 5), (1, 4, 3), (2, 4, 11), (2, 1, 2), (4, 3, 40), (4, 0, 40)])
def test_invalid_jobs_are_refused_before_anything_runs(ctx, K, mod, E):
    import torch
    import miphy
    jobs = _jobs([3, K], [2, mod], [40, E], [0, 0], [0, 3])
    llr = torch.ones(64, dtype=torch.int8, device="cuda")
    pay = torch.full((16,), 0xAA, dtype=torch.uint8, device="cuda")
    st = torch.full((2,), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="miphy error -1"):
        ctx.uci_decode_batch(jobs, llr, pay, st)
    # n == 0 enqueues nothing either
    ctx.uci_decode_batch(np.zeros(0, miphy.UciFieldJob), llr, pay, st)
    torch.cuda.synchronize()
    assert (pay.cpu().numpy() == 0xAA).all() and (st.cpu().numpy() == 0xAA).all()


# ------------------------------------------------------------------ composed path: _ex + uci_decode_batch on one stream
RB_ALL = lambda nprb: [(0xFFFFFFFFFFFFFFFF if nprb >= 64 * (k + 1) else ((1 << max(0, nprb - 64 * k)) - 1)) for k in range(5)]


def _mux_map(O, case, n_in):
    idx = np.arange(n_in)
    digs = []
    for d in range(3):
        v = ((idx // (100 ** d)) % 100 + 1).astype(np.int8)
        digs.append(O.o_ulsch_demultiplex(*case, llr=v)[2])
    maps = []
    for k in range(4):
        a = [digs[d][k].astype(np.int64) for d in range(3)]
        src = (a[0] - 1) + 100 * (a[1] - 1) + 10000 * (a[2] - 1)
        src[a[0] == 0] = -1
        maps.append(src)
    return maps


@pytest.mark.parametrize("mod,O_ack,G_ack_re,rvd_re,O_c1,G_c1_re,O_c2,G_c2_re,with_tb,noise", [
    (4, 1, 20, 44, 0, 0, 0, 0, True, 0.02),
    (6, 2, 18, 40, 5, 60, 0, 0, True, 0.02),
    (2, 4, 50, 0, 1, 31, 7, 90, True, 0.02),
    (8, 1, 12, 0, 0, 0, 0, 0, True, 0.02),
    (4, 3, 25, 0, 4, 40, 0, 0, False, 0.02),
    (2, 11, 8, 0, 6, 6, 9, 6, False, 0.6),   # noisy, short fields: detection fails for some
    (4, 7, 4, 0, 10, 5, 3, 3, False, 1.5),
    (2, 8, 10, 0, 3, 5, 0, 0, False, 0.9),
])
def test_pusch_ex_then_uci_decode(ctx, mod, O_ack, G_ack_re, rvd_re, O_c1, G_c1_re, O_c2, G_c2_re, with_tb, noise):
    import torch
    import miphy
    import oracle_lib as O
    rng = np.random.default_rng(9100 + mod + 13 * O_ack + O_c1)
    nprb, slot, rnti, n_id, scr = 24, 5, 0x3311, 411, 17
    nsc = nprb * 12
    dm = np.zeros(14, np.uint8)
    dm[2] = 1
    rb = np.ones(nprb, np.uint8)
    G = (G_ack_re * mod, G_c1_re * mod, G_c2_re * mod)
    Os = (O_ack, O_c1, O_c2)
    case = (mod, 1, nprb, 0, 14, rvd_re * mod, 1, 1 << 2, 2, G, Os)
    n_in, n_sch, _, ph = O.o_ulsch_demultiplex(*case)
    n_re = n_in // mod
    # ---- transmit side: UCI messages through the TS 38.212 short-block encoder and rate matcher
    tbs_bits = {2: 2976, 4: 6016, 6: 9736, 8: 14600}[mod]
    tb = rng.integers(0, 256, tbs_bits // 8, dtype=np.uint8)
    bg = 1 if tbs_bits > 3824 else 2
    sch_bits = O.o_pdsch_encode(bg, 0, mod, 0, 1, n_sch // mod, tb) if with_tb else rng.integers(0, 2, n_sch, dtype=np.uint8)
    msgs = [rng.integers(0, 2, o, dtype=np.uint8) for o in Os]
    uci_bits = [U.rate_match(U.encode(m, mod), g) if o else np.zeros(0, np.uint8) for m, o, g in zip(msgs, Os, G)]
    maps = _mux_map(O, case, n_in)
    cw = np.zeros(n_in, np.uint8)
    for k, bits in enumerate([sch_bits] + uci_bits):
        m = maps[k]
        cw[m[m >= 0]] = bits[m >= 0]
    sc_bits = cw ^ O.o_gold((rnti << 15) + n_id, 0, n_in)
    for re in ph:
        sc_bits[re * mod + 1] = sc_bits[re * mod]
        sc_bits[re * mod + 2:re * mod + mod] = 1
    sym = O.nr_modulate(sc_bits, mod)
    h = (0.9 * np.exp(1j * 0.4) * (1 + 0.1 * np.cos(np.arange(nsc) / 40.0))).astype(np.complex64)
    grid = np.zeros((1, 14, nsc), np.complex64)
    k = 0
    for sy in range(14):
        if sy == 2:
            continue
        grid[0, sy] = sym[k:k + nsc] * h
        k += nsc
    assert k == n_re
    g3 = np.zeros((1, 14, nsc), np.complex64)
    O.o_dmrs_pdsch_map(slot, 0, 0, scr, 0, 10 ** (3 / 20), dm, rb, [0], g3)
    grid[0, 2] = g3[0, 2] * h
    grid += ((rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * noise).astype(np.complex64)
    # ---- oracle receive chain up to the UCI soft bits
    ce, sc = O.o_dmrs_pusch_estimate(1, slot, 0, scr, 0, np.float32(10.0) ** np.float32(3.0 / 20.0), dm, rb, 0, 14, 1, grid)
    llr, _ = O.o_pusch_demodulate_ex(rnti, n_id, mod, 0, 14, dm, 0, 2, rb, grid, ce[0], float(sc[0, 0, 2]), placeholders=ph)
    _, _, streams, _ = O.o_ulsch_demultiplex(*case, llr=llr)
    # ---- device: _ex, then the UCI decoder on the same stream, no synchronisation in between
    pdus = np.zeros(1, dtype=miphy.PuschPdu)
    p = pdus[0]
    p["numerology"], p["slot_in_frame"], p["rnti"], p["n_id"], p["dmrs_scrambling_id"] = 1, slot, rnti, n_id, scr
    p["tb_bytes"], p["harq_cb_index"], p["mod"], p["nof_rx_ports"], p["start_symbol"], p["nof_symbols"] = tb.size, 0, mod, 1, 0, 14
    p["bg"], p["rv"], p["new_data"], p["rx_ports"], p["use_early_stop"], p["nof_ldpc_iterations"] = bg, 0, 1, [0, 1, 2, 3], 1, 6
    p["dmrs_symbols_mask"], p["grid_nof_prb"], p["rb_mask"], p["grid_offset"], p["tb_offset"] = 1 << 2, nprb, RB_ALL(nprb), 0, 0
    uci = np.zeros(1, dtype=miphy.PuschUci)
    u = uci[0]
    u["nof_harq_ack_bits"], u["nof_csi_part1_bits"], u["nof_csi_part2_bits"] = Os
    u["nof_enc_harq_ack_bits"], u["nof_enc_csi_part1_bits"], u["nof_enc_csi_part2_bits"] = G
    u["nof_harq_ack_rvd"], u["has_codeword"] = rvd_re * mod, int(with_tb)
    u["harq_ack_offset"], u["csi_part1_offset"], u["csi_part2_offset"] = 3, 3 + G[0] + 1, 3 + G[0] + 1 + G[1] + 2
    ncb = miphy.sch_segmentation(tb.size, bg).nof_cbs
    soft = torch.zeros(ncb * miphy.HARQ_CB_STRIDE, dtype=torch.int8, device="cuda")
    msgs_d = torch.zeros(ncb * miphy.HARQ_MSG_STRIDE, dtype=torch.uint8, device="cuda")
    crc = torch.zeros(ncb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(tb.size, dtype=torch.uint8, device="cuda")
    res = torch.zeros(miphy.PuschResult.itemsize, dtype=torch.uint8, device="cuda")
    scal = torch.zeros(20, dtype=torch.float32, device="cuda")
    uci_llr = torch.zeros(3 + sum(G) + 3 + 8, dtype=torch.int8, device="cuda")
    jobs, field = miphy.pusch_uci_field_jobs(pdus, uci)
    pay = torch.full((16 * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    st = torch.full((3,), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.pusch_process_batch_ex(pdus, uci, torch.from_numpy(grid.reshape(-1)).cuda(), soft, msgs_d, crc, out, res, scal, uci_llr, None)
    ctx.uci_decode_batch(jobs, uci_llr, pay, st)
    torch.cuda.synchronize()
    ul, pay, st = uci_llr.cpu().numpy(), pay.cpu().numpy(), st.cpu().numpy()
    assert list(field) == [f for f in range(3) if Os[f]]
    for j, f in enumerate(field):
        K, g, off = Os[f], G[f], int(jobs[j]["llr_offset"])
        got = pay[int(jobs[j]["payload_offset"]):int(jobs[j]["payload_offset"]) + K]
        # exact against the restatement on the device's own soft bits
        rb_bits, rs = U.detect(ul[off:off + g], K, mod)
        assert np.array_equal(got, rb_bits) and st[j] == rs, (f, got, rb_bits, st[j], rs)
        # against the oracle chain: its streams equal the device's up to one quantisation step now and then (the floating-point channel
        # estimate, tests/test_pusch_uci_gpu.py); where they are identical, so are payload and verdict
        ob, os_ = U.detect(streams[1 + f], K, mod)
        if np.array_equal(ul[off:off + g], streams[1 + f]):
            assert np.array_equal(got, ob) and st[j] == os_, f
        if noise <= 0.02:
            assert np.array_equal(got, msgs[f]), (f, got, msgs[f])  # clean channel: the transmitted bits
            assert K <= 2 or st[j] == U.STATUS_VALID
    assert (st[len(field):] == 0xAA).all()
