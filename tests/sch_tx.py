"""A shared-channel transmitter assembled from the oracle's pieces (segmentation, CRCs, LDPC encoder, rate matcher), so that a
test can corrupt the transport block BEHIND the codeblock CRCs: every codeblock then decodes and passes its own CRC while the
transport-block CRC fails, the one outcome o_pdsch_encode cannot produce. Uncorrupted it equals o_pdsch_encode bit for bit
(tests/test_sch_tx.py). TEST INFRASTRUCTURE."""
import numpy as np

from oracle_lib import CRC16, CRC24A, CRC24B, o_crc_bits, o_ldpc_encode, o_rate_match, o_segmentation

FILLER = 254


def _crc_bits(value, n):
    return np.array([(value >> (n - 1 - i)) & 1 for i in range(n)], dtype=np.uint8)


def sch_codeword(bg, rv, mod, Nref, nof_layers, nof_ch_symbols, tb, tb_crc_flip=0, flip_bits=()):
    """Codeword (one bit per byte) of the transport block `tb` (bytes) and the payload the receiver sees (bytes).
    tb_crc_flip is XORed into the transport-block CRC; flip_bits are bit indices into TB + TB CRC. Both act before the
    codeblock CRCs are computed."""
    tb = np.ascontiguousarray(tb, dtype=np.uint8)
    s = o_segmentation(tb.size * 8, bg, mod, nof_layers, nof_ch_symbols)
    bits = np.unpackbits(tb)
    ncrc = s.nof_tb_crc_bits
    assert ncrc == (16 if bits.size <= 3824 else 24)
    crc = o_crc_bits(CRC16 if ncrc == 16 else CRC24A, bits) ^ int(tb_crc_flip)
    assert 0 <= crc < (1 << ncrc)
    b = np.concatenate([bits, _crc_bits(crc, ncrc)])
    for i in flip_bits:
        b[i] ^= 1
    payload = np.packbits(b[:bits.size])
    b = np.concatenate([b, np.zeros(s.zero_pad, np.uint8)])
    assert b.size == s.nof_cbs * s.cb_info_bits
    out = []
    for c in range(s.nof_cbs):
        msg = b[c * s.cb_info_bits:(c + 1) * s.cb_info_bits]
        if s.nof_cbs > 1:
            msg = np.concatenate([msg, _crc_bits(o_crc_bits(CRC24B, msg), 24)])
        msg = np.concatenate([msg, np.full(s.nof_filler_bits, FILLER, np.uint8)])
        assert msg.size == s.K
        out.append(o_rate_match(rv, mod, Nref, s.nof_filler_bits, o_ldpc_encode(bg, s.Z, msg, s.N), s.E[c]))
    cw = np.concatenate(out)
    assert cw.size == nof_ch_symbols * mod
    return cw, payload


def cb_payload_range(seg, c):
    """[first, last] transport-block bit that codeblock c carries (the TB CRC and the zero pad of the last one are not counted)."""
    lo = c * seg.cb_info_bits
    return lo, min(lo + seg.cb_info_bits, seg.tbs) - 1
