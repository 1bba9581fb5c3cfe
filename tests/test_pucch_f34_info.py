"""CPU: miphy_pucch_f34_info through the binding, no device. What the library derives from a PUCCH format 3 / 4 job -- DM-RS symbols,
data symbols per hop, M, E, short block or polar -- must equal the numpy layout of tests/pucch_f34_tx.py for every accepted combination, and
every rule of the issue must refuse with its code and its message. The record sizes are checked against include/miphy.h."""
import itertools
import os
import re

import numpy as np
import pytest

import miphy
import pucch_f34_tx as X
import uci_polar as UP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPP = -1, -4


def info_of(p, K, **changes):
    j = X.job_of(p, K)
    for k, v in changes.items():
        j[k] = v
    return miphy.pucch_f34_info(j)


def expect(p, K):
    dmrs, data = X.layout(p["nsym"], p["hop"], p["add"])
    mask = sum(1 << (p["start"] + o) for o in dmrs[0] + dmrs[1])
    return mask, [len(dmrs[0]), len(dmrs[1])], [len(data[0]), len(data[1])], 12 * p["nprb"], X.nof_soft_bits(p), int(K > 11)


def test_every_accepted_layout_equals_the_numpy_one():
    n = 0
    for nsym, hop, add, pi2 in itertools.product(range(4, 15), (0, 1), (0, 1), (0, 1)):
        shapes = [(3, nprb, 0, 0) for nprb in X.F3_NPRB] + [(4, 1, nsf, idx) for nsf in (2, 4) for idx in range(nsf)]
        for fmt, nprb, nsf, idx in shapes:
            p = X.pdu(fmt, nsym, nprb, hop, add, pi2, nsf, idx, nports=1 + n % 4, prb=n % 5, prb2=17, grid_nprb=34, start=n % (15 - nsym))
            E = X.nof_soft_bits(p)
            for K in (3, 11, 12, 20):
                ok = E > K if K <= 11 else UP.info(K, E) is not None
                if not ok:
                    with pytest.raises(Exception, match="error -1"):
                        info_of(p, K)
                    continue
                got, (mask, ndm, ndata, M, E_, polar) = info_of(p, K), expect(p, K)
                assert (int(got["dmrs_symbols_mask"]), list(got["nof_dmrs_symbols"]), list(got["nof_data_symbols"]), int(got["M"]), int(got["E"]),
                        int(got["polar"])) == (mask, ndm, ndata, M, E_, polar), (fmt, nsym, hop, add, nprb, pi2, nsf, K)
                n += 1
    assert n > 4000


def refused(code, text, p, K, **changes):
    with pytest.raises(Exception) as e:
        info_of(p, K, **changes)
    assert "error %d" % code in str(e.value) and text in str(e.value), str(e.value)
    assert text in miphy.lib().miphy_last_error().decode()


def test_two_prbs_are_unsupported_like_the_length_24_sequence():
    refused(EUNSUPP, "length-24", X.pdu(3, 14, 2), 20)
    with pytest.raises(Exception, match="error -4"):
        miphy.low_papr_sequence(0, 0, 24)


@pytest.mark.parametrize("nprb", [7, 11, 13, 14, 17, 0])
def test_other_prb_counts_are_invalid(nprb):
    refused(EINVAL, "format 3 on %d PRBs" % nprb, X.pdu(3, 14, nprb), 20)


def test_the_rules():
    f3, f4 = X.pdu(3, 14, 4, nports=2), X.pdu(4, 14, 1, occ_len=4, occ_idx=1)
    info_of(f3, 20), info_of(f4, 20)
    refused(EINVAL, "format 2 is not 3 or 4", f3, 20, format=2)
    refused(EINVAL, "occ_index 4 is not below occ_length 4", f4, 20, occ_index=4)
    refused(EINVAL, "occ_index 2 is not below occ_length 2", f4, 20, occ_length=2, occ_index=2)
    refused(EINVAL, "occ_length 3", f4, 20, occ_length=3)
    refused(EINVAL, "format 4 on 2 PRBs", f4, 20, nof_prb=2)
    refused(EINVAL, "2 UCI bits", f3, 2)
    refused(EINVAL, "CSI part 2 (5 bits)", f3, 20, nof_csi_part2=5)
    refused(EINVAL, "invalid number of receive ports 5", f3, 20, nof_ports=5)
    refused(EINVAL, "invalid number of receive ports 0", f3, 20, nof_ports=0)
    refused(EINVAL, "invalid symbol range", f3, 20, nof_symbols=3)
    refused(EINVAL, "invalid symbol range", f3, 20, start_symbol=1)
    refused(EINVAL, "outside the frame", f3, 20, slot=20)
    refused(EINVAL, "leaves the grid", f3, 20, grid_nprb=51)
    refused(EINVAL, "leaves the BWP", f3, 20, starting_prb=49)
    refused(EINVAL, "leaves the BWP", f3, 20, intra_slot_hopping=1, second_hop_prb=49)
    refused(EINVAL, "0 or 1", f3, 20, pi2_bpsk=2)
    refused(EINVAL, "0..1023", f3, 20, n_id_hopping=1024)
    refused(EINVAL, "0..1023", f3, 20, n_id_scrambling=1024)
    with pytest.raises(Exception, match="null argument"):
        miphy.binding.check(miphy.lib().miphy_pucch_f34_info(None, None))


def test_payloads_the_framing_refuses():
    small = X.pdu(4, 4, 1, 1, 0, 1, 4, 0)  # E = 6
    assert info_of(small, 5)["E"] == 6
    refused(EINVAL, "6 bits in 6 soft bits", small, 6)
    refused(EINVAL, "K_r + nPC < E_r", small, 12)
    one_prb = X.pdu(3, 4, 1, 1, 0, 1)  # E = 24
    assert info_of(one_prb, 12)["E"] == 24 and UP.info(12, 24) is not None
    refused(EINVAL, "K_r + nPC < E_r", one_prb, 19)  # 25 + 3 on 24
    refused(EINVAL, "K_r + nPC < E_r", one_prb, 20)
    wide = X.pdu(3, 14, 16)  # E = 4608: the code rate is not a rule
    assert info_of(wide, 1706)["polar"] == 1
    refused(EINVAL, "12 to 1706 bits", wide, 1707)


def test_record_sizes_against_the_header():
    hdr = open(os.path.join(ROOT, "include", "miphy.h")).read()
    sizes = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}
    for name, dtype in (("miphy_pucch_f34_job", miphy.PucchF34Job), ("miphy_pucch_f34_info_t", miphy.PucchF34Info)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            m = re.match(r"\s*(uint\d+_t)\s+(.*)", decl.strip(), flags=re.S)
            if not m:
                continue
            for f in m.group(2).split(","):
                a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
                fields.append((a.group(1), m.group(1), int(a.group(2) or 1)))
        assert [f[0] for f in fields] == list(dtype.names), name
        off = 0
        for fname, ctype, count in fields:  # natural alignment, as the C compiler lays the record out
            off = -(-off // sizes[ctype]) * sizes[ctype]
            assert dtype.fields[fname][1] == off, (name, fname)
            off += sizes[ctype] * count
        assert -(-off // 8) * 8 == dtype.itemsize or off == dtype.itemsize, (name, off, dtype.itemsize)
    assert miphy.PucchF34Job.itemsize == 80 and miphy.PucchF34Info.itemsize == 32
