"""CPU: miphy_pucch_f0_info through the binding, no device. What the library derives from a PUCCH format 0 job -- the hypotheses' cyclic shifts in
table order, D, the free shifts and the default threshold -- must equal the numpy restatement of tests/pucch_f0_ref.py for every accepted
combination, and every rule of the C ABI must refuse with its code and its message. The record sizes are checked against include/miphy.h."""
import itertools
import os
import re

import numpy as np
import pytest

import miphy
import pucch_f0_ref as R
import pucch_f0_tx as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
UCI = ((1, 0), (2, 0), (0, 1), (1, 1), (2, 1))
MASKS = (0, 0x001, 0x820, 0x555, 0xaaa, 0x0ff, 0xf0f, 0x7fe, 0xfff)


def info_of(p, **changes):
    j = X.job_of(p)
    for k, v in changes.items():
        j[k] = v
    return miphy.pucch_f0_info(j)


def test_every_accepted_combination_equals_the_numpy_restatement():
    n = refused = 0
    for (nharq, nsr), ics, mask, known in itertools.product(UCI, range(12), MASKS, (0, 1)):
        nports, nsym = 1 + n % 4, 1 + (n // 4) % 2
        p = X.pdu(nports, nsym, hop=(n // 8) % 2 if nsym == 2 else 0, start=n % (15 - nsym), prb=n % 7, prb2=19, ics=ics, nharq=nharq, nsr=nsr, mask=mask,
                  nid=(37 * n) % 1024, slot=n % 10, numerology=n % 2, noise_var=0.25 * known)
        n += 1
        hyp, fm = R.hypotheses(p), R.free_mask(p)
        if fm == 0 and not known:
            with pytest.raises(Exception, match="no free cyclic shift to estimate the noise from"):
                info_of(p)
            refused += 1
            continue
        got = info_of(p)
        assert int(got["nof_hypotheses"]) == len(hyp) and list(got["shifts"][:len(hyp)]) == hyp, (nharq, nsr, ics)
        assert int(got["D"]) == nports * nsym and int(got["free_mask"]) == fm and int(got["F"]) == bin(fm).count("1"), (nports, nsym, mask)
        want = R.default_threshold(nports * nsym, bin(fm).count("1"), len(hyp), bool(known))
        assert abs(float(got["threshold"]) - want) <= 1e-6 * want, (nports * nsym, bin(fm).count("1"), len(hyp), known, float(got["threshold"]), want)
        assert float(info_of(p, threshold=2.5)["threshold"]) == 2.5
    assert n == 5 * 12 * len(MASKS) * 2 and 0 < refused < n // 4


def test_the_hypothesis_tables():
    assert [X.hypotheses_mcs(a, s) for a, s in UCI] == [(0, 6), (0, 3, 6, 9), (0,), (0, 6, 3, 9), (0, 3, 6, 9, 1, 4, 7, 10)]
    got = info_of(X.pdu(ics=7, nharq=2, nsr=1))
    assert int(got["nof_hypotheses"]) == 8 and list(got["shifts"]) == [7, 10, 1, 4, 8, 11, 2, 5]


def refused(text, p, **changes):
    with pytest.raises(Exception) as e:
        info_of(p, **changes)
    assert "error %d" % EINVAL in str(e.value) and text in str(e.value), str(e.value)
    assert text in miphy.lib().miphy_last_error().decode()


def test_the_rules():
    p = X.pdu(2, 2, 1, start=12, prb=3, prb2=9, ics=4, nharq=1, nsr=1, nid=100, slot=19, numerology=1)
    info_of(p)
    refused("the format is not 0", p, format=1)
    refused("outside the frame", p, slot=20)
    refused("outside the frame", p, numerology=5)
    refused("invalid number of receive ports", p, nof_ports=5)
    refused("invalid number of receive ports", p, nof_ports=0)
    refused("invalid symbol range", p, nof_symbols=3)
    refused("invalid symbol range", p, nof_symbols=0)
    refused("invalid symbol range", p, start_symbol=13)
    refused("invalid symbol range", p, start_symbol=14, nof_symbols=1, intra_slot_hopping=0)
    refused("only with two symbols", p, nof_symbols=1)
    refused("only with two symbols", p, intra_slot_hopping=2)
    refused("the BWP leaves the grid", p, grid_nprb=19)
    refused("the BWP leaves the grid", p, grid_nprb=276, bwp_size_rb=276)
    refused("the allocation leaves the BWP", p, starting_prb=20)
    refused("the allocation leaves the BWP", p, second_hop_prb=20)
    info_of(p, second_hop_prb=20, intra_slot_hopping=0)  # not read without hopping
    refused("initial_cyclic_shift is 0..11", p, initial_cyclic_shift=12)
    refused("nof_harq_ack is 0..2", p, nof_harq_ack=3)
    refused("nof_harq_ack is 0..2", p, nof_sr=2)
    refused("no UCI bits", p, nof_harq_ack=0, nof_sr=0)
    refused("used_shifts_mask", p, used_shifts_mask=0x1000)
    refused("n_id is 0..1023", p, n_id=1024)
    refused("no free cyclic shift to estimate the noise from", p, used_shifts_mask=0xfff)
    assert int(info_of(p, used_shifts_mask=0xfff, noise_var=0.5)["F"]) == 0
    for field in ("threshold", "noise_var"):
        for bad in (-1.0, np.inf, np.nan):
            refused("finite and not negative", p, **{field: bad})
    with pytest.raises(Exception, match="null argument"):
        miphy.binding.check(miphy.lib().miphy_pucch_f0_info(None, None))


def test_record_sizes_against_the_header():
    hdr = open(os.path.join(ROOT, "include", "miphy.h")).read()
    sizes = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8, "float": 4}
    for name, dtype in (("miphy_pucch_f0_job", miphy.PucchF0Job), ("miphy_pucch_f0_info_t", miphy.PucchF0Info)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            m = re.match(r"\s*(uint\d+_t|float)\s+(.*)", decl.strip(), flags=re.S)
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
            assert dtype.fields[fname][0].base.itemsize == sizes[ctype] and (dtype.fields[fname][0].base.kind == "f") == (ctype == "float"), (name, fname)
            off += sizes[ctype] * count
        assert -(-off // 8) * 8 == dtype.itemsize or off == dtype.itemsize, (name, off, dtype.itemsize)
    assert miphy.PucchF0Job.itemsize == 64 and miphy.PucchF0Info.itemsize == 28
