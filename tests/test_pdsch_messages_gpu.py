"""GPU (host validation needs a context; nothing is enqueued): the complete error message of the three layered modulator entry points and the three
layered PDSCH processors for a host batch in which one job breaks a rule -- one rule of every family the entry point checks (a field of the job, a
port, the bit count, the list as a whole, an entry of the list, the precoding), and jobs that break two families at once, which report the earlier
one: the order per job is job, list, precoding, and per batch the first bad job. The other rule tests match substrings; this one pins the prefix
("<entry point>: job <i>: " / "<entry point>: PDU <i>: ") and the arguments too, and that the grid keeps its background.

The expected strings are literals, recorded from a run of these same cases against the library as it was before the three entry points were folded
into one path (the parent of the commit that added this module), not taken from the code under test.

The processors derive the bit count of a PDU themselves, so no PDU can break that rule; their third family is what the encoder accepts instead."""
import numpy as np
import pytest

import dl_grid as D
import pdsch_layers_cases as PC
import pdsch_mapped_cases as MC
import pdsch_precoded_cases as XC
import test_pdsch_mapped_gpu as TM
import test_pdsch_precoded_gpu as TX
from test_pdsch_layers import mod_layers_job
from test_pdsch_layers_gpu import _buffers

pytestmark = pytest.mark.gpu
LC = {c["name"]: c for c in PC.cases()}
MCS = {c["name"]: c for c in MC.cases()}


# ---------------------------------------------------------------------------------------------------- the batches: three jobs, job 1 is the one to break
def _layers_batch(miphy):
    """sweep_L3_mod6, sweep_L2_mod4, sweep_L4_mod8 of pdsch_layers_cases: PRBs 1, 2, 4 of six over three symbols."""
    cases = [LC["sweep_L3_mod6"], LC["sweep_L2_mod4"], LC["sweep_L4_mod8"]]
    grids, cw, goff, coff = _buffers(cases)
    jobs = np.array([mod_layers_job(miphy, c, cw_off=co, grid_off=go) for c, go, co in zip(cases, goff, coff)], dtype=miphy.PdschModLayersJob)
    return dict(jobs=jobs, lists=None, w=None, grids=grids, cw=cw)


def _mapped_batch(miphy):
    """sweep_L1_mod2, sweep_L2_mod4, sweep_L4_mod8 of pdsch_mapped_cases: the list [0 1 4 5 2 3 6 7] on a grid of eight PRBs."""
    jobs, lists, grids, cw = TM._jobs(miphy, [MCS["sweep_L1_mod2"], MCS["sweep_L2_mod4"], MCS["sweep_L4_mod8"]])
    return dict(jobs=jobs, lists=lists, w=None, grids=grids, cw=cw)


def _precoded_batch(miphy):
    """The mapped batch behind precodings onto 2, 4 and 8 antenna ports with PRGs of 4 PRBs."""
    pcs = [XC.precoded(MCS["sweep_L1_mod2"], 2, 4), XC.precoded(MCS["sweep_L2_mod4"], 4, 4, tag="_msg"), XC.precoded(MCS["sweep_L4_mod8"], 8, 4)]
    jobs, lists, w, grids, cw = TX._jobs(miphy, pcs)
    return dict(jobs=jobs, lists=lists, w=w, grids=grids, cw=cw)


def _call_modulator(ctx, entry, b):
    """The host batch b through the entry point; returns (error text or None, whether every grid still holds the bits of its background)."""
    import torch
    gd = torch.from_numpy(np.concatenate(b["grids"])).cuda()
    cw = torch.from_numpy(b["cw"]).cuda()
    err = None
    try:
        if entry == "layers":
            ctx.pdsch_modulate_layers_batch(b["jobs"], cw, gd)
        elif entry == "mapped":
            ctx.pdsch_modulate_mapped_batch(b["jobs"], b["lists"], cw, gd)
        else:
            ctx.pdsch_modulate_precoded_batch(b["jobs"], b["lists"], b["w"], cw, gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return err, np.array_equal(D.bits(gd.cpu().numpy()), D.bits(np.concatenate(b["grids"])))


# the parts of job i of a batch, whatever its kind
def _layers(b, i=1):
    j = b["jobs"][i]
    return j["mapped"]["layers"] if "mapped" in j.dtype.names else (j["layers"] if "layers" in j.dtype.names else j)


def _mapped(b, i=1):
    j = b["jobs"][i]
    return j["mapped"] if "mapped" in j.dtype.names else j


def _set_base(field, value, i=1):
    return lambda b: _layers(b, i)["base"].__setitem__(field, value)


def _more_bits(b):
    _layers(b)["base"]["nof_bits"] = int(_layers(b)["base"]["nof_bits"]) + 1


def _share_port(b):
    _layers(b)["ports"][1] = _layers(b)["ports"][0]


def _port_16(b):
    _layers(b)["ports"][1] = 16


def _five_layers(b):
    _layers(b)["nof_layers"] = 5


def _list_short(b):
    _mapped(b)["nof_prb"] = int(_mapped(b)["nof_prb"]) - 1


def _list_beyond_array(b):
    _mapped(b)["prb_list_offset"] = b["lists"].size - int(_mapped(b)["nof_prb"]) + 1


def _entry_twice(b):
    o = int(_mapped(b)["prb_list_offset"])
    b["lists"][o + 5] = b["lists"][o + 2]  # 4 twice, 3 missing


def _entry_beyond_grid(b):
    b["lists"][int(_mapped(b)["prb_list_offset"]) + 4] = 8


def _pre(field, value, i=1):
    return lambda b: b["jobs"][i]["precoding"].__setitem__(field, value)


def _pre_ports_shared(b):
    b["jobs"][1]["precoding"]["ports"][3] = b["jobs"][1]["precoding"]["ports"][0]


def _pre_weights_beyond(b):
    p = b["jobs"][1]["precoding"]
    p["weights_offset"] = b["w"].size - int(p["nof_prg"]) * int(p["nof_ports"]) * int(p["nof_layers"]) + 1


def _both(*edits):
    return lambda b: [e(b) for e in edits]


# (id, entry point, what to break, the complete message)
MODULATOR = [
    ("layers-field", "layers", _set_base("mod", 3),
     "pdsch_modulate_layers: job 1: invalid modulation order 3"),
    ("layers-field_time", "layers", _set_base("nof_symbols", 0),
     "pdsch_modulate_layers: job 1: invalid time allocation"),
    ("layers-nof_layers", "layers", _five_layers,
     "pdsch_modulate_layers: job 1: invalid number of layers 5 (one codeword: 1..4)"),
    ("layers-port_shared", "layers", _share_port,
     "pdsch_modulate_layers: job 1: layers 0 and 1 share port 0"),
    ("layers-port_16", "layers", _port_16,
     "pdsch_modulate_layers: job 1: invalid port 16 of layer 1"),
    ("layers-bits", "layers", _more_bits,
     "pdsch_modulate_layers: job 1: codeword of 721 bits, the allocation holds 720 on 2 layers"),
    ("layers-port_before_field", "layers", _both(_set_base("mod", 3), _share_port),
     "pdsch_modulate_layers: job 1: layers 0 and 1 share port 0"),
    ("layers-field_before_bits", "layers", _both(_more_bits, _set_base("n_id", 1024)),
     "pdsch_modulate_layers: job 1: invalid scrambling identifiers"),
    ("layers-job_1_before_job_2", "layers", _both(_set_base("mod", 3, i=2), _more_bits),
     "pdsch_modulate_layers: job 1: codeword of 721 bits, the allocation holds 720 on 2 layers"),
    ("mapped-field", "mapped", _set_base("mod", 3),
     "pdsch_modulate_mapped: job 1: invalid modulation order 3"),
    ("mapped-port_shared", "mapped", _share_port,
     "pdsch_modulate_mapped: job 1: layers 0 and 1 share port 0"),
    ("mapped-bits", "mapped", _more_bits,
     "pdsch_modulate_mapped: job 1: codeword of 1921 bits, the allocation holds 1920 on 2 layers"),
    ("mapped-list_count", "mapped", _list_short,
     "pdsch_modulate_mapped: job 1: PRB list of 7 entries for the 8 PRBs of rb_mask"),
    ("mapped-list_beyond_array", "mapped", _list_beyond_array,
     "pdsch_modulate_mapped: job 1: PRB list [26, 26 + 8) exceeds the 33 list entries"),
    ("mapped-entry_twice", "mapped", _entry_twice,
     "pdsch_modulate_mapped: job 1: PRB list entry 5: PRB 4 appears twice"),
    ("mapped-entry_beyond_grid", "mapped", _entry_beyond_grid,
     "pdsch_modulate_mapped: job 1: PRB list entry 4: PRB 8 outside the grid of 8 PRBs"),
    ("mapped-bits_before_list", "mapped", _both(_entry_twice, _more_bits),
     "pdsch_modulate_mapped: job 1: codeword of 1921 bits, the allocation holds 1920 on 2 layers"),
    ("mapped-list_before_entry", "mapped", _both(_entry_twice, _list_short),
     "pdsch_modulate_mapped: job 1: PRB list of 7 entries for the 8 PRBs of rb_mask"),
    ("mapped-job_1_before_job_2", "mapped", _both(_set_base("mod", 3, i=2), _entry_twice),
     "pdsch_modulate_mapped: job 1: PRB list entry 5: PRB 4 appears twice"),
    ("precoded-field", "precoded", _set_base("mod", 3),
     "pdsch_modulate_precoded: job 1: invalid modulation order 3"),
    ("precoded-nof_layers", "precoded", _five_layers,
     "pdsch_modulate_precoded: job 1: invalid number of layers 5 (one codeword: 1..4)"),
    ("precoded-bits", "precoded", _more_bits,
     "pdsch_modulate_precoded: job 1: codeword of 1921 bits, the allocation holds 1920 on 2 layers"),
    ("precoded-list_count", "precoded", _list_short,
     "pdsch_modulate_precoded: job 1: PRB list of 7 entries for the 8 PRBs of rb_mask"),
    ("precoded-entry_twice", "precoded", _entry_twice,
     "pdsch_modulate_precoded: job 1: PRB list entry 5: PRB 4 appears twice"),
    ("precoded-precoding_prg_size", "precoded", _pre("prg_size", 0),
     "pdsch_modulate_precoded: job 1: precoding: invalid PRG size 0 or number of PRGs 2"),
    ("precoded-precoding_layers", "precoded", _pre("nof_layers", 1),
     "pdsch_modulate_precoded: job 1: precoding: 1 layers for a job of 2"),
    ("precoded-precoding_ports_shared", "precoded", _pre_ports_shared,
     "pdsch_modulate_precoded: job 1: precoding: the antenna ports need distinct grid ports below 16"),
    ("precoded-precoding_weights", "precoded", _pre_weights_beyond,
     "pdsch_modulate_precoded: job 1: precoding: weights [77, 77 + 2 x 4 x 2) exceed the 92 weights"),
    ("precoded-field_before_precoding", "precoded", _both(_pre("prg_size", 0), _set_base("dmrs_type", 3)),
     "pdsch_modulate_precoded: job 1: invalid DM-RS type"),
    ("precoded-list_before_precoding", "precoded", _both(_pre("prg_size", 0), _entry_twice),
     "pdsch_modulate_precoded: job 1: PRB list entry 5: PRB 4 appears twice"),
    ("precoded-job_1_before_job_2", "precoded", _both(_set_base("mod", 3, i=2), _pre("nof_prg", 1)),
     "pdsch_modulate_precoded: job 1: precoding: 1 PRGs of 4 PRBs do not reach PRB 7 of rb_mask"),
]
BATCHES = {"layers": _layers_batch, "mapped": _mapped_batch, "precoded": _precoded_batch}


def modulator_message(ctx, k):
    import miphy
    _, entry, edit, _ = MODULATOR[k]
    b = BATCHES[entry](miphy)
    edit(b)
    return _call_modulator(ctx, entry, b)


@pytest.mark.parametrize("k", range(len(MODULATOR)), ids=[m[0] for m in MODULATOR])
def test_modulator_message(ctx, k):
    err, kept = modulator_message(ctx, k)
    print("%s: %r" % (MODULATOR[k][0], err))
    assert err == "miphy error -1: " + MODULATOR[k][3]
    assert kept


# ---------------------------------------------------------------------------------------------------- the processors
def _proc_batch(miphy, entry):
    """The PDUs of tests/test_pdsch_mapped_gpu.py (three: a list of 11 on two layers, a list of 5 on one, none on three) for the layered and the mapped
    processor, those of tests/test_pdsch_precoded_gpu.py (two: a list of 6 on two layers, none on four) for the precoded one."""
    if entry == "precoded":
        rec, lists, w, tb = TX._proc_records(miphy, TX._proc_pdus())
        return dict(rec=rec, lists=lists, w=w, tb=tb, bg=TX._proc_background())
    rec, lists, tb = TM._records(miphy, TM._pdus())
    if entry == "layers":
        rec, lists = np.ascontiguousarray(rec["layers"]), None
    return dict(rec=rec, lists=lists, w=None, tb=tb, bg=TM._grid_background())


def _call_processor(ctx, entry, b):
    import torch
    gd = torch.from_numpy(b["bg"]).cuda()
    tb = torch.from_numpy(b["tb"]).cuda()
    err = None
    try:
        if entry == "layers":
            ctx.pdsch_process_layers_batch(b["rec"], tb, gd)
        elif entry == "mapped":
            ctx.pdsch_process_mapped_batch(b["rec"], b["lists"], tb, gd)
        else:
            ctx.pdsch_process_precoded_batch(b["rec"], b["lists"], b["w"], tb, gd)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    return err, np.array_equal(D.bits(gd.cpu().numpy()), D.bits(b["bg"]))


def _pdu_layers(b, i):
    r = b["rec"][i]
    return r["mapped"]["layers"] if "mapped" in r.dtype.names else (r["layers"] if "layers" in r.dtype.names else r)


def _pdu_mapped(b, i):
    r = b["rec"][i]
    return r["mapped"] if "mapped" in r.dtype.names else r


def _pdu_base(field, value, i=0):
    return lambda b: _pdu_layers(b, i)["base"].__setitem__(field, value)


def _pdu_share_port(b):
    _pdu_layers(b, 0)["ports"][1] = _pdu_layers(b, 0)["ports"][0]


def _pdu_list_short(b):
    _pdu_mapped(b, 0)["nof_prb"] = int(_pdu_mapped(b, 0)["nof_prb"]) - 1


def _pdu_entry_twice(b):
    o = int(_pdu_mapped(b, 0)["prb_list_offset"])
    b["lists"][o + 3] = b["lists"][o + 1]


def _pdu_pre(field, value):
    return lambda b: b["rec"][0]["precoding"].__setitem__(field, value)


def _pdu_pre_ports_shared(b):
    b["rec"][0]["precoding"]["ports"][3] = b["rec"][0]["precoding"]["ports"][0]


# (id, entry point, what to break in PDU 0 -- the one on two layers with a list --, the complete message). The batch is submitted with PDU 0 moved
# behind PDU 1, so the message names PDU 1.
PROCESSOR = [
    ("layers-field", "layers", _pdu_base("mod", 3),
     "pdsch_process_layers: PDU 1: invalid modulation order 3"),
    ("layers-dmrs_mask", "layers", _pdu_base("dmrs_symbols_mask", 0),
     "pdsch_process: PDU 1: invalid DM-RS symbol mask"),
    ("layers-port_shared", "layers", _pdu_share_port,
     "pdsch_process_layers: PDU 1: layers 0 and 1 share port 1"),
    ("layers-encoder", "layers", _pdu_base("rv", 4),
     "pdsch_process_layers: PDU 1: invalid redundancy version"),
    ("layers-port_before_encoder", "layers", _both(_pdu_base("rv", 4), _pdu_share_port),
     "pdsch_process_layers: PDU 1: layers 0 and 1 share port 1"),
    ("mapped-field", "mapped", _pdu_base("mod", 3),
     "pdsch_process_mapped: PDU 1: invalid modulation order 3"),
    ("mapped-dmrs_mask", "mapped", _pdu_base("dmrs_symbols_mask", 0),
     "pdsch_process: PDU 1: invalid DM-RS symbol mask"),
    ("mapped-port_shared", "mapped", _pdu_share_port,
     "pdsch_process_mapped: PDU 1: layers 0 and 1 share port 1"),
    ("mapped-encoder", "mapped", _pdu_base("rv", 4),
     "pdsch_process_mapped: PDU 1: invalid redundancy version"),
    ("mapped-list_count", "mapped", _pdu_list_short,
     "pdsch_process_mapped: PDU 1: PRB list of 10 entries for the 11 PRBs of rb_mask"),
    ("mapped-entry_twice", "mapped", _pdu_entry_twice,
     "pdsch_process_mapped: PDU 1: PRB list entry 3: PRB 13 appears twice"),
    ("mapped-encoder_before_list", "mapped", _both(_pdu_entry_twice, _pdu_base("rv", 4)),
     "pdsch_process_mapped: PDU 1: invalid redundancy version"),
    ("precoded-field", "precoded", _pdu_base("mod", 3),
     "pdsch_process_precoded: PDU 1: invalid modulation order 3"),
    ("precoded-dmrs_mask", "precoded", _pdu_base("dmrs_symbols_mask", 0),
     "pdsch_process: PDU 1: invalid DM-RS symbol mask"),
    ("precoded-encoder", "precoded", _pdu_base("rv", 4),
     "pdsch_process_precoded: PDU 1: invalid redundancy version"),
    ("precoded-list_count", "precoded", _pdu_list_short,
     "pdsch_process_precoded: PDU 1: PRB list of 5 entries for the 6 PRBs of rb_mask"),
    ("precoded-entry_twice", "precoded", _pdu_entry_twice,
     "pdsch_process_precoded: PDU 1: PRB list entry 3: PRB 5 appears twice"),
    ("precoded-precoding_prg_size", "precoded", _pdu_pre("prg_size", 0),
     "pdsch_process_precoded: PDU 1: precoding: invalid PRG size 0 or number of PRGs 8"),
    ("precoded-precoding_ports_shared", "precoded", _pdu_pre_ports_shared,
     "pdsch_process_precoded: PDU 1: precoding: the antenna ports need distinct grid ports below 16"),
    ("precoded-list_before_precoding", "precoded", _both(_pdu_pre("prg_size", 0), _pdu_entry_twice),
     "pdsch_process_precoded: PDU 1: PRB list entry 3: PRB 5 appears twice"),
    ("precoded-encoder_before_list", "precoded", _both(_pdu_entry_twice, _pdu_base("rv", 4)),
     "pdsch_process_precoded: PDU 1: invalid redundancy version"),
]


def processor_message(ctx, k):
    import miphy
    _, entry, edit, _ = PROCESSOR[k]
    b = _proc_batch(miphy, entry)
    edit(b)
    b["rec"][[0, 1]] = b["rec"][[1, 0]]
    return _call_processor(ctx, entry, b)


@pytest.mark.parametrize("k", range(len(PROCESSOR)), ids=[m[0] for m in PROCESSOR])
def test_processor_message(ctx, k):
    err, kept = processor_message(ctx, k)
    print("%s: %r" % (PROCESSOR[k][0], err))
    assert err == "miphy error -1: " + PROCESSOR[k][3]
    assert kept
