"""PUCCH format 0 transmitter and channel, restated in numpy float64 from TS 38.211 6.3.2.3 (the sequence x(n) = r_u^(alpha)(n) on the 12 REs
of one PRB, one or two symbols) with the cyclic shift alpha of 6.3.2.2.2 and the m_cs of TS 38.213 9.2.3; normal cyclic prefix, no group or
sequence hopping (u = n_id mod 30, v = 0). The 23.5 reference neither sends nor receives this format; miphy_pucch_process_f0_batch is checked
against this transmitter composed with tests/pucch_f0_ref.py.

A PDU is a dict: numerology, slot, nports, start, nsym (1 / 2), hop (0 / 1), bwp_start, bwp_size, prb, prb2, ics, nharq (0..2), nsr (0 / 1),
mask (used_shifts_mask), nid, grid_nprb, threshold, noise_var (0 = default / estimate). What a UE sends is the index of a hypothesis in the
table order of hypotheses_mcs(), or None for nothing (DTX; a negative SR alone)."""
import numpy as np

import pucch_tx as T

MCS_HARQ = {1: (0, 6), 2: (0, 3, 6, 9)}  # one bit: 0, 1; two bits (b0, b1): (0,0), (0,1), (1,1), (1,0)
MCS_HARQ_SR = {1: (3, 9), 2: (1, 4, 7, 10)}  # the same with a positive SR
BITS_HARQ = {1: ((0,), (1,)), 2: ((0, 0), (0, 1), (1, 1), (1, 0))}


def hypotheses_mcs(nharq, nsr):
    """m_cs of every hypothesis in table order: H = 1, 2, 4, 4 or 8 of them."""
    if nharq == 0:
        assert nsr == 1
        return (0,)
    return MCS_HARQ[nharq] + (MCS_HARQ_SR[nharq] if nsr else ())


def hypothesis_bits(nharq, nsr, i):
    """The payload bytes of hypothesis i: the HARQ-ACK bits, then the SR bit."""
    if nharq == 0:
        return [1]
    n = len(MCS_HARQ[nharq])
    return list(BITS_HARQ[nharq][i % n]) + ([i // n] if nsr else [])


def hop_prbs(p):
    """Absolute PRB of each symbol of the PDU."""
    return [p["bwp_start"] + (p["prb2"] if (l == 1 and p["hop"]) else p["prb"]) for l in range(p["nsym"])]


def base_sequence(u):
    return np.exp(0.25j * np.pi * T.PHI12[u])


def pdu_symbols(p, hyp):
    """Transmitted REs of one PDU sending hypothesis `hyp`: list of (symbol, first subcarrier, 12 values)."""
    m_cs = hypotheses_mcs(p["nharq"], p["nsr"])[hyp]
    r = base_sequence(p["nid"] % 30)
    out = []
    for l, prb in enumerate(hop_prbs(p)):
        a = T.alpha_index(p["nid"], p["slot"], p["start"] + l, p["ics"] + m_cs)
        out.append((p["start"] + l, 12 * prb, r * np.exp(2j * np.pi * a * np.arange(12) / 12)))
    return out


def build_grid(seed, nports, grid_nprb, noise_std, pdus, hyps, gains_db=None):
    """The received grid of PDUs that share a slot: every transmitting PDU goes through a channel that is flat over the PRB, one complex gain
    per port (magnitude between -3 and +3 dB, times gains_db[i] when given; uniform phase), then AWGN of standard deviation noise_std per RE.
    Deterministic in `seed` (numpy PCG64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    grid = np.zeros((nports, 14, 12 * grid_nprb), np.complex128)
    for i, (p, hyp) in enumerate(zip(pdus, hyps)):
        gain = 10 ** (rng.uniform(-3, 3, nports) / 20) * np.exp(2j * np.pi * rng.uniform(0, 1, nports))
        if gains_db is not None:
            gain = gain * 10 ** (gains_db[i] / 20)
        if hyp is None:
            continue
        for l, sc, v in pdu_symbols(p, hyp):
            grid[:, l, sc:sc + 12] += gain[:, None] * v[None, :]
    noise = (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * (noise_std / np.sqrt(2))
    return (grid + noise).astype(np.complex64)


def pdu(nports=1, nsym=1, hop=0, start=0, prb=0, prb2=0, ics=0, nharq=1, nsr=0, mask=0, nid=0, slot=0, numerology=0, grid_nprb=20, threshold=0.0,
        noise_var=0.0):
    """A PDU whose BWP is the whole grid."""
    return dict(numerology=numerology, slot=slot, nports=nports, start=start, nsym=nsym, hop=hop, bwp_start=0, bwp_size=grid_nprb, prb=prb, prb2=prb2,
                ics=ics, nharq=nharq, nsr=nsr, mask=mask, nid=nid, grid_nprb=grid_nprb, threshold=threshold, noise_var=noise_var)


def job_of(p, grid_offset=0, payload_offset=0, energy_offset=0):
    """The miphy.PucchF0Job record of a PDU."""
    import miphy
    j = np.zeros(1, miphy.PucchF0Job)[0]
    j["format"], j["numerology"], j["slot"], j["nof_ports"] = 0, p["numerology"], p["slot"], p["nports"]
    j["start_symbol"], j["nof_symbols"], j["intra_slot_hopping"] = p["start"], p["nsym"], p["hop"]
    j["bwp_start_rb"], j["bwp_size_rb"], j["starting_prb"], j["second_hop_prb"] = p["bwp_start"], p["bwp_size"], p["prb"], p["prb2"]
    j["initial_cyclic_shift"], j["nof_harq_ack"], j["nof_sr"], j["used_shifts_mask"], j["n_id"] = p["ics"], p["nharq"], p["nsr"], p["mask"], p["nid"]
    j["threshold"], j["noise_var"], j["grid_nprb"] = p["threshold"], p["noise_var"], p["grid_nprb"]
    j["grid_offset"], j["payload_offset"], j["energy_offset"] = grid_offset, payload_offset, energy_offset
    return j
