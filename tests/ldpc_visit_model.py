"""The layered LDPC decoder one layer visit at a time, in numpy, with the two tests for saturated rows of the packed kernel
(csrc/ldpc_pk_device.h, update_rows_pk<..., DETECT>; the argument is DESIGN.md section 4) and a simulation that leaves visits out under
a given rule. Shared by tests/test_ldpc_output_saturation*.py and tools/ldpc_saturation_profile.py; BG1 and even Z only.

The arithmetic is the oracle's (oracle/phy_oracle.c, orc_ldpc_decode): with no rule the soft bits equal o_ldpc_decode(..., want_soft)
byte for byte at every iteration boundary. Rows, lanes and wavefronts are those of ldpc_saturation_model: lane l owns check rows l and
l + Z / 2 of every layer, wavefront w the lanes 64 w .. 64 w + 63, and a wavefront keeps one sticky bit per layer, which changes only at
its own general visits of that layer.

A rule maps the figures of a visit (`Visit`) to one flag per row, "this row's later visits change nothing":
  reads_infinite    every soft bit the row READ is infinite (|s| > 120) -- the rule the kernel started with;
  writes_infinite   every soft bit the row WRITES is infinite, tested on the written values themselves;
  closed_form       the same without per-edge work, from the two smallest |v| clipped at 120 (min1 <= min2), their scaled values s1, s2
                    and the parity of the signs: reads_infinite, or the parity is even and min(min1 + s2, min2 + s1) >= 121;
  device_form       closed_form as the kernel merges it into one comparison (min1u = the unclipped first minimum of the kernel's v,
                    where an infinite soft bit gives |v| >= 135): min(min1u + s2 - 109 [parity odd], min2 + s1) >= 121;
  no_parity         closed_form with the parity term dropped -- WRONG, for the tests that a rule which forgets it is caught."""
import numpy as np

from ldpc_saturation_model import nof_waves, row_reads, wave_rows

LLR_MAX, LLR_INF, INF_MUL = 120, 127, 255
S_INF_MIN = LLR_MAX + 1        # the smallest magnitude of an infinite soft bit
V_INF_MIN = INF_MUL - LLR_MAX  # the smallest |v| of the kernel for an infinite soft bit
ODD_PARITY_DROP = V_INF_MIN + ((LLR_MAX * 52428) >> 16) - S_INF_MIN  # 109, csrc/ldpc_pk_device.h: odd parity passes exactly at min1u >= 135


def scaled(a):
    """0.8 a as the decoder computes it, for 0 <= a <= 120."""
    return (a * 52428) >> 16


def layers_decoded(Z, image):
    """The layers the oracle visits for a dematched image (trailing zeros do not count): orc_ldpc_decode, cb_len."""
    nz = np.flatnonzero(image)
    last = int(nz[-1]) + 1 if nz.size else 0
    cb_len = max(last + 2 * Z, 26 * Z)
    return -(-cb_len // Z) - 22


class Visit:
    """One layer visit of some rows: what they read and write, and the figures the rules are made of (one entry per row)."""

    def __init__(self, soft, c2v, first):
        s = soft.astype(np.int32)
        sc = np.clip(s, -LLR_MAX, LLR_MAX)
        if first:  # no message of the layer exists yet: the raw soft bit
            v = s
            t = sc
        else:  # ldpc_decoder_avx2.cpp:85-105; every |s| > 120 is infinite, as in the kernel (the decoder itself stores +-127 only)
            t = np.clip(sc - c2v, -LLR_MAX, LLR_MAX)
            v = np.where(s > LLR_MAX, LLR_INF, np.where(s < -LLR_MAX, -LLR_INF, t))
        a = np.abs(v)
        ac = np.minimum(a, LLR_MAX)
        idx = np.argmin(ac, axis=1)  # the first edge that holds the minimum
        rows = np.arange(ac.shape[0])
        self.min1 = ac[rows, idx]
        rest = ac.copy()
        rest[rows, idx] = LLR_MAX
        self.min2 = rest.min(axis=1)
        self.s1, self.s2 = scaled(self.min1), scaled(self.min2)
        neg = v < 0
        self.odd = (neg.sum(axis=1) & 1).astype(bool)
        mag = np.repeat(self.s1[:, None], ac.shape[1], axis=1)
        mag[rows, idx] = self.s2
        self.c2v = np.where(neg ^ self.odd[:, None], -mag, mag)
        r = self.c2v + v  # ldpc_decoder_avx2.cpp:205-243 (a message is never infinite)
        self.soft = np.where((r > LLR_MAX) | (v > LLR_MAX), LLR_INF, np.where((r < -LLR_MAX) | (v < -LLR_MAX), -LLR_INF, r)).astype(np.int8)
        self.read_infinite = np.abs(s) > LLR_MAX
        # the kernel's v = 255 (s - clip(s)) + t: |v| <= 120 for a finite soft bit, >= 135 for an infinite one
        self.min1u = np.abs(INF_MUL * (s - sc) + t).min(axis=1)

    def reads_infinite(self):
        return self.read_infinite.all(axis=1)

    def writes_infinite(self):
        return (np.abs(self.soft.astype(np.int32)) > LLR_MAX).all(axis=1)

    def lowest_output(self):
        return np.minimum(self.min1 + self.s2, self.min2 + self.s1)

    def closed_form(self):
        return self.reads_infinite() | (~self.odd & (self.lowest_output() >= S_INF_MIN))

    def device_form(self):
        return np.minimum(self.min1u + self.s2 - ODD_PARITY_DROP * self.odd, self.min2 + self.s1) >= S_INF_MIN

    def no_parity(self):
        return self.reads_infinite() | (self.lowest_output() >= S_INF_MIN)


RULES = {"input": Visit.reads_infinite, "output": Visit.closed_form, "written": Visit.writes_infinite, "device": Visit.device_form,
         "no_parity": Visit.no_parity}


def visits_of(layers, max_iter):
    """Visits of a wavefront in a decode that runs all its iterations: the kernel does not visit layer 0 in iteration 0 (both punctured
    columns are zero there: every message zero, no soft bit changes)."""
    return layers * max_iter - 1


def decode(Z, image, layers, max_iter, rule=None, each_visit=None, each_iteration=None):
    """Decode one codeblock (image = the dematched soft bits behind the two punctured columns) for max_iter iterations without a CRC.
    rule: a key of RULES, or None to run every visit. A wavefront whose rows ALL pass the rule at a visit of layer m leaves out its later
    visits of layer m. each_visit(it, m, rows, Visit) is called for every visit that runs, each_iteration(it, soft) behind every iteration.
    -> (hard bits packed MSB first, visits run per wavefront -- of visits_of(layers, max_iter))."""
    assert Z % 2 == 0 and image.size <= 66 * Z and not (image == -128).any()
    soft = np.zeros(68 * Z, np.int8)
    soft[2 * Z:2 * Z + image.size] = image
    reads = row_reads(Z, layers)
    c2v = [np.zeros(reads[m].shape, np.int32) for m in range(layers)]
    waves = [wave_rows(Z, w) for w in range(nof_waves(Z))]
    dead = np.zeros((len(waves), layers), bool)
    run = np.zeros(len(waves), np.int64)
    test = RULES[rule] if rule is not None else None
    for it in range(max_iter):
        for m in range(layers):
            for w, rows in enumerate(waves):
                if dead[w, m]:
                    continue
                pos = reads[m][rows]
                vis = Visit(soft[pos], c2v[m][rows], it == 0)
                soft[pos] = vis.soft  # (the rows of a layer read disjoint soft bits)
                c2v[m][rows] = vis.c2v
                run[w] += not (it == 0 and m == 0)
                if test is not None and test(vis).all():
                    dead[w, m] = True
                if each_visit is not None:
                    each_visit(it, m, rows, vis)
        if each_iteration is not None:
            each_iteration(it, soft.copy())
    return np.packbits(soft[:22 * Z] <= 0), run


def visits_left_out(Z, image, layers, max_iter, rule):
    """Per wavefront the visits a decode of max_iter iterations leaves out under the rule."""
    return visits_of(layers, max_iter) - decode(Z, image, layers, max_iter, rule)[1]
