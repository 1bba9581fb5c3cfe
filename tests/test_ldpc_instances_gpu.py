"""GPU: every instance of the LDPC decoder kernels the library compiles -- the twelve of the packed kernel (csrc/ldpc_decode_pk.hip,
pk_instances: {dematches while it loads, messages in global memory, parts, address table, leaves out saturated rows}) and the two of the
wave kernel (csrc/ldpc_decode_pkw.hip: messages in LDS / in global memory) -- selected by a smallest batch that selects it, and checked
against the CPU oracle. The selection is proven through the queries the library has: the mask of miphy_debug_ldpc_kernels_used (PACKED /
FUSED / GMSG / SPLIT / WAVE), the launches counted by miphy_debug_ldpc_address_table_launches and miphy_debug_ldpc_row_skip_launches, and
the forced mode itself for the parts of the latency form (four under the automatic choice, two under mode 6). A batch that does not
select its instance fails.

Instances that take plain soft bits run through miphy_ldpc_decode_batch with host descriptors (run_batch of test_ldpc_decode_gpu.py: hard
bits and iteration counts); those that dematch while they load run through a PUSCH decode plan (run_plan of
test_ldpc_address_table_gpu.py / test_ldpc_saturated_rows_gpu.py: hard bits, iteration counts, CRC flags, HARQ soft images, transport
block). One all-zero codeblock sits in a batch of each kind: the kernels leave such a codeblock before its first layer. Transport
blocks and their oracle results are the cached ones of those modules."""
import numpy as np
import pytest

import test_ldpc_address_table_gpu as tab
import test_ldpc_saturated_rows_gpu as sat
from oracle_lib import BG_NS, CRC24B
from test_ldpc_decode_gpu import FUSED, GMSG, PACKED, SCALAR, SPLIT, WAVE, make_codeword, noisy_llr, run_batch

pytestmark = pytest.mark.gpu

AUTO, THROUGHPUT, LATENCY2, NO_TABLE = 0, 4, 6, 0x200  # miphy_debug_force_ldpc_kernel (include/miphy.h)


def counters(lib):
    """(kernels used, launches that read the address table, launches that leave out saturated rows) since the last call."""
    return int(lib.miphy_debug_ldpc_kernels_used(1)), int(lib.miphy_debug_ldpc_address_table_launches(1)), int(lib.miphy_debug_ldpc_row_skip_launches(1))


def plain_cases(bg, Z, nodes_list, crc, zero=False, seed=41):
    """One codeblock per entry of nodes_list (input of that many variable nodes behind the punctured two), and an all-zero one of the
    first length if asked for."""
    rng = np.random.default_rng(seed)
    cases = []
    for k, nodes in enumerate(nodes_list):
        _, cw = make_codeword(bg, Z, rng)
        cases.append(dict(bg=bg, Z=Z, llr=noisy_llr(cw[:nodes * Z], (0.30, 0.45, 0.60)[k % 3], rng), crc=crc, max_iter=6, nf=0))
    if zero:
        cases.append(dict(bg=bg, Z=Z, llr=np.zeros(nodes_list[0] * Z, np.int8), crc=crc, max_iter=6, nf=0))
    return cases


# Z = 384, 4, 5 and 6 layers (inputs of K / Z + 2, + 3, + 4 nodes), i.e. two launch classes (the layer buckets "up to 4" and "up to 6").
# Base graph 1 for the latency form. The throughput geometry (mode 4) moves the messages of such BG1 codeblocks to global memory
# (41 KB of LDS each: three per CU where the registers allow five), so the two throughput instances with their messages in LDS take the
# same layers of base graph 2 (19 to 24 KB).
HIGH_RATE, HIGH_RATE_BG2 = (24, 25, 26), (12, 13, 14)
# name: (cases, mode, kernel bits that must be set, bits that must be clear, launches that leave out saturated rows)
PLAIN = {
    "pk<0,0,1,0,0> plain": (lambda: plain_cases(2, 384, HIGH_RATE_BG2, CRC24B, zero=True), THROUGHPUT, PACKED, FUSED | GMSG | SPLIT | WAVE, 0),
    "pk<0,0,1,0,1> plain, row skip": (lambda: plain_cases(2, 384, HIGH_RATE_BG2, -1, zero=True), THROUGHPUT, PACKED, FUSED | GMSG | SPLIT | WAVE, 2),
    "pk<0,0,4> four parts": (lambda: plain_cases(1, 384, HIGH_RATE, CRC24B), AUTO, PACKED | SPLIT, FUSED | GMSG | WAVE, 0),
    "pk<0,0,2> two parts": (lambda: plain_cases(1, 384, HIGH_RATE, CRC24B), LATENCY2, PACKED | SPLIT, FUSED | GMSG | WAVE, 0),
    "pk<0,1,1> global messages": (lambda: plain_cases(1, 384, (66, 66), CRC24B), THROUGHPUT, PACKED | GMSG, FUSED | SPLIT | WAVE, 0),
    "pkw<0> messages in LDS": (lambda: plain_cases(2, 64, (12, 12, 13), -1, zero=True), THROUGHPUT, WAVE, PACKED | GMSG, 0),
    "pkw<1> global messages": (lambda: plain_cases(1, 60, (BG_NS[1], BG_NS[1]), CRC24B, zero=True), THROUGHPUT, WAVE | GMSG, PACKED, 0),
}


@pytest.mark.parametrize("name", list(PLAIN))
def test_instances_that_take_soft_bits(ctx, name):
    import miphy
    lib = miphy.lib()
    make, mode, must, must_not, row_skip_launches = PLAIN[name]
    cases = make()
    lib.miphy_debug_force_ldpc_kernel(mode)
    try:
        counters(lib)
        bad = run_batch(ctx, cases)
    finally:
        lib.miphy_debug_force_ldpc_kernel(0)
    # (run_batch reads and clears the kernel mask itself when given a mode to check; without one the mask is still there)
    used, table, skip = counters(lib)
    print(name, "used", hex(used), "table launches", table, "row-skip launches", skip)
    assert used & must == must and not used & (must_not | SCALAR), hex(used)
    assert (table, skip) == (0, row_skip_launches), (table, skip)
    assert not bad, bad[:5]


Z384 = ("z384", tab.SIGMAS[4], 100, -1)             # three codeblocks, four layers: passes after two, about four, no iterations
Z384_ZERO = ("z384", (0.30, 0.40, 0.35), 401, 1)   # ... the middle one not received at all
# name: (transport blocks, early stop, mode, kernel bits set, bits clear, table launches, row-skip launches)
DEMATCHED = {
    "pk<1,0,1,1,0> table": ((Z384,), True, THROUGHPUT, PACKED | FUSED, GMSG | SPLIT, 1, 0),
    "pk<1,0,1,1,1> table, row skip": ((Z384,), False, THROUGHPUT, PACKED | FUSED, GMSG | SPLIT, 1, 1),
    "pk<1,0,1,0,0> fused": ((Z384, Z384_ZERO), True, THROUGHPUT | NO_TABLE, PACKED | FUSED, GMSG | SPLIT, 0, 0),
    "pk<1,0,1,0,1> fused, row skip": ((Z384,), False, THROUGHPUT | NO_TABLE, PACKED | FUSED, GMSG | SPLIT, 0, 1),
    "pk<1,0,4> fused, four parts": ((Z384,), True, AUTO, PACKED | FUSED | SPLIT, GMSG, 0, 0),
    "pk<1,0,2> fused, two parts": ((Z384,), True, LATENCY2, PACKED | FUSED | SPLIT, GMSG, 0, 0),
}


@pytest.mark.parametrize("name", list(DEMATCHED))
def test_instances_that_dematch(ctx, name):
    import miphy
    lib = miphy.lib()
    tbs, early_stop, mode, must, must_not, table_launches, row_skip_launches = DEMATCHED[name]
    counters(lib)
    got, table = tab.run_plan(ctx, tbs, 6, early_stop, mode)
    used, _, skip = counters(lib)
    print(name, "used", hex(used), "table launches", table, "row-skip launches", skip)
    assert used & must == must and not used & (must_not | SCALAR | WAVE), hex(used)
    assert (table, skip) == (table_launches, row_skip_launches), (table, skip)
    tab.check_against_oracle(tbs, got, 6, early_stop, name)
    if Z384_ZERO in tbs:  # the codeblock that was not received fails, its neighbours pass
        assert got[1][2].tolist() == [1, 0, 1] and not got[1][0]["tb_crc_ok"]


def test_instance_that_dematches_with_global_messages(ctx):
    """pk<1,1,1>: one transport block at rate 1/3 reaches all 46 layers, and the throughput geometry moves its messages to global memory."""
    t = ("z384_rate_one_third", sat.SIGMA, 100, -1)
    got, table, used = sat.run_plan(ctx, (t,), 6, True, THROUGHPUT)
    print("pk<1,1,1> used", hex(used), "table launches", table)
    assert used & (PACKED | FUSED | GMSG) == PACKED | FUSED | GMSG and not used & (SPLIT | SCALAR | WAVE | sat.ROWSKIP), hex(used)
    assert table == 0
    sat.check_against_oracle((t,), got, 6, True, "pk<1,1,1>")
    assert got[0][0]["tb_crc_ok"]
