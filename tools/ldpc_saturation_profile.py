"""After which iteration do the rows of the packed LDPC decoder saturate on the headline workload, and how many of a codeblock's layer
visits does the skip of saturated rows (csrc/ldpc_decode_pk.hip) leave out?
  python tools/ldpc_saturation_profile.py [--slots 2] [--max-iter 6] [--snr-db 33]        (on the GPU)
  python tools/ldpc_saturation_profile.py --model                                         (CPU model of one transport block)
Default: the bench's own front end runs on the device for a few slots (a child `bench.py --slots S --steps 1 --warmup 0 --dump-outputs`:
OFDM demodulation, channel estimate, demodulator, and the decoder that dematches while it loads), and the HARQ soft buffers it leaves -- at
up to two slots the dump holds every byte of them -- are the dematched LLRs of every codeblock as the decoder saw them. The committed
oracle then decodes each with o_ldpc_decode(..., want_soft) for 0 .. max_iter - 1 iterations. A (wavefront, layer) pair is saturated at
the visit of the first iteration that STARTS with all the soft bits its rows read infinite (|s| > 120) and left out in every iteration
behind it; the layers before it in the iteration before may have finished the job earlier, so these counts are lower bounds.
The EXACT counts come from the per-visit model (tests/ldpc_visit_model.py: the oracle's decoder one visit at a time, leaving visits out as
the kernel does) under both rules: "input" = a pair goes quiet behind a visit that READ infinite soft bits only, "output" = behind a
visit that WROTE infinite soft bits only (the kernel's rule, update_rows_pk<..., DETECT>).
--model: o_pdsch_encode -> o_modulate -> AWGN -> o_demodulate_soft -> o_rate_dematch instead of the device front end."""
import argparse, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran_project_23.5_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from ldpc_saturation_model import infinite, left_out, nof_waves, saturated_from  # noqa: E402
from ldpc_visit_model import visits_left_out, visits_of  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--snr-db", type=float, default=33.0)
ap.add_argument("--max-iter", type=int, default=6)
ap.add_argument("--slots", type=int, default=2)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--model", action="store_true")
a = ap.parse_args()
BG, MOD, NSYM, TBS = 1, 8, 273 * 156, 319784  # bench.py, pusch_workload
seg = O.o_segmentation(TBS, BG, MOD, 1, NSYM)
Z, ncb, lay, nf = seg.Z, seg.nof_cbs, 4, seg.nof_filler_bits
if a.model:
    rng = np.random.default_rng(a.seed)
    cw = O.o_pdsch_encode(BG, 0, MOD, 0, 1, NSYM, rng.integers(0, 256, TBS // 8, dtype=np.uint8))
    nv = 10.0 ** (-a.snr_db / 10.0)
    sym = O.o_modulate(MOD, cw) + (np.sqrt(nv / 2) * (rng.standard_normal(NSYM) + 1j * rng.standard_normal(NSYM))).astype(np.complex64)
    llr = O.o_demodulate_soft(MOD, sym, np.full(NSYM, nv, np.float32))
    images = [O.o_rate_dematch(0, MOD, 0, nf, 1, llr[seg.cw_offset[c]:seg.cw_offset[c] + seg.E[c]], np.zeros(seg.N, np.int8)) for c in range(ncb)]
else:
    assert a.slots <= 2, "the bench dumps a sample of the soft buffers above two slots"
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--slots", str(a.slots), "--steps", "1", "--warmup", "0", "--max-iter", str(a.max_iter),
                        "--snr-db", str(a.snr_db), "--dump-outputs", d], check=True, stdout=subprocess.DEVNULL)
        soft = np.load(os.path.join(d, "harq_soft_buffer_sample.npy")).astype(np.int8)
        assert (np.load(os.path.join(d, "codeblock_crc_ok.npy")) == 1).all()
    assert soft.size % (a.slots * ncb) == 0 and soft.size // (a.slots * ncb) >= seg.N, soft.size
    images = list(soft.reshape(a.slots * ncb, -1)[:, :seg.N])
allin = np.concatenate([im[:24 * Z] for im in images]).astype(np.int32)
print("%s: Z %d, %d codeblocks, %.2f %% of the received soft bits at +-120, largest %d" % ("CPU model" if a.model else "device front end", Z, len(images),
                                                                                        100.0 * np.mean(np.abs(allin[allin != 127]) == 120), np.abs(allin[allin != 127]).max()))
waves, visits, total = nof_waves(Z), visits_of(lay, a.max_iter), 0  # (iteration 0 starts at layer 1)
exact = {"input": 0, "output": 0}
for c, image in enumerate(images):
    snaps = [np.concatenate([np.zeros(2 * Z, np.int8), image])] + [O.o_ldpc_decode(BG, Z, image, nf, -1, k, want_soft=True)[2] for k in range(1, a.max_iter)]
    sat = saturated_from(snaps, Z, lay)
    out = left_out(sat, a.max_iter)
    skipped = [sum(v for (w, m), v in out.items() if w == ww) for ww in range(waves)]
    total += sum(skipped)
    by_rule = {rule: visits_left_out(Z, image[:seg.N], lay, a.max_iter, rule) for rule in exact}
    for rule in exact:
        exact[rule] += int(by_rule[rule].sum())
    if c < 6 or c % 19 == 0:
        print("cb %3d finite soft bits at the start of iterations 0.. %s | saturated from iteration (wavefront x layer) %s | visits left out per wavefront %s of %d"
              % (c, [int((~infinite(s[:(22 + lay) * Z])).sum()) for s in snaps], [[sat[(w, m)] for m in range(lay)] for w in range(waves)], skipped, visits))
        print("       exact, per wavefront: input rule %s, output rule %s" % (by_rule["input"].tolist(), by_rule["output"].tolist()))
pairs = len(images) * waves
print("visits left out, lower bound from iteration boundaries: %.2f of %d per wavefront (%.1f %%), %d codeblocks" % (total / pairs, visits, 100.0 * total / (pairs * visits), len(images)))
for rule in ("input", "output"):
    print("visits left out, exact, %-6s rule: %.2f of %d per wavefront (%.1f %%)" % (rule, exact[rule] / pairs, visits, 100.0 * exact[rule] / (pairs * visits)))
print("visits that run, output rule against input rule: %.2f -> %.2f per wavefront (%.1f %%)" % (
    visits - exact["input"] / pairs, visits - exact["output"] / pairs, 100.0 * (exact["input"] - exact["output"]) / (pairs * visits - exact["input"])))
