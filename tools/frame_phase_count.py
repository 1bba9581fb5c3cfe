"""Instructions of the packed LDPC decoder's loops OUTSIDE the layer visits, counted in the compiler's assembly (the visits themselves:
tools/visit_valu_count.py).
  hipcc <the Makefile's flags for the file> --cuda-device-only -S csrc/ldpc_decode_pk.hip -o pk.s
  python tools/frame_phase_count.py pk.s [more.s ...]
Per function (every kernel instance, and pk_fused_load, which is not inlined) the innermost loops as the compiler marks them ("Inner Loop
Header" and the blocks "in Loop: Header=" it), without those that hold a layer visit (s_setprio <request>), with the VALU / DS /
vector-memory instructions of their blocks, named by what only that phase issues. A loop whose body branches counts every arm (the blocks
of a loop need not be contiguous in the file).
  staging per vector       global load of 16 input bytes and byte / short stores to LDS (stage_vector; pk_fused_load's loop per modulation order)
  image-out per vector     ds_read_b128 and a 16-byte global store (pk_fused_image_out)
  last non-zero search     ds_read_b128 and a compare, no store: the search from the back of the data (28 VALU per step of 64 vectors; the compiler
                           does not always mark its loop as an inner one: --all lists every loop)
  checksum per word        v_bcnt (crc_zmask_partial; with `dot4 N` the hard decision of hard_word is in the loop: N v_dot4 per trip)
  hard bits per word       stores of one word of hard bits, no v_bcnt (store_hard_words; absent where the checksum's words are kept)
  checksum by division     v_lshlrev / v_xor chains with s_cbranch inside are not innermost: listed as `other`
A kernel lists a loop once per copy the compiler made (verdict every iteration, after the last one, the fallback of store_kept_words).
Trips are not in the assembly: at the headline shape (Z = 384, K = 8448, 192 lanes, E = 8968, 256QAM, 9216 bytes of image) a lane stages about 3
vectors and copies 3 vectors of the image (the other 5.25 of the buffer are a store of zeros); of the 264 words two wavefronts take 2 trips of
the checksum and of the output, the third one."""
import re, sys

REQ = 3  # LDPC_PK_SETPRIO: the priority that opens a layer visit


def functions(txt):
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.M | re.S):
        yield m.group(1), m.group(2).split("\n")


def loops(body):
    """The innermost loops as the compiler marks them: the block that is an 'Inner Loop Header' and every block 'in Loop: Header=' it
    (the blocks of a loop need not be contiguous: the byte form of a bit plane is laid out behind the loop it belongs to)."""
    owner, cur, out = {}, None, []
    for i, ln in enumerate(body):
        m = re.match(r"^\.L(BB\d+_\d+):(.*)", ln)
        if m:
            note, k = m.group(2), i + 1
            while k < len(body) and re.match(r"^\s+;", body[k]):  # (the comment of a block in a nest runs over several lines)
                note, k = note + body[k], k + 1
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            cur = m.group(1) if "Inner Loop Header" in note else (h.group(1) if h else None)
            if "Inner Loop Header" in note:
                out.append(cur)
            continue
        if cur is not None:
            owner.setdefault(cur, []).append(ln)
    return [owner.get(h, []) for h in out]


def describe(ops):
    n = lambda *p: sum(1 for o in ops if o.startswith(p))
    valu, ds, vmem = n("v_"), n("ds_"), n("global_", "buffer_", "flat_", "scratch_")
    gl, gs16, gs = n("global_load_dwordx4", "flat_load_dwordx4"), n("global_store_dwordx4"), n("global_store_dword", "global_store_byte", "flat_store")
    if n("v_bcnt"):
        kind = "checksum per word" + (" (dot4 %d: with the hard decision)" % n("v_dot4") if n("v_dot4") else "")
    elif gl and n("ds_write_b8", "ds_write_b16", "ds_write_b32"):
        kind = "staging per vector (%d ds_write_b8, %d wider)" % (n("ds_write_b8"), n("ds_write_b16", "ds_write_b32"))
    elif gs16 and n("ds_read_b128"):
        kind = "image-out per vector"
    elif n("ds_read_b128") and not gs and not gs16 and n("v_cmp"):
        kind = "last non-zero search"
    elif gs and not gs16 and (n("v_dot4") or n("ds_read")):
        kind = "hard bits per word"
    else:
        kind = "other"
    return kind, valu, ds, vmem, n("scratch_")


def main(path):
    txt = open(path).read()
    print("==", path)
    for name, body in functions(txt):
        if "ldpc_decode_pk" not in name and "pk_fused_load" not in name:
            continue
        short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:44]
        rows = []
        for lines in loops(body):
            ops = [ln.split()[0] for ln in lines if ln.startswith("\t") and ln.strip() and ln.strip()[0] not in ".;"]
            if any(re.match(r"\s+s_setprio %d\b" % REQ, ln) for ln in lines):
                continue
            kind, valu, ds, vmem, scr = describe(ops)
            if kind != "other" or "--all" in sys.argv:
                rows.append("   %-58s VALU %3d  DS %2d  vector memory %2d (scratch %d)" % (kind, valu, ds, vmem, scr))
        total = sum(1 for ln in body if ln.startswith("\tv_"))
        print("%s  VALU instructions in all %d" % (short, total))
        for r in rows:
            print(r)


if __name__ == "__main__":
    for p in sys.argv[1:]:
        if not p.startswith("--"):
            main(p)
