"""VALU instructions per layer visit of the packed LDPC decoders, counted in the compiler's assembly.
  hipcc <the Makefile's flags for the file> --cuda-device-only -S csrc/ldpc_decode_pk.hip -o pk.s
  python tools/visit_valu_count.py pk.s [more.s ...]
A visit (update_rows_pk, update_rows_pk_zero) is the code from its `s_setprio <request>` through the first- and second-phase priorities
(ldpc_pk_device.h) to the `s_setprio <first phase>` that ends it, or to the jump to that instruction where the compiler has merged the
tails of the instances of a switch; every instance of a kernel is inlined once, so the static
count of a region is the count a wavefront issues per visit (the stores of the latency form's idle lanes sit under a branch and are
counted as issued). Per kernel: registers, scratch bytes, scratch accesses inside visits; per visit: soft-bit reads (= 2 x edges of the
instance), message reads (0 = a first-visit instance), address-table loads (the instance that reads its soft-bit addresses: the quads of the
next visit, requested in the second phase; their split is counted where the compiler puts it, the request phase), VALU per phase (lane reads and writes, which carry spilled scalar registers, are VALU
instructions and are also shown on their own)."""
import re, sys

REQ, PH1, PH2 = 3, 0, 2  # LDPC_PK_SETPRIO, _SETPRIO1, _SETPRIO2


def visits(lines):
    out, cur, phase = [], None, None
    for ln in lines:
        t = ln.strip()
        if cur is not None and phase == 2 and re.match(r"s_(branch|barrier|setprio %d)\b" % REQ, t):
            out.append(cur)
            cur = None
        m = re.match(r"s_setprio (\d+)", t)
        if m:
            p = int(m.group(1))
            if p == REQ:
                cur, phase = {"valu": [0, 0, 0], "soft_rd": 0, "msg_rd": 0, "scratch": 0, "lane_rd": 0, "tab_rd": 0, "sdwa_add": 0, "pk_add": 0, "pk_mul": 0, "mul24": 0}, 0
            elif cur is not None and p == PH1 and phase == 0:
                phase = 1
            elif cur is not None and p == PH2:
                phase = 2
            elif cur is not None and p == PH1 and phase == 2:
                out.append(cur)
                cur = None
            continue
        if cur is None or not t or t[0] in ".;":
            continue
        op = t.split()[0]
        if op.startswith("v_"):  # (lane reads included: they issue as VALU and SQ_INSTS_VALU counts them)
            cur["valu"][phase] += 1
        cur["lane_rd"] += op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))
        cur["soft_rd"] += op in ("ds_read_i8", "ds_read_u8")
        cur["msg_rd"] += op in ("ds_read_b32", "ds_read2_b32", "ds_read2st64_b32", "global_load_dword")
        cur["scratch"] += op.startswith("scratch_")
        cur["tab_rd"] += op.startswith("buffer_load_dwordx")
        cur["sdwa_add"] += op == "v_add_u32_sdwa"
        cur["pk_add"] += op == "v_pk_add_u16"
        cur["pk_mul"] += op == "v_pk_mul_lo_u16"
        cur["mul24"] += op.startswith("v_mul_u32_u24")
    return out


def main(path):
    txt = open(path).read()
    meta = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)}
    print("==", path)
    for m in re.finditer(r"^(_Z\S*ldpc_decode_pk\S*):[^\n]*\n(.*?)^\s+s_endpgm", txt, re.M | re.S):
        name, body = m.group(1), m.group(2).split("\n")
        scr, vg = meta.get(name, ("?", "?"))
        vs = visits(body)
        print("%s  vgpr %s scratch %s B  visits %d  scratch accesses in visits %d" % (name[len("_ZN12_GLOBAL__N_121"):][:40], vg, scr, len(vs), sum(v["scratch"] for v in vs)))
        for v in vs:
            print("   edges %2d msg_rd %2d | VALU %3d = %3d + %3d + %3d | sdwa_add %2d pk_add_u16 %2d pk_mul %d mul24 %d scratch %d lane_rd %d tab_rd %d" % (
                v["soft_rd"] // 2, v["msg_rd"], sum(v["valu"]), *v["valu"], v["sdwa_add"], v["pk_add"], v["pk_mul"], v["mul24"], v["scratch"], v["lane_rd"], v["tab_rd"]))


if __name__ == "__main__":
    for p in sys.argv[1:]:
        main(p)
