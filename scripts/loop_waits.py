"""The unit loop of every k_units / k_units_mv / k_pool_mv / k_units_deep instantiation as the gfx950 compiler scheduled it (device assembly, no GPU):
    python scripts/loop_waits.py [f64|f32] [filter]
For each kernel: the innermost loop that holds the value-stream load (the last 16-byte global load that sits in a loop: the entry phases come before the unit loop, the
fix-up and y loops behind it load less; in the kernels of hip_kernels_half.hip, whose values are halves, the last nontemporal 8-byte load — HALF_VALUE_LOAD), its `s_waitcnt vmcnt` values in program order, its instruction count, the waits that follow the first load behind the park inside the
chunk refill (the block, in a loop, that parks a descriptor chunk with ds_write_b128: the pattern gather of a dictionary plan, the descriptor load of a 12-byte one), and the kernel's VGPRs and scratch.  tests/test_unit_loop_waits_cpu.py asserts on `unit_loops()`."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kernel_asm import device_asm  # noqa: E402

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")


def _blocks(body):
    """[(label, header label of the innermost loop the block is in or None, [(mnemonic, operands)])] of one function's text, in program order."""
    out, label, header, insns, fresh = [], None, None, [], False
    for line in body.split("\n"):
        m = _LABEL.match(line)
        if m:
            out.append((label, header, insns))
            label, header, insns, fresh = m.group(1)[2:], None, [], True
        if fresh and ";" in line:   # the loop annotations are comments on the label line and the comment-only lines right behind it
            c = line.split(";", 1)[1]
            if "Loop Header:" in c:
                header = label
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", c)
            if h and header is None:
                header = h.group(1)
        m = None if _LABEL.match(line) else _INSN.match(line.split(";")[0])
        if m:
            fresh = False
            insns.append((m.group(1), m.group(2)))
    out.append((label, header, insns))
    return out


HALF_VALUE_LOAD = r"global_load_dwordx2 .*\bnt\b"   # the value-stream load of k_units_half (the x gathers are 8-byte loads too, but not nontemporal)
NT_VALUE_LOAD = r"global_load_dwordx[24] .*\bnt\b"   # ... of k_units_deep (hip_kernels_deep.hip), every value form: the only nontemporal loads of that kernel
DEEP_BATCHES_PER_TRIP = 4                             # its loop is one descriptor chunk per trip: DCHUNK / UNIT_DEEP_UB batches (record: profiles/unit_deep_isa.txt)


def unit_loops(asm, kinds=("k_units",), value_load=r"global_load_dwordx4\b"):
    """{demangled kernel: dict(vmcnt=[...], insns=n, refill_waits=[...] or None, vgpr=n, scratch=n)} for the kernels whose name starts with one of ``kinds``;
    ``value_load``: regular expression (mnemonic + operands) of the value-stream load that marks the unit loop."""
    value_load = re.compile(value_load)
    funcs = re.findall(r"^(_Z\w+):\s*; @\1\n(.*?)^\s+s_endpgm", asm, re.S | re.M)
    meta = {n: b for n, b in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    names = [n for n, _ in funcs]
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for (name, body), d in zip(funcs, dem):
        d = d.split("(")[0].replace("void tilespmv::", "")
        if not d.startswith(tuple(k + "<" for k in kinds)) or name not in meta:
            continue
        blocks = _blocks(body)
        hdr = None
        for _, h, insns in blocks:
            if h is not None and any(value_load.match(op + a) for op, a in insns):
                hdr = h
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta[name]).group(1))
        rec = dict(vmcnt=[], insns=0, refill_waits=None, vgpr=g("next_free_vgpr"), scratch=g("private_segment_fixed_size"))
        for _, h, insns in blocks:
            ops = [op for op, _ in insns]
            if h is not None and "ds_write_b128" in ops:   # the chunk refill (a block of the unit loop or of the chunk loop around it): what follows the first load behind the park
                tail = insns[ops.index("ds_write_b128"):]
                loads = [i for i, (op, _) in enumerate(tail) if op.startswith("global_load")]
                if loads:
                    rec["refill_waits"] = (rec["refill_waits"] or []) + [a.strip() for op, a in tail[loads[0] + 1:] if op == "s_waitcnt"]
            if hdr is None or h != hdr:
                continue
            rec["insns"] += len(insns)
            rec["vmcnt"] += [int(v) for op, a in insns if op == "s_waitcnt" for v in re.findall(r"vmcnt\((\d+)\)", a)]
        res[d] = rec
    return res


def main():
    dt = sys.argv[1] if len(sys.argv) > 1 else "f64"
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    asm = device_asm("hip_kernels.hip", dt, os.environ.get("LOOP_WAITS_ASM", "/tmp/loop_waits_%s.s" % dt))
    recs = list(unit_loops(asm, ("k_units", "k_units_mv", "k_pool_mv")).items())
    if dt == "f64":   # the kernels whose values are halves: a file of their own
        recs += list(unit_loops(device_asm("hip_kernels_half.hip", dt, os.environ.get("LOOP_WAITS_ASM_HALF", "/tmp/loop_waits_half.s")), ("k_units_half",), HALF_VALUE_LOAD).items())
    recs += list(unit_loops(device_asm("hip_kernels_deep.hip", dt, os.environ.get("LOOP_WAITS_ASM_DEEP", "/tmp/loop_waits_deep_%s.s" % dt)), ("k_units_deep",), NT_VALUE_LOAD).items())
    for d, r in recs:
        if d.startswith("k_units_deep<") and flt in d:
            print("%-62s vgpr %3d scratch %3d loop insns %4d = %d x %.1f per batch  vmcnt %s" % (d, r["vgpr"], r["scratch"], r["insns"], DEEP_BATCHES_PER_TRIP, r["insns"] / DEEP_BATCHES_PER_TRIP, ",".join(map(str, r["vmcnt"]))))
        elif flt in d:
            print("%-62s vgpr %3d scratch %3d loop insns %4d vmcnt %-22s refill waits after the gather: %s" %
                  (d, r["vgpr"], r["scratch"], r["insns"], ",".join(map(str, r["vmcnt"])), "-" if r["refill_waits"] is None else (" | ".join(r["refill_waits"]) or "none")))


if __name__ == "__main__":
    main()
