"""The unit loop of k_units as the gfx950 compiler scheduled it, checked without a GPU (scripts/loop_waits.py on the device assembly of both builds; the record of parent
and new is profiles/unit_loop_pipeline_isa.txt).  What must hold for every classic instantiation of entry mode 0 / 2 — the four narrow ones and
k_units<4, 0, 16, {true, false}, true, false, false, false> of both builds among them —: the loop that holds the value-stream load is found, the kernel uses no scratch,
and the loop is not longer than the parent's (whose counts are written down here from that record: the 32-bit x index takes 8 instructions out of every gather, the
address select of a task's last value prefetch puts 3-4 back per value load).  The two-buffer loop and the parked dictionary pattern of the same change were measured slower and are not in the kernel (profiles/unit_loop_pipeline_ab.txt),
so the one-buffer loop's `s_waitcnt vmcnt(0)` in front of the value copy is still there: the test pins that the loop's waits are the parent's, not that there are none."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

from kernel_asm import ROOT, device_asm

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from loop_waits import unit_loops  # noqa: E402

HOT = "k_units<4, 0, 16, true, true, false, false, true>"
PARENT_LOOP_INSNS = {   # in-loop instructions per batch of 4 units at the parent commit (profiles/unit_loop_pipeline_isa.txt)
    "f64": {HOT: 405, "k_units<4, 0, 16, false, true, false, false, true>": 397, "k_units<4, 2, 16, true, true, false, false, true>": 405,
            "k_units<4, 2, 16, false, true, false, false, true>": 393, "k_units<4, 0, 16, true, true, false, false, false>": 422,
            "k_units<4, 0, 16, false, true, false, false, false>": 406},
    "f32": {"k_units<4, 0, 16, true, true, false, false, false>": 327, "k_units<4, 0, 16, false, true, false, false, false>": 317},
}


def _classic_per_strip_or_workgroup(name):
    a = [t.strip() for t in name[name.index("<") + 1:name.rindex(">")].split(",")]
    return name.startswith("k_units<") and a[1] in ("0", "2") and a[5] == "false"


def test_unit_loops_of_both_builds(tmp_path):
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_kernels.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        loops = {k: v for k, v in unit_loops(s).items() if _classic_per_strip_or_workgroup(k)}
        assert len(loops) == (18 if dt == "f64" else 14), (dt, sorted(loops))
        assert not set(PARENT_LOOP_INSNS[dt]) - set(loops), (dt, sorted(loops))
        for k, rec in loops.items():
            print(dt, k, rec)
            assert rec["scratch"] == 0, (dt, k, rec)
            assert rec["insns"] > 0 and rec["vmcnt"], (dt, k, rec)          # the loop with the value-stream load was found and waits for loads
            want = PARENT_LOOP_INSNS[dt].get(k)
            if want is not None:
                assert rec["insns"] <= want, (dt, k, rec["insns"], want)
    hot = unit_loops(asm["f64"])[HOT]
    assert hot["insns"] <= PARENT_LOOP_INSNS["f64"][HOT] - 20 and hot["vgpr"] <= 59, hot   # the hot narrow kernel: clearly shorter, and no more VGPRs than the parent's 59
