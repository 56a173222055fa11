"""What the gfx950 compiler made of hip_kernels.hip, checked without a GPU: no kernel of either build touches scratch memory (a spilled register costs a kernel more than
any instruction it saves), and the number of kernel instantiations stays bounded (round 6 retired the x-window and slab-pacing template axes and made the XCD remap a
run-time branch: 144 -> 91 per value type).  Reads the device assembly (`hipcc -S --cuda-device-only`), the same source and flags as tilespmv_amd/csrc/Makefile."""
from concurrent.futures import ThreadPoolExecutor

from kernel_asm import device_asm, private_segments

MAX_KERNELS = 96


def test_no_kernel_spills_and_the_instantiation_count_is_bounded(tmp_path):
    with ThreadPoolExecutor(2) as ex:
        asm = dict(zip(("f64", "f32"), ex.map(lambda dt: device_asm("hip_kernels.hip", dt, str(tmp_path / (dt + ".s"))), ("f64", "f32"))))
    for dt, s in asm.items():
        spills = private_segments(s)
        assert 40 <= len(spills) <= MAX_KERNELS, (dt, len(spills))
        assert not {k: v for k, v in spills.items() if v}, (dt, {k: v for k, v in spills.items() if v})
        assert ("v_mfma_f64_16x16x4_f64" if dt == "f64" else "v_mfma_f32_16x16x4_f32") in s      # dense tiles run on the matrix cores in both builds
