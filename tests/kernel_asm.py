"""What the gfx950 compiler makes of one file of tilespmv_amd/csrc, read without a GPU (a helper, not a test): the device assembly of a source file, built with the flags of
tilespmv_amd/csrc/Makefile, and the kernels found in it.  Shared by tests/test_kernel_resources.py and the solvers' CPU tests."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm(source_name, dt, out):
    """The device assembly of tilespmv_amd/csrc/<source_name> for value type ``dt`` ("f64" or "f32"), written to ``out`` and returned as text."""
    defs = ["-DMAT_VAL_TYPE=double"] if dt == "f64" else ["-DMAT_VAL_TYPE=float", "-DTILESPMV_F32"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--offload-arch=gfx950", "-munsafe-fp-atomics", "-w"] + defs +
                   ["-S", "--cuda-device-only", os.path.join(ROOT, "tilespmv_amd/csrc", source_name), "-o", out], check=True)
    return open(out).read()


def private_segments(asm):
    """``{kernel name: bytes of private segment (scratch memory: spilled registers, stack arrays)}`` of an assembly text, in the order of the kernels' descriptors."""
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    return {name: int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) for name, body in kernels}
