"""The gfx950 assembly of one library source, compiled with the flags of build_native.py.

    python tools/device_asm.py plastic.hip out.s

To show that a change leaves a source's device code alone, run it in a checkout of each commit and
`diff` the two files: hipcc derives the `__hip_cuid_*` symbol from the whole translation unit, headers
included, so an object file differs in it whenever a header gains a declaration; the assembly then
differs in the lines that name that symbol and in nothing else."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
import build_native as b  # noqa: E402

if len(sys.argv) != 3:
    sys.exit("usage: python tools/device_asm.py SOURCE.hip OUT.s   (SOURCE.hip: a file of plastic-unet_amd/csrc)")
src, out = sys.argv[1], sys.argv[2]
r = subprocess.run([b.HIPCC] + b.CFLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out],
                   capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr)
