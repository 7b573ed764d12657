"""The gfx950 assembly of one library source, compiled with the flags of build_native.py.

    python tools/device_asm.py plastic.hip out.s
    python tools/device_asm.py --compare OLD.s NEW.s

To show that a change leaves a source's device code alone, run the first form in a checkout of each
commit and compare the two files with the second.  hipcc derives the `__hip_cuid_*` symbol from the
whole translation unit, headers included, so an object file differs in it whenever a header gains
a declaration; the comparison leaves the lines that name that symbol out.  It prints one line per
kernel:

    identical           the kernel's text (code and its .amdhsa_kernel block) is the same
    same instructions   the text differs, the multiset of instruction mnemonics does not
    differs             with the mnemonics whose counts differ, as mnemonic old -> new

and exits with status 1 if any kernel differs or exists on one side only."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plastic-unet_amd"))
import build_native as b  # noqa: E402


def kernels(path):
    """{kernel symbol: [its lines]}: the function from its label to .Lfunc_end, and its
    .amdhsa_kernel block (registers, LDS, scratch)."""
    out, cur, in_desc = {}, None, None
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"(\w+):\s+; @(\w+)", line)
        if m and m.group(1) == m.group(2):
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", line)
        if m:
            in_desc = out.setdefault(m.group(1), [])
        if in_desc is not None:
            in_desc.append(line)
            if ".end_amdhsa_kernel" in line:
                in_desc = None
        elif cur is not None:
            cur.append(line)
    return out


def mnemonics(lines):
    c = collections.Counter()
    for line in lines:
        m = re.match(r"\t([a-z_][a-z0-9_]*)(\s|$)", line)
        if m:
            c[m.group(1)] += 1
    return c


def compare(old, new):
    a, n = kernels(old), kernels(new)
    bad = 0
    for k in sorted(set(a) | set(n)):
        if k not in a or k not in n:
            print("%-18s %s" % ("only in " + (old if k in a else new), k))
            bad += 1
        elif a[k] == n[k]:
            print("%-18s %s" % ("identical", k))
        else:
            ma, mn = mnemonics(a[k]), mnemonics(n[k])
            if ma == mn:
                print("%-18s %s" % ("same instructions", k))
            else:
                diff = ", ".join("%s %d -> %d" % (i, ma[i], mn[i]) for i in sorted(set(ma) | set(mn)) if ma[i] != mn[i])
                print("%-18s %s: %s" % ("differs", k, diff))
                bad += 1
    return 1 if bad else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
if len(sys.argv) != 3:
    sys.exit("usage: python tools/device_asm.py SOURCE.hip OUT.s   (SOURCE.hip: a file of plastic-unet_amd/csrc)\n"
             "       python tools/device_asm.py --compare OLD.s NEW.s")
src, out = sys.argv[1], sys.argv[2]
r = subprocess.run([b.HIPCC] + b.CFLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out],
                   capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr)
