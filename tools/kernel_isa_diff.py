#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S \
          -o dev.s sph_hip.hip            (from csrc/, once per tree)
    python tools/kernel_isa_diff.py OLD.s NEW.s

Every function body (.type <sym>,@function ... .Lfunc_end<n>) and every kernel descriptor
(.amdhsa_kernel ... .end_amdhsa_kernel) is hashed on its own.  Local labels (.LBB<n>_<m>, .Ltmp<n>,
.Lfunc_end<n>) are numbered in emission order, which a change of host-side dispatch can reorder: they
are renamed to one fixed name first, and the assembler's comments are dropped.  The metadata that
follows the code is not compared.
Exit status 0: the same symbols with the same code; 1: any difference (listed).
"""
import hashlib
import re
import sys

FUNC = re.compile(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", re.S | re.M)
DESC = re.compile(r"^\t\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", re.S | re.M)
LABEL = re.compile(r"\.L(BB|func_end|tmp)\d+(_\d+)?")
COMMENT = re.compile(r"\s*;.*$", re.M)   # (the compiler's remarks name blocks by number too)


def digest(text):
    return hashlib.sha256(LABEL.sub(r".L\1", COMMENT.sub("", text)).encode()).hexdigest()[:16]


def symbols(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        s = f.read()
    out = {m.group(1): digest(m.group(2)) for m in FUNC.finditer(s)}
    out.update({m.group(1) + ".kd": digest(m.group(2)) for m in DESC.finditer(s)})
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__.strip().splitlines()[0])
        print("usage: kernel_isa_diff.py OLD.s NEW.s")
        return 2
    old, new = symbols(argv[1]), symbols(argv[2])
    differ = [k for k in sorted(set(old) | set(new)) if old.get(k) != new.get(k)]
    kernels = sum(1 for k in new if k.endswith(".kd"))
    print("%d entries old, %d new (%d kernels); %d differ" % (len(old), len(new), kernels, len(differ)))
    for k in differ:
        print("  %-14s %-18s %s" % ("only old" if k not in new else "only new" if k not in old else "changed",
                                    old.get(k, "-"), k))
    return 1 if differ or not old else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
