#!/usr/bin/env python3
"""Device ISA of every translation unit, compared kernel by kernel between two trees (for refactors that must not
change code generation):

    python tools/isa_diff.py asm OLD_DIR /path/to/parent/checkout   # OLD_DIR/<unit>.s for each roger_amd/build.py UNITS entry
    python tools/isa_diff.py asm NEW_DIR                            # ... of this tree
    python tools/isa_diff.py asm DIR [TREE] -DRH_CENSUS               # ... of a measurement build (extra flags go to hipcc)
    python tools/isa_diff.py cmp OLD_DIR NEW_DIR                    # exit status 1 if a kernel changed or appeared

Function bodies and `.amdhsa_kernel` descriptors are compared after dropping `;` comments (loop headers carry the
function's ordinal) and renumbering the `.LBB`, `.Ltmp` and `.Lfunc_end` labels."""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from roger_amd.build import FLAGS, HIPCC, UNITS  # noqa: E402


def asm(out, tree=REPO, extra=()):
    csrc = os.path.join(tree, "roger_amd", "csrc")
    flags = [f for f in FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"), "-I" + csrc] + list(extra)
    os.makedirs(out, exist_ok=True)
    jobs = [subprocess.Popen([HIPCC] + flags + ["--offload-device-only", "-S", os.path.join(csrc, u + ".hip"),
                                                "-o", os.path.join(out, u + ".s")]) for u in UNITS]
    if any([j.wait() for j in jobs]):
        raise SystemExit("hipcc failed")


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.type\s+(\S+),@function\n(.*?)\.Lfunc_end\d+:", text, re.S):
        body = re.sub(r"[ \t]*;.*", "", m.group(2))   # (the padding in front of a comment follows the label's width)
        body = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1", body)
        out[m.group(1)] = body
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        out[m.group(1) + " (descriptor)"] = m.group(2)
    return out


def cmp(old, new):
    bad = False
    for name in sorted(f for f in os.listdir(old) if f.endswith(".s")):
        a, b = kernels(os.path.join(old, name)), kernels(os.path.join(new, name))
        changed = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
        print(f"{name[:-2]}: {len(a)} before, {len(b)} after, {len(a.keys() & b.keys()) - len(changed)} identical")
        for tag, names in (("removed", sorted(a.keys() - b.keys())), ("added", sorted(b.keys() - a.keys())),
                           ("changed", changed)):
            for k in names:
                print(f"  {tag}: {k}")
        bad |= bool(changed or b.keys() - a.keys())
    return bad


if __name__ == "__main__":
    if sys.argv[1:2] == ["asm"]:
        args = [a for a in sys.argv[2:] if not a.startswith("-")]
        asm(*args, extra=[a for a in sys.argv[2:] if a.startswith("-")])
    elif sys.argv[1:2] == ["cmp"]:
        sys.exit(cmp(*sys.argv[2:4]))
    else:
        raise SystemExit(__doc__)
