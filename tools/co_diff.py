#!/usr/bin/env python3
"""Compare the gfx950 code of two builds, kernel by kernel.  CPU only.

    co_diff.py PARENT_BUILD_DIR RESULT_BUILD_DIR   every *.o in both directories that bundles a
                                                   gfx950 code object
    co_diff.py PARENT.co RESULT.co                 two raw code objects (the hiprtc ones)

Per kernel: whether its code is byte-identical, the symbol size, LDS / scratch / VGPRs / SGPRs
from the kernel descriptor (tests/code_objects.py), and whether the multiset of instruction
mnemonics is equal.  The level is 1 for byte-identical code, 2 for the same size, descriptor
fields and mnemonic multiset (the same code in another order), 3 for anything else.  Counts
only: no disassembly is printed."""
import collections
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from code_objects import OBJDUMP, gfx950_code_object, kernel_descriptors  # noqa: E402

FIELDS = ("size", "lds", "scratch", "vgprs", "sgprs")


def mnemonics(co, kernels, work):
    """{kernel: Counter of its instructions' mnemonics}, from llvm-objdump's disassembly."""
    path = os.path.join(work, "co.elf")
    with open(path, "wb") as f:
        f.write(co)
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True,
                          check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        if line.endswith(">:"):  # "<address> <symbol>:"
            sym = line[line.index("<") + 1:-2]
            cur = out.setdefault(sym, collections.Counter()) if sym in kernels else None
        elif cur is not None and line.startswith("\t"):
            cur[line.split("//")[0].split()[0]] += 1
    return out


def compare(name, a, b, work):
    """Print one line per kernel of the two code objects a and b; return the levels' counts."""
    ka, kb = kernel_descriptors(a), kernel_descriptors(b)
    ma = mnemonics(a, ka, os.path.join(work, "a"))
    mb = mnemonics(b, kb, os.path.join(work, "b"))
    levels = collections.Counter()
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            print(f"{name}  {k}: only in the {'result' if k in kb else 'parent'}  level 3")
            levels[3] += 1
            continue
        da, db = ka[k], kb[k]
        same_bytes = a[da["offset"]:da["offset"] + da["size"]] == b[db["offset"]:db["offset"] + db["size"]]
        same_desc = all(da[f] == db[f] for f in FIELDS)
        same_mn = ma.get(k) == mb.get(k)
        level = 1 if same_bytes and same_desc else 2 if same_desc and same_mn else 3
        levels[level] += 1
        desc = " ".join(f"{f} {da[f]}" if da[f] == db[f] else f"{f} {da[f]}->{db[f]}" for f in FIELDS)
        n = sum(ma.get(k, {}).values())
        print(f"{name}  {k}: bytes {'identical' if same_bytes else 'differ'}, {desc}, "
              f"mnemonics {'equal' if same_mn else 'differ'} ({n} instructions)  level {level}")
    return levels


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    pa, pb = argv[1:]
    total = collections.Counter()
    with tempfile.TemporaryDirectory() as tmp:
        if os.path.isdir(pa):
            objs = sorted(o for o in os.listdir(pa) if o.endswith(".o") and os.path.exists(os.path.join(pb, o)))
            n = 0
            for o in objs:
                work = os.path.join(tmp, o)
                try:
                    a = gfx950_code_object(os.path.join(pa, o), os.path.join(work, "pa"))
                    b = gfx950_code_object(os.path.join(pb, o), os.path.join(work, "pb"))
                except (AssertionError, subprocess.CalledProcessError):
                    continue  # host-only object
                for d in ("a", "b"):
                    os.makedirs(os.path.join(work, d))
                lv = compare(o, a, b, work)
                if lv:
                    n += 1
                    print(f"{o}: object bytes {'identical' if a == b else 'differ'}; kernels at level "
                          + ", ".join(f"{l}: {lv[l]}" for l in (1, 2, 3)))
                total += lv
            print(f"{n} objects with kernels")
        else:
            for d in ("a", "b"):
                os.makedirs(os.path.join(tmp, d))
            a, b = open(pa, "rb").read(), open(pb, "rb").read()
            total = compare(os.path.basename(pb), a, b, tmp)
            print(f"object bytes {'identical' if a == b else 'differ'}")
    print("kernels at level " + ", ".join(f"{l}: {total[l]}" for l in (1, 2, 3)))
    return 0 if total[3] == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
