#!/usr/bin/env python3
"""Is the library's device code the same before and after a change that must not touch it?

  tools/device_asm_identity.py emit OUT.s [--rev REV] [-DNAME ...]   device assembly of the working tree (or of commit REV)
  tools/device_asm_identity.py compare A.s B.s                        whole text, then function by function

emit uses the library's own flags (x_maps_amd/_native.py) with -shared replaced by --cuda-device-only -S and a fixed -cuid=, which
makes the text deterministic.  compare reports identical texts, or -- when only the order of the functions differs -- compares them
by name with the function index taken out of the local labels and of the loop comments that quote them, and lists every function whose body differs with the number of
differing lines.  It compares texts and looks for no instruction in particular.  Results: profiles/device_split_identity.md.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(out, rev, defines):
    from x_maps_amd import _native as N
    flags = [f for f in N.HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", "-cuid=xmaps"]
    with tempfile.TemporaryDirectory() as tmp:
        root = ROOT
        if rev:  # the committed tree of REV, unpacked beside nothing else
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "x_maps_amd/csrc", "include"], check=True, capture_output=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
            root = tmp
        src = [os.path.join(root, os.path.relpath(s, ROOT)) for s in N.SOURCES]
        cmd = [N._hipcc()] + flags + defines + src + ["-o", out]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)


def functions(text):
    """{name: body lines} of every function (.type NAME,@function ... .size NAME); the rest (objects, metadata) under '' """
    out, name = {"": []}, ""
    for line in text.split("\n"):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            out[name] = []
        line = re.sub(r"\.L(BB|tmp|func_[a-z]+)\d+", r".L\1", line)
        line = re.sub(r"\bBB\d+_", "BB_", line)  # (the loop comments name blocks as BB<function index>_<block> ...
        out[name].append(re.sub(r"[ \t]+;", " ;", line))  # ... behind padding that depends on the label's length)
        if name and re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
            name = ""
    return out


def compare(a, b):
    ta, tb = open(a).read(), open(b).read()
    fa, fb = functions(ta), functions(tb)
    n = len(fa) - 1
    if ta == tb:
        print(f"identical: whole text, {n} functions")
        return 0
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        la, lb = fa.get(name), fb.get(name)
        if la != lb:
            d = sum(1 for x in difflib.unified_diff(la or [], lb or [], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---"))
            print(f"DIFFERS: {name or '(objects and metadata)'}: {d} lines")
            bad += 1
    print(f"{n} functions compared by name, {bad} differ" if bad else f"identical function by function ({n}); only their order differs")
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 2 and a[0] == "emit":
        rev = a[a.index("--rev") + 1] if "--rev" in a else None
        emit(a[1], rev, [x for x in a[2:] if x.startswith("-D")])
    elif len(a) == 3 and a[0] == "compare":
        sys.exit(compare(a[1], a[2]))
    else:
        sys.exit(__doc__)
