#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, object by object: device_code_digest.py OBJ_DIR_A OBJ_DIR_B

For every *.o in both directories: dump .hip_fatbin, unbundle the gfx950 code object, and print the hash of its .text,
the number of kernels, the kernels present on one side only and the kernels whose bytes differ.  (Whole code objects
differ between two builds of the same source -- they carry a per-compile id -- .text does not.)  Exit status 1 if
anything differs.  Bytes are compared; nothing is searched for."""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernels(obj, tmp):
    """(.text bytes, {kernel name: its bytes}) of the gfx950 code object inside `obj`"""
    fat, co, text = (os.path.join(tmp, n) for n in ("fatbin", "code_object", "text"))
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o"))
    target = next(t for t in run("clang-offload-bundler", "--list", "--type=o", "--input=" + fat).split() if "gfx950" in t)
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + target, "--input=" + fat, "--output=" + co)
    run("llvm-objcopy", "--dump-section", ".text=" + text, co, os.path.join(tmp, "copy.co"))
    blob = open(text, "rb").read()
    base = next(int(f[f.index(".text") + 2], 16) for f in map(str.split, run("llvm-readelf", "-SW", co).splitlines())
                if ".text" in f)
    syms = [f for f in map(str.split, run("llvm-readelf", "-sW", co).splitlines()) if len(f) == 8 and f[3] in ("FUNC", "OBJECT")]
    described = {f[7][:-3] for f in syms if f[7].endswith(".kd")}
    return blob, {f[7]: blob[int(f[1], 16) - base:int(f[1], 16) - base + int(f[2])] for f in syms if f[7] in described}


def main(dir_a, dir_b):
    differs = False
    for name in sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b))):
        if not name.endswith(".o"):
            continue
        sides = []
        for d in (dir_a, dir_b):
            with tempfile.TemporaryDirectory() as tmp:
                sides.append(kernels(os.path.join(d, name), tmp))
        (ta, ka), (tb, kb) = sides
        only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        changed = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        same = ta == tb and not only_a and not only_b and not changed
        differs = differs or not same
        print(f"{name}: .text sha256 {hashlib.sha256(ta).hexdigest()[:16]} / {hashlib.sha256(tb).hexdigest()[:16]}, "
              f"kernels {len(ka)} / {len(kb)}: {'identical' if same else 'DIFFERENT'}")
        for label, names in (("only in A", only_a), ("only in B", only_b), ("bytes differ", changed)):
            for k in names:
                print(f"  {label}: {k}")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
