#!/usr/bin/env python3
"""Fingerprint of the compiled kernels of HIP object files (no GPU): per kernel of the gfx950 code object its mangled name, the
SHA-256 of its instruction text (addresses and // comments stripped) and the register / LDS / scratch numbers of the code
object's notes; per host object the sorted list of its __device_stub__ symbols.

  kernel_fingerprint.py a.o b.o ...      print the fingerprints
  kernel_fingerprint.py BEFORE AFTER     two directories of object files: print only the differences, exit 1 if there are any
"""
import hashlib, os, re, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def fingerprint(obj):
    """-> ({kernel: "sha256 vgpr=.. ..."}, [stub symbols])"""
    tmp = tempfile.mkdtemp(prefix="brats_fp_")
    try:
        shutil.copy(obj, os.path.join(tmp, "k.o"))
        run(LLVM + "llvm-objdump", "--offloading", "k.o", cwd=tmp)
        dev = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
        assert dev, f"no gfx950 code object in {obj}"
        text = run(LLVM + "llvm-objdump", "-d", dev[0], cwd=tmp)
        notes = run(LLVM + "llvm-readelf", "--notes", dev[0], cwd=tmp)
        whole = hashlib.sha256(open(os.path.join(tmp, dev[0]), "rb").read()).hexdigest()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    meta = {}
    for chunk in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:  # one list item of amdhsa.kernels each
        field = dict(re.findall(r"^    \.(\w+): +(\S+)$", "    " + chunk, flags=re.M))
        if "symbol" in field:
            meta[field["name"]] = " ".join(f"{k}={field.get(k, '?')}" for k in NOTES)
    code, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            code[name] = hashlib.sha256()
        elif name and "\t" in line:
            ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()  # "s_load_dword s0, s[4:5], 0x0 // 000000001000: C0020002"
            if ins != "...":  # (objdump's mark for padding zeros behind a function)
                code[name].update((ins + "\n").encode())
    kernels = {k: f"{code[k].hexdigest()} {v}" for k, v in meta.items()}
    kernels["(whole code object)"] = whole
    stubs = sorted({l.split()[-1] for l in run(LLVM + "llvm-objdump", "-t", obj).splitlines() if "__device_stub__" in l and l.split()[-1].startswith("_Z")})
    return kernels, stubs


def main(args):
    if len(args) == 2 and all(os.path.isdir(a) for a in args):
        names = [sorted(f for f in os.listdir(a) if f.endswith(".o")) for a in args]
        diffs = [f"object files differ: {names[0]} / {names[1]}"] if names[0] != names[1] else []
        for f in sorted(set(names[0]) & set(names[1])):
            (k0, s0), (k1, s1) = (fingerprint(os.path.join(a, f)) for a in args)
            same = k0.pop("(whole code object)") == k1.pop("(whole code object)")
            diffs += [f"{f}: kernel {k}: {k0.get(k, 'absent')} -> {k1.get(k, 'absent')}" for k in sorted(set(k0) | set(k1)) if k0.get(k) != k1.get(k)]
            diffs += [f"{f}: stub {s}: {'removed' if s in s0 else 'added'}" for s in sorted(set(s0) ^ set(s1))]
            print(f"{f}: {len(k1)} kernels, {len(s1)} stubs; whole code object {'byte-identical' if same else 'differs'}")
        print("\n".join(diffs) if diffs else "no difference")
        return 1 if diffs else 0
    for obj in args:
        kernels, stubs = fingerprint(obj)
        print(f"== {obj}")
        for k in sorted(kernels):
            print(k, kernels[k])
        print("stubs:", *stubs, sep="\n  ")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]) if len(sys.argv) > 1 else __doc__)
