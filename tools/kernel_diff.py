#!/usr/bin/env python3
"""kernel_diff.py OLD NEW [KERNEL ...] -- compare the gfx950 device code of two builds, function by function.

OLD and NEW are libmistitch.so files or object files.  The gfx950 code objects are extracted the way tests/test_build_checks.py
does (llvm-objdump --offloading, then -d), the disassembly is split by symbol, and addresses, encodings and PC-relative literals
(the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64) are stripped.  One line per function:

    same|differs|only-old|only-new  <symbol>  insns OLD/NEW  vgpr OLD/NEW  sgpr OLD/NEW  lds OLD/NEW  scratch OLD/NEW

(the four resource figures are .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size of the code
object's metadata; device functions that are not kernels have none).  It compares and counts; it looks for no instruction.
KERNEL arguments are substrings of (mangled or demangled) symbol names: the exit status is 1 when a function matching one of them
differs or exists on one side only, or when an argument matches nothing; without arguments, when the two sets of symbols differ.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
PCREG = re.compile(r"s_getpc_b64\s+s\[(\d+):(\d+)\]")
PCADD = re.compile(r"^(s_addc?_u32\s+s(\d+),\s*s\d+,\s*)(0x[0-9a-f]+|-?\d+)$")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def _run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, capture_output=True, text=True).stdout


def _functions(text):
    """disassembly of one code object -> {symbol: [stripped instruction]}"""
    out, cur, pc = {}, None, set()
    for line in text.splitlines():
        m = SYM.match(line.strip())
        if m:
            cur, pc = out.setdefault(m.group(1), []), set()
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = " ".join(line.split("//")[0].split())
        if not ins:
            continue
        m = PCREG.search(ins)
        if m:
            pc = {m.group(1), m.group(2)}
        else:
            m = PCADD.match(ins)
            if m and m.group(2) in pc:
                ins = m.group(1) + "<pcrel>"
                pc.discard(m.group(2))
        cur.append(ins)
    return out


def _metadata(notes):
    """llvm-readelf --notes of one code object -> {kernel symbol: {key: value}}"""
    out, cur = {}, {}
    for line in notes.splitlines() + ["  - .end"]:
        s = line.strip()
        if s.startswith("- ") and line.startswith("  - "):      # a new entry of amdhsa.kernels
            if ".symbol" in cur:
                out[cur[".symbol"].replace(".kd", "")] = cur
            cur = {}
            s = s[2:]
        if ":" in s:
            k, v = s.split(":", 1)
            if k in META or k == ".symbol":
                cur[k] = v.strip().strip("'\"")
    return out


def load(path):
    """-> ({symbol: [instruction]}, {symbol: metadata})"""
    d = tempfile.mkdtemp(prefix="kdiff")
    try:
        shutil.copy(path, os.path.join(d, "in.bin"))
        _run("llvm-objdump", "--offloading", "in.bin", cwd=d)
        objs = sorted(f for f in os.listdir(d) if "gfx950" in f)
        if not objs:
            raise SystemExit("%s: no gfx950 code object" % path)
        funcs, meta = {}, {}
        for f in objs:
            funcs.update(_functions(_run("llvm-objdump", "-d", f, cwd=d)))
            meta.update(_metadata(_run("llvm-readelf", "--notes", f, cwd=d)))
        return funcs, meta
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    (fo, mo), (fn, mn) = load(argv[1]), load(argv[2])
    names = sorted(set(fo) | set(fn))
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")       # readable names where a demangler exists
    demangled = dict(zip(names, subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines())) if filt else {}
    wanted = argv[3:]
    hit = {w: False for w in wanted}
    bad = 0
    for n in names:
        a, b = fo.get(n), fn.get(n)
        state = "only-new" if a is None else "only-old" if b is None else "same" if a == b else "differs"
        cols = ["insns %s/%s" % (len(a) if a is not None else "-", len(b) if b is not None else "-")]
        for key, label in zip(META, ("vgpr", "sgpr", "lds", "scratch")):
            cols.append("%s %s/%s" % (label, mo.get(n, {}).get(key, "-"), mn.get(n, {}).get(key, "-")))
        print("%-8s  %s  %s" % (state, demangled.get(n, n), "  ".join(cols)))
        named = [w for w in wanted if w in n or w in demangled.get(n, n)]
        for w in named:
            hit[w] = True
        if state != "same" and (named or (not wanted and state != "differs")):
            bad = 1
    for w, h in hit.items():
        if not h:
            print("no function matches %r" % w)
            bad = 1
    kern_o, kern_n = set(mo), set(mn)
    print("kernels: %d old, %d new, %d same, %d differ, only old %s, only new %s" % (
        len(kern_o), len(kern_n), sum(1 for k in kern_o & kern_n if fo.get(k) == fn.get(k)),
        sum(1 for k in kern_o & kern_n if fo.get(k) != fn.get(k)), sorted(kern_o - kern_n), sorted(kern_n - kern_o)))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv))
