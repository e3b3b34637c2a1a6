"""One line per device function of the library's gfx950 code object: a hash of its instruction stream, the number of
disassembly lines and the symbol -- to compare the device code of two builds without a GPU (diff two listings).
--resources adds, per kernel, what the code object's metadata says: VGPRs, SGPRs, LDS, scratch, spills.

--function=PREFIX prints the instruction stream of the functions whose demangled name starts with PREFIX instead.

    python scripts/code_object_functions.py [--resources] [--function=PREFIX] [path/to/libhudiff_hip.so] > listing.txt"""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp):
    """llvm-objdump --offloading writes the bundle's members next to its input: work on a copy."""
    so = shutil.copy(lib, os.path.join(tmp, "lib.so"))
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", so, cwd=tmp)
    found = glob.glob(so + ".*gfx950")
    if len(found) != 1:
        raise SystemExit(f"{lib}: expected one gfx950 code object, found {found}")
    return found[0]


def functions(co):
    """{symbol: [instruction lines]} in the order of the disassembly; trailing comments (addresses, encodings) stripped."""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        line = re.sub(r"\s*//.*$", "", line).strip()
        # ("...": llvm-objdump's elision of zero bytes, the padding behind a function -- placement, not instructions)
        if cur is not None and line and line != "..." and not line.startswith("Disassembly of section"):
            cur.append(line)
    return out


def resources(co):
    """{kernel symbol: (vgpr, sgpr, lds, scratch, spills)} from the AMDGPU metadata note."""
    txt = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    res = {}
    for block in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        g = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", block).group(1))
        name = re.search(r"\.name:\s*(\S+)", block).group(1)
        res[name] = (g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"),
                     g("vgpr_spill_count") + g("sgpr_spill_count"))
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lib = args[0] if args else os.path.join(ROOT, "hudiff_amd", "libhudiff_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(lib, tmp)
        fn = functions(co)
        res = resources(co) if "--resources" in sys.argv else {}
    demangled = subprocess.run(["c++filt"], input="\n".join(fn), check=True, capture_output=True, text=True).stdout.splitlines()
    rows = sorted(zip(demangled, fn))
    want = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--function=")]
    if want:                                             # the instruction stream itself, to diff one function of two builds
        for name, sym in rows:
            if any(name.startswith(w) or name.startswith("void " + w) for w in want):
                print(f"<{name}>")
                print("\n".join(fn[sym]))
        return
    for name, sym in rows:
        lines = fn[sym]
        h = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
        extra = ""
        if sym in res:
            extra = "  vgpr %d sgpr %d lds %d scratch %d spills %d" % res[sym]
        print(f"{h} {len(lines):6d}  {name}{extra}")
    print(f"# {len(rows)} functions", file=sys.stderr)


if __name__ == "__main__":
    main()
