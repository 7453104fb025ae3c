#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 device code of sources under pagnerf_amd/csrc (no GPU needed): what a refactor that must not change
a kernel is checked with.

    python scripts/kernel_digest.py mlp_deep.hip mlp_h128.hip > after.txt
    python scripts/kernel_digest.py --csrc OTHER_TREE/pagnerf_amd/csrc mlp_deep.hip mlp_h128.hip > before.txt
    diff before.txt after.txt

Each source is compiled with build.py's flags for it plus --offload-device-only; one line per FUNC symbol of the gfx950 code object:

    name vgpr agpr sgpr lds scratch kernarg max_wg n_instr mnemonic_sha text_sha

name           demangled, without return type, namespace qualifiers and spaces: a kernel that moves to another translation unit, or whose
               parameter struct moves to another namespace, keeps its name
vgpr .. max_wg the kernel's entry in the amdhsa.kernels note (`-` for a function that is not a kernel)
n_instr        instructions of its disassembly, trailing padding dropped
mnemonic_sha   hash of the ordered mnemonics: equal = the same instruction sequence
text_sha       hash of the whole disassembly without comments: operands and registers as well.  The compiler's order of the sources of a
               commutative instruction depends on what else is in the translation unit, so this column can differ where the others do not;
               --dump DIR keeps every kernel's disassembly as DIR/<name>.s for a diff of such a pair.
Lines are sorted by name.  A source that build.py does not list (another tree's) takes the flags of --like SOURCE.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pagnerf_amd import build as pag_build      # noqa: E402  (its flags and compiler; nothing is built into the package)

TARGET = "hipv4-amdgcn-amd-amdhsa--" + pag_build.ARCH
NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size",
             "max_flat_workgroup_size")


def tool(name):
    """An LLVM tool next to the compiler's clang ($LLVM_BIN, <rocm>/llvm/bin), else from PATH."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(pag_build._hipcc())))
    for d in (os.environ.get("LLVM_BIN"), os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin")):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return r.stdout


def device_elf(csrc, src, flags, tmp):
    bundle, elf = os.path.join(tmp, "dev.bundle"), os.path.join(tmp, "dev.elf")
    run([pag_build._hipcc()] + pag_build.COMMON + flags + ["--offload-device-only", "-c", os.path.join(csrc, src), "-o", bundle])
    run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + elf])
    return elf


def plain_name(demangled):
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"\b[A-Za-z_]\w*::", "", s)
    return re.sub(r"^void\s+", "", s).replace(" ", "")


def kernel_notes(elf):
    """symbol -> NOTE_KEYS values from the amdhsa.kernels metadata, which llvm-readelf prints as YAML: a kernel starts at `  - .key:`, its
    own keys follow at four spaces, everything deeper belongs to its .args."""
    kernels, cur = [], None
    for line in run([tool("llvm-readelf"), "--notes", elf]).splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
            kernels.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'\"")
    return {k["name"]: tuple(k.get(n, "?") for n in NOTE_KEYS) for k in kernels if "name" in k}


def disassembly(elf, sym):
    out = run([tool("llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", "--disassemble-symbols=" + sym, elf])
    ins = []
    for line in out.splitlines():
        if not line.startswith(("\t", " ")):        # file header, section and symbol labels
            continue
        line = re.sub(r"\s+", " ", line.split("//")[0].strip())
        if line:
            ins.append(line)
    while ins and ins[-1].split()[0] in ("s_nop", "s_code_end", "..."):
        ins.pop()
    return ins


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12]


def digest(csrc, src, flags, dump=None):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        elf = device_elf(csrc, src, flags, tmp)
        notes = kernel_notes(elf)
        # llvm-objdump knows every mangling the compiler emits (std::bfloat16_t): the symbol table once raw, once demangled, same order
        table = [[l.split(".text\t", 1)[1].split(None, 1)[1].replace(".protected ", "").strip() for l in run([tool("llvm-objdump"), "--syms"] + c + [elf]).splitlines()
                  if " F .text" in l] for c in ([], ["-C"])]
        syms, names = zip(*sorted(set(zip(*table)))) if table[0] else ((), ())
        for sym, dem in zip(syms, names):
            ins = disassembly(elf, sym)
            name = plain_name(dem)
            rows.append(" ".join((name,) + notes.get(sym, ("-",) * len(NOTE_KEYS)) + (str(len(ins)), sha([i.split()[0] for i in ins]), sha(ins))))
            if dump:
                os.makedirs(dump, exist_ok=True)
                with open(os.path.join(dump, re.sub(r"[^\w.,<>()-]", "_", name)[:200] + ".s"), "w") as fh:
                    fh.write("\n".join(ins) + "\n")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="+", help="file names under --csrc")
    ap.add_argument("--csrc", default=pag_build.CSRC, help="source directory (default: this tree's pagnerf_amd/csrc)")
    ap.add_argument("--like", help="a source of build.py whose flags the sources it does not list take")
    ap.add_argument("--dump", help="directory for the per-kernel disassembly")
    a = ap.parse_args()
    rows = []
    for src in a.sources:
        flags = pag_build.SOURCES.get(src, pag_build.SOURCES.get(a.like))
        if flags is None:
            sys.exit("%s is not in build.py's SOURCES: give --like SOURCE" % src)
        rows += digest(a.csrc, src, flags, a.dump)
    print("\n".join(sorted(rows)))


if __name__ == "__main__":
    main()
