#!/usr/bin/env python3
"""kernel_isa_diff.py A.so B.so -- compares the gfx950 kernels of two builds of libepp.so.

Walks the gfx950 bundles of both libraries' .hip_fatbin (as tests/test_kernel_resources.py
does).  Per kernel: its disassembly (llvm-objdump; no addresses, no raw bytes, branch
targets as offsets from the kernel's start) and its metadata note (VGPRs, SGPRs, LDS bytes,
private segment, kernarg size).  Prints three lists: kernels only in A, kernels only in B,
and kernels whose text or metadata differ, with a unified diff for each.  A kernel whose
parameter list changed or whose template lost or gained a parameter (and with it its mangled
name changed) is listed first and then compared with its other self.  Exit status 0 when all lists are empty, 1 otherwise.  It only compares.
"""
import difflib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size", "vgpr_spill_count", "sgpr_spill_count")


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def _code_objects(lib_path, td):
    fb = os.path.join(td, "fatbin")
    _run("llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib_path, os.path.join(td, "stripped"))
    data = open(fb, "rb").read()
    pos, idx = data.find(MAGIC), 0
    assert pos >= 0, f"{lib_path}: no offload bundle in .hip_fatbin"
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + len(MAGIC))[0]
        o = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if "gfx950" in triple and size:
                co = os.path.join(td, f"co{idx}.elf")
                idx += 1
                with open(co, "wb") as f:
                    f.write(data[pos + off:pos + off + size])
                yield co
        pos = data.find(MAGIC, pos + len(MAGIC))


def _metadata(co):
    """{kernel: {key: value}} from the amdhsa.kernels list of the metadata note (YAML: an
    entry opens with "  - .key:", its other keys sit at four spaces, its arguments deeper)."""
    entries, cur, inside = [], None, False
    for line in _run("llvm-readelf", "--notes", co).splitlines():
        if re.match(r"^\S", line):
            inside = line.startswith("amdhsa.kernels:")
            continue
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)", line)
        if not inside or not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
            entries.append(cur)
        cur[m.group(2)] = m.group(3)
    return {e["name"]: {m: e.get(m, "-") for m in META} for e in entries}


def _text(co):
    """{function symbol: [instruction lines]}; a branch's target as +offset from the symbol's start."""
    out, cur, name = {}, None, None
    for line in _run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, [])
            continue
        if cur is None or not line.startswith("\t") or line.strip() == "...":  # ("...": zero fill behind
            continue                                                         # a code object's last kernel)
        ins, _, comment = line.partition("//")
        ins = " ".join(ins.split())
        t = re.search(r"<(.+?)(\+0x[0-9a-f]+)?>\s*$", comment)
        if t:
            ins += " -> " + ("" if t.group(1) == name else t.group(1)) + (t.group(2) or "+0x0")
        cur.append(ins)
    return out


def kernels(lib_path):
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in _code_objects(lib_path, td):
            text = _text(co)
            for name, meta in _metadata(co).items():
                out[name] = (meta, text.get(name, []))
    return out


def _base(name):
    """The demangled name without its parameter list, as (template name, template arguments):
    ("epp::k_knn_tile", ("16",))."""
    out = subprocess.run(["c++filt", name], check=True, capture_output=True, text=True).stdout  # (binutils)
    head = out.replace("(anonymous namespace)::", "").split("(")[0].strip()
    if not head.endswith(">"):
        return head.split()[-1], ()
    depth, lt = 0, len(head)
    while True:  # the "<" that opens the function's own template arguments
        lt -= 1
        depth += (head[lt] == ">") - (head[lt] == "<")
        if depth == 0:
            break
    args, cur = [], ""
    for ch in head[lt + 1:-1]:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return head[:lt].split()[-1], tuple(args + [cur.strip()])


def _within(short, long):
    """short can be had from long by deleting template arguments (a dropped template parameter)."""
    it = iter(long)
    return all(x in it for x in short)


def _resigned(a, b):
    """{A's name: B's name} for kernels in one build only that are one kernel under two mangled
    names: the same template and the same template arguments (the function's parameters
    changed), or one's arguments are the other's with some deleted (a template parameter was
    dropped or added).  Only pairs that are unique in both directions."""
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    base = {k: _base(k) for k in only_a + only_b}

    def same(ka, kb):
        (na, xa), (nb, xb) = base[ka], base[kb]
        return na == nb and (_within(xa, xb) or _within(xb, xa))
    fwd = {ka: [kb for kb in only_b if same(ka, kb)] for ka in only_a}
    back = {kb: [ka for ka in only_a if same(ka, kb)] for kb in only_b}
    return {ka: kbs[0] for ka, kbs in fwd.items() if len(kbs) == 1 and len(back[kbs[0]]) == 1}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"A = {sys.argv[1]}: {len(a)} kernels\nB = {sys.argv[2]}: {len(b)} kernels")
    # a kernel template's mangled name holds its template arguments and parameter types: one
    # whose signature changed is paired by its name without them and compared under A's name
    resigned = _resigned(a, b)
    print(f"\n== signature changed (compared below as one kernel): {len(resigned)}")
    for ka, kb in resigned.items():
        print(f"  {ka}\n    -> {kb}")
        b[ka] = b.pop(kb)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    for title, names in (("only in A", only_a), ("only in B", only_b), ("different", differ)):
        print(f"\n== {title}: {len(names)}")
        for k in names:
            print("  " + k)
    for k in differ:
        (ma, ta), (mb, tb) = a[k], b[k]
        print(f"\n--- {k}")
        for m in META:
            if ma[m] != mb[m]:
                print(f"    .{m}: {ma[m]} -> {mb[m]}")
        print(f"    instructions: {len(ta)} -> {len(tb)}")
        sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(ta, tb, "A", "B", lineterm="", n=2))
    return 1 if resigned or only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
