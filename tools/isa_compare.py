#!/usr/bin/env python3
"""Compares the device code of named kernels between two builds of librrtmg_hip.so (development tool; no GPU needed).

    python tools/isa_compare.py <parent librrtmg_hip.so> <this librrtmg_hip.so> [--all] [-o profiles/isa_compare_band_fluxes.txt]

Every gfx950 code object is taken out of the `.hip_fatbin` section of each library (clang offload bundles, one per
translation unit), disassembled with llvm-objdump -d, and cut into functions.  A kernel's instruction stream is its
disassembly with the addresses and encodings dropped, branch targets rewritten as offsets from the function's start and
pc-relative addresses (s_getpc_b64 + s_add_u32 literal) rewritten -- inside .text as an offset from the function's start,
in a data section as the section's name and the 32 bytes found there -- so that code and constants that merely moved inside
the object compare equal.  Prints one line per kernel of KERNELS (a prefix of the
demangled name; all template instances are compared): "identical" or "DIFFERENT", with the instruction count.  --all: one
line per function of the PARENT's code objects instead (every kernel a default call can launch), and a list of the functions
only this build has.  --renamed: a function that differs is compared once more with the register NUMBERS masked (v12 -> v#,
s[4:5] -> s[#x2]: class and width stay); the same instruction sequence on other registers is reported as "renamed"."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# the kernels a change outside the solve must leave alone (prefixes of the demangled names)
KERNELS = ("rrtmg::sw_solve_all_kernel<", "rrtmg::sw_solve_cloudy_kernel(", "rrtmg::sw_solve_all_dir_kernel<", "rrtmg::sw_solve_cloudy_dir_kernel(",
           "rrtmg::lw_solve_all_kernel<", "rrtmg::sw_fluxheat_kernel(", "rrtmg::lw_fluxheat_kernel(", "rrtmg::sw_components_kernel(")


def code_objects(lib, tmp):
    """The gfx950 code objects bundled in `lib`, as files under `tmp`."""
    sec = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + sec, lib, os.path.join(tmp, "copy.so")])
    data = open(sec, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, "co%d.o" % len(out))
                open(path, "wb").write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + 1)
    return out


def functions(lib):
    """{demangled kernel name: [normalised instruction, ...]} of every function in the gfx950 code objects of `lib`."""
    funcs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            sections = []      # (name, address, size) of the object's sections
            for line in subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-h", co], capture_output=True, text=True, check=True).stdout.splitlines():
                f = line.split()
                if len(f) >= 4 and f[0].isdigit():
                    sections.append((f[1], int(f[3], 16), int(f[2], 16)))
            data = {}          # contents of the data sections a kernel's constants live in
            for n, _, z in sections:
                if n.startswith(".rodata") and z:
                    dump = co + n.replace(".", "_")
                    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", "%s=%s" % (n, dump), co, co + ".copy"])
                    data[n] = open(dump, "rb").read()
            name, start, body, getpc = None, 0, [], {}
            for line in text.splitlines():
                m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
                if m:
                    name, start, body = m.group(2), int(m.group(1), 16), []
                    funcs[name] = body
                    continue
                if name is None or not line.startswith(("\t", " ")):
                    continue
                ins = line.split("//")[0].strip()
                if not ins:
                    continue
                at = re.search(r"//\s*([0-9A-Fa-f]+):", line)
                # s_getpc_b64 s[N:N+1] ; s_add_u32 sN, sN, literal: the literal is the distance to a data address
                m = re.match(r"s_getpc_b64 s\[(\d+):", ins)
                if m and at:
                    getpc[m.group(1)] = int(at.group(1), 16) + 4
                m = re.match(r"s_add_u32 s(\d+), s\1, (0x[0-9a-f]+)$", ins)
                if m and m.group(1) in getpc:
                    lit = int(m.group(2), 16)
                    target = getpc.pop(m.group(1)) + (lit - (1 << 32) if lit >> 31 else lit)
                    # (inside .text: from the function's own start, like a branch target)
                    where = next((("fn%+d" % (target - start)) if n == ".text" else
                                  "%s:%s" % (n, data[n][target - a:target - a + 32].hex()) if n in data else "%s+0x%x" % (n, target - a)
                                  for n, a, z in sections if a <= target < a + z), None)
                    if where:
                        ins = "s_add_u32 s%s, s%s, <%s>" % (m.group(1), m.group(1), where)
                # branch targets: "s_cbranch_scc1 12345 <name+0x1c>" -> offset from the function's start
                ins = re.sub(r"\b\d+ <[^>]*\+(0x[0-9a-f]+)>", lambda t: "+" + t.group(1), ins)
                ins = re.sub(r"\b\d+ <[^>]*>", "+0x0", ins)
                body.append(ins)
    for body in funcs.values():      # the padding behind a function's last s_endpgm (s_code_end, s_nop) is not its code
        while body and not body[-1].startswith("s_endpgm"):
            body.pop()
    return funcs


def masked(body):
    """`body` with every register number masked: what is left is the instruction sequence, the register classes and widths."""
    wide = lambda m: "%s[#x%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1)
    return [re.sub(r"\b([vsa])\d+\b", r"\1#", re.sub(r"\b([vsa])\[(\d+):(\d+)\]", wide, ins)) for ins in body]


def compare(parent, this, every=False, renamed=False):
    a, b = functions(parent), functions(this)
    lines, same = [], True
    if every:
        for n in sorted(a):
            ok = n in b and a[n] == b[n]
            same = same and ok
            word = "identical" if ok else "MISSING  " if n not in b else "renamed  " if renamed and masked(a[n]) == masked(b[n]) else "DIFFERENT"
            lines.append("%s  %s  (%d instructions)" % (word, n, len(a[n])))
        lines += ["new        %s  (%d instructions)" % (n, len(b[n])) for n in sorted(set(b) - set(a))]
        return lines, same
    for k in KERNELS:
        names = sorted(n for n in set(a) | set(b) if n.startswith(k) or n.startswith("void " + k))
        if not names:
            lines.append("%-48s MISSING in both builds" % k)
            same = False
        for n in names:
            ok = n in a and n in b and a[n] == b[n]
            same = same and ok
            word = "identical" if ok else "renamed  " if renamed and n in a and n in b and masked(a[n]) == masked(b[n]) else "DIFFERENT"
            lines.append("%s  %s  (%d instructions)" % (word, n, len(b.get(n, a.get(n, [])))))
    return lines, same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("-o", "--output")
    ap.add_argument("--all", action="store_true", help="every function of the parent's code objects, not only KERNELS")
    ap.add_argument("--renamed", action="store_true", help="report a function that differs in register numbers only as \"renamed\"")
    args = ap.parse_args()
    lines, same = compare(args.parent, args.this, args.all, args.renamed)
    text = "\n".join(["# tools/isa_compare.py: device code of the kernels below, parent commit's build vs this build (llvm-objdump -d of the",
                      "# gfx950 code objects, addresses normalised)"] + lines) + "\n"
    sys.stdout.write(text)
    if args.output:
        open(args.output, "w").write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
