#!/usr/bin/env python3
"""The device code of dp_device.hip in two trees, compared kernel by kernel (cross-compiled, no GPU needed).

  scripts/isa_diff.py CHECKOUT_A CHECKOUT_B [--window MNEMONIC]      both builds: product and -DWHAMD_DEBUG_BUILD (debug against debug)
  scripts/isa_diff.py A.co B.co [--window MNEMONIC]                  two device objects that are already there (a bundle or a plain code object)

A checkout is compiled with the FLAGS of its own Makefile plus --cuda-device-only; the gfx950 object is taken out of the bundle and disassembled.
Per kernel, in the order of B's code object: `identical` (the same instructions, operands included), `same mnemonics` (the same sequence of
mnemonics: register names or immediates differ) or `differs`; for the last two the number of differing lines, whether the multiset of mnemonics is
the same and the first few differences; with --window whether the sequence of mnemonics from the first to the last MNEMONIC is the same.  Then
whether the kernels stand in the same order, and every kernel whose metadata -- registers, spills, scratch, LDS -- differs (all of them with -v).
The exit status says whether everything was identical.  The comparison is on disassembly, not on assembly text: the labels of an inline asm block
carry a counter that changes with the number of expansions, their encodings do not."""
import argparse, difflib, os, re, shutil, subprocess, sys, tempfile
from collections import Counter

LLVM = "/opt/rocm/llvm/bin/"
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw).stdout


def compile_checkout(tree, debug, out):
    csrc = os.path.join(tree, "whatshap_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", mk, re.M).group(1).strip()
    flags = var("FLAGS").replace("$(ARCH)", var("ARCH")).split()
    cmd = [var("HIPCC")] + flags + (["-DWHAMD_DEBUG_BUILD"] if debug else []) + ["--cuda-device-only", "-c", "dp_device.hip", "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return out


def code_object(path, tmp):
    """The gfx950 code object of `path` (which may be a bundle)."""
    with open(path, "rb") as f:
        if f.read(len(BUNDLE_MAGIC)) != BUNDLE_MAGIC:
            return path
    out = os.path.join(tmp, os.path.basename(path) + f".{len(os.listdir(tmp))}.elf")
    run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={path}", f"--output={out}"])
    return out


def kernels_of(path, tmp):
    """(names in the order of the code object, name -> instructions, name -> metadata), names demangled."""
    elf = code_object(path, tmp)
    notes = run([LLVM + "llvm-readelf", "--notes", elf])
    meta, order = {}, []
    for block in re.split(r"^\s*- \.agpr_count", notes, flags=re.M)[1:]:
        sym = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[sym] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in META}
    code, sym = {}, None
    for line in run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", elf]).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1) if m.group(1) in meta else sym   # (a label inside a kernel belongs to the kernel)
            if sym == m.group(1):
                order.append(sym); code[sym] = []
        elif sym and line.startswith("\t"):
            code[sym].append(" ".join(line.split("//")[0].split()))
    plain = {s: s for s in order}
    if shutil.which("c++filt"):   # (the template arguments tell the kernels apart: the parameter list is left out)
        plain = {s: re.sub(r"^void ", "", re.sub(r"\(.*$", "", n.replace("(anonymous namespace)::", ""))) for s, n in zip(order, run(["c++filt"], input="\n".join(order)).splitlines())}
        if len(set(plain.values())) != len(order): plain = {s: s for s in order}
    return [plain[s] for s in order], {plain[s]: code[s] for s in order}, {plain[s]: meta[s] for s in order}


def mnemonics(lines):
    return [l.split()[0] for l in lines if l]


def window(lines, mnemonic):
    m = mnemonics(lines)
    at = [i for i, x in enumerate(m) if x == mnemonic]
    return m[at[0]:at[-1] + 1] if at else []


def compare(a, b, label, args, names=None):
    with tempfile.TemporaryDirectory() as tmp:
        order_a, code_a, meta_a = kernels_of(a, tmp)
        order_b, code_b, meta_b = kernels_of(b, tmp)
    print(f"==== {label}: A = {(names or (a, b))[0]}   B = {(names or (a, b))[1]}")
    same = True
    count = Counter()
    for name in order_b:
        if args.only and not re.search(args.only, name):
            continue
        if name not in code_a:
            print(f"only in B   {name}"); same = False
            continue
        la, lb = code_a[name], code_b[name]
        if la == lb:
            verdict = "identical"
        elif mnemonics(la) == mnemonics(lb):
            verdict = "same mnemonics"
        else:
            verdict = "differs"
        count[verdict] += 1
        if verdict == "identical" and not args.verbose:
            continue
        print(f"{verdict:15s} {name}   ({len(la)} / {len(lb)} instructions)")
        if verdict == "identical":
            continue
        same = False
        ops = [o for o in difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes() if o[0] != "equal"]
        print(f"    differing lines: {sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)}; multiset of mnemonics: "
              f"{'the same' if Counter(mnemonics(la)) == Counter(mnemonics(lb)) else 'DIFFERENT'}"
              + (f"; mnemonics from the first to the last {args.window}: {'the same' if window(la, args.window) == window(lb, args.window) else 'DIFFERENT'}" if args.window else ""))
        for _, i1, i2, j1, j2 in ops[:args.show]:
            for l in la[i1:i2][:4]: print(f"    A {i1:5d}  {l}")
            for l in lb[j1:j2][:4]: print(f"    B {j1:5d}  {l}")
    for name in order_a:
        if name not in code_b:
            print(f"only in A   {name}"); same = False
    print(f"kernels: {len(order_a)} / {len(order_b)}; " + ", ".join(f"{n} {v}" for v, n in count.items()))
    if order_a == order_b:
        print("order of the kernels: the same")
    else:
        same = False
        print("order of the kernels: DIFFERENT")
        for l in difflib.unified_diff(order_a, order_b, "A", "B", lineterm="", n=1): print("    " + l)
    print("metadata (" + " ".join(META) + "):")
    for name in order_b:
        ma, mb = meta_a.get(name), meta_b[name]
        if ma != mb or args.verbose:
            same = same and ma == mb
            fmt = lambda m: " ".join(f"{m[k]:>5d}" for k in META) if m else "-"
            print(f"    {'same    ' if ma == mb else 'DIFFERS '} {name}\n        A {fmt(ma)}\n        B {fmt(mb)}")
    if all(meta_a.get(n) == meta_b[n] for n in order_b) and not args.verbose:
        print("    the same for every kernel")
    return same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a"); ap.add_argument("b")
    ap.add_argument("--window", metavar="MNEMONIC", help="also compare the mnemonics from the first to the last MNEMONIC of a kernel that differs")
    ap.add_argument("--only", metavar="REGEX", help="report only the kernels whose name matches (order and metadata are still compared for all)")
    ap.add_argument("--show", type=int, default=6, help="differences printed per kernel (default 6)")
    ap.add_argument("-v", "--verbose", action="store_true", help="list identical kernels and unchanged metadata too")
    args = ap.parse_args()
    if os.path.isdir(args.a) != os.path.isdir(args.b):
        sys.exit("two checkouts or two device objects")
    if not os.path.isdir(args.a):
        sys.exit(0 if compare(args.a, args.b, "device objects", args) else 1)
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        for debug in (False, True):
            objs = [compile_checkout(os.path.abspath(t), debug, os.path.join(tmp, f"{side}{int(debug)}.co")) for side, t in (("a", args.a), ("b", args.b))]
            same = compare(*objs, "debug build (-DWHAMD_DEBUG_BUILD)" if debug else "product build", args, (args.a, args.b)) and same
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
