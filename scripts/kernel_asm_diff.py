#!/usr/bin/env python3
"""Compare the kernels of two builds of device assembly, text against text.

    hipcc <the flags of _build.py for that file> --cuda-device-only -S x.hip -o x.s
    kernel_asm_diff.py --old old/a.s old/b.s --new new/a.s [--map 'OLD_RE=NEW' ...]

Every function of the ``.s`` files is cut out from its symbol label to its ``.Lfunc_end`` label
(that includes the ``.amdhsa_kernel`` descriptor: registers, LDS, scratch). Comments and blank
lines are dropped, ``.LBB<n>_<m>`` labels lose the function number ``n``, and the function's own
symbol becomes ``<self>``, so two functions compare equal exactly when their instructions,
operands, labels and descriptor agree. Functions are paired by their demangled name without the
parameter list (``c++filt`` or ``llvm-cxxfilt``; the mangled name if neither is installed);
``--map`` rewrites an old name first (a regular expression and its replacement, as ``re.sub``).

Prints ``IDENTICAL`` or the differing lines per function. A ``.amdhsa_kernarg_size`` line may
differ (an added empty argument changes nothing the kernel executes); it is reported and
tolerated. Any other difference, or a function present on one side only, exits with status 1.
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
FUNC_TYPE = re.compile(r"^\s*\.type\s+([\w$.]+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
BLOCK = re.compile(r"\.LBB\d+_")
TOLERATED = ".amdhsa_kernarg_size"


def functions(path):
    """{symbol: [normalised lines]} of one assembly file."""
    out, declared, name, body = {}, set(), None, []
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if name is None:
            m = FUNC_TYPE.match(line)
            if m:
                declared.add(m.group(1))
            m = LABEL.match(line)
            if m and m.group(1) in declared:
                name, body = m.group(1), []
                own = re.compile(r"(?<![\w$])" + re.escape(name) + r"(?![\w$])")  # the whole symbol only
            continue
        if FUNC_END.match(line):
            out[name], name = body, None
            continue
        line = own.sub("<self>", BLOCK.sub(".LBB_", line)).strip()
        if line:
            body.append(line)
    if name is not None:
        raise SystemExit("%s: function %s has no .Lfunc_end" % (path, name))
    return out


def short_names(symbols):
    """Demangled names without return type and parameter list, in the order of ``symbols``."""
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not symbols:
        return list(symbols)
    text = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    names = []
    for full in text.splitlines():
        depth, cut = 0, len(full)
        for i, ch in enumerate(full):  # the first "(" outside template brackets opens the parameter list
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0 and not full.startswith("(anonymous namespace)", i):
                cut = i
                break
        names.append(full[:cut].split(" ", 1)[-1] if full.startswith("void ") else full[:cut])
    return names


def load(paths, rules=()):
    table = {}
    for p in paths:
        funcs = functions(p)
        for sym, name in zip(funcs, short_names(list(funcs))):
            for pat, rep in rules:
                name = re.sub(pat, rep, name)
            if name in table:
                raise SystemExit("%s: %s appears twice" % (p, name))
            table[name] = funcs[sym]
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True, metavar="S", help="assembly of the reference build")
    ap.add_argument("--new", nargs="+", required=True, metavar="S", help="assembly of the build under test")
    ap.add_argument("--map", action="append", default=[], metavar="OLD_RE=NEW",
                    help="rename old functions before pairing (re.sub on the short demangled name)")
    a = ap.parse_args()
    rules = [tuple(m.split("=", 1)) for m in a.map]
    old, new = load(a.old, rules), load(a.new)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%-72s ONLY IN %s" % (name, "OLD" if name in old else "NEW"))
            bad += 1
            continue
        diff = [d for d in difflib.unified_diff(old[name], new[name], "old", "new", n=0, lineterm="")
                if d[0] in "+-" and d[:3] not in ("+++", "---")]
        hard = [d for d in diff if not d[1:].startswith(TOLERATED)]
        verdict = "IDENTICAL" if not diff else ("IDENTICAL but " + TOLERATED if not hard else "DIFFERENT")
        print("%-72s %s (%d lines)" % (name, verdict, len(new[name])))
        for d in diff:
            print("    " + d)
        bad += bool(hard)
    print("%d functions compared, %d differ" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
