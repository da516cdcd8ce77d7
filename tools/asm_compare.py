"""Is the device code of every kernel the same as another commit's? Without a GPU: both trees' .hip units are compiled to gfx950
assembly with the build's flags (`hipcc -S --cuda-device-only`) and compared kernel by kernel after stripping comments, section
directives and per-compile labels. Kernels are matched by demangled name; --gained-false names kernels whose template list gained a
trailing `false` argument since the other commit (a new compile-time parameter whose `false` instantiation must be the old kernel);
--renamed old=new,... names kernels and types that were renamed since: the other commit's names and lines are read under the new names.
--bool-as-int reads a boolean template argument and an integer one of the same value as one (a template parameter that went from
`bool` to `int`: the symbols' `Lb0E` / `Lb1E` became `Li0E` / `Li1E`, in the kernels' own names and in every call of a device function).
A kernel that moved to another unit is found there by its name.

    python tools/asm_compare.py --parent HEAD~1 \\
        --gained-false re_solve_grp_kernel,re_solve_wave_kernel,re_solve_block_kernel,re_variance_full_kernel,re_solve_tall_kernel,re_solve_tall_team_kernel
    python tools/asm_compare.py --parent HEAD~1 --bool-as-int

Prints per unit: kernels identical / different / only in this tree; exit status 1 if a kernel of the other commit differs or is missing.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdmix_amd import build      # noqa: E402


def compile_units(csrc, out):
    """-> {unit: assembly file} for the units of build.SOURCES that exist under csrc (a unit added since the other commit is not there)."""
    os.makedirs(out, exist_ok=True)
    flags = [f for f in build.FLAGS if f != "-shared"] + os.environ.get("GDMIX_EXTRA_FLAGS", "").split()

    def one(f):
        dst = os.path.join(out, f + ".s")
        subprocess.run([build.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, f), "-o", dst], check=True, stderr=subprocess.DEVNULL)
        return dst
    units = [f for f in build.SOURCES if os.path.exists(os.path.join(csrc, f))]
    with ThreadPoolExecutor(len(units)) as ex:
        return dict(zip(units, ex.map(one, units)))


BOOL_AS_INT = False


def functions(path, renamed=()):
    """-> {mangled name: [normalised lines]}, {mangled name: kernel descriptor text}; `renamed`: (old, new) identifiers, applied to the
    text in their mangled (length-prefixed) spelling"""
    txt = open(path).read()
    if BOOL_AS_INT:
        txt = re.sub(r"L[bi]([01])E", r"Li\1E", txt)
    for o, n in renamed:
        txt = txt.replace(f"{len(o)}{o}", f"{len(n)}{n}")
    out, cur, buf = {}, None, []
    for line in txt.splitlines():
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and cur is None and not line.startswith(".L"):
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[cur], cur = buf, None
                continue
            line = re.sub(r";.*$", "", line).rstrip()
            if not line or re.match(r"\s*\.(text|section)\b", line):
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"\.Ltmp\d+|\.L__unnamed_\d+|\.Lfunc_begin\d+|\.Lfunc_end\d+", ".L", line)
            buf.append(line.replace(cur, "SELF"))
    meta = {m.group(1): m.group(2).replace(m.group(1), "SELF") for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S)}
    return out, meta


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d).split("(")[0] for n, d in zip(names, res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD", help="the commit to compare the working tree with")
    ap.add_argument("--gained-false", default="", help="comma list of kernel names whose template arguments gained a trailing `false`")
    ap.add_argument("--renamed", default="", help="comma list of old=new: kernel or type names of the other commit that were renamed since")
    ap.add_argument("--diff", action="store_true", help="print the lines of a kernel that differs")
    ap.add_argument("--bool-as-int", action="store_true", help="template arguments false / true and 0 / 1 are the same argument")
    a = ap.parse_args()
    global BOOL_AS_INT
    BOOL_AS_INT = a.bool_as_int
    renamed = [tuple(r.split("=")) for r in a.renamed.split(",") if r]
    gained = [g for g in a.gained_false.split(",") if g]

    def key(d):
        if any(re.match(rf"(\w+::)*{re.escape(g)}\b", d) for g in gained):
            d = re.sub(r"<false>$", "", re.sub(r", false>$", ">", d))
        return d
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "archive", a.parent, "gdmix_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        s_old = compile_units(os.path.join(old, "gdmix_amd", "csrc"), os.path.join(tmp, "s_old"))
        s_new = compile_units(build.CSRC, os.path.join(tmp, "s_new"))
        new = {unit: functions(s_new[unit]) for unit in build.SOURCES}
        # a kernel that left its unit is looked for, by name, in the other units of this tree
        fn_all = {k: v for f, _ in new.values() for k, v in f.items()}
        mn_all = {k: v for _, m in new.values() for k, v in m.items()}
        moved_by_key = {key(d): k for k, d in demangle(list(fn_all)).items()}
        for unit in build.SOURCES:
            if unit not in s_old:
                print(f"{unit}: a new unit, {len(new[unit][0])} functions")
                continue
            fo, mo = functions(s_old[unit], renamed)
            fn, mn = new[unit]
            do, dn = demangle(list(fo)), demangle(list(fn))
            new_by_key = {key(dn[k]): k for k in fn if k not in fo}
            same = diff = moved = 0
            for k in fo:
                k2 = k if k in fn else new_by_key.get(do[k])      # same symbol, or the symbol that gained its `false`
                f2, m2 = fn, mn
                if k2 is None and (k in fn_all or do[k] in moved_by_key):
                    k2 = k if k in fn_all else moved_by_key[do[k]]
                    print(f"{unit}: {do[k]} is in another unit now")
                    moved += 1
                    f2, m2 = fn_all, mn_all
                if k2 is None:
                    print(f"{unit}: MISSING {do[k]}")
                    bad += 1
                elif fo[k] == f2[k2] and mo.get(k) == m2.get(k2):
                    same += 1
                else:
                    print(f"{unit}: DIFFERENT {do[k]} ({len(fo[k])} -> {len(f2[k2])} lines)")
                    if a.diff:
                        print("\n".join(difflib.unified_diff(fo[k] + mo.get(k, "").splitlines(), f2[k2] + m2.get(k2, "").splitlines(), "other", "this tree", lineterm="", n=1)))
                    diff += 1
                    bad += 1
            print(f"{unit}: {same} identical, {diff} different, {len(new[unit][0]) - same - diff + moved} only in this tree")
    print("every kernel of the other commit is unchanged" if not bad else f"{bad} kernels differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
