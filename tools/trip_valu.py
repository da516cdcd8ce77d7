#!/usr/bin/env python3
"""Static instruction counts of a kernel's main loop from `hipcc -S` output (no GPU): the figures of profiles/grp_dead_slots.txt §2 and
profiles/grp_epl3_slots.txt.

    hipcc <the build's flags> --cuda-device-only -S gdmix_amd/csrc/re_solve.hip -o new.s
    python tools/trip_valu.py new.s [old.s] --match "re_solve_grp_kernel<16, 3, 16, 64, 0>" [--mnemonics]

VALU = mnemonics v_*. "trip" = the largest strongly connected set of basic blocks (for the group kernels: the main loop with the direction
loop inside), the same set of source lines in every build; --span takes the largest union of overlapping backward branches instead, as
grp_dead_slots.txt did (a span of lines, which also holds whatever the compiler placed between the loop's blocks). With two files the counts stand side by side; --mnemonics lists the per-mnemonic difference inside the
trip (what a rewrite of a source loop added or took away)."""
import argparse
import collections
import re
import subprocess


def kernels(path):
    """-> {demangled name without arguments: [instruction / label lines]}"""
    out, cur, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[cur], cur = buf, None
                continue
            line = re.sub(r";.*$", "", line).strip()
            if line and not line.startswith(".") or re.match(r"^\.LBB\d+_\d+:", line):
                buf.append(line)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void ", "", d).split("(")[0]: out[n] for n, d in zip(names, dem)}


def trip_span(lines):
    """-> the lines of the largest union of overlapping backward branches (what profiles/grp_dead_slots.txt §2 counted: it follows the block
    layout, so two builds' figures bound different sets of blocks)"""
    label = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    spans = []
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m:
            t = label.get(m.group(1))
            if t is not None and t < i:
                spans.append((t, i))
    spans.sort()
    merged = []
    for a, b in spans:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    a, b = max(merged, key=lambda s: s[1] - s[0]) if merged else (0, len(lines) - 1)
    return lines[a:b + 1]


def trip_loop(lines):
    """-> the lines of the largest strongly connected set of basic blocks of the control-flow graph: the blocks of the main loop wherever
    the compiler placed them, and none of the prologue or epilogue that a line span picks up between them"""
    starts = {0}
    for i, ln in enumerate(lines):
        if ln.endswith(":"):
            starts.add(i)
        elif re.match(r"s_c?branch|s_endpgm", ln):
            starts.add(i + 1)
    starts = sorted(s for s in starts if s < len(lines))
    block_of = {}
    for b, s in enumerate(starts):
        block_of[s] = b
    label = {ln[:-1]: block_of[i] for i, ln in enumerate(lines) if ln.endswith(":")}
    succ = []
    for b, s in enumerate(starts):
        e = starts[b + 1] if b + 1 < len(starts) else len(lines)
        last = lines[e - 1]
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", last)
        out = []
        if m:
            out.append(label[m.group(1)])
        if not last.startswith(("s_branch", "s_endpgm")) and b + 1 < len(starts):
            out.append(b + 1)
        succ.append(out)
    # Tarjan, iterative
    index, low, on, stack, comps, n = {}, {}, set(), [], [], [0]
    for root in range(len(starts)):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = n[0]
                n[0] += 1
                stack.append(v)
                on.add(v)
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if w not in index:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], index[w])
                continue
            for w in succ[v]:
                if w in on:
                    low[v] = min(low[v], low[w])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                comps.append(comp)
    size = lambda b: (starts[b + 1] if b + 1 < len(starts) else len(lines)) - starts[b]
    best = max(comps, key=lambda c: sum(size(b) for b in c))
    out = []
    for b in sorted(best):
        out += lines[starts[b]:starts[b] + size(b)]
    return out


def counts(lines):
    ins = [ln.split()[0] for ln in lines if not ln.endswith(":")]
    c = collections.Counter(ins)
    pick = lambda pat: sum(v for k, v in c.items() if re.match(pat, k))
    return dict(instructions=len(ins), VALU=pick(r"v_"), v_mov=pick(r"v_mov|v_accvgpr"), v_cndmask=pick(r"v_cndmask"), v_cmp=pick(r"v_cmp"),
                dpp=sum(1 for ln in lines if "dpp" in ln or "row_" in ln or "quad_perm" in ln), fp64=pick(r"v_(fma|mul|add|max|min)_f64"),
                saveexec=pick(r"s_\w+_saveexec"), branch=pick(r"s_cbranch|s_branch"), SALU=pick(r"s_"), lds=pick(r"ds_"), scratch=pick(r"scratch_|buffer_")), c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--match", action="append", required=True, help="demangled kernel name (repeat for several)")
    ap.add_argument("--mnemonics", action="store_true")
    ap.add_argument("--span", action="store_true", help="the trip as a span of lines (the older measure) instead of the loop's own blocks")
    a = ap.parse_args()
    ks = [kernels(f) for f in a.files]
    for name in a.match:
        rows = []
        for k in ks:
            lines = k[name]
            rows.append((counts(lines), counts(trip_span(lines) if a.span else trip_loop(lines))))
        for part, which in ((0, "whole kernel"), (1, "trip")):
            print(f"{name} {which}: " + "  ".join(f"{key} " + " -> ".join(str(r[part][0][key]) for r in rows) for key in rows[0][part][0]))
        if a.mnemonics and len(rows) == 2:
            old, new = rows[0][1][1], rows[1][1][1]
            d = {k: new.get(k, 0) - old.get(k, 0) for k in set(old) | set(new)}
            print("  trip, per mnemonic: " + "  ".join(f"{k} {v:+d}" for k, v in sorted(d.items(), key=lambda kv: -abs(kv[1])) if v))


if __name__ == "__main__":
    main()
