#!/usr/bin/env python3
"""Static counts of wave 0's hit-step loops in the gfx950 assembly of otw.hip.

    hipcc <_build.HIPCC_FLAGS> -mllvm -amdgpu-sched-strategy=max-ilp -S --cuda-device-only -x hip csrc/otw.hip -o otw.s
    python tools/otw_w0_loop_stats.py otw.s [kernel-symbol-substring ...]

A hit-step loop is recognised by shape: a loop (label .. backward branch to it) that holds no other loop, one
`s_barrier`, and `v_readlane` (the argmin of the speculated strip is finished on wave 0 only).  For each the script prints
the instructions between header and back edge, the register copies among them, the `s_and_saveexec` regions and the LDS
waits (`s_waitcnt` with an lgkmcnt field) -- the figures of profiles/otw_w0_loop_summary.md."""
import re
import sys

DEFAULT = ["otw_advance_kernelILi512ELi0EfLb1ELi768E", "otw_advance_kernelILi512ELi0EdLb1ELi512E"]


def functions(lines):
    start, name = None, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            start, name = i, m.group(1)
        elif l.startswith(".Lfunc_end") and name:
            yield name, start, i
            name = None


def is_instr(l):
    s = l.strip()
    return bool(s) and not s.startswith((".", ";", "//")) and not s.endswith(":")


def loops(lines, lo, hi):
    labels = {}
    for i in range(lo, hi):
        m = re.match(r"^(\.LBB\w+):", lines[i])
        if m:
            labels[m.group(1)] = i
    out = []
    for i in range(lo, hi):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", lines[i])
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            out.append((labels[m.group(1)], i))
    # one loop per header: its last back edge
    by_head = {}
    for h, b in out:
        by_head[h] = max(b, by_head.get(h, b))
    return sorted(by_head.items())


def is_hit_loop(s):
    # one step per iteration (one barrier per settle path), the strip's argmin finished here (v_readlane: the two
    # reductions of a Both step at least), and none of the general loop's own chains (which read a strip's worth of band
    # and cost slots)
    return 1 <= s["barrier"] <= 2 and s["readlane"] >= 5 and s["ds_read"] < 20


def stats(lines, h, b):
    body = [l.strip() for l in lines[h:b + 1] if is_instr(l)]
    cnt = lambda pat: sum(1 for l in body if re.match(pat, l))
    return {
        "instr": len(body),
        "v_mov": cnt(r"v_mov_b(32|64)_e"),  # (not the DPP moves of the wave reduction)
        "s_mov": cnt(r"s_mov_b(32|64)\s"),
        "saveexec": cnt(r"s_(and|or|andn2)_saveexec"),
        "lds_wait": sum(1 for l in body if l.startswith("s_waitcnt") and "lgkmcnt" in l),
        "ds_read": cnt(r"ds_read"),
        "barrier": cnt(r"s_barrier"),
        "readlane": cnt(r"v_readlane"),
        "branches": cnt(r"s_c?branch"),
    }


def main():
    path = sys.argv[1]
    want = sys.argv[2:] or DEFAULT
    lines = open(path).read().split("\n")
    for name, lo, hi in functions(lines):
        if not any(w in name for w in want):
            continue
        print(name)
        found = [(h, b, stats(lines, h, b)) for h, b in loops(lines, lo, hi)]
        found = [(h, b, s) for h, b, s in found if is_hit_loop(s)]
        for h, b, s in found:
            if any(h2 <= h and b2 >= b and (h2, b2) != (h, b) for h2, b2, _ in found):
                continue  # a loop the compiler formed inside a hit-step loop
            print("  lines %d-%d  " % (h + 1, b + 1) + "  ".join("%s %d" % kv for kv in s.items()))


if __name__ == "__main__":
    main()
