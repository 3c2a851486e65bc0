"""Which instructions of a step kernel only move data, where do they sit and which source lines do they come from?

    python tools/asm_listing.py [-DJB_DEV_ONLY4] --line-tables -o /tmp/jb.s
    python tools/asm_copies.py /tmp/jb.s [kernel-name-substring] [--lines N] [--cold]

A lone wave issues one VALU instruction in four cycles whether it computes or copies.  This counts, for every step kernel, the five
mnemonics that compute nothing

    v_mov_b32 (the plain _e32 / _e64 forms: a DPP or SDWA move is an exchange, tools/asm_dpp_forms.py), v_mov_b64,
    v_accvgpr_read, v_accvgpr_write (values parked in the accumulation registers), s_nop (wait states)

split whole / step loop / substep loop / hot part / cold block (tools/asm_listing.py), and then per source line (.loc, innermost inlined
frame) for the hot part - with --cold for the cold block as well.  An instruction the compiler generated (line 0: copies it inserted,
wait states) is attributed to the next line of the project's own files that follows it (asm_listing.py next_own_line).  Lines are listed
by their total, the first N of them (default 40).
The counts are static.  Nothing here depends on what the vector code computes; it names only the five mnemonics above and reports."""
import collections
import re
import sys

import asm_listing

KINDS = [("v_mov_b32", re.compile(r"^\s+v_mov_b32(_e32|_e64)?\s")), ("v_mov_b64", re.compile(r"^\s+v_mov_b64(_e32|_e64)?\s")),
         ("accvgpr_read", re.compile(r"^\s+v_accvgpr_read")), ("accvgpr_write", re.compile(r"^\s+v_accvgpr_write")), ("s_nop", re.compile(r"^\s+s_nop\s"))]


def kind(l):
    for k, (_, rx) in enumerate(KINDS):
        if rx.match(l):
            return k
    return -1


def tally(fn, idx):
    """the five columns over the instructions idx"""
    t = [0] * len(KINDS)
    for j in idx:
        if kind(fn.body[j]) >= 0:
            t[kind(fn.body[j])] += 1
    return t


def by_line(fn, idx):
    """[(source line, the five columns)] over the instructions idx, largest total first"""
    own_loc, c = fn.next_own_line(), collections.defaultdict(list)
    for j in idx:
        if kind(fn.body[j]) >= 0:
            c[own_loc[j]].append(j)
    return sorted(((loc, tally(fn, js)) for loc, js in c.items()), key=lambda kv: (-sum(kv[1]), kv[0]))


if __name__ == "__main__":
    args, opts = asm_listing.cli(sys.argv[1:], ("--lines",))
    n_lines = int(opts.get("--lines", 40))
    for fn in asm_listing.parse(*args[:2]):
        parts = dict(fn.parts())
        print("== %s" % fn.short[:60])
        print("%-13s %6s | " % ("", "insts") + " ".join("%13s" % k for k, _ in KINDS) + " | %5s %6s" % ("all 5", "share"))
        for tag, idx in parts.items():
            t = tally(fn, idx)
            print("%-13s %6d | " % (" - " + tag if tag in ("hot part", "cold block") else tag, len(idx)) + " ".join("%13d" % x for x in t) + " | %5d %5.1f%%" % (sum(t), 100.0 * sum(t) / max(len(idx), 1)))
        for tag in ["hot part" if fn.cold else "substep loop"] + (["cold block"] if fn.cold and "--cold" in opts else []):
            rows = by_line(fn, parts[tag])
            print("-- %s by source line (compiler-generated instructions go to the next own line), %d of %d lines" % (tag, min(n_lines, len(rows)), len(rows)))
            print("%-22s " % "line" + " ".join("%13s" % k for k, _ in KINDS) + " | %5s" % "all 5")
            for loc, t in rows[:n_lines]:
                print("%-22s " % loc + " ".join("%13d" % x for x in t) + " | %5d" % sum(t))
