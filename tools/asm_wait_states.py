"""Where does a step kernel wait out a data hazard, between which instructions and for which source lines?

    python tools/asm_listing.py [-DJB_DEV_ONLY4] --line-tables -o /tmp/jb.s
    python tools/asm_wait_states.py /tmp/jb.s [kernel-name-substring] [--lines N] [--pairs N] [--frames N]

The hazard recogniser puts `s_nop N` - N + 1 wait states - between a producer and a consumer that the hardware does not interlock: a
packed result into the next VALU instruction, a VALU result into a permlane swap, a compare into the select that reads its mask, a
VALU write of a register a DPP move reads.  A wave that shares its SIMD hides them behind the other waves; a lone wave issues the s_nop
like any instruction and then idles for N more cycles, so each one is an issue slot that computes nothing.  They go away when an
independent instruction stands between producer and consumer - an ORDER of the source, not a change of what is computed.

For every step kernel and each part of it (hot = the substep loop without its cold block, cold = that block, out = the rest:
tools/asm_listing.py) this reports

    the s_nop count and the wait states they stand for,
    per own source line (compiler-generated instructions go to the next line of the project's own files, as in asm_copies.py),
    per producer class -> consumer class, where the producer is the instruction in front of the s_nop and the consumer the one behind it
    (other s_nop skipped), and - with --pairs - per producer mnemonic -> consumer mnemonic,
    with --frames, per class pair and CALLER of the consumer: the operators and exchanges of jb_lane.hpp are inlined everywhere, so their own
    line says little - the two innermost frames outside jb_lane.hpp and the compiler's headers (the .loc comment's inlined-at chain) name
    the routine that has to be reordered.

Classes: packed (v_pk_*), dpp (a VALU instruction in its DPP form), permlane (v_permlane*_swap and the other lane permutes), compare
(v_cmp*), select (v_cndmask), trans (v_rcp / v_rsq / v_sqrt / v_exp / v_log / v_sin / v_cos), valu (any other VALU), other (SALU,
memory, branches, the start of the part).
The counts are static: how often each s_nop runs is not known here."""
import collections
import re
import sys

import asm_listing

NOP = re.compile(r"^\s+s_nop\s+(\S+)")
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)_")
CLASSES = ("packed", "dpp", "permlane", "compare", "select", "trans", "valu", "other")


def mnemonic(line):
    return line.split()[0] if line.split() else ""


def wait_states(line):
    """s_nop N stands for N + 1 wait states; 0 for any other line"""
    m = NOP.match(line)
    return int(m.group(1), 0) + 1 if m else 0


def classify(line):
    op = mnemonic(line)
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith("v_permlane") or op.startswith("v_readlane") or op.startswith("v_writelane") or op.startswith("v_readfirstlane"):
        return "permlane"
    if "_dpp" in op or re.search(r"\b(quad_perm|row_(shl|shr|ror|mirror|half_mirror|bcast|newbcast|share|xmask))", line):
        return "dpp"
    if op.startswith("v_cmp"):
        return "compare"
    if op.startswith("v_cndmask"):
        return "select"
    if TRANS.match(op):
        return "trans"
    return "valu" if op.startswith("v_") else "other"


def short_op(line):
    """the mnemonic without its encoding suffix, DPP kept"""
    return re.sub(r"_(e32|e64)(?=$|_)", "", mnemonic(line))


def census(fn, wh):
    """every s_nop of the part wh of one function: [(body index, wait states, producer line or None, consumer line or None)]"""
    idx = [j for j in fn.inst_idx if fn.where(j) == wh]
    out = []
    for p, j in enumerate(idx):
        w = wait_states(fn.body[j])
        if not w:
            continue
        a = p - 1
        while a >= 0 and wait_states(fn.body[idx[a]]):
            a -= 1
        b = p + 1
        while b < len(idx) and wait_states(fn.body[idx[b]]):
            b += 1
        out.append((j, w, fn.body[idx[a]] if a >= 0 else None, fn.body[idx[b]] if b < len(idx) else None))
    return out, len(idx)


def caller_frames(fn):
    """{body index: "file:line < file:line"} - the two innermost frames outside jb_lane.hpp and the compiler's headers of the .loc in force
    there (line 0 keeps the last real one)"""
    at, cur = {}, "?"
    for j, l in enumerate(fn.body):
        if asm_listing.LOC.match(l) and ";" in l:
            fr = [(f.split("/")[-1], n) for f, n in re.findall(r"([\w./+-]+):(\d+):\d+", l.split(";", 1)[1])]
            if fr and fr[0][1] != "0":
                cur = " < ".join(["%s:%s" % t for t in fr if t[0] != "jb_lane.hpp" and not t[0].startswith("__clang")][:2]) or "%s:%s" % fr[0]
        at[j] = cur
    return at


def consumer_index(fn, j):
    """body index of the first instruction behind the s_nop at j that is no s_nop (j itself at the end of the function)"""
    for k in fn.inst_idx[fn.inst_idx.index(j) + 1:]:
        if not wait_states(fn.body[k]):
            return k
    return j


def totals(rows):
    return len(rows), sum(r[1] for r in rows)


def by_key(rows, key):
    """[(key, s_nop, wait states)], most wait states first"""
    c = collections.defaultdict(lambda: [0, 0])
    for r in rows:
        k = key(r)
        c[k][0] += 1
        c[k][1] += r[1]
    return sorted(((k, v[0], v[1]) for k, v in c.items()), key=lambda t: (-t[2], -t[1], str(t[0])))


def class_pair(r):
    return (classify(r[2]) if r[2] else "other", classify(r[3]) if r[3] else "other")


def op_pair(r):
    return (short_op(r[2]) if r[2] else "-", short_op(r[3]) if r[3] else "-")


if __name__ == "__main__":
    args, opts = asm_listing.cli(sys.argv[1:], ("--lines", "--pairs", "--frames"))
    n_lines, n_pairs, n_frames = int(opts.get("--lines", 30)), int(opts.get("--pairs", 0)), int(opts.get("--frames", 0))
    for fn in asm_listing.parse(*args[:2]):
        own_loc = fn.next_own_line()
        print("== %s" % fn.short[:60])
        for wh in ("hot", "cold", "out"):
            rows, n = census(fn, wh)
            k, w = totals(rows)
            print("%-4s insts %6d | s_nop %4d (%4.1f%%)  wait states %4d | issue slots with them %6d, of those waiting %4.1f%%" % (wh, n, k, 100.0 * k / max(n, 1), w, n - k + w, 100.0 * w / max(n - k + w, 1)))
        for wh in ("hot", "cold"):
            rows, n = census(fn, wh)
            if not rows:
                continue
            print("-- %s: producer class -> consumer class" % wh)
            print("%-22s %6s %12s" % ("", "s_nop", "wait states"))
            for (a, b), k, w in by_key(rows, class_pair):
                print("%-22s %6d %12d" % (a + " -> " + b, k, w))
            if n_pairs:
                pairs = by_key(rows, op_pair)
                print("-- %s: producer -> consumer, %d of %d pairs" % (wh, min(n_pairs, len(pairs)), len(pairs)))
                for (a, b), k, w in pairs[:n_pairs]:
                    print("%-52s %6d %12d" % (a + " -> " + b, k, w))
            if n_frames:
                frames = caller_frames(fn)
                callers = by_key(rows, lambda r: ("%s -> %s" % class_pair(r), frames[consumer_index(fn, r[0])]))
                print("-- %s: class pair and caller of the consumer, %d of %d" % (wh, min(n_frames, len(callers)), len(callers)))
                for (a, b), k, w in callers[:n_frames]:
                    print("%-22s %-44s %6d %12d" % (a, b, k, w))
            lines = by_key(rows, lambda r: own_loc[r[0]])
            print("-- %s: by source line (compiler-generated instructions go to the next own line), %d of %d lines" % (wh, min(n_lines, len(lines)), len(lines)))
            for loc, k, w in lines[:n_lines]:
                print("%-22s %6d %12d" % (loc, k, w))
