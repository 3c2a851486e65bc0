"""Which instructions of a step kernel only move data, where do they sit and which source lines do they come from?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -disable-vector-combine -w -S --cuda-device-only \
          -gline-tables-only [-DJB_DEV_ONLY4] -o /tmp/jb.s jitterbug_amd/csrc/jb_api.hip
    python tools/asm_copies.py /tmp/jb.s [kernel-name-substring] [--lines N] [--cold]

(build.py's FLAGS without -shared -fPIC, plus line tables: a listing compile, nothing of it ships.)

A lone wave issues one VALU instruction in four cycles whether it computes or copies.  This counts, for every step kernel, the five
mnemonics that compute nothing

    v_mov_b32 (the plain _e32 / _e64 forms: a DPP or SDWA move is an exchange, tools/asm_dpp_forms.py), v_mov_b64,
    v_accvgpr_read, v_accvgpr_write (values parked in the accumulation registers), s_nop (wait states)

split whole / step loop / substep loop / hot part / cold block with tools/asm_spills.py's own delimiting (loops from backward branches,
the substep loop the largest loop inside the outermost one, the cold block bracketed by jb-cold-solve-begin / -end), and then per source
line (.loc, innermost inlined frame) for the hot part - with --cold for the cold block as well.  An instruction the compiler generated
(line 0: copies it inserted, wait states) is attributed to the next line of jb_sim.hpp / jb_lane.hpp / jb_api.hip that follows it: the
copy in front of a v_permlane32_swap belongs to the swap.  Lines are listed by their total, the first N of them (default 40).
The counts are static.  Nothing here depends on what the vector code computes; it names only the five mnemonics above and reports."""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
show_cold = "--cold" in sys.argv
n_lines = 40
if "--lines" in sys.argv:
    n_lines = int(sys.argv[sys.argv.index("--lines") + 1])
    args.remove(sys.argv[sys.argv.index("--lines") + 1])
path = args[0]
want = args[1] if len(args) > 1 else "jb_step_kernel"
lines = open(path).read().split("\n")
starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\S+:", l)]
ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
files = {}
for l in lines:
    m = re.match(r'^\s+\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
OWN = ("jb_sim.hpp", "jb_lane.hpp", "jb_api.hip")
is_inst = re.compile(r"^\s+(v_|s_|ds_|global_|scratch_|buffer_|flat_)")
KINDS = [("v_mov_b32", re.compile(r"^\s+v_mov_b32(_e32|_e64)?\s")), ("v_mov_b64", re.compile(r"^\s+v_mov_b64(_e32|_e64)?\s")),
         ("accvgpr_read", re.compile(r"^\s+v_accvgpr_read")), ("accvgpr_write", re.compile(r"^\s+v_accvgpr_write")), ("s_nop", re.compile(r"^\s+s_nop\s"))]


def kind(l):
    for k, (_, rx) in enumerate(KINDS):
        if rx.match(l):
            return k
    return -1


for (i0, name), i1 in zip(starts, ends):
    if want not in name:
        continue
    body = lines[i0:i1]
    inst_idx = [j for j, l in enumerate(body) if is_inst.match(l)]
    labels = {}
    for j, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = j
    loops = []
    for j, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < j:
            loops.append((labels[m.group(1)], j))
    loops.sort(key=lambda ab: ab[0] - ab[1])          # largest first (tools/asm_spills.py)
    outer = loops[0] if loops else (0, len(body))
    inner = [ab for ab in loops[1:] if ab[0] >= outer[0] and ab[1] <= outer[1]]
    sub = inner[0] if inner else outer
    cb = [j for j, l in enumerate(body) if "jb-cold-solve-begin" in l]
    ce = [j for j, l in enumerate(body) if "jb-cold-solve-end" in l]
    cold = (cb[0], ce[-1]) if cb and ce else None

    # source line of every body line: its own .loc, or - line 0 - the next .loc of the project's own files
    own_loc, pending, cur, cur_zero = {}, [], "?", False
    for j, l in enumerate(body):
        m = re.match(r"^\s+\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            f = files.get(int(m.group(1)), m.group(1))
            if m.group(2) == "0":
                cur_zero = True
            else:
                cur, cur_zero = "%s:%s" % (f, m.group(2)), False
                if f in OWN:
                    for k in pending:
                        own_loc[k] = cur
                    pending = []
        if cur_zero:
            pending.append(j)
        else:
            own_loc[j] = cur
    for k in pending:          # (line 0 to the end of the function: the last real line)
        own_loc[k] = cur

    def tally(lo, hi, skip=None):
        t = [0] * (len(KINDS) + 1)
        for j in inst_idx:
            if lo <= j <= hi and not (skip and skip[0] <= j <= skip[1]):
                t[len(KINDS)] += 1
                k = kind(body[j])
                if k >= 0:
                    t[k] += 1
        return t

    def by_line(lo, hi, skip=None):
        c = collections.defaultdict(lambda: [0] * len(KINDS))
        for j in inst_idx:
            if lo <= j <= hi and not (skip and skip[0] <= j <= skip[1]):
                k = kind(body[j])
                if k >= 0:
                    c[own_loc[j]][k] += 1
        return sorted(c.items(), key=lambda kv: (-sum(kv[1]), kv[0]))

    short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:60]
    print("== %s" % short)
    head = "%-13s %6s | " % ("", "insts") + " ".join("%13s" % k for k, _ in KINDS) + " | %5s %6s" % ("all 5", "share")
    print(head)
    regions = [("whole", (0, len(body)), None), ("step loop", outer, None), ("substep loop", sub, None)]
    if cold:
        regions += [(" - hot part", sub, cold), (" - cold block", cold, None)]
    for tag, (lo, hi), skip in regions:
        t = tally(lo, hi, skip)
        five = sum(t[:len(KINDS)])
        print("%-13s %6d | " % (tag, t[len(KINDS)]) + " ".join("%13d" % x for x in t[:len(KINDS)]) + " | %5d %5.1f%%" % (five, 100.0 * five / max(t[len(KINDS)], 1)))
    listed = [("hot part" if cold else "substep loop", sub, cold)] + ([("cold block", cold, None)] if cold and show_cold else [])
    for tag, (lo, hi), skip in listed:
        rows = by_line(lo, hi, skip)
        print("-- %s by source line (compiler-generated instructions go to the next own line), %d of %d lines" % (tag, min(n_lines, len(rows)), len(rows)))
        print("%-22s " % "line" + " ".join("%13s" % k for k, _ in KINDS) + " | %5s" % "all 5")
        for loc, t in rows[:n_lines]:
            print("%-22s " % loc + " ".join("%13d" % x for x in t) + " | %5d" % sum(t))
