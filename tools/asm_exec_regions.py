"""Which stretches of a step kernel run under a narrowed exec mask, where do they sit and what do they guard?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -disable-vector-combine -w -S --cuda-device-only \
          -gline-tables-only [-DJB_DEV_ONLY4] -o /tmp/jb.s jitterbug_amd/csrc/jb_api.hip
    python tools/asm_exec_regions.py /tmp/jb.s [kernel-name-substring] [--all]

(build.py's FLAGS without -shared -fPIC, plus line tables: a listing compile, nothing of it ships.)

A lone wave pays for every lane predicate the compiler turns into control flow: s_and_saveexec + s_cbranch_execz + s_or exec, the
mask arithmetic that feeds them and the s_nop wait states around an exec write - and the region is a block boundary the scheduler does
not move an LDS read across.  This lists every such region of a step kernel:

    where   hot  = the substep loop without its cold block (the line-searched second solve, bracketed by jb-cold-solve-begin / -end),
            cold = that block, out = outside the substep loop;  depth = how many loops (backward branches) enclose the region's start
    len     instructions from the exec write that opens the region to the one that closes it (nested regions included)
    mem     the region holds an LDS / global / scratch / buffer / flat operation (else it is register-only work under a lane predicate)
    loop    the region is itself the body of a loop with a per-lane exit (closed by s_cbranch_execnz back to its start)
    line    source line of the opening exec write (.loc, innermost inlined frame)

A region opens at s_and_saveexec / s_andn2_saveexec / s_or_saveexec (the else half of an if / else) or at `s_xor_b64 exec, exec, sN`;
it closes at the `s_or_b64 exec, exec, ...` that restores the saved mask or - when the saved mask went through a spill or a copy - at
the target of the s_cbranch_execz that follows the opening, whichever comes first.  Only exec-mask instructions, branches, SALU and
s_nop are looked at; nothing here depends on what the vector code computes.
Loops and the substep loop are found like tools/asm_spills.py finds them."""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
show_all = "--all" in sys.argv
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
is_inst = re.compile(r"^\s+(v_|s_|ds_|global_|scratch_|buffer_|flat_)")
is_mem = re.compile(r"^\s+(ds_|global_|scratch_|buffer_|flat_)")
open_re = re.compile(r"^\s+s_(and|andn2|or)_saveexec_b64\s+(s\[\d+:\d+\]|vcc)")
xor_re = re.compile(r"^\s+s_xor_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)")
close_re = re.compile(r"^\s+s_or_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)")
branch_re = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
not_salu = re.compile(r"^\s+s_(nop|waitcnt|branch|cbranch|endpgm|barrier|sleep|load_|buffer_load|setprio|sethalt|code_end)")
mask_re = re.compile(r"^\s+s_(or|and|xor|andn2|orn2|not)_b64\s")

for (i0, name), i1 in zip(starts, ends):
    if want not in name:
        continue
    body = lines[i0:i1]
    inst_idx = [j for j, l in enumerate(body) if is_inst.match(l)]
    inst_pos = {j: k for k, j in enumerate(inst_idx)}
    labels = {}
    loc_at, cur = {}, "?"
    for j, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = j
        m = re.match(r"^\s+\.loc\s+(\d+)\s+(\d+)", l)
        if m and m.group(2) != "0":      # (line 0: compiler-generated, keep the last real line)
            cur = "%s:%s" % (files.get(int(m.group(1)), m.group(1)), m.group(2))
        loc_at[j] = cur
    loops = []
    for j, l in enumerate(body):
        m = branch_re.match(l)
        if m and m.group(1) in labels and labels[m.group(1)] < j:
            loops.append((labels[m.group(1)], j))
    loops = sorted({a: (a, max(b for a2, b in loops if a2 == a)) for a, _ in loops}.values())      # one loop per header label
    by_size = sorted(loops, key=lambda ab: ab[0] - ab[1])
    outer = by_size[0] if by_size else (0, len(body))
    inner = [ab for ab in by_size[1:] if ab[0] >= outer[0] and ab[1] <= outer[1]]
    sub = inner[0] if inner else outer
    cb = [j for j, l in enumerate(body) if "jb-cold-solve-begin" in l]
    ce = [j for j, l in enumerate(body) if "jb-cold-solve-end" in l]
    cold = (cb[0], ce[-1]) if cb and ce else (-1, -1)

    def where(j):
        if cold[0] <= j <= cold[1]:
            return "cold"
        return "hot" if sub[0] <= j <= sub[1] else "out"

    def next_inst(j):
        k = inst_pos.get(j)
        return inst_idx[k + 1] if k is not None and k + 1 < len(inst_idx) else None

    regions = []
    for j in inst_idx:
        l = body[j]
        mo, mx = open_re.match(l), xor_re.match(l)
        if not (mo or mx):
            continue
        saved = mo.group(2) if mo else mx.group(1)
        # the s_cbranch_execz that skips the region, if there is one right behind the opening (s_nop / mask moves may sit between)
        skip_to = None
        k = j
        for _ in range(4):
            k = next_inst(k)
            if k is None:
                break
            mb = re.match(r"^\s+s_cbranch_execz\s+(\.LBB\d+_\d+)", body[k])
            if mb and labels.get(mb.group(1), -1) > j:
                skip_to = labels[mb.group(1)]
                break
            if not re.match(r"^\s+s_", body[k]):
                break
        end, is_loop = None, False
        for k in inst_idx[inst_pos[j] + 1:]:
            if skip_to is not None and k > skip_to:
                end = skip_to
                break
            mc = close_re.match(body[k])
            if mc and (mo is None or mc.group(1) == saved or skip_to is None):
                end = k
                break
            mb = re.match(r"^\s+s_cbranch_execnz\s+(\.LBB\d+_\d+)", body[k])
            if mb and labels.get(mb.group(1), len(body)) <= j + 2 and labels.get(mb.group(1), -1) >= j - 2:
                end, is_loop = k, True
                break
            if k - j > 4000:
                break
        if end is None:
            end = skip_to if skip_to is not None else j
        inside = [k for k in inst_idx if j < k < end]
        regions.append(dict(at=j, end=end, n=len(inside), mem=any(is_mem.match(body[k]) for k in inside), loop=is_loop or any((a >= j and b <= end) for a, b in loops),
                            where=where(j), depth=sum(1 for a, b in loops if a <= j <= b), loc=loc_at[j], op=l.split()[0]))

    def static(pred, wh):
        return sum(1 for j in inst_idx if where(j) == wh and pred(body[j]))

    def nop_states(wh):
        return sum(int(body[j].split()[1], 0) + 1 for j in inst_idx if where(j) == wh and re.match(r"^\s+s_nop\s", body[j]))

    short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:60]
    print("== %s" % short)
    for wh in ("hot", "cold", "out"):
        rs = [r for r in regions if r["where"] == wh]
        sh = [r for r in rs if r["n"] <= 10]
        print("%-4s insts %6d | SALU %5d  s_nop %4d (%4d wait states)  SALU+wait states %5d | saveexec %4d  cbranch_execz %4d  mask ops %4d  loops %3d"
              % (wh, static(lambda l: True, wh), static(lambda l: re.match(r"^\s+s_", l) and not not_salu.match(l), wh), static(lambda l: re.match(r"^\s+s_nop\s", l), wh), nop_states(wh),
                 static(lambda l: re.match(r"^\s+s_", l) and not not_salu.match(l), wh) + nop_states(wh),
                 static(lambda l: "_saveexec_b64" in l, wh), static(lambda l: re.match(r"^\s+s_cbranch_execz", l), wh), static(lambda l: mask_re.match(l), wh),
                 sum(1 for a, b in loops if where(b) == wh)))
        print("     regions %4d | <= 10 insts %4d, of them register-only %4d | register-only of any length %4d" % (len(rs), len(sh), sum(1 for r in sh if not r["mem"]), sum(1 for r in rs if not r["mem"])))
    nocold = [r for r in regions if r["where"] != "cold"]
    sh = [r for r in nocold if r["n"] <= 10]
    print("outside the cold block: regions %d, <= 10 insts %d, of them register-only %d" % (len(nocold), len(sh), sum(1 for r in sh if not r["mem"])))
    by_line = collections.Counter((r["loc"], r["where"]) for r in regions if not r["mem"] and r["n"] <= 10)
    print("register-only regions of <= 10 insts by source line: " + ", ".join("%s[%s]x%d" % (k[0], k[1], v) for k, v in sorted(by_line.items(), key=lambda kv: -kv[1])[:40]))
    print("%-5s %5s %5s %4s %4s %-20s %s" % ("where", "depth", "len", "mem", "loop", "opens with", "line"))
    for r in regions:
        if show_all or r["where"] != "cold":
            print("%-5s %5d %5d %4s %4s %-20s %s" % (r["where"], r["depth"], r["n"], "mem" if r["mem"] else "-", "loop" if r["loop"] else "-", r["op"], r["loc"]))
