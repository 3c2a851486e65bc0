"""Which stretches of a step kernel run under a narrowed exec mask, where do they sit and what do they guard?

    python tools/asm_listing.py [-DJB_DEV_ONLY4] --line-tables -o /tmp/jb.s
    python tools/asm_exec_regions.py /tmp/jb.s [kernel-name-substring] [--all]

A lone wave pays for every lane predicate the compiler turns into control flow: s_and_saveexec + s_cbranch_execz + s_or exec, the
mask arithmetic that feeds them and the s_nop wait states around an exec write - and the region is a block boundary the scheduler does
not move an LDS read across.  This lists every such region of a step kernel:

    where   hot  = the substep loop without its cold block, cold = that block, out = outside the substep loop (tools/asm_listing.py);
            depth = how many loops enclose the region's start
    len     instructions from the exec write that opens the region to the one that closes it (nested regions included)
    mem     the region holds an LDS / global / scratch / buffer / flat operation (else it is register-only work under a lane predicate)
    loop    the region is itself the body of a loop with a per-lane exit (closed by s_cbranch_execnz back to its start)
    line    source line of the opening exec write (.loc, innermost inlined frame; asm_listing.py last_real_line)

A region opens at s_and_saveexec / s_andn2_saveexec / s_or_saveexec (the else half of an if / else) or at `s_xor_b64 exec, exec, sN`;
it closes at the `s_or_b64 exec, exec, ...` that restores the saved mask or - when the saved mask went through a spill or a copy - at
the target of the s_cbranch_execz that follows the opening, whichever comes first.  Only exec-mask instructions, branches, SALU and
s_nop are looked at; nothing here depends on what the vector code computes."""
import collections
import re
import sys

import asm_listing

is_mem = re.compile(r"^\s+(ds_|global_|scratch_|buffer_|flat_)")
open_re = re.compile(r"^\s+s_(and|andn2|or)_saveexec_b64\s+(s\[\d+:\d+\]|vcc)")
xor_re = re.compile(r"^\s+s_xor_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)")
close_re = re.compile(r"^\s+s_or_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)")
execz_re = re.compile(r"^\s+s_cbranch_execz\s+(\.LBB\d+_\d+)")
execnz_re = re.compile(r"^\s+s_cbranch_execnz\s+(\.LBB\d+_\d+)")
not_salu = re.compile(r"^\s+s_(nop|waitcnt|branch|cbranch|endpgm|barrier|sleep|load_|buffer_load|setprio|sethalt|code_end)")
mask_re = re.compile(r"^\s+s_(or|and|xor|andn2|orn2|not)_b64\s")


def regions(fn):
    """every exec-masked region of one function, in the order they open"""
    body, labels, inst_idx, loc_at = fn.body, fn.labels, fn.inst_idx, fn.last_real_line()
    out = []
    for p, j in enumerate(inst_idx):
        l = body[j]
        mo, mx = open_re.match(l), xor_re.match(l)
        if not (mo or mx):
            continue
        saved = mo.group(2) if mo else mx.group(1)
        # the s_cbranch_execz that skips the region, if there is one right behind the opening (s_nop / mask moves may sit between)
        skip_to = None
        for k in inst_idx[p + 1:p + 5]:
            mb = execz_re.match(body[k])
            if mb and labels.get(mb.group(1), -1) > j:
                skip_to = labels[mb.group(1)]
                break
            if not re.match(r"^\s+s_", body[k]):
                break
        end, is_loop = None, False
        for k in inst_idx[p + 1:]:
            if skip_to is not None and k > skip_to:
                end = skip_to
                break
            mc = close_re.match(body[k])
            if mc and (mo is None or mc.group(1) == saved or skip_to is None):
                end = k
                break
            mb = execnz_re.match(body[k])
            if mb and labels.get(mb.group(1), len(body)) <= j + 2 and labels.get(mb.group(1), -1) >= j - 2:
                end, is_loop = k, True
                break
            if k - j > 4000:
                break
        if end is None:
            end = skip_to if skip_to is not None else j
        inside = [k for k in inst_idx if j < k < end]
        out.append(dict(n=len(inside), mem=any(is_mem.match(body[k]) for k in inside), loop=is_loop or any((a >= j and b <= end) for a, b in fn.loops),
                        where=fn.where(j), depth=sum(1 for a, b in fn.loops if a <= j <= b), loc=loc_at[j], op=l.split()[0]))
    return out


def statics(fn, wh):
    """(instructions, SALU, s_nop, wait states, saveexec, s_cbranch_execz, mask operations, loops closing there) of the part wh"""
    text = [fn.body[j] for j in fn.inst_idx if fn.where(j) == wh]
    nops = [l for l in text if re.match(r"^\s+s_nop\s", l)]
    return (len(text), sum(1 for l in text if re.match(r"^\s+s_", l) and not not_salu.match(l)), len(nops), sum(int(l.split()[1], 0) + 1 for l in nops),
            sum(1 for l in text if "_saveexec_b64" in l), sum(1 for l in text if execz_re.match(l)), sum(1 for l in text if mask_re.match(l)), sum(1 for a, b in fn.loops if fn.where(b) == wh))


def summary(rs):
    """(regions, of <= 10 instructions, of those register-only) among rs"""
    sh = [r for r in rs if r["n"] <= 10]
    return len(rs), len(sh), sum(1 for r in sh if not r["mem"])


if __name__ == "__main__":
    args, opts = asm_listing.cli(sys.argv[1:])
    for fn in asm_listing.parse(*args[:2]):
        regs = regions(fn)
        print("== %s" % fn.short[:60])
        for wh in ("hot", "cold", "out"):
            s = statics(fn, wh)
            print("%-4s insts %6d | SALU %5d  s_nop %4d (%4d wait states)  SALU+wait states %5d | saveexec %4d  cbranch_execz %4d  mask ops %4d  loops %3d" % ((wh,) + s[:4] + (s[1] + s[3],) + s[4:]))
            rs = [r for r in regs if r["where"] == wh]
            print("     regions %4d | <= 10 insts %4d, of them register-only %4d | register-only of any length %4d" % (summary(rs) + (sum(1 for r in rs if not r["mem"]),)))
        print("outside the cold block: regions %d, <= 10 insts %d, of them register-only %d" % summary([r for r in regs if r["where"] != "cold"]))
        by_line = collections.Counter((r["loc"], r["where"]) for r in regs if not r["mem"] and r["n"] <= 10)
        print("register-only regions of <= 10 insts by source line: " + ", ".join("%s[%s]x%d" % (k[0], k[1], v) for k, v in sorted(by_line.items(), key=lambda kv: -kv[1])[:40]))
        print("%-5s %5s %5s %4s %4s %-20s %s" % ("where", "depth", "len", "mem", "loop", "opens with", "line"))
        for r in regs:
            if "--all" in opts or r["where"] != "cold":
                print("%-5s %5d %5d %4s %4s %-20s %s" % (r["where"], r["depth"], r["n"], "mem" if r["mem"] else "-", "loop" if r["loop"] else "-", r["op"], r["loc"]))
