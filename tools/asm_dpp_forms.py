"""What do the quad / row exchanges of jb_lane.hpp cost in the hot part of a step kernel's substep loop - separate DPP moves, the copies
behind them, the wait states in front of them - and which instruction consumes each move that the compiler left unfolded?

    python tools/asm_listing.py -o /tmp/jb.s
    python tools/asm_dpp_forms.py /tmp/jb.s [kernel-name-substring] [--consumers]

One line per step kernel (the hot part of tools/asm_listing.py: the substep loop without its cold block): instructions,
v_mov_b32_e32, v_mov_b32_dpp, the folded DPP forms (v_add_f32_dpp and the like), s_nop, scratch operations, and the number of DPP moves
whose result is next copied by a plain v_mov_b32_e32 (the copy a tied "old" operand forces; must be 0).  With --consumers, the unfolded
moves by DPP control and by the first instruction that reads their result."""
import collections
import re
import sys

import asm_listing


def regs(tok):
    """the 32-bit VGPRs an operand names: v7 -> {7}, v[4:5] -> {4, 5}"""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def operands(l):
    l = l.split(";")[0].strip()
    parts = l.split(None, 1)
    ops = [t.strip() for t in re.split(r",\s*", parts[1].split(" quad_perm")[0].split(" row_")[0])] if len(parts) > 1 else []
    return parts[0], ops


def forms(fn):
    """(counts, unfolded moves by DPP control, unfolded moves by consumer) over the hot part of one function"""
    text = [fn.body[j] for j in fn.hot]
    n = collections.Counter()
    by_ctrl, by_use = collections.Counter(), collections.Counter()
    for k, l in enumerate(text):
        op, ops = operands(l)
        n["insts"] += 1
        n["mov"] += op == "v_mov_b32_e32"
        n["nop"] += op == "s_nop"
        n["scratch"] += "scratch_" in op
        n["accvgpr"] += op.startswith("v_accvgpr")
        if op.endswith("_dpp") and op != "v_mov_b32_dpp":
            n["folded"] += 1
        if op != "v_mov_b32_dpp":
            continue
        n["mov_dpp"] += 1
        ctrl = re.search(r"(quad_perm:\[[\d,]+\]|row_\w+:\d+)", l)
        by_ctrl[ctrl.group(1) if ctrl else "?"] += 1
        dst = regs(ops[0])
        if k + 1 < len(text):
            op2, ops2 = operands(text[k + 1])
            if op2 == "v_mov_b32_e32" and len(ops2) == 2 and regs(ops2[1]) == dst:
                n["copied"] += 1
        use = "none in the block"
        for l2 in text[k + 1:k + 200]:
            op2, ops2 = operands(l2)
            if op2.startswith(("s_cbranch", "s_branch")):
                break
            # the first operand is the destination, except where there is none (stores) or it is read too (accumulating forms)
            all_read = op2.startswith(("v_fmac", "v_mac", "ds_write", "global_store", "scratch_store", "v_cmp"))
            if any(regs(t) & dst for t in (ops2 if all_read else ops2[1:])):
                use = op2
                break
            if ops2 and not all_read and regs(ops2[0]) & dst:
                use = "overwritten"
                break
        by_use[use] += 1
    return n, by_ctrl, by_use


if __name__ == "__main__":
    args, opts = asm_listing.cli(sys.argv[1:])
    for fn in asm_listing.parse(*args[:2]):
        n, by_ctrl, by_use = forms(fn)
        print("%-36s hot part: insts %6d  v_mov_b32_e32 %4d  v_mov_b32_dpp %4d  folded *_dpp %4d  s_nop %4d  scratch %3d  accvgpr %4d  dpp moves copied next %3d" % (
            fn.short[:36], n["insts"], n["mov"], n["mov_dpp"], n["folded"], n["nop"], n["scratch"], n["accvgpr"], n["copied"]))
        if "--consumers" in opts:
            print("    unfolded moves by control : " + ", ".join("%s %d" % kv for kv in by_ctrl.most_common()))
            print("    unfolded moves by consumer: " + ", ".join("%s %d" % kv for kv in by_use.most_common()))
