"""What do the quad / row exchanges of jb_lane.hpp cost in the hot part of a step kernel's substep loop - separate DPP moves, the copies
behind them, the wait states in front of them - and which instruction consumes each move that the compiler left unfolded?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -disable-vector-combine -w -S --cuda-device-only -o /tmp/jb.s jitterbug_amd/csrc/jb_api.hip
    python tools/asm_dpp_forms.py /tmp/jb.s [kernel-name-substring] [--consumers]

One line per step kernel (the hot part as tools/asm_spills.py delimits it: the substep loop without its cold block): instructions,
v_mov_b32_e32, v_mov_b32_dpp, the folded DPP forms (v_add_f32_dpp and the like), s_nop, scratch operations, and the number of DPP moves
whose result is next copied by a plain v_mov_b32_e32 (the copy a tied "old" operand forces; must be 0).  With --consumers, the unfolded
moves by DPP control and by the first instruction that reads their result."""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
path = args[0]
want = args[1] if len(args) > 1 else "jb_step_kernel"
consumers = "--consumers" in sys.argv
lines = open(path).read().split("\n")
starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\S+:", l)]
ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
is_inst = re.compile(r"^\s+(v_|s_|ds_|global_|scratch_|buffer_|flat_)")


def hot_part(body):
    """indices (into body) of the instructions of the substep loop outside its cold block: tools/asm_spills.py's rule"""
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
    loops.sort(key=lambda ab: ab[0] - ab[1])
    outer = loops[0] if loops else (0, len(body))
    inner = [ab for ab in loops[1:] if ab[0] >= outer[0] and ab[1] <= outer[1]]
    sub = inner[0] if inner else outer
    cb = [j for j, l in enumerate(body) if "jb-cold-solve-begin" in l]
    ce = [j for j, l in enumerate(body) if "jb-cold-solve-end" in l]
    cold = (cb[0], ce[-1]) if cb and ce else (-1, -1)
    return [j for j in inst_idx if sub[0] <= j <= sub[1] and not cold[0] <= j <= cold[1]]


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


for (i0, name), i1 in zip(starts, ends):
    if want not in name:
        continue
    body = lines[i0:i1]
    hot = hot_part(body)
    text = [body[j] for j in hot]
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
    short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:36]
    print("%-36s hot part: insts %6d  v_mov_b32_e32 %4d  v_mov_b32_dpp %4d  folded *_dpp %4d  s_nop %4d  scratch %3d  accvgpr %4d  dpp moves copied next %3d" % (
        short, n["insts"], n["mov"], n["mov_dpp"], n["folded"], n["nop"], n["scratch"], n["accvgpr"], n["copied"]))
    if consumers:
        print("    unfolded moves by control : " + ", ".join("%s %d" % kv for kv in by_ctrl.most_common()))
        print("    unfolded moves by consumer: " + ", ".join("%s %d" % kv for kv in by_use.most_common()))
