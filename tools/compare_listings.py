"""Are a change's kernels the parent's, instruction for instruction?  (no GPU needed)

    python tools/asm_listing.py -o NEW.s          (in this tree)
    python tools/asm_listing.py -o PARENT.s       (in a checkout of the parent commit)
    python tools/compare_listings.py PARENT.s NEW.s [--expect-new jb_contacts_kernel] [--allow-commuted]

Compares every kernel of the two listings by its instructions and local labels (directives, comments and debug lines aside) and prints
SAME / DIFFERS / NEW / GONE per kernel; exit status 1 when a kernel differs or is gone, or when a new one is not named by --expect-new.

--allow-commuted: two instructions also count as equal when they are the same opcode with the same destination and the same source
operands in another order - for the opcodes of COMMUTE any two sources, for those of COMMUTE_MUL (a * b + c) the multiplicands only - every
per-source modifier moving with its operand.  Such a kernel prints COMMUTED n and, below it, the n instruction pairs.  (The compiler orders
the operands of a commutative operation by where its values were defined; an edit elsewhere in the module can turn that order round.)"""
import re
import sys

import asm_listing


def kernels(path):
    out = {}
    for f in asm_listing.parse(path, want="jb_"):
        out[f.short] = [l for l in f.body if asm_listing.IS_INST.match(l) or re.match(r"^\.LBB", l)]
    return out

COMMUTE = {"s_and_b32", "s_and_b64", "s_or_b32", "s_or_b64", "s_xor_b32", "s_xor_b64", "v_add_f32", "v_mul_f32", "v_pk_add_f32", "v_pk_mul_f32", "v_min_f32", "v_max_f32"}
COMMUTE_MUL = {"v_fma_f32", "v_pk_fma_f32", "v_fmac_f32"}
PER_SOURCE = ("op_sel", "op_sel_hi", "neg_lo", "neg_hi")          # trailing arrays with one entry per source (then, for op_sel, the destination's)


def operands(line):
    """(mnemonic, destination, sources, rest) of an instruction line whose trailing modifiers are all understood, else None; a source is
    (its text with the modifiers written on it, its entries of the PER_SOURCE arrays), rest what belongs to no single source"""
    m = re.match(r"\s+(\S+)\s+(.*?)\s*(?:;.*|//.*)?$", line)
    if not m or re.search(r"_(dpp|sdwa)$", m.group(1)):          # (a DPP or SDWA form treats its first source differently)
        return None
    parts, depth, cur = [], 0, ""
    for ch in m.group(2):          # commas and blanks outside brackets separate operands and trailing modifiers
        depth += ch in "[(" and 1 or ch in "])" and -1 or 0
        if depth == 0 and ch in ", ":
            parts.append((cur, ch))
            cur = ""
        else:
            cur += ch
    parts.append((cur, ""))
    parts = [(t, sep) for t, sep in parts if t]
    n_ops = next((i + 1 for i, (t, sep) in enumerate(parts) if sep != ","), len(parts))
    ops, mods = [t for t, _ in parts[:n_ops]], [t for t, _ in parts[n_ops:]]
    if len(ops) < 3:
        return None
    per, rest = [[] for _ in ops[1:]], []
    for mod in mods:
        name, _, val = mod.partition(":")
        if name in PER_SOURCE and re.fullmatch(r"\[[01](,[01])*\]", val) and len(val[1:-1].split(",")) >= len(per):
            bits = val[1:-1].split(",")
            for src, bit in zip(per, bits):
                src.append(name + bit)
            rest.append(name + ":" + ",".join(bits[len(per):]))
        elif mod == "clamp":
            rest.append(mod)
        else:
            return None
    return m.group(1), ops[0], [(t, tuple(q)) for t, q in zip(ops[1:], per)], rest


def commuted(x, y):
    """x and y are one instruction with two of its commutable sources exchanged"""
    a, b = operands(x), operands(y)
    if not a or not b or (a[0], a[1], a[3]) != (b[0], b[1], b[3]):
        return False
    base = re.sub(r"_e(32|64)$", "", a[0])
    if not ((base in COMMUTE and len(a[2]) == 2) or (base in COMMUTE_MUL and len(a[2]) in (2, 3))):
        return False
    return a[2] != b[2] and a[2][1::-1] + a[2][2:] == b[2]


def compare(a, b, allow_commuted=False):
    """None: the kernels differ; else the list of (index, line of a, line of b) of their commuted pairs (empty: the same)"""
    if len(a) != len(b):
        return None
    pairs = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    return pairs if not pairs or (allow_commuted and all(commuted(x, y) for _, x, y in pairs)) else None


if __name__ == "__main__":
    pos, opts = asm_listing.cli(sys.argv[1:], ("--expect-new",))
    a, b = kernels(pos[0]), kernels(pos[1])
    expect, bad = opts.get("--expect-new"), 0
    for k in sorted(set(a) | set(b)):
        if k not in a:
            ok = expect is not None and expect in k
            print("NEW    " if ok else "NEW?   ", k[:90], len(b[k]))
            bad += not ok
        elif k not in b:
            print("GONE    ", k[:90])
            bad += 1
        else:
            pairs = compare(a[k], b[k], "--allow-commuted" in opts)
            print("DIFFERS" if pairs is None else "COMMUTED %d" % len(pairs) if pairs else "SAME   ", k[:90], len(a[k]), len(b[k]))
            for i, x, y in pairs or ():
                print("    %d: %s | %s" % (i, x.strip(), y.strip()))
            bad += pairs is None
    sys.exit(1 if bad else 0)
