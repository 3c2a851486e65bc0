"""Where do a step kernel's register spills sit - in the substep loop (hot) or only around it (once per control step / per launch)?

    python tools/asm_listing.py -o /tmp/jb.s
    python tools/asm_spills.py /tmp/jb.s [kernel-name-substring]

For every step kernel: static instruction count, the scratch_ / v_writelane / v_readlane operations and the packed fp32 instructions
(v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) split by the loop they are in (tools/asm_listing.py: step loop, substep loop, hot part,
cold block)."""
import re
import sys

import asm_listing

COLUMNS = [("insts", lambda l: True), ("scratch", lambda l: "scratch_" in l), ("writelane", lambda l: "v_writelane" in l), ("readlane", lambda l: "v_readlane" in l),
           ("accvgpr", lambda l: "v_accvgpr" in l), ("v_pk_*", lambda l: re.match(r"^\s+v_pk_(fma|mul|add)_f32", l) is not None)]
TAGS = {"whole": "whole        %s", "step loop": "step loop    %s", "substep loop": "substep loop %s", "cold block": " - cold block %s",
        "hot part": " - hot part  %s   (the loop without its cold block: the line-searched second solve)"}


def counts(fn):
    """{part: {column: count}} of one function"""
    return {tag: {c: sum(1 for j in idx if pred(fn.body[j])) for c, pred in COLUMNS} for tag, idx in fn.parts()}


if __name__ == "__main__":
    for fn in asm_listing.parse(*sys.argv[1:3]):
        for tag, row in counts(fn).items():
            print("%-44s " % (fn.short[:44] if tag == "whole" else "") + TAGS[tag] % ("insts %6d  scratch %4d  writelane %4d  readlane %4d  accvgpr %4d  v_pk_* %4d" % tuple(row.values())))
