"""Are a change's kernels the parent's, instruction for instruction?  (no GPU needed)

    python tools/asm_listing.py -o NEW.s          (in this tree)
    python tools/asm_listing.py -o PARENT.s       (in a checkout of the parent commit)
    python tools/compare_listings.py PARENT.s NEW.s [--expect-new jb_contacts_kernel]

Compares every kernel of the two listings by its instructions and local labels (directives, comments and debug lines aside) and prints
SAME / DIFFERS / NEW / GONE per kernel; exit status 1 when a kernel differs or is gone, or when a new one is not named by --expect-new."""
import re
import sys

import asm_listing


def kernels(path):
    out = {}
    for f in asm_listing.parse(path, want="jb_"):
        out[f.short] = [l for l in f.body if asm_listing.IS_INST.match(l) or re.match(r"^\.LBB", l)]
    return out


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
            same = a[k] == b[k]
            print("SAME   " if same else "DIFFERS", k[:90], len(a[k]), len(b[k]))
            bad += not same
    sys.exit(1 if bad else 0)
