"""The one place that knows a device listing of jb_api.hip: how it is compiled (the flags the library ships with) and how it is read.

    python tools/asm_listing.py [-DJB_DEV_ONLY4 ...] [--line-tables] -o OUT.s

compiles the listing that tools/asm_spills.py, asm_copies.py, asm_exec_regions.py, asm_dpp_forms.py and asm_wait_states.py report on (asm_copies.py,
asm_exec_regions.py and asm_wait_states.py name source lines: build theirs with --line-tables); tools/kernel_resources.py compiles with the same flags.  Nothing of it ships.

parse(path) gives one Function per kernel.  Loops come from backward branches (a label .LBBn_m defined above its s_branch / s_cbranch):
ONE loop per header label, closed at its LAST back-branch - several back-branches to one header (a `continue`, a rotated latch) are one
loop, not nested ones, and counting them apart would let a shortened copy of the control-step loop pass for the loop inside it.  The
step loop is the largest loop, the substep loop the largest loop inside it, the cold block of the substep loop (the line-searched second
contact solve, jb_sim.hpp substep_impl) is bracketed by the jb-cold-solve-begin / -end comments, the hot part is the substep loop
without it.  Spans are (first, last) line indices into Function.body, both inclusive."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = ("jb_sim.hpp", "jb_lane.hpp", "jb_api.hip")
IS_INST = re.compile(r"^\s+(v_|s_|ds_|global_|scratch_|buffer_|flat_)")
BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")
LOC = re.compile(r"^\s+\.loc\s+(\d+)\s+(\d+)")


def compile_command(mode, out, extra=()):
    """hipcc with build.py's FLAGS minus -shared -fPIC (the code that ships), device only; mode is what makes it a listing or an object"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from jitterbug_amd import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    return [build.hipcc_path()] + flags + list(mode) + ["--cuda-device-only"] + list(extra) + ["-o", out] + [os.path.join(build.CSRC, s) for s in build.SOURCES]


def listing_command(out, defines=(), line_tables=False):
    return compile_command(["-S"], out, list(defines) + (["-gline-tables-only"] if line_tables else []))


def build_listing(out, defines=(), line_tables=False):
    subprocess.check_call(listing_command(out, defines, line_tables))
    return out


def short_name(name):
    return re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)


def within(span, j):
    return span is not None and span[0] <= j <= span[1]


class Function:
    def __init__(self, name, body, files):
        self.name, self.short, self.body, self.files = name, short_name(name), body, files
        self.inst_idx = [j for j, l in enumerate(body) if IS_INST.match(l)]
        self.labels = {l[:l.index(":")]: j for j, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)}
        last = {}          # header line -> its last back-branch
        for j, l in enumerate(body):
            m = BRANCH.match(l)
            if m and self.labels.get(m.group(1), j) < j:
                last[self.labels[m.group(1)]] = j
        self.loops = sorted(last.items())
        by_size = sorted(self.loops, key=lambda ab: ab[0] - ab[1])          # largest first
        self.step_loop = by_size[0] if by_size else (0, len(body))
        inner = [ab for ab in by_size[1:] if ab[0] >= self.step_loop[0] and ab[1] <= self.step_loop[1]]
        self.substep_loop = inner[0] if inner else self.step_loop
        cb = [j for j, l in enumerate(body) if "jb-cold-solve-begin" in l]
        ce = [j for j, l in enumerate(body) if "jb-cold-solve-end" in l]
        self.cold = (cb[0], ce[-1]) if cb and ce else None
        self.hot = self.insts(self.substep_loop, self.cold)

    def insts(self, span, skip=None):
        return [j for j in self.inst_idx if within(span, j) and not within(skip, j)]

    def where(self, j):
        return "cold" if within(self.cold, j) else "hot" if within(self.substep_loop, j) else "out"

    def parts(self):
        """(tag, instruction indices) of whole / step loop / substep loop and, where there is a cold block, hot part / cold block"""
        p = [("whole", self.inst_idx), ("step loop", self.insts(self.step_loop)), ("substep loop", self.insts(self.substep_loop))]
        return p + ([("hot part", self.hot), ("cold block", self.insts(self.cold))] if self.cold else [])

    def _locs(self):
        for j, l in enumerate(self.body):
            m = LOC.match(l)
            yield j, m and (self.files.get(int(m.group(1)), m.group(1)), m.group(2))

    # The two ways to give a source line ("file:line" of .loc, innermost inlined frame) to every body line.  They differ only for what the
    # compiler generated (.loc line 0) and both are meant: a region is named by the statement it was opened for, a copy by its consumer.
    def last_real_line(self):
        """line 0 keeps the last real line: an exec write the compiler placed belongs to the predicate above it (asm_exec_regions.py)"""
        at, cur = [], "?"
        for j, loc in self._locs():
            if loc and loc[1] != "0":
                cur = "%s:%s" % loc
            at.append(cur)
        return at

    def next_own_line(self):
        """line 0 goes to the next line of the project's OWN files: the copy in front of a v_permlane32_swap belongs to the swap
        (asm_copies.py); line 0 up to the end of the function keeps the last real line"""
        at, pending, cur, zero = {}, [], "?", False
        for j, loc in self._locs():
            if loc:
                zero = loc[1] == "0"
                if not zero:
                    cur = "%s:%s" % loc
                    if loc[0] in OWN:
                        at.update((k, cur) for k in pending)
                        pending = []
            if zero:
                pending.append(j)
            else:
                at[j] = cur
        at.update((k, cur) for k in pending)
        return at


def parse(path, want="jb_step_kernel"):
    lines = open(path).read().split("\n")
    files = {}
    for l in lines:
        m = re.match(r'^\s+\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\S+:", l)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    return [Function(name, lines[i0:i1], files) for (i0, name), i1 in zip(starts, ends) if want in name]


def cli(argv, valued=()):
    """the tools' command line: (positional arguments, {--option: value or True}); the options named in `valued` take the next word"""
    pos, opts, it = [], {}, iter(argv)
    for a in it:
        if a in valued:
            opts[a] = next(it)
        elif a.startswith("--"):
            opts[a] = True
        else:
            pos.append(a)
    return pos, opts


if __name__ == "__main__":
    defines, opts = cli(sys.argv[1:], ("-o",))
    print(" ".join(listing_command(opts["-o"], defines, "--line-tables" in opts)))
    build_listing(opts["-o"], defines, "--line-tables" in opts)
