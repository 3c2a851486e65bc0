"""tools/asm_listing.py and the four reports over it (asm_spills / asm_copies / asm_exec_regions / asm_dpp_forms) plus kernel_resources.py and compare_listings.py, on a
listing written by hand: no compiler, no GPU.  Every expected figure below is counted by hand from LISTING (the number in front of a line is its
index within its function), not taken from a run of the tools."""
import os
import subprocess
import sys

import pytest

from jitterbug_amd import build

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.append(TOOLS)          # (behind everything else: the tools are scripts with plain names)
import asm_copies  # noqa: E402
import asm_dpp_forms  # noqa: E402
import asm_exec_regions  # noqa: E402
import asm_listing  # noqa: E402
import asm_spills  # noqa: E402
import compare_listings  # noqa: E402
import kernel_resources  # noqa: E402

# A kernel that is not wanted (with a loop of its own), then a step kernel: the step loop's header .LBB1_1 takes TWO back-branches (43: the
# helper lanes' `continue`, 45: the latch), the substep loop .LBB1_2 (7-41) is nested in it and holds the marked cold block (25-37).  One
# entry per back-branch would find (4,43) "inside" (4,45) and longer than (7,41), and call it the substep loop.
# 14 is a line-0 instruction between jb_sim.hpp:200 and jb_sim.hpp:210, with lines of a file that is not the project's around it.
# 18-23 is a register-only exec region in the hot part, 28-35 one with an LDS operation in the cold block; 9 is a DPP move, 10 copies its result.
LISTING = """\
\t.text
\t.file\t1 "/src/jitterbug_amd/csrc" "jb_api.hip"
\t.file\t2 "/src/jitterbug_amd/csrc/jb_sim.hpp"
\t.file\t3 "/opt/include/hip/math.h"
_ZN2jb17jb_observe_kernelENS_5KArgsEPfS1_:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB0_1:
\tv_mov_b32_e32 v1, v0
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
_ZN12_GLOBAL__N_114jb_step_kernelILi4EEEvNS_5KArgsE:
\t.loc\t1 10 0
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0
.LBB1_1:
\t.loc\t2 100 0
\tv_add_f32_e32 v2, v1, v1
.LBB1_2:
\t.loc\t2 200 0
\tv_mov_b32_dpp v3, v2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
\tv_mov_b32_e32 v4, v3
\t.loc\t3 50 0
\tv_add_f32_dpp v5, v4, v4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf
\t.loc\t2 0 0
\ts_nop 1
\t.loc\t3 60 0
\tv_mul_f32_e32 v6, v5, v5
\t.loc\t2 210 0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB1_3
\tv_fma_f32 v7, v6, v6, v5
\tv_mov_b32_e32 v8, v7
.LBB1_3:
\ts_or_b64 exec, exec, s[2:3]
\t;;#ASMSTART
\t; jb-cold-solve-begin
\t;;#ASMEND
\t.loc\t2 300 0
\ts_and_saveexec_b64 s[6:7], vcc
\ts_cbranch_execz .LBB1_4
\tds_read_b32 v9, v8
\tscratch_load_dword v10, off, off offset:4
\tv_accvgpr_write_b32 a0, v9
\tv_pk_fma_f32 v[12:13], v[12:13], v[12:13], v[12:13]
.LBB1_4:
\ts_or_b64 exec, exec, s[6:7]
\t;;#ASMSTART
\t; jb-cold-solve-end
\t;;#ASMEND
\t.loc\t2 220 0
\tv_accvgpr_read_b32 v11, a0
\ts_cbranch_scc1 .LBB1_2
\t.loc\t1 20 0
\ts_cbranch_vccnz .LBB1_1
\tv_readlane_b32 s8, v11, 0
\ts_branch .LBB1_1
\ts_endpgm
.Lfunc_end1:
"""
INSTS = [2, 3, 6, 9, 10, 12, 14, 16, 18, 19, 20, 21, 23, 28, 29, 30, 31, 32, 33, 35, 40, 41, 43, 44, 45, 46]
HOT = [9, 10, 12, 14, 16, 18, 19, 20, 21, 23, 40, 41]


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = tmp_path_factory.mktemp("asm") / "jb.s"
    p.write_text(LISTING)
    return str(p)


@pytest.fixture(scope="module")
def fn(path):
    fns = asm_listing.parse(path)
    assert len(fns) == 1
    return fns[0]


def test_function_split(path, fn):
    both = asm_listing.parse(path, "kernel")
    assert [f.short for f in both] == ["_ZN2jb17jb_observe_kernelENS_5KArgsEPfS1_", "jb_step_kernelILi4EEEvNS_5KArgsE"]
    assert (len(both[0].body), both[0].inst_idx, both[0].loops) == (6, [1, 3, 4, 5], [(2, 4)])
    assert fn.name == "_ZN12_GLOBAL__N_114jb_step_kernelILi4EEEvNS_5KArgsE" and fn.short == "jb_step_kernelILi4EEEvNS_5KArgsE"
    assert len(fn.body) == 47 and fn.body[0] == fn.name + ":" and fn.body[-1] == "\ts_endpgm"
    assert fn.inst_idx == INSTS
    assert fn.labels == {".LBB1_1": 4, ".LBB1_2": 7, ".LBB1_3": 22, ".LBB1_4": 34}
    assert fn.files == {1: "jb_api.hip", 2: "jb_sim.hpp", 3: "math.h"}


def test_loops_and_parts(fn):
    assert fn.loops == [(4, 45), (7, 41)]          # one loop per header, closed at its last back-branch
    assert (fn.step_loop, fn.substep_loop, fn.cold) == ((4, 45), (7, 41), (25, 37))
    assert fn.hot == HOT
    assert [fn.where(j) for j in (3, 6, 9, 23, 28, 30, 35, 40, 43, 46)] == ["out", "out", "hot", "hot", "cold", "cold", "cold", "hot", "out", "out"]
    assert [(tag, len(idx)) for tag, idx in fn.parts()] == [("whole", 26), ("step loop", 23), ("substep loop", 19), ("hot part", 12), ("cold block", 7)]


def test_no_cold_block(tmp_path):
    p = tmp_path / "plain.s"
    p.write_text(LISTING.replace("jb-cold-solve", "some-other-mark"))
    f, = asm_listing.parse(str(p))
    assert f.cold is None and f.where(30) == "hot" and len(f.hot) == 19
    assert [tag for tag, _ in f.parts()] == ["whole", "step loop", "substep loop"]


def test_line_attributions(fn):
    last, nxt = fn.last_real_line(), fn.next_own_line()
    assert (last[14], nxt[14]) == ("math.h:50", "jb_sim.hpp:210")          # the line-0 s_nop: the two rules differ
    for j, loc in ((3, "jb_api.hip:10"), (10, "jb_sim.hpp:200"), (12, "math.h:50"), (16, "math.h:60"), (18, "jb_sim.hpp:210"), (32, "jb_sim.hpp:300"), (44, "jb_api.hip:20")):
        assert (last[j], nxt[j]) == (loc, loc)
    assert last[0] == "?"


def test_spills_counts(fn):
    c = asm_spills.counts(fn)
    assert list(c["whole"]) == ["insts", "scratch", "writelane", "readlane", "accvgpr", "v_pk_*"]
    assert {tag: list(row.values()) for tag, row in c.items()} == {
        "whole": [26, 1, 0, 1, 2, 1], "step loop": [23, 1, 0, 1, 2, 1], "substep loop": [19, 1, 0, 0, 2, 1], "hot part": [12, 0, 0, 0, 1, 0], "cold block": [7, 1, 0, 0, 1, 1]}


def test_copies_counts(fn):
    parts = dict(fn.parts())          # columns: v_mov_b32 (the DPP move is not one), v_mov_b64, accvgpr_read, accvgpr_write, s_nop
    assert {tag: asm_copies.tally(fn, idx) for tag, idx in parts.items()} == {
        "whole": [3, 0, 1, 1, 1], "step loop": [2, 0, 1, 1, 1], "substep loop": [2, 0, 1, 1, 1], "hot part": [2, 0, 1, 0, 1], "cold block": [0, 0, 0, 1, 0]}
    assert asm_copies.by_line(fn, parts["hot part"]) == [("jb_sim.hpp:210", [1, 0, 0, 0, 1]), ("jb_sim.hpp:200", [1, 0, 0, 0, 0]), ("jb_sim.hpp:220", [0, 0, 1, 0, 0])]
    assert asm_copies.by_line(fn, parts["cold block"]) == [("jb_sim.hpp:300", [0, 0, 0, 1, 0])]


def test_exec_regions_counts(fn):
    regs = asm_exec_regions.regions(fn)
    assert regs == [dict(n=3, mem=False, loop=False, where="hot", depth=2, loc="jb_sim.hpp:210", op="s_and_saveexec_b64"),
                    dict(n=5, mem=True, loop=False, where="cold", depth=2, loc="jb_sim.hpp:300", op="s_and_saveexec_b64")]
    assert asm_exec_regions.summary(regs) == (2, 2, 1)
    assert asm_exec_regions.summary([r for r in regs if r["where"] != "cold"]) == (1, 1, 1)
    # instructions, SALU, s_nop, wait states, saveexec, s_cbranch_execz, mask operations, loops that close there
    assert asm_exec_regions.statics(fn, "hot") == (12, 2, 1, 2, 1, 1, 1, 1)
    assert asm_exec_regions.statics(fn, "cold") == (7, 2, 0, 0, 1, 1, 1, 0)
    assert asm_exec_regions.statics(fn, "out") == (7, 0, 0, 0, 0, 0, 0, 1)


def test_dpp_forms_counts(fn):
    n, by_ctrl, by_use = asm_dpp_forms.forms(fn)
    assert dict(n) == dict(insts=12, mov=2, nop=1, scratch=0, accvgpr=1, folded=1, mov_dpp=1, copied=1)
    assert dict(by_ctrl) == {"quad_perm:[1,0,3,2]": 1} and dict(by_use) == {"v_mov_b32_e32": 1}


def test_kernel_resources_rows():
    remarks = """\
jb_api.hip:9:1: remark: Function Name: _ZN12_GLOBAL__N_114jb_step_kernelILi4EEEvNS_5KArgsE [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     TotalSGPRs: 106 [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     Occupancy [waves/SIMD]: 1 [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     SGPRs Spill: 28 [-Rpass-analysis=kernel-resource-usage]
jb_api.hip:9:1: remark:     LDS Size [bytes/block]: 28084 [-Rpass-analysis=kernel-resource-usage]
"""
    assert kernel_resources.rows(remarks) == {"jb_step_kernelILi4EEEvNS_5KArgsE": ["TotalSGPRs 106", "VGPRs 256", "ScratchSize 0", "Occupancy 1", "SGPRs 28"]}


def test_listing_command_follows_the_product_flags():
    cmd = asm_listing.listing_command("/tmp/out.s")
    shipped = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    assert shipped and "-shared" not in cmd and "-fPIC" not in cmd
    at = [cmd.index(f) for f in shipped]
    assert at == sorted(at) and cmd[at[0]:at[0] + len(shipped)] == shipped          # every flag that ships, in order
    assert "-S" in cmd and "--cuda-device-only" in cmd and "-gline-tables-only" not in cmd
    assert cmd[0] == build.hipcc_path() and cmd[cmd.index("-o") + 1] == "/tmp/out.s" and cmd[-1] == os.path.join(build.CSRC, "jb_api.hip")
    more = asm_listing.listing_command("/tmp/out.s", ["-DJB_DEV_ONLY4"], line_tables=True)
    assert "-DJB_DEV_ONLY4" in more and "-gline-tables-only" in more and [f for f in more if f in shipped] == shipped
    res = asm_listing.compile_command(["-c"], "/tmp/out.o", ["-Rpass-analysis=kernel-resource-usage"])
    assert "-c" in res and "-S" not in res and "--cuda-device-only" in res and [f for f in res if f in shipped] == shipped


KERNEL = "_ZN12_GLOBAL__N_114jb_step_kernelILi4EEEvNS_5KArgsE:\n%s\ts_endpgm\n.Lfunc_end0:\n"
BASE = ["s_and_b64 vcc, s[8:9], s[4:5]", "v_fma_f32 v1, -v2, v3, v4", "v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel_hi:[1,0,1]", "v_sub_f32_e32 v1, v2, v3",
        "v_add_f32_dpp v5, v4, v6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf", "v_mul_f32_e32 v1, v2, v3"]


@pytest.mark.parametrize("at, line, commuted", [
    (0, "s_and_b64 vcc, s[4:5], s[8:9]", True),                                              # a swapped scalar and
    (1, "v_fma_f32 v1, v3, -v2, v4", True),                                                  # swapped multiplicands, the sign with its operand
    (1, "v_fma_f32 v1, -v3, v2, v4", False),                                                 # ... the sign left behind
    (1, "v_fma_f32 v1, -v2, v4, v3", False),                                                 # a swapped addend
    (2, "v_pk_fma_f32 v[0:1], v[4:5], v[2:3], v[6:7] op_sel_hi:[0,1,1]", True),             # the per-source array entries move too
    (2, "v_pk_fma_f32 v[0:1], v[4:5], v[2:3], v[6:7] op_sel_hi:[1,0,1]", False),
    (3, "v_sub_f32_e32 v1, v3, v2", False),                                                  # an opcode outside the list
    (4, "v_add_f32_dpp v5, v6, v4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf", False),   # DPP shuffles its first source only
    (5, "v_mul_f32_e32 v2, v3, v1", False),                                                  # another destination
    (5, "v_mul_f32_e64 v1, v3, v2", False),                                                  # another encoding is another opcode
])
def test_compare_listings_allow_commuted(tmp_path, at, line, commuted):
    new = list(BASE)
    new[at] = line
    a, b = ["\t" + l for l in BASE], ["\t" + l for l in new]
    assert compare_listings.compare(a, a, True) == [] and compare_listings.compare(a, b) is None and compare_listings.compare(a, b[:-1], True) is None
    assert compare_listings.compare(a, b, True) == ([(at, a[at], b[at])] if commuted else None)
    (tmp_path / "a.s").write_text(KERNEL % "".join(l + "\n" for l in a))
    (tmp_path / "b.s").write_text(KERNEL % "".join(l + "\n" for l in b))
    run = lambda *opt: subprocess.run([sys.executable, os.path.join(TOOLS, "compare_listings.py"), str(tmp_path / "a.s"), str(tmp_path / "b.s")] + list(opt), stdout=subprocess.PIPE, text=True)
    plain, allowed = run(), run("--allow-commuted")
    assert plain.returncode == 1 and plain.stdout.startswith("DIFFERS jb_step_kernel")
    assert allowed.returncode == (0 if commuted else 1) and allowed.stdout.startswith("COMMUTED 1 jb_step_kernel" if commuted else "DIFFERS jb_step_kernel")
