"""tools/asm_wait_states.py on a listing written by hand: no compiler, no GPU.  One s_nop per producer -> consumer class the tool names, in
the hot part, the cold block and outside the substep loop; every expected figure is counted by hand from LISTING.

`s_nop N` stands for N + 1 wait states.  The hot part below holds
    packed -> packed        s_nop 0    1     jb_sim.hpp:200 (called from jb_sim.hpp:900)
    valu -> permlane        s_nop 1    2     jb_lane.hpp:99 (line 0: goes to the next own line; called from jb_sim.hpp:1433)
    dpp -> permlane         s_nop 0    1     jb_lane.hpp:99
    compare -> select       s_nop 1    2     jb_sim.hpp:210
    trans -> valu           s_nop 0    1     jb_sim.hpp:220
    valu -> dpp             s_nop 1    2     jb_sim.hpp:230
    other -> select         s_nop 3    4     jb_sim.hpp:240 (an SALU mask write in front of it; a hexadecimal count)
    select -> select        two s_nop in a row (0 and 1): 1 + 2, both with the same producer and consumer      jb_sim.hpp:250
9 s_nop, 16 wait states, among 26 instructions; the cold block one packed -> valu s_nop 2 (3 wait states) among 5 instructions; outside
the substep loop one valu -> permlane s_nop 1 among 8 instructions."""
import os
import subprocess
import sys

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.append(TOOLS)          # (behind everything else: the tools are scripts with plain names)
import asm_listing  # noqa: E402
import asm_wait_states as ws  # noqa: E402

LISTING = """\
\t.text
\t.file\t1 "/src/jitterbug_amd/csrc" "jb_api.hip"
\t.file\t2 "/src/jitterbug_amd/csrc/jb_sim.hpp"
\t.file\t3 "/src/jitterbug_amd/csrc/jb_lane.hpp"
_ZN12_GLOBAL__N_114jb_step_kernelILi4EEEvNS_5KArgsE:
\t.loc\t1 10 0
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0
\ts_nop 1
\tv_permlane32_swap_b32_e32 v1, v0
.LBB0_1:
\t.loc\t2 100 0
\tv_add_f32_e32 v2, v1, v1
.LBB0_2:
\t.loc\t2 200 7                         ; jitterbug_amd/csrc/jb_sim.hpp:200:7 @[ jitterbug_amd/csrc/jb_sim.hpp:900:3 @[ jitterbug_amd/csrc/jb_api.hip:30:1 ] ]
\tv_pk_fma_f32 v[4:5], v[2:3], v[2:3], v[4:5]
\ts_nop 0
\tv_pk_fma_f32 v[4:5], v[6:7], v[6:7], v[4:5]
\tv_add_f32_e32 v8, v4, v5
\t.loc\t3 0 0
\ts_nop 1
\t.loc\t3 99 12                         ; jitterbug_amd/csrc/jb_lane.hpp:99:12 @[ jitterbug_amd/csrc/jb_sim.hpp:1433:9 @[ jitterbug_amd/csrc/jb_sim.hpp:2062:5 @[ jitterbug_amd/csrc/jb_api.hip:30:1 ] ] ]
\tv_permlane16_swap_b32_e32 v8, v9
\tv_add_f32_dpp v10, v8, v8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1
\ts_nop 0
\tv_permlane32_swap_b32_e32 v10, v11
\t.loc\t2 210 0                         ; jitterbug_amd/csrc/jb_sim.hpp:210:0 @[ jitterbug_amd/csrc/jb_api.hip:30:1 ]
\tv_cmp_lt_f32_e32 vcc, v10, v11
\ts_nop 1
\tv_cndmask_b32_e32 v12, v10, v11, vcc
\t.loc\t2 220 0
\tv_rcp_f32_e32 v13, v12
\ts_nop 0
\tv_mul_f32_e32 v14, v13, v12
\t.loc\t2 230 0
\tv_sub_f32_e32 v15, v14, v13
\ts_nop 1
\tv_mov_b32_dpp v16, v15 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1
\t.loc\t2 240 0
\ts_and_b64 s[8:9], s[8:9], vcc
\ts_nop 0x3
\tv_cndmask_b32_e64 v17, v16, v15, s[8:9]
\t.loc\t2 250 0
\tv_cndmask_b32_e64 v18, v17, v15, s[8:9]
\ts_nop 0
\ts_nop 1
\tv_cndmask_b32_e64 v19, v18, v15, s[10:11]
\t;;#ASMSTART
\t; jb-cold-solve-begin
\t;;#ASMEND
\t.loc\t2 300 0
\tv_pk_mul_f32 v[20:21], v[4:5], v[4:5]
\ts_nop 2
\tv_sub_f32_e32 v22, v20, v21
\tds_write_b32 v0, v22
\ts_waitcnt lgkmcnt(0)
\t;;#ASMSTART
\t; jb-cold-solve-end
\t;;#ASMEND
\t.loc\t2 400 0
\ts_cbranch_scc1 .LBB0_2
\ts_cbranch_scc1 .LBB0_1
\tglobal_store_dword v0, v22, s[0:1]
\ts_endpgm
.Lfunc_end0:
"""


def _fn(tmp_path):
    p = tmp_path / "jb.s"
    p.write_text(LISTING)
    (fn,) = asm_listing.parse(str(p))
    return fn, str(p)


def test_an_s_nop_of_n_stands_for_n_plus_one_wait_states():
    assert [ws.wait_states("\ts_nop %s" % n) for n in ("0", "1", "2", "7", "0x3")] == [1, 2, 3, 8, 4]
    assert ws.wait_states("\tv_nop") == 0 and ws.wait_states("\ts_nop_like 1") == 0 and ws.wait_states("\ts_waitcnt vmcnt(0)") == 0


def test_every_class_is_told_by_its_mnemonic_or_its_dpp_control():
    cases = {"packed": "\tv_pk_add_f32 v[0:1], v[2:3], v[4:5]", "permlane": "\tv_permlane16_swap_b32_e32 v0, v1", "compare": "\tv_cmp_class_f32_e64 s[0:1], v0, v1",
             "select": "\tv_cndmask_b32_e32 v0, v1, v2, vcc", "trans": "\tv_rsq_f32_e32 v0, v1", "valu": "\tv_fma_f32 v0, v1, v2, v3", "other": "\ts_mov_b32 s0, 0"}
    for want, line in cases.items():
        assert ws.classify(line) == want, line
    assert ws.classify("\tv_add_f32_dpp v0, v1, v1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf") == "dpp"
    assert ws.classify("\tv_mov_b32_dpp v0, v1 row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1") == "dpp"
    assert ws.classify("\tds_read_b32 v0, v1") == "other" and ws.classify("\tv_mov_b32_e32 v0, v1") == "valu"
    assert set(cases) | {"dpp"} == set(ws.CLASSES)


def test_counts_and_wait_states_per_part(tmp_path):
    fn, _ = _fn(tmp_path)
    got = {wh: (ws.totals(ws.census(fn, wh)[0]), ws.census(fn, wh)[1]) for wh in ("hot", "cold", "out")}
    assert got == {"hot": ((9, 16), 26), "cold": ((1, 3), 5), "out": ((1, 2), 8)}


def test_producer_and_consumer_classes(tmp_path):
    fn, _ = _fn(tmp_path)
    hot = {k: (n, w) for k, n, w in ws.by_key(ws.census(fn, "hot")[0], ws.class_pair)}
    assert hot == {("packed", "packed"): (1, 1), ("valu", "permlane"): (1, 2), ("dpp", "permlane"): (1, 1), ("compare", "select"): (1, 2), ("trans", "valu"): (1, 1),
                   ("valu", "dpp"): (1, 2), ("other", "select"): (1, 4), ("select", "select"): (2, 3)}
    assert ws.by_key(ws.census(fn, "cold")[0], ws.class_pair) == [(("packed", "valu"), 1, 3)]
    assert ws.by_key(ws.census(fn, "out")[0], ws.class_pair) == [(("valu", "permlane"), 1, 2)]
    ops = {k: w for k, n, w in ws.by_key(ws.census(fn, "hot")[0], ws.op_pair)}
    assert ops[("v_add_f32", "v_permlane16_swap_b32")] == 2 and ops[("v_add_f32_dpp", "v_permlane32_swap_b32")] == 1 and ops[("v_cndmask_b32", "v_cndmask_b32")] == 3


def test_source_lines_and_callers(tmp_path):
    fn, _ = _fn(tmp_path)
    rows = ws.census(fn, "hot")[0]
    own = fn.next_own_line()
    lines = {k: (n, w) for k, n, w in ws.by_key(rows, lambda r: own[r[0]])}
    # the line-0 s_nop in front of the swap goes to the swap's line, not to the add's
    assert lines == {"jb_sim.hpp:200": (1, 1), "jb_lane.hpp:99": (2, 3), "jb_sim.hpp:210": (1, 2), "jb_sim.hpp:220": (1, 1), "jb_sim.hpp:230": (1, 2),
                     "jb_sim.hpp:240": (1, 4), "jb_sim.hpp:250": (2, 3)}
    frames = ws.caller_frames(fn)
    callers = {k: w for k, n, w in ws.by_key(rows, lambda r: frames[ws.consumer_index(fn, r[0])])}
    # what jb_lane.hpp's swap is charged to: the two frames outside it
    assert callers["jb_sim.hpp:1433 < jb_sim.hpp:2062"] == 3
    assert callers["jb_sim.hpp:200 < jb_sim.hpp:900"] == 1


def test_the_report_runs_as_a_script(tmp_path):
    _, path = _fn(tmp_path)
    out = subprocess.check_output([sys.executable, os.path.join(TOOLS, "asm_wait_states.py"), path, "--pairs", "5", "--frames", "5"], text=True)
    lines = out.split("\n")
    assert lines[0].startswith("== jb_step_kernel")
    assert [l.split("|")[1].split() for l in lines[1:4]] == [["s_nop", "9", "(34.6%)", "wait", "states", "16"], ["s_nop", "1", "(20.0%)", "wait", "states", "3"],
                                                            ["s_nop", "1", "(12.5%)", "wait", "states", "2"]]
    assert any(l.split() == ["compare", "->", "select", "1", "2"] for l in lines)
