"""tests/build_harness.py build_source: a target's dependencies are what the compiler finds, not a hand-kept list."""
import os

from tests import build_harness as bh


def test_dependencies_hold_headers_the_hand_kept_lists_lacked():
    """include/jitterbug_model.h comes in through jb_model_build.hpp and tests/pass_harness.hpp through the harness: neither was in the
    readout test's list; host_run.hpp and jb_forward.hpp only come in with the -D options the substep harnesses set themselves"""
    names = {os.path.basename(d) for d in bh.depends(os.path.join(bh.HERE, "readout_harness.cpp"))}
    assert {"readout_harness.cpp", "pass_harness.hpp", "jitterbug_model.h", "jb_readout.hpp", "jb_snapshot.hpp"} <= names and "host_run.hpp" not in names
    assert "jb_default_params.h" in {os.path.basename(d) for d in bh.depends(os.path.join(bh.HERE, "readout_harness.cpp"), ["-O1", "-DJBR_MAIN"])}
    assert "host_run.hpp" in {os.path.basename(d) for d in bh.depends(os.path.join(bh.HERE, "forward_harness.cpp"))}


def test_touching_a_header_included_through_another_triggers_a_rebuild(tmp_path, monkeypatch):
    (tmp_path / "inner.hpp").write_text("static int inner() { return 7; }\n")
    (tmp_path / "outer.hpp").write_text('#include "inner.hpp"\n')
    src = tmp_path / "probe.cpp"
    src.write_text('#include "outer.hpp"\nextern "C" int probe() { return inner(); }\n')
    compiles = []
    real = bh.subprocess.check_call
    monkeypatch.setattr(bh.subprocess, "check_call", lambda cmd, *a, **k: (compiles.append(cmd), real(cmd, *a, **k))[1])
    flags = ["-O0", "-fPIC", "-shared"]
    out = bh.build_source(str(src), "libjb_builder_probe_%d.so" % os.getpid(), flags)
    try:
        assert len(compiles) == 1 and os.path.exists(out)
        assert bh.build_source(str(src), os.path.basename(out), flags) == out and len(compiles) == 1          # up to date: nothing runs
        later = os.path.getmtime(out) + 5
        os.utime(tmp_path / "inner.hpp", (later, later))
        bh.build_source(str(src), os.path.basename(out), flags)
        assert len(compiles) == 2
    finally:
        os.remove(out)
