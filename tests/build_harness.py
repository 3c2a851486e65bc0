"""Builds tests/_build/libjb_hostsim.so: the simulator source compiled for the host (test infrastructure); build_source() builds any other
host harness of tests/ - a library for ctypes or a stand-alone program - into tests/_build."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_build", "libjb_hostsim.so")
SRC = os.path.join(HERE, "host_harness.cpp")
DEPS = [SRC, os.path.join(HERE, "host_run.hpp")] + [os.path.join(HERE, "..", "jitterbug_amd", "csrc", f) for f in ("jb_sim.hpp", "jb_lane.hpp", "jb_step.hpp", "jb_task.hpp", "jb_model_build.hpp", "jb_device_guard.hpp", "jb_owned.hpp", "jb_witness.hpp", "jb_variant.hpp")]


def build(row_k=None, defines=None):
    """row_k: build with a row cache of that many contacts (-DJB_ROW_K): a tiny cache sends almost every contact through the
    beyond-the-cache path (candidate kept, rows recomputed per pass), which ordinary rollouts hardly ever reach.
    defines: {name: value} of further -D options (e.g. JB_LS_CAP=1: a line-searched second solve that gets one outer pass and so ends at
    its cap); the output file is named after them, so every set of options keeps a library of its own."""
    defines = dict(defines or {})
    suffix = ("" if row_k is None else "_rowk%d" % row_k) + "".join("_%s%s" % (k.lower(), defines[k]) for k in sorted(defines))
    out = OUT.replace(".so", suffix + ".so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in DEPS):
        return out
    opts = (["-DJB_ROW_K=%d" % row_k] if row_k is not None else []) + ["-D%s=%s" % (k, defines[k]) for k in sorted(defines)]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas"] + opts + ["-o", out, SRC])
    return out


def depends(src, extra=()):
    """Every file `src` is compiled from, as the compiler itself finds them (g++ -MM) under the -D options of `extra`."""
    rule = subprocess.check_output(["g++", "-std=c++17", "-MM"] + [f for f in extra if f.startswith("-D")] + [src], text=True)
    return rule.replace("\\\n", " ").split()[1:]


def build_source(src, out_name, extra):
    """tests/_build/<out_name> from the one source file `src` with the flags `extra`, rebuilt when any file of depends() is newer."""
    out = os.path.join(HERE, "_build", out_name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not (os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in depends(src, extra))):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + list(extra) + ["-o", out, src])
    return out


if __name__ == "__main__":
    print(build())
