"""jb_lane.hpp's DPP exchanges on the host: tests/lane_exchange_check.cpp is a stand-alone program (its own main, nothing but the lane
header) that holds the condition under which a DPP move may set bound_ctrl - every lane has a source lane - against a lane-by-lane model of
the DPP controls, and the controls the device helpers use against the Quad<T> emulation the host builds of jb_sim.hpp run on: same lanes,
same bits, fp32 and fp64.  No fused exchange-and-consume helper exists (tools/experiments/dpp_forms.txt: none paid), so there is no
composition to compare here - the exchanges themselves are what the device and the host must agree on."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lane_exchange_check.cpp")
HEADER = os.path.join(HERE, "..", "jitterbug_amd", "csrc", "jb_lane.hpp")


def _build(flags=(), tag=""):
    out = os.path.join(HERE, "_build", "lane_exchange_check" + tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not (os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in (SRC, HEADER, os.path.abspath(__file__)))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Wno-unknown-pragmas"] + list(flags) + ["-o", out, SRC])
    return out


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]


def test_dpp_controls_and_host_emulation_agree():
    _run(_build())


def test_the_same_in_an_unoptimised_build():
    """-O0 -ffp-contract=off: the comparison does not hang on what the optimiser makes of the emulation"""
    _run(_build(("-O0", "-ffp-contract=off"), "_O0"))
