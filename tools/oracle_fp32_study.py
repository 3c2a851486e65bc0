"""Supporting evidence for the parity protocol's conditioning (tests/parity_protocol.py MARGIN_TOL): the ORACLE'S OWN algorithm - MuJoCo's
pipeline as oracle/jb_oracle.c restates it: world-frame Jacobian dynamics, dense Cholesky, dense Newton contact solve - compiled in fp32
(`#define double float` after the system headers; a throw-away build under oracle/_build, test infrastructure) and stepped teacher-forced
against its fp64 build.  If a completely different fp32 implementation also fails the tolerance exactly on the env-steps that come within
nanometres of a contact switch, and nowhere else, then those failures are a property of fp32 and the model's discontinuity, not of the HIP
kernel.
    python tools/oracle_fp32_study.py [n_envs] [steps]
Measured (64 envs x 60 steps): entries within tolerance 99.98 %; every env-step with margin >= 30 nm fully within (worst 1.8e-6)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jitterbug_amd import model  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.parity_protocol import within  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
bd = os.path.join(ROOT, "oracle", "_build")
os.makedirs(bd, exist_ok=True)
src = open(os.path.join(ROOT, "oracle", "jb_oracle.c")).read()
inc = '#include "../include/jitterbug_model.h"'
src = src.replace(inc, '#include "%s"\n#define double float' % os.path.join(ROOT, "include", "jitterbug_model.h"))
tmp_c, so = os.path.join(bd, "jb_oracle_fp32.c"), os.path.join(bd, "libjb_oracle32.so")
open(tmp_c, "w").write(src)
subprocess.check_call(["gcc", "-O2", "-fPIC", "-fopenmp", "-shared", "-std=gnu11", "-w", "-o", so, tmp_c, "-lm"])
L = C.CDLL(so)
fp = C.POINTER(C.c_float)


class Opts32(C.Structure):
    _fields_ = [("contacts", C.c_int), ("implicit_damp", C.c_int), ("solver_iters", C.c_int), ("solver_tol", C.c_float), ("warmstart", C.c_int), ("feet_only", C.c_int), ("solver", C.c_int)]


L.jbo_default_opts.argtypes = [C.POINTER(Opts32)]
L.jbo_step_physics.argtypes = [fp, fp, fp, C.c_float, C.c_int, C.POINTER(Opts32), fp, C.c_void_p]
o = Opts32()
L.jbo_default_opts(C.byref(o))
o.solver_tol = 1e-7                      # fp32 cannot resolve the fp64 build's 1e-12
P = model.default_params()
P32 = P.astype(np.float32)
task = "move_from_origin"
env = O.OracleEnv(n, task, P, seed=3)
env.reset()
rng = np.random.default_rng(3)
rows = []
for t in range(steps):
    a = rng.uniform(-1, 1, n)
    q0, v0, tg = env.get_state()
    oo, _, _ = env.step(a, auto_reset=False)
    mar = env.margins()
    for i in range(n):
        q, v = q0[i].astype(np.float32).copy(), v0[i].astype(np.float32).copy()
        L.jbo_step_physics(P32.ctypes.data_as(fp), q.ctypes.data_as(fp), v.ctypes.data_as(fp), np.float32(a[i]), 50, C.byref(o), None, None)
        of = O.observation(P, task, q.astype(np.float64), v.astype(np.float64), tg[i])
        err = np.abs(of - oo[i])
        rows.append((mar[i], within(of, oo[i]).mean(), err.max()))
rows = np.array(rows)
print("fp32 build of the oracle's own algorithm vs its fp64 build, %d env-steps: entries within tolerance %.4f, env-steps fully within %.4f, worst %.3g"
      % (len(rows), rows[:, 1].mean(), (rows[:, 1] == 1).mean(), rows[:, 2].max()))
m = rows[:, 0] >= 3e-8
print("env-steps with margin >= 30 nm (%.1f %%): fully within %.4f, worst %.3g; below: fully within %.4f"
      % (100 * m.mean(), (rows[m, 1] == 1).mean(), rows[m, 2].max(), (rows[~m, 1] == 1).mean() if (~m).any() else float("nan")))
