"""What does the contact pass cost per env-state, against a forward pass on the same states?  (run on the GPU box)

    python tools/contacts_timing.py [--parent-lib PATH/libjitterbug_hip.so] [--repeats 15] [--out profiles/contacts_timing.txt]

The pass (jb_contacts_device: one substep on a copy of the state, then the per-slot evaluation) at 4096 env-states - the current state of
4096 envs - and at 65 536 - a stack of 16 snapshots of them -, with geom_frc only and with all four outputs, in microseconds per
env-state.  The yardstick is a forward pass (qacc + qfrc) over the same number of env-states prepared the same way, measured in a child
process of its own on the library named by --parent-lib (the build of the parent commit: JITTERBUG_HIP_LIB; without it, this tree's
library, and the report says so).  Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back
launches.  A record, not a gate."""
import argparse
import json
import sys

import pass_timing as pt

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--forward-only", type=int, default=0, help="(the child process) time forward passes over this many snapshots of 4096 envs and print one JSON line")
args = pt.arguments(ap)

import torch

from jitterbug_amd import model

dev = torch.device("cuda", 0)
N = 4096

if args.forward_only:
    n_snaps = args.forward_only
    env, stream, _, snaps, ctrl = pt.prepared(N, n_snaps)
    m = n_snaps * N
    qacc, qfrc = (torch.zeros((m, model.NV), device=dev, dtype=torch.float32) for _ in range(2))
    torch.cuda.synchronize()
    (med, lo, hi), = pt.timed(args, stream, [lambda: env.forward_device(ctrl.data_ptr(), qacc.data_ptr(), qfrc.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=n_snaps)], 20 if n_snaps == 1 else 3)
    print(json.dumps(dict(m=m, ms=med, lo=lo, hi=hi, variant=env.kernel_variant)))
    env.close()
    sys.exit(0)

lines = ["contact pass against a forward pass (qacc + qfrc) of %s on the same states; median (min .. max) over %d repeats"
         % (pt.whose(args.parent_lib), args.repeats)]
for n_snaps in (1, 16):
    fw = pt.child(__file__, args, "--forward-only", n_snaps)
    env, stream, _, snaps, ctrl = pt.prepared(N, n_snaps)
    m = n_snaps * N
    if n_snaps == 1:
        lines.append("N = %d envs, step kernel variant %s" % (N, env.kernel_variant))
    for all_outputs in (False, True):
        gf = torch.zeros((m, model.NGEOM, 3), device=dev, dtype=torch.float32)
        table = torch.zeros((m, model.NCONTACT, model.CONTACT_WIDTH), device=dev, dtype=torch.float32) if all_outputs else None
        ncon = torch.zeros((m,), device=dev, dtype=torch.int32) if all_outputs else None
        un = torch.zeros((m,), device=dev, dtype=torch.uint8) if all_outputs else None
        torch.cuda.synchronize()

        def contacts():
            env.contacts_device(ctrl.data_ptr(), None if table is None else table.data_ptr(), None if ncon is None else ncon.data_ptr(), gf.data_ptr(),
                                None if un is None else un.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=n_snaps)
        (med, lo, hi), = pt.timed(args, stream, [contacts], 20 if n_snaps == 1 else 3)
        lines.append("%6d env-states (%2d x %d)  %-13s contacts %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  forward %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  ratio %.2f;  mean ncon %s"
                     % (m, n_snaps, N, "all four" if all_outputs else "geom_frc only", med, lo, hi, 1e3 * med / m, fw["ms"], fw["lo"], fw["hi"], 1e3 * fw["ms"] / m, med / fw["ms"],
                        "%.2f" % ncon.float().mean().item() if ncon is not None else "-"))
        del gf, table, ncon, un
    env.close()
pt.report(args, lines)
