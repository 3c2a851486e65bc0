"""How far the GPU's fp32 episode reset (jb_task.hpp episode_reset) lies from the oracle's fp64 one: the drawn root quaternion, the target and the
first observation over many (env, episode) draws.  The record behind tests/episode_inputs.py RESET_QUAT_MEASURED.
The angle of the drawn rotation is u x 2 pi formed in fp32: up to 6.28 its rounding alone is half an ulp of 4.8e-7 rad, the constant's own
rounding adds 2.8e-8 relative, so half the angle - what the quaternion takes the sine and cosine of - carries up to ~2.1e-7 rad before the
sine's own rounding.

usage: python tools/reset_error.py [n_envs] [episodes] [seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jitterbug_amd import model                      # noqa: E402
from jitterbug_amd.vec_env import JitterbugVecEnv    # noqa: E402
from oracle import oracle as O                       # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    episodes = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 11
    for task in ("move_to_pose", "move_in_direction"):
        g = JitterbugVecEnv(n, task, seed=seed)
        o = O.OracleEnv(n, task, model.default_params(), seed=seed)
        worst = dict(quat=0.0, target=0.0, obs=0.0, obs_rel=0.0)
        for _ in range(episodes):
            og, oo = g.reset(), o.reset()
            qg, _, tg = g.get_state()
            qo, _, to = o.get_state()
            assert np.array_equal(qg[:, :3], np.float32(qo[:, :3]).astype(np.float64)) and not qg[:, 7:].any()
            worst["quat"] = max(worst["quat"], float(np.abs(qg[:, 3:7] - qo[:, 3:7]).max()))
            worst["target"] = max(worst["target"], float(np.abs(tg - to).max()))
            worst["obs"] = max(worst["obs"], float(np.abs(og - oo).max()))
            worst["obs_rel"] = max(worst["obs_rel"], float((np.abs(og - oo) - 2e-6 * np.abs(oo)).max()))
        g.close()
        print("%s, %d envs x %d episodes, seed %d: worst |quaternion error| %.4g, worst |target error| %.4g, worst |observation error| %.4g (beyond 2e-6 relative: %.4g)"
              % (task, n, episodes, seed, worst["quat"], worst["target"], worst["obs"], worst["obs_rel"]))


if __name__ == "__main__":
    main()
