"""Sampling-based planning on the batched simulator: the simulator as its own exact model.

An MPPI planner (model-predictive path integral control; the family also covers CEM and random shooting) copies the state of G "plant"
robots into G x M lanes of a "model" env (JitterbugVecEnv.restore_device with the fork map src[j] = j // M: one launch, bit-exact - the
model lanes ARE the plant, warm start and episode clocks included), rolls M candidate action tapes K steps ahead per robot and scores
them on the device (score_tapes_device: one fused K-step launch + one return kernel), and averages the tapes with softmax weights.

torch carries the device buffers and the update, as in jitterbug_amd.distributed; the update is [K, G*M]-sized plumbing, not a hot
path.  Every piece of planner state lives in the MPPIPlanner object."""
import numpy as np

from .vec_env import JitterbugVecEnv


class MPPIPlanner:
    """MPPI over action tapes for G robots at once.

        planner = MPPIPlanner("move_from_origin", n_groups=G, n_candidates=M, horizon=K)
        plant.snapshot_device(snap.data_ptr())            # or blob = plant.save_state()
        actions = planner.plan(snap.data_ptr())           # float32 [G], one action per plant env

    The plant must hold G envs of the same task (and, for the prediction to be exact, the same model, kernel variant and
    envs_per_wave as the planner's env - see include/jitterbug_hip.h)."""

    def __init__(self, task, n_groups, n_candidates, horizon, gamma=1.0, temperature=1.0, noise_sigma=0.5, seed=0, device_id=0, **env_kwargs):
        import torch
        self.torch = torch
        self.G, self.M, self.K = int(n_groups), int(n_candidates), int(horizon)
        assert self.G >= 1 and self.M >= 1 and self.K >= 1
        self.gamma, self.temperature, self.noise_sigma = float(gamma), float(temperature), float(noise_sigma)
        assert self.temperature > 0
        self.device = torch.device("cuda", int(device_id))
        self.env = JitterbugVecEnv(self.G * self.M, task, seed=seed, device_id=device_id, **env_kwargs)
        n = self.G * self.M
        self._src_host = (np.arange(n) // self.M).astype(np.int32)          # lane j models plant env j // M
        self._src = torch.from_numpy(self._src_host).to(self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self.nominal = torch.zeros((self.K, self.G), device=self.device, dtype=torch.float32)      # the tape the candidates are drawn around
        self.candidates = torch.zeros((self.K, n), device=self.device, dtype=torch.float32)        # last plan(): candidate tapes, lane j = g * M + m
        self.returns = torch.zeros((n,), device=self.device, dtype=torch.float32)                  # last plan(): their (discounted) returns
        self.alive = torch.zeros((n,), device=self.device, dtype=torch.int32)                      # ... and the steps each counted
        self._env_stream = torch.cuda.ExternalStream(int(self.env.stream), device=self.device) if self.env.stream else torch.cuda.default_stream(self.device)

    def close(self):
        self.env.close()

    def plan(self, plant_snapshot):
        """plant_snapshot: a device pointer (int) to a snapshot of the G plant envs (snapshot_device), or a save_state() blob.
        Returns the next action of every plant env, float32 [G] on the device; the nominal tape is shifted by one step.  The plant's
        snapshot is only read."""
        torch = self.torch
        K, G, M = self.K, self.G, self.M
        cur = torch.cuda.current_stream(self.device)
        # candidates = nominal + clipped Gaussian noise (candidate 0 of every group is the nominal tape itself)
        noise = torch.randn((K, G, M), generator=self._gen, device=self.device, dtype=torch.float32) * self.noise_sigma
        noise[:, :, 0] = 0.0
        self.candidates = (self.nominal[:, :, None] + noise).clamp_(-1.0, 1.0).reshape(K, G * M).contiguous()
        self._env_stream.wait_stream(cur)                      # (the tapes - and a device snapshot - were produced on the current stream)
        if isinstance(plant_snapshot, (int, np.integer)):
            self.env.restore_device(int(plant_snapshot), n_src=G, src_ptr=self._src.data_ptr())
        else:
            self.env.load_state(plant_snapshot, src=self._src_host)
        self.env.score_tapes_device(K, self.candidates.data_ptr(), self.gamma, self.returns.data_ptr(), self.alive.data_ptr())
        cur.wait_stream(self._env_stream)
        self.nominal = self.update(self.candidates, self.returns)
        action = self.nominal[0].clone()
        self.nominal = torch.cat([self.nominal[1:], self.nominal[-1:]], dim=0)      # shift: the last action is held
        return action

    def update(self, candidates, returns):
        """The softmax-weighted average of the candidate tapes per group, in fp64: w = softmax((R - max R) / temperature) over a group's
        M candidates, tape[k, g] = sum_m w[g, m] * candidate[k, g, m]."""
        torch = self.torch
        R = returns.double().view(self.G, self.M)
        w = torch.softmax((R - R.max(dim=1, keepdim=True).values) / self.temperature, dim=1)
        return (candidates.double().view(self.K, self.G, self.M) * w[None]).sum(dim=2).float()

    def best_tape(self):
        """The arg-max candidate of the last plan() per group and the return the model predicts for it: (tapes [K, G], returns [G])."""
        R = self.returns.view(self.G, self.M)
        best = R.argmax(dim=1)
        idx = self.torch.arange(self.G, device=self.device)
        return self.candidates.view(self.K, self.G, self.M)[:, idx, best].contiguous(), R[idx, best].clone()
