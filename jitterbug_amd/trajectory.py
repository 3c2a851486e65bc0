"""Recorded trajectories: a stack of device snapshots and the world poses read out of it.

`record(venv, n_steps, actions)` steps a JitterbugVecEnv, takes a device snapshot before the first step and after every step (232 bytes
per env each, one launch) into one buffer, and runs ONE readout over the whole stack (JitterbugVecEnv.readout_device): frame k is what a
live readout after step k would have given, bit for bit.  `Trajectory.save_npz` writes chosen envs' frames with the geom shapes and the
names - everything a viewer needs, none in particular: no renderer is in scope.

Hindsight relabelling sits on the same stack: `Trajectory.achieved()`, `Trajectory.relabel(task, targets)` and
`Trajectory.hindsight_targets(strategy)` score the recorded states under any task and any goal with ONE evaluate pass each
(JitterbugVecEnv.evaluate_device) - no restore, no set_state, the env's own state and target are not touched.

torch carries the device buffers, as in jitterbug_amd.planning; the hot paths are the library's own kernels."""
import numpy as np

from . import model


class Trajectory:
    """frames [K+1, N, 33, 12] and clearance [K+1, N, 22] (float32 torch device tensors; rows as JitterbugVecEnv.readout gives them),
    snapshots [K+1, snapshot_bytes] (uint8: the stack itself - restore_device row k to continue from step k) and the packed rows
    [K, N, D+2] = [obs | reward | done] of the steps.  qfrc [K, N, 15] (record(..., forces=True), else None): the contact forces in joint
    space at the state BEFORE step k under action k, as JitterbugVecEnv.forward gives them (0-2: the ground reaction in world axes).
    geom_frc [K, N, 22, 3] and ncon [K, N] (record(..., contacts=True), else None): the floor's force on each geom and the number of
    contacts at the state BEFORE step k under action k, as JitterbugVecEnv.contacts gives them.

    achieved(), relabel() and hindsight_targets() evaluate the task layer on the stack through the env that recorded it (its constant
    tables; its state is only read), so they need that env open."""

    def __init__(self, frames, clearance, snapshots, rows, params, qfrc=None, geom_frc=None, ncon=None, venv=None):
        self.frames, self.clearance, self.snapshots, self.rows, self.qfrc = frames, clearance, snapshots, rows, qfrc
        self.geom_frc, self.ncon = geom_frc, ncon
        self._params = params          # env index -> float64[NPARAM] table that env was simulated with
        self._venv = venv              # the env that recorded the stack: the evaluate passes run on its handle
        self._achieved = None

    @property
    def n_steps(self):
        return int(self.frames.shape[0]) - 1

    def _recorder(self):
        if self._venv is None:
            raise ValueError("this Trajectory was made without the env that recorded it: nothing to evaluate the task layer with")
        return self._venv

    def _evaluate(self, first, count, task, targets, **outputs):
        """ONE evaluate pass over snapshots first .. first + count - 1 on the env's stream, ordered against torch's current stream"""
        import torch
        venv = self._recorder()
        dev = self.snapshots.device
        cur = torch.cuda.current_stream(dev)
        env_stream = torch.cuda.ExternalStream(int(venv.stream), device=dev) if venv.stream else torch.cuda.default_stream(dev)
        env_stream.wait_stream(cur)
        venv.evaluate_device(task, None if targets is None else targets.data_ptr(), snaps_ptr=self.snapshots[first].data_ptr(), n_snaps=count,
                             **{k + "_ptr": v.data_ptr() for k, v in outputs.items()})
        cur.wait_stream(env_stream)

    def achieved(self):
        """float32 [K+1, N, 3] on the device: (px, py, yaw) of every recorded state, the goal it attains in the target's coordinates
        (JitterbugVecEnv.evaluate's 'achieved').  One evaluate pass over the whole stack, cached."""
        import torch
        if self._achieved is None:
            out = torch.empty((self.n_steps + 1, self.rows.shape[1], 3), dtype=torch.float32, device=self.snapshots.device)
            self._evaluate(0, self.n_steps + 1, None, None, achieved=out)
            self._achieved = out
        return self._achieved

    def relabel(self, task=None, targets=None):
        """float32 rows [K, N, D(task) + 2] on the device: row k = [obs | reward | done] of snapshot k + 1 - the state step k led to -
        under `task` (a name or an index; None: the recorded env's own) and `targets` ([N, 3], held over the trajectory, or [K, N, 3];
        None: the targets stored in the snapshots, only with the env's own task).  The done column is the recorded one.  ONE evaluate pass
        over snapshots 1 .. K.  With no arguments the rows are the recorded ones bit for bit on every step with done == 0; after a step
        that ended an episode with an in-kernel reset the snapshot holds the NEXT episode's first state, whose reward is not the recorded
        one."""
        import torch
        venv = self._recorder()
        K, N = self.n_steps, int(self.rows.shape[1])
        tid = venv._task_index(task)
        D = venv.obs_dim if tid < 0 else model.OBS_DIM[model.TASKS[tid]]
        dev = self.snapshots.device
        t = None
        if targets is not None:
            t = torch.as_tensor(targets, dtype=torch.float32, device=dev)
            if t.dim() == 2:
                t = t.unsqueeze(0).expand(K, N, 3)
            t = t.reshape(K, N, 3).contiguous()
        obs = torch.empty((K, N, D), dtype=torch.float32, device=dev)
        rew = torch.empty((K, N, 1), dtype=torch.float32, device=dev)
        if K > 0:
            self._evaluate(1, K, tid if tid >= 0 else None, t, obs=obs, reward=rew)
        return torch.cat([obs, rew, self.rows[:, :, -1:]], dim=2)

    def episode_ends(self):
        """int64 [K, N] on the device: for transition k (the step from snapshot k to snapshot k + 1) the last recorded step of its
        episode, as a snapshot index - j + 1 for the first step j >= k whose recorded done flag is set, K when the recording ends first"""
        import torch
        K = self.n_steps
        done = self.rows[:, :, -1] != 0
        step = torch.arange(1, K + 1, device=done.device, dtype=torch.int64).unsqueeze(1)
        end = torch.where(done, step, torch.full_like(step, K))          # [K, N]: the step that ends here, K where none does
        return torch.flip(torch.cummin(torch.flip(end, (0,)), 0).values, (0,))

    def hindsight_steps(self, strategy="final", seed=0):
        """int64 [K, N] on the device: the goal step g of every transition k (the step from snapshot k to snapshot k + 1), a snapshot index
        with k < g <= episode_ends()[k] - the goal never crosses a recorded done flag.  "final": the episode's last recorded step;
        "future": uniform over the later steps of the episode, from a torch generator seeded with `seed` (reproducible for a seed)."""
        import torch
        if strategy not in ("final", "future"):
            raise ValueError("strategy must be 'final' or 'future', not %r" % (strategy,))
        K, N = self.n_steps, int(self.rows.shape[1])
        end = self.episode_ends()
        if strategy == "final":
            return end
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        u = torch.rand((K, N), generator=gen, dtype=torch.float64).to(end.device)
        first = torch.arange(1, K + 1, device=end.device, dtype=torch.int64).unsqueeze(1)          # transition k may pick k + 1 .. its episode's end
        return torch.minimum(first + torch.floor(u * (end - first + 1).to(torch.float64)).to(torch.int64), end)

    def hindsight_targets(self, strategy="final", seed=0):
        """float32 [K, N, 3] on the device: for transition k a goal the robot DID attain later in the same episode, achieved()[g] at the
        goal step g = hindsight_steps(strategy, seed)[k].  Feed it to relabel().  (After a step that an in-kernel reset ended, the
        snapshot - and so the goal - is the next episode's first state; record with auto_reset=False to keep terminal states.)"""
        import torch
        g = self.hindsight_steps(strategy, seed)
        return torch.gather(self.achieved(), 0, g.unsqueeze(2).expand(g.shape[0], g.shape[1], 3)).contiguous()

    def save_npz(self, path, envs):
        """Write envs `envs` (a list of indices): frames [K+1, E, 33, 12], clearance [K+1, E, 22], geom_type [E, 22]
        (0 sphere, 1 cylinder, 2 box, 3 ellipsoid) and geom_size [E, 22, 3] from the envs' model tables, frame_names [33], geom_names [22],
        body_names [10], envs [E]; with recorded forces also qfrc [K, E, 15], with recorded contacts geom_frc [K, E, 22, 3] and ncon [K, E]."""
        envs = [int(e) for e in envs]
        P = np.stack([np.asarray(self._params(e), dtype=np.float64) for e in envs])
        g = P[:, model.P_GEOM:model.P_GEOM + model.NGEOM * model.GEOM_STRIDE].reshape(len(envs), model.NGEOM, model.GEOM_STRIDE)
        idx = self.frames.new_tensor(envs).long()
        extra = {} if self.qfrc is None else dict(qfrc=self.qfrc.index_select(1, idx).cpu().numpy())
        if self.geom_frc is not None:
            extra.update(geom_frc=self.geom_frc.index_select(1, idx).cpu().numpy(), ncon=self.ncon.index_select(1, idx).cpu().numpy())
        np.savez(path, frames=self.frames.index_select(1, idx).cpu().numpy(), clearance=self.clearance.index_select(1, idx).cpu().numpy(),
                 geom_type=g[:, :, model.G_TYPE].astype(np.int32), geom_size=g[:, :, model.G_SIZE:model.G_SIZE + 3].copy(),
                 frame_names=np.array(model.BODY_NAMES + model.GEOM_NAMES + ("target",)), geom_names=np.array(model.GEOM_NAMES),
                 body_names=np.array(model.BODY_NAMES), envs=np.array(envs, dtype=np.int64), **extra)


def record(venv, n_steps, actions=None, forces=False, contacts=False):
    """Step `venv` n_steps times - with the action tape `actions` [n_steps, N], or with the task's heuristic policy evaluated in the step
    kernel when None - and return the Trajectory.  The steps are the ordinary single-step launches: the env ends in the state, and with
    the rows, n_steps calls of step would have produced; snapshots and the readout only read.  forces=True (needs the action tape): ONE
    forward pass (JitterbugVecEnv.forward_device) over snapshots 0 .. K-1 with the tape keeps qfrc [K, N, 15] - row k is what a live forward
    before step k with action k would have given, bit for bit.  contacts=True (needs the tape too): ONE contact pass
    (JitterbugVecEnv.contacts_device) over the same snapshots keeps geom_frc [K, N, 22, 3] and ncon [K, N], row k likewise."""
    import torch
    K, N = int(n_steps), venv.num_envs
    assert K >= 0
    if (forces or contacts) and actions is None:
        raise ValueError("record(forces=True / contacts=True) needs the action tape: the heuristic policy's actions stay inside the step kernel")
    dev = torch.device("cuda", int(venv.cfg.device_id))
    cur = torch.cuda.current_stream(dev)
    env_stream = torch.cuda.ExternalStream(int(venv.stream), device=dev) if venv.stream else torch.cuda.default_stream(dev)
    nb = venv.snapshot_bytes
    snaps = torch.empty((K + 1, nb), dtype=torch.uint8, device=dev)
    rows = torch.empty((K, N, venv.obs_dim + 2), dtype=torch.float32, device=dev)
    frames = torch.empty((K + 1, N, model.NFRAME, 12), dtype=torch.float32, device=dev)
    clearance = torch.empty((K + 1, N, model.NGEOM), dtype=torch.float32, device=dev)
    tape = None
    if actions is not None:
        tape = torch.as_tensor(np.ascontiguousarray(np.asarray(actions, dtype=np.float32).reshape(K, N))).to(dev)
    env_stream.wait_stream(cur)          # (the tape was copied on the current stream)
    venv.snapshot_device(snaps[0].data_ptr())
    for k in range(K):
        venv.step_many_device(1, None if tape is None else tape[k].data_ptr(), rows[k].data_ptr())
        venv.snapshot_device(snaps[k + 1].data_ptr())
    venv.readout_device(frames.data_ptr(), clearance.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=K + 1)
    qfrc = None
    if forces:
        qfrc = torch.empty((K, N, model.NV), dtype=torch.float32, device=dev)
        if K > 0:
            venv.forward_device(tape.data_ptr(), qfrc_ptr=qfrc.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=K)
    geom_frc = ncon = None
    if contacts:
        geom_frc = torch.empty((K, N, model.NGEOM, 3), dtype=torch.float32, device=dev)
        ncon = torch.empty((K, N), dtype=torch.int32, device=dev)
        if K > 0:
            venv.contacts_device(tape.data_ptr(), ncon_ptr=ncon.data_ptr(), geom_frc_ptr=geom_frc.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=K)
    cur.wait_stream(env_stream)
    venv.synchronize()
    return Trajectory(frames, clearance, snaps, rows, venv.model_params, qfrc, geom_frc, ncon, venv=venv)
