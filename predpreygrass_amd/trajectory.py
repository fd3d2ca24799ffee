"""AgentTrajectories: per-agent trajectories from the tensor API, without leaving the device.

The rows of `BatchedPredPreyGrass` / `BatchedRedQueen` change with every call (dead rows are dropped, last call's newborns are
merged into sorted position, new newborns are appended), so row r of call t + 1 is in general not the agent of row r of call t.
`env.link()` (`ppg_link`, include/ppg.h) gives the map between two consecutive outputs; this class stores it next to the rewards
and runs the backward recursions of a learner -- discounted returns, GAE -- through it: one gather per step, the whole horizon in
one kernel launch (`env.backward()`, `ppg_backward`).

    traj = AgentTrajectories(env, horizon=T)
    for t in range(T):
        env.step(actions)            # or random_actions=True, with or without auto_reset
        traj.record()                # after EVERY step: the link compares with the output the previous record() saw
    G = traj.returns(0.99)           # float64 [T,B,S]; G[t, b, r] belongs to the agent in row r of call t
    A = traj.gae(values, 0.99, 0.95)
    G, A = traj.returns_and_gae(values, 0.99, 0.95)   # both in ONE launch

What it stores per step, in preallocated [T,B,S] device tensors: `reward` (float64), `in_use`, `terminated` (PPG_ROW_DIED),
`truncated` (PPG_ROW_TRUNC) and `next_row` (int16): the row the agent of row r of call t has in call t + 1, or -1 -- it died, the
env was reset in between (auto-reset: ids restart, nothing links across episodes), or t is the last recorded step.  An agent's
successor term is zero where `next_row` is -1 or the row terminated / was truncated in call t:

    G[t] = reward[t] + gamma * G[t + 1][next_row[t]]

so the horizon's last step is treated like an episode end; record one step more than is used to bootstrap from values instead.
The recursions run in the `ppg_backward` kernel (csrc/ppg_backward.h: one wavefront per env, step t + 1 in LDS): as a torch loop
over the horizon -- about ten small launches per step, kept verbatim as `returns_torch()` / `gae_torch()` -- GAE over 128 steps of
4096 envs took 20.8 ms, twice the rollout it post-processes, against 0.56 ms (profiles/EXPERIMENTS.md, `ppg_backward`); both give the
same bits.
Recording (`record()`) is one launch too: `env.record()` (`ppg_record`, csrc/ppg_record.h) is the link kernel followed by the stores
of the step.  As torch ops behind `ppg_link` -- about nineteen small launches, kept verbatim as `record_torch()` -- a recorded step of
4096 envs took 162.2 µs launch to launch, with the kernel 115.5 µs, where the step alone takes 99.6 µs and step + `link()` 113.5 µs
(profiles/EXPERIMENTS.md, `ppg_record`); both give the same bytes.

    traj = AgentTrajectories(env, horizon=T, step_on_device=True)   # the step index is an int32 device tensor, `traj.t_dev`
    loop = GraphedCollector(env, traj)                              # actions + step + record captured ONCE as a HIP graph
    loop.replay(T - 1)                                              # (the uncaptured warm pass was step 0); no host work per step

With `step_on_device` the kernel reads the step index when it runs and an increment follows it on the same stream, so nothing in
the launch depends on a host value and a recorded step can be replayed; `len(traj)` and the backward methods read the index back
once.  A record past the horizon then stores nothing (it still links) instead of raising.  Not for `SubBatchedPredPreyGrass` as a
whole: give each sub-batch its own AgentTrajectories.

What the agents saw and did is stored next to that on request, compacted: `obs_rows=(n_pred, n_prey)` gives the trajectory an
`ObservationStore`, and `record(actions)` then also appends the observation rows in use -- about a fifth of the [B,capacity] rows at
the default population -- to one dense tensor per species (`env.record_obs()`, `ppg_record_obs`, csrc/ppg_obs_store.h: two launches,
nothing read back, so it replays inside GraphedCollector's graph).  The slot a row lands in is the learner's sample index:

    traj = AgentTrajectories(env, horizon=T, obs_rows=(T * B * 12, T * B * 40))
    for t in range(T):
        env.step(actions); traj.record(actions)        # `actions` answered the observations stored one record() earlier
    G, A = traj.returns_and_gae(values, 0.99, 0.95)
    n, obs, index, action = traj.samples(PREY)         # dense [n,C,R,R], int64 [n] flat (t,b,r), int8 [n]; one read-back
    g, a = traj.flat(G, PREY), traj.flat(A, PREY)      # [n]: G.reshape(-1)[index]

`action[k]` is the action taken FROM the observation in slot k; it is written by the record() one step later, so the samples of the
last recorded step (and of rows whose env was not stepped again) hold `_abi.ACTION_UNSET`.  Rows that no longer fit the store are
dropped whole and counted (`store.counts()`).

What the BEHAVIOUR policy thought of every sample -- log pi_old(a|o) for PPO's ratio, the entropy, the logits for a KL term -- is stored
in the same slots on request: `logp=(A_pred, A_prey)`.  It cannot be recomputed from the stored observations: `FusedPolicy.act()` draws
the actions from the float32 logits of its bf16 matrix-core kernels, which differ from a float32 `PolicyNet` forward,
so a learner that recomputes them starts its first epoch with a ratio that is not 1.  `record_policy(logits)` stands between `act` and
`step` (`env.record_logp()`, `ppg_record_logp`, csrc/ppg_logp.h: two launches, float64 arithmetic rounded once, nothing read back):

    traj = AgentTrajectories(env, horizon=T, obs_rows=rows, logp=(A_pred, A_prey))
    bufs = (torch.zeros((B * env.pred_capacity, A_pred), device=dev), torch.zeros((B * env.prey_capacity, A_prey), device=dev))
    env.step(first_actions); traj.record(first_actions)
    for t in range(1, T):
        fused.act(env, sample=True, seed=seed + t, logits=bufs)     # actions into env.actions, logits into bufs
        traj.record_policy(bufs)                                    # logp / entropy / dist of the samples of the last record()
        env.step(env.actions); traj.record(env.actions)
    logp, entropy, dist = traj.behaviour(PREY)                      # [n], [n] or None, [n,A] or None: NaN where no policy was recorded
    values = traj.scatter(v_pred, v_prey)                           # a critic's per-sample values back into [len,B,S] for gae()

and the closed loop replays as one HIP graph: `GraphedCollector(env, traj, act=lambda: fused.act(env, sample=True, seed=seed_tensor,
logits=bufs), logits=bufs)`.  The samples of the last recorded step keep NaN until a further act + record_policy() covers them.

The column PPO optimises against -- the advantage, and the return or value target -- comes in the same slots, in one launch
(`env.backward_samples()`, `ppg_backward_samples`, csrc/ppg_backward.h): the critic's per-sample values are read through `store.slot`,
the recursion of `ppg_backward` runs in float64, and every stored sample's A and G are rounded once to float32 at its slot.  It gives
the bits of scatter() -> returns_and_gae() -> flat() -> .float() (kept verbatim as `targets_torch()`) without the three float64
[len,B,S] tensors that path allocates, writes and reads back to pick a fifth of their elements:

    v_pred, v_prey = critic(traj.samples(PREDATOR)[1]), critic(traj.samples(PREY)[1])   # float32 / float64 [n_s], one value per sample
    adv, ret, stats = traj.targets(v_pred, v_prey, 0.99, 0.95)      # adv[s], ret[s]: float32 [n_s] in the order of samples(s)
    count, mean, std = traj.advantage_moments(stats)                # float64 [2] each, no read-back
    adv_n = (adv[PREY] - mean[PREY]) / (std[PREY] + 1e-8)           # the usual value target: adv[PREY] + v_prey

The values themselves come from the store without a torch forward when the critic is a `FusedPolicy` of `PolicyNet(..., n_actions=1)`
networks: `v = traj.values(critic)` runs the policy kernels over `store.obs` (`FusedPolicy.evaluate()`, `ppg_policy_evaluate`: the row
count is read from `store.cursor` on the device) and `traj.targets(v[0][:n_pred], v[1][:n_prey], ...)` takes them;
`traj.logits(fused, s)` is the same for the actor's logits under its current weights.

and the minibatch step of the learner closes the loop: PPO's clipped loss (RLlib's `compute_loss_for_module`) and its gradients from those
columns and the learner's fresh logits and values, in two launches (`env.ppo_loss()`, `ppg_ppo_loss`, csrc/ppg_ppo.h), nothing read back:

    norm = traj.advantage_norm(stats)                               # float64 [2,2]: {mean, 1 / (std + eps)} per species
    index = torch.randperm(n_prey, device=dev).to(torch.int32)[:128]          # slots of a minibatch
    logits, values = prey_net(obs[index.long()])
    loss, st, grad_logits, grad_values = traj.ppo_loss(PREY, logits, values, index, adv[PREY], ret[PREY], adv_norm=norm)
    torch.autograd.backward([logits, values], [grad_logits, grad_values]); optimizer.step()

Samples whose action is still ACTION_UNSET or whose logp is still NaN are skipped, so an index over all slots is legal.
`ppo_loss_function()` is the same behind `loss.backward()`, `ppo_loss_torch()` the same loss as torch ops.

The network on either side of that loss runs on the device too: `NetLearner(env, net, max_rows)` is `net(obs[index.long()])` as one
launch and its backward as two (`env.net_forward()` / `env.net_backward()`, `ppg_net_forward` / `ppg_net_backward`, csrc/ppg_net.h:
float32, no atomics), attached to autograd, and `traj.forward(learner, PREY, index)` applies it to the store:

    actor, critic = NetLearner(env, prey_net, 128), NetLearner(env, prey_critic, 128)
    logits, values = traj.forward(actor, PREY, index), traj.forward(critic, PREY, index)[:, 0]
"""
from __future__ import annotations

import types

import torch

from . import _abi
from .batched import capture_graph, net_grad_views


class ObservationStore:
    """The tensors of `ppg_obs_store` (include/ppg.h) for one env: per species s (0 predators, 1 prey) `obs[s]` [rows[s],C,R,R],
    `sample[s]` int32 [rows[s]] -- the flat index (t * B + b) * S + r of the row in slot k -- and `action[s]` int8 [rows[s]] (None
    with actions=False); `slot` int32 [T,B,S], the slot of every row of every step or -1; `cursor` int64 [4] on the device: rows stored
    {pred, prey}, rows dropped {pred, prey}.  dtype: the env's observation dtype (default), or torch.float32 on a float64 env -- the
    rows are then rounded to float32 as they are stored.
    logp=(A_pred, A_prey): the store also keeps what the behaviour policy thought of every sample (`record_logp()`): `logp[s]` float32
    [rows[s]], `entropy[s]` likewise (entropy=True) and `dist[s]` float32 [rows[s], A_s], the logits (dist=True); `logp` and `entropy`
    hold NaN in every slot no policy was recorded for.  Without it the three are None."""

    def __init__(self, env, horizon, rows, dtype=None, actions=True, logp=None, entropy=True, dist=False):
        self.env, self.horizon = env, int(horizon)
        self.capacity = (int(rows[0]), int(rows[1]))
        if self.horizon < 1 or min(self.capacity) < 0:
            raise ValueError("horizon must be >= 1 and rows >= 0")
        dtype = env.obs_dtype if dtype is None else dtype
        if dtype != env.obs_dtype and not (dtype == torch.float32 and env.obs_dtype == torch.float64):
            raise ValueError(f"dtype must be the env's {env.obs_dtype} (or torch.float32 on a float64 env), not {dtype}")
        self.f32 = dtype != env.obs_dtype
        dev = env.device
        self.obs = [torch.zeros((n,) + tuple(src.shape[2:]), dtype=dtype, device=dev)
                    for n, src in zip(self.capacity, (env.obs_pred, env.obs_prey))]
        self.sample = [torch.zeros((n,), dtype=torch.int32, device=dev) for n in self.capacity]
        self.action = [torch.full((n,), _abi.ACTION_UNSET, dtype=torch.int8, device=dev) for n in self.capacity] if actions else None
        self.slot = torch.full((self.horizon, env.batch_size, env.S), -1, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros((4,), dtype=torch.int64, device=dev)
        self.n_actions = self.logp = self.entropy = self.dist = None
        if logp is not None:
            self.n_actions = (int(logp[0]), int(logp[1]))
            if not all(1 <= a <= 32 for a in self.n_actions):
                raise ValueError(f"logp = {self.n_actions}: the action counts must be in 1..32")
            self.logp = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in self.capacity]
            if entropy:
                self.entropy = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in self.capacity]
            if dist:
                self.dist = [torch.zeros((n, a), dtype=torch.float32, device=dev) for n, a in zip(self.capacity, self.n_actions)]

    def clear(self):
        """Start filling from slot 0 again (the tensors keep their bytes: everything below the cursor is rewritten as it moves; `logp`
        and `entropy`, which are written one call later and only where a policy acted, are refilled with NaN)."""
        self.cursor.zero_()
        for xs in (self.logp, self.entropy):
            if xs is not None:
                for x in xs:
                    x.fill_(float("nan"))
        return self

    def counts(self):
        """((stored, dropped) of the predators, (stored, dropped) of the prey): one read-back."""
        c = self.cursor.tolist()
        return (c[0], c[2]), (c[1], c[3])

    def record(self, t, actions=None, stream=None):
        """env.record_obs() into this store."""
        self.env.record_obs(self, t, actions if self.action is not None else None, f32=self.f32, stream=stream)
        return self

    def record_logp(self, t, logits, actions=None, stream=None):
        """env.record_logp() into this store: t is the step the env's current output was recorded as (or the device word, which names
        the next one), logits the pair `FusedPolicy.act(..., logits=...)` filled."""
        self.env.record_logp(self, t, logits, actions, stream=stream)
        return self

    def record_logp_torch(self, t, logits, actions=None):
        """record_logp(t, logits, actions) as torch ops: the same result (float64 arithmetic rounded once; `dist` the same bits),
        `nonzero`-based, so the host waits for the device at every call (timing baseline, fallback).  t: an int."""
        env, t = self.env, int(t)
        if self.logp is None:
            raise ValueError("the store keeps no log-probabilities: ObservationStore(..., logp=(A_pred, A_prey))")
        if not 0 <= t < self.horizon:
            raise ValueError(f"t = {t} is outside [0, {self.horizon})")
        actions, live = env.actions if actions is None else actions, env.live_mask()
        for s, (first, cap) in enumerate(((0, env.pred_capacity), (env.pred_capacity, env.prey_capacity))):
            if logits[s] is None:
                continue
            A = self.n_actions[s]
            b, j = live[:, first:first + cap].nonzero(as_tuple=True)   # env-major, rows ascending: the logits' order
            k = self.slot[t][b, first + j].long()
            ok = (k >= 0) & (k < self.capacity[s])
            row, k, a = logits[s][:b.numel()][ok], k[ok], actions[b, first + j][ok].long()
            d = row.double() - row.double().max(dim=1, keepdim=True).values
            masked = d == float("-inf")
            e = torch.where(masked, torch.zeros_like(d), d.exp())
            total = e.sum(dim=1)
            w = torch.where(masked, torch.zeros_like(d), e * d).sum(dim=1)
            ls = total.log()
            valid = (a >= 0) & (a < A)
            lp = d.gather(1, a.clamp(0, A - 1).unsqueeze(1)).squeeze(1) - ls
            self.logp[s][k] = torch.where(valid, lp, torch.full_like(lp, float("nan"))).float()
            if self.entropy is not None:
                self.entropy[s][k] = (ls - w / total).float()
            if self.dist is not None:
                self.dist[s][k] = row
        return self

    def record_obs_torch(self, t, actions=None):
        """record(t, actions) as torch ops: the same bytes, `nonzero`-based, so the host waits for the device at every call (timing
        baseline, fallback).  t: an int."""
        env, t = self.env, int(t)
        if not 0 <= t < self.horizon:
            raise ValueError(f"t = {t} is outside [0, {self.horizon})")
        B, S, dev = env.batch_size, env.S, env.device
        cursor = self.cursor.tolist()
        slot_t, live = torch.full((B, S), -1, dtype=torch.int32, device=dev), env.live_mask()
        for s, (first, cap, src) in enumerate(((0, env.pred_capacity, env.obs_pred), (env.pred_capacity, env.prey_capacity, env.obs_prey))):
            b, j = live[:, first:first + cap].nonzero(as_tuple=True)   # env-major, rows ascending
            k = cursor[s] + torch.arange(b.numel(), device=dev)
            keep = k < self.capacity[s]
            b, j, k = b[keep], j[keep], k[keep]
            self.obs[s][k] = src[b, j].to(self.obs[s].dtype)
            self.sample[s][k] = ((t * B + b) * S + first + j).to(torch.int32)
            if self.action is not None:
                self.action[s][k] = _abi.ACTION_UNSET
            slot_t[b, first + j] = k.to(torch.int32)
            if actions is not None and self.action is not None and t > 0:
                prev = self.slot[t - 1][:, first:first + cap]
                ok = (prev >= 0) & (prev < self.capacity[s])
                self.action[s][prev[ok].long()] = actions[:, first:first + cap][ok]
            end = cursor[s] + int(keep.numel())
            cursor[2 + s] += end - min(end, self.capacity[s])
            cursor[s] = min(end, self.capacity[s])
        self.slot[t].copy_(slot_t)
        self.cursor.copy_(torch.tensor(cursor, dtype=torch.int64))
        return self


class AgentTrajectories:
    def __init__(self, env, horizon, step_on_device=False, obs_rows=None, logp=None, entropy=True, dist=False):
        self.env = env
        self.horizon = int(horizon)
        if self.horizon < 1:
            raise ValueError("horizon must be >= 1")
        T, B, S, dev = self.horizon, env.batch_size, env.S, env.device
        self.reward = torch.zeros((T, B, S), dtype=torch.float64, device=dev)
        self.in_use = torch.zeros((T, B, S), dtype=torch.bool, device=dev)
        self.terminated = torch.zeros((T, B, S), dtype=torch.bool, device=dev)
        self.truncated = torch.zeros((T, B, S), dtype=torch.bool, device=dev)
        self.next_row = torch.full((T, B, S), -1, dtype=torch.int16, device=dev)
        # step_on_device: the step index lives in `t_dev` (int32 [1] on the device), read by the record kernel when it runs and
        # counted up behind it on the same stream -- no host value in the launch, so step + record can be captured and replayed
        # (GraphedCollector).  A record() past the horizon then writes nothing (and still links) instead of raising.
        self.step_on_device = bool(step_on_device)
        self.t_dev = torch.zeros((1,), dtype=torch.int32, device=dev) if self.step_on_device else None
        self._t = 0
        # obs_rows = (n_pred, n_prey): record() also appends the observation rows in use (and the actions it is given) to a compact
        # store of that many rows per species -- `store`, read through samples() and flat()
        # logp = (A_pred, A_prey): the store also keeps the behaviour policy's log-probabilities (record_policy(), behaviour())
        if logp is not None and obs_rows is None:
            raise ValueError("logp needs a store: AgentTrajectories(..., obs_rows=(n_pred, n_prey), logp=(A_pred, A_prey))")
        self.store = ObservationStore(env, self.horizon, obs_rows, logp=logp, entropy=entropy, dist=dist) if obs_rows is not None else None

    @property
    def t(self):
        """Steps recorded so far.  With step_on_device: one read-back of t_dev, clamped to [0, horizon]."""
        if self.step_on_device:
            return min(max(int(self.t_dev.item()), 0), self.horizon)
        return self._t

    @t.setter
    def t(self, value):
        if self.step_on_device:
            self.t_dev.fill_(int(value))
        else:
            self._t = int(value)

    def clear(self):
        """Start a new trajectory in the same tensors (the next record() is step 0 and links to nothing before it)."""
        if self.step_on_device:
            self.t_dev.zero_()
        else:
            self._t = 0
        if self.store is not None:
            self.store.clear()
        return self

    def __len__(self):
        return self.t

    def record(self, actions=None):
        """Store the output of the env's last call as step t.  Call it after every env.step of the trajectory, on the stream the
        step ran on (torch's current stream).  ONE launch: `env.record()` (`ppg_record`: the link kernel plus the stores;
        record_torch() is the same as torch ops).  With step_on_device the launch reads t_dev and an increment of it follows on the
        same stream; past the horizon such a call stores nothing.
        With a store (obs_rows) two more launches follow with the same step index: `env.record_obs()` appends the observation rows in
        use; actions: the int8 [B,S] tensor the step was given, stored as the actions of the previous record()'s samples (None: the
        actions stay ACTION_UNSET, e.g. device-drawn random actions)."""
        if not self.step_on_device and self._t >= self.horizon:
            raise RuntimeError(f"the trajectory is full ({self.horizon} steps): clear() it")
        t = self.t_dev if self.step_on_device else self._t
        self.env.record(self.reward, self.in_use, self.terminated, self.truncated, self.next_row, t)
        if self.store is not None:
            self.store.record(t, actions)
        if self.step_on_device:
            self.t_dev.add_(1)
        else:
            self._t += 1
        return self

    def _need_store(self, what, logp=False):
        """RuntimeError unless the trajectory has a store (logp: one that keeps log-probabilities): what `what` refuses without it."""
        if self.store is None or (logp and self.store.logp is None):
            hint = "AgentTrajectories(..., obs_rows=(n_pred, n_prey), logp=(A_pred, A_prey))" if logp else \
                "a store: AgentTrajectories(..., obs_rows=(n_pred, n_prey))"
            raise RuntimeError(f"{what}() needs {hint}")

    def record_policy(self, logits, actions=None):
        """Store what the behaviour policy thought of the samples of the LAST record(): call it between `fused.act(env, ...,
        logits=logits)` and the `env.step()` that uses those actions.  logits: the pair act() filled (either may be None); actions:
        the tensor it wrote (default `env.actions`).  Two launches (`env.record_logp()`), nothing read back.  The step is t - 1 on the
        host, or `t_dev` with step_on_device -- the kernels subtract the one themselves; before the first record() and past the
        horizon nothing is written."""
        self._need_store("record_policy", logp=True)
        if self.step_on_device:
            self.store.record_logp(self.t_dev, logits, actions)
        elif self._t > 0:
            self.store.record_logp(self._t - 1, logits, actions)
        return self

    def behaviour(self, species):
        """(logp[:n], entropy[:n] or None, dist[:n] or None) of one species, in the order of samples(): float32 [n], [n] and
        [n, A_s] (one read-back of the cursor).  NaN in logp / entropy where no policy was recorded for a sample."""
        self._need_store("behaviour", logp=True)
        st = self.store
        n = int(st.cursor[species].item())
        return (st.logp[species][:n], None if st.entropy is None else st.entropy[species][:n],
                None if st.dist is None else st.dist[species][:n])

    def logits(self, fused, species, out=None):
        """The outputs of `fused`'s network of one species (0 predators, 1 prey) over the stored samples, under its CURRENT weights:
        float32 [capacity_s, A_s] with row k = the network's logits for the observation in slot k -- bit for bit what `act()` would
        write for that row (`FusedPolicy.evaluate()`, `ppg_policy_evaluate`: the matrix-core kernels over `store.obs[species]`).
        After `fused.update()` this is the learner's view of every sample without a torch forward: KL against `behaviour()`'s dist,
        early stopping, offline greedy evaluation.  The count is `store.cursor[species]`, read by the kernel on the device: nothing is
        read back; rows at and behind it keep what they held (zeros in a tensor the call allocates).  Stream-ordered like an act."""
        self._need_store("logits")
        st = self.store
        return fused.evaluate(species, st.obs[species], count=st.cursor[species:species + 1], out=out)

    def values(self, critic):
        """(v_pred, v_prey): a critic's value of every stored sample, float32 [capacity_s] per species (None for a species the critic
        has no network for), v[s][k] = the value of the observation in slot k.  critic: a `FusedPolicy` of `PolicyNet(...,
        n_actions=1)` networks (`load_rllib_state_dict(..., head="vf")`), whose one output is the value -- evaluated by the policy
        kernels over the store (`logits()`), no float32 torch forward over millions of rows, nothing read back.  What targets() takes:

            v = traj.values(critic)
            adv, ret, stats = traj.targets(v[0][:n_pred], v[1][:n_prey], 0.99, 0.95)      # n_s = traj.samples(s)[0]"""
        self._need_store("values")
        out = []
        for s, net in enumerate(critic.nets):
            if net is None:
                out.append(None)
                continue
            if net.n_actions != 1:
                raise ValueError(f"a critic is a network with n_actions = 1 (its output is the value); species {s} has {net.n_actions}")
            out.append(self.logits(critic, s).squeeze(-1))
        return tuple(out)

    def scatter(self, x_pred, x_prey, fill=0.0):
        """The inverse of flat(): a [len,B,S] tensor with x_s[k] at the (t, b, r) of sample k of species s and `fill` everywhere else --
        what brings a critic's per-sample values into the layout gae() takes.  x_pred / x_prey: [n_s] tensors of one dtype in sample
        order (either may be None).  Plain torch index ops, one read-back of the cursor."""
        self._need_store("scatter")
        given = [x for x in (x_pred, x_prey) if x is not None]
        if not given:
            raise ValueError("scatter() needs at least one of x_pred, x_prey")
        n_steps, cursor = self.t, self.store.cursor.tolist()
        B, S = self.reward.shape[1:]
        out = torch.full((n_steps, B, S), fill, dtype=given[0].dtype, device=self.reward.device)
        flat = out.reshape(-1)
        for s, x in enumerate((x_pred, x_prey)):
            if x is None:
                continue
            n = cursor[s]
            if tuple(x.shape) != (n,) or x.dtype != out.dtype:
                raise ValueError(f"x of species {s} must be a {out.dtype} tensor [{n}] (the samples stored), not {x.dtype} {list(x.shape)}")
            flat[self.store.sample[s][:n].long()] = x.to(out.device)
        return out

    def record_obs_torch(self, actions=None):
        """record(actions) of a trajectory with a store as torch ops: record_torch() plus ObservationStore.record_obs_torch() -- the
        same bytes; the host waits for the device (timing baseline, fallback)."""
        self._need_store("record_obs_torch")
        t = self.t
        self.record_torch()
        self.store.record_obs_torch(t, actions)
        return self

    def samples(self, species):
        """(n, obs[:n], index[:n], action[:n]) of one species (0 predators, 1 prey): the rows stored so far (one read-back), their
        observations [n,C,R,R], the flat index (t * B + b) * S + r of each as int64 -- `x.reshape(-1)[index]` picks a sample's element
        of any [len,B,S] tensor, which is what flat() does -- and the actions taken from them (None for a store without actions).
        Samples are ordered by step, then env, then row."""
        self._need_store("samples")
        st = self.store
        n = int(st.cursor[species].item())
        return n, st.obs[species][:n], st.sample[species][:n].long(), None if st.action is None else st.action[species][:n]

    def flat(self, x, species):
        """The elements of a [len,B,S] tensor (returns, advantages, values ...) that belong to the stored samples of a species, in
        sample order: x.reshape(-1)[index[:n]]."""
        return x.reshape(-1)[self.samples(species)[2]]

    def record_torch(self):
        """record() as torch ops behind `env.link()`: the same bytes, about nineteen small launches (timing baseline, fallback)."""
        if self.step_on_device:
            raise RuntimeError("record_torch() needs the step index on the host: AgentTrajectories(..., step_on_device=False)")
        if self.t >= self.horizon:
            raise RuntimeError(f"the trajectory is full ({self.horizon} steps): clear() it")
        env, t = self.env, self.t
        _, next_row = env.link()
        if t > 0:
            self.next_row[t - 1].copy_(next_row)
        self.next_row[t].fill_(-1)
        used = env.live_mask()
        self.in_use[t].copy_(used)
        self.reward[t].copy_(env.row_reward)
        self.terminated[t].copy_(((env.row_flags & _abi.ROW_DIED) != 0) & used)
        self.truncated[t].copy_(((env.row_flags & _abi.ROW_TRUNC) != 0) & used)
        self.t = t + 1
        return self

    def _successor(self, t, x_next):
        """x of step t + 1 brought into the rows of step t; 0 where the agent of a row has no successor."""
        nxt = self.next_row[t]
        has = (nxt >= 0) & self.in_use[t] & ~self.terminated[t] & ~self.truncated[t]
        moved = torch.gather(x_next, 1, nxt.clamp_min(0).long())
        return torch.where(has, moved, torch.zeros_like(moved))

    def _backward(self, values, gamma, lam, returns):
        """The first len(self) steps of the stored tensors (a contiguous prefix) through env.backward()."""
        n = self.t   # (step_on_device: the one read-back)
        B, S = self.reward.shape[1:]
        if values is not None:
            if tuple(values.shape) != (n, B, S):
                raise ValueError(f"values must be [{n},{B},{S}]")
            if values.dtype not in (torch.float64, torch.float32):
                values = values.to(torch.float32)   # (exact for bfloat16 / float16)
            values = values.to(self.reward.device).contiguous()
        if n == 0:
            empty = torch.zeros((0, B, S), dtype=torch.float64, device=self.reward.device)
            return (empty if returns else None), (empty.clone() if values is not None else None)
        return self.env.backward(self.reward[:n], self.next_row[:n], self.in_use[:n], self.terminated[:n], self.truncated[:n],
                                 gamma, lam, values=values, returns=returns)

    def returns(self, gamma):
        """Discounted return of every agent from every step on: float64 [len,B,S], 0 in rows not in use."""
        return self._backward(None, gamma, 1.0, True)[0]

    def gae(self, values, gamma, lam):
        """Generalised advantage estimate: delta[t] = reward[t] + gamma * V[t + 1][next_row[t]] - V[t],
        A[t] = delta[t] + gamma * lam * A[t + 1][next_row[t]], successor terms zero where there is no successor.
        values: [len,B,S] (float64 / float32 as they are, any other float dtype through float32; row r of values[t] = the agent in
        row r of call t).  Returns float64 [len,B,S]."""
        return self._backward(values, gamma, lam, False)[1]

    def returns_and_gae(self, values, gamma, lam):
        """(returns(gamma), gae(values, gamma, lam)) in ONE launch."""
        return self._backward(values, gamma, lam, True)

    def returns_torch(self, gamma):
        """returns() as a torch loop over the steps: the same bits, about five launches per step (timing baseline, fallback)."""
        n = self.t
        G = torch.zeros((n,) + tuple(self.reward.shape[1:]), dtype=torch.float64, device=self.reward.device)
        g_next = torch.zeros_like(G[0]) if n else None
        zero = torch.zeros_like(G[0]) if n else None
        for t in range(n - 1, -1, -1):
            succ = self._successor(t, g_next) if t + 1 < n else zero
            g = self.reward[t] + succ * float(gamma)   # (two roundings, mul then add: what float64 Python arithmetic does)
            g_next = torch.where(self.in_use[t], g, zero)
            G[t] = g_next
        return G

    def gae_torch(self, values, gamma, lam):
        """gae() as a torch loop over the steps: the same bits (timing baseline, fallback).  values: any float dtype."""
        n = self.t
        if tuple(values.shape) != (n,) + tuple(self.reward.shape[1:]):
            raise ValueError(f"values must be [{n},{self.reward.shape[1]},{self.reward.shape[2]}]")
        V = values.to(device=self.reward.device, dtype=torch.float64)
        A = torch.zeros_like(V)
        zero = torch.zeros_like(V[0]) if n else None
        a_next = zero
        gl = float(gamma) * float(lam)
        for t in range(n - 1, -1, -1):
            v_succ = self._successor(t, V[t + 1]) if t + 1 < n else zero
            a_succ = self._successor(t, a_next) if t + 1 < n else zero
            delta = (self.reward[t] + v_succ * float(gamma)) - V[t]
            a = delta + a_succ * gl
            a_next = torch.where(self.in_use[t], a, zero)
            A[t] = a_next
        return A

    @staticmethod
    def _sample_values(v, n, s):
        """A species' per-sample values as targets() / targets_torch() take them: [n], float64 / float32 as they are, any other float
        dtype through float32 (exact for bfloat16 / float16)."""
        if v is None:
            return None
        if tuple(v.shape) != (n,) or not v.dtype.is_floating_point:
            raise ValueError(f"the values of species {s} must be a float tensor [{n}] (the samples stored), not {v.dtype} {list(v.shape)}")
        return v if v.dtype in (torch.float64, torch.float32) else v.to(torch.float32)

    def targets(self, v_pred, v_prey, gamma, lam, returns=True, stats=True):
        """(adv, ret, stats): the advantage and the discounted return of every stored sample, in the order of samples() -- `adv[s]`,
        `ret[s]` float32 [n_s] per species s (ret is None with returns=False) -- from the critic's per-sample values v_pred / v_prey
        ([n_s] each, one dtype; None: V = 0 for that species), over the first len(self) steps.  ONE launch (`env.backward_samples()`,
        `ppg_backward_samples`): the values are read through `store.slot`, the recursion runs in float64 -- rows the store dropped
        take part with V = 0 -- and A and G are rounded once to float32 at the sample's slot: the bits of targets_torch(), without a
        [len,B,S] tensor of values, returns or advantages.  stats (None with stats=False): float64 [B,2,3], per env and species
        {count, sum A, sum A * A} of the unrounded advantages, for advantage_moments().  One read-back: the store's cursor (with
        step_on_device the step index comes with it).  An empty trajectory gives empty tensors without a launch."""
        self._need_store("targets")
        st, dev = self.store, self.reward.device
        if self.step_on_device:
            n_pred, n_prey, n = torch.cat((st.cursor[:2], self.t_dev.to(torch.int64))).tolist()   # (the one read-back)
            n = min(max(n, 0), self.horizon)
        else:
            (n_pred, n_prey), n = st.cursor[:2].tolist(), self._t
        values = [self._sample_values(v, count, s) for s, (v, count) in enumerate(((v_pred, n_pred), (v_prey, n_prey)))]
        if values[0] is not None and values[1] is not None and values[0].dtype != values[1].dtype:
            raise ValueError(f"v_pred and v_prey must have one dtype, not {values[0].dtype} and {values[1].dtype}")
        values = [None if v is None else v.to(dev).contiguous() for v in values]
        B = self.reward.shape[1]
        if n == 0:
            empty = lambda: [torch.zeros((0,), dtype=torch.float32, device=dev) for _ in range(2)]
            return empty(), (empty() if returns else None), (torch.zeros((B, 2, 3), dtype=torch.float64, device=dev) if stats else None)
        # (the samples stored so far are the store as far as this call goes: a slot word is compared with n_s, and the outputs are [n_s])
        view = types.SimpleNamespace(horizon=st.horizon, capacity=(n_pred, n_prey), slot=st.slot)
        return self.env.backward_samples(view, self.reward[:n], self.next_row[:n], self.in_use[:n], self.terminated[:n],
                                         self.truncated[:n], gamma, lam, values=values, returns=returns, stats=stats)

    def targets_torch(self, v_pred, v_prey, gamma, lam, returns=True, stats=True):
        """targets() as the composition it replaces -- scatter() into [len,B,S], returns_and_gae(), flat() per species, .float(): the
        same bits in adv and ret (timing baseline, fallback).  stats are index_add sums here: the same counts, the sums equal to
        targets()'s up to the order of the additions."""
        self._need_store("targets_torch")
        n_steps, cursor = self.t, self.store.cursor.tolist()
        B, S = self.reward.shape[1:]
        v_pred, v_prey = (self._sample_values(v, cursor[s], s) for s, v in enumerate((v_pred, v_prey)))
        if v_pred is None and v_prey is None:
            values = torch.zeros((n_steps, B, S), dtype=torch.float64, device=self.reward.device)
        else:
            values = self.scatter(v_pred, v_prey)
        G, A = self.returns_and_gae(values, gamma, lam)
        index = [self.samples(s)[2] for s in (0, 1)]
        a64 = [A.reshape(-1)[i] for i in index]
        adv = [a.float() for a in a64]
        ret = [G.reshape(-1)[i].float() for i in index] if returns else None
        moments = None
        if stats:
            moments = torch.zeros((B, 2, 3), dtype=torch.float64, device=self.reward.device)
            for s, (i, a) in enumerate(zip(index, a64)):
                b = (i // S) % B
                for c, x in enumerate((torch.ones_like(a), a, a * a)):
                    moments[:, s, c].index_add_(0, b, x)
        return adv, ret, moments

    @staticmethod
    def advantage_moments(stats):
        """(count, mean, std) of the advantages per species -- float64 [2] device tensors, nothing read back -- from the `stats` of
        targets(): the [B,2,3] sums are added over the envs (`stats.sum(0)`), mean = sum / n, std = sqrt(max(sq / n - mean^2, 0)) (the
        population variance, clamped at 0 against its own rounding).  A species without a stored sample (n = 0) gets mean 0 and std
        0: its sums are 0 and they are divided by 1, so no NaN reaches a learner that normalises an empty tensor."""
        total = stats.sum(0)
        count = total[:, 0]
        n = count.clamp_min(1.0)
        mean = total[:, 1] / n
        var = (total[:, 2] / n - mean * mean).clamp_min(0.0)
        return count, mean, var.sqrt()

    @staticmethod
    def advantage_norm(stats, eps=1e-8):
        """float64 [2,2] on the device, per species {mean, 1 / (std + eps)} from the `stats` of targets() (advantage_moments(), nothing
        read back): row s is the `adv_norm` of ppo_loss(s, ...), which then uses (A - mean) / (std + eps) as the advantage."""
        _, mean, std = AgentTrajectories.advantage_moments(stats)
        return torch.stack((mean, 1.0 / (std + eps)), dim=1).contiguous()

    _PPO_STATS = ("n", "policy_loss", "vf_loss", "vf_loss_unclipped", "entropy", "kl", "clip_fraction", "approx_kl")

    def _ppo_columns(self, species, advantage, value_target, values, index, adv_norm, kl_coeff):
        """What ppo_loss() and ppo_loss_torch() take from the store for n = len(advantage) samples: (action[:n], logp[:n], dist[:n] or
        None, the species' adv_norm [2] or None); ValueError for what both refuse."""
        self._need_store("ppo_loss", logp=True)
        st = self.store
        if st.action is None:
            raise RuntimeError("ppo_loss() needs a store that keeps actions")
        if index is not None and (not isinstance(index, torch.Tensor) or index.dtype != torch.int32):
            raise ValueError(f"index must have dtype=torch.int32 (the slot numbers of the store), not {getattr(index, 'dtype', type(index))}")
        if advantage.dim() != 1 or advantage.shape[0] > st.capacity[species]:
            raise ValueError(f"advantage must be [n] with n <= the store's {st.capacity[species]} rows, not {tuple(advantage.shape)}")
        if (values is None) != (value_target is None):
            raise ValueError("values and value_target come together: both tensors, or both None")
        if kl_coeff != 0 and st.dist is None:
            raise ValueError("kl_coeff != 0 needs the behaviour policy's logits: AgentTrajectories(..., dist=True)")
        if adv_norm is not None:
            if tuple(adv_norm.shape) == (2, 2):
                adv_norm = adv_norm[species]
            if tuple(adv_norm.shape) != (2,) or adv_norm.dtype != torch.float64:
                raise ValueError(f"adv_norm must be a float64 tensor [2] or [2,2] (advantage_norm()), not {adv_norm.dtype} {list(adv_norm.shape)}")
        n = advantage.shape[0]
        return st.action[species][:n], st.logp[species][:n], None if st.dist is None else st.dist[species][:n], adv_norm

    def forward(self, learner, species, index=None):
        """`learner(store.obs[species], index)`: a `NetLearner`'s output for the samples in slots `index` (int32 [M]; None: every row of
        the store's tensor), float32 [M,n_out] attached to its network's parameters -- the logits of an actor; a critic's values are
        column 0."""
        self._need_store("forward")
        return learner(self.store.obs[species], index)

    def ppo_loss(self, species, logits, values, index, advantage, value_target, *, clip=0.3, vf_clip=10.0, vf_coeff=1.0, ent_coeff=0.0,
                 kl_coeff=0.2, adv_norm=None):
        """(loss, stats, grad_logits, grad_values): PPO's clipped loss of one minibatch of one species -- the mean over the valid
        samples of -min(A r, A clamp(r, 1 - clip, 1 + clip)) + vf_coeff min((v - target)^2, vf_clip) - ent_coeff H + kl_coeff
        KL(old || new), RLlib's `PPOTorchLearner.compute_loss_for_module` -- and its gradients, in two launches (`env.ppo_loss()`,
        `ppg_ppo_loss`, csrc/ppg_ppo.h: float64 arithmetic rounded once at the stores), nothing read back.
        logits float32 [M,A] and values float32 [M] (or None: no value term): the learner's outputs for the samples in slots `index`,
        int32 [M] (None: slots 0 .. M - 1); advantage, value_target: float32 [n] in sample order (targets(); value_target None exactly
        when values is); adv_norm: advantage_norm(stats) or its row.  `action`, `logp` and `dist` come from the store; a sample whose
        slot is outside [0, n), whose action is still ACTION_UNSET or whose logp is still NaN (the last step's, until a further
        record_policy()) is skipped: not counted, gradient +0.0.
        stats: 0-dim float64 device tensors n, policy_loss, vf_loss, vf_loss_unclipped, entropy, kl, clip_fraction, approx_kl (means
        over the valid samples; with n = 0 all 0), and loss = policy_loss + vf_coeff vf_loss - ent_coeff entropy + kl_coeff kl, composed
        from `partial.sum(0)` with torch ops.  grad_logits [M,A] / grad_values [M] ARE d loss / d logits and d loss / d values, so the
        backward pass that costs nothing more is
            torch.autograd.backward([logits, values], [grad_logits, grad_values])
        in front of optimizer.step(); `ppo_loss_function()` wraps the same call for `loss.backward()`."""
        action, logp, dist, adv_norm = self._ppo_columns(species, advantage, value_target, values, index, adv_norm, kl_coeff)
        grad_logits, grad_values, partial = self.env.ppo_loss(
            logits.detach(), action, logp, advantage, index=index, values=None if values is None else values.detach(),
            value_target=value_target, dist=dist, adv_norm=adv_norm, clip=clip, vf_clip=vf_clip, vf_coeff=vf_coeff, ent_coeff=ent_coeff,
            kl_coeff=kl_coeff)
        total = partial.sum(0)
        n = total[0]
        mean = total[1:] / n.clamp_min(1.0)
        stats = dict(zip(self._PPO_STATS, (n, -mean[0], *mean[1:].unbind(0))))
        return _ppo_compose(stats, vf_coeff, ent_coeff, kl_coeff, values is not None), stats, grad_logits, grad_values

    def ppo_loss_torch(self, species, logits, values, index, advantage, value_target, *, clip=0.3, vf_clip=10.0, vf_coeff=1.0,
                       ent_coeff=0.0, kl_coeff=0.2, adv_norm=None, dtype=torch.float32):
        """(loss, stats) of ppo_loss() as plain differentiable torch ops in `dtype` -- RLlib's formulas spelled out: log_softmax, the
        gather at the action, exp, clamp, min, the entropy and the KL of two categoricals, the clipped squared error, and a mean over
        the valid samples (the others are selected away in front of every op, so that they neither count nor put a NaN into a
        gradient) -- some forty small launches and a dozen [M,A] temporaries, and as many again for `loss.backward()` (timing
        baseline, cross-check, fallback)."""
        action, logp, dist, adv_norm = self._ppo_columns(species, advantage, value_target, values, index, adv_norm, kl_coeff)
        M, A = logits.shape
        n = advantage.shape[0]
        k = torch.arange(M, device=logits.device) if index is None else index.long()
        inside = (k >= 0) & (k < n)
        k = torch.where(inside, k, torch.zeros_like(k))
        if n == 0:
            act, lp_old = torch.full((M,), -1, device=logits.device), torch.full((M,), float("nan"), dtype=dtype, device=logits.device)
        else:
            act, lp_old = action[k].long(), logp[k].to(dtype)
        valid = inside & (act >= 0) & (act < A) & torch.isfinite(lp_old)
        pick = lambda x, fill=0.0: torch.where(valid, x, torch.full_like(x, fill))
        count = valid.sum().to(dtype)
        denom = count.clamp_min(1.0)
        masked_mean = lambda x: pick(x).sum() / denom

        def log_probs(raw):
            raw = torch.where(valid[:, None], raw.to(dtype), torch.zeros((), dtype=dtype, device=raw.device))
            lp = torch.log_softmax(raw, dim=1)
            finite = lp > float("-inf")
            return lp, torch.where(finite, lp, torch.zeros_like(lp)), lp.exp()
        lp, lp_safe, p = log_probs(logits)
        act = pick(act, 0)
        lp_a = lp.gather(1, act[:, None])[:, 0]
        adv = advantage.to(dtype)[k] if n else torch.zeros((M,), dtype=dtype, device=logits.device)
        if adv_norm is not None:
            adv = (adv - adv_norm[0].to(dtype)) * adv_norm[1].to(dtype)
        adv, lp_old = pick(adv), pick(lp_old)
        ratio = (lp_a - lp_old).exp()
        s1, s2 = adv * ratio, adv * ratio.clamp(1.0 - clip, 1.0 + clip)
        surrogate = torch.min(s1, s2)
        entropy = -(p * lp_safe).sum(1)
        zero = torch.zeros((), dtype=dtype, device=logits.device)
        kl = vf = vfc = None
        if dist is not None and n:
            lq, lq_safe, q = log_probs(dist[k])
            kl = torch.where(q > 0, q * (lq_safe - lp), torch.zeros_like(q)).sum(1)
        if values is not None:
            target = value_target.to(dtype)[k] if n else torch.zeros((M,), dtype=dtype, device=logits.device)
            vf = (pick(values.to(dtype)) - pick(target)) ** 2
            vfc = vf.clamp(0.0, vf_clip)
        stats = {"n": count, "policy_loss": -masked_mean(surrogate), "vf_loss": zero if vfc is None else masked_mean(vfc),
                 "vf_loss_unclipped": zero if vf is None else masked_mean(vf), "entropy": masked_mean(entropy),
                 "kl": zero if kl is None else masked_mean(kl), "clip_fraction": masked_mean((s2 < s1).to(dtype)),
                 "approx_kl": masked_mean(lp_old - lp_a)}
        return _ppo_compose(stats, vf_coeff, ent_coeff, kl_coeff, values is not None), stats


def _ppo_compose(stats, vf_coeff, ent_coeff, kl_coeff, has_values):
    """The loss scalar from the means: a term whose coefficient is 0 is left out, not multiplied by 0 (an infinite KL that is not
    optimised against does not make the loss NaN)."""
    loss = stats["policy_loss"]
    if has_values and vf_coeff != 0:
        loss = loss + vf_coeff * stats["vf_loss"]
    if ent_coeff != 0:
        loss = loss - ent_coeff * stats["entropy"]
    if kl_coeff != 0:
        loss = loss + kl_coeff * stats["kl"]
    return loss


class _PpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, traj, species, index, advantage, value_target, kw):
        loss, stats, grad_logits, grad_values = traj.ppo_loss(species, logits, values, index, advantage, value_target, **kw)
        ctx.save_for_backward(grad_logits, *(() if grad_values is None else (grad_values,)))
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        saved = ctx.saved_tensors
        scale = grad_output.to(torch.float32)
        return (saved[0] * scale, saved[1] * scale if len(saved) > 1 else None) + (None,) * 6


def ppo_loss_function(traj, species, logits, values, index, advantage, value_target, **kw):
    """`traj.ppo_loss(...)` as a `torch.autograd.Function`: returns (loss, stats) with `loss` attached to `logits` and `values`, so that
    `loss.backward()` (or a sum of both species' losses) works as with ppo_loss_torch().  The gradients were computed by the forward
    call; backward multiplies the stored grad_logits / grad_values by `grad_output`, ONE elementwise op per tensor -- what
    `torch.autograd.backward([logits, values], [grad_logits, grad_values])` on ppo_loss()'s own outputs saves.  Keyword arguments: those
    of ppo_loss()."""
    out = {}
    loss = _PpoLoss.apply(logits, values, _StatsSink(traj, out), species, index, advantage, value_target, kw)
    return loss, out["stats"]


class _StatsSink:
    """Hands ppo_loss()'s stats out of the autograd Function's forward (which can only return tensors that take part in the graph)."""

    def __init__(self, traj, out):
        self.traj, self.out = traj, out

    def ppo_loss(self, *args, **kw):
        result = self.traj.ppo_loss(*args, **kw)
        self.out["stats"] = result[1]
        return result


class _NetForward(torch.autograd.Function):
    """NetLearner's two calls as one node of the autograd graph of the network's parameters."""

    @staticmethod
    def forward(ctx, learner, obs, index, *params):
        out = learner._forward(obs, index, pending=True)
        ctx.learner, ctx.token, ctx.obs, ctx.index = learner, learner._pending, obs, index
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return (None, None, None, *ctx.learner._backward(ctx.token, ctx.obs, ctx.index, grad_out))


class NetLearner:
    """A `policy.PolicyNet`'s minibatch forward and backward on the device in three launches (`env.net_forward()` / `env.net_backward()`,
    `ppg_net_forward` / `ppg_net_backward`, csrc/ppg_net.h: float32, no atomics), in place of `net(obs[index.long()])` and its autograd
    graph of a dozen modules -- the parameters are read where the optimiser keeps them, so an `optimizer.step()` needs no hand-over.

        learner = NetLearner(env, actor, max_rows=4096)
        logits = learner(traj.store.obs[s], index)          # float32 [M,A], attached to actor's parameters
        loss, stats = ppo_loss_function(traj, s, logits, values, index, adv, ret); loss.backward(); optimizer.step()

    net: its parameters float32 and contiguous on the env's device.  The learner owns the activation workspace and the partial sums
    for up to max_rows rows, and `grads`, a flat float32 buffer of every parameter's gradient (conv0.weight, conv0.bias, ...,
    fc0.weight, fc0.bias, ...) with the per-parameter views `grad_views`; the backward pass hands those views to autograd, which adds
    them into `p.grad` (`torch.autograd.backward([logits], [grad_logits])` and `loss.backward()` alike).  A critic is a net with
    n_actions = 1: its values are `learner(obs, index)[:, 0]`.
    One forward's activations live in the workspace until its backward has run: a second forward in between raises RuntimeError
    (`release()` gives up a forward whose backward will never come); so does a backward after a parameter was changed in place, as
    autograd's own saved tensors would.  With autograd disabled (`torch.no_grad()`) a call only
    evaluates and holds nothing.  groups: 0, or the number of workgroups of both calls."""

    def __init__(self, env, net, max_rows, groups=0):
        self.env, self.net, self.max_rows, self.groups = env, net, int(max_rows), int(groups)
        need = env.net_bytes(net, self.max_rows, self.groups)
        self.tile_rows = need[3]
        dev = env.device
        self.workspace = torch.empty((need[0] // 4,), dtype=torch.float32, device=dev)
        self.partial = torch.empty((need[1] // 4,), dtype=torch.float32, device=dev)
        self.grads = torch.zeros((need[2],), dtype=torch.float32, device=dev)
        views = net_grad_views(net, self.grads)
        self._params = [p for p, _ in views]
        self.grad_views = [v for _, v in views]   # (kept: autograd copies a gradient somebody else still holds instead of adopting it)
        self._pending = None
        self._calls = 0

    def _rows(self, obs, index):
        M = int(index.shape[0] if index is not None else obs.shape[0])
        if M > self.max_rows:
            raise ValueError(f"{M} rows, but the learner was built for max_rows = {self.max_rows}")
        return M

    def _forward(self, obs, index, pending):
        if self._pending is not None:
            raise RuntimeError("NetLearner: a second forward before the backward of the first would overwrite its activations "
                               "(run the backward pass, or release() the pending forward)")
        out, _ = self.env.net_forward(self.net, obs, index, M=self._rows(obs, index), groups=self.groups, workspace=self.workspace)
        if pending:
            self._calls += 1
            self._pending = self._calls
            self._versions = [p._version for p in self._params]
        return out

    def _backward(self, token, obs, index, grad_out):
        if token != self._pending:
            raise RuntimeError("NetLearner: the activations of this forward are gone (a backward ran already, or release())")
        if [p._version for p in self._params] != self._versions:   # (the kernels read the parameters when they run, as autograd's saved tensors)
            raise RuntimeError("NetLearner: a parameter was changed in place between the forward and its backward; the stored "
                               "activations belong to the old weights (run the backward before optimizer.step(), or release())")
        self.env.net_backward(self.net, obs, index, grad_out.contiguous(), self.workspace, M=self._rows(obs, index), groups=self.groups,
                              grads=self.grads, partial=self.partial)
        self._pending = None
        return self.grad_views

    def release(self):
        """Forget a forward whose backward will not run."""
        self._pending = None

    def __call__(self, obs, index=None):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._params):
            return _NetForward.apply(self, obs, index, *self._params)
        return self._forward(obs, index, pending=False)


class GraphedCollector:
    """One recorded step -- actions, `ppg_step`, `ppg_record` and the increment of the step index -- captured ONCE into a HIP graph
    and replayed: the capture protocol of policy.GraphedPolicyStep for a rollout that is recorded.  No host work per step.

        traj = AgentTrajectories(env, horizon=T, step_on_device=True)
        loop = GraphedCollector(env, traj)          # records step 0 (the uncaptured warm pass), then captures
        loop.replay(T - 1)                          # steps 1 .. T-1
        G = traj.returns(0.99)

    act: a callable that enqueues whatever fills `env.actions` on the current stream -- e.g. ``fused.act(env, sample=True,
    seed=seed_tensor)`` plus the increment of the seed tensor; without it the step draws uniform random actions on the device.
    The body (act, step, record) runs once uncaptured on a side stream -- that pass IS a recorded step, step 0 of an empty `traj`; it
    also creates the env's link tensors and leaves the link snapshot valid -- and is then captured as one linear chain on one stream.
    Replays past the horizon keep stepping and linking and store nothing (`ppg_record`: a step index outside [0, T) writes no
    buffer); `len(traj)` stays at T.

    Limit: whether the link snapshot may be linked to (the library's host flag, cleared by reset / set_placement / import_state) is
    baked into the graph when it is captured -- as "valid".  After `env.reset()`, `env.set_placement()` or `env.import_state()` run

        traj.clear(); env.step(...); traj.record()      # eager: this record links nothing and takes the fresh snapshot

    before the next replay(); a replay right after a reset would link the new rows to the old episode's snapshot.

    logits: the (logits_pred, logits_prey) buffers `act` fills, for a trajectory with `logp=`: the body becomes act,
    `traj.record_policy(logits, env.actions)`, step, record -- the closed loop of a PPO collector, still one linear chain:

        bufs = (torch.zeros((B * env.pred_capacity, A), device=dev), torch.zeros((B * env.prey_capacity, A), device=dev))
        traj = AgentTrajectories(env, T, step_on_device=True, obs_rows=rows, logp=(A, A))

        def act():
            fused.act(env, sample=True, seed=seed_tensor, logits=bufs)
            seed_tensor.add_(1)
        loop = GraphedCollector(env, traj, act=act, logits=bufs)
        loop.replay(T - 1)
        logp, entropy, dist = traj.behaviour(PREY)

    The warm pass acts on an output no record() has stored, so its record_policy() writes nothing; replay i stores the policy of
    step i - 1, and the samples of the last recorded step keep NaN.
    After `fused.update(...)` the next replay acts with the new weights: they land where the captured kernels read them."""

    def __init__(self, env, traj, act=None, auto_reset=True, logits=None):
        if not getattr(traj, "step_on_device", False):
            raise ValueError("GraphedCollector needs AgentTrajectories(..., step_on_device=True)")
        if traj.env is not env:
            raise ValueError("traj records another env")
        if env.device.type != "cuda":
            raise RuntimeError("GraphedCollector captures a HIP graph: the env must be on a GPU")
        if logits is not None and act is None:
            raise ValueError("logits are what `act` fills: GraphedCollector(env, traj, act=..., logits=...)")
        self.env, self.traj = env, traj

        def body():
            if act is not None:
                act()
                if logits is not None:   # (the samples of the previous record(); in the warm pass of an empty trajectory: nothing)
                    traj.record_policy(logits, env.actions)
                env.step(env.actions, auto_reset=auto_reset)
                traj.record(env.actions)   # (a trajectory with a store keeps them as the actions of the previous step's samples)
            else:
                env.step(random_actions=True, auto_reset=auto_reset)
                traj.record()
        self.graph = capture_graph(env.device, body)

    def replay(self, n: int = 1):
        for _ in range(n):
            self.graph.replay()
        return self
