"""Times what storing the behaviour policy's log-probabilities costs in a closed collection loop, on a real MI355X:
`env.record_logp()` (`ppg_record_logp`: log-softmax at the action, entropy, two launches, nothing read back) against its torch
restatement (`ObservationStore.record_logp_torch()`: `nonzero`, `log_softmax`-style float64 ops and index-scatters; the host waits
every step).  Per step, launch to launch, in alternating blocks within one process:

    (a) act + step + record + record_obs
    (b) act + record_logp + step + record + record_obs
    (c) act + record_logp_torch + step + record + record_obs

`act` is `FusedPolicy.act(env, sample=True, logits=bufs)` in all three, so the logits are written in all three.  HIP events around
blocks of `--block` steps, a warm-up round, `--reps` rounds of (a), (b), (c) in that order; every series is printed, with the added
cost (b) - (a) and (c) - (a) of every round -- the kernel path must be the cheaper one in EVERY round (the process ends with status 1
otherwise) -- and the medians.  Before any timing logp and entropy of record_logp() are compared with record_logp_torch() at the timed
size.

    python tools/time_record_logp.py                        # 4096 envs, default config
    python tools/time_record_logp.py --batch 64 --reps 3 --preroll 50 --block 16   # a rehearsal at a small size

The measurement runs in a child process under a time limit."""
import argparse
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)


def child(args):
    import numpy as np
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.policy import FusedPolicy, PolicyNet
    from predpreygrass_amd.trajectory import AgentTrajectories, ObservationStore
    assert torch.cuda.is_available(), "time_record_logp needs a ROCm GPU"
    B, T = args.batch, args.block
    # (bfloat16 observation rows, which the policy kernels read directly: the dtype plays no part in the call under test and keeps
    #  the store of a 4096-env block at a few GB)
    env = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", seed=1, obs_dtype=torch.bfloat16)
    torch.manual_seed(0)
    nets = [PolicyNet(config_env["predator_obs_range"]), PolicyNet(config_env["prey_obs_range"])]
    with torch.no_grad():   # (logits of order one, so that the sampled actions differ)
        for net in nets:
            for m in net.conv + net.fc:
                m.weight.mul_(3.0)
    fused = FusedPolicy(nets[0], nets[1])
    A = (nets[0].n_actions, nets[1].n_actions)
    bufs = tuple(torch.zeros((B * cap, a), dtype=torch.float32, device=env.device) for cap, a in zip((env.pred_capacity, env.prey_capacity), A))
    key = [0]

    def act():
        key[0] += 1
        fused.act(env, sample=True, seed=key[0], logits=bufs)

    env.reset()
    for _ in range(args.preroll):   # to the population the policy settles at
        act()
        env.step(env.actions, auto_reset=True)
    live = env.live_mask()
    n_pred, n_prey = live[:, :env.pred_capacity].sum().item(), live[:, env.pred_capacity:].sum().item()
    rows = (int(T * n_pred * 1.5) + B, int(T * n_prey * 1.5) + B)
    traj = AgentTrajectories(env, T, obs_rows=rows, logp=A)
    other = ObservationStore(env, T, rows, logp=A)

    # the results must agree before any time is worth reporting
    for t in range(min(T, 8)):
        act()
        if t > 0:
            traj.record_policy(bufs)
            other.record_logp_torch(t - 1, bufs)
        env.step(env.actions, auto_reset=True)
        traj.record(env.actions)
        other.record(t, env.actions)
    torch.cuda.synchronize()
    assert torch.equal(traj.store.slot, other.slot) and torch.equal(traj.store.cursor, other.cursor)
    for s in (0, 1):
        n = int(traj.store.cursor[s])
        assert n > 0, "nothing was stored"
        for x, y in ((traj.store.logp[s], other.logp[s]), (traj.store.entropy[s], other.entropy[s])):
            x, y = x[:n].cpu().numpy(), y[:n].cpu().numpy()
            fin = np.isfinite(y)
            assert np.array_equal(np.isnan(x), np.isnan(y)) and fin.any(), "kernel != record_logp_torch(): NaN in other slots"
            tol = np.maximum(np.spacing(np.abs(y[fin])).astype(np.float64), 1e-11)
            assert (np.abs(x[fin].astype(np.float64) - y[fin].astype(np.float64)) <= tol).all(), "kernel != record_logp_torch()"

    def block(policy):
        def run(n):
            traj.clear()
            for t in range(n):
                act()
                if t > 0:
                    policy(t - 1)
                env.step(env.actions, auto_reset=True)
                traj.record(env.actions)
        return run
    modes = [("(a) act + step + record + record_obs", block(lambda t: None)),
             ("(b) act + record_logp + step + record + record_obs", block(lambda t: traj.store.record_logp(t, bufs))),
             ("(c) act + record_logp_torch + step + record + record_obs", block(lambda t: traj.store.record_logp_torch(t, bufs)))]
    counts = []
    times = alternate(modes, args.reps, T, after={name: lambda: counts.append(traj.store.counts()) for name, _ in modes})
    (sp, dp), (sq, dq) = counts[-1]
    stored, dropped = (sp / T, sq / T), dp + dq
    ta, tb, tc = (times[name] for name, _ in modes)
    print(f"### B = {B}, S = {env.S}, {A[0]} / {A[1]} actions, kernel {env.step_kernel_name()}; {stored[0]:.0f} predator + {stored[1]:.0f} prey "
          f"rows stored per step, {dropped} dropped; µs per step, launch to launch, {args.reps} rounds of blocks of {T} steps, median (min-max)", flush=True)
    print("| what | µs per step | every round |\n|---|---|---|")
    for name, _ in modes:
        print(f"| {name} | {fmt(times[name], 1)} | {' '.join(f'{x:.1f}' for x in times[name])} |", flush=True)
    kernel, torch_ops = [y - x for x, y in zip(ta, tb)], [y - x for x, y in zip(ta, tc)]
    print(f"| (b) - (a): record_logp() | {fmt(kernel, 1)} | {' '.join(f'{x:.1f}' for x in kernel)} |")
    print(f"| (c) - (a): record_logp_torch() | {fmt(torch_ops, 1)} | {' '.join(f'{x:.1f}' for x in torch_ops)} |", flush=True)
    cheaper = all(k < t for k, t in zip(kernel, torch_ops))
    print(f"record_logp() is {'cheaper than' if cheaper else 'NOT cheaper than'} record_logp_torch() in every round", flush=True)
    fused.close()
    return 0 if cheaper else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--block", type=int, default=64, help="steps between two events = the horizon of the store")
    ap.add_argument("--reps", type=int, default=7, help="timed rounds")
    ap.add_argument("--preroll", type=int, default=300, help="steps before anything is timed")
    ap.add_argument("--limit", type=int, default=300, help="seconds the child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    passed = ["--batch", str(args.batch), "--block", str(args.block), "--reps", str(args.reps), "--preroll", str(args.preroll)]
    return run_children(__file__, 1, passed, args.limit, lambda i: "the measurement")


if __name__ == "__main__":
    sys.exit(main())
