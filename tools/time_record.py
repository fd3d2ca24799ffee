"""Times what recording a step costs behind the step, on a real MI355X: the torch ops `AgentTrajectories.record()` used to be
(`record_torch()`, about nineteen small launches behind `ppg_link`) against the kernel (`env.record()`, `ppg_record`: the link plus
the stores in one launch) and against a captured and replayed step + record (`trajectory.GraphedCollector`).  Per step, launch to
launch, in alternating blocks within one process:

    (a) the step alone                     (b) step + link()
    (c) step + record_torch()              (d) step + record()  [the kernel, host step index]
    (e) GraphedCollector.replay            [step + kernel + increment of the device step index, one graph launch]

HIP events around blocks of `--block` steps, a warm-up block of every mode, `--reps` blocks each, median and min-max of the
per-step time.  Before any timing the bytes of record() are compared with record_torch() on a twin env at the timed size.

    python tools/time_record.py                        # the two shapes of profiles/EXPERIMENTS.md, one child process each
    python tools/time_record.py --batch 64 --reps 3 --preroll 50   # a rehearsal at a small size

Each shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started."""
import argparse
import statistics
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)

SHAPES = [("default", {}), ("p128q256", {"pred_capacity": 128, "prey_capacity": 256})]
NAMES = ("reward", "in_use", "terminated", "truncated", "next_row")


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.trajectory import AgentTrajectories, GraphedCollector
    assert torch.cuda.is_available(), "time_record needs a ROCm GPU"
    kw = dict(SHAPES[args.child][1])
    B, T = args.batch, args.horizon
    env = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", seed=1, **kw)
    twin = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", seed=1, **kw)
    S = env.S

    def step(e=env):
        e.step(random_actions=True, auto_reset=True)

    def kernel_record(traj):
        """record() through the kernel whatever AgentTrajectories.record() defaults to."""
        if traj.t >= traj.horizon:
            traj.clear()
        traj.env.record(traj.reward, traj.in_use, traj.terminated, traj.truncated, traj.next_row, traj.t)
        traj.t = traj.t + 1

    def torch_record(traj):
        if traj.t >= traj.horizon:
            traj.clear()
        traj.record_torch()

    env.reset()
    twin.reset()
    for _ in range(args.preroll):   # to a stationary population
        step(env)
        step(twin)
    # the results must not differ (byte for byte) before any time is worth reporting
    traj, want = AgentTrajectories(env, T), AgentTrajectories(twin, T)
    for _ in range(min(T, 16)):
        step(env)
        step(twin)
        kernel_record(traj)
        torch_record(want)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(getattr(traj, k).view(torch.uint8), getattr(want, k).view(torch.uint8)), f"kernel != record_torch(): {k}"
    assert bool((traj.next_row >= 0).any()), "nothing linked"
    live = env.live_mask()
    n_pred, n_prey = live[:, :env.pred_capacity].sum().item() / B, live[:, env.pred_capacity:].sum().item() / B
    del twin, want

    dev_traj = AgentTrajectories(env, T, step_on_device=True)
    loop = GraphedCollector(env, dev_traj)

    def block_a(n):
        for _ in range(n):
            step()

    def block_b(n):
        for _ in range(n):
            step()
            env.link()

    def block_c(n):
        for _ in range(n):
            step()
            torch_record(traj)

    def block_d(n):
        for _ in range(n):
            step()
            kernel_record(traj)

    def block_e(n):
        dev_traj.clear()   # (one small launch per block: the horizon is the block)
        loop.replay(n)

    modes = [("(a) the step alone", block_a), ("(b) step + link()", block_b), ("(c) step + record_torch()", block_c),
             ("(d) step + record(), the kernel", block_d), ("(e) GraphedCollector.replay", block_e)]
    n = min(args.block, T)
    times = alternate(modes, args.reps, n)
    print(f"### B = {B}, S = {S} ({SHAPES[args.child][0]}), horizon {T}: {n_pred:.1f} predator + {n_prey:.1f} prey rows per env after "
          f"{args.preroll} steps, kernel {env.step_kernel_name()}, plan {env.wave_plan()}; µs per step, launch to launch, {args.reps} blocks "
          f"of {n} steps each, median (min-max)", flush=True)
    print("| what | µs per step |\n|---|---|")
    for name, _ in modes:
        print(f"| {name} | {fmt(times[name], 1)} |", flush=True)
    med = {name[:3]: statistics.median(ts) for name, ts in times.items()}
    spread = {name[:3]: max(ts) - min(ts) for name, ts in times.items()}
    print(f"record_torch() costs {med['(c)'] - med['(a)']:.1f} µs per step, the kernel {med['(d)'] - med['(a)']:.1f}, link() alone "
          f"{med['(b)'] - med['(a)']:.1f}; (c) - (d) = {med['(c)'] - med['(d)']:.1f} µs against spreads of {spread['(c)']:.1f} (c) and "
          f"{spread['(d)']:.1f} (d); replayed {med['(e)']:.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--block", type=int, default=128, help="steps between two events (at most the horizon)")
    ap.add_argument("--reps", type=int, default=9, help="timed blocks per mode")
    ap.add_argument("--preroll", type=int, default=700, help="steps before anything is timed")
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    passed = ["--batch", str(args.batch), "--horizon", str(args.horizon), "--block", str(args.block), "--reps", str(args.reps),
              "--preroll", str(args.preroll)]
    return run_children(__file__, len(SHAPES), passed, args.limit, lambda i: f"shape {i}")


if __name__ == "__main__":
    sys.exit(main())
