"""Times the backward pass over recorded trajectories (returns / GAE): the torch recursion of AgentTrajectories
(`returns_torch` / `gae_torch`, what the library did before `ppg_backward`) against the kernel (`returns` / `gae` /
`returns_and_gae`), on a real MI355X.  HIP events, warm-up, several repetitions, median and spread; the kernel's outputs are
compared bit for bit with the torch recursion's at the timed size first.

    python tools/time_backward.py                      # the three shapes of profiles/EXPERIMENTS.md, one child process each
    python tools/time_backward.py --batch 64 --reps 3  # a rehearsal at a small size

Each shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.  The kernel is also timed with its loads placed at the top of each step instead of one step ahead
(PPG_BACKWARD_PREFETCH=0, read when a handle is created), alternating with the default in one process."""
import argparse
import os
import statistics
import sys

from timing import fmt, repeat_ms, run_children   # (tools/timing.py)

SHAPES = [("default", {}, 32), ("default", {}, 128), ("p128q256", {"pred_capacity": 128, "prey_capacity": 256}, 32)]
PEAK = 8.0e12   # bytes/s (MI355X HBM3E, spec)


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.trajectory import AgentTrajectories
    assert torch.cuda.is_available(), "time_backward needs a ROCm GPU"
    kw = dict(SHAPES[args.child][1])
    T, B = SHAPES[args.child][2], args.batch
    env = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", **kw)
    os.environ["PPG_BACKWARD_PREFETCH"] = "0"
    env_np = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", **kw)   # only its handle is used: B, S, load placement
    del os.environ["PPG_BACKWARD_PREFETCH"]
    S = env.S
    env.reset()
    traj = AgentTrajectories(env, T)
    for _ in range(T):
        env.step(random_actions=True, auto_reset=True)
        traj.record()
    values = torch.randn((T, B, S), dtype=torch.float64, device=env.device, generator=torch.Generator(env.device).manual_seed(1))
    gamma, lam = 0.99, 0.95
    # the results must not differ (bit for bit) before any time is worth reporting
    G, A = traj.returns_and_gae(values, gamma, lam)
    assert torch.equal(G, traj.returns_torch(gamma)) and torch.equal(A, traj.gae_torch(values, gamma, lam)), "kernel != torch recursion"
    stored = (traj.reward, traj.next_row, traj.in_use, traj.terminated, traj.truncated)
    G2, A2 = env_np.backward(*stored, gamma, lam, values=values)
    assert torch.equal(G, G2) and torch.equal(A, A2), "load placement changed a result"
    del G, A, G2, A2
    links = int(((traj.next_row >= 0) & traj.in_use).sum())
    n = T * B * S
    inputs = 8 + 2 + 3
    rows = [("(a) returns_torch()", lambda: traj.returns_torch(gamma), args.reps_torch, None),
            ("(b) gae_torch()", lambda: traj.gae_torch(values, gamma, lam), args.reps_torch, None),
            ("(c) returns()", lambda: traj.returns(gamma), args.reps, n * (inputs + 8)),
            ("(d) gae()", lambda: traj.gae(values, gamma, lam), args.reps, n * (inputs + 8 + 8)),
            ("(e) returns_and_gae()", lambda: traj.returns_and_gae(values, gamma, lam), args.reps, n * (inputs + 8 + 16))]
    print(f"### B = {B}, S = {S} ({SHAPES[args.child][0]}), T = {T}: {int(traj.in_use.sum()) / (T * B):.1f} rows in use per env-step, "
          f"{links / max(1, (T - 1) * B):.1f} links per env-step; ms, median (min-max)", flush=True)
    print("| what | ms | bytes moved | of 8 TB/s |\n|---|---|---|---|")
    med = {}
    for name, fn, reps, nbytes in rows:
        ts = repeat_ms(fn, reps, args.warmup)
        med[name[:3]] = ts
        extra = f" {nbytes / 1e6:.0f} MB | {nbytes / (statistics.median(ts) * 1e-3) / PEAK:.3f} |" if nbytes else " | |"
        print(f"| {name} | {fmt(ts, 3)} |{extra}", flush=True)
    # load placement: one step ahead (default) against the top of the step, alternating in one process
    ahead, top = [], []
    both = lambda e: (lambda: e.backward(*stored, gamma, lam, values=values))
    for _ in range(3):
        ahead += repeat_ms(both(env), max(3, args.reps // 3), 1)
        top += repeat_ms(both(env_np), max(3, args.reps // 3), 1)
    print(f"| (e) through env.backward(), loads one step ahead | {fmt(ahead, 3)} | | |")
    print(f"| (e) through env.backward(), loads at the top of the step | {fmt(top, 3)} | | |")
    d, b = med["(d)"], med["(b)"]
    print(f"gae(): torch {statistics.median(b):.3f} ms -> kernel {statistics.median(d):.3f} ms = {statistics.median(b) / statistics.median(d):.1f}x "
          f"(spread: torch {max(b) - min(b):.3f}, kernel {max(d) - min(d):.3f} ms)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15, help="repetitions of the kernel calls")
    ap.add_argument("--reps-torch", type=int, default=5, help="repetitions of the torch recursions")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    passed = ["--batch", str(args.batch), "--reps", str(args.reps), "--reps-torch", str(args.reps_torch), "--warmup", str(args.warmup)]
    return run_children(__file__, len(SHAPES), passed, args.limit, lambda i: f"shape {i}")


if __name__ == "__main__":
    sys.exit(main())
