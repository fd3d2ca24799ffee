"""Times advantages and returns in SAMPLE order over recorded trajectories on a real MI355X: `AgentTrajectories.targets()` (the
`ppg_backward_samples` kernel, one launch) against `targets_torch()` -- scatter() of the per-sample values into [T,B,S], returns_and_gae()
(`ppg_backward`), four flat() gathers and .float(): what the library offered before the kernel -- on the same data.  HIP events,
warm-up, several repetitions, median and range; all outputs are compared for equal bytes at the timed size first.

    python tools/time_backward_samples.py                      # the three shapes of tools/time_backward.py, one child process each
    python tools/time_backward_samples.py --batch 64 --reps 3  # a rehearsal at a small size

Each shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.  The store is filled by recorded random-action steps, the per-sample values are random.  The kernel is
also timed with its loads one step ahead (PPG_BACKWARD_PREFETCH=1, read when a handle is created) and at the top of each step (=0,
its default), alternating in one process, and without the stats and without the returns."""
import argparse
import os
import statistics
import sys
import types

from time_backward import PEAK, SHAPES   # (tools/time_backward.py: the shapes of the ppg_backward record)
from timing import fmt, repeat_ms, run_children   # (tools/timing.py)

# store rows per env-step (predators, prey): about twice what the default population has in use (15-17 rows per env-step); the
# observations themselves are not what is timed, so the envs hold them as bfloat16 (10 GB of store at 128 steps of 4096 envs)
ROWS = (14, 22)


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.trajectory import AgentTrajectories
    assert torch.cuda.is_available(), "time_backward_samples needs a ROCm GPU"
    name, kw, T = SHAPES[args.child]
    kw, B = dict(kw), args.batch
    env = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", obs_dtype=torch.bfloat16, **kw)
    placed = {}   # (only the handles of these two are used: B, S and the load placement, which is read when a handle is created)
    for knob in ("0", "1"):
        os.environ["PPG_BACKWARD_PREFETCH"] = knob
        placed[knob] = BatchedPredPreyGrass(config_env, batch_size=B, device="cuda:0", obs_dtype=torch.bfloat16, **kw)
    del os.environ["PPG_BACKWARD_PREFETCH"]
    S = env.S
    env.reset()
    traj = AgentTrajectories(env, T, obs_rows=tuple(T * B * r for r in ROWS))
    for _ in range(T):
        env.step(random_actions=True, auto_reset=True)
        traj.record()
    (n_pred, dropped_pred), (n_prey, dropped_prey) = traj.store.counts()
    # (rows the store dropped take part in both computations with V = 0: fewer samples, the same comparison)
    print(f"rows dropped by the store: {dropped_pred} predator, {dropped_prey} prey", flush=True)
    gen = torch.Generator(env.device).manual_seed(1)
    v = [torch.randn((n,), dtype=torch.float32, device=env.device, generator=gen) for n in (n_pred, n_prey)]
    gamma, lam = 0.99, 0.95
    # the results must not differ (bit for bit) before any time is worth reporting
    adv, ret, stats = traj.targets(v[0], v[1], gamma, lam)
    adv_t, ret_t, stats_t = traj.targets_torch(v[0], v[1], gamma, lam)
    for s in (0, 1):
        assert torch.equal(adv[s].view(torch.int32), adv_t[s].view(torch.int32)), "kernel != torch composition (advantages)"
        assert torch.equal(ret[s].view(torch.int32), ret_t[s].view(torch.int32)), "kernel != torch composition (returns)"
    assert torch.equal(stats[:, :, 0], stats_t[:, :, 0]) and torch.allclose(stats, stats_t, rtol=1e-12, atol=1e-9), "stats"
    stored = (traj.reward, traj.next_row, traj.in_use, traj.terminated, traj.truncated)
    view = types.SimpleNamespace(horizon=T, capacity=(n_pred, n_prey), slot=traj.store.slot)
    for e in placed.values():
        adv2, ret2, stats2 = e.backward_samples(view, *stored, gamma, lam, values=v, stats=True)
        assert all(torch.equal(x, y) for x, y in zip(adv + ret + [stats], adv2 + ret2 + [stats2])), "load placement changed a result"
    del adv_t, ret_t, stats_t, adv2, ret2, stats2
    n, ns = T * B * S, n_pred + n_prey
    # bytes counted: per [T,B,S] element reward 8 + next_row 2 + three flags 3 + slot 4 read; per stored sample a value read (4) and
    # two float32 written.  The composition: the scatter writes a float32 [T,B,S] (fill + samples), ppg_backward reads 13 + 4 and
    # writes 16 per element, four gathers read an index (4, widened to 8) and 8 and write 8, four casts read 8 and write 4
    kernel_bytes = n * 17 + ns * 12
    torch_bytes = n * (4 + 17 + 16) + ns * (2 * 4 + 4) + 2 * ns * (4 + 8 + 8 + 8 + 8 + 4)
    rows = [("(a) targets_torch(): scatter + ppg_backward + 4 gathers + .float()", lambda: traj.targets_torch(v[0], v[1], gamma, lam, stats=False), args.reps_torch, torch_bytes),
            ("(b) targets_torch() with index_add stats", lambda: traj.targets_torch(v[0], v[1], gamma, lam), args.reps_torch, None),
            ("(c) targets(): advantages + returns + stats", lambda: traj.targets(v[0], v[1], gamma, lam), args.reps, kernel_bytes),
            ("(d) targets(stats=False)", lambda: traj.targets(v[0], v[1], gamma, lam, stats=False), args.reps, kernel_bytes),
            ("(e) targets(returns=False)", lambda: traj.targets(v[0], v[1], gamma, lam, returns=False), args.reps, kernel_bytes - ns * 4)]
    print(f"### B = {B}, S = {S} ({name}), T = {T}: {n_pred} predator + {n_prey} prey samples ({ns / n:.3f} of the [T,B,S] elements); "
          f"ms, median (min-max)", flush=True)
    print("| what | ms | bytes counted | of 8 TB/s |\n|---|---|---|---|")
    med = {}
    for label, fn, reps, nbytes in rows:
        ts = repeat_ms(fn, reps, args.warmup)
        med[label[:3]] = ts
        extra = f" {nbytes / 1e6:.0f} MB | {nbytes / (statistics.median(ts) * 1e-3) / PEAK:.3f} |" if nbytes else " | |"
        print(f"| {label} | {fmt(ts, 3)} |{extra}", flush=True)
    # load placement: one step ahead (default) against the top of the step, alternating in one process
    ahead, top = [], []
    both = lambda e: (lambda: e.backward_samples(view, *stored, gamma, lam, values=v, stats=True))
    for _ in range(3):
        ahead += repeat_ms(both(placed["1"]), max(3, args.reps // 3), 1)
        top += repeat_ms(both(placed["0"]), max(3, args.reps // 3), 1)
    print(f"| (c) through env.backward_samples(), loads one step ahead (PPG_BACKWARD_PREFETCH=1) | {fmt(ahead, 3)} | | |")
    print(f"| (c) through env.backward_samples(), loads at the top of the step (=0, the default) | {fmt(top, 3)} | | |")
    a, c = med["(a)"], med["(c)"]
    verdict = "ranges disjoint, the kernel's the lower" if max(c) < min(a) else "RANGES OVERLAP OR THE KERNEL IS NOT THE LOWER"
    print(f"targets(): torch composition {statistics.median(a):.3f} ms -> kernel {statistics.median(c):.3f} ms = "
          f"{statistics.median(a) / statistics.median(c):.1f}x ({verdict})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=15, help="repetitions of the kernel calls")
    ap.add_argument("--reps-torch", type=int, default=7, help="repetitions of the torch composition")
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
