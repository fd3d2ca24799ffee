"""Times the learner-to-actor hand-over on a real MI355X: `FusedPolicy.update(pred_net, prey_net)` (the `ppg_policy_repack` kernel,
one launch per species, parameters read in place on the device; steady state, after the first call has built the repack maps)
against the only way there was before it, `fused.close(); fused = FusedPolicy(pred_net, prey_net)` from the same device-resident
networks (a read-back of every parameter, the repack on the CPU, an allocation and a blocking upload).  HIP events around alternating
blocks (a block of updates is `--ratio` times as many calls as a block of recreations), a warm-up round, median and range; the host time an update call takes is printed next to it.  Before the clock starts the
updated policy's logits are compared, bit for bit, with the recreated one's.

    python tools/time_policy_update.py                     # the reference network at R = 7 and 9, the FC chain (256, 256) at R = 9
    python tools/time_policy_update.py --reps 3 --steps 5  # a rehearsal

Each network runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.  What the table cannot show is the point of the update: it does not make the host wait, and graphs captured around
`act()` stay valid -- a recreated policy has its weights at new addresses and every captured loop must be captured again."""
import argparse
import statistics
import sys
import time

from timing import alternate, fmt, run_children   # (tools/timing.py)

# (label, predator window, prey window, PolicyNet keywords)
NETWORKS = [("hwc (16, 32, 64), R = 7", 7, 7, {}),
            ("hwc (16, 32, 64), R = 9", 9, 9, {}),
            ("hwc (16, 32, 64) + FC chain (256, 256), R = 9", 9, 9, dict(head_hiddens=(256, 256)))]


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.policy import FusedPolicy, PolicyNet
    assert torch.cuda.is_available(), "time_policy_update needs a ROCm GPU"
    label, Rp, Rq, kw = NETWORKS[args.child]
    torch.manual_seed(1)
    nets = [PolicyNet(Rp, **kw).to("cuda:0"), PolicyNet(Rq, **kw).to("cuda:0")]
    other = [PolicyNet(Rp, **kw).to("cuda:0"), PolicyNet(Rq, **kw).to("cuda:0")]
    env = BatchedPredPreyGrass({**config_env, "predator_obs_range": Rp, "prey_obs_range": Rq}, batch_size=8, device="cuda:0", seed=1)
    env.reset()
    for _ in range(10):
        env.step(random_actions=True, auto_reset=True)
    box = {"updated": FusedPolicy(other[0], other[1]), "recreated": FusedPolicy(other[0], other[1])}
    box["updated"].update(nets[0], nets[1])       # the first call: builds and uploads the maps
    box["recreated"].close()
    box["recreated"] = FusedPolicy(nets[0], nets[1])
    a, b = box["updated"].act(env, want_logits=True), box["recreated"].act(env, want_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0), "update != recreate"
    host = []

    def update(steps):   # (args.ratio hand-overs per step: a block of updates should last about as long as a block of recreations)
        t0 = time.perf_counter()
        for _ in range(steps * args.ratio):
            box["updated"].update(nets[0], nets[1])
        host.append((time.perf_counter() - t0) * 1e6 / (steps * args.ratio))

    def recreate(steps):
        for _ in range(steps):
            box["recreated"].close()
            box["recreated"] = FusedPolicy(nets[0], nets[1])
    times = alternate([("update", update), ("recreate", recreate)], args.reps, args.steps)
    u, r = [t / args.ratio for t in times["update"]], times["recreate"]
    verdict = "ranges disjoint, the update's the lower" if max(u) < min(r) else "RANGES OVERLAP OR THE UPDATE IS NOT THE LOWER"
    print(f"| {label} | {fmt(u, 1)} | {fmt(host[1:], 1)} | {fmt(r, 1)} | {statistics.median(r) / statistics.median(u):.1f}x ({verdict}) |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="timed rounds of alternating blocks")
    ap.add_argument("--steps", type=int, default=20, help="recreations per block")
    ap.add_argument("--ratio", type=int, default=100, help="updates per recreation: a block of updates is steps x ratio calls")
    ap.add_argument("--limit", type=int, default=120, help="seconds a network's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    print("| networks (both species) | update(), µs per call (HIP events) | update(), host µs per call | close() + FusedPolicy(), µs per call | recreate / update |\n"
          "|---|---|---|---|---|", flush=True)
    return run_children(__file__, len(NETWORKS), ["--reps", str(args.reps), "--steps", str(args.steps), "--ratio", str(args.ratio)], args.limit, lambda i: f"network {NETWORKS[i][0]}")


if __name__ == "__main__":
    sys.exit(main())
