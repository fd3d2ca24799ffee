"""Times `FusedPolicy.evaluate()` over a recorded sample store on a real MI355X: both species' networks over every stored sample of
4096 envs x 8 recorded steps (`ppg_policy_evaluate`: the plan kernel ppg_policy_plan_rows + the bf16 matrix-core forward kernels of
`act`, the count read from `store.cursor` on the device) against the only thing there was before it, `PolicyNet.forward` in float32
over the same rows, in chunks so that its activations fit.  One child process per row dtype (float64, float32, bfloat16 stores of
envs of that dtype).  HIP events around alternating blocks, a warm-up round, median and range (tools/timing.py); before the clock
starts the two are compared (the kernels round to bf16 between layers: the largest difference is printed).

    python tools/time_policy_evaluate.py                       # 4096 envs, 8 steps, the reference's networks (R = 7 / 9)
    python tools/time_policy_evaluate.py --envs 64 --reps 2    # a rehearsal

After a child that fails or runs out of time nothing more is started."""
import argparse
import statistics
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)

DTYPES = ["float64", "float32", "bfloat16"]


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.policy import FusedPolicy, PolicyNet
    from predpreygrass_amd.trajectory import AgentTrajectories
    assert torch.cuda.is_available(), "time_policy_evaluate needs a ROCm GPU"
    dev, dtype = "cuda:0", getattr(torch, DTYPES[args.child])
    torch.manual_seed(1)
    nets = [PolicyNet(7).to(dev), PolicyNet(9).to(dev)]
    fused = FusedPolicy(nets[0], nets[1])
    env = BatchedPredPreyGrass(dict(config_env), batch_size=args.envs, device=dev, obs_dtype=dtype, seed=1)
    env.reset()
    for _ in range(args.grow):      # let the populations grow towards the benchmark's
        env.step(random_actions=True, auto_reset=True)
    T = args.record
    traj = AgentTrajectories(env, T, obs_rows=(T * args.envs * env.pred_capacity, T * args.envs * env.prey_capacity))
    for t in range(T):
        fused.act(env, sample=True, seed=50 + t)
        env.step(env.actions, auto_reset=True)
        traj.record(env.actions)
    st = traj.store
    n = st.cursor[:2].tolist()
    assert st.cursor[2:].tolist() == [0, 0] and min(n) > 0
    outs = [torch.zeros((st.capacity[s], 9), dtype=torch.float32, device=dev) for s in (0, 1)]

    def evaluate(steps):
        for _ in range(steps):
            for s in (0, 1):
                fused.evaluate(s, st.obs[s], count=st.cursor[s:s + 1], out=outs[s])

    ref = [torch.zeros((n[s], 9), dtype=torch.float32, device=dev) for s in (0, 1)]

    def forward(steps):
        with torch.no_grad():
            for _ in range(steps):
                for s in (0, 1):
                    for lo in range(0, n[s], args.chunk):
                        ref[s][lo:lo + args.chunk] = nets[s](st.obs[s][lo:min(lo + args.chunk, n[s])])
    evaluate(1)
    forward(1)
    torch.cuda.synchronize()
    err = max(float((outs[s][:n[s]] - ref[s]).abs().max()) / max(1.0, float(ref[s].abs().max())) for s in (0, 1))
    times = alternate([("evaluate", evaluate), ("forward", forward)], args.reps, args.steps)
    e, f = [t / 1000.0 for t in times["evaluate"]], [t / 1000.0 for t in times["forward"]]   # ms per evaluation of both species
    rows = n[0] + n[1]
    verdict = "ranges disjoint, evaluate the lower" if max(e) < min(f) else "RANGES OVERLAP OR EVALUATE IS NOT THE LOWER"
    print(f"| {DTYPES[args.child]} | {n[0]} + {n[1]} | {fmt(e, 3)} | {rows / statistics.median(e) / 1e3:.1f} | {fmt(f, 2)} | "
          f"{statistics.median(f) / statistics.median(e):.1f}x ({verdict}) | {err:.2e} |", flush=True)
    fused.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--record", type=int, default=8, help="recorded steps")
    ap.add_argument("--grow", type=int, default=200, help="random-action steps in front of the recorded ones")
    ap.add_argument("--chunk", type=int, default=65536, help="rows per float32 torch forward")
    ap.add_argument("--reps", type=int, default=7, help="timed rounds of alternating blocks")
    ap.add_argument("--steps", type=int, default=3, help="evaluations of both species per block")
    ap.add_argument("--limit", type=int, default=240, help="seconds a dtype's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    print("| rows | samples (predators + prey) | evaluate(), both species, ms (HIP events) | M rows/s | PolicyNet.forward float32, chunked, ms | forward / evaluate | max rel. difference |\n"
          "|---|---|---|---|---|---|---|", flush=True)
    passthrough = [x for k in ("envs", "record", "grow", "chunk", "reps", "steps") for x in (f"--{k}", str(getattr(args, k)))]
    return run_children(__file__, len(DTYPES), passthrough, args.limit, lambda i: f"dtype {DTYPES[i]}")


if __name__ == "__main__":
    sys.exit(main())
