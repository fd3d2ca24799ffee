"""Times one PPO minibatch step of the loss on a real MI355X: `AgentTrajectories.ppo_loss()` (the `ppg_ppo_loss` kernels, two launches)
plus `torch.autograd.backward([logits, values], [grad_logits, grad_values])` against `ppo_loss_torch(dtype=torch.float32)` plus
`loss.backward()` -- the composition a user had to write before the kernels -- on the same data, with `dist` and `values`.  HIP
events around alternating blocks, a warm-up round, median and range; the two losses and gradients are compared at the timed size
first.

    python tools/time_ppo_loss.py                     # M in {128, 4096, 131072} x A in {9, 25}, one child process each
    python tools/time_ppo_loss.py --reps 3 --steps 5  # a rehearsal

Each shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.  The store's columns are synthetic (random old logits and actions, their log-probabilities, random advantages and targets);
the new logits are the old ones plus noise, so that all three clip branches occur.  In both modes the logits and values are one
elementwise op behind leaf tensors, as they are behind a network."""
import argparse
import statistics
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)

SHAPES = [(M, A) for M in (128, 4096, 131072) for A in (9, 25)]
HYPER = dict(clip=0.3, vf_clip=10.0, vf_coeff=1.0, ent_coeff=0.01, kl_coeff=0.2)


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.trajectory import AgentTrajectories
    assert torch.cuda.is_available(), "time_ppo_loss needs a ROCm GPU"
    M, A = SHAPES[args.child]
    n = 2 * M                                    # samples in the store: a minibatch is half of them
    env = BatchedPredPreyGrass(config_env, batch_size=1, device="cuda:0", obs_dtype=torch.bfloat16)
    traj = AgentTrajectories(env, 1, obs_rows=(n, 0), logp=(A, A), dist=True)
    st, dev = traj.store, env.device
    gen = torch.Generator(dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    st.dist[0].copy_(rnd(n, A) * 1.5)
    st.action[0].copy_(torch.randint(0, A, (n,), device=dev, generator=gen).to(torch.int8))
    st.logp[0].copy_(torch.log_softmax(st.dist[0].double(), 1).gather(1, st.action[0].long()[:, None])[:, 0].float())
    adv, target = rnd(n), rnd(n) * 2
    index = torch.randperm(n, device=dev, generator=gen)[:M].to(torch.int32)
    z = (st.dist[0][index.long()] + 0.3 * rnd(M, A)).requires_grad_(True)
    zv = (target[index.long()] + rnd(M)).requires_grad_(True)

    def kernel_step():
        logits, values = z * 1.0, zv * 1.0
        loss, stats, gl, gv = traj.ppo_loss(0, logits, values, index, adv, target, **HYPER)
        torch.autograd.backward([logits, values], [gl, gv])
        return loss

    def torch_step():
        logits, values = z * 1.0, zv * 1.0
        loss, stats = traj.ppo_loss_torch(0, logits, values, index, adv, target, dtype=torch.float32, **HYPER)
        loss.backward()
        return loss

    def grads(step):
        z.grad = zv.grad = None
        loss = step()
        return float(loss.detach()), z.grad.clone(), zv.grad.clone()
    lk, gk, vk = grads(kernel_step)
    lt, gt, vt = grads(torch_step)
    assert abs(lk - lt) <= 1e-4 * max(1.0, abs(lk)), ("kernel != torch composition (loss)", lk, lt)
    assert torch.allclose(gk, gt, rtol=1e-3, atol=1e-6 / M) and torch.allclose(vk, vt, rtol=1e-3, atol=1e-6 / M), "kernel != torch composition (gradients)"

    def block(step):
        def run(steps):
            for _ in range(steps):
                z.grad = zv.grad = None
                step()
        return run
    times = alternate([("kernel", block(kernel_step)), ("torch", block(torch_step))], args.reps, args.steps)
    k, t = times["kernel"], times["torch"]
    verdict = "ranges disjoint, the kernel's the lower" if max(k) < min(t) else "RANGES OVERLAP OR THE KERNEL IS NOT THE LOWER"
    print(f"| {M} | {A} | {fmt(k, 1)} | {fmt(t, 1)} | {statistics.median(t) / statistics.median(k):.1f}x ({verdict}) |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="timed rounds of alternating blocks")
    ap.add_argument("--steps", type=int, default=20, help="minibatch steps per block")
    ap.add_argument("--limit", type=int, default=120, help="seconds a shape's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    print("| M | A | ppo_loss() + autograd.backward, µs per step | ppo_loss_torch(float32) + loss.backward(), µs per step | torch / kernel |\n"
          "|---|---|---|---|---|", flush=True)
    return run_children(__file__, len(SHAPES), ["--reps", str(args.reps), "--steps", str(args.steps)], args.limit, lambda i: f"shape {SHAPES[i]}")


if __name__ == "__main__":
    sys.exit(main())
