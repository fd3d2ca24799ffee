"""Times one PPO minibatch step of the networks on a real MI355X: the kernel path -- `NetLearner` forward (`ppg_net_forward`, one
launch) for actor and critic, `AgentTrajectories.ppo_loss()` (two launches), `torch.autograd.backward([logits, values], [grad_logits,
grad_values])` (`ppg_net_backward`, two launches per network, and autograd's accumulation into `p.grad`) -- against the torch
composition on the same data: `net(obs[index.long()])` for actor and critic, the same `ppo_loss()`, the same `autograd.backward`.
HIP events around alternating blocks, a warm-up round, median and range; first, at the timed size, the outputs and parameter gradients
of each path are measured against the same step with the networks in float64 (max|x - ref| / max|ref| per tensor, the worst printed).

    python tools/time_net_step.py                     # M in {128, 4096} x {predator R = 7, prey R = 9}, A = 9, one child process each
    python tools/time_net_step.py --reps 3 --steps 5  # a rehearsal

Each shape runs in a child process of its own under a time limit; after a child that fails or runs out of time nothing more is
started.  The store is synthetic: observation rows of zeros and small energies, random old logits and actions with their
log-probabilities, random advantages and targets.  The networks are the reference's (three convolutions 16 / 32 / 64, channels-last,
one linear head), the critic the same with one output."""
import argparse
import statistics
import sys

from timing import alternate, fmt, run_children   # (tools/timing.py)

SHAPES = [(M, s) for M in (128, 4096) for s in (0, 1)]
SPECIES = ("predator", "prey")
A = 9
HYPER = dict(clip=0.3, vf_clip=10.0, vf_coeff=1.0, ent_coeff=0.01, kl_coeff=0.2)


def child(args):
    import torch
    from predpreygrass_amd.batched import BatchedPredPreyGrass
    from predpreygrass_amd.config import config_env
    from predpreygrass_amd.policy import PolicyNet
    from predpreygrass_amd.trajectory import AgentTrajectories, NetLearner
    assert torch.cuda.is_available(), "time_net_step needs a ROCm GPU"
    M, s = SHAPES[args.child]
    n = 2 * M                                    # samples in the store: a minibatch is half of them
    env = BatchedPredPreyGrass(config_env, batch_size=1, device="cuda:0", obs_dtype=torch.bfloat16)
    R = (env.Rp, env.Rq)[s]
    traj = AgentTrajectories(env, 1, obs_rows=(n, 0) if s == 0 else (0, n), logp=(A, A), dist=True)
    st, dev = traj.store, env.device
    gen = torch.Generator(dev).manual_seed(1)
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float32, device=dev, generator=gen)
    shape = tuple(st.obs[s].shape)
    energy = torch.randint(1, 257, shape, device=dev, generator=gen).float() / 64.0
    st.obs[s].copy_(torch.where(torch.rand(shape, device=dev, generator=gen) < 0.3, energy, torch.zeros_like(energy)))
    st.dist[s].copy_(rnd(n, A) * 1.5)
    st.action[s].copy_(torch.randint(0, A, (n,), device=dev, generator=gen).to(torch.int8))
    st.logp[s].copy_(torch.log_softmax(st.dist[s].double(), 1).gather(1, st.action[s].long()[:, None])[:, 0].float())
    adv, target = rnd(n), rnd(n) * 2
    index = torch.randperm(n, device=dev, generator=gen)[:M].to(torch.int32)
    torch.manual_seed(3)
    nets = [PolicyNet(R, n_out).to(dev) for n_out in (A, 1)]
    learners = [NetLearner(env, net, max_rows=M) for net in nets]
    params = [p for net in nets for p in net.parameters()]

    def step(kernel):
        if kernel:
            logits, values = traj.forward(learners[0], s, index), traj.forward(learners[1], s, index)[:, 0]
        else:
            rows = st.obs[s][index.long()]
            logits, values = nets[0](rows), nets[1](rows)[:, 0]
        loss, stats, gl, gv = traj.ppo_loss(s, logits, values, index, adv, target, **HYPER)
        torch.autograd.backward([logits, values], [gl, gv])
        return logits, values, gl, gv

    def outcome(kernel):
        for p in params:
            p.grad = None
        logits, values, gl, gv = step(kernel)
        return [logits.detach().clone(), values.detach().clone(), gl.clone(), gv.clone()] + [p.grad.clone() for p in params]

    def reference():
        """The same step with the networks in float64 (torch on the CPU; the loss kernel on the device): what each float32 path is
        measured against."""
        import copy
        twins = [copy.deepcopy(net).cpu().double() for net in nets]
        rows = st.obs[s][index.long()].to(torch.float32).double().cpu()

        def forward(net):
            x = net.encoder.actor_encoder.net[0].cnn(rows.permute(0, 3, 1, 2))
            return net.pi.net.mlp(x.permute(0, 2, 3, 1).flatten(1))
        logits, values = forward(twins[0]), forward(twins[1])[:, 0]
        loss, stats, gl, gv = traj.ppo_loss(s, logits.float().to(dev), values.float().to(dev).contiguous(), index, adv, target, **HYPER)
        torch.autograd.backward([logits, values], [gl.double().cpu(), gv.double().cpu()])
        return [logits.detach(), values.detach(), gl.double().cpu(), gv.double().cpu()] + [p.grad for net in twins for p in net.parameters()]
    names = ["logits", "values", "grad_logits", "grad_values"] + [f"{role}.{n}" for role, net in zip(("actor", "critic"), nets) for n, _ in net.named_parameters()]
    ref = reference()
    worst = {}
    for path, kernel in (("kernel", True), ("torch", False)):
        errs = [float((x.double().cpu() - r).abs().max() / r.abs().max()) for x, r in zip(outcome(kernel), ref)]
        e, name = max(zip(errs, names))
        print(f"# M = {M} {SPECIES[s]} {path} path against float64: " + ", ".join(f"{n.replace('encoder.actor_encoder.net.0.', '').replace('pi.net.', '')} {x:.1e}"
                                                                                 for x, n in zip(errs, names)), flush=True)
        worst[path] = f"{e:.1e} ({name.replace('encoder.actor_encoder.net.0.', '').replace('pi.net.', '')})"
        # the measure of tests/net_cases.py, per tensor, against float64; the tests hold the kernels to 1e-4 on their shapes -- here the
        # figure is printed into the table, and 1e-3 only stops a timing of something that computes another thing
        assert e <= 1e-3, (path, "differs from the float64 step", name, e)

    def block(kernel):
        def run(steps):
            for _ in range(steps):
                for p in params:
                    p.grad = None
                step(kernel)
        return run
    times = alternate([("kernel", block(True)), ("torch", block(False))], args.reps, args.steps)
    k, t = times["kernel"], times["torch"]
    verdict = "ranges disjoint, the kernel path the lower" if max(k) < min(t) else "RANGES OVERLAP OR THE KERNEL PATH IS NOT THE LOWER"
    print(f"| {M} | {SPECIES[s]} R = {R} | {learners[0].tile_rows} | {fmt(k, 1)} | {fmt(t, 1)} | "
          f"{statistics.median(t) / statistics.median(k):.2f}x ({verdict}) | {worst['kernel']} | {worst['torch']} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="timed rounds of alternating blocks")
    ap.add_argument("--steps", type=int, default=20, help="minibatch steps per block")
    ap.add_argument("--limit", type=int, default=120, help="seconds a shape's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    print("| M | species | TS | learner + ppo_loss + autograd.backward, µs per step | net(obs[index]) + ppo_loss + autograd.backward, µs per step | torch / kernel | kernel path against float64, worst tensor | torch path against float64, worst tensor |\n"
          "|---|---|---|---|---|---|---|---|", flush=True)
    return run_children(__file__, len(SHAPES), ["--reps", str(args.reps), "--steps", str(args.steps)], args.limit, lambda i: f"shape {SHAPES[i]}")


if __name__ == "__main__":
    sys.exit(main())
