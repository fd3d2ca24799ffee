"""`FusedPolicy.update()` / `ppg_policy_update` (kernel ppg_policy_repack) on the MI355X: the weights an update gathers from float32
parameters in device memory are, to the bit, the weights a fresh `FusedPolicy` of those networks uploads -- judged by what the policy
kernels compute from them, in every kernel family --; one species alone; captured loops keep running and act with the new weights; the
update itself captured, reading the parameters in place at every replay; staging of parameters that cannot be read in place; and the
refusals, all of them host checks in front of any launch."""
import ctypes

import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass, capture_graph
from predpreygrass_amd.config import config_env
from predpreygrass_amd.policy import FusedPolicy, GraphedPolicyStep, PolicyNet
from tests.test_policy import make_nets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 8
STATE = ("row_xy", "row_energy", "row_id", "row_flags", "row_reward", "row_cumrew", "env_state", "grass_energy", "obs_pred", "obs_prey", "actions")


def nets_on_device(seed, Rp=7, Rq=9, **kw):
    return [n.to(DEV) for n in make_nets(Rp, Rq, seed=seed, **kw)]


def small_env(Rp=7, Rq=9, steps=12, seed=4, **kw):
    env = BatchedPredPreyGrass({**config_env, "predator_obs_range": Rp, "prey_obs_range": Rq}, batch_size=B, device=DEV, seed=seed, **kw)
    env.reset()
    for _ in range(steps):
        env.step(random_actions=True, auto_reset=True)
    return env


def observe(fused, env):
    """(logits_pred, logits_prey, greedy actions, sampled actions) of one env state."""
    lg = fused.act(env, want_logits=True)
    greedy = env.actions.clone()
    fused.act(env, sample=True, seed=5)
    torch.cuda.synchronize()
    return [None if x is None else x.clone() for x in lg] + [greedy, env.actions.clone()]


def same(got, want):
    return all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("family,Rp,Rq,kw", [
    ("pipeline", 7, 9, {}),
    ("one-role direct", 7, 9, {}),
    ("more than three convolutions", 7, 9, dict(conv_channels=(16, 32, 64, 64))),
    ("FC chain 256-256", 7, 9, dict(head_hiddens=(256, 256))),
    ("FC chain 96-160", 7, 9, dict(head_hiddens=(96, 160))),
    ("chw, nchw flatten", 7, 9, dict(layout="chw")),
], ids=lambda v: v.replace(" ", "-").replace(",", "") if isinstance(v, str) else None)
def test_update_equals_create(family, Rp, Rq, kw, monkeypatch):
    """FusedPolicy(A).update(B) acts exactly like FusedPolicy(B) -- logits, greedy actions, sampled actions with the same seed -- and
    not like A."""
    if family == "one-role direct":
        monkeypatch.setenv("PPG_POLICY_PIPE", "0")
    A, Bn = nets_on_device(71, Rp, Rq, **kw), nets_on_device(72, Rp, Rq, **kw)
    env = small_env(Rp, Rq)
    fused = FusedPolicy(A[0], A[1])
    old = observe(fused, env)
    assert fused.update(Bn[0], Bn[1]) is fused and fused.nets == (Bn[0], Bn[1]) and fused._staged == [[], []]
    got = observe(fused, env)
    fresh = FusedPolicy(Bn[0], Bn[1])
    want = observe(fresh, env)
    assert same(got, want)
    assert not torch.equal(got[0], old[0]) and not torch.equal(got[1], old[1]) and bool(got[0].abs().sum() > 0) and bool(got[1].abs().sum() > 0)
    fused.update(A[0], A[1])                      # and back: nothing of B is left
    assert same(observe(fused, env), old)
    fused.close()
    fresh.close()


def test_update_of_one_species_leaves_the_other_alone():
    A, Bn = nets_on_device(73), nets_on_device(74)
    env = small_env()
    fused = FusedPolicy(A[0], A[1])
    old = observe(fused, env)
    fused.update(prey_net=Bn[1])
    assert fused.nets == (A[0], Bn[1])
    got = observe(fused, env)
    mixed = FusedPolicy(A[0], Bn[1])
    assert torch.equal(got[0], old[0]) and not torch.equal(got[1], old[1]) and same(got, observe(mixed, env))
    fused.update(pred_net=Bn[0])
    both = FusedPolicy(Bn[0], Bn[1])
    assert same(observe(fused, env), observe(both, env))
    for f in (fused, mixed, both):
        f.close()


def test_a_captured_policy_step_acts_with_the_new_weights_after_an_update():
    """GraphedPolicyStep captured with A: warm pass + 2 replays, update(B), 3 replays == an eager loop that swaps to a fresh
    FusedPolicy(B) at step 3 (same keys); a loop that keeps A ends elsewhere."""
    A, Bn = nets_on_device(75), nets_on_device(76)
    a, b, c = (small_env(obs_dtype=torch.bfloat16, seed=21) for _ in range(3))
    fused, keep_a, fresh_b = FusedPolicy(A[0], A[1]), FusedPolicy(A[0], A[1]), FusedPolicy(Bn[0], Bn[1])
    loop = GraphedPolicyStep(fused, a, seed=1000)        # (its warm pass is step 0)
    loop.replay(2)
    fused.update(Bn[0], Bn[1])
    loop.replay(3)
    for t in range(6):
        (keep_a if t < 3 else fresh_b).act(b, sample=True, seed=1000 + t)
        b.step(b.actions, auto_reset=True)
        keep_a.act(c, sample=True, seed=1000 + t)
        c.step(c.actions, auto_reset=True)
    torch.cuda.synchronize()
    assert int(loop.seed.item()) == 1006
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.actions, c.actions)
    for f in (fused, keep_a, fresh_b):
        f.close()


def test_a_captured_collector_acts_with_the_new_weights_after_an_update():
    """The same through trajectory.GraphedCollector with logits=bufs: the store's log-probabilities (and the rest of the behaviour
    policy's tensors) equal an eager twin's that swaps to a fresh FusedPolicy(B) at step 3."""
    from predpreygrass_amd.trajectory import AgentTrajectories, GraphedCollector
    from tests import obs_store_cases as oc
    from tests.test_logp_gpu import buffers
    T = 6
    A, Bn = nets_on_device(77), nets_on_device(78)
    env, twin = (BatchedPredPreyGrass(dict(config_env), batch_size=B, device=DEV, seed=3) for _ in range(2))
    env.reset()
    twin.reset()
    fused, keep_a, fresh_b = FusedPolicy(A[0], A[1]), FusedPolicy(A[0], A[1]), FusedPolicy(Bn[0], Bn[1])
    n_act = (A[0].n_actions, A[1].n_actions)
    bufs, twin_bufs = buffers(env, n_act), buffers(twin, n_act)
    seed, twin_seed = (torch.full((1,), 1000, dtype=torch.int64, device=DEV) for _ in range(2))

    def act():
        fused.act(env, sample=True, seed=seed, logits=bufs)
        seed.add_(1)
    rows = (T * B * env.pred_capacity, T * B * env.prey_capacity)
    traj = AgentTrajectories(env, T, step_on_device=True, obs_rows=rows, logp=n_act, dist=True)
    want = AgentTrajectories(twin, T, obs_rows=rows, logp=n_act, dist=True)
    loop = GraphedCollector(env, traj, act=act, logits=bufs)
    loop.replay(2)
    fused.update(Bn[0], Bn[1])
    loop.replay(3)
    for t in range(T):
        (keep_a if t < 3 else fresh_b).act(twin, sample=True, seed=twin_seed, logits=twin_bufs)
        twin_seed.add_(1)
        want.record_policy(twin_bufs)
        twin.step(twin.actions, auto_reset=True)
        want.record(twin.actions)
    torch.cuda.synchronize()
    assert len(traj) == T == len(want)
    for s in (0, 1):
        for name in ("logp", "entropy", "dist", "action"):
            x, y = getattr(traj.store, name)[s], getattr(want.store, name)[s]
            assert (oc.bits_of(x) == oc.bits_of(y)).all(), (name, s)
        assert bool(torch.isfinite(traj.store.logp[s]).any())
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    for f in (fused, keep_a, fresh_b):
        f.close()


def test_a_captured_update_reads_the_parameters_in_place_at_every_replay():
    """[update; act] captured once: after the nets' parameters change IN PLACE (what an optimiser step does) a replay alone -- no host
    code of the policy -- acts with the changed parameters: the learner-to-actor hand-over with no host in it."""
    nets = nets_on_device(79)
    env = small_env()
    fused = FusedPolicy(nets[0], nets[1])
    bufs = tuple(torch.zeros((B * cap, 9), dtype=torch.float32, device=DEV) for cap in (env.pred_capacity, env.prey_capacity))
    fused.update(nets[0], nets[1])               # the one eager update: it allocates the repack maps

    def body():
        fused.update(nets[0], nets[1])
        fused.act(env, logits=bufs)
    graph = capture_graph(env.device, body)
    torch.cuda.synchronize()
    before = [x.clone() for x in bufs]
    gen = torch.Generator(DEV).manual_seed(1)
    with torch.no_grad():
        for net in nets:
            for p in net.parameters():
                p.add_(0.01 * torch.randn(p.shape, device=DEV, generator=gen))
    graph.replay()
    torch.cuda.synchronize()
    fresh = FusedPolicy(nets[0], nets[1])
    want = fresh.act(env, want_logits=True)
    torch.cuda.synchronize()
    for t in range(2):
        assert torch.equal(bufs[t], want[t]) and not torch.equal(bufs[t], before[t])
    fused.close()
    fresh.close()


def test_update_stages_parameters_it_cannot_read_in_place():
    """CPU nets, float64 nets and non-contiguous parameters give the bytes of float32 device nets."""
    A, Bn = nets_on_device(80), make_nets(seed=81)          # Bn on the CPU
    env = small_env()
    fused = FusedPolicy(A[0], A[1])
    fused.update(Bn[0], Bn[1])
    assert [len(s) for s in fused._staged] == [len(list(n.parameters())) for n in Bn]
    got = observe(fused, env)
    fresh = FusedPolicy(Bn[0], Bn[1])
    want = observe(fresh, env)
    assert same(got, want)
    fused.update(A[0], A[1])
    assert fused._staged == [[], []] and not same(observe(fused, env), want)
    import copy
    doubles = [copy.deepcopy(n).double().to(DEV) for n in Bn]
    fused.update(doubles[0], doubles[1])
    assert same(observe(fused, env), want)
    fused.update(A[0], A[1])
    strided = [copy.deepcopy(n).to(DEV) for n in Bn]
    with torch.no_grad():
        for n in strided:                                    # the same values behind a transposed (non-contiguous) weight
            w = n.fc[-1].weight
            n.fc[-1].weight = torch.nn.Parameter(w.t().contiguous().t())
            assert not n.fc[-1].weight.is_contiguous()
    fused.update(strided[0], strided[1])
    assert [len(s) for s in fused._staged] == [1, 1] and same(observe(fused, env), want)
    fused.close()
    assert fused._staged == [[], []]
    fresh.close()


def test_update_refuses_what_it_cannot_load():
    """Another architecture, a net for a species created as None, a closed policy: ValueError from the host checks, nothing launched,
    the logits unchanged."""
    A = nets_on_device(82)
    env = small_env()
    fused = FusedPolicy(A[0], A[1])
    old = observe(fused, env)
    other_range = PolicyNet(9).to(DEV)                                           # the predators read 7 x 7 windows
    deeper_head = PolicyNet(7, head_hiddens=(256,)).to(DEV)
    other_channels = PolicyNet(7, conv_channels=(16, 32, 48)).to(DEV)
    other_prey = nets_on_device(83)[1]
    for bad in (other_range, deeper_head, other_channels):
        with pytest.raises(ValueError):
            fused.update(pred_net=bad)
        with pytest.raises(ValueError):
            fused.update(bad, other_prey)                                        # nothing of a refused call is applied: not the good prey net either
    assert fused.nets == (A[0], A[1]) and same(observe(fused, env), old)
    prey_only = FusedPolicy(None, A[1])
    with pytest.raises(ValueError):
        prey_only.update(pred_net=A[0])
    alone = observe(prey_only, env)
    prey_only.update(prey_net=A[1])
    assert prey_only.nets == (None, A[1]) and same(observe(prey_only, env), alone)
    prey_only.close()
    # the library's own shape check (behind the Python one) names the field
    sp = fused._spec(other_range, lambda p: p.data_ptr())
    assert fused._lib.ppg_policy_update(fused._handles[0], ctypes.byref(sp), None) == -1
    assert b"obs_range is 9" in fused._lib.ppg_policy_last_error(fused._handles[0])
    sp = fused._spec(A[0], lambda p: p.data_ptr())
    sp.fc_b[0] = None
    assert fused._lib.ppg_policy_update(fused._handles[0], ctypes.byref(sp), None) == -1
    assert b"NULL" in fused._lib.ppg_policy_last_error(fused._handles[0])
    assert same(observe(fused, env), old)
    fused.close()
    with pytest.raises(ValueError):
        fused.update(A[0], A[1])
