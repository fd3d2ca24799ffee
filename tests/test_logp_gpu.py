"""`ppg_record_logp` (kernels ppg_logp_scan / ppg_logp_rows), `env.record_logp()`, `ObservationStore(logp=...)`,
`AgentTrajectories.record_policy()` / `behaviour()` / `scatter()` on the MI355X: the scenarios of tests/logp_cases.py, which
test_logp_emulated.py runs through the wave emulator with synthetic logits; a handle of 130 envs; the real policy
(`FusedPolicy.act(..., logits=bufs)`) against a twin's `want_logits=True`; the closed loop captured and replayed by
`GraphedCollector(..., logits=bufs)` against an eager twin."""
import numpy as np
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env
from predpreygrass_amd.red_queen import BatchedRedQueen
from predpreygrass_amd.trajectory import AgentTrajectories, GraphedCollector
from tests import logp_cases as cases
from tests import obs_store_cases as oc
from tests.record_cases import CFG_BASE, of, same_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 16


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


BK = cases.image_cases.Backend(make, make_rq, torch.cuda.synchronize)


@pytest.mark.parametrize("name", list(cases.ROLLOUT_ACTIONS))
def test_record_policy_over_a_rollout_against_numpy_on_gpu(name):
    cfg, kw, _ = cases.RECORDED[name]
    cases.rollout((make_rq if name == "gen2" else make)(cfg, B, **kw), name)


@pytest.mark.parametrize("A", [(9, 9), (1, 32), (32, 5)])
def test_record_logp_logit_and_action_values_on_gpu(A):
    cases.values(BK, A)


@pytest.mark.parametrize("batch", [1, 5, 67, 130])
def test_record_logp_batch_sizes_on_gpu(batch):
    cases.batch_size(BK, batch)


def test_record_logp_more_than_64_rows_per_species_on_gpu():
    cases.row_capacities(BK)


def test_record_logp_capacity_cut_inside_a_run_on_gpu():
    cases.capacity_cut(BK)


def test_record_logp_capacity_zero_on_gpu():
    cases.capacity_zero(BK)


def test_record_logp_ignores_corrupted_slot_words_on_gpu():
    cases.corrupted_slots(BK)


def test_record_logp_skipped_species_on_gpu():
    cases.skipped_species(BK)


def test_record_logp_device_step_index_on_gpu():
    cases.device_step_index(BK)


def test_record_logp_argument_checking_on_gpu():
    cases.argument_checking(BK, "cpu")


def test_record_logp_torch_equals_the_kernel_on_gpu():
    cases.torch_baseline(BK)


def test_scatter_is_the_inverse_of_flat_on_gpu():
    cases.scatter(make(CFG_BASE, B, prey_capacity=128, seed=3))


# ---- the real policy -------------------------------------------------------------------------------------------------------------

def policy(seed):
    """(FusedPolicy of two scaled default networks, (A_pred, A_prey))."""
    from predpreygrass_amd.policy import FusedPolicy
    from tests.test_policy import make_nets
    nets = make_nets(seed=seed)
    fused = FusedPolicy(nets[0], nets[1])
    A = (nets[0].n_actions, nets[1].n_actions)
    return fused, A


def buffers(env, A):
    return tuple(torch.zeros((env.batch_size * cap, a), dtype=torch.float32, device=DEV) for cap, a in zip((env.pred_capacity, env.prey_capacity), A))


def all_tensors(store):
    return {**oc.plain_tensors(store), **cases.policy_tensors(store)}


def test_the_real_policys_logits_reach_the_store():
    """act(sample=True, logits=bufs) + record_policy + step + record: the stored dist is, bit for bit, what `want_logits=True` returns
    on an identical twin; logp and entropy match the numpy reference on those logits at the stored actions; every sample of a step
    but the last has a finite logp."""
    T = 5
    env, twin = make(dict(config_env), B, seed=2), make(dict(config_env), B, seed=2)
    env.reset()
    twin.reset()
    fused, A = policy(seed=5)
    bufs = buffers(env, A)
    rows = (T * B * env.pred_capacity, T * B * env.prey_capacity)
    traj = AgentTrajectories(env, T, obs_rows=rows, logp=A, dist=True)
    ref, lref = oc.Ref(env, traj.store), cases.LogpRef(env, traj.store)
    with pytest.raises(ValueError):
        fused.act(env, sample=True, logits=(bufs[0][:-1], bufs[1]))
    with pytest.raises(ValueError):
        fused.act(env, sample=True, logits=(bufs[0].double(), bufs[1]))
    with pytest.raises(ValueError):
        fused.act(env, sample=True, logits=(bufs[0].cpu(), bufs[1]))
    for t in range(T):
        got = fused.act(env, sample=True, seed=100 + t, logits=bufs)
        assert got[0] is bufs[0] and got[1] is bufs[1]
        traj.record_policy(bufs)
        lg = fused.act(twin, sample=True, seed=100 + t, want_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(env.actions, twin.actions)
        if t > 0:
            lref.record(env, t - 1, lg, twin.actions, ref.slot)
        env.step(env.actions, auto_reset=True)
        twin.step(twin.actions, auto_reset=True)
        traj.record(env.actions)
        torch.cuda.synchronize()
        ref.record(env, t, env.actions)
    ref.check(traj.store, "real policy: the store's own tensors")
    lref.check(traj.store, "real policy")
    oc.nothing_dropped(ref, "real policy")
    for s in (0, 1):
        n, _, index, action = traj.samples(s)
        logp, entropy, dist = traj.behaviour(s)
        last = index >= (T - 1) * B * env.S
        assert n > 0 and bool(last.any()) and bool((~last).any())
        assert bool(torch.isfinite(logp[~last]).all()) and bool((logp[~last] <= 0).all()) and bool(torch.isnan(logp[last]).all())
        assert bool(((action[~last] >= 0) & (action[~last] < A[s])).all()) and bool((dist[~last] != 0).any())
        assert bool(torch.isfinite(entropy[~last]).all()) and bool((entropy[~last] >= 0).all())
    fused.close()


def test_graphed_collector_with_logits_matches_an_eager_twin():
    """The warm pass and T - 1 replays of act + record_policy + step + record + record_obs store what T eager iterations store on a
    twin: the five trajectory tensors and every tensor of the store, logp / entropy / dist included, bit for bit.  Past the horizon:
    the device word is T at the first further replay, which names step T - 1 -- that replay's record_policy() gives the LAST step's
    samples their policy (as one further act + record_policy() does on the twin) and touches nothing else; the replay after it
    changes nothing at all."""
    T = 10
    kw = dict(prey_capacity=128, seed=3)
    env, twin = make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw)
    env.reset()
    twin.reset()
    fused, A = policy(seed=8)
    bufs, twin_bufs = buffers(env, A), buffers(twin, A)
    seed, twin_seed = (torch.full((1,), 1000, dtype=torch.int64, device=DEV) for _ in range(2))

    def actor(e, b, key):
        def act():
            fused.act(e, sample=True, seed=key, logits=b)
            key.add_(1)
        return act
    act, twin_act = actor(env, bufs, seed), actor(twin, twin_bufs, twin_seed)
    rows = (T * B * 32, T * B * 96)
    traj = AgentTrajectories(env, T, step_on_device=True, obs_rows=rows, logp=A, dist=True)
    want = AgentTrajectories(twin, T, obs_rows=rows, logp=A, dist=True)
    loop = GraphedCollector(env, traj, act=act, logits=bufs)
    assert len(traj) == 1
    loop.replay(T - 1)
    for _ in range(T):
        twin_act()
        want.record_policy(twin_bufs)
        twin.step(twin.actions, auto_reset=True)
        want.record(twin.actions)
    torch.cuda.synchronize()
    assert len(traj) == T == len(want) and int(seed.item()) == 1000 + T

    def same_stores(tag):
        same_tensors(of(traj), of(want), tag)
        for (name, x), y in zip(all_tensors(traj.store).items(), all_tensors(want.store).values()):
            assert np.array_equal(oc.bits_of(x), oc.bits_of(y)), (tag, name)
    same_stores("warm pass + T - 1 replays")
    (sp, dp), (sq, dq) = traj.store.counts()
    assert sp > 0 and sq > 0 and dp == dq == 0
    for s in (0, 1):
        n, _, index, action = traj.samples(s)
        logp, entropy, dist = traj.behaviour(s)
        last = index >= (T - 1) * B * env.S
        assert bool(torch.isfinite(logp[~last]).all()) and bool(torch.isnan(logp[last]).all()) and bool(last.any()) and bool((~last).any())
        assert bool((action[~last] != oc.UNSET).all())
    before = {k: oc.bits_of(v) for k, v in all_tensors(traj.store).items()}
    loop.replay(1)    # past the horizon: the word is T = the last step + 1
    twin_act()
    want.record_policy(twin_bufs)
    torch.cuda.synchronize()
    assert len(traj) == T
    same_stores("the first replay past the horizon")
    for name, x in all_tensors(traj.store).items():
        now = oc.bits_of(x)
        if name[:-1] in ("logp", "entropy", "dist"):
            s = int(name[-1])
            n, _, index, _ = traj.samples(s)
            old = (index < (T - 1) * B * env.S).cpu().numpy()
            assert np.array_equal(now[:n][old], before[name][:n][old]) and np.array_equal(now[n:], before[name][n:]), name
            if name.startswith("logp"):
                assert np.isfinite(now[:n].view("<f4")).all()
        else:
            assert np.array_equal(now, before[name]), (name, "a replay past the horizon wrote")
    after = {k: oc.bits_of(v) for k, v in all_tensors(traj.store).items()}
    loop.replay(1)    # the word is T + 1: nothing
    torch.cuda.synchronize()
    assert len(traj) == T
    for name, x in all_tensors(traj.store).items():
        assert np.array_equal(oc.bits_of(x), after[name]), (name, "the second replay past the horizon wrote")
    same_tensors(of(traj), of(want), "two replays past the horizon")
    fused.close()
