"""`ppg_record` (kernel ppg_record_rows), `env.record()`, `AgentTrajectories.record()` and `trajectory.GraphedCollector` on the
MI355X: the scenarios of tests/record_cases.py, which test_record_emulated.py runs through the wave emulator, at 64 envs; one launch
of 4096 envs; a captured and replayed recorded step against an eager twin."""
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from predpreygrass_amd.trajectory import AgentTrajectories, GraphedCollector
from tests import record_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64
ENVS = [0, 1, 17, 40, 63]


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


def make_named(name, batch=B):
    cfg, kw, steps = cases.RECORDED[name]
    return (make_rq if name == "gen2" else make)(cfg, batch, **kw), steps


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_against_numpy_on_gpu(name):
    env, steps = make_named(name)
    cases.against_numpy(env, steps, envs=ENVS)


@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_record_against_numpy_every_row_register_count_on_gpu(cp, cq, cfg):
    cases.against_numpy_capacity(make, cp, cq, cfg, B, envs=ENVS)


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_against_record_torch_on_a_twin_on_gpu(name):
    (env, steps), (twin, _) = make_named(name), make_named(name)
    cases.against_torch(env, twin, steps)


def test_record_full_batch_on_gpu():
    """4096 one-wave workgroups of S = 192: more than the wave slots of the GPU's first round of workgroups."""
    env, twin = cases.twins(make, cases.CFG_BASE, 4096, prey_capacity=128, seed=3)
    assert env.S == 192
    env.reset()
    twin.reset()
    a, b = AgentTrajectories(env, 3), AgentTrajectories(twin, 3)
    for _ in range(3):
        env.step(random_actions=True, auto_reset=True)
        twin.step(random_actions=True, auto_reset=True)
        a.record()
        b.record_torch()
    cases.same_tensors(cases.of(a), cases.of(b), "4096 envs")
    assert bool((a.next_row >= 0).any())


def test_record_returns_the_link_maps_on_gpu():
    cases.returned_maps_are_the_links(*cases.twins(make, cases.CFG_BASE, B, seed=2))


@pytest.mark.parametrize("family", ["base", "p128"])
def test_record_writes_exactly_the_documented_elements_on_gpu(family):
    cases.exactly_the_documented_elements(make_named(family)[0])


def test_record_mixing_and_invalidation_on_gpu():
    cases.mixing_and_invalidation(make(cases.CFG_BASE, B, seed=1))
    cases.mixing_and_invalidation(make_rq(cases.CFG_RQ, B, seed=1))


def test_record_device_step_index_on_gpu():
    cases.device_step_index(*cases.twins(make, cases.CFG_BASE, B, prey_capacity=128, seed=3))


def test_record_argument_checking_on_gpu():
    cases.argument_checking(make(cases.CFG_BASE, 3), "cpu")


@pytest.mark.parametrize("with_act", [False, True], ids=["random_actions", "act_callable"])
def test_graphed_collector_matches_an_eager_twin(with_act):
    """The warm pass and T - 1 replays record what T eager steps record on a twin; replays past the horizon store nothing; after
    env.reset() the documented sequence (clear, one eager step + record, replays) matches the twin again."""
    T = 12
    env, twin = cases.twins(make, cases.CFG_BASE, B, prey_capacity=128, seed=3)
    env.reset()
    twin.reset()

    def filler(e):
        """Actions from a torch op on the current stream: a function of the env's own state, so both envs draw the same ones."""
        def act():
            torch.remainder(e.env_state[:, cases._abi.ENV_CALLS:cases._abi.ENV_CALLS + 1] + e.row_id, 5, out=e._act32)
            e.actions.copy_(e._act32)
        e._act32 = torch.zeros((B, e.S), dtype=torch.int32, device=DEV)
        return act
    act, twin_act = (filler(env), filler(twin)) if with_act else (None, None)

    def eager_step():
        if with_act:
            twin_act()
            twin.step(twin.actions, auto_reset=True)
        else:
            twin.step(random_actions=True, auto_reset=True)

    traj, want = AgentTrajectories(env, T, step_on_device=True), AgentTrajectories(twin, T)
    with pytest.raises(ValueError):
        GraphedCollector(twin, want)   # (the step index has to live on the device)
    loop = GraphedCollector(env, traj, act=act)
    assert len(traj) == 1
    loop.replay(T - 1)
    for _ in range(T):
        eager_step()
        want.record_torch()
    torch.cuda.synchronize()
    assert len(traj) == T == len(want)
    cases.same_tensors(cases.of(traj), cases.of(want), "warm pass + T - 1 replays")
    assert bool((traj.next_row >= 0).any()) and bool(traj.in_use.any())
    loop.replay(2)   # past the horizon: the env steps on, nothing is stored
    for _ in range(2):
        eager_step()
    torch.cuda.synchronize()
    assert len(traj) == T
    cases.same_tensors(cases.of(traj), cases.of(want), "two replays past the horizon")
    # after a reset: clear(), one eager step + record (it takes the fresh snapshot), then replays
    env.reset()
    twin.reset()
    traj.clear()
    want.clear()
    if with_act:
        act()
        env.step(env.actions, auto_reset=True)
    else:
        env.step(random_actions=True, auto_reset=True)
    traj.record()
    loop.replay(T - 1)
    for _ in range(T):
        eager_step()
        want.record_torch()
    torch.cuda.synchronize()
    assert len(traj) == T
    cases.same_tensors(cases.of(traj), cases.of(want), "after reset()")
    assert torch.equal(env.row_id, twin.row_id) and torch.equal(env.env_state, twin.env_state)
