"""`ppg_record_obs` (kernels ppg_obs_scan / ppg_obs_rows), `env.record_obs()`, `trajectory.ObservationStore` and
`AgentTrajectories(obs_rows=...)` on the MI355X: the scenarios of tests/obs_store_cases.py, which test_obs_store_emulated.py runs
through the wave emulator; a handle of 130 envs; observation tensors on spread pages; a captured and replayed recorded step with a
store against an eager twin."""
import numpy as np
import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from predpreygrass_amd.trajectory import AgentTrajectories, GraphedCollector
from tests import image_cases
from tests import obs_store_cases as cases
from tests.record_cases import CFG_BASE, of, same_tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 16


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


BK = cases.image_cases.Backend(make, make_rq, torch.cuda.synchronize)


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_obs_against_numpy_on_gpu(name):
    cfg, kw, steps = cases.RECORDED[name]
    cases.against_numpy((make_rq if name == "gen2" else make)(cfg, B, **kw), name, steps)


@pytest.mark.parametrize("gid", list(cases.GEOMETRIES))
def test_record_obs_geometries_on_gpu(gid):
    cases.geometry(BK, gid)


def test_record_obs_into_a_store_that_is_not_word_aligned_on_gpu():
    cases.geometry_shifted_store(BK)


@pytest.mark.parametrize("batch", [1, 5, 67, 130])
def test_record_obs_batch_sizes_on_gpu(batch):
    cases.batch_size(BK, batch)


def test_record_obs_capacity_cut_inside_a_run_on_gpu():
    cases.capacity_cut(BK)


def test_record_obs_capacity_zero_on_gpu():
    cases.capacity_zero(BK)


def test_record_obs_device_step_index_on_gpu():
    cases.device_step_index(BK)


def test_record_obs_argument_checking_on_gpu():
    cases.argument_checking(BK, "cpu")


def test_agent_trajectories_with_a_store_on_gpu():
    kw = dict(prey_capacity=128, seed=3)
    cases.trajectories(make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw))


def test_record_obs_from_spread_observation_tensors():
    """obs_spread=32: the observation tensors live on physical pages picked from a stretch of device memory 32 times their size."""
    g = cases.GEOMETRIES["f32_3_7"]
    env = make(image_cases.geometry_config(g), 5, obs_dtype=torch.float32, pred_capacity=g.caps[0], prey_capacity=g.caps[1], seed=g.seed,
               obs_spread=32)
    assert env.obs_pred.data_ptr() % 16 == 0 and env.obs_prey.data_ptr() % 16 == 0
    env.reset()
    store = cases.GuardedStore(env, 4, (4 * 5 * 64, 4 * 5 * 64))
    ref, _ = cases.run(env, store, 4, torch.Generator().manual_seed(6), tag="spread pages")
    cases.nothing_dropped(ref, "spread pages")
    store.guards_untouched("spread pages")


def test_graphed_collector_with_a_store_matches_an_eager_twin():
    """The warm pass and T - 1 replays of actions + step + record + record_obs store what T eager steps store on a twin -- the five
    trajectory tensors and every tensor of the store, the actions included; replays past the horizon store nothing."""
    T = 10
    kw = dict(prey_capacity=128, seed=3)
    env, twin = make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw)
    env.reset()
    twin.reset()

    def filler(e):
        """Actions from torch ops on the current stream: a function of the env's call counter and ids, the same on both envs."""
        def act():
            torch.remainder(e.env_state[:, _abi.ENV_CALLS:_abi.ENV_CALLS + 1] + e.row_id, 5, out=e._act32)
            e.actions.copy_(e._act32)
        e._act32 = torch.zeros((B, e.S), dtype=torch.int32, device=DEV)
        return act
    act, twin_act = filler(env), filler(twin)
    rows = (T * B * 32, T * B * 96)
    traj = AgentTrajectories(env, T, step_on_device=True, obs_rows=rows)
    want = AgentTrajectories(twin, T, obs_rows=rows)
    loop = GraphedCollector(env, traj, act=act)
    assert len(traj) == 1
    loop.replay(T - 1)
    for _ in range(T):
        twin_act()
        twin.step(twin.actions, auto_reset=True)
        want.record(twin.actions)
    torch.cuda.synchronize()
    assert len(traj) == T == len(want)

    def same_stores(tag):
        same_tensors(of(traj), of(want), tag)
        for (name, x), y in zip(cases.plain_tensors(traj.store).items(), cases.plain_tensors(want.store).values()):
            assert np.array_equal(cases.bits_of(x), cases.bits_of(y)), (tag, name)
    same_stores("warm pass + T - 1 replays")
    (sp, dp), (sq, dq) = traj.store.counts()
    assert sp > 0 and sq > 0 and dp == dq == 0
    for s in (0, 1):
        n, obs, index, action = traj.samples(s)
        assert bool(((action >= 0) & (action < 5)).any()) and bool((action[index >= (T - 1) * B * env.S] == cases.UNSET).all())
        assert bool((obs != 0).any())
    loop.replay(2)   # past the horizon: the env steps on, nothing is stored, the cursor stays
    torch.cuda.synchronize()
    assert len(traj) == T
    same_stores("two replays past the horizon")
