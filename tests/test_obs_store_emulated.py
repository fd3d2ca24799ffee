"""`ppg_record_obs` (csrc/ppg_obs_store.h), `env.record_obs()`, `trajectory.ObservationStore` and `AgentTrajectories(obs_rows=...)`
through the kernel source compiled for the CPU wave emulator: the scenarios of tests/obs_store_cases.py.  The same scenarios run on
the GPU in test_obs_store_gpu.py."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import obs_store_cases as cases
from tests.emu_backend import library

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


BK = cases.image_cases.Backend(make, make_rq, lambda: None)


def make_named(name):
    cfg, kw, steps = cases.RECORDED[name]
    return (make_rq if name == "gen2" else make)(cfg, B, **kw), steps


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_obs_against_numpy(name):
    env, steps = make_named(name)
    cases.against_numpy(env, name, steps)


@pytest.mark.parametrize("gid", list(cases.GEOMETRIES))
def test_record_obs_geometries(gid):
    cases.geometry(BK, gid)


def test_record_obs_into_a_store_that_is_not_word_aligned():
    cases.geometry_shifted_store(BK)


@pytest.mark.parametrize("batch", [1, 5, 67])
def test_record_obs_batch_sizes(batch):
    cases.batch_size(BK, batch)


def test_record_obs_capacity_cut_inside_a_run():
    cases.capacity_cut(BK)


def test_record_obs_capacity_zero():
    cases.capacity_zero(BK)


def test_record_obs_device_step_index():
    cases.device_step_index(BK)


def test_record_obs_argument_checking():
    cases.argument_checking(BK, "meta")


def test_agent_trajectories_with_a_store():
    from tests.record_cases import CFG_BASE
    kw = dict(prey_capacity=128, seed=3)
    cases.trajectories(make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw), make(CFG_BASE, B, **kw))
