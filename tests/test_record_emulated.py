"""`ppg_record` (csrc/ppg_record.h), `env.record()` and `AgentTrajectories.record()` through the kernel source compiled for the CPU
wave emulator: the scenarios of tests/record_cases.py at 3 envs.  The same scenarios run on the GPU in test_record_gpu.py."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import record_cases as cases
from tests.emu_backend import library

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


def make_named(name):
    cfg, kw, steps = cases.RECORDED[name]
    return (make_rq if name == "gen2" else make)(cfg, B, **kw), steps


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_against_numpy(name):
    env, steps = make_named(name)
    cases.against_numpy(env, steps)


@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_record_against_numpy_every_row_register_count(cp, cq, cfg):
    cases.against_numpy_capacity(make, cp, cq, cfg, B)


@pytest.mark.parametrize("name", list(cases.RECORDED))
def test_record_against_record_torch_on_a_twin(name):
    (env, steps), (twin, _) = make_named(name), make_named(name)
    cases.against_torch(env, twin, steps)


def test_record_returns_the_link_maps():
    cases.returned_maps_are_the_links(*cases.twins(make, cases.CFG_BASE, B, seed=2))


@pytest.mark.parametrize("family", ["base", "p128"])
def test_record_writes_exactly_the_documented_elements(family):
    cases.exactly_the_documented_elements(make_named(family)[0])


def test_record_mixing_and_invalidation():
    cases.mixing_and_invalidation(make(cases.CFG_BASE, B, seed=1))
    cases.mixing_and_invalidation(make_rq(cases.CFG_RQ, B, seed=1))


def test_record_device_step_index():
    cases.device_step_index(*cases.twins(make, cases.CFG_BASE, B, prey_capacity=128, seed=3))


def test_record_argument_checking():
    cases.argument_checking(make(cases.CFG_BASE, B), "meta")
