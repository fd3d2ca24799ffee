"""`ppg_backward` (csrc/ppg_backward.h), `env.backward()` and `AgentTrajectories.returns_and_gae()` through the kernel source
compiled for the CPU wave emulator: synthetic trajectories at every row-register count and recorded ones, bit for bit against the
numpy recursion of tests/backward_cases.py.  The same scenarios run on the GPU in test_backward_gpu.py."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import backward_cases as cases
from tests.emu_backend import library

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


@pytest.mark.parametrize("T", cases.HORIZONS)
@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_backward_synthetic(cp, cq, cfg, T):
    cases.synthetic_case(make, cp, cq, cfg, T, B)


def test_backward_next_row_outside_the_rows_means_no_successor():
    cases.out_of_range_links(make)


def test_backward_recorded_base_family():
    env = make(cases.CFG_BASE, B, prey_capacity=128, seed=3)
    assert (env.pred_capacity, env.prey_capacity) == (64, 128)
    cases.recorded(env)


def test_backward_recorded_128_predator_rows():
    env = make(cases.CFG_P2, B, pred_capacity=128, prey_capacity=256, seed=7)
    cases.recorded(env, n_steps=60, need_pred_rows=64)


def test_backward_recorded_second_generation():
    cases.recorded(make_rq(cases.CFG_RQ, B, seed=4))


def test_backward_argument_checking():
    cases.argument_checking(make(cases.CFG_BASE, B), "meta")
