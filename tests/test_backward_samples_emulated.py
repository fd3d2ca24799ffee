"""`ppg_backward_samples` (csrc/ppg_backward.h), `env.backward_samples()` and `AgentTrajectories.targets()` through the kernel source
compiled for the CPU wave emulator: synthetic trajectories and slot tables at every row-register count and recorded ones, bit for bit
against the numpy reference of tests/backward_samples_cases.py.  The same scenarios run on the GPU in test_backward_samples_gpu.py."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import backward_samples_cases as cases
from tests.emu_backend import library
from tests.link_cases import CFG_BASE, CFG_P2, CFG_RQ

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


@pytest.mark.parametrize("T", cases.HORIZONS)
@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_backward_samples_synthetic(cp, cq, cfg, T):
    cases.synthetic_case(make, cp, cq, cfg, T, B)


def test_backward_samples_next_row_outside_the_rows_means_no_successor():
    cases.out_of_range_links(make)


def test_backward_samples_recorded_base_family():
    cases.recorded(lambda: make(CFG_BASE, B, prey_capacity=128, seed=3))


def test_backward_samples_recorded_128_predator_rows():
    # (two envs: the emulator steps them 2 x 60 times, once per step-index placement)
    cases.recorded(lambda: make(CFG_P2, 2, pred_capacity=128, prey_capacity=256, seed=7), n_steps=60, need_pred_rows=64)


def test_backward_samples_recorded_second_generation():
    cases.recorded(lambda: make_rq(CFG_RQ, B, seed=4))


def test_backward_samples_argument_checking():
    cases.argument_checking(make(CFG_BASE, B), "meta")
