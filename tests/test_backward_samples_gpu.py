"""`ppg_backward_samples` (kernel ppg_backward_samples_rows), `env.backward_samples()` and `AgentTrajectories.targets()` on the MI355X:
the scenarios of tests/backward_samples_cases.py, which test_backward_samples_emulated.py runs through the wave emulator, at 64 envs;
one launch of 4096 envs."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import backward_samples_cases as cases
from tests.link_cases import CFG_BASE, CFG_P2, CFG_RQ

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


@pytest.mark.parametrize("T", cases.HORIZONS)
@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_backward_samples_synthetic_on_gpu(cp, cq, cfg, T):
    cases.synthetic_case(make, cp, cq, cfg, T, B)


def test_backward_samples_full_batch_on_gpu():
    """4096 one-wave workgroups of S = 192: more than the wave slots of the GPU's first round of workgroups."""
    cp, cq, cfg = cases.CAPACITIES[1]
    cases.synthetic_case(make, cp, cq, cfg, 3, 4096)


def test_backward_samples_next_row_outside_the_rows_means_no_successor_on_gpu():
    cases.out_of_range_links(make)


def test_backward_samples_recorded_base_family_on_gpu():
    cases.recorded(lambda: make(CFG_BASE, B, prey_capacity=128, seed=3))


def test_backward_samples_recorded_128_predator_rows_on_gpu():
    cases.recorded(lambda: make(CFG_P2, B, pred_capacity=128, prey_capacity=256, seed=7), n_steps=60, need_pred_rows=64)


def test_backward_samples_recorded_second_generation_on_gpu():
    cases.recorded(lambda: make_rq(CFG_RQ, B, seed=4))


def test_backward_samples_argument_checking_on_gpu():
    cases.argument_checking(make(CFG_BASE, 3), "cpu")
