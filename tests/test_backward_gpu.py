"""`ppg_backward` (kernel ppg_backward_rows), `env.backward()` and `AgentTrajectories.returns_and_gae()` on the MI355X: the scenarios
of tests/backward_cases.py, which test_backward_emulated.py runs through the wave emulator, at 64 envs; one launch of 4096 envs."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import backward_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64
ENVS = [0, 1, 17, 40, 63]


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


@pytest.mark.parametrize("T", cases.HORIZONS)
@pytest.mark.parametrize("cp,cq,cfg", cases.CAPACITIES, ids=[f"S{cp + cq}" for cp, cq, _ in cases.CAPACITIES])
def test_backward_synthetic_on_gpu(cp, cq, cfg, T):
    cases.synthetic_case(make, cp, cq, cfg, T, B)


def test_backward_full_batch_on_gpu():
    """4096 one-wave workgroups of S = 192: more than the wave slots of the GPU's first round of workgroups."""
    cp, cq, cfg = cases.CAPACITIES[1]
    cases.synthetic_case(make, cp, cq, cfg, 3, 4096)


def test_backward_recorded_base_family_on_gpu():
    env = make(cases.CFG_BASE, B, prey_capacity=128, seed=3)
    assert (env.pred_capacity, env.prey_capacity) == (64, 128)
    cases.recorded(env, envs=ENVS)


def test_backward_recorded_128_predator_rows_on_gpu():
    env = make(cases.CFG_P2, B, pred_capacity=128, prey_capacity=256, seed=7)
    cases.recorded(env, n_steps=60, envs=ENVS, need_pred_rows=64)


def test_backward_recorded_second_generation_on_gpu():
    cases.recorded(make_rq(cases.CFG_RQ, B, seed=4), envs=ENVS)


def test_backward_argument_checking_on_gpu():
    cases.argument_checking(make(cases.CFG_BASE, 3), "cpu")
