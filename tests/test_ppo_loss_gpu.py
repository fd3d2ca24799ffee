"""`ppg_ppo_loss` (kernels ppg_ppo_count / ppg_ppo_rows), `env.ppo_loss()`, `AgentTrajectories.ppo_loss()` / `ppo_loss_torch()` /
`advantage_norm()` and `trajectory.ppo_loss_function()` on the MI355X: the scenarios of tests/ppo_loss_cases.py, which
test_ppo_loss_emulated.py runs through the wave emulator, and a minibatch of 300 chunks, in which hundreds of workgroups read every
count."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import ppo_loss_cases as cases
from tests.record_cases import CFG_BASE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 16


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


@pytest.fixture(scope="module")
def env():
    return make(CFG_BASE, 3, prey_capacity=128, seed=3)


@pytest.mark.parametrize("M", cases.SHAPES_M)
def test_ppo_loss_shapes_and_options_against_numpy_on_gpu(env, M):
    cases.shapes(env, M)


def test_ppo_loss_of_300_chunks_on_gpu(env):
    cases.large(env)


def test_ppo_loss_invalid_samples_are_selected_away_on_gpu(env):
    cases.invalid_samples(env)


def test_ppo_loss_clip_branches_masked_actions_and_divergence_on_gpu(env):
    cases.clip_branches(env)


def test_ppo_loss_of_identical_logits_on_gpu(env):
    cases.exact_identity(env)


def test_ppo_loss_untouched_memory_and_refused_calls_on_gpu(env):
    cases.untouched(env, "cpu")


@pytest.mark.parametrize("name", list(cases.logp_cases.ROLLOUT_ACTIONS))
def test_ppo_loss_over_a_recorded_rollout_on_gpu(name):
    cfg, kw, _ = cases.RECORDED[name]
    cases.recorded((make_rq if name == "gen2" else make)(cfg, B, **kw), name)
