"""`ppg_ppo_loss` (csrc/ppg_ppo.h), `env.ppo_loss()`, `AgentTrajectories.ppo_loss()` / `ppo_loss_torch()` / `advantage_norm()` and
`trajectory.ppo_loss_function()` through the kernel source compiled for the CPU wave emulator: the scenarios of tests/ppo_loss_cases.py.
The same scenarios run on the GPU in test_ppo_loss_gpu.py, which adds a minibatch of 300 chunks."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import ppo_loss_cases as cases
from tests.emu_backend import library
from tests.record_cases import CFG_BASE

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


@pytest.fixture(scope="module")
def env():
    return make(CFG_BASE, B, prey_capacity=128, seed=3)


def test_the_fixed_seeds_keep_every_branch_decision_clear_of_its_boundary():
    cases.margins_hold()


@pytest.mark.parametrize("M", cases.SHAPES_M)
def test_ppo_loss_shapes_and_options_against_numpy(env, M):
    cases.shapes(env, M)


def test_ppo_loss_invalid_samples_are_selected_away(env):
    cases.invalid_samples(env)


def test_ppo_loss_clip_branches_masked_actions_and_divergence(env):
    cases.clip_branches(env)


def test_ppo_loss_of_identical_logits(env):
    cases.exact_identity(env)


def test_ppo_loss_untouched_memory_and_refused_calls(env):
    cases.untouched(env, "meta")


@pytest.mark.parametrize("name", list(cases.logp_cases.ROLLOUT_ACTIONS))
def test_ppo_loss_over_a_recorded_rollout(name):
    cfg, kw, _ = cases.RECORDED[name]
    cases.recorded((make_rq if name == "gen2" else make)(cfg, B, **kw), name)
