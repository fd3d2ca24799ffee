"""`ppg_net_forward` / `ppg_net_backward` (csrc/ppg_net.h), `env.net_forward()` / `env.net_backward()`, `trajectory.NetLearner` and
`AgentTrajectories.forward()` through the kernel source compiled for the CPU wave emulator: the scenarios of tests/net_cases.py.
The same scenarios run on the GPU in test_net_gpu.py, which adds the store at M = 128 and 4096 and the captured graph."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from tests import net_cases as cases
from tests.emu_backend import library
from tests.record_cases import CFG_BASE


@pytest.fixture(scope="module")
def env():
    return BatchedPredPreyGrass(CFG_BASE, batch_size=3, _library=library(), prey_capacity=128, seed=3)


def test_the_inputs_keep_every_reference_tensor_away_from_zero_and_torch_float32_within_1e_5(env):
    cases.inputs_hold(env)


@pytest.mark.parametrize("name", list(cases.NETWORKS))
def test_net_shapes_of_M_against_float64_autograd(env, name):
    cases.shapes(env, name)


@pytest.mark.parametrize("name", cases.SMALLEST + ("predator_r7_a9",))
def test_net_row_dtypes(env, name):
    cases.row_dtypes(env, name)


@pytest.mark.parametrize("name", cases.SMALLEST + ("prey_critic_r9", "r7_chw_hidden_256_64_a9", "r15_chw_c8_a9"))
def test_net_invalid_slots_are_selected_away(env, name):
    cases.invalid_slots(env, name)


def test_net_relu_at_zero_takes_gradient_zero(env):
    cases.relu_at_zero(env)


@pytest.mark.parametrize("name", ("r5_chw_c5_8_16_a9", "predator_r7_a9"))
def test_net_backward_is_deterministic(env, name):
    cases.determinism(env, name)


def test_net_untouched_memory_and_refused_calls(env):
    cases.untouched(env)


def test_net_learner_through_autograd(env):
    cases.autograd(env, M=16, conv=(8, 16))


def test_net_ten_sgd_steps_follow_the_torch_path(env):
    cases.sgd_steps(env)
