"""`ppg_net_forward` / `ppg_net_backward` (kernels ppg_net_fwd / ppg_net_bwd / ppg_net_reduce), `env.net_forward()` /
`env.net_backward()`, `trajectory.NetLearner` and `AgentTrajectories.forward()` on the MI355X: the scenarios of tests/net_cases.py, which
test_net_emulated.py runs through the wave emulator, and on top the reference's networks over a recorded rollout's store at M = 128
and 4096, automatic groups against one group, and forward + ppo_loss + backward captured in one graph."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from tests import net_cases as cases
from tests.record_cases import CFG_BASE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def env():
    return BatchedPredPreyGrass(CFG_BASE, batch_size=16, device=DEV, prey_capacity=128, seed=3)


@pytest.mark.parametrize("name", list(cases.NETWORKS))
def test_net_shapes_of_M_against_float64_autograd_on_gpu(env, name):
    cases.shapes(env, name)


@pytest.mark.parametrize("name", cases.SMALLEST + ("predator_r7_a9",))
def test_net_row_dtypes_on_gpu(env, name):
    cases.row_dtypes(env, name)


@pytest.mark.parametrize("name", cases.SMALLEST + ("prey_critic_r9", "r7_chw_hidden_256_64_a9", "r15_chw_c8_a9"))
def test_net_invalid_slots_are_selected_away_on_gpu(env, name):
    cases.invalid_slots(env, name)


def test_net_relu_at_zero_takes_gradient_zero_on_gpu(env):
    cases.relu_at_zero(env)


@pytest.mark.parametrize("name", ("r5_chw_c5_8_16_a9", "predator_r7_a9"))
def test_net_backward_is_deterministic_on_gpu(env, name):
    cases.determinism(env, name)
    cases.determinism(env, name, M=1500)


def test_net_untouched_memory_and_refused_calls_on_gpu(env):
    cases.untouched(env)


def test_net_learner_through_autograd_on_gpu(env):
    cases.autograd(env)


def test_net_ten_sgd_steps_follow_the_torch_path_on_gpu(env):
    cases.sgd_steps(env)


@pytest.mark.parametrize("M", (128, 4096))
def test_net_reference_networks_over_the_store_on_gpu(env, M):
    cases.store_minibatch(env, M)


def test_net_automatic_groups_against_one_group_on_gpu(env):
    cases.store_minibatch(env, 515, groups=(0, 1))


def test_net_forward_loss_and_backward_in_one_graph_on_gpu(env):
    cases.graphed(env)
