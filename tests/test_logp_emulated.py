"""`ppg_record_logp` (csrc/ppg_logp.h), `env.record_logp()`, `ObservationStore(logp=...)`, `AgentTrajectories.record_policy()` /
`behaviour()` / `scatter()` through the kernel source compiled for the CPU wave emulator: the scenarios of tests/logp_cases.py, with
synthetic logits.  The same scenarios run on the GPU in test_logp_gpu.py, which adds the real policy and the captured loop."""
import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import logp_cases as cases
from tests.emu_backend import library

B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


BK = cases.image_cases.Backend(make, make_rq, lambda: None)


@pytest.mark.parametrize("name", list(cases.ROLLOUT_ACTIONS))
def test_record_policy_over_a_rollout_against_numpy(name):
    cfg, kw, _ = cases.RECORDED[name]
    cases.rollout((make_rq if name == "gen2" else make)(cfg, B, **kw), name)


@pytest.mark.parametrize("A", [(9, 9), (1, 32), (32, 5)])
def test_record_logp_logit_and_action_values(A):
    cases.values(BK, A)


@pytest.mark.parametrize("batch", [1, 5, 67])
def test_record_logp_batch_sizes(batch):
    cases.batch_size(BK, batch)


def test_record_logp_more_than_64_rows_per_species():
    cases.row_capacities(BK)


def test_record_logp_capacity_cut_inside_a_run():
    cases.capacity_cut(BK)


def test_record_logp_capacity_zero():
    cases.capacity_zero(BK)


def test_record_logp_ignores_corrupted_slot_words():
    cases.corrupted_slots(BK)


def test_record_logp_skipped_species():
    cases.skipped_species(BK)


def test_record_logp_device_step_index():
    cases.device_step_index(BK)


def test_record_logp_argument_checking():
    cases.argument_checking(BK, "meta")


def test_record_logp_torch_equals_the_kernel():
    cases.torch_baseline(BK)


def test_scatter_is_the_inverse_of_flat():
    from tests.record_cases import CFG_BASE
    cases.scatter(make(CFG_BASE, B, prey_capacity=128, seed=3))
