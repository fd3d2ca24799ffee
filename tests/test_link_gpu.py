"""`ppg_link` (kernel ppg_link_rows) and predpreygrass_amd.trajectory on the MI355X: the scenarios of tests/link_cases.py, which
test_link_emulated.py runs through the wave emulator, at 64 envs; a full batch on the default cooperative plan; a fused rollout
between two link calls."""
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import link_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64
ENVS = [0, 1, 17, 40, 63]


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


@pytest.mark.parametrize("cfg,prey_cap,calls", [(cases.CFG_BASE_Q1, 64, 100), (cases.CFG_BASE, 128, 100), (cases.CFG_BASE_Q4, 256, 60)])
def test_link_base_family_on_gpu(cfg, prey_cap, calls):
    env = make(cfg, B, prey_capacity=prey_cap, seed=11)
    assert (env.pred_capacity, env.prey_capacity) == (64, prey_cap)
    seen = cases.link_vs_id_join(env, calls, envs=ENVS)
    if prey_cap == 256:
        assert seen["prey_rows"] > 128, seen


def test_link_128_predator_rows_births_cross_row_64_on_gpu():
    env = make(cases.CFG_P2, B, pred_capacity=128, prey_capacity=256, seed=7)
    assert cases.link_vs_id_join(env, 90, envs=ENVS)["pred_rows"] > 64


def test_link_second_generation_on_gpu():
    cases.link_vs_id_join(make_rq(cases.CFG_RQ, B, seed=5), 100, envs=ENVS)


def test_link_walls_on_gpu():
    env = make_rq(cases.CFG_RQ, B, walls=True, seed=6).set_walls(cases.WALLS)
    cases.link_vs_id_join(env, 80, envs=ENVS)


def test_link_drive_on_gpu():
    env = make(cases.CFG_DRIVE, B, seed=9)
    assert env.obs_channels_pred > 4
    cases.link_vs_id_join(env, 80, envs=ENVS)


def test_link_full_batch_on_the_default_cooperative_plan():
    """4096 envs of the default config, 200 calls: the step runs on its default (cooperative) plan, the link kernel next to it.
    The default episode is 1000 steps long: no auto-reset falls into the run, births and deaths do."""
    env = make(config_env, 4096)
    assert env.wave_plan()[2] > 0 and env.step_kernel_name().startswith("ppgc"), (env.wave_plan(), env.step_kernel_name())
    cases.link_vs_id_join(env, 200, envs=[0, 1, 2047, 4095], need=("birth", "death"))
    assert env.wave_plan()[2] > 0


@pytest.mark.parametrize("batch,envs", [(B, ENVS), (4096, [0, 1, 2047, 4095])])
def test_link_across_a_fused_rollout_on_gpu(batch, envs):
    """ppg_rollout(8) between two link calls: the 8-step maps (4096 envs: the fused cooperative rollout kernel)."""
    env = make(cases.CFG_BASE, batch, seed=2)
    cases.link_across_rollout(env, n_rounds=12, K=8, envs=envs)


@pytest.mark.parametrize("family", ["base", "second_generation"])
def test_returns_and_gae_vs_agent_names_on_gpu(family):
    env = make(cases.CFG_BASE, B, seed=3) if family == "base" else make_rq(cases.CFG_RQ, B, seed=4)
    traj = cases.returns_vs_names(env, 70, 0.97, envs=ENVS)
    assert traj.reward.device.type == "cuda" and traj.next_row.dtype == torch.int16


def test_invalidation_on_gpu():
    cases.invalidation(make(cases.CFG_BASE, 3, seed=1))
    cases.invalidation(make_rq(cases.CFG_RQ, 3, seed=1), set_placement=False)


def test_sub_batches_forward_link_on_gpu():
    from predpreygrass_amd.subbatch import SubBatchedPredPreyGrass
    env = SubBatchedPredPreyGrass(cases.CFG_BASE, batch_size=128, n_sub=2, device=DEV)
    env.reset()
    env.link()
    env.step(random_actions=True)
    maps = env.link()
    env.synchronize()
    assert len(maps) == 2 and all(bool((p >= 0).any()) and tuple(p.shape) == (64, e.S) for (p, n), e in zip(maps, env.subs))
