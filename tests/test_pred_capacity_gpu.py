"""128 predator rows per environment on the MI355X: the ppg_*_p2q<NQ>g kernels against the C oracles (the scenarios of
tests/pred_capacity_cases.py, which test_pred_capacity_emulated.py runs through the wave emulator)."""
import numpy as np
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env
from predpreygrass_amd.env import PredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import pred_capacity_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


@pytest.mark.parametrize("B,envs", [(3, None), (64, [0, 17, 63])])
@pytest.mark.parametrize("cfg,prey_cap", [(cases.CFG_START, 256), (cases.CFG_START_Q2, 128)])
def test_start_above_64_predators_on_gpu(B, envs, cfg, prey_cap):
    env = make(cfg, B, pred_capacity=128, prey_capacity=prey_cap)
    assert env.step_kernel_name() == f"ppg_step_p2q{prey_cap // 64}g"
    assert cases.rollout_base(env, cfg, seed0=31, n_calls=200, envs=envs) > 64


@pytest.mark.parametrize("B,envs", [(3, None), (64, [0, 5, 40])])
def test_predators_cross_64_by_births_on_gpu(B, envs):
    env = make(cases.CFG_CROSS, B, pred_capacity=128, prey_capacity=256)
    assert cases.rollout_base(env, cases.CFG_CROSS, seed0=7, n_calls=160, envs=envs) > 64


@pytest.mark.parametrize("kick", [False, True])
def test_dict_class_explicit_order_on_gpu(kick):
    cfg = dict(cases.CFG_START)
    if kick:
        cfg.update(kickback_reward_predator=7.0, kickback_reward_prey=3.0, predator_creation_energy_threshold=6.0,
                   n_possible_predators=125)

    def mk(c):
        return PredPreyGrass(c, prey_capacity=256, pred_capacity=128, device=DEV)
    env, most = cases.dict_class_vs_oracle(mk, cfg, seed=8 if kick else 5, n_calls=40)
    assert most > 64
    assert env._b.step_kernel_name() == ("ppg_step_kick_p2q4g" if kick else "ppg_step_p2q4g")


@pytest.mark.parametrize("B,envs", [(3, None), (64, [0, 33, 63])])
def test_second_generation_on_gpu(B, envs):
    env = make_rq(cases.CFG_RQ, B, pred_capacity=128, prey_capacity=256)
    assert env.step_kernel_name() == "ppg2_step_p2q4g"
    assert cases.rollout_rq(env, cases.CFG_RQ, seed0=11, n_calls=120, envs=envs) > 64


@pytest.mark.parametrize("shuffle", [False, True])
def test_second_generation_caller_uniforms_on_gpu(shuffle):
    env = make_rq(cases.CFG_RQ, 3, pred_capacity=128, prey_capacity=128)
    assert env.step_kernel_name() == "ppg2_step_p2q2g"
    most, n_ordered = cases.rq_with_caller_uniforms(env, cases.CFG_RQ, seed=3, n_calls=60, shuffle=shuffle)
    assert most > 64 and (n_ordered > 0) == shuffle


@pytest.mark.parametrize("B", [3, 64])
def test_fused_rollout_equals_single_steps_on_gpu(B):
    env = cases.fused_rollout_equals_steps(make, cases.CFG_START, B, 70)
    torch.cuda.synchronize()
    assert env.step_kernel_name() == "ppg_step_p2q2g"   # (prey capacity 128)


def test_state_tools_on_gpu():
    cases.state_tools(make, cases.CFG_START, 3, 6)


@pytest.mark.parametrize("B", [3, 64])
def test_overflow_contract_on_gpu(B):
    cases.overflow_contract(make, cases.CFG_BOOM, B, 250)
    env = PredPreyGrass(cases.CFG_BOOM, prey_capacity=256, pred_capacity=128, device=DEV)
    assert env._b.pred_capacity == 128
    obs, _ = env.reset(seed=1)
    live = list(obs)
    rng = np.random.default_rng(0)
    with pytest.raises(RuntimeError, match="agent row capacity exceeded"):
        for _ in range(250):
            o, _, te, tr, _ = env.step({a: int(rng.integers(9)) for a in live})
            live = [a for a in o if not te[a] and not tr[a]]


def test_full_size_batch_on_gpu():
    """4096 envs on a 40x40 grid with 80 predators each, 200 calls; a handful of envs checked against the oracle on every call."""
    cfg = {**config_env, "grid_size": 40, "n_initial_active_predator": 80, "n_initial_active_prey": 150,
           "initial_num_grass": 300, "max_steps": 150}
    env = make(cfg, 4096, pred_capacity=128, prey_capacity=256)
    assert env.step_kernel_name() == "ppg_step_p2q4g" and env.wave_plan() == (1, 0, 0)
    assert cases.rollout_base(env, cfg, seed0=77, n_calls=200, envs=[0, 1, 2047, 4095], check_grid=False) > 64


def test_policy_refuses_128_predator_rows_on_gpu():
    from predpreygrass_amd.policy import FusedPolicy, PolicyNet
    env = make(cases.CFG_START, 2, pred_capacity=128, prey_capacity=256)
    env.reset(seed=1)
    fused = FusedPolicy(PolicyNet(env.Rp), PolicyNet(env.Rq), device=DEV)
    with pytest.raises((ValueError, RuntimeError), match="predator rows"):
        fused.act([env])
