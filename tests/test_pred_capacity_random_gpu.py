"""Random configurations on 128 predator rows on the MI355X: the one-wave ppg_*_p2q<NQ>g / ppg2_*_p2q<NQ>g kernels against the C
oracles, call by call and bit for bit (the scenarios of tests/pred_capacity_random.py; test_pred_capacity_random_emulated.py runs them
through the wave emulator over other seeds and checks, on the oracle alone, what both seed sets reach).  Every environment has B = 1
or 3 on a grid of at most 30 for at most 45 calls."""
import numpy as np
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.env import PredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from predpreygrass_amd.red_queen import PredPreyGrass as RQPredPreyGrass
from tests import pred_capacity_cases as cases
from tests import pred_capacity_random as rand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


def dict_env(cfg, prey_cap):
    env = PredPreyGrass(cfg, prey_capacity=prey_cap, pred_capacity=128, device=DEV)
    assert env._b.step_kernel_name().endswith(f"_p2q{env._b.prey_capacity // 64}g"), env._b.step_kernel_name()
    return env


def dict_env_rq(cfg, prey_cap):
    env = RQPredPreyGrass(cfg, prey_capacity=prey_cap, pred_capacity=128, device=DEV, _check_analytics=True)
    assert env._b.step_kernel_name() == f"ppg2_step_p2q{env._b.prey_capacity // 64}g", env._b.step_kernel_name()
    return env


@pytest.mark.parametrize("seed", rand.GPU_BASE_SEEDS)
def test_random_p2_config_matches_oracle_on_gpu(seed):
    rand.differential_base(dict_env, seed)


@pytest.mark.parametrize("seed", rand.GPU_RQ_SEEDS)
def test_random_gen2_p2_config_matches_oracle_on_gpu(seed):
    rand.differential_rq(dict_env_rq, seed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("i", range(rand.N_DTYPE_CONFIGS))
def test_observation_dtypes_match_oracle_on_gpu(i, dtype):
    cfg, prey_cap = rand.dtype_config(i)
    _, most = rand.rollout_dtype_vs_oracle(make, cfg, prey_cap, dtype, seed0=100 + i, n_calls=30)
    assert most > 64


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16], ids=["float64", "float32", "bfloat16"])
def test_observe_rewrites_the_rows_of_the_step_on_gpu(dtype):
    cfg, prey_cap = rand.dtype_config(3)
    rand.observe_matches(rand.env_with_many_predators(make, cfg, 7, seed=3, prey_capacity=prey_cap, obs_dtype=dtype))


def test_observe_rewrites_the_rows_of_the_step_second_generation_on_gpu():
    rand.observe_matches(rand.env_with_many_predators(make_rq, cases.CFG_RQ, 7, seed=3, prey_capacity=256))
    cfg, prey_cap = rand.random_config_rq_p2(np.random.default_rng(1000 + rand.EMU_RQ_SEEDS[0]))
    rand.observe_matches(rand.env_with_many_predators(make_rq, cfg, 3, seed=5, prey_capacity=prey_cap))
