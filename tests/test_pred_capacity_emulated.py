"""128 predator rows per environment (two predator row registers, ppg_*_p2q<NQ>g kernels) through the kernel source compiled
for the CPU wave emulator: every call compared with the C oracles.  The same scenarios run on the GPU in
test_pred_capacity_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env
from predpreygrass_amd.env import PredPreyGrass, VectorPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen, config_env_base
from predpreygrass_amd.red_queen import PredPreyGrass as RQPredPreyGrass
from tests import pred_capacity_cases as cases
from tests.emu_backend import library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


@pytest.mark.parametrize("cfg,prey_cap,calls", [(cases.CFG_START, 256, 200), (cases.CFG_START_Q2, 128, 120)])
def test_start_above_64_predators(cfg, prey_cap, calls):
    env = make(cfg, 3, pred_capacity=128, prey_capacity=prey_cap)
    assert env.step_kernel_name() == f"ppg_step_p2q{prey_cap // 64}g"
    assert cases.rollout_base(env, cfg, seed0=31, n_calls=calls) > 64


def test_predators_cross_64_by_births():
    env = make(cases.CFG_CROSS, 3, pred_capacity=128, prey_capacity=256)
    most = cases.rollout_base(env, cases.CFG_CROSS, seed0=7, n_calls=160)
    assert most > 64, most


def test_dict_class_explicit_order_past_rank_63():
    def mk(cfg):
        return PredPreyGrass(cfg, prey_capacity=256, pred_capacity=128, _library=library())
    env, most = cases.dict_class_vs_oracle(mk, cases.CFG_START, seed=5, n_calls=40)
    assert env._b.pred_capacity == 128 and most > 64


def test_dict_class_explicit_order_kickback():
    cfg = {**cases.CFG_START, "kickback_reward_predator": 7.0, "kickback_reward_prey": 3.0,
           "predator_creation_energy_threshold": 6.0, "n_possible_predators": 125}   # (the id pool keeps it below 128 rows)

    def mk(cfg):
        return PredPreyGrass(cfg, prey_capacity=256, pred_capacity=128, _library=library())
    env, most = cases.dict_class_vs_oracle(mk, cfg, seed=8, n_calls=40)
    assert env._b.step_kernel_name() == "ppg_step_kick_p2q4g" and most > 64


def test_second_generation_philox():
    env = make_rq(cases.CFG_RQ, 3, pred_capacity=128, prey_capacity=256)
    assert env.step_kernel_name() == "ppg2_step_p2q4g"
    assert cases.rollout_rq(env, cases.CFG_RQ, seed0=11, n_calls=120) > 64


@pytest.mark.parametrize("shuffle", [False, True])
def test_second_generation_caller_uniforms(shuffle):
    env = make_rq(cases.CFG_RQ, 2, pred_capacity=128, prey_capacity=128)
    most, n_ordered = cases.rq_with_caller_uniforms(env, cases.CFG_RQ, seed=3, n_calls=60, shuffle=shuffle)
    assert most > 64 and (n_ordered > 0) == shuffle


def test_fused_rollout_equals_single_steps():
    cases.fused_rollout_equals_steps(make, cases.CFG_START, 3, 70)


def test_state_tools():
    cases.state_tools(make, cases.CFG_START, 3, 6)


def test_overflow_contract():
    cases.overflow_contract(make, cases.CFG_BOOM, 2, 250)
    env = PredPreyGrass(cases.CFG_BOOM, prey_capacity=256, pred_capacity=128, _library=library())
    assert env._b.pred_capacity == 128
    rng = np.random.default_rng(0)
    obs, _ = env.reset(seed=1)
    live = list(obs)
    with pytest.raises(RuntimeError, match="agent row capacity exceeded"):
        for _ in range(250):
            o, _, te, tr, _ = env.step({a: int(rng.integers(9)) for a in live})
            live = [a for a in o if not te[a] and not tr[a]]


def test_dict_classes_keep_64_rows_unless_asked():
    """Without pred_capacity the dict classes keep 64 predator rows and name the keyword when the initial predators need more."""
    assert PredPreyGrass(config_env, _library=library())._b.pred_capacity == 64
    assert VectorPredPreyGrass(config_env, num_envs=2, _library=library()).batch.pred_capacity == 64
    assert RQPredPreyGrass(config_env_base, _library=library())._b.pred_capacity == 64
    assert make(config_env, 1).pred_capacity == 64
    with pytest.raises(ValueError, match="pred_capacity=128"):
        PredPreyGrass(cases.CFG_START, prey_capacity=256, _library=library())
    with pytest.raises(ValueError, match="pred_capacity=128"):
        VectorPredPreyGrass(cases.CFG_START, num_envs=2, prey_capacity=256, _library=library())
    with pytest.raises(ValueError, match="pred_capacity=128"):
        RQPredPreyGrass(cases.CFG_RQ, _library=library())
    assert PredPreyGrass(cases.CFG_START, prey_capacity=256, pred_capacity=128, _library=library())._b.pred_capacity == 128
    assert VectorPredPreyGrass(cases.CFG_START, num_envs=2, prey_capacity=256, pred_capacity=128,
                               _library=library()).batch.pred_capacity == 128
    assert RQPredPreyGrass(cases.CFG_RQ, pred_capacity=128, _library=library())._b.pred_capacity == 128


def test_rejections():
    with pytest.raises(ValueError, match="pred_capacity"):
        make(config_env, 1, pred_capacity=96)
    with pytest.raises(ValueError, match="pred_capacity"):
        make_rq(config_env_base, 1, pred_capacity=96)
    with pytest.raises(ValueError, match="prey_capacity 128 or 256"):
        make(config_env, 1, pred_capacity=128, prey_capacity=64)
    with pytest.raises(ValueError, match="walls"):
        make_rq(config_env_base, 1, pred_capacity=128, walls=True)
    with pytest.raises(ValueError, match="drive"):
        make({**config_env, "enable_drive_channels": True}, 1, pred_capacity=128)
    # walls / drive dict classes keep rejecting more than 64 initial predators
    from predpreygrass_amd.drive_conditioned import PredPreyGrass as DrivePredPreyGrass
    from predpreygrass_amd.walls_occlusion import PredPreyGrass as WallsPredPreyGrass
    with pytest.raises(ValueError, match="row capacities"):
        DrivePredPreyGrass(cases.CFG_START, _library=library())
    with pytest.raises(ValueError, match="row capacities"):
        WallsPredPreyGrass(cases.CFG_RQ, _library=library())
    env = make(cases.CFG_START, 2, pred_capacity=128, prey_capacity=256)
    with pytest.raises(RuntimeError, match="one-wave"):
        env.set_wave_plan(4, 0, 2)
    with pytest.raises(RuntimeError, match="one-wave"):
        env.set_wave_plan(2, 0, 0)
    env.set_wave_plan(1, 0, 0)
    assert env.wave_plan() == (1, 0, 0) and env.step_kernel_name() == "ppg_step_p2q4g"
    assert env._lib.ppg_set_envs_in_flight(env._handle, 64) == 0 and env.wave_plan() == (1, 0, 0)   # (64 envs: eight waves otherwise)


_SAN_CODE = (
    "import sys; sys.path.insert(0, %r)\n"
    "from tests.emu_backend import library\n"
    "from tests import pred_capacity_cases as cases\n"
    "from predpreygrass_amd.batched import BatchedPredPreyGrass\n"
    "from predpreygrass_amd.red_queen import BatchedRedQueen\n"
    "lib = library(sanitize=%r)\n"
    "mk = lambda cfg, B, **kw: BatchedPredPreyGrass(cfg, batch_size=B, _library=lib, **kw)\n"
    "assert cases.rollout_base(mk(cases.CFG_START, 2, pred_capacity=128, prey_capacity=256), cases.CFG_START, 31, 40) > 64\n"
    "assert cases.rollout_base(mk(cases.CFG_START_Q2, 2, pred_capacity=128, prey_capacity=128), cases.CFG_START_Q2, 31, 30) > 64\n"
    "cases.rollout_base(mk(cases.CFG_CROSS, 2, pred_capacity=128, prey_capacity=256), cases.CFG_CROSS, 7, 60)\n"
    "rq = BatchedRedQueen(cases.CFG_RQ, batch_size=2, _library=lib, pred_capacity=128, prey_capacity=256)\n"
    "assert cases.rollout_rq(rq, cases.CFG_RQ, 11, 40) > 64\n"
    "print('SAN-CLEAN')\n")


def test_128_predator_rows_clean_under_ubsan():
    code = _SAN_CODE % (ROOT, True)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0 and "SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])


def test_128_predator_rows_clean_under_address_sanitizer():
    from tests.emu_backend import asan_runtime, build
    rt = asan_runtime()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("gcc has no libasan.so here")
    build(sanitize="address")
    code = _SAN_CODE % (ROOT, "address")
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", PYTHONMALLOC="malloc")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1800, env=env)
    assert out.returncode == 0 and "SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
