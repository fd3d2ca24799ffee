"""The resident split (`ppg_set_resident_envs`, KParams::resident_envs) through the kernel source compiled for the CPU wave emulator:
which envs write their observations with non-temporal stores is a cache policy, so every output must be the same bits whatever the
count is -- and equal to the C oracle call by call.  7 envs on the plan (4, 0, 2): the last workgroup holds one env, and the count 3
puts the cut inside a workgroup's pair of envs.  The same through `ppg_rollout`, whose fused kernels ignore the word."""
import pytest
import torch

from oracle.ppg_oracle import OracleEnv
from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env
from tests.emu_backend import library
from tests.parity_utils import compare_env_with_oracle

B, SEED0 = 7, 4242
CONFIGS = {
    "default": dict(config_env),
    # (a short episode: truncation calls and auto-resets inside the 24 calls)
    "8x8_windows_5_7": {**config_env, "grid_size": 8, "predator_obs_range": 5, "prey_obs_range": 7, "initial_num_grass": 20,
                        "max_steps": 10},
}
OUTPUTS = ("obs_pred", "obs_prey", "row_reward", "row_flags", "row_id", "row_xy", "row_energy", "row_cumrew", "row_parent",
           "grass_xy", "grass_energy", "env_state")


def _bits(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).clone()


def _run(cfg, dtype, n_resident, fused):
    """24 transitions with device-side random actions and auto-reset, a rebalance every 4 steps (fused: every `ppg_rollout(6)`), the
    count written again behind every rebalance; every call checked against one oracle per env.  Returns every output after every call."""
    env = BatchedPredPreyGrass(cfg, batch_size=B, obs_dtype=dtype, _library=library())
    env.set_wave_plan(4, 0, 2)
    assert env.wave_plan() == (4, 0, 2), env.wave_plan()
    assert env.resident_envs() == B   # never written: every env is resident
    oracles = [OracleEnv(cfg) for _ in range(B)]
    env.set_seeds(SEED0)
    env.env_state.zero_()   # every env done: the first auto-reset call performs the reset (as in parity_utils.rollout_vs_oracle)
    env.env_state[:, _abi.ENV_FLAGS] = _abi.ENVF_DONE
    env.env_state[:, _abi.ENV_EPISODE] = -1
    per_call, calls = (6, 4) if fused else (1, 24)
    snaps = []
    for t in range(calls):
        if fused or t % 4 == 0:
            env.rebalance()
            env.set_resident_envs(n_resident)
            assert env.resident_envs() == n_resident
        if fused:
            env.rollout(per_call, random_actions=True, auto_reset=True)
        else:
            env.step(random_actions=True, auto_reset=True)
        tables = env.host_tables()
        for b in range(B):
            assert oracles[b].rollout_random((SEED0 + b) & (2 ** 64 - 1), per_call) == per_call
            compare_env_with_oracle(env, b, oracles[b], tables, tag=f"resident {n_resident} call {t}")
        snaps.append({n: _bits(getattr(env, n)) for n in OUTPUTS})
    return snaps


@pytest.mark.parametrize("fused", [False, True], ids=["step", "rollout"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16], ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_outputs_do_not_depend_on_the_resident_count(name, dtype, fused):
    runs = {n: _run(CONFIGS[name], dtype, n, fused) for n in (0, 3, 7)}
    for n in (3, 7):
        for t, (a, b) in enumerate(zip(runs[0], runs[n])):
            for out in OUTPUTS:
                assert torch.equal(a[out], b[out]), (name, n, "call", t, out)


def test_rebalance_writes_the_count_of_envs_that_fit(monkeypatch):
    """The emulated library computes the same cut as the device kernel: 7 envs fit any real budget, a budget of a few rows does not."""
    cfg = CONFIGS["default"]
    env = BatchedPredPreyGrass(cfg, batch_size=B, _library=library())
    env.reset(seed=5)
    env.rebalance()
    assert env.resident_envs() == B
    rows = env.env_state[:, [_abi.ENV_N_PRED_ROWS, _abi.ENV_N_PREY_ROWS]].to(torch.int64)
    per_env = rows[:, 0] * env.obs_pred[0, 0].numel() * 8 + rows[:, 1] * env.obs_prey[0, 0].numel() * 8
    monkeypatch.setenv("PPG_RESIDENT_BYTES", str(int(per_env[:3].sum())))   # exactly three envs
    small = BatchedPredPreyGrass(cfg, batch_size=B, _library=library())
    small.reset(seed=5)
    small.rebalance()
    assert small.resident_envs() == 3
    monkeypatch.setenv("PPG_RESIDENT_BYTES", "0")   # off: rebalance leaves the word alone
    off = BatchedPredPreyGrass(cfg, batch_size=B, _library=library())
    off.reset(seed=5)
    off.set_resident_envs(2)
    off.rebalance()
    assert off.resident_envs() == 2
