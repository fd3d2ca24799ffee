"""The resident split on the MI355X: the cooperative step kernels write the observations of envs behind the resident count with
non-temporal stores -- the same bits whatever the count is -- and `ppg_rebalance` computes the count on the device as the number of
leading envs whose rows in use fit the handle's share of the budget (include/ppg.h: ppg_set_resident_envs)."""
import numpy as np
import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.config import config_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUTPUTS = ("obs_pred", "obs_prey", "row_reward", "row_flags", "row_id", "row_xy", "row_energy", "row_cumrew", "row_parent",
           "grass_xy", "grass_energy", "env_state")


def _bits(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).clone()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16], ids=["f64", "f32", "bf16"])
def test_outputs_do_not_depend_on_the_resident_count_on_gpu(dtype):
    """9 envs on the plan (4, 0, 2) -- the last workgroup holds one env -- 24 steps of device-side random actions with auto-reset (a
    short episode: resets inside), a rebalance every 4 steps; counts 0, 3 (inside a workgroup's pair) and 9."""
    cfg = {**config_env, "max_steps": 10}
    runs = {}
    for n in (0, 3, 9):
        env = BatchedPredPreyGrass(cfg, batch_size=9, device=DEV, obs_dtype=dtype, seed=31)
        env.set_wave_plan(4, 0, 2)
        assert env.wave_plan() == (4, 0, 2)
        snaps = []
        for t in range(24):
            if t % 4 == 0:
                env.rebalance()
                env.set_resident_envs(n)
                assert env.resident_envs() == n
            env.step(random_actions=True, auto_reset=True)
            snaps.append({o: _bits(getattr(env, o)) for o in OUTPUTS})
        runs[n] = snaps
    assert int(runs[0][-1]["obs_prey"].ne(0).sum()) > 0
    for n in (3, 9):
        for t, (a, b) in enumerate(zip(runs[0], runs[n])):
            for o in OUTPUTS:
                assert torch.equal(a[o], b[o]), (n, "call", t, o)


@pytest.mark.parametrize("in_flight", [64, 192])
def test_rebalance_computes_the_cut_on_gpu(in_flight, monkeypatch):
    """64 envs some steps into their episodes; budgets that put the cut at 0, inside the batch and at the batch size, against a numpy
    prefix sum over the row counts in env_state with the share formula budget * batch / envs in flight."""
    B = 64
    probe = BatchedPredPreyGrass(config_env, batch_size=B, device=DEV, seed=3)
    bytes_p = probe.obs_pred[0, 0].numel() * 8
    bytes_q = probe.obs_prey[0, 0].numel() * 8
    one_env = 6 * bytes_p + 8 * bytes_q   # the initial populations
    for budget in (0, 1, one_env * 20 * in_flight // B, one_env * 40 * in_flight // B + 12345, 1 << 40):
        monkeypatch.setenv("PPG_RESIDENT_BYTES", str(budget))
        env = BatchedPredPreyGrass(config_env, batch_size=B, device=DEV, seed=3)
        assert env._lib.ppg_set_envs_in_flight(env._handle, in_flight) == 0
        for _ in range(12):
            env.step(random_actions=True, auto_reset=True)
        env.rebalance()
        es = env.env_state.cpu().numpy().astype(np.int64)
        per_env = es[:, _abi.ENV_N_PRED_ROWS] * bytes_p + es[:, _abi.ENV_N_PREY_ROWS] * bytes_q
        share = budget * B // in_flight
        want = int((np.cumsum(per_env) <= share).sum())
        got = env.resident_envs()
        if budget == 0:   # off: the word was never written
            assert got == B
            continue
        assert got == want, (budget, share, got, want)
        assert {1: 0, 1 << 40: B}.get(budget, got) == got
        if budget not in (1, 1 << 40):
            assert 0 < got < B, (budget, got)
        env.step(random_actions=True, auto_reset=True)   # and a step with that cut runs
        torch.cuda.synchronize()
