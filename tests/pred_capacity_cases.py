"""Scenarios of environments with 128 predator rows (two predator row registers in the kernels), shared by the wave-emulator
tests (test_pred_capacity_emulated.py) and the GPU tests (test_pred_capacity_gpu.py).  Every check compares the kernels with the
C oracles, which keep dense grids and ordered dicts without any row cap.

`make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a BatchedRedQueen, both on the backend under test."""
import ctypes as C

import numpy as np
import torch

from oracle.ppg_oracle import OracleEnv
from oracle.rq_oracle import RQOracleEnv
from predpreygrass_amd import _abi
from predpreygrass_amd.config import config_env
from predpreygrass_amd.red_queen import config_env_base
from tests.parity_utils import compare_env_with_oracle
from tests.parity_utils_rq import compare_env_with_oracle as compare_env_with_oracle_rq
from tests.parity_utils_rq import fill_actions as fill_actions_rq

# 70 predators from the start: prey capacity 256 (four prey registers) and 128 (two)
CFG_START = {**config_env, "grid_size": 30, "n_initial_active_predator": 70, "n_initial_active_prey": 120,
             "initial_num_grass": 200, "max_steps": 90}
CFG_START_Q2 = {**config_env, "grid_size": 22, "n_initial_active_predator": 66, "n_initial_active_prey": 40,
                "initial_num_grass": 60, "max_steps": 70, "prey_creation_energy_threshold": 100.0}
# about 50 predators that breed cheaply on plenty of prey: the population crosses 64 by births (newborns land in register 1); the id
# pool stops it below 128
CFG_CROSS = {**config_env, "grid_size": 24, "n_initial_active_predator": 50, "n_initial_active_prey": 150,
             "initial_num_grass": 120, "predator_creation_energy_threshold": 6.0, "prey_creation_energy_threshold": 5.0,
             "energy_gain_per_step_grass": 0.2, "n_possible_predators": 125, "max_steps": 120}
# the same without the id pool: a predator boom past 128 rows
CFG_BOOM = {**CFG_CROSS, "n_initial_active_predator": 100, "n_possible_predators": 2000, "max_steps": 300}
# second generation: both predator types, more than 64 predator rows that breed
# (the id pools, 60 + 60, keep it below 128 rows)
CFG_RQ = {**config_env_base, "grid_size": 24, "n_possible_type_1_predators": 60, "n_possible_type_2_predators": 60,
          "n_initial_active_type_1_predator": 40, "n_initial_active_type_2_predator": 30,
          "n_initial_active_type_1_prey": 40, "n_initial_active_type_2_prey": 40, "initial_num_grass": 120,
          "predator_creation_energy_threshold": 7.0, "reproduction_cooldown_steps": 2, "max_steps": 80}


def _start(env, seed0):
    """The first auto-reset call performs the reset (episode 0), as in parity_utils.rollout_vs_oracle."""
    env.set_seeds(seed0)
    env.env_state.zero_()
    env.env_state[:, _abi.ENV_FLAGS] = _abi.ENVF_DONE
    env.env_state[:, _abi.ENV_EPISODE] = -1


def rollout_base(env, cfg, seed0, n_calls, envs=None, check_grid=True):
    """Device reset + device random actions + auto-reset, every call of the envs in `envs` compared with its oracle (tables,
    observations, the rebuilt grid).  Returns the largest live predator count seen."""
    envs = list(range(env.batch_size)) if envs is None else envs
    oracles = {b: OracleEnv(cfg) for b in envs}
    _start(env, seed0)
    most = 0
    for t in range(n_calls):
        env.step(random_actions=True, auto_reset=True)
        for b in envs:
            assert oracles[b].rollout_random((seed0 + b) & (2 ** 64 - 1), 1) == 1
        tables = env.host_tables()
        grid = env.export_grid().cpu().numpy() if check_grid else None
        for b in envs:
            es = tables["env_state"][b]
            assert int(es[_abi.ENV_STATUS]) & ~_abi.STATUS_FALLBACK_SPAWN == 0, (t, b, "status", int(es[_abi.ENV_STATUS]))
            compare_env_with_oracle(env, b, oracles[b], tables, tag=f"call {t}")
            if check_grid:
                assert grid[b].tobytes() == oracles[b].grid_world_state.tobytes(), (t, b, "grid")
            most = max(most, int(es[_abi.ENV_N_PRED_ALIVE]))
    return most


def rollout_rq(env, cfg, seed0, n_calls, envs=None, check_grid=True):
    """The same for the second generation (Philox reproduction uniforms on the device).  Returns the largest predator row count."""
    envs = list(range(env.batch_size)) if envs is None else envs
    oracles = {b: RQOracleEnv(cfg) for b in envs}
    _start(env, seed0)
    most = 0
    for t in range(n_calls):
        env.step(random_actions=True, auto_reset=True)
        for b in envs:
            assert oracles[b].rollout_random((seed0 + b) & (2 ** 64 - 1), 1) == 1
        tables = env.host_tables()
        grid = env.export_grid().cpu().numpy() if check_grid else None
        for b in envs:
            es = tables["env_state"][b]
            assert int(es[_abi.ENV_STATUS]) & ~_abi.STATUS_FALLBACK_SPAWN == 0, (t, b, "status", int(es[_abi.ENV_STATUS]))
            compare_env_with_oracle_rq(env, b, oracles[b], tables, tag=f"call {t}")
            if check_grid:
                assert grid[b].astype(np.float32).tobytes() == oracles[b].grid_world_state.tobytes(), (t, b, "grid")
            most = max(most, int(es[_abi.ENV_N_PRED_ROWS]))
    return most


def rq_with_caller_uniforms(env, cfg, seed, n_calls, shuffle):
    """Env 0 of `env` driven by host action dicts and caller-supplied reproduction uniforms (ppg_step_uniforms), against the oracle
    stepped with the same dicts and uniforms; shuffle=True: every dict in a random order (explicit action order, ranks past 63)."""
    rng = np.random.default_rng(seed)
    orc = RQOracleEnv(cfg)
    env.reset(seed=seed)
    placement = _placement_of(env, 0)
    orc.reset_from_placement(*placement)
    env.set_placement(*[np.repeat(np.asarray(a)[None], env.batch_size, axis=0) for a in placement])   # (every env: env 0's cells)
    rank = torch.zeros((env.batch_size, env.S), dtype=torch.uint8, device=env.device)
    ar = env.action_ranges
    most = n_ordered = 0
    for t in range(n_calls):
        recs = env.records(0)
        live = [r[0] for r in recs if not r[4]]
        acts = {n: int(rng.integers(ar[1 if "type_2" in n else 0] ** 2)) for n in live}
        if shuffle:
            names = list(acts)
            rng.shuffle(names)
            acts = {n: acts[n] for n in names}
        in_order = fill_actions_rq(env, 0, recs, acts, rank)
        n_ordered += not in_order
        u = rng.random(4 * env.S + 8)
        ut = torch.zeros((env.batch_size, u.size), dtype=torch.float64, device=env.device)
        ut[0] = torch.from_numpy(u)
        env.step(uniforms=ut, act_rank=None if in_order else rank)
        orc.step(acts, uniforms=u)
        tables = env.host_tables()
        es = tables["env_state"][0]
        assert int(es[_abi.ENV_STATUS]) & ~_abi.STATUS_FALLBACK_SPAWN == 0, (t, "status", int(es[_abi.ENV_STATUS]))
        compare_env_with_oracle_rq(env, 0, orc, tables, tag=f"call {t}")
        assert env.export_grid().cpu().numpy()[0].astype(np.float32).tobytes() == orc.grid_world_state.tobytes(), (t, "grid")
        most = max(most, int(es[_abi.ENV_N_PRED_ROWS]))
        if bool(int(es[_abi.ENV_FLAGS]) & (_abi.ENVF_TERM_ALL | _abi.ENVF_TRUNC_ALL)):
            break
    return most, n_ordered


def _placement_of(env, b):
    """(pred_xy, prey_xy, grass_xy) of env b as [n, 2] arrays, from its row tables right after a reset."""
    t = env.host_tables()
    es = t["env_state"][b]
    nP, nQ, cp = int(es[_abi.ENV_N_PRED_ROWS]), int(es[_abi.ENV_N_PREY_ROWS]), env.pred_capacity
    xy = t["row_xy"][b].astype(np.int64) & 0xFFFF

    def pairs(v):
        return np.stack([v >> 8, v & 255], axis=1)
    return pairs(xy[:nP]), pairs(xy[cp:cp + nQ]), pairs(t["grass_xy"][b][: env.n_grass].astype(np.int64) & 0xFFFF)


def dict_class_vs_oracle(make_dict_env, cfg, seed, n_calls, shuffle=True):
    """env.PredPreyGrass driven with (shuffled) action dicts of random actions, call by call against the oracle stepped with the
    same dicts: observations, rewards, flags in the reference's dict order.  Returns the largest number of acting predators."""
    from predpreygrass_amd.placement import reference_placement
    rng = np.random.default_rng(seed)
    env = make_dict_env(cfg)
    orc = OracleEnv(cfg)
    obs, _ = env.reset(seed=seed)
    nP, nQ = cfg["n_initial_active_predator"], cfg["n_initial_active_prey"]
    cells = np.asarray(reference_placement(cfg["grid_size"], nP + nQ + cfg["initial_num_grass"], seed))
    oobs, _ = orc.reset_from_placement(cells[:nP], cells[nP:nP + nQ], cells[nP + nQ:])
    _same_dicts((obs,), (oobs,), "reset")
    most = 0
    live = list(obs)   # the live-agent protocol: the agents observed and not terminated in the last call
    for t in range(n_calls):
        acts = {a: int(rng.integers(9)) for a in live}
        if shuffle:
            names = list(acts)
            rng.shuffle(names)
            acts = {n: acts[n] for n in names}
        most = max(most, sum(1 for a in acts if a.startswith("predator")))
        got = env.step(acts)
        want = orc.step(acts)
        _same_dicts(got[:4], want[:4], f"call {t}")
        live = [a for a in got[0] if not got[2][a] and not got[3][a]]
        if got[2]["__all__"] or got[3]["__all__"]:
            break
    return env, most


def _same_dicts(got, want, tag):
    for g, w in zip(got, want):
        assert list(g) == list(w), (tag, "keys")
        for k in w:
            gv, wv = np.asarray(g[k]), np.asarray(w[k])
            assert gv.tobytes() == wv.astype(gv.dtype).tobytes(), (tag, k)


def state_of(env):
    names = ["row_xy", "row_energy", "row_id", "row_key", "row_cumrew", "row_flags", "row_reward", "grass_xy", "grass_energy",
             "env_state", "obs_pred", "obs_prey"]
    return {n: getattr(env, n).clone() for n in names}


def assert_same_state(a, b, env):
    """The rows in use, grass, env words and the observation rows in use of two state dicts are equal."""
    assert torch.equal(a["env_state"], b["env_state"])
    nP, nQ = a["env_state"][:, _abi.ENV_N_PRED_ROWS], a["env_state"][:, _abi.ENV_N_PREY_ROWS]
    cp = env.pred_capacity
    rows = torch.arange(env.S, device=env.device)[None, :]
    used = (rows < nP[:, None]) | ((rows >= cp) & (rows < cp + nQ[:, None]))
    for n in ("row_xy", "row_energy", "row_id", "row_key", "row_cumrew", "row_flags", "row_reward"):
        assert torch.equal(a[n][used], b[n][used]), n
    assert torch.equal(a["grass_xy"], b["grass_xy"]) and torch.equal(a["grass_energy"], b["grass_energy"])
    assert torch.equal(a["obs_pred"][used[:, :cp]], b["obs_pred"][used[:, :cp]])
    assert torch.equal(a["obs_prey"][used[:, cp:]], b["obs_prey"][used[:, cp:]])


def fused_rollout_equals_steps(make, cfg, B, K):
    a, b = make(cfg, B, seed=21, pred_capacity=128), make(cfg, B, seed=21, pred_capacity=128)
    a.reset()
    b.reset()
    for _ in range(K):
        a.step(random_actions=True, auto_reset=True)
    b.rollout(K // 2, random_actions=True, auto_reset=True)
    b.rollout(K - K // 2, random_actions=True, auto_reset=True)
    assert_same_state(state_of(a), state_of(b), a)
    return a


def state_tools(make, cfg, B, calls):
    """Snapshot export -> import into another env; ppg_fetch == the tensors; ppg_pack rows == plain indexing -- with more than 64
    live predators in some env."""
    from predpreygrass_amd.distributed import parse_image
    from tests.test_distributed import local_rows_reference
    env = make(cfg, B, seed=4, pred_capacity=128, prey_capacity=256)
    env.reset()
    for _ in range(calls):
        env.step(random_actions=True, auto_reset=True)
    nP = env.env_state[:, _abi.ENV_N_PRED_ROWS]
    assert int(nP.max()) > 64, int(nP.max())
    # snapshot: export env B-1, import it into env 0 of a second handle, step both: same results
    other = make(cfg, B, seed=9, pred_capacity=128, prey_capacity=256)
    other.reset()
    blob = env.export_state(B - 1)
    other.import_state(blob, 0)
    other.observe() if hasattr(other, "observe") else None
    assert other.export_state(0) == blob
    # fetch == the tensors
    tables, obs_p, obs_q = env.fetch(0, B)
    for name, _, _ in env._fetch_fields():
        want = getattr(env, name)[0:B].cpu().numpy().reshape(B, -1)
        assert np.array_equal(tables[name].reshape(B, -1).view(want.dtype), want), name
    for i in range(B):
        n_p = int(nP[i])
        assert obs_p[i].shape[0] == n_p
        assert np.array_equal(np.asarray(obs_p[i]).reshape(n_p, -1), env.obs_pred[i, :n_p].cpu().numpy().reshape(n_p, -1))
    # pack
    lib = env._lib
    handles = (C.c_void_p * 1)(env._handle)
    want = local_rows_reference(env)
    need = int(lib.ppg_pack_bytes(env._handle, B, want["id_pred"].numel(), want["id_prey"].numel(), 0))
    img = torch.zeros(need + 4096, dtype=torch.uint8, device=env.device)
    assert lib.ppg_pack(handles, 1, C.c_void_p(img.data_ptr()), img.numel(), 0, env._stream()) == 0
    if env.device.type == "cuda":
        torch.cuda.synchronize()
    got = parse_image(img)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    # a handle of 64 predator rows cannot join a pack call with it (capacity-equality check)
    small = make(cfg | {"n_initial_active_predator": 40}, B, pred_capacity=64, prey_capacity=256)
    small.reset()
    mixed = (C.c_void_p * 2)(env._handle, small._handle)
    assert lib.ppg_pack(mixed, 2, C.c_void_p(img.data_ptr()), img.numel(), 0, env._stream()) == -1
    return env


def overflow_contract(make, cfg, B, calls):
    """A predator boom on 128 rows: PPG_STATUS_PRED_OVERFLOW is flagged and no env holds more than 128 predator rows."""
    env = make(cfg, B, seed=2, pred_capacity=128, prey_capacity=256)
    env.reset()
    hit = False
    for _ in range(calls):
        env.step(random_actions=True)
        es = env.env_state
        assert int(es[:, _abi.ENV_N_PRED_ROWS].max()) <= 128
        if bool((es[:, _abi.ENV_STATUS] & _abi.STATUS_PRED_OVERFLOW).any()):
            hit = True
            break
    assert hit, "no predator overflow"
    return env
