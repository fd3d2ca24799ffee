"""Randomised differential test: random configurations x partial, shuffled action dicts, the HIP
kernel source (under the wave emulator here; on the GPU in test_hip_parity.py) vs the oracle, call by
call, bit for bit.  Covers what the golden cases cannot enumerate: tiny grids, windows larger than the
grid, even observation ranges, empty populations, agents left out of the action dict
(predpreygrass_rllib_env.py:244,259 iterate over action_dict, not over agents), arbitrary dict order."""
import numpy as np
import pytest

from oracle.ppg_oracle import OracleEnv
from predpreygrass_amd.config import config_env
from predpreygrass_amd.env import PredPreyGrass
from tests.emu_backend import library


def random_config(rng):
    G = int(rng.integers(2, 31))
    cells = G * G
    P0 = int(rng.integers(0, min(12, cells // 3) + 1))
    Q0 = int(rng.integers(0, min(20, cells // 3) + 1))
    NG = int(rng.integers(0, min(60, cells - P0 - Q0) + 1))
    mode = str(rng.choice(["sparse", "sparse", "dense_energy_delta", "dense_energy_delta_plus_reproduction"]))
    kick = {"kickback_reward_predator": float(rng.choice([10.0, 3.0])), "kickback_reward_prey": float(rng.choice([10.0, 1.25]))} \
        if (mode == "sparse" and rng.random() < 0.4) else {}
    return {
        **config_env, **kick,
        "grid_size": G, "max_steps": int(rng.integers(0, 40)),
        "predator_obs_range": int(rng.integers(1, 16)), "prey_obs_range": int(rng.integers(1, 16)),
        "n_initial_active_predator": P0, "n_initial_active_prey": Q0, "initial_num_grass": NG,
        "n_possible_predators": int(rng.integers(P0, P0 + 30)), "n_possible_prey": int(rng.integers(Q0, Q0 + 40)),
        "energy_loss_per_step_predator": float(rng.choice([0.15, 0.5, 1.0, 0.0])),
        "energy_loss_per_step_prey": float(rng.choice([0.05, 0.3, 1.0])),
        "predator_creation_energy_threshold": float(rng.choice([12.0, 6.0, 5.5])),
        "prey_creation_energy_threshold": float(rng.choice([8.0, 3.5, 4.0])),
        "initial_energy_predator": float(rng.choice([5.0, 1.0])), "initial_energy_prey": float(rng.choice([3.0, 0.5])),
        "initial_energy_grass": float(rng.choice([2.0, 0.7])), "energy_gain_per_step_grass": float(rng.choice([0.04, 0.5, 0.0])),
        "reward_predator_catch_prey": float(rng.choice([0.0, 1.5])), "reward_prey_eat_grass": float(rng.choice([0.0, 0.25])),
        "reward_predator_step": float(rng.choice([0.0, -0.01])), "reward_prey_step": float(rng.choice([0.0, 0.02])),
        "penalty_prey_caught": float(rng.choice([0.0, -2.0])),
        "reproduction_reward_predator": float(rng.choice([10.0, 7.0])), "reproduction_reward_prey": float(rng.choice([10.0, 3.0])),
        "reward_mode": mode,
        **({"season_length_steps": int(rng.integers(1, 9)), "season_high_multiplier": 1.5, "season_low_multiplier": 0.5}
           if rng.random() < 0.3 else {}),
    }


def random_placement(rng, cfg):
    G = cfg["grid_size"]
    n = cfg["n_initial_active_predator"] + cfg["n_initial_active_prey"] + cfg["initial_num_grass"]
    cells = rng.choice(G * G, size=n, replace=False)
    xy = np.stack([cells // G, cells % G], axis=1).astype(np.int32)
    P, Q = cfg["n_initial_active_predator"], cfg["n_initial_active_prey"]
    return xy[:P], xy[P:P + Q], xy[P + Q:]


def run_differential(make_env, seed, max_calls=45, config_fn=random_config):
    rng = np.random.default_rng(seed)
    cfg = config_fn(rng)
    placement = random_placement(rng, cfg)
    env = make_env(cfg)
    orc = OracleEnv(cfg)
    orc.set_seed(0, 0)
    o1, _ = env.reset(options={"placement": placement})
    o2, _ = orc.reset_from_placement(*placement)
    assert list(o1) == list(o2)
    for k in o2:
        assert o1[k].tobytes() == o2[k].tobytes(), ("reset", seed, k)
    live = list(o1)
    p_act = float(rng.choice([1.0, 1.0, 0.8, 0.3]))
    shuffle = bool(rng.integers(0, 2))
    for t in range(max_calls):
        names = [a for a in live if rng.random() < p_act]
        if shuffle:
            rng.shuffle(names)
        actions = {a: int(rng.integers(0, 9)) for a in names}
        r2 = orc.step(actions)
        if orc.last_failed_spawns:
            # no free cell for a newborn: the reference raises TypeError (predpreygrass_rllib_env.py:401-405,766);
            # the oracle counts it, this implementation raises the same exception type
            with pytest.raises(TypeError):
                env.step(actions)
            return cfg
        r1 = env.step(actions)
        for i, what in enumerate(("obs", "rew", "term", "trunc")):
            assert list(r1[i]) == list(r2[i]), (seed, t, what, list(r1[i]), list(r2[i]))
            for k in r2[i]:
                a, b = r1[i][k], r2[i][k]
                if what == "obs":
                    assert a.tobytes() == b.tobytes(), (seed, t, what, k)
                elif what == "rew":
                    assert np.float64(a).tobytes() == np.float64(b).tobytes(), (seed, t, what, k, a, b)
                else:
                    assert bool(a) == bool(b), (seed, t, what, k)
        assert env.grid_world_state.tobytes() == orc.grid_world_state.tobytes(), (seed, t, "grid")
        assert env.agents == orc.agents, (seed, t, "agents")
        assert env.current_step == orc.current_step
        live = [a for a in r2[0] if not r2[2][a]]
        if r2[2]["__all__"] or r2[3]["__all__"]:
            # one more call after the end: truncation repeats, termination keeps stepping like the reference
            if r2[3]["__all__"]:
                break
    return cfg


@pytest.mark.parametrize("seed", range(40))
def test_random_config_matches_oracle_emulated(seed):
    # the oracle's spawn fallback uses env seed 0 / episode 0; so does a placement-reset env here
    run_differential(lambda cfg: PredPreyGrass(cfg, _library=library()), seed)


BIG_CONFIGS = [
    # largest observation windows (15x15 > 8 chunks per agent -> generic LDS-descriptor path), 64x64 grid, 1000 grass
    {"grid_size": 64, "predator_obs_range": 15, "prey_obs_range": 13, "initial_num_grass": 1000,
     "n_initial_active_predator": 40, "n_initial_active_prey": 100, "max_steps": 30},
    # row tables full at reset: 64 predators / 128 prey (every birth must be flagged as overflow, not corrupt state)
    {"grid_size": 40, "predator_obs_range": 7, "prey_obs_range": 9, "initial_num_grass": 300,
     "n_initial_active_predator": 64, "n_initial_active_prey": 128, "max_steps": 12,
     "n_possible_predators": 64, "n_possible_prey": 128},
    # the largest grid the LDS layout admits with 7x7 / 9x9 windows
    {"grid_size": 80, "predator_obs_range": 7, "prey_obs_range": 9, "initial_num_grass": 500,
     "n_initial_active_predator": 30, "n_initial_active_prey": 60, "max_steps": 20},
]


def run_big(make_env, cfg_over, seed=0, calls=25):
    rng = np.random.default_rng(seed)
    cfg = {**config_env, **cfg_over}
    placement = random_placement(rng, cfg)
    env = make_env(cfg)
    orc = OracleEnv(cfg)
    o1, _ = env.reset(options={"placement": placement})
    o2, _ = orc.reset_from_placement(*placement)
    assert list(o1) == list(o2) and all(o1[k].tobytes() == o2[k].tobytes() for k in o2)
    live = list(o1)
    for t in range(calls):
        actions = {a: int(rng.integers(0, 9)) for a in live}
        r2 = orc.step(actions)
        r1 = env.step(actions)
        assert list(r1[0]) == list(r2[0]), (t,)
        for k in r2[0]:
            assert r1[0][k].tobytes() == r2[0][k].tobytes(), (t, k)
            assert np.float64(r1[1][k]).tobytes() == np.float64(r2[1][k]).tobytes() and r1[2][k] == r2[2][k]
        assert env.grid_world_state.tobytes() == orc.grid_world_state.tobytes(), (t, "grid")
        live = [a for a in r2[0] if not r2[2][a]]
        if r2[2]["__all__"] or r2[3]["__all__"]:
            break


@pytest.mark.parametrize("idx", range(len(BIG_CONFIGS)))
def test_maximum_size_configs_emulated(idx):
    run_big(lambda cfg: PredPreyGrass(cfg, prey_capacity=256 if idx == 0 else None, _library=library()),
            BIG_CONFIGS[idx], seed=idx)


def test_configurations_beyond_the_limits_are_rejected_with_a_message():
    with pytest.raises(ValueError, match="LDS|grid_size"):
        PredPreyGrass({**config_env, "grid_size": 88, "predator_obs_range": 15, "prey_obs_range": 15,
                       "initial_num_grass": 4000}, _library=library())
    with pytest.raises(ValueError, match="capacities|capacity"):
        PredPreyGrass({**config_env, "n_initial_active_predator": 65}, _library=library())
