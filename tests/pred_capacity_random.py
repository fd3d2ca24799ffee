"""Random configurations for environments with 128 predator rows (the one-wave ppg_*_p2q<NQ>g / ppg2_*_p2q<NQ>g kernels), shared by
the wave-emulator tests (test_pred_capacity_random_emulated.py) and the GPU tests (test_pred_capacity_random_gpu.py).  No tests of its
own.  Every comparison is tobytes() equality against the C oracles (oracle/ppg_oracle.c, oracle/rq_oracle.c); there are no tolerances.

The two generators start from the ones of test_random_configs.py / test_rq_random_configs.py (windows 1..15, reward modes, kickback,
seasonal keys, energies, thresholds) and move the populations to where only a handle with pred_capacity=128 can go: 65..128 initial
predators on grids of 12..30.  The dict-class differentials are the run_differential functions of those two files, called with these
generators (`config_fn`).  `CoverageEnv` / `CoverageEnvRQ` are the oracle dressed as the class under test: run through the same
run_differential they drive the oracle alone over a seed set and count what the set reaches."""
import numpy as np
import torch

from oracle.ppg_oracle import OracleEnv
from oracle.rq_oracle import RQOracleEnv
from predpreygrass_amd import _abi
from tests import pred_capacity_cases as cases
from tests import test_random_configs as T1
from tests import test_rq_random_configs as T2
from tests.parity_utils import compare_env_with_oracle

# seed sets: the emulator's and the GPU's are disjoint, together 70 base-family + 60 second-generation configurations.  The bases were
# chosen with the oracle alone (coverage_of below, the conditions of test_seed_sets_reach_what_they_are_for); that test's comment has
# the counted figures.
EMU_BASE_SEEDS = range(0, 40)
GPU_BASE_SEEDS = range(50, 80)
EMU_RQ_SEEDS = range(0, 30)
GPU_RQ_SEEDS = range(190, 220)
# the observation-dtype rollouts: the configurations random_config_p2 draws from these seeds, picked by what they draw -- windows
# 6/14 on a grid of 12 (dense), 1/2 (dense + reproduction), 13/1 on a grid of 12 (kickback), 15/8 (seasonal), 12/15 with max_steps 0,
# 9/11 on a grid of 30 with 200 patches; three with prey capacity 128, three with 256
DTYPE_SEEDS = (9001, 9003, 9014, 9019, 9035, 9002)
N_DTYPE_CONFIGS = len(DTYPE_SEEDS)


def random_config_p2(rng):
    """-> (config, prey capacity) of the base family with 65..128 initial predators."""
    cfg = T1.random_config(rng)
    G = int(rng.integers(12, 31))
    cells = G * G
    P0 = int(rng.integers(65, min(128, cells // 2) + 1))
    cap = int(rng.choice([128, 256]))
    Q0 = int(rng.integers(0, min(cap - 20, (cells - P0) // 2) + 1))
    # (above 255 patches the host forces 16-bit cell maps: 200 keeps ppg_*_p2q2g on its 8-bit maps, value-table entries 65..128 included)
    NG = int(rng.integers(0, min(200, cells - P0 - Q0) + 1))
    cfg.update(
        grid_size=G, n_initial_active_predator=P0, n_initial_active_prey=Q0, initial_num_grass=NG,
        # ids are never reused: the pools keep every run inside the row tables (the overflow contract has its own test)
        n_possible_predators=int(rng.integers(P0, 129)), n_possible_prey=int(rng.integers(Q0, cap + 1)),
        # (the inherited 0..40 ends a third of the runs within six calls; 0 = truncation right after reset)
        max_steps=0 if rng.random() < 0.1 else int(rng.integers(12, 41)),
        # cheap births twice as often as dear ones: newborns into rows >= 64
        predator_creation_energy_threshold=float(rng.choice([5.5, 6.0, 5.5, 6.0, 12.0, 12.0])))
    return cfg, cap


def random_config_rq_p2(rng):
    """-> (config, prey capacity) of the second generation without walls: both predator types, 65..120 initial predators."""
    cfg = T2.random_config(rng)
    G = int(rng.integers(12, 29))
    cells = G * G
    P = int(rng.integers(65, min(120, cells // 2) + 1))
    p1 = int(rng.integers(1, P))            # both types: 1..P-1 of type 1
    p2 = P - p1
    cap = int(rng.choice([128, 256]))
    q1, q2 = cfg["n_initial_active_type_1_prey"], cfg["n_initial_active_type_2_prey"]
    NG = min(cfg["initial_num_grass"], cells - P - q1 - q2)
    # id pools: predators sum to <= 128, prey to <= the prey capacity (ids are never reused)
    room_p = 128 - P
    e1 = int(rng.integers(0, room_p + 1))
    e2 = int(rng.integers(0, room_p - e1 + 1))
    room_q = min(40, cap - q1 - q2)
    f1 = int(rng.integers(0, room_q + 1))
    f2 = int(rng.integers(0, room_q - f1 + 1))
    cfg.update(
        grid_size=G, initial_num_grass=NG,
        max_steps=0 if rng.random() < 0.1 else int(rng.integers(12, 45)),   # (0 = truncation right after reset, about one seed in ten)
        n_initial_active_type_1_predator=p1, n_initial_active_type_2_predator=p2,
        n_possible_type_1_predators=p1 + e1, n_possible_type_2_predators=p2 + e2,
        n_possible_type_1_prey=q1 + f1, n_possible_type_2_prey=q2 + f2)
    return cfg, cap


def differential_base(make_env, seed):
    """tests.test_random_configs.run_differential with random_config_p2: `make_env(cfg, prey_capacity)` builds the dict class under
    test with 128 predator rows.  Returns the config."""
    drawn = {}

    def config_fn(rng):
        cfg, drawn["cap"] = random_config_p2(rng)
        return cfg
    return T1.run_differential(lambda cfg: make_env(cfg, drawn["cap"]), seed, config_fn=config_fn)


def differential_rq(make_env, seed):
    """The same for the second generation (tests.test_rq_random_configs.run_differential with random_config_rq_p2)."""
    drawn = {}

    def config_fn(rng):
        cfg, drawn["cap"] = random_config_rq_p2(rng)
        return cfg
    return T2.run_differential(lambda cfg: make_env(cfg, drawn["cap"]), seed, config_fn=config_fn)


def dtype_config(i):
    return random_config_p2(np.random.default_rng(DTYPE_SEEDS[i]))


def rollout_dtype_vs_oracle(make, cfg, prey_cap, dtype, seed0, n_calls):
    """BatchedPredPreyGrass, B = 3, float32 / bfloat16 observation rows: device reset, device random actions, auto-reset; every env
    compared with its own oracle on every call (compare_env_with_oracle: the oracle's float64 block .astype(float32), or
    .float().bfloat16() as int16 bit patterns).  Returns the largest number of predator rows seen."""
    env = make(cfg, 3, pred_capacity=128, prey_capacity=prey_cap, obs_dtype=dtype)
    assert env.obs_pred.dtype == dtype and env.step_kernel_name().endswith(f"p2q{env.prey_capacity // 64}g")
    oracles = [OracleEnv(cfg) for _ in range(3)]
    cases._start(env, seed0)
    most = 0
    for t in range(n_calls):
        env.step(random_actions=True, auto_reset=True)
        tables = env.host_tables()
        for b, orc in enumerate(oracles):
            assert orc.rollout_random((seed0 + b) & (2 ** 64 - 1), 1) == 1
            assert orc._out.failed_spawns == 0, "the oracle ran out of cells: pick another configuration"
            st = int(tables["env_state"][b][_abi.ENV_STATUS])
            assert st & ~_abi.STATUS_FALLBACK_SPAWN == 0, (t, b, "status", st)
            compare_env_with_oracle(env, b, orc, tables, tag=f"{dtype} call {t}")
            most = max(most, int(tables["env_state"][b][_abi.ENV_N_PRED_ROWS]))
    return env, most


def observe_matches(env):
    """observe() on a handle with more than 64 predator rows in some env rewrites every live observation row in use with the bits the
    step left there, and changes no table.  (Rows that terminated in the last call are in use but not live: ppg_observe, include/ppg.h,
    recomputes "all live rows" and leaves those alone.)"""
    nP = env.env_state[:, _abi.ENV_N_PRED_ROWS]
    assert int(nP.max()) > 64, int(nP.max())
    names = ["row_xy", "row_energy", "row_id", "row_key", "row_cumrew", "row_flags", "row_reward", "row_parent", "row_lastrep",
             "grass_xy", "grass_energy", "env_state", "env_seed"]
    before = {n: getattr(env, n).clone() for n in names}
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[env.obs_pred.element_size()]
    obs_p, obs_q = env.obs_pred.clone(), env.obs_prey.clone()
    env.obs_pred.view(bits).fill_(0x55)    # (a pattern no observation holds: 0x55.. is neither 0 nor an energy of these runs)
    env.obs_prey.view(bits).fill_(0x55)
    env.observe()
    for n in names:
        assert torch.equal(getattr(env, n), before[n]), n
    cp = env.pred_capacity
    rows = torch.arange(env.S, device=env.device)[None, :]
    nQ = env.env_state[:, _abi.ENV_N_PREY_ROWS]
    live = (env.row_flags & _abi.ROW_DIED) == 0
    used_p = (rows[:, :cp] < nP[:, None]) & live[:, :cp]
    used_q = (rows[:, : env.prey_capacity] < nQ[:, None]) & live[:, cp:]
    assert int(used_p.sum()) > 64
    assert torch.equal(env.obs_pred.view(bits)[used_p], obs_p.view(bits)[used_p]), "predator rows"
    assert torch.equal(env.obs_prey.view(bits)[used_q], obs_q.view(bits)[used_q]), "prey rows"


def env_with_many_predators(make, cfg, calls, seed, **kw):
    """A handle stepped `calls` times from a device reset (random actions, auto-reset) for observe_matches."""
    env = make(cfg, 3, seed=seed, pred_capacity=128, **kw)
    env.reset()
    for _ in range(calls):
        env.step(random_actions=True, auto_reset=True)
    return env


# ---------------------------------------------------------------------------------------------------------------------------------
# what a seed set reaches, counted on the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------

class _Counts:
    def __init__(self):
        self.calls = 0
        self.births_reg1 = 0          # predator newborns whose row is >= 64 (>= 64 predator rows in use before them)
        self.deaths_both = 0          # calls in which predators die in rows < 64 and in rows >= 64
        self.fallback = 0             # spawns through the fallback (STATUS_FALLBACK_SPAWN on the kernel side)
        self.failed = False           # the run ended in the last_failed_spawns early return
        self.partial = False          # some call left live agents out of the dict
        self.shuffled = False         # some call's dict order differed from row order within a species
        self.most = 0                 # largest number of predator rows of a call

    def call(self, live, actions, obs, term, species_of, orc):
        """One call: `live` the names alive before it in row order, `obs` / `term` what it returned."""
        self.calls += 1
        self.fallback += orc.last_fallback_spawns
        self.partial |= any(a not in actions for a in live)
        row = {a: i for i, a in enumerate(live)}
        for sp in (0, 1):
            r = [row[a] for a in actions if a in row and species_of(a) == sp]
            self.shuffled |= r != sorted(r)
        if orc.last_failed_spawns:
            self.failed = True
            return
        was = set(live)
        preds = [a for a in obs if species_of(a) == 0]   # the call's predator rows: survivors in row order, then newborns
        self.most = max(self.most, len(preds))
        self.births_reg1 += sum(1 for i, a in enumerate(preds) if a not in was and i >= 64)
        died = [i for i, a in enumerate(preds) if term[a]]
        self.deaths_both += bool(died) and died[0] < 64 <= died[-1]


class CoverageEnv(OracleEnv):
    """The oracle with the dict class's interface, for tests.test_random_configs.run_differential: the differential then compares the
    oracle with itself (never fails) and `counts` says what the seed reached."""

    def __init__(self, cfg, prey_cap):
        super().__init__(cfg)
        self.set_seed(0, 0)
        self.counts, self.cfg, self.prey_cap = _Counts(), cfg, prey_cap

    def reset(self, *, seed=None, options=None):
        obs, info = self.reset_from_placement(*options["placement"])
        self._live = list(obs)
        return obs, info

    def step(self, actions):
        r = super().step(actions)
        self.counts.call(self._live, actions, r[0], r[2], lambda a: int(a.startswith("prey")), self)
        if self.last_failed_spawns:
            raise TypeError("no free cell for a newborn")
        self._live = [a for a in r[0] if not r[2][a]]
        return r


class CoverageEnvRQ(RQOracleEnv):
    """The same for tests.test_rq_random_configs.run_differential (the env draws its reproduction uniforms from the PCG64 stream that
    reset(seed) seeds, RQ:91)."""

    def __init__(self, cfg, prey_cap):
        super().__init__(cfg)
        self.set_seed(0, 0)
        self.counts, self.cfg, self.prey_cap = _Counts(), cfg, prey_cap
        ar = (int(self.config["type_1_action_range"]) ** 2, int(self.config["type_2_action_range"]) ** 2)

        class _Spaces(dict):
            def __missing__(self, name):
                return type("Discrete", (), {"n": ar[int(name[5]) - 1]})
        self.action_spaces = _Spaces()

    def reset(self, *, seed=None, options=None):
        self._stream = np.random.default_rng(seed)
        obs, info = self.reset_from_placement(*options["placement"])
        self._live = list(obs)
        return obs, info

    def step(self, actions):
        state = self._stream.bit_generator.state
        u = self._stream.random(2 * len(self._live) + 2)
        r = super().step(actions, uniforms=u)
        self._stream.bit_generator.state = state
        self._stream.bit_generator.advance(self.last_draws)
        self.counts.call(self._live, actions, r[0], r[2], lambda a: int("prey" in a), self)
        if self.last_failed_spawns:
            raise TypeError("no free cell for a newborn")
        self._live = [a for a in r[0] if not r[2][a]]
        return r

    _next_idx = property(lambda self: dict(enumerate(self.next_ids)))

    @property
    def agent_energies(self):   # (with the two dicts run_differential reads beside it, built once per call)
        st = {a: s for a in self.agents if (s := self.agent_state(a)) is not None}
        self.cumulative_rewards = {a: s["cumulative_reward"] for a, s in st.items()}
        self.agent_last_reproduction = {a: s["last_reproduction"] for a, s in st.items()}
        return {a: s["energy"] for a, s in st.items()}


def coverage_of(family, seeds):
    """[(cfg, prey capacity, counts)] of every seed of a set, from the oracle alone."""
    out = []
    for seed in seeds:
        made = []

        def mk(cfg, cap):
            made.append((CoverageEnvRQ if family == "rq" else CoverageEnv)(cfg, cap))
            return made[-1]
        (differential_rq if family == "rq" else differential_base)(mk, seed)
        out.append((made[0].cfg, made[0].prey_cap, made[0].counts))
    return out


def check_coverage(family, seeds):
    """The conditions a seed set has to meet (a random suite that silently stops reaching a case is worthless).  Returns the counted
    figures."""
    cov = coverage_of(family, seeds)
    n = len(cov)
    cfgs = [c for c, _, _ in cov]
    fig = {}
    for sp in ("predator", "prey"):
        w = [c[f"{sp}_obs_range"] for c in cfgs]
        fig[f"{sp} windows 1/15/even"] = (w.count(1), w.count(15), sum(1 for x in w if x % 2 == 0))
        assert 1 in w and 15 in w and any(x % 2 == 0 for x in w), (sp, sorted(set(w)))
    fig["window wider than the grid"] = sum(1 for c in cfgs if max(c["predator_obs_range"], c["prey_obs_range"]) > c["grid_size"])
    assert fig["window wider than the grid"] >= 1
    if family == "base":
        modes = [c["reward_mode"] for c in cfgs]
        fig["reward modes"] = {m: modes.count(m) for m in ("sparse", "dense_energy_delta", "dense_energy_delta_plus_reproduction")}
        assert all(fig["reward modes"].values()), fig["reward modes"]
        kick = [("kickback_reward_predator" in c, k.shuffled) for c, _, k in cov]
        fig["kickback"] = sum(1 for a, _ in kick if a)
        fig["kickback with a shuffled dict"] = sum(1 for a, b in kick if a and b)
        assert fig["kickback"] >= 1 and fig["kickback with a shuffled dict"] >= 1
        fig["seasonal"] = sum(1 for c in cfgs if "season_length_steps" in c)
        assert fig["seasonal"] >= 1
        fig["partial dicts"] = sum(1 for _, _, k in cov if k.partial)
        assert fig["partial dicts"] >= 1
    caps = [cap for _, cap, _ in cov]
    fig["prey capacity 128/256"] = (caps.count(128), caps.count(256))
    assert 128 in caps and 256 in caps
    fig["max_steps == 0"] = sum(1 for c in cfgs if c["max_steps"] == 0)
    assert fig["max_steps == 0"] >= 1
    fig["predator births into rows >= 64"] = sum(k.births_reg1 for _, _, k in cov)
    assert fig["predator births into rows >= 64"] >= 20
    fig["calls with predator deaths in both registers"] = sum(k.deaths_both for _, _, k in cov)
    assert fig["calls with predator deaths in both registers"] >= 1
    fig["fallback spawns"] = sum(k.fallback for _, _, k in cov)
    assert fig["fallback spawns"] >= 1
    fig["seeds with >= 10 calls"] = sum(1 for _, _, k in cov if k.calls >= 10)
    assert fig["seeds with >= 10 calls"] >= {30: 25, 40: 33}[n], (fig["seeds with >= 10 calls"], n)
    fig["seeds ending in a failed spawn"] = sum(1 for _, _, k in cov if k.failed)
    assert fig["seeds ending in a failed spawn"] <= n // 10
    return fig

