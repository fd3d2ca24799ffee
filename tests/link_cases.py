"""Scenarios of `ppg_link` (rows of one call <-> rows of the next; include/ppg.h) and of predpreygrass_amd.trajectory, shared by
the wave-emulator tests (test_link_emulated.py) and the GPU tests (test_link_gpu.py).  The reference of every check is computed on
the host from `host_tables()` / `records()`: a numpy join of the row_id tables, and a per-agent-NAME backward recursion in Python
floats.

`make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a BatchedRedQueen, both on the backend under test."""
import numpy as np
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.config import config_env
from predpreygrass_amd.red_queen import config_env_base
from predpreygrass_amd.trajectory import AgentTrajectories
from tests.pred_capacity_cases import CFG_CROSS

# short episodes (auto-resets inside a run), cheap births, predators that starve before the episode ends
CFG_BASE = {**config_env, "max_steps": 30, "predator_creation_energy_threshold": 6.0, "prey_creation_energy_threshold": 4.0,
            "energy_gain_per_step_grass": 0.2, "initial_energy_predator": 3.0}
# prey capacity 64: a small grid that cannot feed more than 64 prey
CFG_BASE_Q1 = {**CFG_BASE, "grid_size": 12, "initial_num_grass": 30}
# prey capacity 256: enough prey to use the third and fourth prey register
CFG_BASE_Q4 = {**CFG_BASE, "n_initial_active_prey": 140, "initial_num_grass": 200, "max_steps": 25}
# 128 predator rows: births cross row 64 (tests/pred_capacity_cases.py), episodes cut short
CFG_P2 = {**CFG_CROSS, "max_steps": 40}
CFG_RQ = {**config_env_base, "max_steps": 30, "predator_creation_energy_threshold": 7.0, "prey_creation_energy_threshold": 4.0,
          "reproduction_cooldown_steps": 2, "n_initial_active_type_2_predator": 4, "n_possible_type_2_predators": 500,
          "initial_energy_predator": 3.0, "energy_loss_per_step_predator": 0.12}
CFG_DRIVE = {**CFG_BASE, "enable_drive_channels": True}
WALLS = [(5, y) for y in range(3, 12)] + [(x, 15) for x in range(10, 20)]


def tables_of(env):
    """host_tables() as copies: on the CPU backend they are views of the tensors the next call overwrites."""
    return {k: v.copy() for k, v in env.host_tables().items()}


def id_join(prev, cur, b, cp, S):
    """(prev_row, next_row) of env b from the host tables of two calls: same species, same row_id, same ENV_EPISODE, both rows in
    use.  Also checks that a row_id matches at most once (ids are unique within an episode)."""
    want_prev, want_next = np.full(S, -1, np.int16), np.full(S, -1, np.int16)
    eo, en = prev["env_state"][b], cur["env_state"][b]
    if int(eo[_abi.ENV_EPISODE]) != int(en[_abi.ENV_EPISODE]):
        return want_prev, want_next
    for lo, w in ((0, _abi.ENV_N_PRED_ROWS), (cp, _abi.ENV_N_PREY_ROWS)):
        n_old, n_new = int(eo[w]), int(en[w])
        old, new = prev["row_id"][b, lo:lo + n_old], cur["row_id"][b, lo:lo + n_new]
        r, j = np.nonzero(new[:, None] == old[None, :])
        assert len(set(r.tolist())) == len(r) and len(set(j.tolist())) == len(j), (b, "a row_id occurs twice")
        want_prev[lo + r] = lo + j
        want_next[lo + j] = lo + r
    return want_prev, want_next


def in_use_mask(tables, b, cp, S):
    es = tables["env_state"][b]
    rows = np.arange(S)
    return np.where(rows < cp, rows < int(es[_abi.ENV_N_PRED_ROWS]), rows - cp < int(es[_abi.ENV_N_PREY_ROWS]))


def check_maps(env, prev, cur, got_prev, got_next, envs, tag):
    """Both maps of the envs in `envs` against the id join, and the invariants of the contract."""
    cp, S = env.pred_capacity, env.S
    for b in envs:
        want_prev, want_next = id_join(prev, cur, b, cp, S)
        assert np.array_equal(got_prev[b], want_prev), (tag, b, "prev_row")
        assert np.array_equal(got_next[b], want_next), (tag, b, "next_row")
        p, n = got_prev[b].astype(np.int64), got_next[b].astype(np.int64)
        used_now, used_old = in_use_mask(cur, b, cp, S), in_use_mask(prev, b, cp, S)
        linked = p[p >= 0]
        assert len(np.unique(linked)) == len(linked), (tag, b, "prev_row is not injective")
        assert np.array_equal(n[linked], np.nonzero(p >= 0)[0]), (tag, b, "next_row[prev_row[r]] != r")
        newborn = (cur["row_flags"][b] & _abi.ROW_NEWBORN) != 0
        assert (p[newborn & used_now] == -1).all(), (tag, b, "a newborn row is linked")
        assert (p[~used_now] == -1).all() and (n[~used_old] == -1).all(), (tag, b, "an unused row is linked")
        # both ends of a link are the same species
        assert ((p[p >= 0] < cp) == (np.nonzero(p >= 0)[0] < cp)).all(), (tag, b, "species")


def link_vs_id_join(env, n_calls, envs=None, need=("reset", "birth", "death")):
    """After every step(random_actions, auto_reset) both maps of link() equal the numpy join of the previous and the current
    host tables.  Returns the counts of auto-resets, newborn rows, died rows and links seen in the checked envs and the largest row counts."""
    envs = list(range(env.batch_size)) if envs is None else envs
    env.reset()
    p, n = env.link()
    assert bool((p == -1).all()) and bool((n == -1).all()), "link() right after reset() must link nothing"
    prev = tables_of(env)
    seen = {"reset": 0, "birth": 0, "death": 0, "links": 0, "pred_rows": 0, "prey_rows": 0}
    for t in range(n_calls):
        env.step(random_actions=True, auto_reset=True)
        p, n = env.link()
        p, n = p.cpu().numpy(), n.cpu().numpy()
        cur = tables_of(env)
        check_maps(env, prev, cur, p, n, envs, f"call {t}")
        for b in envs:
            used = in_use_mask(cur, b, env.pred_capacity, env.S)
            if int(cur["env_state"][b, _abi.ENV_FLAGS]) & _abi.ENVF_WAS_RESET:
                seen["reset"] += 1
                assert (p[b] == -1).all() and (n[b] == -1).all(), (t, b, "linked across an auto-reset")
            seen["birth"] += int(((cur["row_flags"][b] & _abi.ROW_NEWBORN) != 0)[used].sum())
            seen["death"] += int(((cur["row_flags"][b] & _abi.ROW_DIED) != 0)[used].sum())
            seen["links"] += int((p[b] >= 0).sum())
            seen["pred_rows"] = max(seen["pred_rows"], int(cur["env_state"][b, _abi.ENV_N_PRED_ROWS]))
            seen["prey_rows"] = max(seen["prey_rows"], int(cur["env_state"][b, _abi.ENV_N_PREY_ROWS]))
        prev = cur
    for k in need:
        assert seen[k] > 0, (k, seen)   # (the run must not pass vacuously)
    assert seen["links"] > 0, seen
    return seen


def link_across_rollout(env, n_rounds, K, envs=None):
    """`rollout(K)` between two link() calls: the maps are the K-step maps -- the id join across those K steps."""
    envs = list(range(env.batch_size)) if envs is None else envs
    env.reset()
    env.link()
    prev = tables_of(env)
    links = gone = 0
    for t in range(n_rounds):
        env.rollout(K, random_actions=True, auto_reset=True)
        p, n = env.link()
        p, n = p.cpu().numpy(), n.cpu().numpy()
        cur = tables_of(env)
        check_maps(env, prev, cur, p, n, envs, f"round {t}")
        for b in envs:
            links += int((p[b] >= 0).sum())
            gone += int(((n[b] == -1) & in_use_mask(prev, b, env.pred_capacity, env.S)).sum())
        prev = cur
    assert links > 0 and gone > 0, (links, gone)


def returns_vs_names(env, T, gamma, lam=0.9, envs=None):
    """T calls recorded by AgentTrajectories; returns() and gae() bit for bit against the same backward recursions run per agent
    NAME (plus episode: names restart with an auto-reset) in Python floats over the reward series of env.records()."""
    envs = list(range(env.batch_size)) if envs is None else envs
    B, S, cp = env.batch_size, env.S, env.pred_capacity
    env.reset()
    traj = AgentTrajectories(env, T)
    steps = []   # per call: {b: {(episode, name): (absolute row, reward, done)}}
    for t in range(T):
        env.step(random_actions=True, auto_reset=True)
        traj.record()
        tables = tables_of(env)
        here = {}
        for b in envs:
            ep = int(tables["env_state"][b, _abi.ENV_EPISODE])
            here[b] = {(ep, name): (r + (cp if ty else 0), float(rew), bool(term or trunc))
                       for name, ty, r, rew, term, trunc in env.records(b, tables)}
            assert len(here[b]) == int(in_use_mask(tables, b, cp, S).sum()), (t, b, "a name occurs twice")
        steps.append(here)
    assert len(traj) == T
    values = torch.rand((T, B, S), dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 4.0 - 2.0
    got_G = traj.returns(gamma).cpu().numpy()
    got_A = traj.gae(values.to(env.device), gamma, lam).cpu().numpy()
    V = values.numpy()
    want_G, want_A = np.zeros((T, B, S)), np.zeros((T, B, S))
    gl = float(gamma) * float(lam)
    n_succ = n_end = 0
    for b in envs:
        nxt = {}   # (episode, name) -> (row, G, A) at call t + 1
        for t in range(T - 1, -1, -1):
            now = {}
            for key, (row, rew, done) in steps[t][b].items():
                if not done and key in nxt:
                    row1, g1, a1 = nxt[key]
                    g_succ, a_succ, v_succ = g1, a1, float(V[t + 1, b, row1])
                    n_succ += 1
                else:
                    g_succ = a_succ = v_succ = 0.0
                    n_end += 1
                g = rew + g_succ * float(gamma)
                a = ((rew + v_succ * float(gamma)) - float(V[t, b, row])) + a_succ * gl
                now[key] = (row, g, a)
                want_G[t, b, row], want_A[t, b, row] = g, a
            nxt = now
    assert n_succ > 0 and n_end > T * len(envs), (n_succ, n_end)
    assert np.abs(want_G[:, envs]).max() > 0.0, "no reward was seen: the comparison would be empty"
    assert got_G[:, envs].tobytes() == want_G[:, envs].tobytes(), "returns()"
    assert got_A[:, envs].tobytes() == want_A[:, envs].tobytes(), "gae()"
    return traj


def invalidation(env, set_placement=True):
    """import_state into env 0: the next link() gives -1 for env 0 (and still links the others); reset(): -1 for all envs;
    set_placement (ppg_reset_from_state): likewise.  Either output pointer may be NULL."""
    import ctypes as C
    B = env.batch_size
    assert B >= 2
    env.reset()
    env.link()
    for _ in range(3):
        env.step(random_actions=True)
        p, n = env.link()
    assert bool((p[0] >= 0).any()) and bool((p[1] >= 0).any())
    blob = env.export_state(1)
    env.import_state(blob, 0)
    p, n = env.link()
    assert bool((p[0] == -1).all()) and bool((n[0] == -1).all()), "env 0 was imported: nothing may link"
    for b in range(1, B):
        assert bool((p[b] >= 0).any()) and bool((n[b] >= 0).any()), (b, "the other envs keep their links")
    prev = tables_of(env)
    env.step(random_actions=True)
    p, n = env.link()
    check_maps(env, prev, tables_of(env), p.cpu().numpy(), n.cpu().numpy(), range(B), "after import")
    assert bool((p[0] >= 0).any())
    # either pointer may be NULL: the other map is written as usual.  No step lies between this call and the last one, so every row
    # in use links to itself -- except the rows still flagged NEWBORN, which never link backwards
    cur = tables_of(env)
    cp, S = env.pred_capacity, env.S
    want = np.full((B, S), -1, np.int16)
    for b in range(B):
        keep = in_use_mask(cur, b, cp, S) & ((cur["row_flags"][b] & _abi.ROW_NEWBORN) == 0)
        want[b, keep] = np.nonzero(keep)[0]
    n.fill_(7)
    p.fill_(7)
    assert env._lib.ppg_link(env._handle, None, C.c_void_p(n.data_ptr()), env._stream()) == 0
    assert np.array_equal(n.cpu().numpy(), want) and bool((p == 7).all())
    n.fill_(7)
    assert env._lib.ppg_link(env._handle, C.c_void_p(p.data_ptr()), None, env._stream()) == 0
    assert np.array_equal(p.cpu().numpy(), want) and bool((n == 7).all())
    assert env._lib.ppg_link(env._handle, None, None, env._stream()) == 0
    env.step(random_actions=True)
    env.reset()
    p, n = env.link()
    assert bool((p == -1).all()) and bool((n == -1).all()), "reset(): nothing may link"
    if set_placement:
        env.step(random_actions=True)
        p, n = env.link()
        assert bool((p >= 0).any())
        env.reset()   # (a valid placement to hand back: rows 0..P0-1 / cp..cp+Q0-1 and the grass table)
        env.link()
        t = tables_of(env)

        def pairs(v):
            v = v.astype(np.int64) & 0xFFFF
            return np.stack([v >> 8, v & 255], axis=-1)
        env.set_placement(pairs(t["row_xy"][:, : env.P0]), pairs(t["row_xy"][:, cp: cp + env.Q0]), pairs(t["grass_xy"][:, : env.n_grass]))
        p, n = env.link()
        assert bool((p == -1).all()) and bool((n == -1).all()), "set_placement(): nothing may link"
