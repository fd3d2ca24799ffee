"""Scenarios of `ppg_backward` (returns and GAE over a recorded horizon in one launch; include/ppg.h), `env.backward()` and
`AgentTrajectories.returns_and_gae()`, shared by the wave-emulator tests (test_backward_emulated.py) and the GPU tests
(test_backward_gpu.py).

The reference is `reference()`: a numpy float64 recursion written from the formulas of include/ppg.h -- per step one
`np.take_along_axis` and `np.where`, a multiply and an add as two numpy operations (two roundings).  It does not use
predpreygrass_amd.trajectory.  Every comparison is `tobytes() == tobytes()`.

`make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a BatchedRedQueen, both on the backend under test."""
import ctypes as C
import functools

import numpy as np
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.trajectory import AgentTrajectories
from tests.link_cases import CFG_BASE, CFG_BASE_Q1, CFG_P2, CFG_RQ, in_use_mask, tables_of

GAMMA, LAM = 0.97, 0.9
# every (pred_capacity, prey_capacity) ppg_create takes with a different S / 64 (2, 3, 4, 5, 6) and a config that fits it
CFG_P2_Q2 = {**CFG_P2, "n_initial_active_prey": 100}   # (the initial prey of CFG_P2 need more than 128 rows)
CAPACITIES = [(64, 64, CFG_BASE_Q1), (64, 128, CFG_BASE), (128, 128, CFG_P2_Q2), (64, 256, CFG_BASE), (128, 256, CFG_P2)]
HORIZONS = [1, 2, 3, 33]   # 1: no successor at all; 2: the first gather


def outside(S):
    """next_row values that mean "no successor" like -1."""
    return (S, S + 7, -2, 32767, -32768)


def reference(reward, next_row, in_use, terminated, truncated, values, gamma, lam):
    """(G, A) float64 [T,B,S]; A is None without values."""
    T, B, S = reward.shape
    gamma, gl = float(gamma), float(gamma) * float(lam)
    G, A = np.zeros((T, B, S)), (np.zeros((T, B, S)) if values is not None else None)
    V = None if values is None else values.astype(np.float64)   # (float32 widens exactly)
    zero = np.zeros((B, S))
    with np.errstate(invalid="ignore"):   # NaN words in rows not in use take part in the arithmetic and are selected away
        for t in range(T - 1, -1, -1):
            used = in_use[t].astype(bool)
            nx = next_row[t].astype(np.int64)
            g_succ = a_succ = v_succ = zero
            if t + 1 < T:
                has = used & ~terminated[t].astype(bool) & ~truncated[t].astype(bool) & (nx >= 0) & (nx < S)
                idx = np.where(has, nx, 0)
                g_succ = np.where(has, np.take_along_axis(G[t + 1], idx, 1), 0.0)
                if V is not None:
                    a_succ = np.where(has, np.take_along_axis(A[t + 1], idx, 1), 0.0)
                    v_succ = np.where(has, np.take_along_axis(V[t + 1], idx, 1), 0.0)
            gm = g_succ * gamma
            G[t] = np.where(used, reward[t] + gm, 0.0)
            if V is not None:
                vm = v_succ * gamma
                delta = (reward[t] + vm) - V[t]
                am = a_succ * gl
                A[t] = np.where(used, delta + am, 0.0)
    return G, A


@functools.lru_cache(maxsize=None)
def synthetic(cp, cq, T, B, seed):
    """A seeded synthetic trajectory as a dict of numpy arrays (read-only: shared between tests), its reference outputs and the
    counts the non-vacuity asserts need."""
    S = cp + cq
    rng = np.random.default_rng(seed)
    in_use = np.zeros((T, B, S), bool)
    for t in range(T):
        for b in range(B):
            # 0: both species at full capacity, 1: no predator, 3: no prey (from the third step on: the two-step cases need both species
            # at both steps to link across the species boundary), else random counts
            mode = (3 * t + b) % 5
            n_pred = cp if mode == 0 else 0 if mode == 1 and t >= 2 else int(rng.integers(1, cp + 1))
            n_prey = cq if mode == 0 else 0 if mode == 3 and t >= 2 else int(rng.integers(1, cq + 1))
            in_use[t, b, :n_pred] = True
            in_use[t, b, cp:cp + n_prey] = True
    # rows not in use: any word at all (in [-1, S)); rows in use: a random injective partial map into the next step's rows in use
    next_row = rng.integers(-1, S, (T, B, S)).astype(np.int16)
    next_row[in_use] = -1
    resets = 0
    for t in range(T - 1):
        for b in range(B):
            if (t + 2 * b) % 7 == 5:   # a reset between the two calls: nothing links
                resets += 1
                continue
            src, dst = rng.permutation(np.nonzero(in_use[t, b])[0]), rng.permutation(np.nonzero(in_use[t + 1, b])[0])
            k = min(len(src), len(dst))
            k = k - int(rng.integers(0, k // 4 + 1))   # (some agents are gone, some rows of the next step are newborns)
            next_row[t, b, src[:k]] = dst[:k]
    next_row[T - 1][in_use[T - 1]] = rng.integers(-1, S, int(in_use[T - 1].sum())).astype(np.int16)   # the last step's links are never taken
    terminated, truncated = rng.random((T, B, S)) < 0.10, rng.random((T, B, S)) < 0.05   # (rows not in use too: ignored there)
    reward = rng.normal(size=(T, B, S))
    pick = rng.random((T, B, S))
    reward[pick < 0.1] = -0.0
    reward[(pick >= 0.1) & (pick < 0.2)] = 0.0
    values = rng.normal(size=(T, B, S)).astype(np.float32).astype(np.float64)   # (representable in float32: one set for both dtypes)
    reward[~in_use] = np.nan
    values[~in_use] = np.nan
    case = dict(reward=reward, next_row=next_row, in_use=in_use, terminated=terminated, truncated=truncated, values=values)
    for v in case.values():
        v.setflags(write=False)
    # what the generated data holds (steps with a next step only)
    nx = next_row[:-1].astype(np.int64)
    flagged = terminated[:-1] | truncated[:-1]
    taken = in_use[:-1] & ~flagged & (nx >= 0)
    rows = np.broadcast_to(np.arange(S), nx.shape)
    stats = dict(taken=int(taken.sum()), ends=int(in_use.sum()) - int(taken.sum()), resets=resets,
                 flagged_with_link=int((in_use[:-1] & flagged & (nx >= 0)).sum()),
                 down=int((taken & (rows >= 64) & (nx < 64)).sum()), up=int((taken & (rows < 64) & (nx >= 64)).sum()),
                 high=int((taken & ((rows >= 320) | (nx >= 320))).sum()),
                 neg_zero=int((np.signbit(reward) & (reward == 0.0) & in_use).sum()))
    want = reference(reward, next_row, in_use, terminated, truncated, values, GAMMA, LAM)
    for v in want:
        v.setflags(write=False)
    return case, want, stats


def check_not_vacuous(stats, T, S):
    assert stats["ends"] > 0 and stats["neg_zero"] > 0, stats
    if T == 1:
        return
    assert stats["taken"] > 0 and stats["flagged_with_link"] > 0 and stats["down"] > 0 and stats["up"] > 0, stats
    if S == 384:
        assert stats["high"] > 0, stats
    if T >= 33:
        assert stats["resets"] > 0, stats


def to_device(env, case, **replace):
    return {k: torch.from_numpy(np.array(replace.get(k, v))).to(env.device) for k, v in case.items()}


def backward(env, d, values=None, **kw):
    return env.backward(d["reward"], d["next_row"], d["in_use"], d["terminated"], d["truncated"], GAMMA, LAM, values=values, **kw)


def same(got, want):
    return got.cpu().numpy().tobytes() == want.tobytes()


def check_outputs(env, case, want, tag):
    """The four required outcomes against the reference, +0.0 in rows not in use, no NaN."""
    wantG, wantA = want
    d = to_device(env, case)
    G, none = backward(env, d)
    assert none is None and same(G, wantG), (tag, "returns only")
    none, A = backward(env, d, values=d["values"], returns=False)
    assert none is None and same(A, wantA), (tag, "advantages only")
    G2, A2 = backward(env, d, values=d["values"])
    assert same(G2, wantG) and same(A2, wantA), (tag, "both in one call")
    G3, A3 = backward(env, d, values=d["values"].to(torch.float32))
    assert same(G3, wantG) and same(A3, wantA), (tag, "float32 values")
    unused = ~case["in_use"]
    for x in (wantG, wantA):   # (the outputs are these bytes)
        assert not np.isnan(x).any(), tag
        assert (x[unused].view(np.int64) == 0).all(), (tag, "a row not in use is not +0.0")


def synthetic_case(make, cp, cq, cfg, T, B, seed=None):
    env = make(cfg, B, pred_capacity=cp, prey_capacity=cq)
    assert env.S == cp + cq
    case, want, stats = synthetic(cp, cq, T, B, 1000 * T + cp + cq if seed is None else seed)
    check_not_vacuous(stats, T, env.S)
    check_outputs(env, case, want, (cp, cq, T, B))


def out_of_range_links(make):
    """next_row values of S, S + 7, -2, 32767 and -32768 in rows in use behave as -1."""
    cp, cq, cfg = CAPACITIES[-1]
    T, B = 5, 3
    env = make(cfg, B, pred_capacity=cp, prey_capacity=cq)
    case, _, _ = synthetic(cp, cq, T, B, 77)
    S = cp + cq
    nx = case["next_row"].copy()
    taken = case["in_use"] & ~case["terminated"] & ~case["truncated"] & (nx >= 0)
    taken[-1] = False
    t, b, r = np.nonzero(taken)
    assert len(t) > 50
    hit = np.arange(len(t)) % 3 == 0   # a third of the links that were taken
    bad = np.array(outside(S), np.int64)[np.arange(int(hit.sum())) % 5].astype(np.int16)
    nx[t[hit], b[hit], r[hit]] = bad
    cut = nx.copy()
    cut[t[hit], b[hit], r[hit]] = -1
    args = [case[k] for k in ("in_use", "terminated", "truncated", "values")]
    want = reference(case["reward"], cut, *args, GAMMA, LAM)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, reference(case["reward"], nx, *args, GAMMA, LAM)))
    assert want[0].tobytes() != synthetic(cp, cq, T, B, 77)[1][0].tobytes(), "cutting the links changed nothing"
    d = to_device(env, case, next_row=nx)
    G, A = backward(env, d, values=d["values"])
    assert same(G, want[0]) and same(A, want[1])


def recorded(env, n_steps=40, envs=None, need_pred_rows=0):
    """n_steps random-action steps with auto-reset recorded by AgentTrajectories: returns_and_gae() against the numpy recursion over
    the stored tensors and against returns_torch() / gae_torch(); returns() / gae() are the same tensors."""
    envs = list(range(env.batch_size)) if envs is None else envs
    cp, S = env.pred_capacity, env.S
    env.reset()
    traj = AgentTrajectories(env, n_steps)
    seen = {"reset": 0, "birth": 0, "death": 0, "pred_rows": 0}
    for _ in range(n_steps):
        env.step(random_actions=True, auto_reset=True)
        traj.record()
        cur = tables_of(env)
        for b in envs:
            used = in_use_mask(cur, b, cp, S)
            seen["reset"] += bool(int(cur["env_state"][b, _abi.ENV_FLAGS]) & _abi.ENVF_WAS_RESET)
            seen["birth"] += int(((cur["row_flags"][b] & _abi.ROW_NEWBORN) != 0)[used].sum())
            seen["death"] += int(((cur["row_flags"][b] & _abi.ROW_DIED) != 0)[used].sum())
            seen["pred_rows"] = max(seen["pred_rows"], int(cur["env_state"][b, _abi.ENV_N_PRED_ROWS]))
    assert seen["reset"] > 0 and seen["birth"] > 0 and seen["death"] > 0 and seen["pred_rows"] > need_pred_rows, seen
    values = torch.rand((n_steps, env.batch_size, S), dtype=torch.float64, generator=torch.Generator().manual_seed(9)) * 4.0 - 2.0
    G, A = traj.returns_and_gae(values.to(env.device), GAMMA, LAM)
    stored = [getattr(traj, k).cpu().numpy() for k in ("reward", "next_row", "in_use", "terminated", "truncated")]
    wantG, wantA = reference(*stored, values.numpy(), GAMMA, LAM)
    assert np.abs(wantG).max() > 0.0 and (stored[1] >= 0).any(), "nothing was recorded: the comparison would be empty"
    assert same(G, wantG), "returns_and_gae: returns"
    assert same(A, wantA), "returns_and_gae: advantages"
    assert same(traj.returns_torch(GAMMA), wantG) and same(traj.gae_torch(values.to(env.device), GAMMA, LAM), wantA), "the torch recursion"
    assert same(traj.returns(GAMMA), wantG) and same(traj.gae(values.to(env.device), GAMMA, LAM), wantA)
    # float16 values go in through float32 (exact); an empty trajectory gives empty tensors without a launch
    half = values.to(torch.float16)
    assert same(traj.gae(half.to(env.device), GAMMA, LAM), reference(*stored, half.to(torch.float64).numpy(), GAMMA, LAM)[1])
    traj.clear()
    G0, A0 = traj.returns_and_gae(values[:0].to(env.device), GAMMA, LAM)
    assert tuple(G0.shape) == tuple(A0.shape) == (0, env.batch_size, S) and G0.dtype == A0.dtype == torch.float64
    assert tuple(traj.returns(GAMMA).shape) == (0, env.batch_size, S)
    return seen


def argument_checking(env, other_device):
    """Every PPG_EINVAL case of ppg_backward returns non-zero, says why and launches nothing; the Python wrapper raises ValueError
    on a wrong shape, dtype, device or a non-contiguous input."""
    T, B, S = 2, env.batch_size, env.S
    d = dict(reward=torch.zeros((T, B, S), dtype=torch.float64), next_row=torch.full((T, B, S), -1, dtype=torch.int16),
             in_use=torch.ones((T, B, S), dtype=torch.bool), terminated=torch.zeros((T, B, S), dtype=torch.bool),
             truncated=torch.zeros((T, B, S), dtype=torch.bool), values=torch.zeros((T, B, S), dtype=torch.float64))
    d = {k: v.to(env.device) for k, v in d.items()}
    G, A = (torch.full((T, B, S), 7.0, dtype=torch.float64, device=env.device) for _ in range(2))

    def raw(n_steps=T, values="values", dtype=_abi.F64, out=(True, True), **null):
        p = {k: (None if k in null else C.c_void_p(v.data_ptr())) for k, v in d.items()}
        return env._lib.ppg_backward(env._handle, n_steps, p["reward"], p["next_row"], p["in_use"], p["terminated"], p["truncated"],
                                     p[values] if values else None, dtype, GAMMA, LAM,
                                     C.c_void_p(G.data_ptr()) if out[0] else None, C.c_void_p(A.data_ptr()) if out[1] else None, env._stream())
    refused = [dict(n_steps=0), dict(n_steps=-3), dict(out=(False, False)), dict(values=None, out=(True, True)),
               dict(values=None, out=(False, True)), dict(dtype=2), dict(dtype=-1)] + [{k: None} for k in d if k != "values"]
    for kw in refused:
        assert raw(**kw) != 0, kw
        assert b"ppg_backward" in env._lib.ppg_last_error(env._handle), kw
    if env.device.type == "cuda":
        torch.cuda.synchronize()
    assert bool((G == 7.0).all()) and bool((A == 7.0).all()), "a refused call wrote to its outputs"
    assert raw() == 0 and raw(values=None, out=(True, False)) == 0   # (the accepted forms of the same call)
    if env.device.type == "cuda":
        torch.cuda.synchronize()
    assert bool((G == 0.0).all()) and bool((A == 0.0).all())

    import pytest
    ok = backward(env, d, values=d["values"])
    assert ok[0].shape == ok[1].shape == (T, B, S)
    wrong = [dict(reward=d["reward"][:, :, :-1].contiguous()), dict(reward=d["reward"][0]), dict(reward=d["reward"].to(torch.float32)),
             dict(next_row=d["next_row"].to(torch.int32)), dict(in_use=d["in_use"].to(torch.int16)),
             dict(values=d["values"].to(torch.float16)), dict(values=d["values"][:1]),
             dict(terminated=d["terminated"].to(other_device)), dict(values=d["values"].to(other_device)),
             dict(truncated=d["truncated"].transpose(0, 1).contiguous().transpose(0, 1)),
             dict(reward=torch.zeros((T, B, 2 * S), dtype=torch.float64, device=env.device)[:, :, ::2])]
    for kw in wrong:
        e = {**d, **kw}
        with pytest.raises(ValueError):
            backward(env, e, values=e["values"])
    with pytest.raises(ValueError):
        backward(env, d, returns=False)                       # nothing asked for
    with pytest.raises(ValueError):
        backward(env, d, advantages=True)                     # advantages without values
    with pytest.raises(ValueError):
        backward(env, {k: v[:0] for k, v in d.items()})       # T = 0
