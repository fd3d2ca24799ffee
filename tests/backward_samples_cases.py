"""Scenarios of `ppg_backward_samples` (returns and GAE from and into sample order in one launch; include/ppg.h),
`env.backward_samples()` and `AgentTrajectories.targets()` / `advantage_moments()`, shared by the wave-emulator tests
(test_backward_samples_emulated.py) and the GPU tests (test_backward_samples_gpu.py).  No tests of its own.

The reference (`reference`) is numpy only and does not use predpreygrass_amd.trajectory: V is built from the slot table and the
per-sample values with `np.where`, `tests.backward_cases.reference` (the numpy recursion `ppg_backward` is checked against) gives G and
A in float64, the stored rows are picked by slot and rounded with `astype(np.float32)`; the per-env sums are a loop over arrays of 64
lanes in the order include/ppg.h states, the butterfly as `x = x + x[lanes ^ m]`.  Every comparison of an output is `tobytes() ==
tobytes()` over the WHOLE tensor: the outputs start filled with 7.0 and so does the reference, so every stored sample is compared and
every other slot must have kept its 7.0.

Synthetic slot tables (`slots`) are built on top of `tests.backward_cases.synthetic` as `ppg_record_obs` would fill them -- per step,
env-major, rows ascending, a running cursor per species.  The predator store has room for everything (and five slots more, which
stay above the cursor).  The prey store is cut at 60 % of the prey rows of the steps in front of the last one, so the last step is
dropped whole and one before it in part (a dropped row can have a stored successor -- a predator -- only if it is not of the last
step; at T = 1 the one step is cut).  Then the words of every third dropped row are
overwritten with `capacity`, `capacity + 5`, -2 and INT32_MAX, and rows not in use get arbitrary words, valid-looking slots among
them.  The values are float32-representable random numbers with NaN in every slot at or above the stored count."""
import ctypes as C
import functools
import types

import numpy as np
import torch

from predpreygrass_amd import _abi
from tests import backward_cases as bc
from tests.backward_cases import CAPACITIES, GAMMA, HORIZONS, LAM   # noqa: F401  (the test files take them from here)

FILL = 7.0                       # what every output holds before a call
INT32_MAX = 2 ** 31 - 1
LANES = np.arange(64)


# ---- the reference ------------------------------------------------------------------------------------------------------------

def stored_rows(in_use, slot, capacity, cp):
    """(stored bool [T,B,S], prey bool [S]): the rows whose advantage / return is written."""
    prey = np.arange(in_use.shape[2]) >= cp
    cap = np.where(prey, capacity[1], capacity[0])
    return in_use.astype(bool) & (slot >= 0) & (slot < cap), prey


def reference(case, slot, capacity, values, cp, n_steps=None, want=("advantage", "returns", "stats")):
    """dict(advantage=[float32 [capacity[s]]] * 2, returns=..., stats=float64 [B,2,3], A=float64 [n,B,S], stored=bool [n,B,S]) of the
    first n_steps steps of `case` (a dict of backward_cases.synthetic's arrays); values: [v_pred, v_prey], float arrays [capacity[s]]
    or None; slots no stored row has hold FILL."""
    n = case["reward"].shape[0] if n_steps is None else n_steps
    d = {k: v[:n] for k, v in case.items() if k != "values"}
    k = slot[:n].astype(np.int64)
    stored, prey = stored_rows(d["in_use"], k, capacity, cp)
    V = np.zeros(k.shape)
    for s, v in enumerate(values):
        if v is not None and v.size:
            mine = stored & (prey if s else ~prey)
            V = np.where(mine, v.astype(np.float64)[np.where(mine, k, 0)], V)   # (a selection: NaN above the stored count stays out)
    G, A = bc.reference(d["reward"], d["next_row"], d["in_use"], d["terminated"], d["truncated"], V, GAMMA, LAM)
    out = dict(A=A, G=G, stored=stored)
    for name, x in (("advantage", A), ("returns", G)):
        if name in want:
            out[name] = []
            for s in (0, 1):
                mine = stored & (prey if s else ~prey)
                o = np.full(capacity[s], FILL, np.float32)
                o[k[mine]] = x[mine].astype(np.float32)
                out[name].append(o)
    if "stats" in want:
        B, S = k.shape[1:]
        acc = np.zeros((B, 2, 3, 64))                     # per env and species: n, sum, sq of every lane, started at +0.0
        for t in range(n - 1, -1, -1):
            for q in range(S // 64):
                s = 0 if 64 * q < cp else 1
                m, a = stored[t][:, 64 * q + LANES], A[t][:, 64 * q + LANES]
                acc[:, s, 0] = np.where(m, acc[:, s, 0] + 1.0, acc[:, s, 0])
                acc[:, s, 1] = np.where(m, acc[:, s, 1] + a, acc[:, s, 1])
                p = a * a
                acc[:, s, 2] = np.where(m, acc[:, s, 2] + p, acc[:, s, 2])
        for m in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[..., LANES ^ m]
        assert (acc == acc[..., :1]).all()                # (the butterfly is commutative: every lane ends with the same bits)
        out["stats"] = np.ascontiguousarray(acc[..., 0])
    return out


# ---- synthetic slot tables ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def slots(cp, cq, T, B, seed):
    """(case, slot int32 [T + 1,B,S], capacity, values [2] float64 [capacity[s]], counts) on backward_cases.synthetic(cp, cq, T, B,
    seed); all arrays read-only.  The store's horizon is T + 1: slot[T] holds valid-looking slots no call may read."""
    case, _, stats = bc.synthetic(cp, cq, T, B, seed)
    S = cp + cq
    rng = np.random.default_rng(seed + 5)
    in_use = case["in_use"]
    n_prey = int(in_use[:max(T - 1, 1), :, cp:].sum())    # (of the steps in front of the last one)
    capacity = (int(in_use[:, :, :cp].sum()) + 5, max(1, int(0.6 * n_prey)))
    slot = np.full((T + 1, B, S), -1, np.int64)
    cursor = [0, 0]
    for t in range(T):
        for b in range(B):
            for s, (first, rows) in enumerate(((0, cp), (cp, cq))):
                r = first + np.nonzero(in_use[t, b, first:first + rows])[0]
                k = cursor[s] + np.arange(len(r))
                slot[t, b, r] = np.where(k < capacity[s], k, -1)
                cursor[s] = min(cursor[s] + len(r), capacity[s])
    n_stored = tuple(cursor)
    dropped = in_use & (slot[:T] < 0)
    t, b, r = np.nonzero(dropped)
    hit = np.arange(len(t)) % 3 == 0
    kind = np.arange(int(hit.sum())) % 4                  # capacity, capacity + 5, -2, INT32_MAX in turn
    cap_of_row = np.where(r[hit] >= cp, capacity[1], capacity[0])
    slot[t[hit], b[hit], r[hit]] = np.select([kind == 0, kind == 1, kind == 2], [cap_of_row, cap_of_row + 5, -2], INT32_MAX)
    unused = ~in_use
    slot[:T][unused] = rng.integers(-3, max(capacity) + 3, int(unused.sum()))   # any word, valid-looking slots among them
    slot[T] = rng.integers(0, min(n_stored) if min(n_stored) else 1, (B, S))    # a step beyond n_steps: never read
    slot = slot.astype(np.int32)
    values = []
    for s in (0, 1):
        v = rng.normal(size=capacity[s]).astype(np.float32).astype(np.float64)   # (representable in float32: one set for both dtypes)
        v[n_stored[s]:] = np.nan
        values.append(v)
    # what the generated data holds
    stored, prey = stored_rows(in_use, slot[:T], capacity, cp)
    nx = case["next_row"][:-1].astype(np.int64)
    taken = in_use[:-1] & ~(case["terminated"][:-1] | case["truncated"][:-1]) & (nx >= 0)
    succ_stored = np.take_along_axis(stored[1:], np.where(taken, nx, 0), 2)
    succ_dropped = np.take_along_axis(dropped[1:], np.where(taken, nx, 0), 2)
    counts = dict(stats, stored_pred=int(stored[:, :, :cp].sum()), stored_prey=int(stored[:, :, cp:].sum()),
                  dropped_prey=int(dropped[:, :, cp:].sum()), junk=int(hit.sum()),
                  stored_to_dropped=int((taken & stored[:-1] & succ_dropped).sum()),
                  dropped_to_stored=int((taken & dropped[:-1] & succ_stored).sum()), n_stored=n_stored)
    assert counts["stored_pred"] == n_stored[0] and counts["stored_prey"] == n_stored[1]
    for x in [slot] + values:
        x.setflags(write=False)
    return case, slot, capacity, values, counts


def check_not_vacuous(counts, T, S, ref):
    bc.check_not_vacuous(counts, T, S)                    # (links across the r = 64 lane boundary both ways among them)
    assert counts["stored_pred"] > 0 and counts["stored_prey"] > 0 and counts["dropped_prey"] > 0 and counts["junk"] >= 4, counts
    if T >= 2:
        assert counts["stored_to_dropped"] > 0 and counts["dropped_to_stored"] > 0, counts
    m = ref["stored"]
    assert (ref["A"][m] != ref["G"][m]).any(), "no stored sample tells the advantage from the return"
    for name in ("advantage", "returns"):
        for x in ref[name]:
            assert not np.isnan(x).any(), "a NaN of an unreferenced slot reached an output"


# ---- calls ----------------------------------------------------------------------------------------------------------------------

def sync(env):
    if env.device.type == "cuda":
        torch.cuda.synchronize()


def device_case(env, case, slot, **replace):
    d = {k: torch.from_numpy(np.array(replace.get(k, v))).to(env.device) for k, v in case.items() if k != "values"}
    d["slot"] = torch.from_numpy(np.array(slot)).to(env.device)
    return d


def raw(env, d, capacity, values, n_steps, dtype=torch.float64, want=("advantage", "returns", "stats")):
    """ppg_backward_samples through the raw entry point on outputs of exactly their sizes, filled with FILL.  Returns (rc, dict of the
    output tensors)."""
    dev = env.device
    out = {name: [torch.full((n,), FILL, dtype=torch.float32, device=dev) for n in capacity] for name in ("advantage", "returns") if name in want}
    if "stats" in want:
        out["stats"] = torch.full((env.batch_size, 2, 3), FILL, dtype=torch.float64, device=dev)
    vals = [None if v is None else torch.from_numpy(np.array(v)).to(dtype).to(dev) for v in values]
    st, tg = _abi.PpgObsStore(), _abi.PpgSampleTargets()
    st.horizon, st.slot = d["slot"].shape[0], d["slot"].data_ptr()
    anchor = d["slot"].data_ptr()                         # (an empty tensor has no address; nothing is addressed through it)
    for s in (0, 1):
        st.capacity[s] = capacity[s]
        if vals[s] is not None:
            tg.values[s] = vals[s].data_ptr() or anchor
        for name in ("advantage", "returns"):
            if name in want:
                getattr(tg, name)[s] = out[name][s].data_ptr() or anchor
    if "stats" in want:
        tg.stats = out["stats"].data_ptr()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in d.items()}
    rc = env._lib.ppg_backward_samples(env._handle, n_steps, p["reward"], p["next_row"], p["in_use"], p["terminated"], p["truncated"],
                                       C.byref(st), C.byref(tg), _abi.F32 if dtype == torch.float32 else _abi.F64, GAMMA, LAM,
                                       env._stream())
    sync(env)
    return rc, out


def same(got, want):
    return got.cpu().numpy().tobytes() == want.tobytes()


def check(out, ref, tag, want=("advantage", "returns", "stats")):
    assert set(out) == set(want), (tag, sorted(out))
    for name in want:
        if name == "stats":
            assert same(out[name], ref[name]), (tag, name)
        else:
            for s in (0, 1):
                assert same(out[name][s], ref[name][s]), (tag, name, s)


def synthetic_case(make, cp, cq, cfg, T, B):
    env = make(cfg, B, pred_capacity=cp, prey_capacity=cq)
    assert env.S == cp + cq and env.pred_capacity == cp
    # (seeds: checked on the CPU against check_not_vacuous for every CAPACITIES x HORIZONS at B = 3 and 64 and for the full batch; the
    # seeds of backward_cases.synthetic_case, 1000 T + S, leave no dropped row with a stored successor at T = 3, B = 3, S = 192 / 384)
    case, slot, capacity, values, counts = slots(cp, cq, T, B, 1000 * T + cp + cq + 1)
    ref = reference(case, slot, capacity, values, cp)
    check_not_vacuous(counts, T, env.S, ref)
    for s in (0, 1):                                      # exactly the stored slots change
        assert np.array_equal(ref["advantage"][s] != FILL, np.arange(capacity[s]) < counts["n_stored"][s])
    d = device_case(env, case, slot)
    tag = (cp, cq, T, B)
    rc, out = raw(env, d, capacity, values, T)
    assert rc == 0, env._lib.ppg_last_error(env._handle)
    check(out, ref, (tag, "float64 values"))
    rc, out = raw(env, d, capacity, values, T, dtype=torch.float32)
    assert rc == 0
    check(out, ref, (tag, "float32 values"))
    for want in (("advantage", "stats"), ("returns",), ("advantage", "returns"), ("advantage",)):
        rc, out = raw(env, d, capacity, values if "advantage" in want else [None, None], T, want=want)
        assert rc == 0, want
        check(out, ref, (tag, want), want)
    no_pred = reference(case, slot, capacity, [None, values[1]], cp)
    assert no_pred["advantage"][0].tobytes() != ref["advantage"][0].tobytes()
    rc, out = raw(env, d, capacity, [None, values[1]], T)
    assert rc == 0
    check(out, no_pred, (tag, "values[0] = NULL"))
    if T > 1:                                             # fewer steps than recorded: the later steps' slots keep FILL
        short = reference(case, slot, capacity, values, cp, n_steps=T - 1)
        assert (short["advantage"][0] == FILL).sum() > (ref["advantage"][0] == FILL).sum()
        rc, out = raw(env, d, capacity, values, T - 1)
        assert rc == 0
        check(out, short, (tag, "n_steps = T - 1"))
    for zero in (0, 1):                                   # a species whose store holds nothing: every row of it is dropped
        cap0 = tuple(0 if s == zero else c for s, c in enumerate(capacity))
        vals0 = [v[:c] for v, c in zip(values, cap0)]
        none = reference(case, slot, cap0, vals0, cp)
        assert none["advantage"][zero].size == 0 and (none["stats"][:, zero] == 0).all() and (none["stats"][:, 1 - zero, 0] > 0).any()
        rc, out = raw(env, d, cap0, vals0, T)
        assert rc == 0
        check(out, none, (tag, f"capacity[{zero}] = 0"))
    # the wrapper: newly allocated outputs, zero where nothing is stored
    store = types.SimpleNamespace(horizon=T + 1, capacity=capacity, slot=d["slot"])
    vals = [torch.from_numpy(np.array(v)).to(env.device) for v in values]
    adv, ret, stats = env.backward_samples(store, d["reward"][:T], d["next_row"][:T], d["in_use"][:T], d["terminated"][:T],
                                           d["truncated"][:T], GAMMA, LAM, values=vals, stats=True)
    sync(env)
    for s in (0, 1):
        for got, name in ((adv[s], "advantage"), (ret[s], "returns")):
            assert got.dtype == torch.float32 and same(got, np.where(ref[name][s] == FILL, np.float32(0.0), ref[name][s])), (tag, name, s)
    assert same(stats, ref["stats"])
    adv, ret, stats = env.backward_samples(store, d["reward"][:T], d["next_row"][:T], d["in_use"][:T], d["terminated"][:T],
                                           d["truncated"][:T], GAMMA, LAM, advantages=False)
    assert adv is None and stats is None and same(ret[1], np.where(ref["returns"][1] == FILL, np.float32(0.0), ref["returns"][1]))


def out_of_range_links(make):
    """The scenario of backward_cases.out_of_range_links -- next_row values of S, S + 7, -2, 32767 and -32768 in rows in use behave as
    -1 -- through the new call."""
    cp, cq, cfg = CAPACITIES[-1]
    T, B = 5, 3
    env = make(cfg, B, pred_capacity=cp, prey_capacity=cq)
    case, slot, capacity, values, _ = slots(cp, cq, T, B, 77)
    S = cp + cq
    nx = case["next_row"].copy()
    taken = case["in_use"] & ~case["terminated"] & ~case["truncated"] & (nx >= 0)
    taken[-1] = False
    t, b, r = np.nonzero(taken)
    assert len(t) > 50
    hit = np.arange(len(t)) % 3 == 0                      # a third of the links that were taken
    nx[t[hit], b[hit], r[hit]] = np.array(bc.outside(S), np.int64)[np.arange(int(hit.sum())) % 5].astype(np.int16)
    cut = nx.copy()
    cut[t[hit], b[hit], r[hit]] = -1
    want = reference({**case, "next_row": cut}, slot, capacity, values, cp)
    assert want["advantage"][0].tobytes() != reference(case, slot, capacity, values, cp)["advantage"][0].tobytes(), "cutting the links changed nothing"
    rc, out = raw(env, device_case(env, case, slot, next_row=nx), capacity, values, T)
    assert rc == 0
    check(out, want, "out-of-range links")


# ---- recorded trajectories -------------------------------------------------------------------------------------------------------

def moments_close(stats, A64, tag):
    """advantage_moments(stats) against numpy float64 over the unrounded advantages A64 [n] of one species.  Bounds: a float64 sum of n
    terms in any order is within (n - 1) * 2^-53 * sum|x| of the exact one (first order), so two orders differ by at most
    n * 2^-52 * sum|x|; likewise the squares with sum x^2 (both sides form the same products).  mean = sum / n and var = sq / n - mean^2
    add a few roundings of their own (4 ulp of the operands taken), and std = sqrt(var) moves by d(var) / (2 std)."""
    count, mean, std = stats
    n = A64.size
    assert int(count) == n, (tag, "count", float(count), n)
    if n == 0:
        assert float(mean) == 0.0 and float(std) == 0.0, tag
        return
    u = 2.0 ** -52
    tol_sum, tol_sq = n * u * np.abs(A64).sum(), n * u * (A64 * A64).sum()
    want_mean, want_std = float(np.mean(A64)), float(np.std(A64))
    tol_mean = tol_sum / n + 4 * u * abs(want_mean)
    assert abs(float(mean) - want_mean) <= tol_mean, (tag, "mean", float(mean), want_mean, tol_mean)
    second = float((A64 * A64).sum()) / n
    tol_var = tol_sq / n + 2 * abs(want_mean) * tol_mean + 4 * u * second
    assert want_std > 0 and abs(float(std) - want_std) <= tol_var / (2 * want_std) + 4 * u * want_std, (tag, "std", float(std), want_std)


def recorded(make_env, n_steps=40, need_pred_rows=0, prey_rows_per_env_step=4):
    """n_steps random-action steps with auto-reset recorded by AgentTrajectories with a store whose prey side overflows: targets()
    against the numpy reference over the stored tensors, against targets_torch() bit for bit, advantage_moments() within the
    summation bound, the same bytes with step_on_device=True, float32 values, an empty trajectory."""
    from predpreygrass_amd.trajectory import AgentTrajectories
    got = []
    for on_device in (False, True):
        env = make_env()
        B, S, cp = env.batch_size, env.S, env.pred_capacity
        env.reset()
        traj = AgentTrajectories(env, n_steps, obs_rows=(n_steps * B * cp, n_steps * B * prey_rows_per_env_step), step_on_device=on_device)
        for _ in range(n_steps):
            env.step(random_actions=True, auto_reset=True)
            traj.record()
        sync(env)
        (sp, dp), (sq, dq) = traj.store.counts()
        assert sp > 0 and sq > 0 and dq > 0 and dp == 0, ((sp, dp), (sq, dq))
        gen = torch.Generator().manual_seed(9)
        v = [(torch.rand((n,), dtype=torch.float64, generator=gen) * 4.0 - 2.0).to(env.device) for n in (sp, sq)]
        adv, ret, stats = traj.targets(v[0], v[1], GAMMA, LAM)
        sync(env)
        got.append([x.cpu().numpy().tobytes() for x in adv + ret + [stats]])
        if on_device:
            continue
        case = {k: getattr(traj, k).cpu().numpy() for k in ("reward", "next_row", "in_use", "terminated", "truncated")}
        assert int(case["in_use"][:, :, :cp].sum(2).max()) > need_pred_rows and (case["next_row"] >= 0).any()
        slot, capacity = traj.store.slot.cpu().numpy(), traj.store.capacity
        pad = [np.concatenate([x.cpu().numpy(), np.full(c - x.numel(), np.nan)]) for x, c in zip(v, capacity)]
        ref = reference(case, slot, capacity, pad, cp)
        stored, prey = stored_rows(case["in_use"], slot, capacity, cp)
        assert (case["in_use"] & ~stored)[:, :, cp:].any() and np.abs(ref["A"][stored]).max() > 0
        for s, n in enumerate((sp, sq)):
            assert adv[s].shape == ret[s].shape == (n,) and adv[s].dtype == ret[s].dtype == torch.float32
            assert same(adv[s], ref["advantage"][s][:n]) and same(ret[s], ref["returns"][s][:n]), ("targets() against numpy", s)
            assert (ref["advantage"][s][n:] == FILL).all()
        assert same(stats, ref["stats"]), "stats against the lane-order loop"
        adv_t, ret_t, stats_t = traj.targets_torch(v[0], v[1], GAMMA, LAM)
        for s in (0, 1):
            assert torch.equal(adv[s].view(torch.int32), adv_t[s].view(torch.int32)), ("targets_torch(): advantages", s)
            assert torch.equal(ret[s].view(torch.int32), ret_t[s].view(torch.int32)), ("targets_torch(): returns", s)
        assert torch.equal(stats[:, :, 0], stats_t[:, :, 0])
        moments, moments_t = traj.advantage_moments(stats), traj.advantage_moments(stats_t)
        for s in (0, 1):
            A64 = ref["A"][stored & (prey if s else ~prey)]
            moments_close([x[s].cpu() for x in moments], A64, ("targets()", s))
            moments_close([x[s].cpu() for x in moments_t], A64, ("targets_torch()", s))
        assert all(x.dtype == torch.float64 and x.device == env.device and tuple(x.shape) == (2,) for x in moments)
        # float32 values go in as they are; advantages only; no values at all
        v32 = [x.to(torch.float32) for x in v]
        pad32 = [np.concatenate([x.cpu().numpy().astype(np.float64), np.full(c - x.numel(), np.nan)]) for x, c in zip(v32, capacity)]
        ref32 = reference(case, slot, capacity, pad32, cp, want=("advantage",))
        adv32, none, none2 = traj.targets(v32[0], v32[1], GAMMA, LAM, returns=False, stats=False)
        assert none is None and none2 is None and all(same(adv32[s], ref32["advantage"][s][:n]) for s, n in enumerate((sp, sq)))
        ref0 = reference(case, slot, capacity, [None, None], cp, want=("advantage",))
        adv0 = traj.targets(None, None, GAMMA, LAM)[0]
        assert all(same(adv0[s], ref0["advantage"][s][:n]) for s, n in enumerate((sp, sq)))
        assert all(torch.equal(x, y) for x, y in zip(adv0, traj.targets_torch(None, None, GAMMA, LAM)[0]))
        import pytest
        with pytest.raises(ValueError):
            traj.targets(v[0][:-1], v[1], GAMMA, LAM)
        with pytest.raises(ValueError):
            traj.targets(v[0], v32[1], GAMMA, LAM)
        with pytest.raises(RuntimeError):
            AgentTrajectories(env, n_steps).targets(v[0], v[1], GAMMA, LAM)
        # an empty trajectory: empty tensors, no launch
        traj.clear()
        adv, ret, stats = traj.targets(v[0][:0], v[1][:0], GAMMA, LAM)
        assert all(tuple(x.shape) == (0,) and x.dtype == torch.float32 for x in adv + ret) and tuple(stats.shape) == (B, 2, 3)
        moments_close([x[0].cpu() for x in traj.advantage_moments(stats)], np.zeros(0), "empty")
    assert got[0] == got[1], "step_on_device=True gave other bytes"


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def argument_checking(env, other_device):
    """Every PPG_EINVAL case of ppg_backward_samples returns non-zero, names the function and writes nothing (outputs filled with a
    sentinel); the Python wrapper raises ValueError on a wrong shape, dtype, device, a non-contiguous input or values shorter than
    the capacity."""
    import pytest
    T, B, S, dev = 2, env.batch_size, env.S, env.device
    H = T + 1
    capacity = (T * B * 3, T * B * 5)
    d = dict(reward=torch.zeros((T, B, S), dtype=torch.float64), next_row=torch.full((T, B, S), -1, dtype=torch.int16),
             in_use=torch.zeros((T, B, S), dtype=torch.bool), terminated=torch.zeros((T, B, S), dtype=torch.bool),
             truncated=torch.zeros((T, B, S), dtype=torch.bool))
    slot = torch.full((H, B, S), -1, dtype=torch.int32)
    cp = env.pred_capacity
    for t in range(T):
        for b in range(B):
            for s, (first, n) in enumerate(((0, 3), (cp, 5))):
                d["in_use"][t, b, first:first + n] = True
                slot[t, b, first:first + n] = torch.arange(n, dtype=torch.int32) + (t * B + b) * n
    d = {k: v.to(dev) for k, v in d.items()}
    slot = slot.to(dev)
    values = [torch.ones((n,), dtype=torch.float64, device=dev) for n in capacity]
    out = dict(advantage=[torch.full((n,), FILL, dtype=torch.float32, device=dev) for n in capacity],
               returns=[torch.full((n,), FILL, dtype=torch.float32, device=dev) for n in capacity],
               stats=torch.full((B, 2, 3), FILL, dtype=torch.float64, device=dev))

    def call(n_steps=T, horizon=H, cap=capacity, null=(), dtype=_abi.F64, st=True, tg=True):
        s_, t_ = _abi.PpgObsStore(), _abi.PpgSampleTargets()
        s_.horizon = horizon
        s_.slot = None if "slot" in null else slot.data_ptr()
        for s in (0, 1):
            s_.capacity[s] = cap[s]
            t_.values[s] = None if f"values{s}" in null else values[s].data_ptr()
            t_.advantage[s] = None if f"advantage{s}" in null else out["advantage"][s].data_ptr()
            t_.returns[s] = None if f"returns{s}" in null else out["returns"][s].data_ptr()
        t_.stats = None if "stats" in null else out["stats"].data_ptr()
        p = {k: (None if k in null else C.c_void_p(v.data_ptr())) for k, v in d.items()}
        return env._lib.ppg_backward_samples(env._handle, n_steps, p["reward"], p["next_row"], p["in_use"], p["terminated"],
                                             p["truncated"], C.byref(s_) if st else None, C.byref(t_) if tg else None, dtype, GAMMA, LAM,
                                             env._stream())
    refused = [dict(n_steps=0), dict(n_steps=-3), dict(n_steps=H + 1), dict(n_steps=T, horizon=T - 1), dict(st=False), dict(tg=False),
               dict(null=("slot",)), dict(cap=(-1, capacity[1])), dict(cap=(capacity[0], 2 ** 31)), dict(cap=(capacity[0], -(2 ** 40))),
               dict(horizon=2 ** 31 - 1), dict(null=("advantage0",)), dict(null=("advantage1",)), dict(null=("returns0",)),
               dict(null=("returns1",)), dict(null=("advantage0", "advantage1", "returns0", "returns1", "stats")),
               dict(null=("advantage0", "advantage1")), dict(dtype=2), dict(dtype=-1), dict(dtype=2, null=("values0",))] + \
              [dict(null=(k,)) for k in d]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert env._lib.ppg_last_error(env._handle).startswith(b"ppg_backward_samples:"), (kw, env._lib.ppg_last_error(env._handle))
    sync(env)
    for x in out["advantage"] + out["returns"] + [out["stats"]]:
        assert bool((x == FILL).all()), "a refused call wrote to its outputs"
    # (the accepted forms: one pair, no stats, no values with any dtype code, the whole horizon)
    for kw in (dict(null=("returns0", "returns1")), dict(null=("advantage0", "advantage1", "stats")), dict(null=("stats",)),
               dict(null=("values0", "values1"), dtype=5), dict(null=("values0",)), dict(cap=(0, 0)), dict()):
        assert call(**kw) == 0, (kw, env._lib.ppg_last_error(env._handle))
    sync(env)
    n_written = T * B * 3
    assert bool((out["advantage"][0][:n_written] != FILL).all()) and bool((out["advantage"][0][n_written:] == FILL).all())
    assert out["stats"][:, 0, 0].cpu().tolist() == [float(T * 3)] * B and out["stats"][:, 1, 0].cpu().tolist() == [float(T * 5)] * B

    store = types.SimpleNamespace(horizon=H, capacity=capacity, slot=slot)

    def wrapped(store=store, values=values, **kw):
        e = {**d, **kw}
        return env.backward_samples(store, e["reward"], e["next_row"], e["in_use"], e["terminated"], e["truncated"], GAMMA, LAM,
                                    values=values, stats=True)
    adv, ret, stats = wrapped()
    assert adv[0].shape == (capacity[0],) and ret[1].shape == (capacity[1],) and stats.shape == (B, 2, 3)
    wrong = [dict(reward=d["reward"][:, :, :-1].contiguous()), dict(reward=d["reward"][0]), dict(reward=d["reward"].to(torch.float32)),
             dict(next_row=d["next_row"].to(torch.int32)), dict(in_use=d["in_use"].to(torch.int16)),
             dict(terminated=d["terminated"].to(other_device)),
             dict(truncated=d["truncated"].transpose(0, 1).contiguous().transpose(0, 1)),
             dict(reward=torch.zeros((T, B, 2 * S), dtype=torch.float64, device=dev)[:, :, ::2]),
             dict(reward=torch.zeros((H + 1, B, S), dtype=torch.float64, device=dev)),           # more steps than the store's horizon
             dict(values=[values[0].to(torch.float16), values[1].to(torch.float16)]), dict(values=[values[0][:-1], values[1]]),
             dict(values=[values[0], values[1].to(torch.float32)]), dict(values=[values[0].to(other_device), values[1]]),
             dict(values=[values[0].reshape(-1, 1), values[1]]), dict(values=[values[0]]),
             dict(values=[torch.ones((2 * capacity[0],), dtype=torch.float64, device=dev)[::2], values[1]]),
             dict(store=types.SimpleNamespace(horizon=H, capacity=capacity, slot=slot.to(torch.int64))),
             dict(store=types.SimpleNamespace(horizon=H, capacity=capacity, slot=slot[:, :, :-1].contiguous())),
             dict(store=types.SimpleNamespace(horizon=H, capacity=capacity, slot=slot.to(other_device))),
             dict(store=types.SimpleNamespace(horizon=H, capacity=(-1, capacity[1]), slot=slot))]
    for kw in wrong:
        with pytest.raises(ValueError):
            wrapped(**kw)
    e = d
    with pytest.raises(ValueError):
        env.backward_samples(store, e["reward"], e["next_row"], e["in_use"], e["terminated"], e["truncated"], GAMMA, LAM,
                             advantages=False, returns=False)
    with pytest.raises(ValueError):
        env.backward_samples(store, e["reward"], e["next_row"], e["in_use"], e["terminated"], e["truncated"], GAMMA, LAM,
                             advantages=False, stats=True)
