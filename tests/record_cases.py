"""Scenarios of `ppg_record` (the link plus one step's stores into trajectory buffers, one launch; include/ppg.h), `env.record()`
and `AgentTrajectories.record()`, shared by the wave-emulator tests (test_record_emulated.py) and the GPU tests
(test_record_gpu.py).

The reference of `against_numpy` is built on the host from `tables_of(env)` after every call: the id join of tests/link_cases.py,
the row counts, the flag bits and the reward table.  It does not use predpreygrass_amd.trajectory.  The other scenarios compare
with `record_torch()` (the torch ops `record()` used to be) on a twin env of the same config and seed.  Every comparison is byte
equality.

`make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a BatchedRedQueen, both on the backend under test."""
import ctypes as C

import numpy as np
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.trajectory import AgentTrajectories
from tests.backward_cases import CAPACITIES
from tests.link_cases import CFG_BASE, CFG_P2, CFG_RQ, id_join, in_use_mask, tables_of

NAMES = ("reward", "in_use", "terminated", "truncated", "next_row")
# (config, constructor keywords, steps) of backward_cases.recorded: known to produce auto-resets, births and deaths
RECORDED = {"base": (CFG_BASE, dict(prey_capacity=128, seed=3), 40),
            "p128": (CFG_P2, dict(pred_capacity=128, prey_capacity=256, seed=7), 60),
            "gen2": (CFG_RQ, dict(seed=4), 40)}
SHORT = 8   # steps where only the shape matters


def fresh(env, T):
    """The five [T,B,S] tensors as a trajectory starts out: zeros, next_row -1.  Flags as bool (what AgentTrajectories holds)."""
    B, S, dev = env.batch_size, env.S, env.device
    d = dict(reward=torch.zeros((T, B, S), dtype=torch.float64, device=dev), next_row=torch.full((T, B, S), -1, dtype=torch.int16, device=dev))
    for k in ("in_use", "terminated", "truncated"):
        d[k] = torch.zeros((T, B, S), dtype=torch.bool, device=dev)
    return d


def args(d):
    return tuple(d[k] for k in NAMES)


def of(traj):
    return {k: getattr(traj, k) for k in NAMES}


def raw_bytes(x):
    return x.cpu().contiguous().view(torch.uint8).numpy().tobytes()


def same_tensors(a, b, tag):
    for k in NAMES:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (tag, k)


def sync(env):
    if env.device.type == "cuda":
        torch.cuda.synchronize()


def against_numpy(env, n_steps, envs=None, need=("reset", "birth", "death")):
    """After every step(random_actions, auto_reset) + env.record(t) the reference of step t's five slices and of step t-1's next_row
    is built from the host tables; at the end all five tensors equal it in the checked envs."""
    envs = list(range(env.batch_size)) if envs is None else envs
    T, cp, S = n_steps, env.pred_capacity, env.S
    env.reset()
    d = fresh(env, T)
    want = dict(reward=np.zeros((T, len(envs), S)), next_row=np.full((T, len(envs), S), -1, np.int16))
    for k in ("in_use", "terminated", "truncated"):
        want[k] = np.zeros((T, len(envs), S), bool)
    seen = {"reset": 0, "birth": 0, "death": 0, "links": 0}
    prev = None
    for t in range(T):
        env.step(random_actions=True, auto_reset=True)
        env.record(*args(d), t)
        cur = tables_of(env)
        for k, b in enumerate(envs):
            used = in_use_mask(cur, b, cp, S)
            flags = cur["row_flags"][b]
            want["in_use"][t, k] = used
            want["reward"][t, k] = cur["row_reward"][b]
            want["terminated"][t, k] = used & ((flags & _abi.ROW_DIED) != 0)
            want["truncated"][t, k] = used & ((flags & _abi.ROW_TRUNC) != 0)
            if t > 0:
                want["next_row"][t - 1, k] = id_join(prev, cur, b, cp, S)[1]
                seen["links"] += int((want["next_row"][t - 1, k] >= 0).sum())
            seen["reset"] += bool(int(cur["env_state"][b, _abi.ENV_FLAGS]) & _abi.ENVF_WAS_RESET)
            seen["birth"] += int(((flags & _abi.ROW_NEWBORN) != 0)[used].sum())
            seen["death"] += int(((flags & _abi.ROW_DIED) != 0)[used].sum())
        prev = cur
    for k in need:
        assert seen[k] > 0, (k, seen)   # (the run must not pass vacuously)
    assert seen["links"] > 0, seen
    for k in NAMES:
        got = d[k].cpu().numpy()[:, envs]
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k
    assert want["terminated"].any() or "death" not in need
    return seen


def against_numpy_capacity(make, cp, cq, cfg, B, envs=None):
    """SHORT steps at one (pred_capacity, prey_capacity): only the row-register count matters."""
    env = make(cfg, B, pred_capacity=cp, prey_capacity=cq, seed=5)
    assert env.S == cp + cq
    against_numpy(env, SHORT, envs, need=())


def twins(make, cfg, B, **kw):
    return make(cfg, B, **kw), make(cfg, B, **kw)


def against_torch(env, twin, n_steps, step_on_device=False):
    """record() on env, record_torch() on its twin: the five tensors and the returned [B,S] link maps are equal after every step, over
    all envs."""
    env.reset()
    twin.reset()
    a, b = AgentTrajectories(env, n_steps, step_on_device=step_on_device), AgentTrajectories(twin, n_steps)
    for t in range(n_steps):
        env.step(random_actions=True, auto_reset=True)
        twin.step(random_actions=True, auto_reset=True)
        a.record()
        b.record_torch()
        for got, want, name in zip(env._link_tensors(), twin._link_tensors(), ("prev_row", "next_row")):
            assert torch.equal(got, want), (t, name)
    assert len(a) == len(b) == n_steps
    same_tensors(of(a), of(b), "after the run")
    assert bool((a.next_row >= 0).any()) and bool(a.terminated.any()) and bool((a.reward != 0).any()), "nothing was recorded"
    return a, b


def returned_maps_are_the_links(env, twin):
    """env.record() returns the env's own link tensors, written as by link()."""
    env.reset()
    twin.reset()
    d = fresh(env, 3)
    for t in range(3):
        env.step(random_actions=True)
        twin.step(random_actions=True)
        p, n = env.record(*args(d), t)
        q, m = twin.link()
        assert p is env._link_tensors()[0] and n is env._link_tensors()[1]
        assert torch.equal(p, q) and torch.equal(n, m), t
    assert bool((p >= 0).any())


CANARY16 = 0x5555


def canaried(env, T, guard=1000):
    """The five buffers as views into larger tensors filled with a canary (NaN for reward, 0x55 bytes elsewhere), `guard` elements
    in front and behind.  Returns (views, whole tensors).  Flags are uint8: a bool tensor cannot hold 0x55."""
    B, S, dev = env.batch_size, env.S, env.device
    n = T * B * S
    whole = dict(reward=torch.full((n + 2 * guard,), float("nan"), dtype=torch.float64, device=dev),
                 next_row=torch.full((n + 2 * guard,), CANARY16, dtype=torch.int16, device=dev))
    for k in ("in_use", "terminated", "truncated"):
        whole[k] = torch.full((n + 2 * guard,), 0x55, dtype=torch.uint8, device=dev)
    views = {k: v[guard:guard + n].view(T, B, S) for k, v in whole.items()}
    assert all(v.is_contiguous() for v in views.values())
    return views, whole


def exactly_the_documented_elements(env, T=5):
    """record() at t = 0, a middle t and t = T-1 into canary-filled buffers: step t's slices hold no canary, next_row[t-1] is written
    only for t > 0, every other element and both guard regions keep their bytes."""
    guard = 1000
    B, S = env.batch_size, env.S
    env.reset()
    env.step(random_actions=True)
    env.link()   # (the records below link to something)
    for t in (0, T // 2, T - 1):
        views, whole = canaried(env, T, guard)
        before = {k: raw_bytes(v) for k, v in whole.items()}
        env.step(random_actions=True)
        env.record(*args(views), t)
        sync(env)
        got = {k: v.cpu().numpy() for k, v in views.items()}
        assert not np.isnan(got["reward"][t]).any()
        for k in ("in_use", "terminated", "truncated"):
            assert (got[k][t] <= 1).all(), (t, k)
        assert got["in_use"][t].any()
        assert (got["next_row"][t] == -1).all()
        if t > 0:
            assert (got["next_row"][t - 1] != CANARY16).all() and (got["next_row"][t - 1] >= 0).any(), t
        # everything else: byte for byte what it was
        for k, v in whole.items():
            item = v.element_size()
            now = np.frombuffer(raw_bytes(v), np.uint8).reshape(-1, item)
            was = np.frombuffer(before[k], np.uint8).reshape(-1, item)
            written = np.zeros(len(now), bool)
            written[guard + t * B * S: guard + (t + 1) * B * S] = True
            if k == "next_row" and t > 0:
                written[guard + (t - 1) * B * S: guard + t * B * S] = True
            assert (now[~written] == was[~written]).all(), (t, k, "an element outside the documented ones was written")
            assert (~written[:guard]).all() and (~written[-guard:]).all()


def mixing_and_invalidation(env):
    """link() between two record()s; record() right after reset() and after import_state of one env; clear() then record()."""
    B, cp, S = env.batch_size, env.pred_capacity, env.S
    assert B >= 2
    T = 7
    env.reset()
    traj = AgentTrajectories(env, T)
    env.step(random_actions=True)
    traj.record()                                   # t = 0
    env.step(random_actions=True)
    env.link()                                      # a link call in between: the snapshot moves on to this output
    at_link = tables_of(env)
    env.step(random_actions=True)
    traj.record()                                   # t = 1: next_row[0] is the map from the link() call's rows, not from step 0's
    cur = tables_of(env)
    got = traj.next_row[0].cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], id_join(at_link, cur, b, cp, S)[1]), (b, "link() between two record()s")
    assert (got >= 0).any()
    env.reset()
    traj.record()                                   # t = 2, right after reset(): nothing links
    assert bool((traj.next_row[1] == -1).all()), "record() after reset() linked rows"
    assert bool(traj.in_use[2].any())
    env.step(random_actions=True)
    traj.record()                                   # t = 3
    assert bool((traj.next_row[2] >= 0).any())
    env.import_state(env.export_state(1), 0)
    traj.record()                                   # t = 4: env 0 was imported
    assert bool((traj.next_row[3][0] == -1).all()), "env 0 was imported: nothing may link"
    for b in range(1, B):
        assert bool((traj.next_row[3][b] >= 0).any()), (b, "the other envs keep their links")
    env.step(random_actions=True)
    traj.record()                                   # t = 5
    assert bool((traj.next_row[4][0] >= 0).any())
    # clear(), then record(): step 0 again, and no next_row[-1]
    traj.next_row[T - 1].fill_(123)
    keep = {k: raw_bytes(v[1:]) for k, v in of(traj).items()}
    traj.clear()
    assert len(traj) == 0
    env.step(random_actions=True)
    traj.record()
    assert len(traj) == 1
    assert bool((traj.next_row[T - 1] == 123).all()) and bool((traj.next_row[0] == -1).all())
    for k, v in of(traj).items():
        assert raw_bytes(v[1:]) == keep[k], (k, "record() at step 0 wrote outside step 0")


def device_step_index(env, twin, T=12, n_eager=10):
    """step_on_device=True gives the bytes of the host index; a device word outside [0, T) makes the launch a link()."""
    env.reset()
    twin.reset()
    a, b = AgentTrajectories(env, T, step_on_device=True), AgentTrajectories(twin, T)
    assert a.t_dev.dtype == torch.int32 and a.t_dev.numel() == 1
    for t in range(n_eager):
        env.step(random_actions=True, auto_reset=True)
        twin.step(random_actions=True, auto_reset=True)
        a.record()
        b.record()
    assert len(a) == len(b) == n_eager
    same_tensors(of(a), of(b), "device index against host index")
    assert bool((a.next_row >= 0).any())
    import pytest
    with pytest.raises(RuntimeError):
        a.record_torch()
    for word in (T, T + 5, -1, -2 ** 31):
        a.t_dev.fill_(word)
        before = {k: raw_bytes(v) for k, v in of(a).items()}
        env.step(random_actions=True, auto_reset=True)
        twin.step(random_actions=True, auto_reset=True)
        p, n = env.record(*args(of(a)), a.t_dev)
        q, m = twin.link()
        assert torch.equal(p, q) and torch.equal(n, m), (word, "the launch must be link()")
        assert bool((p >= 0).any())
        sync(env)
        for k, v in of(a).items():
            assert raw_bytes(v) == before[k], (word, k, "a buffer was written")
        assert 0 <= len(a) <= T
    # record() past the horizon in this mode stores nothing and counts on
    a.t_dev.fill_(T)
    a.record()
    assert len(a) == T and int(a.t_dev.item()) == T + 1
    a.clear()
    assert len(a) == 0 and int(a.t_dev.item()) == 0


def argument_checking(env, other_device):
    """Every PPG_EINVAL case of ppg_record returns non-zero, names ppg_record and leaves canary-filled buffers untouched; the Python
    wrapper raises ValueError on a wrong dtype, shape, device or a non-contiguous input; a full trajectory raises RuntimeError."""
    import pytest
    T, B, S = 3, env.batch_size, env.S
    env.reset()
    env.step(random_actions=True)
    views, whole = canaried(env, T)
    before = {k: raw_bytes(v) for k, v in whole.items()}
    word = torch.zeros((1,), dtype=torch.int32, device=env.device)

    def raw(buf=True, horizon=T, step=0, flags=0, **null):
        b = _abi.PpgRecordBuffers(horizon, *[None if k in null else views[k].data_ptr() for k in NAMES])
        return env._lib.ppg_record(env._handle, C.byref(b) if buf else None, step, flags, None, None, env._stream())
    refused = [dict(buf=False), dict(horizon=0), dict(horizon=-4), dict(step=T), dict(step=T + 9), dict(step=2 ** 63), dict(step=2 ** 64 - 1),
               dict(flags=0x2), dict(flags=0x80000001, step=word.data_ptr()), dict(flags=0x1, step=0)] + [{k: None} for k in NAMES]
    for kw in refused:
        assert raw(**kw) != 0, kw
        assert b"ppg_record" in env._lib.ppg_last_error(env._handle), kw
    sync(env)
    for k, v in whole.items():
        assert raw_bytes(v) == before[k], (k, "a refused call wrote to its buffers")
    assert raw() == 0 and raw(step=T - 1) == 0 and raw(flags=0x1, step=word.data_ptr()) == 0   # (the accepted forms of the same call)
    sync(env)
    assert not bool(torch.isnan(views["reward"][0]).any()) and not bool(torch.isnan(views["reward"][T - 1]).any())

    d = fresh(env, T)
    env.record(*args(d), 0)
    wrong = [dict(reward=d["reward"].to(torch.float32)), dict(next_row=d["next_row"].to(torch.int32)), dict(in_use=d["in_use"].to(torch.int16)),
             dict(reward=d["reward"][:, :, :-1].contiguous()), dict(reward=d["reward"][0]), dict(truncated=d["truncated"][:1]),
             dict(terminated=d["terminated"].to(other_device)), dict(next_row=d["next_row"].to(other_device)),
             dict(truncated=d["truncated"].transpose(0, 1).contiguous().transpose(0, 1)),
             dict(reward=torch.zeros((T, B, 2 * S), dtype=torch.float64, device=env.device)[:, :, ::2])]
    for kw in wrong:
        with pytest.raises(ValueError):
            env.record(*args({**d, **kw}), 0)
    for t in (-1, T, word.to(torch.int64), torch.zeros((2,), dtype=torch.int32, device=env.device), word.to(other_device)):
        with pytest.raises(ValueError):
            env.record(*args(d), t)
    traj = AgentTrajectories(env, 2)
    traj.record().record()
    with pytest.raises(RuntimeError):
        traj.record()
    with pytest.raises(RuntimeError):
        traj.record_torch()
