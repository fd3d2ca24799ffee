"""Scenarios of `ppg_record_obs` (the observation rows in use appended to a compact per-species sample store; include/ppg.h,
csrc/ppg_obs_store.h), `env.record_obs()`, `trajectory.ObservationStore` and `AgentTrajectories(obs_rows=...)`, shared by the
wave-emulator tests (test_obs_store_emulated.py) and the GPU tests (test_obs_store_gpu.py).  No tests of its own.

The reference (`Ref`) is a numpy model of the store, advanced on the host after every call from `tables_of(env)`, `.cpu()` copies of
the env's observation tensors (as raw bits) and of the action tensor, following the text of include/ppg.h.  It uses no code from
predpreygrass_amd.trajectory.  Every comparison is byte equality of whole tensors: obs, sample, action, slot and cursor -- so a row
that should not have been written shows as well as one that should.  Every scenario that is not about overflow asserts that no row
was dropped: a kernel cannot pass by dropping rows.

Which copy loop of csrc/ppg_obs_store.h a geometry is here for (`GEOMETRIES`, `REACH`); `copy_arms` / `convert_arms` derive the
loops every copy of a run takes from the reference alone, and `geometry` holds each case to its arms on both backends:
    f64_7_9      float64, 7x7 / 9x9 windows: blocks of 1568 / 2592 bytes, every run 16-byte aligned -> the 16-byte main loop (four
                 loads in flight) and its tail; with PPG_OBS_F32 the converting loop without a head (784 / 1296 bytes per row)
    f32_3_7      float32, 3x3 / 7x7: 144 / 784 bytes, aligned, predator runs shorter than 64 lanes x 16 bytes
    bf16_1_1     bfloat16, 1x1: 8-byte rows -> destinations 8 bytes off a 16-byte line: the head words, bodies of a few 16-byte words
                 and the tail words (a run of ONE row that ends inside the head: tests/obs_store_san_main.cpp)
    bf16_3_5     bfloat16, 3x3 / 5x5: 72 / 200-byte rows -> head, 16-byte body from a source that is only 8-byte aligned, tail words
    drive_5_7    float64 drive-conditioned handle, 5 / 7 channels, 5x5 / 7x7: 1000 / 2744-byte rows (8 mod 16): head + body + tail;
                 with PPG_OBS_F32 rows of 500 / 1372 bytes (4 mod 16): heads of 1, 2 and 3 elements in front of the quads, and a tail
    walls_3_5    second generation, walls + visibility channel, float32, 5 channels: 180 / 500-byte rows (4 mod 16): heads of 1-3 words
    gen2_7_9     second generation, float32, 7x7 / 9x9: aligned
    bf16_shifted bf16_3_5 into store tensors that start 2 bytes into their allocation: nothing is 4-byte aligned -> the byte loop

A backend is an `image_cases.Backend(make, make_rq, sync)`: `make(cfg, B, **kw)` builds a BatchedPredPreyGrass, `make_rq(cfg, B, **kw)` a
BatchedRedQueen, both on the backend under test."""
import ctypes as C
import types

import numpy as np
import torch

from predpreygrass_amd import _abi
from tests import image_cases
from tests.image_cases import Geometry
from tests.link_cases import tables_of
from tests.record_cases import RECORDED, sync

UNSET = -128                                   # include/ppg.h: PPG_ACTION_UNSET
STEP_ON_DEVICE, F32 = 0x1, 0x2                 # PPG_OBS_STEP_ON_DEVICE, PPG_OBS_F32
FILL, GUARD = 0x5A, 64                         # bytes of a guarded store before a call, elements behind every tensor
N_ACTIONS = 5                                  # 0 .. 4 are actions of every family
# rows per env and step the stores of the RECORDED runs are sized for (predators, prey): above what the runs reach, below the
# [B,capacity] slabs; the runs assert that nothing was dropped
BUDGET = {"base": (24, 64), "p128": (128, 160), "gen2": (24, 64)}

GEOMETRIES = {
    "f64_7_9": Geometry("base", "float64", 7, 9, (4, 4), (64, 128), 12, 6, 1, {}),
    "f32_3_7": Geometry("base", "float32", 3, 7, (4, 4), (64, 64), 10, 6, 2, {}),
    "bf16_1_1": Geometry("base", "bfloat16", 1, 1, (4, 4), (64, 64), 8, 6, 4, {"initial_num_grass": 15}),
    "bf16_3_5": Geometry("base", "bfloat16", 3, 5, (4, 4), (64, 128), 10, 6, 3, {}),
    "drive_5_7": Geometry("base", "float64", 5, 7, (5, 7), (64, 128), 12, 6, 7,
                          {"enable_drive_channels": True, "predator_drive_channels": ["hunger_pressure"],
                           "prey_drive_channels": ["hunger_pressure", "reproductive_readiness", "grass_opportunity"]}),
    "walls_3_5": Geometry("walls", "float32", 3, 5, (5, 5), (64, 128), 12, 6, 5, {}),
    "gen2_7_9": Geometry("gen2", "float32", 7, 9, (4, 4), (64, 128), 14, 6, 8, {}),
}
# {geometry: {flags: arms that the copies of the run must reach}}
REACH = {
    "f64_7_9": {0: {"16B main", "16B tail"}, F32: {"f32 quads main", "f32 quads tail"}},
    "f32_3_7": {0: {"16B tail", "16B short"}},
    "bf16_1_1": {0: {"head", "16B short", "tail words"}},
    "bf16_3_5": {0: {"head", "16B tail", "tail words"}},
    "drive_5_7": {0: {"head", "16B main", "16B tail", "tail words"}, F32: {"f32 head 1", "f32 head 2", "f32 head 3", "f32 quads tail", "f32 tail"}},
    "walls_3_5": {0: {"head", "16B tail", "tail words"}},
    "gen2_7_9": {0: {"16B main"}},
}
_NP_BITS = {8: "<u8", 4: "<u4", 2: "<u2"}


def obs_bits(env, f32=False):
    """[pred, prey] as [B, rows, block] unsigned integers: the bits ppg_record_obs stores (f32: rounded to float32 first)."""
    out = []
    for t in (env.obs_pred, env.obs_prey):
        t = t.cpu()
        if f32 and t.dtype == torch.float64:
            t = torch.from_numpy(t.numpy().astype(np.float32))
        out.append(image_cases._obs_bits(t))
    return out


def bits_of(x):
    """A device tensor as a numpy array of unsigned integers of its element size."""
    x = x.detach().cpu().contiguous()
    return x.view(image_cases._BITS[x.element_size()]).numpy().view(_NP_BITS.get(x.element_size(), "u1")).copy()


def random_actions(env, gen):
    return torch.randint(0, N_ACTIONS, (env.batch_size, env.S), generator=gen, dtype=torch.int8).to(env.device)


class GuardedStore:
    """The tensors `env.record_obs()` takes, each a view of exactly its size at the head of an allocation filled with 0x5A bytes that
    goes on for GUARD elements behind it.  shift_obs: the observation tensors start that many ELEMENTS into the allocation."""

    def __init__(self, env, horizon, rows, f32=False, actions=True, shift_obs=0):
        self.horizon, self.capacity, self.f32 = int(horizon), (int(rows[0]), int(rows[1])), f32
        dev = env.device
        dtype = torch.float32 if f32 and env.obs_dtype == torch.float64 else env.obs_dtype
        self.whole = {}

        def guarded(name, shape, dt, shift=0):
            n = int(np.prod(shape))
            size = torch.empty((), dtype=dt).element_size()
            raw = torch.full(((shift + n + GUARD) * size,), FILL, dtype=torch.uint8, device=dev)
            self.whole[name] = (raw, shift * size, n * size)
            return raw[shift * size:(shift + n) * size].view(dt).view(shape)
        self.obs = [guarded(f"obs{s}", (n,) + tuple(src.shape[2:]), dtype, shift_obs)
                    for s, (n, src) in enumerate(zip(self.capacity, (env.obs_pred, env.obs_prey)))]
        self.sample = [guarded(f"sample{s}", (n,), torch.int32) for s, n in enumerate(self.capacity)]
        self.action = [guarded(f"action{s}", (n,), torch.int8) for s, n in enumerate(self.capacity)] if actions else None
        self.slot = guarded("slot", (self.horizon, env.batch_size, env.S), torch.int32)
        self.cursor = guarded("cursor", (4,), torch.int64)
        self.cursor.zero_()

    def tensors(self):
        d = {"slot": self.slot, "cursor": self.cursor}
        for s in (0, 1):
            d[f"obs{s}"], d[f"sample{s}"] = self.obs[s], self.sample[s]
            if self.action is not None:
                d[f"action{s}"] = self.action[s]
        return d

    def guards_untouched(self, tag):
        for name, (raw, lo, n) in self.whole.items():
            host = raw.cpu().numpy()
            assert (host[:lo] == FILL).all() and (host[lo + n:] == FILL).all(), (tag, name, "bytes outside the tensor were written")

    def snapshot(self):
        return {name: raw.cpu().numpy().copy() for name, (raw, _, _) in self.whole.items()}


def plain_tensors(store):
    """{name: tensor} of a trajectory.ObservationStore (or a GuardedStore)."""
    if isinstance(store, GuardedStore):
        return store.tensors()
    d = {"slot": store.slot, "cursor": store.cursor}
    for s in (0, 1):
        d[f"obs{s}"], d[f"sample{s}"] = store.obs[s], store.sample[s]
        if store.action is not None:
            d[f"action{s}"] = store.action[s]
    return d


class Ref:
    """The store in numpy.  It starts from the bytes the device tensors hold and is advanced by `record`, which restates the rules of
    include/ppg.h for one call."""

    def __init__(self, env, store):
        self.B, self.S, self.cp, self.cq = env.batch_size, env.S, env.pred_capacity, env.prey_capacity
        self.T, self.capacity, self.f32 = store.horizon, tuple(store.capacity), bool(getattr(store, "f32", False))
        self.t = {k: bits_of(v) for k, v in plain_tensors(store).items()}
        for s in (0, 1):
            self.t[f"obs{s}"] = self.t[f"obs{s}"].reshape(self.capacity[s], int(np.prod(store.obs[s].shape[1:])))
        self.slot, self.cursor = self.t["slot"].view("<i4"), self.t["cursor"].view("<i8")
        self.live = [0, 0]       # row-steps in use seen so far
        self.arms = {0: set(), 1: set()}

    def record(self, env, t, actions=None):
        """One call with a step index inside [0, T)."""
        es, obs = tables_of(env)["env_state"], obs_bits(env, self.f32)
        have_actions = actions is not None and "action0" in self.t and t > 0
        acts = actions.cpu().numpy() if have_actions else None
        self.slot[t] = -1
        for s, (first, cap, word) in enumerate(((0, self.cp, _abi.ENV_N_PRED_ROWS), (self.cp, self.cq, _abi.ENV_N_PREY_ROWS))):
            k = int(self.cursor[s])
            elem = self.t[f"obs{s}"].dtype.itemsize
            for b in range(self.B):
                n = min(max(int(es[b, word]), 0), cap)
                fit = min(n, max(self.capacity[s] - k, 0))
                self.t[f"obs{s}"][k:k + fit] = obs[s][b, :fit]
                self.t[f"sample{s}"][k:k + fit] = (t * self.B + b) * self.S + first + np.arange(fit)
                if "action0" in self.t:
                    self.t[f"action{s}"].view("i1")[k:k + fit] = UNSET
                self.slot[t, b, first:first + fit] = k + np.arange(fit)
                if fit:
                    blk_bytes = obs[s].shape[2] * elem
                    self.arms[s] |= (convert_arms if self.f32 and env.obs_dtype == torch.float64 else copy_arms)(k * blk_bytes, fit * blk_bytes)
                self.cursor[2 + s] += n - fit
                self.live[s] += n
                k += fit
            self.cursor[s] = k
            if have_actions:
                prev = self.slot[t - 1][:, first:first + cap]
                ok = (prev >= 0) & (prev < self.capacity[s])
                self.t[f"action{s}"].view("i1")[prev[ok]] = acts[:, first:first + cap][ok]

    def check(self, store, tag):
        for name, x in plain_tensors(store).items():
            got = bits_of(x).reshape(self.t[name].shape)
            if not np.array_equal(got, self.t[name]):
                at = np.argwhere(got != self.t[name])[0].tolist()
                raise AssertionError(f"{tag}: {name} differs first at {at}: got {got[tuple(at)]}, want {self.t[name][tuple(at)]}; "
                                     f"cursor {self.cursor.tolist()}")

    def counts(self):
        c = self.cursor.tolist()
        return (c[0], c[2]), (c[1], c[3])


def copy_arms(dst, nbytes):
    """The loops of obs_copy one run takes: destination offset `dst` into a 16-byte aligned store (the source of a run is the start of
    an env's region: 16-byte aligned), `nbytes` bytes, both multiples of 4."""
    assert dst % 4 == 0 and nbytes % 4 == 0
    arms = set()
    head = min((16 - dst % 16) % 16, nbytes)
    if head:
        arms.add("head")
        if head == nbytes:
            arms.add("ends in head")
    n16 = (nbytes - head) // 16
    arms |= image_cases._pack16_trips(n16)
    if nbytes - head - 16 * n16:
        arms.add("tail words")
    return arms


def convert_arms(dst, nbytes):
    """The loops of obs_copy_f32 for a run of nbytes / 4 elements at destination offset dst."""
    arms, n = set(), nbytes // 4
    head = min(((16 - dst % 16) % 16) // 4, n)
    if head:
        arms.add(f"f32 head {head}")
    n4 = (n - head) // 4
    for ln in range(64):   # (the two loops over the quads, lane by lane)
        i = ln
        while i + 64 < n4:
            arms.add("f32 quads main")
            i += 128
        if i < n4:
            arms.add("f32 quads tail")
    if n - head - 4 * n4:
        arms.add("f32 tail")
    return arms


def run(env, store, n_steps, gen, tag="", check_each=True):
    """n_steps of step(explicit random actions, auto_reset) + env.record_obs(store, t, actions), the reference advanced after every
    call and ALL tensors compared (check_each=False: the cursor after every call, all tensors at the end).  Returns (ref, seen)."""
    ref = Ref(env, store)
    seen = {"reset": 0, "birth": 0, "death": 0}
    for t in range(n_steps):
        actions = random_actions(env, gen)
        env.step(actions, auto_reset=True)
        env.record_obs(store, t, actions, f32=getattr(store, "f32", False))
        sync(env)
        ref.record(env, t, actions)
        if check_each or t == n_steps - 1:
            ref.check(store, f"{tag} step {t}")
        assert store.cursor.tolist() == ref.cursor.tolist(), (tag, t, store.cursor.tolist(), ref.cursor.tolist())
        cur = tables_of(env)
        for b in range(env.batch_size):
            n = (int(cur["env_state"][b, _abi.ENV_N_PRED_ROWS]), int(cur["env_state"][b, _abi.ENV_N_PREY_ROWS]))
            flags = np.concatenate([cur["row_flags"][b, :n[0]], cur["row_flags"][b, env.pred_capacity:env.pred_capacity + n[1]]])
            seen["reset"] += bool(int(cur["env_state"][b, _abi.ENV_FLAGS]) & _abi.ENVF_WAS_RESET)
            seen["birth"] += int(((flags & _abi.ROW_NEWBORN) != 0).sum())
            seen["death"] += int(((flags & _abi.ROW_DIED) != 0).sum())
    return ref, seen


def nothing_dropped(ref, tag):
    (sp, dp), (sq, dq) = ref.counts()
    assert dp == 0 and dq == 0, (tag, "rows were dropped", ref.counts())
    assert [sp, sq] == ref.live and sp > 0 and sq > 0, (tag, ref.counts(), ref.live)


# ---- 1. against numpy on the RECORDED configs ------------------------------------------------------------------------------------

def against_numpy(env, name, n_steps):
    from predpreygrass_amd.trajectory import ObservationStore   # (the tensors only; the reference does not use it)
    B = env.batch_size
    env.reset()
    store = ObservationStore(env, n_steps, tuple(n_steps * B * r for r in BUDGET[name]))
    ref, seen = run(env, store, n_steps, torch.Generator().manual_seed(11), tag=name, check_each=False)
    nothing_dropped(ref, name)
    for k in ("reset", "birth", "death"):
        assert seen[k] > 0, (k, seen)   # (the run must not pass vacuously)
    for s in (0, 1):   # actions reached the store, and the last step's samples are still unset
        a = store.action[s][:ref.counts()[s][0]].cpu().numpy()
        assert ((a >= 0) & (a < N_ACTIONS)).any() and (a == UNSET).any(), (name, s)
    assert store.counts() == ref.counts()
    return ref


# ---- 2. geometries ------------------------------------------------------------------------------------------------------------

def new_env(bk, gid, B):
    g = GEOMETRIES[gid]
    env = image_cases.new_handle(bk, g, B, seed=g.seed)
    if g.family == "walls":
        env.set_walls(image_cases._WALLS)
    env.reset()
    return env


def geometry(bk, gid, B=5):
    """Every flag set of REACH[gid]: g.calls steps into a guarded store, every tensor compared after every call, the arms reached
    (by the predator and the prey copies together)."""
    g = GEOMETRIES[gid]
    for flags, want in REACH[gid].items():
        env = new_env(bk, gid, B)
        T = g.calls
        store = GuardedStore(env, T, (T * B * g.caps[0], T * B * g.caps[1]), f32=bool(flags & F32))
        ref, _ = run(env, store, T, torch.Generator().manual_seed(g.seed), tag=f"{gid} flags {flags}")
        nothing_dropped(ref, gid)
        store.guards_untouched(gid)
        assert want <= ref.arms[0] | ref.arms[1], (gid, flags, sorted(ref.arms[0]), sorted(ref.arms[1]))
        if flags & F32:
            assert store.obs[0].dtype == torch.float32 and env.obs_pred.dtype == torch.float64
        assert bool((store.obs[0] != 0).any()) and bool((store.obs[1] != 0).any()), (gid, "only zeros were stored")
        env.close()


def geometry_shifted_store(bk):
    """bf16_3_5 into observation tensors that start one element (2 bytes) into their allocation: the byte loop."""
    env = new_env(bk, "bf16_3_5", 3)
    store = GuardedStore(env, 4, (4 * 3 * 64, 4 * 3 * 128), shift_obs=1)
    assert store.obs[0].data_ptr() % 4 == 2 and store.obs[1].data_ptr() % 4 == 2
    ref, _ = run(env, store, 4, torch.Generator().manual_seed(5), tag="shifted store")
    nothing_dropped(ref, "shifted store")
    store.guards_untouched("shifted store")


# ---- 3. batch sizes ---------------------------------------------------------------------------------------------------------------

def batch_size(bk, B, T=3):
    """One handle of B envs: the scan's lanes get (B + 63) // 64 envs each, the last ones fewer or none."""
    env = new_env(bk, "f32_3_7", B)
    store = GuardedStore(env, T, (T * B * 16, T * B * 40))
    ref, _ = run(env, store, T, torch.Generator().manual_seed(B), tag=f"B={B}")
    nothing_dropped(ref, f"B={B}")
    store.guards_untouched(f"B={B}")
    return ref


# ---- 4. capacity --------------------------------------------------------------------------------------------------------------

def _row_counts(bk, gid, B, T, seed):
    """[T,B,2] rows in use of a run (a twin env, the same seeds and actions as the run that follows)."""
    env = new_env(bk, gid, B)
    gen, out = torch.Generator().manual_seed(seed), []
    for _ in range(T):
        env.step(random_actions(env, gen), auto_reset=True)
        es = tables_of(env)["env_state"]
        out.append(np.stack([es[:, _abi.ENV_N_PRED_ROWS], es[:, _abi.ENV_N_PREY_ROWS]], axis=1).astype(np.int64))
    env.close()
    return np.stack(out)


def capacity_cut(bk, gid="bf16_3_5", B=5, T=5):
    """Stores sized so that the predator store ends inside the predator run of env 2 at step 1 and the prey store inside the prey run of
    env 3 at step 2: the rows behind the cut are dropped whole (slot -1), later calls drop everything, stored + dropped = the rows in
    use, nothing behind `capacity` rows is written."""
    counts = _row_counts(bk, gid, B, T, seed=21)
    assert counts[1, 2, 0] >= 2 and counts[2, 3, 1] >= 2, counts[:3]
    cap_p = int(counts[0, :, 0].sum() + counts[1, :2, 0].sum() + counts[1, 2, 0] // 2)
    cap_q = int(counts[:2, :, 1].sum() + counts[2, :3, 1].sum() + counts[2, 3, 1] // 2)
    env = new_env(bk, gid, B)
    store = GuardedStore(env, T, (cap_p, cap_q))
    ref, _ = run(env, store, T, torch.Generator().manual_seed(21), tag="capacity cut")
    store.guards_untouched("capacity cut")
    (sp, dp), (sq, dq) = ref.counts()
    assert (sp, sq) == (cap_p, cap_q) and [sp + dp, sq + dq] == ref.live == counts.sum(axis=(0, 1)).tolist(), (ref.counts(), ref.live)
    slot = store.slot.cpu().numpy()
    cp = env.pred_capacity
    # the cut fell inside the two runs: some of their rows have a slot, the rest -1
    for (t, b, s) in ((1, 2, 0), (2, 3, 1)):
        run_slots = slot[t, b, (cp if s else 0):(cp if s else 0) + counts[t, b, s]]
        assert (run_slots >= 0).any() and (run_slots == -1).any() and run_slots.max() == (cap_p, cap_q)[s] - 1, (t, b, s, run_slots)
    # later calls drop everything
    assert (slot[2:, :, :cp] == -1).all() and (slot[3:, :, cp:] == -1).all()
    # every dropped row has slot -1: the slots handed out are exactly 0 .. capacity - 1, once each
    for s, sl in enumerate((slot[:, :, :cp], slot[:, :, cp:])):
        assert sorted(sl[sl >= 0].tolist()) == list(range((cap_p, cap_q)[s]))
    assert tuple(map(tuple, store.cursor.cpu().numpy().reshape(2, 2).T.tolist())) == ref.counts()


def capacity_zero(bk, gid="bf16_3_5", B=3, T=3):
    """capacity 0 for one species (its tensors are empty): all its rows are dropped, the other species is stored as usual."""
    for zero in (0, 1):
        env = new_env(bk, gid, B)
        rows = [T * B * 64, T * B * 128]
        rows[zero] = 0
        store = GuardedStore(env, T, rows)
        ref, _ = run(env, store, T, torch.Generator().manual_seed(3), tag=f"capacity[{zero}] = 0")
        store.guards_untouched(f"capacity[{zero}] = 0")
        counts = ref.counts()
        assert counts[zero] == (0, ref.live[zero]) and counts[1 - zero] == (ref.live[1 - zero], 0) and min(ref.live) > 0, (counts, ref.live)
        slot = store.slot.cpu().numpy()
        cp = env.pred_capacity
        assert ((slot[:, :, :cp] if zero == 0 else slot[:, :, cp:]) == -1).all()


# ---- 5. the step index on the device ------------------------------------------------------------------------------------------

def device_step_index(bk, gid="bf16_3_5", B=3, T=4):
    """The same bytes as the host index on a twin; a word outside [0, T) changes nothing, the cursor included."""
    env, twin = new_env(bk, gid, B), new_env(bk, gid, B)
    rows = (T * B * 64, T * B * 128)
    a, b = GuardedStore(env, T, rows), GuardedStore(twin, T, rows)
    word = torch.zeros((1,), dtype=torch.int32, device=env.device)
    gen_a, gen_b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    for t in range(T):
        for e, st, gen, step in ((env, a, gen_a, word), (twin, b, gen_b, t)):
            actions = random_actions(e, gen)
            e.step(actions, auto_reset=True)
            e.record_obs(st, step, actions)
        word.add_(1)
    sync(env)
    for (name, x), y in zip(a.tensors().items(), b.tensors().values()):
        assert np.array_equal(bits_of(x), bits_of(y)), name
    assert int(a.cursor[0]) > 0 and int(a.cursor[1]) > 0 and a.cursor[2:].tolist() == [0, 0]
    for value in (T, T + 7, -1, -2 ** 31, 2 ** 31 - 1):
        word.fill_(value)
        before = a.snapshot()
        actions = random_actions(env, gen_a)
        env.step(actions, auto_reset=True)
        env.record_obs(a, word, actions)
        sync(env)
        for name, raw in a.snapshot().items():
            assert np.array_equal(raw, before[name]), (value, name, "a call past the horizon wrote")


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------

def argument_checking(bk, other_device, gid="bf16_3_5", B=2, T=3):
    """Every PPG_EINVAL case of ppg_record_obs returns non-zero, names ppg_record_obs in ppg_last_error and leaves the tensors and the
    cursor untouched; the Python wrapper raises ValueError on a wrong dtype, shape, device, a short tensor or a bad step."""
    import pytest
    env = new_env(bk, gid, B)
    env.step(random_actions(env, torch.Generator().manual_seed(1)))
    rows = (T * B * 64, T * B * 128)
    store = GuardedStore(env, T, rows)
    word = torch.zeros((1,), dtype=torch.int32, device=env.device)
    before = store.snapshot()

    def raw(st=True, horizon=T, step=0, flags=0, capacity=rows, null=(), handle=env):
        s = _abi.PpgObsStore()
        s.horizon = horizon
        for i in (0, 1):
            s.obs[i] = None if f"obs{i}" in null else store.obs[i].data_ptr()
            s.sample[i] = None if f"sample{i}" in null else store.sample[i].data_ptr()
            s.action[i] = None if f"action{i}" in null else store.action[i].data_ptr()
            s.capacity[i] = capacity[i]
        s.slot = None if "slot" in null else store.slot.data_ptr()
        s.cursor = None if "cursor" in null else store.cursor.data_ptr()
        return handle._lib.ppg_record_obs(handle._handle, C.byref(s) if st else None, step, flags, None, handle._stream())
    refused = [dict(st=False), dict(horizon=0), dict(horizon=-3), dict(step=T), dict(step=2 ** 63), dict(step=2 ** 64 - 1),
               dict(capacity=(-1, rows[1])), dict(capacity=(rows[0], -(2 ** 40))), dict(capacity=(2 ** 31, rows[1])),
               dict(horizon=2 ** 31 - 1), dict(flags=0x4), dict(flags=0x80000001, step=word.data_ptr()), dict(flags=STEP_ON_DEVICE, step=0),
               dict(flags=F32), dict(null=("action0",)), dict(null=("action1",))] + \
              [dict(null=(k,)) for k in ("slot", "cursor", "sample0", "sample1", "obs0", "obs1")]
    for kw in refused:
        assert raw(**kw) == -1, kw
        assert b"ppg_record_obs" in env._lib.ppg_last_error(env._handle), kw
    sync(env)
    for name, now in store.snapshot().items():
        assert np.array_equal(now, before[name]), (name, "a refused call wrote")
    # (the accepted forms of the same call: both action pointers NULL, the last step, the device word, capacity 0)
    assert raw(null=("action0", "action1")) == 0 and raw(step=T - 1) == 0 and raw(flags=STEP_ON_DEVICE, step=word.data_ptr()) == 0
    f64 = new_env(bk, "f64_7_9", 1)   # PPG_OBS_F32 is refused for bfloat16 rows only
    st64 = GuardedStore(f64, 1, (64, 128), f32=True)
    f64.record_obs(st64, 0, f32=True)
    sync(env)
    assert int(store.cursor[0]) > 0 and int(st64.cursor[0]) > 0
    assert raw(capacity=(0, 0)) == 0

    good = GuardedStore(env, T, rows)
    acts = random_actions(env, torch.Generator().manual_seed(2))
    env.record_obs(good, 0, acts)

    def variant(**kw):
        v = types.SimpleNamespace(horizon=good.horizon, capacity=good.capacity, obs=list(good.obs), sample=list(good.sample),
                                  action=list(good.action), slot=good.slot, cursor=good.cursor)
        for k, x in kw.items():
            if isinstance(getattr(v, k), list) and isinstance(x, torch.Tensor):
                getattr(v, k)[0] = x
            else:
                setattr(v, k, x)
        return v
    wrong = [dict(obs=good.obs[0].to(torch.float32)), dict(obs=good.obs[0][:, :, :, :-1].contiguous()), dict(obs=good.obs[0][:-1]),
             dict(obs=good.obs[0].to(other_device)), dict(sample=good.sample[0].to(torch.int64)), dict(sample=good.sample[0][:5]),
             dict(action=good.action[0].to(torch.uint8)), dict(slot=good.slot[:, :, :-1].contiguous()), dict(slot=good.slot.to(torch.int64)),
             dict(cursor=good.cursor.to(torch.int32)), dict(cursor=good.cursor[:3]), dict(capacity=(-1, rows[1])),
             dict(slot=torch.zeros((T, B, 2 * env.S), dtype=torch.int32, device=env.device)[:, :, ::2])]
    for kw in wrong:
        with pytest.raises(ValueError):
            env.record_obs(variant(**kw), 0, acts)
    for t in (-1, T, word.to(torch.int64), word.to(other_device)):
        with pytest.raises(ValueError):
            env.record_obs(good, t, acts)
    for bad in (acts.to(torch.int32), acts[:, :-1].contiguous(), acts.to(other_device)):
        with pytest.raises(ValueError):
            env.record_obs(good, 1, bad)
    with pytest.raises(ValueError):
        env.record_obs(variant(action=None), 1, acts)   # actions for a store that keeps none
    with pytest.raises(ValueError):
        env.record_obs(good, 1, acts, f32=True)         # bfloat16 rows


# ---- 7. AgentTrajectories(obs_rows=...) ----------------------------------------------------------------------------------------

def trajectories(env, twin, plain, T=8):
    """samples() and flat() against boolean-mask indexing of the [T,B,S] tensors; record_obs_torch() on a twin gives the same bytes;
    a trajectory without obs_rows on a third env of the same seed holds the same five tensors."""
    import pytest
    from predpreygrass_amd.trajectory import AgentTrajectories, ObservationStore
    from tests.record_cases import of, same_tensors
    B, S, cp = env.batch_size, env.S, env.pred_capacity
    rows = (T * B * 32, T * B * 96)
    for e in (env, twin, plain):
        e.reset()
    a, b, c = AgentTrajectories(env, T, obs_rows=rows), AgentTrajectories(twin, T, obs_rows=rows), AgentTrajectories(plain, T)
    assert isinstance(a.store, ObservationStore) and c.store is None
    with pytest.raises(RuntimeError):
        c.samples(0)
    gen = torch.Generator().manual_seed(17)
    obs_seen = [[], []]
    for t in range(T):
        actions = random_actions(env, gen)
        for e in (env, twin, plain):
            e.step(actions, auto_reset=True)
        a.record(actions)
        b.record_obs_torch(actions)
        c.record()
        for s, x in enumerate((env.obs_pred, env.obs_prey)):
            obs_seen[s].append(x.clone())
    sync(env)
    assert len(a) == len(b) == len(c) == T
    same_tensors(of(a), of(b), "kernel against torch ops")
    same_tensors(of(a), of(c), "with and without a store")
    for (name, x), y in zip(plain_tensors(a.store).items(), plain_tensors(b.store).values()):
        assert np.array_equal(bits_of(x), bits_of(y)), (name, "record_obs_torch() on the twin differs")
    (sp, dp), (sq, dq) = a.store.counts()
    assert dp == dq == 0 and sp > 0 and sq > 0
    G = torch.rand((T, B, S), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(env.device)
    species = torch.arange(S, device=env.device) >= cp
    for s in (0, 1):
        mask = a.in_use & (species == bool(s))                     # [T,B,S]: boolean-mask indexing runs in (t, b, r) order
        n, obs, index, action = a.samples(s)
        assert n == int(mask.sum()) == (sp, sq)[s]
        assert torch.equal(index, mask.reshape(-1).nonzero().reshape(-1)) and index.dtype == torch.int64
        assert torch.equal(a.flat(G, s), G[mask])
        seen = torch.stack(obs_seen[s])                             # [T,B,cap,C,R,R]
        want = seen[mask[:, :, cp:] if s else mask[:, :, :cp]]
        assert obs.shape == want.shape and torch.equal(bits_view(obs), bits_view(want))
        assert action.shape == (n,) and bool((action[index < (T - 1) * B * S] != UNSET).any()) and bool((action[index >= (T - 1) * B * S] == UNSET).all())
    a.clear()
    assert a.store.counts() == ((0, 0), (0, 0)) and len(a) == 0


def bits_view(x):
    return x.contiguous().view(image_cases._BITS[x.element_size()])
