"""Scenarios of `ppg_record_logp` (the behaviour policy's log-probabilities, entropies and logits written into the slots of a sample
store; include/ppg.h, csrc/ppg_logp.h), `env.record_logp()`, `ObservationStore(logp=...)`, `AgentTrajectories.record_policy()` /
`behaviour()` / `scatter()`, shared by the wave-emulator tests (test_logp_emulated.py) and the GPU tests (test_logp_gpu.py).  No tests
of its own.

The logits are synthetic tensors here (the policy kernels have no CPU path; test_logp_gpu.py adds the real policy).  The reference
(`ref_rows`, `LogpRef`) is plain numpy float64 from the same float32 logits -- max-shifted log-sum-exp summed in ascending action order
and the entropy formula of include/ppg.h -- placed through the slot table of the numpy store model of tests/obs_store_cases.py (`Ref`),
which follows the text of include/ppg.h and uses no code of predpreygrass_amd.trajectory.

Tolerance of `logp` and `entropy` (`close`): |got - float32(ref)| <= max(1 float32 ulp of ref, 1e-11).  Both sides compute in float64
with exp / log good to about an ulp of double and round once, so they can differ only where the two float64 results straddle a
float32 rounding boundary: one ulp.  The absolute floor is for entropies near zero, where the float64 error itself -- 32 terms of
|l - m| <= 256 times a few 2^-53, about 2e-12 -- exceeds an ulp of the result.  +-inf and NaN must agree exactly.  `dist` and every
element the call must not touch -- NaN-filled slots of other steps and of dropped rows, the guard bytes around every tensor, slot,
cursor, obs, sample, action -- are compared bit for bit."""
import ctypes as C
import types

import numpy as np
import torch

from predpreygrass_amd import _abi
from tests import image_cases
from tests import obs_store_cases as oc
from tests.link_cases import tables_of
from tests.obs_store_cases import FILL, GUARD, UNSET, GuardedStore, Ref, bits_of, new_env, random_actions
from tests.record_cases import RECORDED, sync

STEP_ON_DEVICE = 0x1                            # PPG_LOGP_STEP_ON_DEVICE
ROLLOUT_ACTIONS = {"base": (9, 9), "gen2": (25, 25)}
NEG_INF = float("-inf")


# ---- the reference ------------------------------------------------------------------------------------------------------------

def ref_rows(rows, acts):
    """(logp, entropy) as float32 [n] of float32 logits rows [n,A] at the actions acts [n]: float64, rounded once."""
    n, A = rows.shape
    acts = np.asarray(acts, dtype=np.int64)
    with np.errstate(all="ignore"):
        l = rows.astype(np.float64)
        d = l - l.max(axis=1, keepdims=True)      # (a NaN in a row makes the whole row NaN; all -inf gives -inf - -inf = NaN)
        masked = np.isneginf(d)
        e = np.where(masked, 0.0, np.exp(d))
        s, w = np.zeros(n), np.zeros(n)
        for a in range(A):                          # ascending a; a masked action adds exactly 0 to both sums
            s = s + e[:, a]
            w = w + np.where(masked[:, a], 0.0, e[:, a] * d[:, a])
        ls = np.log(s)
        valid = (acts >= 0) & (acts < A)
        lp = np.where(valid, d[np.arange(n), np.clip(acts, 0, A - 1)] - ls, np.nan)
        h = ls - w / s
    return lp.astype(np.float32), h.astype(np.float32)


def close(got, want, tag):
    """got within max(1 float32 ulp of want, 1e-11) of want; NaN and +-inf in exactly the same places."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN in other places", np.argwhere(np.isnan(got) != nan)[:5].tolist())
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (tag, "+-inf differ")
    fin = ~nan & ~inf
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    tol = np.maximum(np.spacing(np.abs(want[fin])).astype(np.float64), 1e-11)
    bad = np.abs(g - w) > tol
    assert not bad.any(), (tag, int(bad.sum()), "of", bad.size, "outside the tolerance; first:", g[bad][:3], w[bad][:3])


class GuardedLogpStore(GuardedStore):
    """A GuardedStore plus logp / entropy / dist, each a view of exactly its size in front of GUARD elements of 0x5A bytes; logp and
    entropy start filled with NaN (what ObservationStore does), dist keeps the 0x5A bytes."""

    def __init__(self, env, horizon, rows, n_actions, entropy=True, dist=True, **kw):
        super().__init__(env, horizon, rows, **kw)
        self.n_actions = (int(n_actions[0]), int(n_actions[1]))

        def guarded(name, shape, nan):
            n = int(np.prod(shape))
            raw = torch.full(((n + GUARD) * 4,), FILL, dtype=torch.uint8, device=env.device)
            self.whole[name] = (raw, 0, n * 4)
            x = raw[:n * 4].view(torch.float32).view(shape)
            if nan:
                x.fill_(float("nan"))
            return x
        self.logp = [guarded(f"logp{s}", (n,), True) for s, n in enumerate(self.capacity)]
        self.entropy = [guarded(f"entropy{s}", (n,), True) for s, n in enumerate(self.capacity)] if entropy else None
        self.dist = [guarded(f"dist{s}", (n, a), False) for s, (n, a) in enumerate(zip(self.capacity, self.n_actions))] if dist else None


def policy_tensors(store):
    d = {}
    for s in (0, 1):
        d[f"logp{s}"] = store.logp[s]
        if store.entropy is not None:
            d[f"entropy{s}"] = store.entropy[s]
        if store.dist is not None:
            d[f"dist{s}"] = store.dist[s]
    return d


class LogpRef:
    """logp / entropy / dist of a store in numpy: starts from the bits the device tensors hold, `record` restates one call."""

    def __init__(self, env, store):
        self.B, self.S, self.cp, self.cq, self.T = env.batch_size, env.S, env.pred_capacity, env.prey_capacity, int(store.horizon)
        self.capacity, self.A = tuple(store.capacity), tuple(store.n_actions)
        self.bits = {k: bits_of(v) for k, v in policy_tensors(store).items()}          # uint32; floats are views of these
        self.first = {k: v.copy() for k, v in self.bits.items()}
        self.written = [np.zeros(n, bool) for n in self.capacity]

    def rows_of(self, env, t, slot):
        """Per species: (k, i, b, r) of every row in use at a slot inside the capacity, i = its logits row."""
        es = tables_of(env)["env_state"]
        out = []
        for s, (first, cap, word) in enumerate(((0, self.cp, _abi.ENV_N_PRED_ROWS), (self.cp, self.cq, _abi.ENV_N_PREY_ROWS))):
            i, found = 0, []
            for b in range(self.B):
                n = min(max(int(es[b, word]), 0), cap)
                for j in range(n):
                    k = int(slot[t, b, first + j])
                    if 0 <= k < self.capacity[s]:
                        found.append((k, i + j, b, first + j))
                i += n
            out.append(np.array(found, dtype=np.int64).reshape(-1, 4))
        return out

    def record(self, env, t, logits, actions, slot):
        """One call for the recorded step t (outside [0, T): nothing).  slot: int32 [T,B,S], the numpy model's."""
        if not 0 <= t < self.T:
            return
        acts = actions.cpu().numpy()
        for s, found in enumerate(self.rows_of(env, t, slot)):
            if logits[s] is None or not len(found):
                continue
            k, i, b, r = found.T
            rows = logits[s].cpu().numpy()[i]
            lp, h = ref_rows(rows, acts[b, r])
            self.bits[f"logp{s}"].view("<f4")[k] = lp
            if f"entropy{s}" in self.bits:
                self.bits[f"entropy{s}"].view("<f4")[k] = h
            if f"dist{s}" in self.bits:
                self.bits[f"dist{s}"].reshape(self.capacity[s], self.A[s])[k] = rows.view("<u4")
            self.written[s][k] = True

    def check(self, store, tag):
        for name, x in policy_tensors(store).items():
            s = int(name[-1])
            got, want = bits_of(x).reshape(self.bits[name].shape), self.bits[name]
            if name.startswith("dist"):
                assert np.array_equal(got, want), (tag, name, "differs bit for bit", np.argwhere(got != want)[:3].tolist())
                continue
            w = self.written[s]
            assert np.array_equal(got[~w], self.first[name][~w]), (tag, name, "a slot no call was to write has changed")
            close(got.view("<f4")[w], want.view("<f4")[w], f"{tag} {name}")


# ---- logits and actions of a call ---------------------------------------------------------------------------------------------

def synthetic(env, gen, A, scale=3.0):
    """([logits_pred, logits_prey] float32 [B * capacity_s, A_s], random in EVERY row; actions int8 [B,S], valid for each species)."""
    B, cp, cq, dev = env.batch_size, env.pred_capacity, env.prey_capacity, env.device
    logits = [(torch.randn((B * cap, a), generator=gen) * scale).to(torch.float32).to(dev) for cap, a in zip((cp, cq), A)]
    acts = torch.cat([torch.randint(0, a, (B, cap), generator=gen, dtype=torch.int8) for cap, a in zip((cp, cq), A)], dim=1)
    return logits, acts.contiguous().to(dev)


def special_rows(A, rng):
    """[(name, float32 [A], action or None = any valid one)]: the logit values of the issue that fit A actions."""
    def rnd():
        return (rng.standard_normal(A) * 3).astype(np.float32)
    out = [("equal", np.full(A, 0.25, np.float32), None),
           ("+-80", np.where(np.arange(A) % 2 == 0, 80.0, -80.0).astype(np.float32), None),
           ("148", np.concatenate([[148.0], rng.uniform(-148, 148, A - 1)]).astype(np.float32), A - 1),
           ("ordinary", rnd(), None),
           ("all -inf", np.full(A, NEG_INF, np.float32), None),
           ("a NaN", np.concatenate([rnd()[:A - 1], [np.nan]]).astype(np.float32), 0)]
    if A > 1:
        x = rnd(); x[A // 2] = NEG_INF
        out.append(("one -inf", x, 0 if A // 2 else 1))
        x = rnd(); x[A // 2] = NEG_INF
        out.append(("-inf at the action", x, A // 2))
        out.append(("near-zero entropy", np.concatenate([[0.0], np.full(A - 1, -20.0)]).astype(np.float32), 0))
        out.append(("-148 at the action", np.concatenate([[148.0], np.full(A - 1, -148.0)]).astype(np.float32), A - 1))
    if A > 2:
        x = np.full(A, NEG_INF, np.float32); x[1] = 1.5; x[A - 1] = -0.5
        out.append(("several -inf", x, 1))
    for bad in (UNSET, A, -1, 127):   # actions outside [0, A): NaN logp; entropy and dist still written
        out.append((f"action {bad}", rnd(), bad))
    return out


def float32_implementations_fail():
    """The value rows tell a float32 or non-max-shifted implementation from the reference (so the cases can fail)."""
    with np.errstate(all="ignore"):
        big = np.array([[148.0, -148.0, 3.0]], np.float32)
        naive = big[0, 1] - np.log(np.exp(big[0]).sum(dtype=np.float32))             # float32, not shifted: exp(148) overflows
        assert not np.isfinite(naive) and np.isfinite(ref_rows(big, [1])[0][0])
        row = np.concatenate([[0.0], np.full(8, -20.0)]).astype(np.float32)[None]      # float32, shifted: 1 + 8 e^-20 rounds to 1
        e = np.exp(row[0] - row[0].max()).astype(np.float32)
        s = e.sum(dtype=np.float32)
        h32 = np.float32(np.log(s) - (e * row[0]).sum(dtype=np.float32) / s)
        want = ref_rows(row, [0])[1][0]
        assert abs(float(h32) - float(want)) > 100 * max(float(np.spacing(want)), 1e-11), (h32, want)


def with_special_rows(env, lref, t, slot, A, gen, rng):
    """synthetic(), with the rows of special_rows() dealt out over the rows in use of both species (each pattern several times) and
    their actions set.  Returns (logits, actions, {(species, pattern): [slots]})."""
    logits, acts = synthetic(env, gen, A)
    host, a_host, where = [x.cpu().numpy().copy() for x in logits], acts.cpu().numpy().copy(), {}
    for s, found in enumerate(lref.rows_of(env, t, slot)):
        pats = special_rows(A[s], rng)
        for q, (k, i, b, r) in enumerate(found.tolist()):
            name, row, action = pats[q % len(pats)]
            host[s][i] = row
            if action is not None:
                a_host[b, r] = action
            where.setdefault((s, name), []).append(k)
    return [torch.from_numpy(x).to(env.device) for x in host], torch.from_numpy(a_host).to(env.device), where


def stepped(env, store, ref, t, gen):
    """One env step with explicit random actions and auto-reset, stored as step t; the numpy store model follows."""
    actions = random_actions(env, gen)
    env.step(actions, auto_reset=True)
    env.record_obs(store, t, actions)
    sync(env)
    ref.record(env, t, actions)


def run(env, store, T, A, seed, tag, logits_of=None, every=None):
    """T times: step + record_obs as step t, then synthetic logits / actions and env.record_logp(store, t, ...); both numpy models
    follow and all policy tensors are compared after every call, the store's own tensors and the guards at the end."""
    ref, lref = Ref(env, store), LogpRef(env, store)
    gen, gen2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 1000)
    for t in range(T):
        stepped(env, store, ref, t, gen)
        if every is not None:
            every(t, ref)
        logits, acts = synthetic(env, gen2, A)
        if logits_of is not None:
            logits = logits_of(logits)
        env.record_logp(store, t, logits, acts)
        sync(env)
        lref.record(env, t, logits, acts, ref.slot)
        lref.check(store, f"{tag} step {t}")
    ref.check(store, f"{tag}: the store's own tensors")
    store.guards_untouched(tag)
    return ref, lref


# ---- 1. rollouts through AgentTrajectories -----------------------------------------------------------------------------------

def rollout(env, name):
    """The RECORDED run `name` (births, deaths, auto-resets): record_policy() between act and step at EVERY step, the first one
    (nothing recorded yet: nothing written) included."""
    from predpreygrass_amd.trajectory import AgentTrajectories
    cfg, kw, T = RECORDED[name]
    A, B, S = ROLLOUT_ACTIONS[name], env.batch_size, env.S
    env.reset()
    traj = AgentTrajectories(env, T, obs_rows=tuple(T * B * r for r in oc.BUDGET[name]), logp=A, dist=True)
    store = traj.store
    ref, lref = Ref(env, store), LogpRef(env, store)
    gen, gen2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(12)
    resets = 0
    for t in range(T):
        logits, acts = synthetic(env, gen2, A)
        traj.record_policy(logits, acts)            # the policy that acted on the output stored as step t - 1
        if t > 0:
            lref.record(env, t - 1, logits, acts, ref.slot)
        else:
            sync(env)
            assert all(bool(torch.isnan(x).all()) for x in store.logp + store.entropy), "record_policy() before any record() wrote"
        actions = random_actions(env, gen)
        env.step(actions, auto_reset=True)
        traj.record(actions)
        sync(env)
        ref.record(env, t, actions)
        resets += int((tables_of(env)["env_state"][:, _abi.ENV_FLAGS] & _abi.ENVF_WAS_RESET != 0).sum())
    assert resets > 0, "the run saw no auto-reset"
    ref.check(store, name)
    lref.check(store, name)
    oc.nothing_dropped(ref, name)
    for s in (0, 1):
        n, _, index, _ = traj.samples(s)
        logp, entropy, dist = traj.behaviour(s)
        assert logp.shape == (n,) and entropy.shape == (n,) and dist.shape == (n, A[s]) and n > 0
        last = (index >= (T - 1) * B * S).cpu().numpy()
        lp = logp.cpu().numpy()
        assert np.isfinite(lp[~last]).all() and (lp[~last] <= 0).all() and np.isnan(lp[last]).all() and last.any() and (~last).any()
    traj.clear()
    assert all(bool(torch.isnan(x).all()) for x in store.logp + store.entropy) and store.counts() == ((0, 0), (0, 0))


# ---- 2. logit values, action values, action counts ------------------------------------------------------------------------------

def values(bk, A, B=5, T=3):
    """Every row in use carries one of special_rows(): all equal, +-80, 148, -inf (one, several, at the action, the whole row), a
    NaN, an entropy near zero; actions PPG_ACTION_UNSET, A, -1 and 127."""
    float32_implementations_fail()
    env = new_env(bk, "f32_3_7", B)
    store = GuardedLogpStore(env, T, (T * B * 16, T * B * 40), A)
    ref, lref = Ref(env, store), LogpRef(env, store)
    gen, gen2, rng = torch.Generator().manual_seed(31), torch.Generator().manual_seed(32), np.random.default_rng(33)
    for t in range(T):
        stepped(env, store, ref, t, gen)
        logits, acts, where = with_special_rows(env, lref, t, ref.slot, A, gen2, rng)
        env.record_logp(store, t, logits, acts)
        sync(env)
        lref.record(env, t, logits, acts, ref.slot)
        lref.check(store, f"A={A} step {t}")
        for s in (0, 1):
            lp, h = store.logp[s].cpu().numpy(), store.entropy[s].cpu().numpy()
            names = {name for (sp, name) in where if sp == s}
            assert {"equal", "148", "all -inf", "a NaN", f"action {UNSET}", f"action {A[s]}", "action -1", "action 127"} <= names, names
            for name in names:
                k = where[(s, name)]
                if name.startswith("action "):        # no such action: NaN logp, the entropy all the same
                    assert np.isnan(lp[k]).all() and np.isfinite(h[k]).all(), (s, name)
                elif name in ("all -inf", "a NaN"):
                    assert np.isnan(lp[k]).all() and np.isnan(h[k]).all(), (s, name)
                elif name == "-inf at the action":
                    assert (lp[k] == NEG_INF).all() and np.isfinite(h[k]).all(), (s, name)
                else:
                    assert np.isfinite(lp[k]).all() and np.isfinite(h[k]).all(), (s, name)
                if name == "equal":
                    close(lp[k], np.full(len(k), -np.log(A[s]), np.float32), "uniform row")
                    close(h[k], np.full(len(k), np.log(A[s]), np.float32), "uniform row")
    ref.check(store, f"A={A}")
    store.guards_untouched(f"A={A}")
    oc.nothing_dropped(ref, f"A={A}")


# ---- 3. batch sizes, row capacities ------------------------------------------------------------------------------------------

def batch_size(bk, B, T=3):
    """One handle of B envs: the scan's lanes get (B + 63) // 64 envs each, the last ones fewer or none."""
    env = new_env(bk, "f32_3_7", B)
    store = GuardedLogpStore(env, T, (T * B * 16, T * B * 40), (9, 5))
    ref, _ = run(env, store, T, (9, 5), B, f"B={B}")
    oc.nothing_dropped(ref, f"B={B}")


def row_capacities(bk, B=2, T=2):
    """128 predator and 256 prey rows with more than 64 / 128 of them in use: the second and third trip of the `j += 64` loop."""
    g = image_cases.GEOMETRIES["i"]
    env = image_cases.new_handle(bk, g, B, seed=g.seed)
    env.reset()
    store = GuardedLogpStore(env, T, (T * B * 128, T * B * 256), (5, 7))
    seen = []
    ref, lref = run(env, store, T, (5, 7), 9, "128 / 256 rows",
                    every=lambda t, ref: seen.append(tables_of(env)["env_state"][:, [_abi.ENV_N_PRED_ROWS, _abi.ENV_N_PREY_ROWS]].max(axis=0)))
    assert max(x[0] for x in seen) > 64 and max(x[1] for x in seen) > 128, seen
    oc.nothing_dropped(ref, "128 / 256 rows")


# ---- 4. capacity, corrupted slots, a skipped species ---------------------------------------------------------------------------

def capacity_cut(bk, gid="bf16_3_5", B=5, T=4):
    """The stores of obs_store_cases.capacity_cut (they end inside a predator run at step 1 and inside a prey run at step 2): rows
    behind the cut have slot -1 and write nothing; nothing behind `capacity` elements is written."""
    counts = oc._row_counts(bk, gid, B, T, seed=21)
    cap_p = int(counts[0, :, 0].sum() + counts[1, :2, 0].sum() + counts[1, 2, 0] // 2)
    cap_q = int(counts[:2, :, 1].sum() + counts[2, :3, 1].sum() + counts[2, 3, 1] // 2)
    env = new_env(bk, gid, B)
    store = GuardedLogpStore(env, T, (cap_p, cap_q), (9, 32))
    ref, lref = run(env, store, T, (9, 32), 21, "capacity cut")
    (sp, dp), (sq, dq) = ref.counts()
    assert (sp, sq) == (cap_p, cap_q) and dp > 0 and dq > 0 and all(w.all() for w in lref.written)
    slot = store.slot.cpu().numpy()
    cp = env.pred_capacity
    for (t, b, s) in ((1, 2, 0), (2, 3, 1)):   # the cut fell inside the two runs
        run_slots = slot[t, b, (cp if s else 0):(cp if s else 0) + counts[t, b, s]]
        assert (run_slots >= 0).any() and (run_slots == -1).any(), (t, b, s, run_slots)


def capacity_zero(bk, gid="bf16_3_5", B=3, T=2):
    """capacity 0 for one species: its (empty) tensors are never addressed, the other species is written as usual."""
    for zero in (0, 1):
        rows = [T * B * 64, T * B * 128]
        rows[zero] = 0
        env = new_env(bk, gid, B)
        store = GuardedLogpStore(env, T, rows, (9, 9))
        _, lref = run(env, store, T, (9, 9), 3, f"capacity[{zero}] = 0")
        assert lref.written[1 - zero].any() and store.logp[zero].numel() == 0


def corrupted_slots(bk, gid="bf16_3_5", B=3, T=3):
    """slot[t] as a stale or foreign buffer would leave it: words of rows in use that are negative, >= capacity or exactly the
    capacity.  They are ignored, not followed -- those rows write nothing."""
    env = new_env(bk, gid, B)
    rows = (T * B * 20, T * B * 60)
    store = GuardedLogpStore(env, T, rows, (9, 9))
    junk = [2 ** 31 - 1, -(2 ** 31), -2, 0x5A5A5A5A, -(2 ** 31) + 1]

    def corrupt(t, ref):
        es = tables_of(env)["env_state"]
        cp = env.pred_capacity
        for b in range(B):
            for first, n, cap in ((0, int(es[b, _abi.ENV_N_PRED_ROWS]), rows[0]), (cp, int(es[b, _abi.ENV_N_PREY_ROWS]), rows[1])):
                for q, j in enumerate(range(0, n, 3)):
                    ref.slot[t, b, first + j] = cap if q == 0 else junk[(b + q) % len(junk)]
        store.slot.copy_(torch.from_numpy(ref.slot.copy()).to(env.device))
    _, lref = run(env, store, T, (9, 9), 13, "corrupted slots", every=corrupt)
    for s in (0, 1):
        n = int(store.cursor[s])
        assert lref.written[s].any() and not lref.written[s][:n].all(), "the corrupted rows were written, or nothing was"


def skipped_species(bk, gid="bf16_3_5", B=3, T=2):
    """One species' logits None: its tensors keep their NaN, the other species is written."""
    for skip in (0, 1):
        env = new_env(bk, gid, B)
        store = GuardedLogpStore(env, T, (T * B * 64, T * B * 128), (9, 9))

        def drop(logits):
            return [None if s == skip else x for s, x in enumerate(logits)]
        _, lref = run(env, store, T, (9, 9), 5, f"species {skip} skipped", logits_of=drop)
        assert bool(torch.isnan(store.logp[skip]).all()) and bool(torch.isnan(store.entropy[skip]).all())
        assert not lref.written[skip].any() and lref.written[1 - skip].any()
    # both skipped: the arguments are checked, nothing is launched
    before = store.snapshot()
    env.record_logp(store, 0, (None, None), random_actions(env, torch.Generator().manual_seed(1)))
    sync(env)
    for name, raw in store.snapshot().items():
        assert np.array_equal(raw, before[name]), name


# ---- 5. the step index on the device -------------------------------------------------------------------------------------------

def device_step_index(bk, gid="bf16_3_5", B=3, T=4):
    """The device word names the NEXT step: 0 writes nothing (t = -1); 1 .. T write steps 0 .. T - 1 -- the same bits as the host
    index on a twin, T being the last step; T + 1 and other words outside write nothing."""
    env, twin = new_env(bk, gid, B), new_env(bk, gid, B)
    rows, A = (T * B * 64, T * B * 128), (9, 9)
    a, b = GuardedLogpStore(env, T, rows, A), GuardedLogpStore(twin, T, rows, A)
    ref, lref = Ref(twin, b), LogpRef(twin, b)
    word = torch.zeros((1,), dtype=torch.int32, device=env.device)
    gen_a, gen_b, gen2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9), torch.Generator().manual_seed(10)

    def nothing(value):
        word.fill_(value)
        before = a.snapshot()
        logits, acts = synthetic(env, gen2, A)
        env.record_logp(a, word, logits, acts)
        sync(env)
        for name, raw in a.snapshot().items():
            assert np.array_equal(raw, before[name]), (value, name, "a call outside the horizon wrote")
    nothing(0)
    for t in range(T):
        acts_a, acts_b = random_actions(env, gen_a), random_actions(twin, gen_b)
        env.step(acts_a, auto_reset=True)
        twin.step(acts_b, auto_reset=True)
        word.fill_(t)
        env.record_obs(a, word, acts_a)
        twin.record_obs(b, t, acts_b)
        sync(twin)
        ref.record(twin, t, acts_b)
        word.add_(1)                                  # (what follows record() in a captured step)
        logits, acts = synthetic(env, gen2, A)
        env.record_logp(a, word, logits, acts)
        twin.record_logp(b, t, logits, acts)
        sync(env)
        lref.record(twin, t, logits, acts, ref.slot)
    assert int(word.item()) == T and lref.written[0].any() and lref.written[1].any()
    lref.check(a, "device word")
    for (name, x), y in zip({**a.tensors(), **policy_tensors(a)}.items(), {**b.tensors(), **policy_tensors(b)}.values()):
        assert np.array_equal(bits_of(x), bits_of(y)), (name, "device word and host index differ")
    last = ref.slot[T - 1][:, :env.pred_capacity]
    last = last[last >= 0]
    assert last.size and np.isfinite(a.logp[0].cpu().numpy()[last]).all()   # word = T wrote the last step
    for value in (T + 1, T + 7, -1, -(2 ** 31), 2 ** 31 - 1):
        nothing(value)
    a.guards_untouched("device word")


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------

def argument_checking(bk, other_device, gid="bf16_3_5", B=2, T=3):
    """Every PPG_EINVAL case of ppg_record_logp returns -1, names ppg_record_logp in ppg_last_error and writes nothing; the Python
    wrapper raises ValueError on a wrong dtype, shape, device, a short tensor, a bad step or a store without logp."""
    import pytest
    env = new_env(bk, gid, B)
    gen = torch.Generator().manual_seed(1)
    rows, A = (T * B * 64, T * B * 128), (9, 5)
    store = GuardedLogpStore(env, T, rows, A)
    ref = Ref(env, store)
    stepped(env, store, ref, 0, gen)
    logits, acts = synthetic(env, gen, A)
    word = torch.ones((1,), dtype=torch.int32, device=env.device)
    before = store.snapshot()

    def raw(st=True, out=True, horizon=T, step=0, flags=0, capacity=rows, null=(), n_actions=A, lg=(True, True), actions=True):
        s, o = _abi.PpgObsStore(), _abi.PpgLogpStore()
        s.horizon = horizon
        s.slot = None if "slot" in null else store.slot.data_ptr()
        for i in (0, 1):
            s.capacity[i], o.n_actions[i] = capacity[i], n_actions[i]
            o.logp[i] = None if f"logp{i}" in null else store.logp[i].data_ptr()
            o.entropy[i] = None if f"entropy{i}" in null else store.entropy[i].data_ptr()
            o.dist[i] = None if f"dist{i}" in null else store.dist[i].data_ptr()
        return env._lib.ppg_record_logp(env._handle, C.byref(s) if st else None, C.byref(o) if out else None, step, flags,
                                        logits[0].data_ptr() if lg[0] else None, logits[1].data_ptr() if lg[1] else None,
                                        acts.data_ptr() if actions else None, env._stream())
    refused = [dict(st=False), dict(out=False), dict(actions=False), dict(null=("slot",)), dict(null=("logp0",)), dict(null=("logp1",)),
               dict(null=("entropy0",)), dict(null=("entropy1",)), dict(null=("dist0",)), dict(null=("dist1",)),
               dict(n_actions=(0, 5)), dict(n_actions=(9, 33)), dict(n_actions=(-1, 5)), dict(n_actions=(9, 2 ** 31 - 1)),
               dict(horizon=0), dict(horizon=-3), dict(horizon=2 ** 31 - 1), dict(capacity=(-1, rows[1])), dict(capacity=(rows[0], -(2 ** 40))),
               dict(capacity=(2 ** 31, rows[1])), dict(step=T), dict(step=2 ** 63), dict(step=2 ** 64 - 1),
               dict(flags=STEP_ON_DEVICE, step=0), dict(flags=0x2), dict(flags=0x80000001, step=word.data_ptr())]
    for kw in refused:
        assert raw(**kw) == -1, kw
        assert b"ppg_record_logp" in env._lib.ppg_last_error(env._handle), kw
    sync(env)
    for name, now in store.snapshot().items():
        assert np.array_equal(now, before[name]), (name, "a refused call wrote")
    # (the accepted forms: optional pairs both NULL, a skipped species without logp and with any n_actions, the last step, the word)
    for kw in (dict(null=("entropy0", "entropy1")), dict(null=("dist0", "dist1")), dict(null=("logp0",), lg=(False, True), n_actions=(0, 5)),
               dict(lg=(False, False)), dict(step=T - 1), dict(flags=STEP_ON_DEVICE, step=word.data_ptr()), dict(capacity=(0, 0))):
        assert raw(**kw) == 0, kw
    sync(env)
    assert not bool(torch.isnan(store.logp[0]).all())

    def variant(**kw):
        v = types.SimpleNamespace(horizon=T, capacity=store.capacity, n_actions=A, slot=store.slot, logp=list(store.logp),
                                  entropy=list(store.entropy), dist=list(store.dist))
        for k, x in kw.items():
            if isinstance(getattr(v, k), list) and isinstance(x, torch.Tensor):
                getattr(v, k)[0] = x
            else:
                setattr(v, k, x)
        return v
    env.record_logp(variant(), 0, logits, acts)
    env.record_logp(variant(entropy=None, dist=None), 0, logits, acts)
    wrong = [dict(logp=store.logp[0].to(torch.float64)), dict(logp=store.logp[0][:5]), dict(logp=store.logp[0].to(other_device)),
             dict(logp=None), dict(entropy=store.entropy[0].to(torch.float16)), dict(entropy=store.entropy[0][:-1]),
             dict(dist=store.dist[0][:, :-1].contiguous()), dict(dist=store.dist[0].reshape(-1)), dict(dist=store.dist[0][:-1]),
             dict(slot=store.slot.to(torch.int64)), dict(slot=store.slot[:, :, :-1].contiguous()), dict(n_actions=(0, 5)),
             dict(n_actions=(9, 33)), dict(capacity=(-1, rows[1]))]
    for kw in wrong:
        with pytest.raises(ValueError):
            env.record_logp(variant(**kw), 0, logits, acts)
    for bad in ((logits[0].double(), logits[1]), (logits[0][:-1], logits[1]), (logits[0], logits[1][:, :-1].contiguous()),
                (logits[0].to(other_device), logits[1]), (logits[0],), (logits[0].t().contiguous().t(), logits[1])):
        with pytest.raises(ValueError):
            env.record_logp(store, 0, bad, acts)
    for t in (-1, T, word.to(torch.int64), word.to(other_device)):
        with pytest.raises(ValueError):
            env.record_logp(store, t, logits, acts)
    for bad in (acts.to(torch.int32), acts[:, :-1].contiguous(), acts.to(other_device)):
        with pytest.raises(ValueError):
            env.record_logp(store, 0, logits, bad)
    from predpreygrass_amd.trajectory import AgentTrajectories, ObservationStore
    with pytest.raises(ValueError):
        env.record_logp(ObservationStore(env, T, rows), 0, logits, acts)      # a store without logp
    with pytest.raises(ValueError):
        ObservationStore(env, T, rows, logp=(9, 33))
    with pytest.raises(ValueError):
        AgentTrajectories(env, T, logp=(9, 9))                               # logp without a store
    with pytest.raises(RuntimeError):
        AgentTrajectories(env, T, obs_rows=rows).record_policy(logits, acts)
    with pytest.raises(RuntimeError):
        AgentTrajectories(env, T, obs_rows=rows).behaviour(0)
    plain = ObservationStore(env, T, rows, logp=A, entropy=False)
    assert plain.entropy is None and plain.dist is None and bool(torch.isnan(plain.logp[1]).all())
    env.record_logp(plain, 0, logits)                                          # actions default to env.actions


# ---- 7. the torch restatement, scatter() -----------------------------------------------------------------------------------------

def torch_baseline(bk, A=(9, 32), B=5, T=3):
    """ObservationStore.record_logp_torch() against record_logp() on the same env: logp and entropy within the tolerance, dist bit for
    bit, NaN in the same slots -- over the special rows and actions of `values`."""
    from predpreygrass_amd.trajectory import ObservationStore
    env = new_env(bk, "f32_3_7", B)
    rows = (T * B * 16, T * B * 40)
    a, b = ObservationStore(env, T, rows, logp=A, dist=True), ObservationStore(env, T, rows, logp=A, dist=True)
    ref, lref = Ref(env, a), LogpRef(env, a)
    gen, gen2, rng = torch.Generator().manual_seed(41), torch.Generator().manual_seed(42), np.random.default_rng(43)
    for t in range(T):
        actions = random_actions(env, gen)
        env.step(actions, auto_reset=True)
        a.record(t, actions)
        b.record(t, actions)
        sync(env)
        ref.record(env, t, actions)
        logits, acts, _ = with_special_rows(env, lref, t, ref.slot, A, gen2, rng)
        a.record_logp(t, logits, acts)
        b.record_logp_torch(t, logits, acts)
        lref.record(env, t, logits, acts, ref.slot)
    sync(env)
    lref.check(a, "kernel")
    lref.check(b, "torch ops")
    for s in (0, 1):
        assert lref.written[s].any()
        assert np.array_equal(bits_of(a.dist[s]), bits_of(b.dist[s])), "dist"
        for x, y in ((a.logp[s], b.logp[s]), (a.entropy[s], b.entropy[s])):
            close(x.cpu().numpy(), y.cpu().numpy(), "kernel against torch ops")
    for name, x in oc.plain_tensors(a).items():
        assert np.array_equal(bits_of(x), bits_of(oc.plain_tensors(b)[name])), name


def scatter(env, T=8):
    """scatter() is the inverse of flat(): x where a row has a slot, `fill` elsewhere; through gae() it gives the bits of the original
    values when nothing was dropped."""
    import pytest
    from predpreygrass_amd.trajectory import AgentTrajectories
    B, S = env.batch_size, env.S
    env.reset()
    traj = AgentTrajectories(env, T, obs_rows=(T * B * 32, T * B * 96))
    gen = torch.Generator().manual_seed(17)
    for t in range(T):
        actions = random_actions(env, gen)
        env.step(actions, auto_reset=True)
        traj.record(actions)
    sync(env)
    (sp, dp), (sq, dq) = traj.store.counts()
    assert dp == dq == 0 and sp > 0 and sq > 0
    x = torch.rand((T, B, S), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(env.device)
    for fill in (0.0, -7.5):
        back = traj.scatter(traj.flat(x, 0), traj.flat(x, 1), fill=fill)
        want = torch.where(traj.store.slot >= 0, x, torch.full_like(x, fill))
        assert back.shape == x.shape and back.dtype == x.dtype and torch.equal(back, want)
    assert bool((traj.store.slot >= 0).eq(traj.in_use).all())
    values = traj.scatter(traj.flat(x, 0), traj.flat(x, 1))
    assert torch.equal(traj.gae(values, 0.99, 0.95).view(torch.int64), traj.gae(x, 0.99, 0.95).view(torch.int64))
    only_prey = traj.scatter(None, traj.flat(x, 1), fill=1.0)
    cp = env.pred_capacity
    assert bool((only_prey[:, :, :cp] == 1.0).all()) and torch.equal(only_prey[:, :, cp:], torch.where(traj.store.slot[:, :, cp:] >= 0, x[:, :, cp:], torch.ones_like(x[:, :, cp:])))
    with pytest.raises(ValueError):
        traj.scatter(traj.flat(x, 0)[:-1], traj.flat(x, 1))
    with pytest.raises(ValueError):
        traj.scatter(None, None)
    with pytest.raises(RuntimeError):
        AgentTrajectories(env, T).scatter(traj.flat(x, 0), traj.flat(x, 1))
