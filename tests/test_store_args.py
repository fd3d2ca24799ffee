"""Every refusal of the three calls that take a sample store -- `record_obs()`, `record_logp()`, `backward_samples()` of
`BatchedPredPreyGrass` -- with its exception type and its COMPLETE message, through the kernel source compiled for the CPU wave
emulator: one entry of WANT per single mistake, nothing launched and nothing written after any of them; the forms that are accepted;
and `live_mask()`.

The literals of WANT were produced by running CASES against the package as it was BEFORE the three calls got their common argument
builder (`_store_args` / `_rows_arg`), and this file passes against that package too: copied into a checkout of that commit,
everything passes except the two tests marked "new" below -- the order in which TWO mistakes are reported, which the builder states
once and which is the one thing that differs, and `live_mask()`, which that package does not have.  That is how the pins are checked."""
import types

import numpy as np
import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.trajectory import ObservationStore
from tests import link_cases
from tests.emu_backend import library

B, T, S = 2, 3, 192
CAP, A = (20, 40), (9, 9)
F32, I32, I8 = torch.float32, torch.int32, torch.int8


def make_env(dtype=F32, batch=B, cfg=None):
    return BatchedPredPreyGrass(cfg, batch_size=batch, obs_dtype=dtype, prey_capacity=128, seed=3, _library=library())


@pytest.fixture(scope="module")
def world():
    """The env (float32 rows) after reset, its bfloat16 twin, the store of capacity (20, 40) with logp and dist, the empty store."""
    env, env_bf16 = make_env().reset(), make_env(torch.bfloat16).reset()
    assert env.S == S
    return types.SimpleNamespace(env=env, env_bf16=env_bf16, store=ObservationStore(env, T, CAP, logp=A, dist=True),
                                 empty=ObservationStore(env, T, (0, 0), logp=A, dist=True))


STORE_LISTS = ("obs", "sample", "action", "logp", "entropy", "dist")
STORE_FIELDS = ("horizon", "capacity", "n_actions", "slot", "cursor") + STORE_LISTS


def view_of(store):
    """The store as a plain object a case may change: the same tensors, its own lists."""
    return types.SimpleNamespace(**{k: list(getattr(store, k)) if k in STORE_LISTS or k in ("capacity", "n_actions") else getattr(store, k)
                                    for k in STORE_FIELDS})


def tensors_of(store):
    return [store.slot, store.cursor] + [x for k in STORE_LISTS for x in getattr(store, k)]


def call_args(call, env):
    """The keyword arguments of a correct call."""
    if call == "record_obs":
        return dict(t=0, actions=torch.zeros((B, S), dtype=I8), f32=False)
    if call == "record_logp":
        return dict(t=0, logits=[torch.zeros((B * c, a), dtype=F32) for c, a in zip((env.pred_capacity, env.prey_capacity), A)],
                    actions=torch.zeros((B, S), dtype=I8))
    z = lambda dtype, fill=0: torch.full((T, B, S), fill, dtype=dtype)
    return dict(reward=z(torch.float64), next_row=z(torch.int16, -1), in_use=z(torch.bool), terminated=z(torch.bool),
                truncated=z(torch.bool), gamma=0.99, lam=0.95, values=[torch.zeros((c,), dtype=F32) for c in CAP])


def bad(x, how):
    """x wrong in one respect: its dtype, its trailing shape (one more dimension for a vector), its first dimension, its strides."""
    if how == "dtype":   # (one the argument does not take: uint8 stands in for bool, so not that)
        other = {torch.float32: torch.float64, torch.float64: torch.float32, torch.bool: torch.int16, torch.int64: I32}
        return x.to(other.get(x.dtype, torch.int64))
    if how == "shape":
        return x[..., :-1].contiguous() if x.dim() > 1 else x[:, None].contiguous()
    if how == "rows":
        return x[:-1].contiguous()
    y = x.repeat_interleave(2, dim=0)[::2]
    assert how == "strides" and tuple(y.shape) == tuple(x.shape) and not y.is_contiguous()
    return y


def set_item(field, s, how):
    def change(st, kw):
        getattr(st, field)[s] = bad(getattr(st, field)[s], how)
    return change


def set_attr(field, how):
    def change(st, kw):
        setattr(st, field, bad(getattr(st, field), how))
    return change


def set_kw(name, s, how):
    def change(st, kw):
        if s is None:
            kw[name] = bad(kw[name], how)
        else:
            kw[name][s] = bad(kw[name][s], how)
    return change


def assign(target, name, value, s=None):
    def change(st, kw):
        box = st.__dict__ if target == "store" else kw
        if s is None:
            box[name] = value
        else:
            box[name][s] = value
    return change


ROWS, FIXED = ("dtype", "shape", "rows", "strides"), ("dtype", "shape", "strides")
T_CASES = {"t = -1": assign("kw", "t", -1), f"t = {T}": assign("kw", "t", T), "t int64 tensor": assign("kw", "t", torch.zeros((1,), dtype=torch.int64))}
CAP_CASES = {f"capacity[{s}] = -1": assign("store", "capacity", -1, s) for s in (0, 1)}
# call -> {id: change(store view, keyword arguments)}; "bf16" in an id: the call goes to the bfloat16 env
CASES = {
    "record_obs": {
        **{f"store.slot {h}": set_attr("slot", h) for h in FIXED},
        **{f"store.{f}[{s}] {h}": set_item(f, s, h) for f in ("obs", "sample", "action") for s in (0, 1) for h in ROWS},
        **{f"store.cursor {h}": set_attr("cursor", h) for h in FIXED},
        **{f"actions {h}": set_kw("actions", None, h) for h in FIXED},
        **CAP_CASES, **T_CASES,
        "actions for a store that keeps none": assign("store", "action", None),
        "f32=True on a bf16 env": assign("kw", "f32", True),
    },
    "record_logp": {
        **{f"store.slot {h}": set_attr("slot", h) for h in FIXED},
        **{f"store.{f}[{s}] {h}": set_item(f, s, h) for f in ("logp", "entropy", "dist") for s in (0, 1) for h in ROWS},
        **{f"logits[{s}] {h}": set_kw("logits", s, h) for s in (0, 1) for h in ROWS},
        **{f"actions {h}": set_kw("actions", None, h) for h in FIXED},
        **CAP_CASES, **T_CASES,
        "n_actions[0] = 0": assign("store", "n_actions", 0, 0), "n_actions[1] = 33": assign("store", "n_actions", 33, 1),
        "a store without logp": assign("store", "logp", None),
        "logits not a pair": assign("kw", "logits", [None]),
    },
    "backward_samples": {
        **{f"store.slot {h}": set_attr("slot", h) for h in FIXED},
        **{f"values[{s}] {h}": set_kw("values", s, h) for s in (0, 1) for h in ("shape", "rows", "strides")},
        **{f"values[{s}] dtype": assign("kw", "values", torch.zeros((CAP[s],), dtype=torch.float16), s) for s in (0, 1)},
        **{f"{n} {h}": set_kw(n, None, h) for n in ("reward", "next_row", "in_use", "terminated", "truncated") for h in FIXED},
        **CAP_CASES,
        "values not a pair": assign("kw", "values", [None, None, None]),
        "values of two dtypes": assign("kw", "values", torch.zeros((CAP[1],), dtype=torch.float64), 1),
        "more steps than the horizon": assign("store", "horizon", T - 1),
        "neither returns nor advantages": lambda st, kw: kw.update(returns=False, advantages=False),
        "stats without advantages": lambda st, kw: kw.update(stats=True, advantages=False),
    },
}
V = ValueError
WANT = {
    'record_obs: store.slot dtype': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int64 tensor [3, 2, 192] on cpu'),
    'record_obs: store.slot shape': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int32 tensor [3, 2, 191] on cpu'),
    'record_obs: store.slot strides': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a non-contiguous torch.int32 tensor [3, 2, 192] on cpu'),
    'record_obs: store.obs[0] dtype': (V, 'store.obs[0] must be a contiguous torch.float32 tensor [*,4,7,7] on cpu, not a torch.float64 tensor [20, 4, 7, 7] on cpu'),
    'record_obs: store.obs[0] shape': (V, 'store.obs[0] must be a contiguous torch.float32 tensor [*,4,7,7] on cpu, not a torch.float32 tensor [20, 4, 7, 6] on cpu'),
    'record_obs: store.obs[0] rows': (V, 'store.obs[0] has 19 rows, fewer than the capacity 20'),
    'record_obs: store.obs[0] strides': (V, 'store.obs[0] must be a contiguous torch.float32 tensor [*,4,7,7] on cpu, not a non-contiguous torch.float32 tensor [20, 4, 7, 7] on cpu'),
    'record_obs: store.obs[1] dtype': (V, 'store.obs[1] must be a contiguous torch.float32 tensor [*,4,9,9] on cpu, not a torch.float64 tensor [40, 4, 9, 9] on cpu'),
    'record_obs: store.obs[1] shape': (V, 'store.obs[1] must be a contiguous torch.float32 tensor [*,4,9,9] on cpu, not a torch.float32 tensor [40, 4, 9, 8] on cpu'),
    'record_obs: store.obs[1] rows': (V, 'store.obs[1] has 39 rows, fewer than the capacity 40'),
    'record_obs: store.obs[1] strides': (V, 'store.obs[1] must be a contiguous torch.float32 tensor [*,4,9,9] on cpu, not a non-contiguous torch.float32 tensor [40, 4, 9, 9] on cpu'),
    'record_obs: store.sample[0] dtype': (V, 'store.sample[0] must be a contiguous torch.int32 tensor [*] on cpu, not a torch.int64 tensor [20] on cpu'),
    'record_obs: store.sample[0] shape': (V, 'store.sample[0] must be a contiguous torch.int32 tensor [*] on cpu, not a torch.int32 tensor [20, 1] on cpu'),
    'record_obs: store.sample[0] rows': (V, 'store.sample[0] has 19 rows, fewer than the capacity 20'),
    'record_obs: store.sample[0] strides': (V, 'store.sample[0] must be a contiguous torch.int32 tensor [*] on cpu, not a non-contiguous torch.int32 tensor [20] on cpu'),
    'record_obs: store.sample[1] dtype': (V, 'store.sample[1] must be a contiguous torch.int32 tensor [*] on cpu, not a torch.int64 tensor [40] on cpu'),
    'record_obs: store.sample[1] shape': (V, 'store.sample[1] must be a contiguous torch.int32 tensor [*] on cpu, not a torch.int32 tensor [40, 1] on cpu'),
    'record_obs: store.sample[1] rows': (V, 'store.sample[1] has 39 rows, fewer than the capacity 40'),
    'record_obs: store.sample[1] strides': (V, 'store.sample[1] must be a contiguous torch.int32 tensor [*] on cpu, not a non-contiguous torch.int32 tensor [40] on cpu'),
    'record_obs: store.action[0] dtype': (V, 'store.action[0] must be a contiguous torch.int8 tensor [*] on cpu, not a torch.int64 tensor [20] on cpu'),
    'record_obs: store.action[0] shape': (V, 'store.action[0] must be a contiguous torch.int8 tensor [*] on cpu, not a torch.int8 tensor [20, 1] on cpu'),
    'record_obs: store.action[0] rows': (V, 'store.action[0] has 19 rows, fewer than the capacity 20'),
    'record_obs: store.action[0] strides': (V, 'store.action[0] must be a contiguous torch.int8 tensor [*] on cpu, not a non-contiguous torch.int8 tensor [20] on cpu'),
    'record_obs: store.action[1] dtype': (V, 'store.action[1] must be a contiguous torch.int8 tensor [*] on cpu, not a torch.int64 tensor [40] on cpu'),
    'record_obs: store.action[1] shape': (V, 'store.action[1] must be a contiguous torch.int8 tensor [*] on cpu, not a torch.int8 tensor [40, 1] on cpu'),
    'record_obs: store.action[1] rows': (V, 'store.action[1] has 39 rows, fewer than the capacity 40'),
    'record_obs: store.action[1] strides': (V, 'store.action[1] must be a contiguous torch.int8 tensor [*] on cpu, not a non-contiguous torch.int8 tensor [40] on cpu'),
    'record_obs: store.cursor dtype': (V, 'store.cursor must be a contiguous torch.int64 tensor [4] on cpu, not a torch.int32 tensor [4] on cpu'),
    'record_obs: store.cursor shape': (V, 'store.cursor must be a contiguous torch.int64 tensor [4] on cpu, not a torch.int64 tensor [4, 1] on cpu'),
    'record_obs: store.cursor strides': (V, 'store.cursor must be a contiguous torch.int64 tensor [4] on cpu, not a non-contiguous torch.int64 tensor [4] on cpu'),
    'record_obs: actions dtype': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a torch.int64 tensor [2, 192] on cpu'),
    'record_obs: actions shape': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a torch.int8 tensor [2, 191] on cpu'),
    'record_obs: actions strides': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a non-contiguous torch.int8 tensor [2, 192] on cpu'),
    'record_obs: capacity[0] = -1': (V, 'store.capacity[0] = -1 < 0'),
    'record_obs: capacity[1] = -1': (V, 'store.capacity[1] = -1 < 0'),
    'record_obs: t = -1': (V, 't = -1 is outside [0, 3)'),
    'record_obs: t = 3': (V, 't = 3 is outside [0, 3)'),
    'record_obs: t int64 tensor': (V, 't must be an int or a one-element int32 tensor on cpu'),
    'record_obs: actions for a store that keeps none': (V, 'actions were given but the store keeps none'),
    'record_obs: f32=True on a bf16 env': (V, 'f32=True is for float64 (and float32) observations, not bfloat16'),
    'record_logp: store.slot dtype': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int64 tensor [3, 2, 192] on cpu'),
    'record_logp: store.slot shape': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int32 tensor [3, 2, 191] on cpu'),
    'record_logp: store.slot strides': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a non-contiguous torch.int32 tensor [3, 2, 192] on cpu'),
    'record_logp: store.logp[0] dtype': (V, 'store.logp[0] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float64 tensor [20] on cpu'),
    'record_logp: store.logp[0] shape': (V, 'store.logp[0] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float32 tensor [20, 1] on cpu'),
    'record_logp: store.logp[0] rows': (V, 'store.logp[0] has 19 rows, fewer than the capacity 20'),
    'record_logp: store.logp[0] strides': (V, 'store.logp[0] must be a contiguous torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [20] on cpu'),
    'record_logp: store.logp[1] dtype': (V, 'store.logp[1] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float64 tensor [40] on cpu'),
    'record_logp: store.logp[1] shape': (V, 'store.logp[1] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float32 tensor [40, 1] on cpu'),
    'record_logp: store.logp[1] rows': (V, 'store.logp[1] has 39 rows, fewer than the capacity 40'),
    'record_logp: store.logp[1] strides': (V, 'store.logp[1] must be a contiguous torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [40] on cpu'),
    'record_logp: store.entropy[0] dtype': (V, 'store.entropy[0] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float64 tensor [20] on cpu'),
    'record_logp: store.entropy[0] shape': (V, 'store.entropy[0] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float32 tensor [20, 1] on cpu'),
    'record_logp: store.entropy[0] rows': (V, 'store.entropy[0] has 19 rows, fewer than the capacity 20'),
    'record_logp: store.entropy[0] strides': (V, 'store.entropy[0] must be a contiguous torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [20] on cpu'),
    'record_logp: store.entropy[1] dtype': (V, 'store.entropy[1] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float64 tensor [40] on cpu'),
    'record_logp: store.entropy[1] shape': (V, 'store.entropy[1] must be a contiguous torch.float32 tensor [*] on cpu, not a torch.float32 tensor [40, 1] on cpu'),
    'record_logp: store.entropy[1] rows': (V, 'store.entropy[1] has 39 rows, fewer than the capacity 40'),
    'record_logp: store.entropy[1] strides': (V, 'store.entropy[1] must be a contiguous torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [40] on cpu'),
    'record_logp: store.dist[0] dtype': (V, 'store.dist[0] must be a contiguous torch.float32 tensor [*,9] on cpu, not a torch.float64 tensor [20, 9] on cpu'),
    'record_logp: store.dist[0] shape': (V, 'store.dist[0] must be a contiguous torch.float32 tensor [*,9] on cpu, not a torch.float32 tensor [20, 8] on cpu'),
    'record_logp: store.dist[0] rows': (V, 'store.dist[0] has 19 rows, fewer than the capacity 20'),
    'record_logp: store.dist[0] strides': (V, 'store.dist[0] must be a contiguous torch.float32 tensor [*,9] on cpu, not a non-contiguous torch.float32 tensor [20, 9] on cpu'),
    'record_logp: store.dist[1] dtype': (V, 'store.dist[1] must be a contiguous torch.float32 tensor [*,9] on cpu, not a torch.float64 tensor [40, 9] on cpu'),
    'record_logp: store.dist[1] shape': (V, 'store.dist[1] must be a contiguous torch.float32 tensor [*,9] on cpu, not a torch.float32 tensor [40, 8] on cpu'),
    'record_logp: store.dist[1] rows': (V, 'store.dist[1] has 39 rows, fewer than the capacity 40'),
    'record_logp: store.dist[1] strides': (V, 'store.dist[1] must be a contiguous torch.float32 tensor [*,9] on cpu, not a non-contiguous torch.float32 tensor [40, 9] on cpu'),
    'record_logp: logits[0] dtype': (V, 'logits[0] must be a contiguous torch.float32 tensor [128,9] on cpu, not a torch.float64 tensor [128, 9] on cpu'),
    'record_logp: logits[0] shape': (V, 'logits[0] must be a contiguous torch.float32 tensor [128,9] on cpu, not a torch.float32 tensor [128, 8] on cpu'),
    'record_logp: logits[0] rows': (V, 'logits[0] must be a contiguous torch.float32 tensor [128,9] on cpu, not a torch.float32 tensor [127, 9] on cpu'),
    'record_logp: logits[0] strides': (V, 'logits[0] must be a contiguous torch.float32 tensor [128,9] on cpu, not a non-contiguous torch.float32 tensor [128, 9] on cpu'),
    'record_logp: logits[1] dtype': (V, 'logits[1] must be a contiguous torch.float32 tensor [256,9] on cpu, not a torch.float64 tensor [256, 9] on cpu'),
    'record_logp: logits[1] shape': (V, 'logits[1] must be a contiguous torch.float32 tensor [256,9] on cpu, not a torch.float32 tensor [256, 8] on cpu'),
    'record_logp: logits[1] rows': (V, 'logits[1] must be a contiguous torch.float32 tensor [256,9] on cpu, not a torch.float32 tensor [255, 9] on cpu'),
    'record_logp: logits[1] strides': (V, 'logits[1] must be a contiguous torch.float32 tensor [256,9] on cpu, not a non-contiguous torch.float32 tensor [256, 9] on cpu'),
    'record_logp: actions dtype': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a torch.int64 tensor [2, 192] on cpu'),
    'record_logp: actions shape': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a torch.int8 tensor [2, 191] on cpu'),
    'record_logp: actions strides': (V, 'actions must be a contiguous torch.int8 tensor [2,192] on cpu, not a non-contiguous torch.int8 tensor [2, 192] on cpu'),
    'record_logp: capacity[0] = -1': (V, 'store.capacity[0] = -1 < 0'),
    'record_logp: capacity[1] = -1': (V, 'store.capacity[1] = -1 < 0'),
    'record_logp: t = -1': (V, 't = -1 is outside [0, 3)'),
    'record_logp: t = 3': (V, 't = 3 is outside [0, 3)'),
    'record_logp: t int64 tensor': (V, 't must be an int or a one-element int32 tensor on cpu'),
    'record_logp: n_actions[0] = 0': (V, 'store.n_actions[0] = 0 is outside 1..32'),
    'record_logp: n_actions[1] = 33': (V, 'store.n_actions[1] = 33 is outside 1..32'),
    'record_logp: a store without logp': (V, 'the store keeps no log-probabilities: ObservationStore(..., logp=(A_pred, A_prey))'),
    'record_logp: logits not a pair': (V, 'logits must be the pair (logits_pred, logits_prey); either may be None'),
    'backward_samples: store.slot dtype': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int64 tensor [3, 2, 192] on cpu'),
    'backward_samples: store.slot shape': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a torch.int32 tensor [3, 2, 191] on cpu'),
    'backward_samples: store.slot strides': (V, 'store.slot must be a contiguous torch.int32 tensor [3,2,192] on cpu, not a non-contiguous torch.int32 tensor [3, 2, 192] on cpu'),
    'backward_samples: values[0] shape': (V, 'values[0] must be a contiguous torch.float64 / torch.float32 tensor [*] on cpu, not a torch.float32 tensor [20, 1] on cpu'),
    'backward_samples: values[0] rows': (V, 'values[0] has 19 elements, fewer than the capacity 20'),
    'backward_samples: values[0] strides': (V, 'values[0] must be a contiguous torch.float64 / torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [20] on cpu'),
    'backward_samples: values[1] shape': (V, 'values[1] must be a contiguous torch.float64 / torch.float32 tensor [*] on cpu, not a torch.float32 tensor [40, 1] on cpu'),
    'backward_samples: values[1] rows': (V, 'values[1] has 39 elements, fewer than the capacity 40'),
    'backward_samples: values[1] strides': (V, 'values[1] must be a contiguous torch.float64 / torch.float32 tensor [*] on cpu, not a non-contiguous torch.float32 tensor [40] on cpu'),
    'backward_samples: values[0] dtype': (V, 'values of the two species must have one dtype'),
    'backward_samples: values[1] dtype': (V, 'values of the two species must have one dtype'),
    'backward_samples: reward dtype': (V, 'reward must be a contiguous torch.float64 tensor [3,2,192] on cpu, not a torch.float32 tensor [3, 2, 192] on cpu'),
    'backward_samples: reward shape': (V, 'reward must be [T,2,192] with T >= 1, not (3, 2, 191)'),
    'backward_samples: reward strides': (V, 'reward must be a contiguous torch.float64 tensor [3,2,192] on cpu, not a non-contiguous torch.float64 tensor [3, 2, 192] on cpu'),
    'backward_samples: next_row dtype': (V, 'next_row must be a contiguous torch.int16 tensor [3,2,192] on cpu, not a torch.int64 tensor [3, 2, 192] on cpu'),
    'backward_samples: next_row shape': (V, 'next_row must be a contiguous torch.int16 tensor [3,2,192] on cpu, not a torch.int16 tensor [3, 2, 191] on cpu'),
    'backward_samples: next_row strides': (V, 'next_row must be a contiguous torch.int16 tensor [3,2,192] on cpu, not a non-contiguous torch.int16 tensor [3, 2, 192] on cpu'),
    'backward_samples: in_use dtype': (V, 'in_use must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.int16 tensor [3, 2, 192] on cpu'),
    'backward_samples: in_use shape': (V, 'in_use must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.bool tensor [3, 2, 191] on cpu'),
    'backward_samples: in_use strides': (V, 'in_use must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a non-contiguous torch.bool tensor [3, 2, 192] on cpu'),
    'backward_samples: terminated dtype': (V, 'terminated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.int16 tensor [3, 2, 192] on cpu'),
    'backward_samples: terminated shape': (V, 'terminated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.bool tensor [3, 2, 191] on cpu'),
    'backward_samples: terminated strides': (V, 'terminated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a non-contiguous torch.bool tensor [3, 2, 192] on cpu'),
    'backward_samples: truncated dtype': (V, 'truncated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.int16 tensor [3, 2, 192] on cpu'),
    'backward_samples: truncated shape': (V, 'truncated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a torch.bool tensor [3, 2, 191] on cpu'),
    'backward_samples: truncated strides': (V, 'truncated must be a contiguous torch.bool / torch.uint8 tensor [3,2,192] on cpu, not a non-contiguous torch.bool tensor [3, 2, 192] on cpu'),
    'backward_samples: capacity[0] = -1': (V, 'store.capacity[0] = -1 < 0'),
    'backward_samples: capacity[1] = -1': (V, 'store.capacity[1] = -1 < 0'),
    'backward_samples: values not a pair': (V, 'values must be the pair (v_pred, v_prey); either may be None'),
    'backward_samples: values of two dtypes': (V, 'values of the two species must have one dtype'),
    'backward_samples: more steps than the horizon': (V, "3 steps, but the store's horizon is 2"),
    'backward_samples: neither returns nor advantages': (V, 'backward_samples: neither returns nor advantages asked for'),
    'backward_samples: stats without advantages': (V, 'backward_samples: stats need advantages'),
}


def run(world, call, case):
    env = world.env_bf16 if "bf16" in case else world.env
    st, kw = view_of(world.store), call_args(call, env)
    CASES[call][case](st, kw)
    return getattr(env, call)(st, **kw)


ALL = [(call, case) for call in CASES for case in CASES[call]]


def test_the_table_names_every_case_once():
    assert sorted(WANT) == sorted(f"{call}: {case}" for call, case in ALL)


@pytest.mark.parametrize("call,case", ALL, ids=[f"{call}: {case}" for call, case in ALL])
def test_a_single_mistake_is_refused_with_this_message_and_nothing_is_written(world, call, case):
    before = [x.clone() for x in tensors_of(world.store)]
    kind, message = WANT[f"{call}: {case}"]
    with pytest.raises(kind) as err:
        run(world, call, case)
    assert type(err.value) is kind and str(err.value) == message
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(tensors_of(world.store), before))


def test_accepted_forms(world):
    """Capacity 0 with empty tensors (which have no address), either logits None, either values None."""
    env = world.env
    env.record_obs(world.empty, 0, torch.zeros((B, S), dtype=I8))
    kw = call_args("record_logp", env)
    env.record_logp(world.empty, 0, kw["logits"], kw["actions"])
    assert world.empty.cursor.tolist()[:2] == [0, 0] and sum(world.empty.cursor.tolist()[2:]) > 0   # (every row in use was dropped)
    kw = call_args("backward_samples", env)
    kw["values"] = [torch.zeros((0,), dtype=F32)] * 2
    adv, ret, stats = env.backward_samples(world.empty, **kw, stats=True)
    assert [tuple(x.shape) for x in adv + ret] == [(0,)] * 4 and tuple(stats.shape) == (B, 2, 3)
    env.record_obs(world.store, 0, None)
    for pair in ([None, 1], [0, None], [None, None]):
        kw = call_args("record_logp", env)
        env.record_logp(world.store, 0, [None if s is None else kw["logits"][s] for s in pair])
        kw = call_args("backward_samples", env)
        adv, ret, stats = env.backward_samples(world.store, **{**kw, "values": [None if s is None else kw["values"][s] for s in pair]})
        assert [tuple(x.shape) for x in adv + ret] == [(n,) for n in CAP + CAP] and stats is None
    world.store.clear()
    world.empty.clear()


# new: the ONE order the common builder checks in (BatchedPredPreyGrass._store_args) -- store.slot, the capacities, the per-species
# tensors, store.cursor, logits / values, the step, actions.  (call, two cases of CASES, the one that is reported)
TWO_MISTAKES = [
    ("record_obs", "store.cursor dtype", "store.slot dtype", "store.slot dtype"),
    ("record_obs", "store.obs[0] dtype", "capacity[1] = -1", "capacity[1] = -1"),
    ("record_obs", "store.cursor shape", "store.action[1] rows", "store.action[1] rows"),
    ("record_obs", "actions dtype", "t = -1", "t = -1"),
    ("record_logp", "store.logp[0] strides", "capacity[1] = -1", "capacity[1] = -1"),
    ("record_logp", "logits[0] dtype", "store.dist[0] shape", "store.dist[0] shape"),
    ("backward_samples", "values[0] rows", "capacity[1] = -1", "capacity[1] = -1"),
    ("backward_samples", "capacity[0] = -1", "store.slot strides", "store.slot strides"),
]


@pytest.mark.parametrize("call,first,second,reported", TWO_MISTAKES)
def test_new_two_mistakes_are_reported_in_the_builders_order(world, call, first, second, reported):
    st, kw = view_of(world.store), call_args(call, world.env)
    CASES[call][first](st, kw)
    CASES[call][second](st, kw)
    kind, message = WANT[f"{call}: {reported}"]
    with pytest.raises(kind) as err:
        getattr(world.env, call)(st, **kw)
    assert str(err.value) == message


def test_new_live_mask_is_step_batchs_mask_and_the_row_counts(world):
    env = make_env(batch=3, cfg=link_cases.CFG_BASE).reset()
    births = deaths = 0
    for _ in range(12):
        out = env.step_batch(random_actions=True, auto_reset=True)
        live = env.live_mask()
        assert live.dtype == torch.bool and tuple(live.shape) == (3, env.S) and torch.equal(live, out[5])
        tables = env.host_tables()
        for b in range(3):
            used = link_cases.in_use_mask(tables, b, env.pred_capacity, env.S)
            assert np.array_equal(live[b].numpy(), used), b
            births += int(((tables["row_flags"][b] & _abi.ROW_NEWBORN) != 0)[used].sum())
            deaths += int(((tables["row_flags"][b] & _abi.ROW_DIED) != 0)[used].sum())
    assert births > 0 and deaths > 0, (births, deaths)   # (the row counts moved both ways)
