"""`stream=` of step() / link() / record() / backward() and of FusedPolicy.act(want_logits=True) on the MI355X: the same sequence on
torch's current stream and on a side stream -- given as a torch.cuda.Stream, or as its raw handle -- writes the same bytes, and the
env's two link tensors are allocated once.  Also the device condition of the tensor-argument check (tests/test_tensor_args.py has
the others): a CPU tensor handed to a GPU env is refused in Python."""
import contextlib

import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from tests import record_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T = 3, 4
WARM = 60   # steps before the sequence: the default config pays its first reward (a birth) some twenty steps after a reset
GAMMA, LAM = 0.97, 0.9
FORMS = {"torch.cuda.Stream": lambda s: s, "raw handle": lambda s: s.cuda_stream}


def make():
    env = BatchedPredPreyGrass(None, batch_size=B, device=DEV, prey_capacity=128, seed=7)
    assert env.S == 192
    env.reset()
    for _ in range(WARM):
        env.step(random_actions=True, auto_reset=True)
    return env


def sequence(env, values, side=None, form=None):
    """step + link(), then T times step + record(t), then backward(): everything the calls return, cloned in stream order.  side: the
    stream the launches go to (None: torch's current stream, no `stream` argument), form: how it is handed over."""
    kw = {} if side is None else {"stream": FORMS[form](side)}
    on = contextlib.nullcontext() if side is None else torch.cuda.stream(side)   # (only the test's own clones run under it)
    d = cases.fresh(env, T)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())   # the reset, the fills of `d` and of `values` come first
    out, ptrs = {}, []
    env.step(random_actions=True, auto_reset=True, **kw)
    p, n = env.link(**kw)
    ptrs.append((p.data_ptr(), n.data_ptr()))
    with on:
        out["link"] = (p.clone(), n.clone())
    for t in range(T):
        env.step(random_actions=True, auto_reset=True, **kw)
        p, n = env.record(*cases.args(d), t, **kw)
        ptrs.append((p.data_ptr(), n.data_ptr()))
        with on:
            out[f"record {t}"] = (p.clone(), n.clone())
    out["G"], out["A"] = env.backward(d["reward"], d["next_row"], d["in_use"], d["terminated"], d["truncated"], GAMMA, LAM, values=values, **kw)
    out["trajectory"] = cases.args(d)
    return out, ptrs


@pytest.mark.parametrize("form", list(FORMS))
def test_a_side_stream_gives_what_the_current_stream_gives(form):
    a, b = make(), make()
    values = torch.randn((T, B, a.S), generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    want, _ = sequence(a, values)
    got, ptrs = sequence(b, values, side, form)
    torch.cuda.synchronize()
    assert list(got) == list(want)
    for k in want:
        w, g = (x if isinstance(x, tuple) else (x,) for x in (want[k], got[k]))
        for i, (x, y) in enumerate(zip(w, g)):
            assert x.dtype == y.dtype and torch.equal(x, y), (k, i)
    assert len(set(ptrs)) == 1 and ptrs[0] == tuple(x.data_ptr() for x in b._link_rows), "the link tensors are the env's own two"
    assert torch.equal(a.env_state, b.env_state) and torch.equal(a.obs_prey, b.obs_prey)
    # (the run must not pass vacuously)
    assert bool((got["record 3"][1] >= 0).any()) and bool(got["trajectory"][1].any()) and bool((got["G"] != 0).any()) and bool((got["A"] != 0).any())


@pytest.mark.parametrize("form", list(FORMS))
def test_policy_logits_on_a_side_stream(form):
    from predpreygrass_amd.policy import FusedPolicy
    from tests.test_policy import make_nets
    fused = FusedPolicy(*make_nets())
    a, b = make(), make()
    side = torch.cuda.Stream(device=DEV)
    want = fused.act(a, want_logits=True)
    side.wait_stream(torch.cuda.current_stream())
    got = fused.act(b, want_logits=True, stream=FORMS[form](side))
    torch.cuda.synchronize()
    for t in range(2):
        assert got[t].shape == want[t].shape and torch.equal(got[t], want[t]), t
        assert bool((got[t] != 0).any())
    assert torch.equal(a.actions, b.actions) and bool((b.actions != _abi.ACTION_NONE).any())


@pytest.mark.parametrize("form", list(FORMS))
def test_a_cpu_tensor_is_refused_by_a_gpu_env(form):
    env = make()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    before = env.env_state.clone()
    with pytest.raises(ValueError, match="actions"):
        env.step(actions=torch.zeros((B, env.S), dtype=torch.int8), stream=FORMS[form](side))
    torch.cuda.synchronize()
    assert torch.equal(env.env_state, before), "the refused call launched something"
