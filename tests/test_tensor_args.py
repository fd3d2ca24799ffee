"""The one check of a tensor argument (`BatchedPredPreyGrass._tensor_arg`) at every call that takes actions, ranks or uniforms,
through the kernel source compiled for the CPU wave emulator: a wrong dtype, a wrong shape and a non-contiguous view each raise
ValueError naming the argument before anything is launched; a correct argument gives what a twin env computes from the same values.
The device condition of the check needs two devices: tests/test_stream_args_gpu.py."""
import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen, config_env_base
from predpreygrass_amd.subbatch import SubBatchedPredPreyGrass
from tests.emu_backend import library

B, S, U = 2, 192, 400   # U: more uniforms than a step of these envs draws (two per live agent)
OUTPUTS = ("obs_pred", "obs_prey", "row_reward", "row_flags", "row_id", "row_xy", "row_energy", "env_state", "grass_energy")


def base():
    return BatchedPredPreyGrass(None, batch_size=B, prey_capacity=128, seed=3, _library=library())


def gen2():
    return BatchedRedQueen(config_env_base, batch_size=B, prey_capacity=128, seed=3, _library=library())


def group():
    return SubBatchedPredPreyGrass(None, batch_size=2 * B, n_sub=2, device="cpu", seed=3, prey_capacity=128, _library=library())


MAKE = {"base": base, "gen2": gen2, "group": group}


@pytest.fixture(scope="module")
def envs():
    """One env per family for the refusals, built once; every test resets the one it uses."""
    made = {"base": base(), "gen2": gen2(), "group": group()}
    assert made["base"].S == made["gen2"].S == S and all(e.S == S for e in made["group"].subs)
    return made


def good(name, seed=0):
    """A correct value of the argument `name`: random actions for every row, ranks in row order, uniforms in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if name == "actions":
        return torch.randint(0, 9, (B, S), generator=g, dtype=torch.int8)
    if name == "tape":
        return torch.randint(0, 9, (2, B, S), generator=g, dtype=torch.int8)
    if name == "act_rank":   # every row acts, in row order: row r of its type is the r-th of its type's sequence
        return torch.cat([torch.arange(64), torch.arange(128)]).to(torch.uint8).repeat(B, 1)
    return torch.rand((B, U), generator=g, dtype=torch.float64)


# id -> (family, argument name in the message, key of good(), call(env, value))
CALLS = {
    "step(actions=)": ("base", "actions", "actions", lambda e, x: e.step(actions=x)),
    "step(act_rank=)": ("base", "act_rank", "act_rank", lambda e, x: e.step(actions=good("actions"), act_rank=x)),
    "rollout(2, actions=)": ("base", "actions", "tape", lambda e, x: e.rollout(2, actions=x)),
    "gen2 step(actions=)": ("gen2", "actions", "actions", lambda e, x: e.step(actions=x)),
    "gen2 step(uniforms=)": ("gen2", "uniforms", "uniforms", lambda e, x: e.step(uniforms=x)),
    "gen2 step(uniforms=, actions=)": ("gen2", "actions", "actions", lambda e, x: e.step(uniforms=good("uniforms"), actions=x)),
    "gen2 step(uniforms=, act_rank=)": ("gen2", "act_rank", "act_rank",
                                        lambda e, x: e.step(uniforms=good("uniforms"), actions=good("actions"), act_rank=x)),
    "sub-batched step(actions=[...])": ("group", "actions", "actions", lambda e, x: e.step(actions=[good("actions", 1), x])),
}


def wrong(name, g):
    """(what, tensor) for every way `g` can be wrong on its own device."""
    other = {torch.int8: torch.int16, torch.uint8: torch.int8, torch.float64: torch.float32}[g.dtype]
    out = [("dtype", g.to(other)), ("dtype bool", g.to(torch.bool)), ("shape: first dimension", g[:1].contiguous()),
           ("shape: one dimension more", g[None].contiguous()), ("shape: one dimension less", g[0].contiguous())]
    if name != "uniforms":   # (their last dimension is free)
        out.append(("shape: last dimension", g[..., :-1].contiguous()))
    doubled = g.repeat_interleave(2, dim=-1)
    out += [("non-contiguous: strided slice of a larger tensor", doubled[..., ::2]),
            ("non-contiguous: transposed", g.transpose(0, 1).contiguous().transpose(0, 1))]
    for what, x in out[-2:]:
        assert tuple(x.shape) == tuple(g.shape) and x.dtype == g.dtype and not x.is_contiguous(), what
    return out


def state(env):
    return [getattr(e, n).clone() for e in getattr(env, "subs", [env]) for n in OUTPUTS]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("call", list(CALLS))
def test_a_wrong_tensor_argument_raises_before_any_launch(envs, call):
    family, name, key, fn = CALLS[call]
    env = envs[family].reset()
    before = state(env)
    for what, x in wrong(key, good(key)):
        with pytest.raises(ValueError, match=name) as err:
            fn(env, x)
        assert "contiguous" in str(err.value) and str(x.dtype) in str(err.value), (what, str(err.value))   # (what it wants, what it got)
        assert same(state(env), before), (what, "the refused call changed the env: something was launched")


def test_a_rollout_without_tape_or_random_actions_is_refused(envs):
    env = envs["base"].reset()
    before = state(env)
    with pytest.raises(ValueError):
        env.rollout(2)
    assert same(state(env), before)


@pytest.mark.parametrize("family", ["base", "gen2"])
def test_act_rank_with_random_actions_is_a_value_error_on_every_path(envs, family):
    """The base class's refusal; with `uniforms=` the second generation used to hand this to the library (RuntimeError)."""
    env = envs[family].reset()
    before = state(env)
    paths = [{}] + ([dict(uniforms=good("uniforms"))] if family == "gen2" else [])
    for kw in paths:
        with pytest.raises(ValueError, match="act_rank"):
            env.step(random_actions=True, act_rank=good("act_rank"), **kw)
    assert same(state(env), before)


@pytest.mark.parametrize("family", ["base", "gen2", "group"])
def test_random_actions_look_at_no_tensor(envs, family):
    env = envs[family].reset()
    bad = torch.zeros((1,), dtype=torch.float32)   # wrong in every respect, and not looked at
    env.step(actions=[bad, bad] if family == "group" else bad, random_actions=True)
    if family == "gen2":
        env.step(actions=bad, random_actions=True, uniforms=good("uniforms"))
    assert all(int(e.env_state[0, _abi.ENV_STEP]) >= 1 for e in getattr(env, "subs", [env]))


def own_actions(env, a):
    env.actions.copy_(a)
    return env


@pytest.mark.parametrize("call", list(CALLS))
def test_a_correct_argument_gives_what_the_twin_computes(call):
    """The twin gets the same values another way: through its own action tensor, as single steps instead of a tape, without ranks
    where the ranks say "row order", with further unused uniforms behind the same ones."""
    family, _, key, fn = CALLS[call]
    env, twin = (MAKE[family]().reset() for _ in range(2))   # (fresh: a used env keeps stale rows)
    start = state(env)
    assert same(start, state(twin))
    x = good(key)
    fn(env, x)
    if call == "step(actions=)" or call == "gen2 step(actions=)":
        own_actions(twin, x).step()
    elif call == "step(act_rank=)":
        own_actions(twin, good("actions")).step()
    elif call == "rollout(2, actions=)":
        for t in range(2):
            twin.step(actions=x[t].clone())
    elif call == "sub-batched step(actions=[...])":
        for e, a in zip(twin.subs, (good("actions", 1), x)):
            own_actions(e, a)
        twin.step()
    else:   # the second generation's uniforms= path
        assert int(env.env_state[:, _abi.ENV_DRAWS].max()) <= U
        longer = torch.cat([x if key == "uniforms" else good("uniforms"), torch.full((B, 7), 0.5, dtype=torch.float64)], dim=1).contiguous()
        if key != "uniforms":
            own_actions(twin, x if key == "actions" else good("actions"))
        twin.step(uniforms=longer)
    assert same(state(env), state(twin)), call
    assert not same(state(env), start), "the step changed nothing: the comparison is empty"
