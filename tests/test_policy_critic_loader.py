"""`load_rllib_state_dict(..., head="vf")`: the critic of an RLlib PPO RLModule state dict as a `PolicyNet(..., n_actions=1)` -- the
network `FusedPolicy.evaluate()` / `AgentTrajectories.values()` run --, from synthetic state dicts in the shapes of
tests/golden/rllib_checkpoint/state_listing.json: a separate critic encoder (what the pinned checkpoint holds) and a shared one
(vf_share_layers).  head="pi", the default, returns exactly what it returned before."""
import json
import os

import pytest
import torch

from predpreygrass_amd.policy import PolicyNet, load_rllib_state_dict

LISTING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rllib_checkpoint", "state_listing.json")


def checkpoint_shaped_state(seed=0):
    """Random tensors under the keys and in the shapes of the pinned checkpoint's predator module (Box(5,9,9), four convolutions, a
    separate critic encoder, Linear(2880, 9) / Linear(2880, 1))."""
    listing = json.load(open(LISTING))["type_1_predator"]["state"]
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v["shape"], generator=gen) for k, v in listing.items()}


def shared_encoder_state(sd):
    """The same module with vf_share_layers: one encoder under encoder.encoder..., no critic encoder."""
    out = {}
    for k, v in sd.items():
        if "critic_encoder" in k:
            continue
        out[k.replace("encoder.actor_encoder.", "encoder.encoder.")] = v
    return out


def tensors_of(net):
    return {k: v for k, v in net.state_dict().items()}


@pytest.mark.parametrize("as_numpy", [False, True])
def test_vf_head_with_a_separate_critic_encoder(as_numpy):
    sd = checkpoint_shaped_state()
    given = {k: v.numpy() for k, v in sd.items()} if as_numpy else sd
    critic = load_rllib_state_dict(given, head="vf")
    assert isinstance(critic, PolicyNet)
    assert (critic.n_actions, critic.layout, critic.obs_range, critic.obs_channels) == (1, "hwc", 9, 5)
    assert critic.conv_channels == (16, 32, 64, 64) and critic.head_hiddens == ()
    got = tensors_of(critic)
    for l, idx in enumerate((1, 4, 7, 10)):   # the critic's tensors under PolicyNet's names, layers in numeric key order
        for part in ("weight", "bias"):
            assert torch.equal(got[f"encoder.actor_encoder.net.0.cnn.{idx}.{part}"], sd[f"encoder.critic_encoder.net.0.cnn.{idx}.{part}"])
            assert not torch.equal(got[f"encoder.actor_encoder.net.0.cnn.{idx}.{part}"], sd[f"encoder.actor_encoder.net.0.cnn.{idx}.{part}"])
    assert torch.equal(got["pi.net.mlp.0.weight"], sd["vf.net.mlp.0.weight"]) and torch.equal(got["pi.net.mlp.0.bias"], sd["vf.net.mlp.0.bias"])
    assert set(got) == {f"encoder.actor_encoder.net.0.cnn.{i}.{p}" for i in (1, 4, 7, 10) for p in ("weight", "bias")} | \
        {"pi.net.mlp.0.weight", "pi.net.mlp.0.bias"}
    x = torch.rand(3, 5, 9, 9)
    assert tuple(critic(x).shape) == (3, 1)


def test_vf_head_with_a_shared_encoder():
    sd = shared_encoder_state(checkpoint_shaped_state(1))
    critic, actor = load_rllib_state_dict(sd, head="vf"), load_rllib_state_dict(sd)
    assert critic.n_actions == 1 and actor.n_actions == 9
    for a, b in zip(critic.conv, actor.conv):   # one encoder serves both
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert torch.equal(critic.fc[0].weight, sd["vf.net.mlp.0.weight"]) and torch.equal(actor.fc[0].weight, sd["pi.net.mlp.0.weight"])


def test_vf_head_with_hidden_layers_and_other_windows():
    """head_fcnet_hiddens gives vf.net.mlp.{0,2}; the reading of the Box follows from the shapes as for the actor."""
    from tests.test_policy import rllib_style_state_dict
    for layout, R in (("hwc", 7), ("chw", 9)):
        torch.manual_seed(R)
        src = PolicyNet(R, 9, layout, head_hiddens=(256,))
        sd = rllib_style_state_dict(src)
        critic = load_rllib_state_dict(sd, head="vf")
        assert (critic.n_actions, critic.layout, critic.obs_range, critic.head_hiddens) == (1, layout, R, (256,))
        assert torch.equal(critic.fc[0].weight, sd["vf.net.mlp.0.weight"]) and torch.equal(critic.fc[1].weight, sd["vf.net.mlp.2.weight"])
        assert torch.equal(critic.conv[0].weight, sd["encoder.critic_encoder.net.0.cnn.1.weight"])


def test_pi_head_is_untouched_and_an_unknown_head_is_refused():
    sd = checkpoint_shaped_state(2)
    default, named = load_rllib_state_dict(sd), load_rllib_state_dict(sd, head="pi")
    want = {k: v for k, v in sd.items() if k.startswith("encoder.actor_encoder.") or k.startswith("pi.net.")}
    for net in (default, named):
        got = tensors_of(net)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert net.n_actions == 9
    with pytest.raises(ValueError):
        load_rllib_state_dict(sd, head="critic")
    no_vf = {k: v for k, v in sd.items() if not k.startswith("vf.")}
    with pytest.raises(ValueError):
        load_rllib_state_dict(no_vf, head="vf")
