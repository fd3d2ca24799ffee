"""Scenarios of `ppg_net_forward` / `ppg_net_backward` (a PolicyNet's float32 minibatch forward and backward; include/ppg.h,
csrc/ppg_net.h), `env.net_forward()` / `env.net_backward()`, `trajectory.NetLearner` and `AgentTrajectories.forward()`, shared by the
wave-emulator tests (test_net_emulated.py) and the GPU tests (test_net_gpu.py).  No tests of its own.

Reference (`reference`): the same `PolicyNet` as `.double()`, run on `obs[index].double()` (the rows first converted as
`obs.to(torch.float32)` does) with torch autograd on the CPU; it is computed once per (network, batch) and shared.
Measure (`measure`), per tensor -- `out` and every gradient tensor: max|x - ref| / max|ref|.  Bound: 1e-4.  A float32 chain over N terms
errs by about sqrt(N) * 2^-24 of the sum of magnitudes and at most N * 2^-24; the longest chain here is a weight gradient over
M * P <= 130 * 81 terms, so typical errors are near 6e-6, while a dropped tap, a transposed weight, a wrong flatten order or a missed
ReLU mask shows at 1e-2 or more.  `inputs_hold()` (run on the CPU by test_net_emulated.py) checks what the bound rests on: torch's own
float32 autograd stays below 1e-5 under the same measure on every batch, and every reference tensor's max|ref| exceeds 1e-3 -- the
observations are zeros and small energies as the env writes them and the weights PyTorch's default initialisation times 4 -- so the
relative bound never sits on a zero tensor.  The figures are in profiles/EXPERIMENTS.md."""
import ctypes as C
import functools

import numpy as np
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import net_grad_views
from predpreygrass_amd.policy import PolicyNet
from tests.record_cases import sync

BOUND = 1e-4
TORCH_F32_BOUND = 1e-5
MIN_REF = 1e-3
CAPACITY = 41
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# name -> PolicyNet(obs_range, n_actions, layout, obs_channels, conv_channels, head_hiddens, flatten)
NETWORKS = {
    "r5_hwc_8_a3": (5, 3, "hwc", 4, (8,), (), None),
    "r5_chw_c5_8_16_a9": (5, 9, "chw", 5, (8, 16), (), None),
    "r5_hwc_flat_nchw_a2": (5, 2, "hwc", 4, (8, 8), (), "nchw"),
    "r5_chw_flat_nhwc_a2": (5, 2, "chw", 4, (8, 8), (), "nhwc"),
    "r5_hwc_six_convs_a9": (5, 9, "hwc", 4, (8,) * 6, (), None),
    "predator_r7_a9": (7, 9, "hwc", 4, (16, 32, 64), (), None),
    "prey_r9_a25": (9, 25, "hwc", 4, (16, 32, 64), (), None),
    "predator_critic_r7": (7, 1, "hwc", 4, (16, 32, 64), (), None),
    "prey_critic_r9": (9, 1, "hwc", 4, (16, 32, 64), (), None),
    "r7_chw_hidden_32_a9": (7, 9, "chw", 4, (16, 32, 64), (32,), None),
    "r7_chw_hidden_256_64_a9": (7, 9, "chw", 4, (16, 32, 64), (256, 64), None),
    "r15_chw_c8_a9": (15, 9, "chw", 8, (16, 32, 64), (), None),
}
SMALLEST = ("r5_hwc_8_a3", "r5_chw_c5_8_16_a9")
M_KINDS = ("1", "TS-1", "TS", "TS+1", "2TS+3", "5TS+1/groups=2")


def make_net(name, seed=0):
    """The network `name` on the CPU: PyTorch's default initialisation (seeded) scaled up by 4."""
    R, A, layout, C_, conv, hidden, flatten = NETWORKS[name]
    torch.manual_seed(1000 + seed + sum(map(ord, name)))
    net = PolicyNet(R, A, layout, obs_channels=C_, conv_channels=conv, head_hiddens=hidden, flatten=flatten)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(4.0)
    return net


def clone_net(net, dtype=torch.float32, device="cpu"):
    twin = PolicyNet(net.obs_range, net.n_actions, net.layout, obs_channels=net.obs_channels, conv_channels=net.conv_channels,
                     head_hiddens=net.head_hiddens, flatten=net.flatten)
    twin.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return twin.to(dtype).to(device)


def params_of(net):
    """conv0.weight, conv0.bias, ..., fc0.weight, fc0.bias, ...: the order of the flat gradient buffer."""
    return [p for m in net.conv + net.fc for p in (m.weight, m.bias)]


def forward_in(net, rows):
    """PolicyNet.forward without its cast to float32: `net` in the dtype of its parameters."""
    x = rows
    if net.layout == "hwc":
        x = x.permute(0, 3, 1, 2)
    x = net.encoder.actor_encoder.net[0].cnn(x)
    if net.flatten == "nhwc":
        x = x.permute(0, 2, 3, 1)
    return net.pi.net.mlp(x.flatten(1))


def observations(net, capacity, seed, dtype=torch.float32):
    """[capacity,C,R,R]: mostly zeros, energies up to 4 elsewhere (multiples of 1/64: exact in bfloat16 too)."""
    g = torch.Generator().manual_seed(seed)
    shape = (capacity, net.obs_channels, net.obs_range, net.obs_range)
    e = torch.randint(1, 257, shape, generator=g).to(torch.float32) / 64.0
    return torch.where(torch.rand(shape, generator=g) < 0.3, e, torch.zeros(shape)).to(dtype)


def tile_rows(env, net):
    return env.net_bytes(net, 1)[3]


def rows_of(kind, TS):
    """(M, groups) of a shape of M_KINDS, or None where it is no minibatch (TS - 1 = 0)."""
    M = {"1": 1, "TS-1": TS - 1, "TS": TS, "TS+1": TS + 1, "2TS+3": 2 * TS + 3, "5TS+1/groups=2": 5 * TS + 1}[kind]
    return (M, 2 if "groups" in kind else 0) if M >= 1 else None


def batch(name, M, index="perm", dtype=torch.float32, seed=0, capacity=CAPACITY):
    """A CPU batch: net, obs [capacity,...] of `dtype`, index int32 [M] (a permutation with repeats) or None, grad_out [M,n_out]."""
    net = make_net(name)
    g = torch.Generator().manual_seed(77 + seed + 13 * M)
    obs = observations(net, max(capacity, M), 5 + seed, dtype)
    idx = None
    if index == "perm":
        idx = torch.randint(0, obs.shape[0], (M,), generator=g).to(torch.int32)
        if M >= 2:
            idx[M - 1] = idx[0]   # the same slot twice in a minibatch is legal
    grad_out = torch.randn((M, net.n_actions), generator=g)
    return dict(name=name, net=net, obs=obs, index=idx, grad_out=grad_out, M=M)


def reference_of(net, obs, index, grad_out, valid=None, dtype=torch.float64):
    """(out, [gradients]) of `net` as `dtype` on the CPU with autograd over the rows obs[index] (valid: bool [M], the others are
    selections: out 0, nothing in any gradient)."""
    ref = clone_net(net, dtype)
    M = grad_out.shape[0]
    k = torch.arange(M) if index is None else index.long()
    valid = torch.ones(M, dtype=torch.bool) if valid is None else valid
    rows = obs.cpu()[k[valid]].to(torch.float32).to(dtype)
    out = torch.zeros((M, net.n_actions), dtype=dtype)
    if rows.shape[0]:
        o = forward_in(ref, rows)
        o.backward(grad_out.cpu()[valid].to(dtype))
        out[valid] = o.detach()
    return out, [torch.zeros_like(p) if p.grad is None else p.grad for p in params_of(ref)]


@functools.lru_cache(maxsize=None)
def _cached(name, M, index, dtype, seed):
    b = batch(name, M, index, dtype, seed)
    return b, reference_of(b["net"], b["obs"], b["index"], b["grad_out"])


def measure(got, ref):
    ref = ref.detach().cpu().double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def tensor_names(net):
    return ["out"] + [f"{kind}{l}.{p}" for kind, n in (("conv", len(net.conv)), ("fc", len(net.fc))) for l in range(n) for p in ("weight", "bias")]


def check(got_out, got_grads, ref, net, tag, bound=BOUND):
    worst = 0.0
    for name, got, want in zip(tensor_names(net), [got_out, *got_grads], [ref[0], *ref[1]]):
        assert tuple(got.shape) == tuple(want.shape), (tag, name, got.shape, want.shape)
        err = measure(got, want)
        print(f"{tag} {name}: {err:.2e}")
        assert err <= bound, (tag, name, err)
        worst = max(worst, err)
    return worst


def run(env, b, groups=0, net=None):
    """(out, [gradient views], flat gradients, partial) of the two raw tensor calls on the backend under test."""
    dev = env.device
    net = clone_net(b["net"], device=dev) if net is None else net
    obs = b["obs"].to(dev)
    idx = None if b["index"] is None else b["index"].to(dev)
    out, ws = env.net_forward(net, obs, idx, M=b["M"], groups=groups)
    flat, partial = env.net_backward(net, obs, idx, b["grad_out"].to(dev), ws, M=b["M"], groups=groups)
    sync(env)
    return out, [v for _, v in net_grad_views(net, flat)], flat, partial


# ---- 0. what the bound rests on (CPU only) -------------------------------------------------------------------------------------------

def all_batches(TS_of):
    for name in NETWORKS:
        for kind in M_KINDS:
            mg = rows_of(kind, TS_of(name))
            if mg:
                for index in (None, "perm"):
                    yield name, kind, mg, index


def inputs_hold(env, report=None):
    """Every batch of `shapes`: torch's float32 autograd within TORCH_F32_BOUND of the float64 reference, every max|ref| above MIN_REF."""
    for name, kind, (M, groups), index in all_batches(lambda n: tile_rows(env, make_net(n))):
        b, ref = _cached(name, M, index, torch.float32, 0)
        f32 = reference_of(b["net"], b["obs"], b["index"], b["grad_out"], dtype=torch.float32)
        worst = 0.0
        for tname, got, want in zip(tensor_names(b["net"]), [f32[0], *f32[1]], [ref[0], *ref[1]]):
            assert float(want.abs().max()) > MIN_REF, (name, kind, index, tname, float(want.abs().max()))
            worst = max(worst, measure(got, want))
        assert worst < TORCH_F32_BOUND, (name, kind, index, worst)
        if report is not None:
            report.append((name, kind, index, worst))


# ---- 1. shapes of M, with and without an index -----------------------------------------------------------------------------------------

def shapes(env, name, report=None):
    TS = tile_rows(env, make_net(name))
    for kind in M_KINDS:
        mg = rows_of(kind, TS)
        if not mg:
            continue
        for index in (None, "perm"):
            b, ref = _cached(name, mg[0], index, torch.float32, 0)
            out, grads, _, _ = run(env, b, groups=mg[1])
            worst = check(out, grads, ref, b["net"], f"{name} M={kind} index={index}")
            if report is not None:
                report.append((name, kind, index, worst))


# ---- 2. row dtypes ------------------------------------------------------------------------------------------------------------------------

def row_dtypes(env, name):
    TS = tile_rows(env, make_net(name))
    for dtype in (torch.float64, torch.float32, torch.bfloat16):
        b, ref = _cached(name, 2 * TS + 3, "perm", dtype, 1)
        out, grads, _, _ = run(env, b)
        check(out, grads, ref, b["net"], f"{name} rows {dtype}")
    # float64 rows that float32 cannot hold are rounded as .to(torch.float32) rounds them
    b = batch(name, TS + 1, "perm", torch.float64, 2)
    b["obs"] = b["obs"] * (1.0 + 2.0 ** -30)
    out, grads, _, _ = run(env, b)
    check(out, grads, reference_of(b["net"], b["obs"], b["index"], b["grad_out"]), b["net"], f"{name} rows float64 off the float32 grid")


# ---- 3. invalid slots -----------------------------------------------------------------------------------------------------------------------

def invalid_slots(env, name):
    """-1, capacity, INT32_MIN and INT32_MAX mixed into a minibatch: +0.0 out rows, NaN grad_out rows never read, observation rows outside
    the indexed set NaN and never read; appended behind the valid rows of the last tile they change no bit of any gradient."""
    net = make_net(name)
    TS = tile_rows(env, net)
    cap = CAPACITY
    bad = torch.tensor([-1, cap, INT32_MIN, INT32_MAX], dtype=torch.int64)
    # (a) mixed in
    M = 3 * TS + 2
    b = batch(name, M, "perm", seed=3)
    where = torch.tensor([0, TS, 2 * TS + 1, M - 1][:min(4, M)])
    idx = b["index"].long()
    idx[where] = bad[:len(where)]
    b["index"] = idx.to(torch.int32)
    valid = torch.ones(M, dtype=torch.bool)
    valid[where] = False
    b["grad_out"][where] = float("nan")
    used = torch.zeros(cap, dtype=torch.bool)
    used[idx[valid]] = True
    b["obs"][~used] = float("nan")
    ref = reference_of(net, b["obs"], b["index"], b["grad_out"], valid)
    out, grads, _, _ = run(env, b)
    check(out, grads, ref, net, f"{name} invalid slots mixed in")
    rows = out.cpu().numpy()[where.numpy()]
    assert rows.view(np.uint32).max() == 0, "an invalid row's out is not +0.0"
    # (b) appended at the end of the last tile: the gradients of the minibatch without them, to the bits
    for n_valid in ((2 * TS + 1,) if TS > 1 else ()):
        short = batch(name, n_valid, "perm", seed=4)
        room = (-n_valid) % TS
        assert 1 <= room
        long_ = dict(short)
        long_["M"] = n_valid + room
        long_["index"] = torch.cat([short["index"], bad[:room].to(torch.int32)])
        long_["grad_out"] = torch.cat([short["grad_out"], torch.full((room, net.n_actions), float("nan"))])
        out_s, _, flat_s, _ = run(env, short)
        out_l, _, flat_l, _ = run(env, long_)
        assert torch.equal(flat_s.cpu().view(torch.int32), flat_l.cpu().view(torch.int32)), "appended invalid rows changed a gradient bit"
        assert torch.equal(out_s.cpu().view(torch.int32), out_l[:n_valid].cpu().view(torch.int32))
        assert out_l[n_valid:].cpu().view(torch.int32).abs().max() == 0
    # (c) a minibatch of selections only, and a store of capacity 0
    none = batch(name, TS + 1, "perm", seed=5)
    none["index"] = bad[torch.arange(TS + 1) % 4].to(torch.int32)
    none["grad_out"][:] = float("nan")
    none["obs"][:] = float("nan")
    out, _, flat, _ = run(env, none)
    assert out.cpu().view(torch.int32).abs().max() == 0 and flat.cpu().view(torch.int32).abs().max() == 0
    empty = dict(none, obs=none["obs"][:0], index=None)
    out, _, flat, _ = run(env, empty)
    assert out.cpu().view(torch.int32).abs().max() == 0 and flat.cpu().view(torch.int32).abs().max() == 0


# ---- 4. ReLU at zero ------------------------------------------------------------------------------------------------------------------------

def relu_at_zero(env):
    """A convolution channel and a hidden unit whose pre-activation is exactly 0 take torch's convention: gradient 0."""
    for name in ("r5_hwc_8_a3", "r7_chw_hidden_32_a9"):
        b = batch(name, 6, "perm", seed=6)
        net = b["net"]
        with torch.no_grad():
            net.conv[0].weight[0].zero_()
            net.conv[0].bias[0] = 0.0
            if len(net.fc) > 1:
                net.fc[0].weight[1].zero_()
                net.fc[0].bias[1] = 0.0
        ref = reference_of(net, b["obs"], b["index"], b["grad_out"])
        out, grads, _, _ = run(env, b)
        check(out, grads, ref, net, f"{name} relu at zero")
        assert not bool(grads[0][0].any()) and float(grads[1][0]) == 0.0 and not bool(ref[1][0][0].any())
        if len(net.fc) > 1:
            w = grads[2 * len(net.conv)]
            assert not bool(w[1].any()) and not bool(ref[1][2 * len(net.conv)][1].any())


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------

def determinism(env, name, M=None):
    TS = tile_rows(env, make_net(name))
    b = batch(name, M or 5 * TS + 1, "perm", seed=7)
    first = run(env, b)
    second = run(env, b)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[2].view(torch.int32), second[2].view(torch.int32)), "two backward calls on the same inputs differ"


# ---- 6. untouched memory, refused calls -------------------------------------------------------------------------------------------------------

GUARD, FILL = 64, 0x5A


def guarded(env, n, dtype=torch.float32):
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * GUARD) * size,), FILL, dtype=torch.uint8, device=env.device)
    return raw[GUARD * size:(GUARD + n) * size].view(dtype), raw


def untouched(env, name="r5_chw_c5_8_16_a9"):
    """The raw calls into buffers of exactly their stated size between guard bytes; every refused call returns -1 with its message and
    writes nothing."""
    import pytest
    lib, dev = env._lib, env.device
    b = batch(name, 0 + 11, "perm", seed=8)
    M = b["M"]
    net = clone_net(b["net"], device=dev)
    A = net.n_actions
    ws_bytes, partial_bytes, n_params, TS = env.net_bytes(net, M)
    obs, idx, grad_out = b["obs"].to(dev), b["index"].to(dev), b["grad_out"].to(dev)
    views, whole = {}, {}
    for key, n in (("out", M * A), ("workspace", ws_bytes // 4), ("partial", partial_bytes // 4)):
        views[key], whole[key] = guarded(env, n)
    # every gradient tensor in a guarded block of its own: an overrun into a neighbouring parameter's gradient shows in the guard bytes
    grad_blocks = []
    for q, p in enumerate(params_of(net)):
        views[f"grad{q}"], whole[f"grad{q}"] = guarded(env, p.numel())
        grad_blocks.append(views[f"grad{q}"].view(p.shape))
    before = {k: v.cpu().numpy().copy() for k, v in whole.items()}
    spec = env._net_spec(net)
    from predpreygrass_amd.policy import FusedPolicy
    blocks = iter(grad_blocks)
    gspec = FusedPolicy._spec(net, lambda p: next(blocks).data_ptr())
    assert n_params == sum(g.numel() for g in grad_blocks)

    def mb_of(**kw):
        mb = _abi.PpgNetBatch()
        mb.obs, mb.obs_dtype, mb.groups, mb.capacity = obs.data_ptr(), 1, 0, obs.shape[0]
        mb.index, mb.M, mb.out = idx.data_ptr(), M, views["out"].data_ptr()
        mb.workspace, mb.workspace_bytes = views["workspace"].data_ptr(), ws_bytes
        for k, v in kw.items():
            setattr(mb, k, v)
        return mb

    def spec_of(base, **kw):
        sp = _abi.PpgPolicySpec.from_buffer_copy(bytes(base))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(sp, k)[v[0]] = v[1]
            else:
                setattr(sp, k, v)
        return sp

    def forward(mb=None, sp=spec, null=()):
        return lib.ppg_net_forward(env._handle, None if "spec" in null else C.byref(sp), None if "mb" in null else C.byref(mb or mb_of()),
                                   env._stream())

    def backward(mb=None, sp=spec, gs=gspec, null=(), pbytes=partial_bytes):
        return lib.ppg_net_backward(env._handle, None if "spec" in null else C.byref(sp), None if "mb" in null else C.byref(mb or mb_of()),
                                    None if "grad_out" in null else C.c_void_p(grad_out.data_ptr()),
                                    None if "grads" in null else C.byref(gs),
                                    None if "partial" in null else C.c_void_p(views["partial"].data_ptr()), pbytes, env._stream())

    bad_batches = [dict(obs=None), dict(workspace=None), dict(M=0), dict(M=-3), dict(M=2 ** 24 + 1), dict(capacity=-1),
                   dict(capacity=2 ** 31), dict(workspace_bytes=ws_bytes - 4), dict(obs_dtype=3), dict(obs_dtype=-1), dict(groups=-1)]
    bad_specs = [dict(n_conv=0), dict(n_conv=7), dict(conv_out=(0, 17)), dict(obs_range=16), dict(obs_channels=9), dict(layout=2),
                 dict(flatten=2), dict(n_fc=0), dict(n_actions=33), dict(fc_out=(0, A + 1)), dict(conv_w=(1, None)), dict(fc_b=(0, None))]
    refused = [("f", lambda: forward(null=("spec",))), ("f", lambda: forward(null=("mb",))), ("f", lambda: forward(mb_of(out=None))),
               ("b", lambda: backward(null=("spec",))), ("b", lambda: backward(null=("mb",))), ("b", lambda: backward(null=("grad_out",))),
               ("b", lambda: backward(null=("grads",))), ("b", lambda: backward(null=("partial",))),
               ("b", lambda: backward(pbytes=partial_bytes - 4)), ("b", lambda: backward(gs=spec_of(gspec, conv_b=(0, None))))]
    refused += [(w, (lambda kw=kw, fn=fn: fn(mb_of(**kw)))) for kw in bad_batches for w, fn in (("f", forward), ("b", backward))]
    refused += [(w, (lambda kw=kw, fn=fn: fn(sp=spec_of(spec, **kw)))) for kw in bad_specs for w, fn in (("f", forward), ("b", backward))]
    for n, (which, call) in enumerate(refused):
        assert call() == -1, n
        want = b"ppg_net_forward:" if which == "f" else b"ppg_net_backward:"
        assert lib.ppg_last_error(env._handle).startswith(want), (n, lib.ppg_last_error(env._handle))
    # the shape rules speak ppg_policy_create_spec's words
    forward(sp=spec_of(spec, conv_out=(0, 17)))
    assert b"convolution 1 has 17 output channels: the kernels take up to 16 / 32 / 64 / 64 ..." in lib.ppg_last_error(env._handle)
    out4 = (C.c_uint64 * 4)()
    assert lib.ppg_net_bytes(C.byref(spec_of(spec, obs_range=16)), M, 0, C.byref(out4)) == -1
    assert lib.ppg_net_bytes(C.byref(spec), 0, 0, C.byref(out4)) == -1 and lib.ppg_net_bytes(None, M, 0, C.byref(out4)) == -1
    sync(env)
    for k, v in whole.items():
        assert np.array_equal(v.cpu().numpy(), before[k]), (k, "a refused call wrote")
    assert forward() == 0 and backward() == 0
    sync(env)
    ref = reference_of(b["net"], b["obs"], b["index"], b["grad_out"])
    check(views["out"].view(M, A), grad_blocks, ref, net, "raw calls")
    for k, v in whole.items():
        raw = v.cpu().numpy()
        assert (raw[:GUARD * 4] == FILL).all() and (raw[-GUARD * 4:] == FILL).all(), (k, "a guard byte was written")
    assert torch.equal(obs.cpu(), b["obs"]) and torch.equal(grad_out.cpu(), b["grad_out"])
    # the wrappers' own refusals
    ws = views["workspace"]
    wrong = [lambda: env.net_forward(net, obs.to(torch.float16), idx), lambda: env.net_forward(net, obs[:, :, :-1].contiguous(), idx),
             lambda: env.net_forward(net, obs, idx.long()), lambda: env.net_forward(net, obs, idx, M=M - 1),
             lambda: env.net_forward(net, obs, idx, out=views["out"].view(M, A)[:-1]),
             lambda: env.net_forward(net, obs, idx, workspace=ws[:-1]), lambda: env.net_forward(net.double(), obs, idx),
             lambda: env.net_backward(net.float(), obs, idx, grad_out[:-1], ws), lambda: env.net_backward(net, obs, idx, grad_out.double(), ws),
             lambda: env.net_backward(net, obs, idx, grad_out, ws, grads=torch.empty((n_params - 1,), device=dev)),
             lambda: env.net_backward(net, obs, idx, grad_out, ws, partial=views["partial"][:-1])]
    for n, call in enumerate(wrong):
        with pytest.raises(ValueError):
            call()
        net.float()
    sync(env)
    for k, v in whole.items():
        raw = v.cpu().numpy()
        assert (raw[:GUARD * 4] == FILL).all() and (raw[-GUARD * 4:] == FILL).all(), (k, "a guard byte was written")


# ---- 7. autograd: NetLearner, ppo_loss_function, an optimiser ----------------------------------------------------------------------------------

def recorded_trajectory(env, T=6, seed=21):
    """A short rollout with synthetic logits through AgentTrajectories (as ppo_loss_cases.recorded): the store, and per species the
    advantages, returns and advantage norm."""
    from predpreygrass_amd.trajectory import AgentTrajectories
    from tests import logp_cases, obs_store_cases as oc
    A, B = logp_cases.ROLLOUT_ACTIONS["base"], env.batch_size
    env.reset()
    traj = AgentTrajectories(env, T, obs_rows=tuple(T * B * r for r in oc.BUDGET["base"]), logp=A, dist=True)
    gen, gen2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 1)
    for t in range(T):
        logits, acts = logp_cases.synthetic(env, gen2, A, scale=1.5)
        traj.record_policy(logits, acts)
        actions = oc.random_actions(env, gen)
        env.step(actions, auto_reset=True)
        traj.record(actions)
    sync(env)
    counts = traj.store.cursor[:2].tolist()
    v = [torch.randn((n,), generator=gen2).to(env.device) for n in counts]
    adv, ret, moments = traj.targets(v[0], v[1], 0.99, 0.95)
    return traj, counts, adv, ret, traj.advantage_norm(moments), A


def species_nets(env, s, A, conv, seed):
    """(actor, critic) for species s of the env's observation geometry, on the env's device."""
    R = (env.Rp, env.Rq)[s]
    nets = []
    for n_out in (A, 1):
        torch.manual_seed(seed + n_out)
        net = PolicyNet(R, n_out, "hwc", obs_channels=4, conv_channels=conv)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(4.0 if n_out > 1 else 1.0)
        nets.append(net.to(env.device))
    return nets


HYPER = dict(clip=0.3, vf_clip=10.0, vf_coeff=0.5, ent_coeff=0.01, kl_coeff=0.2)


def autograd(env, M=24, conv=(16, 32, 64)):
    """NetLearner's output through ppo_loss_function and loss.backward() against the all-torch path, per species; a second backward
    accumulates; torch.autograd.backward with explicit gradients; a second forward before the backward raises."""
    import pytest
    from predpreygrass_amd.trajectory import NetLearner, ppo_loss_function
    traj, counts, adv, ret, norm, A = recorded_trajectory(env)
    gen = torch.Generator().manual_seed(5)
    for s in (0, 1):
        n = counts[s]
        assert n >= M
        index = torch.randperm(n, generator=gen)[:M].to(torch.int32).to(env.device)
        actor, critic = species_nets(env, s, A[s], conv, 40 + s)
        twins = [clone_net(net, device=env.device) for net in (actor, critic)]
        learners = [NetLearner(env, net, max_rows=M + 3) for net in (actor, critic)]
        obs = traj.store.obs[s]

        def step(kernel):
            if kernel:
                logits, values = traj.forward(learners[0], s, index), traj.forward(learners[1], s, index)[:, 0]
            else:
                rows = obs[index.long()]
                logits, values = twins[0](rows), twins[1](rows)[:, 0]
            loss, _ = ppo_loss_function(traj, s, logits, values, index, adv[s], ret[s], adv_norm=norm, **HYPER)
            loss.backward()
            return float(loss.detach())
        lk, lt = step(True), step(False)
        sync(env)
        assert abs(lk - lt) <= 1e-4 * max(abs(lt), 1.0), (lk, lt)
        for net, twin, tag in ((actor, twins[0], "actor"), (critic, twins[1], "critic")):
            for (name, p), q in zip(net.named_parameters(), twin.parameters()):
                assert float(q.grad.abs().max()) > 0, (tag, name)
                err = measure(p.grad, q.grad)
                print(f"species {s} {tag} {name}: p.grad against the all-torch path {err:.2e}")
                assert err <= BOUND, (s, tag, name, err)
        once = [p.grad.clone() for p in actor.parameters()]
        assert all(p.grad.data_ptr() != v.data_ptr() for p, v in zip(params_of(actor), learners[0].grad_views))
        step(True)   # a second backward accumulates
        for p, g in zip(actor.parameters(), once):
            assert torch.equal(p.grad, g + g), "a second backward did not accumulate"
        # explicit gradients, as INTEGRATION.md's loop has them
        for p in actor.parameters():
            p.grad = None
        logits = learners[0](obs, index)
        gl = torch.randn(logits.shape, generator=gen).to(env.device)
        torch.autograd.backward([logits], [gl])
        want = reference_of(actor, obs, index.cpu(), gl)
        check(logits, [p.grad for p in params_of(actor)], want, actor, f"species {s} autograd.backward([logits], [grad_logits])")
        # the workspace belongs to one forward until its backward
        first = learners[0](obs, index)
        with pytest.raises(RuntimeError, match="second forward"):
            learners[0](obs, index)
        first.sum().backward()
        with torch.no_grad():
            assert torch.equal(learners[0](obs, index), learners[0](obs, index))   # evaluation holds nothing
        held = learners[0](obs, index)
        learners[0].release()
        again = learners[0](obs, index)
        with pytest.raises(RuntimeError, match="are gone"):
            held.sum().backward()
        again.sum().backward()
        moved = learners[0](obs, index)
        with torch.no_grad():
            params_of(actor)[0].mul_(1.0)   # an in-place change between forward and backward: the activations are of other weights
        with pytest.raises(RuntimeError, match="changed in place"):
            moved.sum().backward()
        learners[0].release()
        with pytest.raises(ValueError, match="max_rows"):
            learners[0](obs, torch.zeros(M + 4, dtype=torch.int32, device=env.device))


def sgd_steps(env, M=24, conv=(8, 8), steps=10, lr=1e-3):
    """Ten SGD steps of the kernel path and of the torch path from the same weights: the final losses within 1e-3 relative."""
    from predpreygrass_amd.trajectory import NetLearner, ppo_loss_function
    traj, counts, adv, ret, norm, A = recorded_trajectory(env)
    s = 1
    gen = torch.Generator().manual_seed(9)
    index = torch.randperm(counts[s], generator=gen)[:M].to(torch.int32).to(env.device)
    obs = traj.store.obs[s]
    nets = species_nets(env, s, A[s], conv, 60)
    twins = [clone_net(net, device=env.device) for net in nets]
    learners = [NetLearner(env, net, max_rows=M) for net in nets]
    losses = []
    for kernel, pair in ((True, nets), (False, twins)):
        opt = torch.optim.SGD([p for net in pair for p in net.parameters()], lr=lr)
        for _ in range(steps + 1):
            opt.zero_grad()
            if kernel:
                logits, values = learners[0](obs, index), learners[1](obs, index)[:, 0]
            else:
                rows = obs[index.long()]
                logits, values = pair[0](rows), pair[1](rows)[:, 0]
            loss, _ = ppo_loss_function(traj, s, logits, values, index, adv[s], ret[s], adv_norm=norm, **HYPER)
            last = float(loss.detach())
            loss.backward()
            opt.step()
        losses.append(last)
    diff = abs(losses[0] - losses[1]) / abs(losses[1])
    print(f"loss after {steps} SGD steps: kernel path {losses[0]!r}, torch path {losses[1]!r}, relative difference {diff:.2e}")
    assert diff <= 1e-3, (losses, diff)
    return diff


# ---- 8. GPU only ---------------------------------------------------------------------------------------------------------------------------

def store_minibatch(env, M, groups=(0,)):
    """The reference's two networks (and their critics) over a recorded rollout's store through AgentTrajectories.forward at M rows (with
    repeats where the store holds fewer), against the float64 reference; `groups`: each forced G gives gradients within the bound too."""
    from predpreygrass_amd.trajectory import NetLearner
    traj, counts, adv, ret, norm, A = recorded_trajectory(env)
    gen = torch.Generator().manual_seed(31)
    for s in (0, 1):
        index = torch.randint(0, counts[s], (M,), generator=gen).to(torch.int32)
        for net in species_nets(env, s, A[s], (16, 32, 64), 70 + s):
            obs = traj.store.obs[s]
            grad_out = torch.randn((M, net.n_actions), generator=gen)
            ref = reference_of(net, obs, index, grad_out)
            for g in groups:
                learner = NetLearner(env, net, max_rows=M, groups=g)
                for p in net.parameters():
                    p.grad = None
                out = traj.forward(learner, s, index.to(env.device))
                torch.autograd.backward([out], [grad_out.to(env.device)])
                sync(env)
                check(out, [p.grad for p in params_of(net)], ref, net, f"species {s} n_out {net.n_actions} M={M} groups={g}")


def graphed(env, M=128):
    """forward + ppo_loss + backward captured in one graph and replayed after the weights changed: the replay's gradients are those of
    the new weights."""
    from predpreygrass_amd.batched import capture_graph
    traj, counts, adv, ret, norm, A = recorded_trajectory(env)
    for s in (0, 1):   # (the prey network's tile takes 73 728 B of LDS: above the 64 KB a kernel gets without being asked)
        _graphed_species(env, traj, counts, adv, norm, A, s, M)


def _graphed_species(env, traj, counts, adv, norm, A, s, M):
    from predpreygrass_amd.batched import capture_graph
    dev = env.device
    gen = torch.Generator().manual_seed(41)
    index = torch.randint(0, counts[s], (M,), generator=gen).to(torch.int32).to(dev)
    actor, _ = species_nets(env, s, A[s], (16, 32, 64), 80)
    obs = traj.store.obs[s]
    need = env.net_bytes(actor, M)
    out = torch.empty((M, A[s]), dtype=torch.float32, device=dev)
    ws = torch.empty((need[0] // 4,), dtype=torch.float32, device=dev)
    flat = torch.empty((need[2],), dtype=torch.float32, device=dev)
    partial = torch.empty((need[1] // 4,), dtype=torch.float32, device=dev)
    held = {}

    def body():
        env.net_forward(actor, obs, index, out=out, workspace=ws)
        held["loss"] = traj.ppo_loss(s, out, None, index, adv[s], None, adv_norm=norm, **HYPER)
        env.net_backward(actor, obs, index, held["loss"][2], ws, grads=flat, partial=partial)
    graph = capture_graph(dev, body)
    with torch.no_grad():
        for p in actor.parameters():
            p.mul_(0.5).add_(0.01)
    graph.replay()
    sync(env)
    grad_logits = held["loss"][2].clone()
    ref = reference_of(actor, obs, index.cpu(), grad_logits)
    check(out, [v for _, v in net_grad_views(actor, flat)], ref, actor, f"species {s}: graph replay with changed weights")
    eager_out, _ = env.net_forward(actor, obs, index)
    assert torch.equal(eager_out, out)
