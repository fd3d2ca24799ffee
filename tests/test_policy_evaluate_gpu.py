"""`FusedPolicy.evaluate()` / `ppg_policy_evaluate` (plan kernel ppg_policy_plan_rows in front of the forward kernels of
ppg_policy_act) and `AgentTrajectories.values()` / `logits()` on the MI355X.  The reference is `act`: over a recorded sample store the
evaluation gives, bit for bit, the logits `act` wrote for the same rows -- same kernels, same rows, same weights -- in every kernel
family and row dtype; counts as an int and as a device word; independence of a row's position; shares larger than a tile; a critic
(n_actions = 1) against the float32 torch forward within tests/test_policy.py's tolerance; HIP graphs on both sides; the refusals."""
import ctypes

import pytest
import torch

from predpreygrass_amd import _abi
from predpreygrass_amd.batched import BatchedPredPreyGrass, capture_graph
from predpreygrass_amd.config import config_env
from predpreygrass_amd.policy import FusedPolicy, GraphedPolicyStep, PolicyNet
from predpreygrass_amd.trajectory import AgentTrajectories, ObservationStore
from tests.test_policy import REL_TOL, make_nets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T = 8, 5
STATE = ("row_xy", "row_energy", "row_id", "row_flags", "row_reward", "row_cumrew", "env_state", "grass_energy", "obs_pred", "obs_prey", "actions")

# one network per kernel family: (predator window, prey window, PolicyNet keywords, PPG_POLICY_PIPE)
FAMILIES = {
    "rllib-default-pipeline": (7, 9, {}, None),
    "one-role-direct": (7, 9, {}, "0"),
    "fc-chain": (7, 9, dict(head_hiddens=(256, 256)), None),
    "chw": (7, 9, dict(layout="chw"), None),
    "deep": (7, 9, dict(conv_channels=(16, 32, 64, 64)), None),
    "16-channel-staging": (9, 11, {}, None),
}


def bits(x):
    return x.contiguous().view(torch.int32)


def make_policy(family, seed, monkeypatch, **more):
    Rp, Rq, kw, pipe = FAMILIES[family]
    if pipe is not None:
        monkeypatch.setenv("PPG_POLICY_PIPE", pipe)
    nets = [n.to(DEV) for n in make_nets(Rp, Rq, seed=seed, **kw, **more)]
    return nets, FusedPolicy(nets[0], nets[1])


def make_env(Rp=7, Rq=9, seed=4, **kw):
    env = BatchedPredPreyGrass({**config_env, "predator_obs_range": Rp, "prey_obs_range": Rq}, batch_size=B, device=DEV, seed=seed, **kw)
    env.reset()
    return env


def record_rollout(env, fused, A, store_dtype=None, seed=100):
    """T steps of act(logits=bufs) -> record_policy -> step -> record into a store with dist=True that drops nothing."""
    bufs = tuple(torch.zeros((B * cap, a), dtype=torch.float32, device=DEV) for cap, a in zip((env.pred_capacity, env.prey_capacity), A))
    rows = (T * B * env.pred_capacity, T * B * env.prey_capacity)
    traj = AgentTrajectories(env, T, obs_rows=rows, logp=A, dist=True)
    if store_dtype is not None:
        traj.store = ObservationStore(env, T, rows, dtype=store_dtype, logp=A, dist=True)
    for t in range(T):
        fused.act(env, sample=True, seed=seed + t, logits=bufs)
        traj.record_policy(bufs)
        env.step(env.actions, auto_reset=True)
        traj.record(env.actions)
    torch.cuda.synchronize()
    assert traj.store.cursor[2:].tolist() == [0, 0]
    return traj


@pytest.fixture(scope="module")
def recorded():
    """A recorded store of the default networks on a float64 env, shared by the tests that only need rows: (nets, traj)."""
    nets = [n.to(DEV) for n in make_nets(seed=31)]
    fused = FusedPolicy(nets[0], nets[1])
    traj = record_rollout(make_env(), fused, (9, 9))
    fused.close()
    return nets, traj


# ---- 1. equals act ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env_dtype,store_dtype", [(torch.float64, None), (torch.float32, None), (torch.bfloat16, None), (torch.float64, torch.float32)],
                         ids=["f64", "f32", "bf16", "f32-store-on-f64-env"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_evaluate_over_the_store_equals_what_act_wrote(family, env_dtype, store_dtype, monkeypatch):
    Rp, Rq = FAMILIES[family][:2]
    nets, fused = make_policy(family, 33, monkeypatch)
    traj = record_rollout(make_env(Rp, Rq, obs_dtype=env_dtype), fused, (9, 9), store_dtype)
    st = traj.store
    for s in (0, 1):
        got = fused.evaluate(s, st.obs[s], count=st.cursor[s:s + 1])
        also = traj.logits(fused, s)
        torch.cuda.synchronize()
        n = int(st.cursor[s])
        acted = ~torch.isnan(st.logp[s])
        assert n > 0 and bool(acted[:n].any()) and not bool(acted[n:].any())
        assert tuple(got.shape) == (st.capacity[s], 9) and got.dtype == torch.float32
        assert torch.equal(bits(got[acted]), bits(st.dist[s][acted])), (family, s)
        assert bool((got[acted] != 0).any())
        assert torch.equal(bits(got), bits(also))
        assert float(got[n:].abs().sum()) == 0.0            # (zero-filled by the call, not written behind the count)
    fused.close()


# ---- 2. counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["rllib-default-pipeline", "fc-chain", "chw"])
def test_counts_as_an_int_and_as_a_device_word(family, recorded, monkeypatch):
    _, traj = recorded
    nets, fused = make_policy(family, 35, monkeypatch)
    obs = traj.store.obs[1][:517]
    rows = obs.shape[0]
    full = fused.evaluate(1, obs)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full).all()) and bool((full != 0).any())
    for count in (0, 1, 33, 128, 129, rows, rows + 7):
        clamp = min(count, rows)
        a = torch.full((rows, 9), float("nan"), device=DEV)
        b = a.clone()
        word = torch.full((1,), count, dtype=torch.int64, device=DEV)
        assert fused.evaluate(1, obs, count=count, out=a) is a
        assert fused.evaluate(1, obs, count=word, out=b) is b
        torch.cuda.synchronize()
        for x in (a, b):
            assert bool(torch.isfinite(x[:clamp]).all()) and bool(torch.isnan(x[clamp:]).all()), (family, count)
            assert torch.equal(bits(x[:clamp]), bits(full[:clamp])), (family, count)
    neg = torch.full((rows, 9), float("nan"), device=DEV)
    fused.evaluate(1, obs, count=torch.full((1,), -5, dtype=torch.int64, device=DEV), out=neg)
    fused.evaluate(1, obs, count=-5, out=neg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(neg).all())
    fused.close()


# ---- 3. position independence -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["rllib-default-pipeline", "one-role-direct", "fc-chain", "chw", "deep"])
def test_a_rows_output_does_not_depend_on_its_position(family, recorded, monkeypatch):
    _, traj = recorded
    nets, fused = make_policy(family, 36, monkeypatch)
    for s in (0, 1):
        obs = traj.store.obs[s][:int(traj.store.cursor[s])]
        perm = torch.randperm(obs.shape[0], device=DEV, generator=torch.Generator(DEV).manual_seed(s))
        plain, moved = fused.evaluate(s, obs), fused.evaluate(s, obs[perm].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(bits(moved), bits(plain[perm])), (family, s)
    fused.close()


# ---- 4. a share larger than a tile -------------------------------------------------------------------------------------------------

def test_a_workgroups_share_of_several_tiles(monkeypatch):
    """2 * grid * 128 + 5 rows on the one-role direct-head kernels: every workgroup's share is two tiles and a bit; the rows against an
    evaluation of the same tensor in two halves (other shares, other tiles, other places inside them)."""
    nets, fused = make_policy("chw", 37, monkeypatch)
    sp = fused._spec(nets[1], lambda p: 0)
    d = (ctypes.c_int32 * 12)()
    assert fused._lib.ppg_policy_describe(ctypes.byref(sp), d, 12) == 0 and d[0] == 1       # one-role direct head: one workgroup per CU
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * grid * 128 + 5
    obs = torch.randint(0, 2, (rows, 4, 9, 9), device=DEV, generator=torch.Generator(DEV).manual_seed(9)).to(torch.bfloat16)
    whole = fused.evaluate(1, obs)
    half = rows // 2 + 1
    first, second = fused.evaluate(1, obs[:half]), fused.evaluate(1, obs[half:])
    torch.cuda.synchronize()
    assert torch.equal(bits(whole), bits(torch.cat((first, second))))
    assert bool(torch.isfinite(whole).all()) and bool((whole[-1] != 0).any()) and whole.unique(dim=0).shape[0] > rows // 2
    fused.close()


# ---- 5. critic ---------------------------------------------------------------------------------------------------------------------

def test_a_critic_is_a_network_with_one_action(recorded, monkeypatch):
    _, traj = recorded
    nets, critic = make_policy("rllib-default-pipeline", 38, monkeypatch, n_actions=1)
    st = traj.store
    n = st.cursor[:2].tolist()
    v = traj.values(critic)
    direct = [critic.evaluate(s, st.obs[s], count=st.cursor[s:s + 1]).squeeze(-1) for s in (0, 1)]
    torch.cuda.synchronize()
    for s in (0, 1):
        assert tuple(v[s].shape) == (st.capacity[s],) and v[s].dtype == torch.float32
        with torch.no_grad():
            want = nets[s](st.obs[s][:n[s]]).squeeze(-1)
        err, scale = float((v[s][:n[s]] - want).abs().max()), max(1.0, float(want.abs().max()))
        print(f"critic species {s}: max |dv| {err:.3e} on max |v| {scale:.3e} over {n[s]} samples")
        assert err <= REL_TOL * scale and float(want.abs().max()) > 0.05
        assert torch.equal(bits(v[s]), bits(direct[s]))
    a = traj.targets(v[0][:n[0]], v[1][:n[1]], 0.99, 0.95)
    b = traj.targets(direct[0][:n[0]].clone(), direct[1][:n[1]].clone(), 0.99, 0.95)
    torch.cuda.synchronize()
    for s in (0, 1):
        assert torch.equal(bits(a[0][s]), bits(b[0][s])) and torch.equal(bits(a[1][s]), bits(b[1][s]))
        assert bool((a[0][s] != 0).any())
    assert torch.equal(a[2], b[2])
    # one species alone, and an actor is no critic
    prey_only = FusedPolicy(None, nets[1])
    alone = traj.values(prey_only)
    torch.cuda.synchronize()
    assert alone[0] is None and torch.equal(bits(alone[1]), bits(v[1]))
    actor = FusedPolicy(None, make_nets(seed=1)[1])
    with pytest.raises(ValueError):
        traj.values(actor)
    for f in (critic, prey_only, actor):
        f.close()


# ---- 6. graphs ---------------------------------------------------------------------------------------------------------------------

def test_an_evaluate_moves_nothing_a_captured_act_reads(recorded):
    """GraphedPolicyStep captured first; evaluates of growing capacity (each reallocates evaluate's own plan) between its replays: the
    same states and actions as an eager loop with the same evaluates interleaved, and the evaluations agree too."""
    nets, traj = recorded
    a, b = (make_env(seed=21, obs_dtype=torch.bfloat16) for _ in range(2))
    fa, fb = FusedPolicy(nets[0], nets[1]), FusedPolicy(nets[0], nets[1])
    loop = GraphedPolicyStep(fa, a, seed=1000)     # (its warm pass is step 0)
    fb.act(b, sample=True, seed=1000)
    b.step(b.actions, auto_reset=True)
    obs = traj.store.obs
    for t, rows in enumerate((40, 300, 1500), start=1):
        ea = [fa.evaluate(s, obs[s][:rows]) for s in (0, 1)]
        loop.replay(1)
        eb = [fb.evaluate(s, obs[s][:rows]) for s in (0, 1)]
        fb.act(b, sample=True, seed=1000 + t)
        b.step(b.actions, auto_reset=True)
        torch.cuda.synchronize()
        for x, y in zip(ea, eb):
            assert torch.equal(bits(x), bits(y)) and bool((x != 0).any())
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    fa.close()
    fb.close()


def test_an_evaluate_between_replays_of_a_captured_act_that_has_a_plan(recorded, monkeypatch):
    """The one-launch pipeline form above has no plan buffer; the direct-head kernels do (ppg_policy_plan2 writes it, the forward
    launches read it at the captured address): an act captured first replays to the same logits and actions after evaluates that
    allocate and grow evaluate's buffers."""
    _, traj = recorded
    nets, fused = make_policy("chw", 39, monkeypatch)
    env = make_env(seed=22)
    for _ in range(6):
        env.step(random_actions=True, auto_reset=True)
    bufs = tuple(torch.zeros((B * cap, 9), dtype=torch.float32, device=DEV) for cap in (env.pred_capacity, env.prey_capacity))
    graph = capture_graph(env.device, lambda: fused.act(env, logits=bufs))
    torch.cuda.synchronize()
    want = [x.clone() for x in bufs] + [env.actions.clone()]
    assert bool((want[0] != 0).any()) and bool((want[1] != 0).any())
    for rows in (50, 2000):
        for s in (0, 1):
            fused.evaluate(s, traj.store.obs[s][:rows])
        for x in bufs:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(bufs[0]), bits(want[0])) and torch.equal(bits(bufs[1]), bits(want[1])) and torch.equal(env.actions, want[2])
    fused.close()


def test_a_captured_evaluate_replays_with_the_new_weights_after_an_update(recorded):
    nets, traj = recorded
    other = [n.to(DEV) for n in make_nets(seed=77)]
    st = traj.store
    fused = FusedPolicy(nets[0], nets[1])
    fused.update(nets[0], nets[1])                 # (the one eager update: it allocates the repack maps)
    outs = [torch.full((st.capacity[s], 9), float("nan"), device=DEV) for s in (0, 1)]
    for s in (0, 1):                               # the one eager call per species: it allocates the plan
        fused.evaluate(s, st.obs[s], count=st.cursor[s:s + 1], out=outs[s])

    def body():
        for s in (0, 1):
            fused.evaluate(s, st.obs[s], count=st.cursor[s:s + 1], out=outs[s])
    graph = capture_graph(torch.device(DEV), body)
    torch.cuda.synchronize()
    before = [x.clone() for x in outs]
    fused.update(other[0], other[1])
    graph.replay()
    torch.cuda.synchronize()
    fresh = FusedPolicy(other[0], other[1])
    for s in (0, 1):
        n = int(st.cursor[s])
        want = fresh.evaluate(s, st.obs[s], count=n)
        torch.cuda.synchronize()
        assert torch.equal(bits(outs[s][:n]), bits(want[:n])) and not torch.equal(bits(outs[s][:n]), bits(before[s][:n]))
        assert bool(torch.isnan(outs[s][n:]).all())
    fused.close()
    fresh.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_evaluate_refuses_before_any_launch(recorded):
    nets, traj = recorded
    st = traj.store
    fused = FusedPolicy(None, nets[1])
    obs = st.obs[1][:64]
    out = torch.full((64, 9), float("nan"), device=DEV)
    bad = [
        dict(species=0, obs=st.obs[0][:64]),                               # a species created as None
        dict(species=2, obs=obs),
        dict(species=1, obs=st.obs[0][:64]),                               # the predators' 7 x 7 rows
        dict(species=1, obs=obs[:, :3]),
        dict(species=1, obs=obs.permute(0, 1, 3, 2)),                      # not contiguous
        dict(species=1, obs=obs.to(torch.float16)),
        dict(species=1, obs=obs.cpu()),
        dict(species=1, obs=obs, count=torch.zeros(1, dtype=torch.int32, device=DEV)),
        dict(species=1, obs=obs, count=torch.zeros(2, dtype=torch.int64, device=DEV)),
        dict(species=1, obs=obs, count=torch.zeros(1, dtype=torch.int64)),
        dict(species=1, obs=obs, count=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            fused.evaluate(out=out, **kw)
    for wrong in (out[:63], out.double(), out.cpu(), torch.zeros((64, 8), device=DEV), out.t()):
        with pytest.raises(ValueError):
            fused.evaluate(1, obs, out=wrong)
    # the library's own refusals (behind the Python checks): PPG_EINVAL with a message
    lib, h = fused._lib, fused._handles[1]

    def call(**kw):
        r = _abi.PpgPolicyRows()
        r.obs, r.obs_dtype, r.capacity, r.count, r.out = obs.data_ptr(), 0, 64, 64, out.data_ptr()
        for k, v in kw.items():
            setattr(r, k, v)
        return lib.ppg_policy_evaluate(h, ctypes.byref(r), None)
    for kw, word in ((dict(obs=None), b"obs"), (dict(out=None), b"out"), (dict(obs_dtype=7), b"obs_dtype"), (dict(obs_dtype=-1), b"obs_dtype"),
                     (dict(obs_dtype=3), b"cell layout"), (dict(capacity=-1), b"capacity")):
        assert call(**kw) == -1, kw
        assert word in lib.ppg_policy_last_error(h), kw
    assert lib.ppg_policy_evaluate(None, None, None) == -1 and lib.ppg_policy_evaluate(h, None, None) == -1
    assert call(capacity=0) == 0 and call(count=0) == 0 and call(capacity=0, obs=None, out=None) == 0    # nothing to do: no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    fused.close()
    with pytest.raises(ValueError):
        fused.evaluate(1, obs, out=out)
    with pytest.raises(RuntimeError):
        AgentTrajectories(traj.env, 2).values(fused)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
