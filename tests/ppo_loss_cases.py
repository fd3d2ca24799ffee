"""Scenarios of `ppg_ppo_loss` (PPO's clipped loss and its gradients over one minibatch; include/ppg.h, csrc/ppg_ppo.h),
`env.ppo_loss()`, `AgentTrajectories.ppo_loss()` / `ppo_loss_torch()` / `advantage_norm()` and `trajectory.ppo_loss_function()`, shared by
the wave-emulator tests (test_ppo_loss_emulated.py) and the GPU tests (test_ppo_loss_gpu.py).  No tests of its own.

The reference (`reference`) is plain numpy float64 written from the text of include/ppg.h: validity as a selection, the arithmetic line
by line with the sums over the actions in ascending order, and `partial` in the lane order (lane l of chunk g owns rows
1024 g + 64 j + l, j ascending) followed by the xor butterfly m = 1, 2, 4, 8, 16, 32.  It uses no code of predpreygrass_amd.

Tolerance (`close`).  Both sides do the same IEEE float64 operations in the same order and round once at the store, so they can differ
only where exp() / log() differ, each good to about an ulp of double on each side, and through what that difference is multiplied
with on its way to the output.  The reference therefore carries, next to every output element, the sum of the absolute values of
its addends, each weighted by its first-order sensitivity -- `bound` below:
  - lp_c = d_c - ls has the addends d_c (exact) and ls: bound(lp_c) = |d_c| + |ls|;
  - r = exp(lp_a - logp_old): an absolute difference in the exponent is a relative one in r, so everything r multiplies gets the
    factor 1 + bound(lp_a) + |logp_old| (this is the one constant the issue's formula does not name: without it a surrogate term whose
    log-ratio is far larger than the ratio itself would be held to less than the exponent's own rounding);
  - sums add the bounds of their terms, products multiply a bound by the absolute value of the other factor.
An element passes when |got - ref| <= 1 float32 ulp of ref + 64 * 2^-53 * bound (the ulp: the two float64 results may straddle a
float32 rounding boundary; 64: a few ulps of exp and log on each side, over at most 32 actions' worth of shared sums such as s and H,
which enter every element once and are counted once in the bound).  `partial` is float64 and is not rounded: the float32 ulp is
replaced by 1024 * 2^-53 * bound, the rounding of a chunk's 1024 additions if the two sides' addends differ.  NaN and +-inf must agree
exactly in place.  `partial[:, 0]` (n), `partial[:, 6]` (clipped rows) and every +0.0 of an invalid row are compared bit for bit.

The branch decisions (s2 < s1, vf > vf_clip) are discontinuous, so `reference(..., margins=True)` asserts that no valid row has r
within 1e-6 relative of 1 - clip or 1 + clip, or vf within 1e-6 relative of vf_clip: the seeds below are fixed and satisfy it
(test_ppo_loss_emulated.py checks every scenario's batches on the CPU), and no row is excluded from any comparison."""
import ctypes as C
import itertools

import numpy as np
import torch

from predpreygrass_amd import _abi
from tests import logp_cases
from tests import obs_store_cases as oc
from tests.obs_store_cases import UNSET, random_actions
from tests.record_cases import RECORDED, sync

CHUNK = 1024
EPS = 2.0 ** -53
HYPER = dict(clip=0.3, vf_clip=10.0, vf_coeff=0.5, ent_coeff=0.01, kl_coeff=0.2)
SHAPES_M = (1, 63, 64, 65, 1024, 1025, 2 * 1024 + 7)
SHAPES_A = (1, 2, 9, 25, 32)
INVALID_KINDS = ("k=-1", "k=capacity", "unset", "action=A", "logp nan", "logp -inf")
NAN = float("nan")


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _log_softmax_rows(l):
    """(d, masked, ls, lp, p, bound(lp)) of float64 rows [n,A]: max-shifted, summed in ascending action order."""
    n, A = l.shape
    m = np.full(n, -np.inf)
    for c in range(A):
        m = np.where(l[:, c] > m, l[:, c], m)      # (a NaN is never the maximum)
    d = l - m[:, None]
    masked = d == -np.inf
    e = np.where(masked, 0.0, np.exp(d))
    s = np.zeros(n)
    for c in range(A):
        s = np.where(masked[:, c], s, s + e[:, c])
    ls = np.log(s)
    lp = d - ls[:, None]
    p = e / s[:, None]
    return d, masked, ls, lp, p, np.abs(d) + np.abs(ls)[:, None]


def _chunk_sums(x, valid, M):
    """partial's order: [G] sums of x over the valid rows -- per lane from +0.0 in ascending j, then the xor butterfly."""
    G = (M + CHUNK - 1) // CHUNK
    xs, vs = np.zeros(G * CHUNK), np.zeros(G * CHUNK, bool)
    xs[:M], vs[:M] = x, valid
    xs, vs = xs.reshape(G, CHUNK // 64, 64), vs.reshape(G, CHUNK // 64, 64)
    acc = np.zeros((G, 64))
    for j in range(CHUNK // 64):
        acc = np.where(vs[:, j], acc + xs[:, j], acc)
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[:, lanes ^ m]
    return acc[:, 0]


def reference(b, margins=True):
    """The contract of include/ppg.h on a batch `b` (dict of numpy arrays and hyperparameters, `batch()` below).  Returns a dict:
    grad_logits float32 [M,A], grad_values float32 [M] or None, partial float64 [G,8], the bounds `*_bound` of each (see the module
    docstring), `valid` [M], and the per-row float64 `r`, `kl`, `clipped`."""
    logits, A = b["logits"], b["logits"].shape[1]
    M, cap = logits.shape[0], b["action"].shape[0]
    k = np.arange(M, dtype=np.int64) if b["index"] is None else b["index"].astype(np.int64)
    inside = (k >= 0) & (k < cap)
    ks = np.where(inside, k, 0)
    if cap == 0:
        act, lp_old = np.full(M, -1), np.full(M, np.nan)
    else:
        act, lp_old = b["action"][ks].astype(np.int64), b["logp"][ks].astype(np.float64)
    valid = inside & (act >= 0) & (act < A) & np.isfinite(lp_old)
    V = np.flatnonzero(valid)
    nv = len(V)
    G = (M + CHUNK - 1) // CHUNK
    has_v, has_kl = b["values"] is not None, b["dist"] is not None
    g, g_bound = np.zeros((M, A)), np.zeros((M, A))
    gv, gv_bound = np.zeros(M), np.zeros(M)
    cols = np.zeros((M, 8))
    cols_bound = np.zeros((M, 8))
    out = {"valid": valid, "r": np.full(M, np.nan), "kl": np.zeros(M), "clipped": np.zeros(M, bool)}
    with np.errstate(all="ignore"):
        n = float(nv)
        w = 1.0 / n if n > 0 else 0.0
        if nv:
            kv, a = ks[V], act[V]
            rows = np.arange(nv)
            d, masked, ls, lp, p, lp_b = _log_softmax_rows(logits[V].astype(np.float64))
            hsum, h_b = np.zeros(nv), np.zeros(nv)
            for c in range(A):
                t = p[:, c] * lp[:, c]
                hsum = np.where(masked[:, c], hsum, hsum + t)
                h_b = np.where(masked[:, c], h_b, h_b + p[:, c] * lp_b[:, c])
            H = 0.0 - hsum
            kl, kl_b = np.zeros(nv), np.zeros(nv)
            if has_kl:
                _, _, _, lq, q, lq_b = _log_softmax_rows(b["dist"][kv].astype(np.float64))
                for c in range(A):
                    t = q[:, c] * (lq[:, c] - lp[:, c])
                    kl = np.where(q[:, c] != 0.0, kl + t, kl)
                    kl_b = np.where(q[:, c] != 0.0, kl_b + q[:, c] * (lq_b[:, c] + lp_b[:, c]), kl_b)
            lp_a = lp[rows, a]
            old = lp_old[V]
            r = np.exp(lp_a - old)
            r_factor = 1.0 + lp_b[rows, a] + np.abs(old)
            adv = b["advantage"][kv].astype(np.float64)
            if b["adv_norm"] is not None:
                adv = (adv - b["adv_norm"][0]) * b["adv_norm"][1]
            lo, hi = 1.0 - b["clip"], 1.0 + b["clip"]
            rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
            s1, s2 = adv * r, adv * rc
            clipped = s2 < s1
            surr = np.where(clipped, s2, s1)
            c1 = np.where(clipped, 0.0, s1)
            if margins:
                near = np.isfinite(r) & ((np.abs(r - lo) <= 1e-6 * lo) | (np.abs(r - hi) <= 1e-6 * hi))
                assert not near.any(), ("a ratio sits on a clip boundary", r[near][:3])
            if has_v:
                e = b["values"][V].astype(np.float64) - b["value_target"][kv].astype(np.float64)
                vf = e * e
                over = vf > b["vf_clip"]
                if margins:
                    near = np.isfinite(vf) & (np.abs(vf - b["vf_clip"]) <= 1e-6 * b["vf_clip"])
                    assert not near.any(), ("a squared error sits on vf_clip", vf[near][:3])
                vfc = np.where(over, b["vf_clip"], vf)
                gv[V] = w * (b["vf_coeff"] * np.where(over, 0.0, e + e))
                gv_bound[V] = np.abs(gv[V])
                cols[V, 2], cols[V, 3] = vfc, vf
                cols_bound[V, 2], cols_bound[V, 3] = np.abs(vfc), np.abs(vf)
            for c in range(A):
                delta = (a == c).astype(np.float64)
                y = b["ent_coeff"] * (p[:, c] * (lp[:, c] + H)) - c1 * (delta - p[:, c])
                yb = abs(b["ent_coeff"]) * p[:, c] * (lp_b[:, c] + h_b) + np.abs(c1) * r_factor * (delta + p[:, c])
                if has_kl:
                    y = y + b["kl_coeff"] * (p[:, c] - q[:, c])
                    yb = yb + abs(b["kl_coeff"]) * (p[:, c] + q[:, c])
                g[V, c] = np.where(masked[:, c], 0.0, w * y)
                g_bound[V, c] = np.where(masked[:, c], 0.0, w * yb)
            cols[V, 1], cols_bound[V, 1] = surr, np.abs(surr) * r_factor
            cols[V, 4], cols_bound[V, 4] = H, h_b
            cols[V, 5], cols_bound[V, 5] = kl, kl_b
            cols[V, 6] = clipped
            cols[V, 7], cols_bound[V, 7] = old - lp_a, np.abs(old) + lp_b[rows, a]
            out["r"][V], out["kl"][V], out["clipped"][V] = r, kl, clipped
        cols[:, 0] = 1.0
        partial = np.stack([_chunk_sums(cols[:, c], valid, M) for c in range(8)], axis=1)
        bound = np.stack([_chunk_sums(np.where(np.isfinite(cols_bound[:, c]), cols_bound[:, c], 0.0), valid, M) for c in range(8)], axis=1)
        assert partial.shape == (G, 8) and partial[:, 0].sum() == n
        out.update(grad_logits=g.astype(np.float32), grad_logits_bound=g_bound,
                   grad_values=gv.astype(np.float32) if has_v else None, grad_values_bound=gv_bound,
                   partial=partial, partial_bound=bound)
    return out


def close(got, want, bound, tag, f32=True):
    """|got - want| <= (1 float32 ulp of want, or 1024 * 2^-53 * bound for the float64 `partial`) + 64 * 2^-53 * bound; NaN and +-inf
    in exactly the same places."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN in other places", np.argwhere(np.isnan(got) != nan)[:5].tolist())
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (tag, "+-inf differ")
    fin = ~nan & ~inf
    with np.errstate(all="ignore"):
        first = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) if f32 else 1024 * EPS * bound
        tol = first + 64 * EPS * np.where(np.isfinite(bound), bound, 0.0)
    bad = fin & (np.abs(np.where(fin, got - want, 0.0)) > tol)
    assert not bad.any(), (tag, int(bad.sum()), "of", bad.size, "outside the tolerance; first:", got[bad][:3], want[bad][:3], tol[bad][:3])


def same_bits(got, want, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert np.array_equal(got.view(u), want.view(u)), (tag, "differs bit for bit", np.argwhere(got.view(u) != want.view(u))[:3].tolist())


def check(got, ref, tag):
    """(grad_logits, grad_values, partial) as numpy against reference()'s dict."""
    gl, gv, partial = got
    invalid = ~ref["valid"]
    same_bits(gl[invalid], np.zeros_like(gl[invalid]), f"{tag}: gradient rows of invalid samples")
    close(gl, ref["grad_logits"], ref["grad_logits_bound"], f"{tag}: grad_logits")
    if ref["grad_values"] is None:
        assert gv is None, tag
    else:
        same_bits(gv[invalid], np.zeros_like(gv[invalid]), f"{tag}: value gradients of invalid samples")
        close(gv, ref["grad_values"], ref["grad_values_bound"], f"{tag}: grad_values")
    same_bits(partial[:, 0], ref["partial"][:, 0], f"{tag}: n")
    same_bits(partial[:, 6], ref["partial"][:, 6], f"{tag}: clipped rows")
    close(partial, ref["partial"], ref["partial_bound"], f"{tag}: partial", f32=False)


# ---- batches ------------------------------------------------------------------------------------------------------------------

def _logp_of(dist, action):
    """float32 log-softmax of float32 rows at the actions, float64 rounded once: what ppg_record_logp stores."""
    l = dist.astype(np.float64)
    d = l - l.max(axis=1, keepdims=True)
    return (d[np.arange(len(l)), action] - np.log(np.exp(d).sum(axis=1))).astype(np.float32)


def batch(seed, M, A, index="perm", values=True, dist=True, adv_norm=True, invalid=(), spread=0.3, hyper=HYPER, poison=NAN, scale=1.5):
    """A minibatch of M rows over store columns of M + 8 slots (index None: M slots).  The new logits are the old ones plus
    `spread` * noise, so that the ratios fall below, inside and above [1 - clip, 1 + clip]; the values are the targets plus noise of
    two sizes, so that vf falls on both sides of vf_clip.  index: None, "perm" or "repeats".  invalid: the kinds of INVALID_KINDS to
    mix in (each into about a twelfth of the rows, at least one); their logits rows, and the advantage, target and dist of the slots
    that are invalid by their columns, are filled with `poison`."""
    rng = np.random.default_rng(seed)
    cap = M if index is None else M + 8
    old = (rng.standard_normal((cap, A)) * scale).astype(np.float32)
    action = rng.integers(0, A, cap).astype(np.int8)
    logp = _logp_of(old, action)
    advantage = rng.standard_normal(cap).astype(np.float32)
    mean, std = float(advantage.mean()), float(advantage.std())
    target = (rng.standard_normal(cap) * 2).astype(np.float32)
    if index is None:
        idx = None
        k = np.arange(M)
    else:
        k = rng.permutation(M) if index == "perm" else rng.integers(0, M, M)
        idx = k.astype(np.int32)
    logits = (old[k] + spread * rng.standard_normal((M, A))).astype(np.float32)
    vals = (target[k] + rng.standard_normal(M) * np.where(rng.random(M) < 0.5, 0.7, 5.0)).astype(np.float32)
    bad_slot = {"unset": M, "action=A": M + 1, "logp nan": M + 2, "logp -inf": M + 3}
    kinds = [x for x in invalid if idx is not None or x in bad_slot]
    if kinds:
        rows = rng.permutation(M)[:max(len(kinds), M // 12 * len(kinds))] if M >= len(kinds) else np.arange(M)
        for q, i in enumerate(rows):
            kind = kinds[q % len(kinds)]
            slot = i if idx is None else bad_slot.get(kind)
            if kind == "k=-1":
                idx[i] = (-1, -(2 ** 31), -7)[q % 3]
            elif kind == "k=capacity":
                idx[i] = (cap, cap + 3, 2 ** 31 - 1)[q % 3]
            else:
                if idx is not None:
                    idx[i] = slot
                if kind == "unset":
                    action[slot] = UNSET
                elif kind == "action=A":
                    action[slot] = (A, -1, 127)[q % 3]
                elif kind == "logp nan":
                    logp[slot] = np.nan
                else:
                    logp[slot] = (-np.inf, np.inf)[q % 2]
                advantage[slot] = target[slot] = old[slot] = poison
            logits[i] = poison
            vals[i] = poison
    return dict(logits=logits, index=idx, values=vals if values else None, action=action, logp=logp, dist=old if dist else None,
                advantage=advantage, value_target=target if values else None,
                adv_norm=np.array([mean, 1.0 / (std + 1e-8)]) if adv_norm else None,
                **{**hyper, **({} if dist else {"kl_coeff": 0.0})})


TENSORS = ("logits", "index", "values", "action", "logp", "dist", "advantage", "value_target", "adv_norm")


def on_device(env, b):
    return {name: None if b[name] is None else torch.from_numpy(b[name].copy()).to(env.device) for name in TENSORS}


def run(env, b, dev=None):
    """env.ppo_loss() on a batch; the outputs as numpy.  No input may change."""
    dev = on_device(env, b) if dev is None else dev
    gl, gv, partial = env.ppo_loss(dev["logits"], dev["action"], dev["logp"], dev["advantage"], index=dev["index"], values=dev["values"],
                                   value_target=dev["value_target"], dist=dev["dist"], adv_norm=dev["adv_norm"],
                                   **{h: b[h] for h in HYPER})
    sync(env)
    M, A = b["logits"].shape
    assert gl.shape == (M, A) and gl.dtype == torch.float32 and partial.shape == ((M + CHUNK - 1) // CHUNK, 8) and partial.dtype == torch.float64
    assert (gv is None) == (b["values"] is None) and (gv is None or (gv.shape == (M,) and gv.dtype == torch.float32))
    for name in TENSORS:
        if b[name] is not None:
            same_bits(dev[name].cpu().numpy(), b[name], f"input {name} was written")
    return gl.cpu().numpy(), None if gv is None else gv.cpu().numpy(), partial.cpu().numpy()


# ---- 1. shapes and options ----------------------------------------------------------------------------------------------------

SHAPE_CASES = [(M, A, index, values, dist, norm)
               for q, ((M, A), (index, values, dist, norm)) in enumerate(zip(
                   itertools.product(SHAPES_M, SHAPES_A),
                   itertools.cycle(itertools.product((None, "perm", "repeats"), (True, False), (True, False), (True, False)))))]


def shape_batches(M):
    """The batches of `shapes(env, M)`: every A, the options dealt out over the (M, A) pairs so that each option value meets each M."""
    return [(f"M={M} A={A} index={index} values={values} dist={dist} adv_norm={norm}",
             batch(1000 + 37 * M + A, M, A, index=index, values=values, dist=dist, adv_norm=norm, invalid=INVALID_KINDS if M > 1 else ()))
            for (m, A, index, values, dist, norm) in SHAPE_CASES if m == M]


def shapes(env, M):
    for tag, b in shape_batches(M):
        ref = reference(b)
        if M > 1:
            assert ref["valid"].any() and (~ref["valid"]).any(), tag
        check(run(env, b), ref, tag)


def large_batch(M=300 * 1024, A=9):
    return batch(79, M, A, index="perm", invalid=INVALID_KINDS)


def large(env, M=300 * 1024, A=9):
    """Hundreds of workgroups read every count."""
    b = large_batch(M, A)
    ref = reference(b)
    assert ref["partial"].shape[0] == 300
    check(run(env, b), ref, f"M={M}")


# ---- 2. invalid samples ----------------------------------------------------------------------------------------------------------

def invalid_samples(env, M=1024 + 300, A=9):
    """Each kind mixed into a batch, poisoned with NaN: against the reference; against the same batch poisoned with finite numbers,
    bit for bit (nothing of an invalid row is read); and appended behind a batch of valid rows, whose sums, n and gradient rows must
    not change by a bit.  An all-invalid batch: n = 0, every gradient +0.0, every sum +0.0."""
    for index in ("perm", None):
        kinds = [x for x in INVALID_KINDS if index is not None or not x.startswith("k=")]
        for kind in kinds + [tuple(kinds)]:
            kw = dict(index=index, invalid=(kind,) if isinstance(kind, str) else kind)
            b, twin = batch(5, M, A, **kw), batch(5, M, A, poison=0.25, **kw)
            ref = reference(b)
            n_bad = int((~ref["valid"]).sum())
            assert 0 < n_bad < M, (kind, n_bad)
            got = run(env, b)
            check(got, ref, f"invalid {kind} index={index}")
            for x, y, name in zip(got, run(env, twin), ("grad_logits", "grad_values", "partial")):
                same_bits(x, y, f"invalid {kind}: {name} depends on what an invalid row holds")
    base = batch(6, 1024 + 64, A, index="perm")            # (a multiple of 64: appended rows start a new j in every lane)
    want = run(env, base)
    assert reference(base)["valid"].all()
    more = {**base}
    extra = 1024 + 5                                       # (one more chunk, whose sums are all +0.0)
    cap = base["action"].shape[0]
    more["index"] = np.concatenate([base["index"], np.resize(np.array([-1, cap, cap + 9, -5], np.int32), extra)])
    more["logits"] = np.concatenate([base["logits"], np.full((extra, A), np.nan, np.float32)])
    more["values"] = np.concatenate([base["values"], np.full(extra, np.nan, np.float32)])
    got = run(env, more)
    M0, G0 = base["logits"].shape[0], want[2].shape[0]
    same_bits(got[0][:M0], want[0], "appended invalid rows changed a gradient row")
    same_bits(got[1][:M0], want[1], "appended invalid rows changed a value gradient")
    same_bits(got[2][:G0], want[2], "appended invalid rows changed a sum")
    for x in (got[0][M0:], got[1][M0:], got[2][G0:]):
        same_bits(x, np.zeros_like(x), "appended invalid rows are not +0.0")
    nothing = batch(7, 65, A, index="perm")
    nothing["logp"][:] = np.nan
    nothing["logits"][:] = np.nan
    got = run(env, nothing)
    for x in got:
        same_bits(x, np.zeros_like(x), "an all-invalid batch is not all +0.0")
    check(got, reference(nothing), "all invalid")


# ---- 3. clip branches, masked actions, divergence -----------------------------------------------------------------------------------

def clip_branches(env, A=5):
    """Every combination of sign(Ad) in {-, 0, +} with r below, inside and above the clip range, and vf below and above vf_clip: one
    row each, built by hand; then a -inf new logit (masked: p = 0, gradient +0.0), a -inf old logit, a -inf new logit where the old
    policy had mass (KL = +inf), a NaN logit and a +inf logit in a valid row (NaN out, not masked)."""
    combos = list(itertools.product((-1.5, 0.0, 2.0), (0.5, 1.1, 1.6), (1.0, 5.0)))
    extra = ["-inf new", "-inf old", "-inf new only", "nan", "+inf"]
    M = len(combos) + len(extra)
    rng = np.random.default_rng(3)
    old = (rng.standard_normal((M, A)) * 1.2).astype(np.float32)
    action = rng.integers(0, A, M).astype(np.int8)
    action[len(combos):] = 0
    logits = old.copy()
    advantage, target, vals = np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.float32)
    logp = _logp_of(old, action)
    for i, (adv, ratio, err) in enumerate(combos):
        advantage[i] = adv
        logp[i] = np.float32(float(logp[i]) - np.log(ratio))     # new logits = old ones: r = exp(lp_a - logp) ~ ratio
        target[i], vals[i] = 0.5, 0.5 + err                      # vf = 1 or 25 against vf_clip = 10
    e = len(combos)
    advantage[e:] = 1.0
    logits[e, 2] = old[e, 2] = -np.inf           # masked in both
    old[e + 1, 3] = -np.inf                      # masked in the old policy only: q = 0, its term is skipped
    logits[e + 2, 1] = -np.inf                   # masked in the new policy only: KL = +inf
    logits[e + 3, 4] = np.nan
    logits[e + 4, 4] = np.inf
    b = dict(logits=logits, index=None, values=vals, action=action, logp=logp, dist=old, advantage=advantage, value_target=target,
             adv_norm=None, **HYPER)
    ref = reference(b)
    assert ref["valid"].all()
    lo, hi = 1 - HYPER["clip"], 1 + HYPER["clip"]
    seen = {(np.sign(adv), "below" if r < lo else "above" if r > hi else "inside", bool(c)) for (adv, _, _), r, c in
            zip(combos, ref["r"], ref["clipped"])}
    assert len({x[:2] for x in seen}) == 9 and {(1.0, "above", True), (-1.0, "below", True), (1.0, "below", False), (0.0, "above", False)} <= seen
    got = run(env, b)
    check(got, ref, "clip branches")
    gl, gv, partial = got
    same_bits(gl[e, 2:3], np.zeros(1, np.float32), "the gradient of a masked action")
    assert np.isfinite(gl[e]).all() and np.isfinite(gl[e + 1]).all() and gl[e + 2, 1] == 0.0 and np.signbit(gl[e + 2, 1]) == False  # noqa: E712
    assert ref["kl"][e + 2] == np.inf and np.isfinite(ref["kl"][e + 1]) and np.isnan(gl[e + 3]).all()
    assert np.isnan(gl[e + 4, 4]) and not gl[e + 4, :4].any()       # (+inf: the other actions are -inf below the maximum, masked)
    assert np.isnan(partial[0, 1]) and (gv[:e][[c[2] > 3 for c in combos]] == 0).all() and (gv[:e][[c[2] < 3 for c in combos]] != 0).all()


def exact_identity(env, M=1024 + 77, A=9):
    """New logits equal to dist[k] bit for bit: KL is exactly 0 for every row, no row is clipped, and |r - 1| <= 2^-23 -- logp[k] is
    the float32 rounding of the float64 log-probability the kernel forms again, and the logits here are small enough (scale 0.5)
    that every |logp| is below 4, where half a float32 ulp is at most 2^-23.  The kernel does not return r: its column 7, the sum
    of logp_old - lp_a over a chunk's rows, is held to the chunk's row count times that."""
    b = batch(9, M, A, index="perm", spread=0.0, scale=0.5)
    assert np.array_equal(b["logits"], b["dist"][b["index"]]) and (np.abs(b["logp"]) < 4.0).all()
    ref = reference(b)
    assert ref["valid"].all()
    assert (ref["kl"] == 0.0).all() and not ref["clipped"].any() and (np.abs(ref["r"] - 1.0) <= 2.0 ** -23).all()
    got = run(env, b)
    check(got, ref, "identity")
    assert (np.abs(got[2][:, 7]) <= got[2][:, 0] * 2.0 ** -23).all()
    same_bits(got[2][:, 5], np.zeros(got[2].shape[0]), "KL of identical logits")
    same_bits(got[2][:, 6], np.zeros(got[2].shape[0]), "clip fraction of identical logits")
    # without advantage, entropy and value terms the gradient is kl_coeff * (p - q) = exactly 0
    flat = {**b, "advantage": np.zeros_like(b["advantage"]), "adv_norm": None, "ent_coeff": 0.0, "values": None, "value_target": None}
    gl, _, _ = run(env, flat)
    assert (gl == 0.0).all()


# ---- 4. untouched memory, refused calls -------------------------------------------------------------------------------------------

GUARD, FILL = 64, 0x5A


def guarded(env, shape, dtype):
    """(view of exactly `shape`, the whole buffer): GUARD elements of 0x5A bytes on both sides."""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * GUARD) * size,), FILL, dtype=torch.uint8, device=env.device)
    return raw[GUARD * size:(GUARD + n) * size].view(dtype).view(shape), raw


def raw_call(env, dev, hyper, M, A, capacity, outs, null=(), mb=True):
    s = _abi.PpgPpoBatch()
    s.M, s.A, s.capacity = M, A, capacity
    for name in TENSORS:
        setattr(s, name, None if name in null or dev[name] is None else dev[name].data_ptr())
    for h in HYPER:
        setattr(s, h, hyper[h])
    ptr = lambda name: None if name in null or outs[name] is None else C.c_void_p(outs[name].data_ptr())
    return env._lib.ppg_ppo_loss(env._handle, C.byref(s) if mb else None, ptr("grad_logits"), ptr("grad_values"), ptr("partial"), env._stream())


def untouched(env, other_device, M=1024 + 9, A=9):
    """The raw call into outputs of exactly their size between guard elements; every refused call -- each PPG_EINVAL of include/ppg.h
    and each ValueError of the wrappers -- returns -1 with "ppg_ppo_loss:" in ppg_last_error and writes nothing."""
    import pytest
    b = batch(11, M, A, index="perm", invalid=INVALID_KINDS)
    dev = on_device(env, b)
    cap = b["action"].shape[0]
    G = (M + CHUNK - 1) // CHUNK
    views, whole = {}, {}
    for name, shape, dtype in (("grad_logits", (M, A), torch.float32), ("grad_values", (M,), torch.float32), ("partial", (G, 8), torch.float64)):
        views[name], whole[name] = guarded(env, shape, dtype)
    before = {k: v.cpu().numpy().copy() for k, v in whole.items()}
    refused = [dict(mb=False), dict(null=("logits",)), dict(null=("action",)), dict(null=("logp",)), dict(null=("advantage",)),
               dict(null=("grad_logits",)), dict(null=("partial",)), dict(M=0), dict(M=-4), dict(M=2 ** 31), dict(A=0), dict(A=33), dict(A=-1),
               dict(capacity=-1), dict(capacity=2 ** 31), dict(null=("values",)), dict(null=("value_target",)),
               dict(null=("values", "value_target")), dict(null=("dist",)), dict(clip=-0.1), dict(clip=NAN), dict(clip=float("inf")),
               dict(vf_clip=-1.0), dict(vf_clip=NAN), dict(vf_clip=float("inf"))]
    for kw in refused:
        hyper = {**b, **{k: v for k, v in kw.items() if k in HYPER}}
        rc = raw_call(env, dev, hyper, kw.get("M", M), kw.get("A", A), kw.get("capacity", cap), views, null=kw.get("null", ()), mb=kw.get("mb", True))
        assert rc == -1, kw
        assert env._lib.ppg_last_error(env._handle).startswith(b"ppg_ppo_loss:"), (kw, env._lib.ppg_last_error(env._handle))
    sync(env)
    for k, v in whole.items():
        assert np.array_equal(v.cpu().numpy(), before[k]), (k, "a refused call wrote")
    assert raw_call(env, dev, b, M, A, cap, views) == 0
    sync(env)
    ref = reference(b)
    check(tuple(views[k].cpu().numpy() for k in ("grad_logits", "grad_values", "partial")), ref, "raw call")
    for k, v in whole.items():
        raw, size = v.cpu().numpy(), views[k].element_size()
        assert (raw[:GUARD * size] == FILL).all() and (raw[-GUARD * size:] == FILL).all(), (k, "a guard element was written")
    for name in TENSORS:
        same_bits(dev[name].cpu().numpy(), b[name], f"input {name} was written")
    # (accepted: no values and no grad_values; values without grad_values; no dist with kl_coeff 0; capacity 0)
    none = {**views, "grad_values": None}
    assert raw_call(env, dev, b, M, A, cap, none, null=("values", "value_target")) == 0
    assert raw_call(env, dev, b, M, A, cap, none) == 0
    assert raw_call(env, dev, {**b, "kl_coeff": 0.0}, M, A, cap, views, null=("dist",)) == 0
    assert raw_call(env, dev, b, M, A, 0, views) == 0
    sync(env)
    assert float(views["partial"][:, 0].sum()) == 0.0 and not bool(views["grad_logits"].any())

    def call(**kw):
        a = {**dev, **kw}
        return env.ppo_loss(a["logits"], a["action"], a["logp"], a["advantage"], index=a["index"], values=a["values"],
                            value_target=a["value_target"], dist=a["dist"], adv_norm=a["adv_norm"],
                            **{h: kw.get(h, b[h]) for h in HYPER})
    with pytest.raises(ValueError, match="dtype=torch.int32"):
        call(index=dev["index"].long())
    wrong = [dict(logits=dev["logits"].double()), dict(logits=dev["logits"][:, :0]), dict(logits=dev["logits"].reshape(-1)),
             dict(logits=dev["logits"].t().contiguous().t()), dict(logits=dev["logits"].to(other_device)), dict(index=dev["index"][:-1]),
             dict(values=dev["values"][:-1]), dict(values=dev["values"].double()), dict(values=None), dict(value_target=None),
             dict(action=dev["action"].to(torch.int32)), dict(action=dev["action"].reshape(-1, 1)), dict(logp=dev["logp"][:-1]),
             dict(logp=dev["logp"].double()), dict(dist=dev["dist"][:, :-1].contiguous()), dict(dist=dev["dist"][:-1]),
             dict(dist=None), dict(advantage=dev["advantage"][:-1]), dict(advantage=dev["advantage"].double()),
             dict(value_target=dev["value_target"][:-1]), dict(adv_norm=dev["adv_norm"].float()), dict(adv_norm=dev["adv_norm"][:1]),
             dict(clip=-1.0), dict(vf_clip=NAN)]
    for kw in wrong:
        with pytest.raises(ValueError):
            call(**kw)
    sync(env)
    for k, v in whole.items():
        raw, size = v.cpu().numpy(), views[k].element_size()
        assert (raw[:GUARD * size] == FILL).all() and (raw[-GUARD * size:] == FILL).all(), (k, "a guard element was written")


# ---- 5. the recorded path: record_obs -> record_logp -> targets -> advantage_norm -> traj.ppo_loss ---------------------------------

def recorded(env, name, T=8):
    """A short rollout with synthetic logits (logp_cases.synthetic) through AgentTrajectories, then one minibatch per species over a
    shuffled int32 permutation of ALL its slots -- the last step's samples, whose action and logp are still unset, included --
    against the reference fed the store's columns; the loss and the stats against their composition from the reference's sums; the
    spelled-out torch loss in float64 with .backward() against the kernel's gradients; ppo_loss_function() under a grad_output of
    -2.5 against that multiple."""
    import pytest
    from predpreygrass_amd.trajectory import AgentTrajectories, ppo_loss_function
    A, B = logp_cases.ROLLOUT_ACTIONS[name], env.batch_size
    env.reset()
    traj = AgentTrajectories(env, T, obs_rows=tuple(T * B * r for r in oc.BUDGET[name]), logp=A, dist=True)
    gen, gen2 = torch.Generator().manual_seed(21), torch.Generator().manual_seed(22)
    for t in range(T):
        logits, acts = logp_cases.synthetic(env, gen2, A, scale=1.5)
        traj.record_policy(logits, acts)
        actions = acts if name == "gen2" else random_actions(env, gen)
        env.step(actions, auto_reset=True)
        traj.record(actions)
    sync(env)
    counts = traj.store.cursor[:2].tolist()
    v = [torch.randn((n,), generator=gen2).to(env.device) for n in counts]
    adv, ret, moments = traj.targets(v[0], v[1], 0.99, 0.95)
    norm = traj.advantage_norm(moments)
    assert norm.shape == (2, 2) and norm.dtype == torch.float64
    count, mean, std = (x.cpu().numpy() for x in traj.advantage_moments(moments))
    same_bits(norm.cpu().numpy(), np.stack((mean, 1.0 / (std + 1e-8)), axis=1), "advantage_norm")
    hyper = dict(HYPER)
    for s in (0, 1):
        n = counts[s]
        assert n > 64
        st = traj.store
        index = torch.randperm(n, generator=gen2).to(torch.int32).to(env.device)
        new = (st.dist[s][:n][index.long()].cpu() + 0.3 * torch.randn((n, A[s]), generator=gen2)).to(env.device)
        values = (ret[s][index.long()].cpu() + torch.randn((n,), generator=gen2)).to(env.device)
        loss, stats, gl, gv = traj.ppo_loss(s, new, values, index, adv[s], ret[s], adv_norm=norm, **hyper)
        sync(env)
        b = dict(logits=new.cpu().numpy(), index=index.cpu().numpy(), values=values.cpu().numpy(), action=st.action[s][:n].cpu().numpy(),
                 logp=st.logp[s][:n].cpu().numpy(), dist=st.dist[s][:n].cpu().numpy(), advantage=adv[s].cpu().numpy(),
                 value_target=ret[s].cpu().numpy(), adv_norm=norm[s].cpu().numpy(), **hyper)
        ref = reference(b)
        n_valid = int(ref["valid"].sum())
        assert 0 < n_valid < n, (name, s, n_valid, n, "the last step's samples must be invalid, the others valid")
        assert (b["action"][~ref["valid"][np.argsort(b["index"])]] == UNSET).any() or np.isnan(b["logp"]).any()
        total, bound = ref["partial"].sum(0), ref["partial_bound"].sum(0)
        means = total[1:] / n_valid
        want = dict(zip(AgentTrajectories._PPO_STATS, (float(n_valid), -means[0], *means[1:])))
        assert set(stats) == set(want) and all(x.dim() == 0 and x.device == new.device for x in stats.values())
        assert float(stats["n"]) == n_valid and float(stats["clip_fraction"]) == want["clip_fraction"] and 0 < want["clip_fraction"] < 1
        for c, key in enumerate(AgentTrajectories._PPO_STATS[1:]):
            close(abs(float(stats[key])), abs(want[key]), bound[c + 1] / n_valid, f"{name} species {s} {key}", f32=False)
        want_loss = want["policy_loss"] + hyper["vf_coeff"] * want["vf_loss"] - hyper["ent_coeff"] * want["entropy"] + hyper["kl_coeff"] * want["kl"]
        loss_bound = (bound[1] + hyper["vf_coeff"] * bound[2] + hyper["ent_coeff"] * bound[4] + hyper["kl_coeff"] * bound[5]) / n_valid
        close(float(loss), want_loss, loss_bound, f"{name} species {s} loss", f32=False)
        # (grad_logits / grad_values through env.ppo_loss's own outputs: the raw tuple has partial where traj has loss and stats)
        check((gl.cpu().numpy(), gv.cpu().numpy(), ref["partial"]), ref, f"{name} species {s}")
        # the spelled-out torch loss, float64, through autograd
        x, y = new.clone().requires_grad_(True), values.clone().requires_grad_(True)
        tl, tstats = traj.ppo_loss_torch(s, x, y, index, adv[s], ret[s], adv_norm=norm, dtype=torch.float64, **hyper)
        tl.backward()
        close(float(tl.detach()), want_loss, loss_bound, f"{name} species {s} torch loss", f32=False)
        assert float(tstats["n"]) == n_valid
        close(x.grad.cpu().numpy(), ref["grad_logits"], ref["grad_logits_bound"], f"{name} species {s}: autograd grad_logits")
        close(y.grad.cpu().numpy(), ref["grad_values"], ref["grad_values_bound"], f"{name} species {s}: autograd grad_values")
        # loss.backward() through the Function, under a grad_output that is not 1
        x, y = new.clone().requires_grad_(True), values.clone().requires_grad_(True)
        fl, fstats = ppo_loss_function(traj, s, x, y, index, adv[s], ret[s], adv_norm=norm, **hyper)
        (fl * -2.5).backward()
        same_bits(np.float64(float(fl.detach())), np.float64(float(loss)), "ppo_loss_function's loss")
        same_bits(x.grad.cpu().numpy(), (gl * -2.5).cpu().numpy(), "ppo_loss_function: grad_logits * grad_output")
        same_bits(y.grad.cpu().numpy(), (gv * -2.5).cpu().numpy(), "ppo_loss_function: grad_values * grad_output")
        assert set(fstats) == set(stats)
        # the zero-overhead backward: the gradients as they are
        x, y = new.clone().requires_grad_(True), values.clone().requires_grad_(True)
        x2, y2 = x * 1.0, y * 1.0
        torch.autograd.backward([x2, y2], [gl, gv])
        same_bits(x.grad.cpu().numpy(), gl.cpu().numpy(), "autograd.backward of the returned gradients")
        with pytest.raises(ValueError, match="dtype=torch.int32"):
            traj.ppo_loss(s, new, values, index.long(), adv[s], ret[s])
        with pytest.raises(ValueError):
            traj.ppo_loss(s, new, None, index, adv[s], ret[s])
        with pytest.raises(ValueError):
            traj.ppo_loss(s, new, values, index, adv[s], ret[s], adv_norm=norm.float())
    plain = AgentTrajectories(env, T, obs_rows=(64, 64), logp=A)          # a store without dist
    with pytest.raises(ValueError):
        plain.ppo_loss(0, new[:8], None, None, adv[0][:8], None, kl_coeff=0.2)
    with pytest.raises(RuntimeError):
        AgentTrajectories(env, T, obs_rows=(64, 64)).ppo_loss(0, new[:8], None, None, adv[0][:8], None, kl_coeff=0.0)


def margins_hold():
    """Every fixed-seed batch of the scenarios keeps its branch decisions clear of the boundaries (reference() asserts it)."""
    for M in SHAPES_M:
        for _, b in shape_batches(M):
            reference(b)
    reference(batch(5, 1024 + 300, 9, index="perm", invalid=INVALID_KINDS))
    reference(batch(6, 1024 + 64, 9, index="perm"))
    reference(batch(11, 1024 + 9, 9, index="perm", invalid=INVALID_KINDS))
    reference(large_batch())
