"""The plan of ppg_policy_evaluate, checked without a GPU: `ppg_policy_rows_plan` (the words the kernel ppg_policy_plan_rows writes,
made by the same inline functions of csrc/ppg_policy_plan.h on the CPU) against a numpy restatement of `plan_body`
(csrc/ppg_policy.h: the plan kernel of ppg_policy_act -- per-thread runs of envs, a scan over 1024 partial sums, a two-level bisection
per tile) fed the row counts of the pseudo-envs a dense row tensor is read as: clamp(count - e * CH, 0, CH).

The restatement is the reference; it follows plan_body as it is written, not the new inlines.  On top of word equality every tile is
walked the way the forward kernels do (phase_conv: start at tile_env[tile], step forward while the next prefix sum is <= n; the
direct-head kernels: bisect between tile_env[tile] and tile_env[tile + 1]) and every sample in [0, count) must be reached exactly once,
at the address index n -- (env * CH + row) -- and none at or above count."""
import ctypes

import numpy as np
import pytest

from predpreygrass_amd import _abi
from tests.policy_update_cases import SHAPES, make_spec

CH, HDR, TILE = _abi.POLICY_ROWS_CHUNK, _abi.POLICY_PLAN_HEADER, 128
SLOTS = (1, 3, 512)
CAPACITIES = (1, 200, 70_000)


def counts_of(capacity):
    return sorted({0, 1, 31, 32, 33, 127, 128, 129, capacity - 1, capacity, capacity + 5})


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    return _abi.bind(ctypes.CDLL(g.build_hip()))


def describe(lib, sp):
    out = (ctypes.c_int32 * 12)()
    assert lib.ppg_policy_describe(ctypes.byref(sp), out, 12) == 0
    return list(out)


@pytest.fixture(scope="module")
def networks(lib):
    """One network per kernel family (0 the FC chain: tile mode; 1 direct head, 2 deep, 3 the pipeline: range mode): (family, spec,
    range_tile, range_st)."""
    found = {}
    for shape in SHAPES:
        sp, keep = make_spec(shape)
        d = describe(lib, sp)
        if d[0] not in found:
            found[d[0]] = (shape, sp, keep, d)
    assert sorted(found) == [0, 1, 2, 3]
    return found


def range_mode_of(lib, family, sp, d):
    """(range_tile, range_st) as ppg_policy_run hands them to the plan kernel: the pipeline's table size comes with the description;
    the one-role direct-head kernels cut a tile of 128 into whole sub-groups."""
    st = d[1]
    if family == 0:
        return 0, st
    return (d[4] if family == 3 else st * (TILE // st)), st


def bisect_last(le, lo, hi):
    """Vectorised `while (a < b) { mid = (a + b + 1) >> 1; if (le(mid)) a = mid; else b = mid - 1; }` over arrays lo, hi."""
    a, b = lo.copy(), hi.copy()
    while True:
        open_ = a < b
        if not open_.any():
            return a
        mid = (a + b + 1) >> 1
        ok = le(mid)
        a = np.where(open_ & ok, mid, a)
        b = np.where(open_ & ~ok, mid - 1, b)


def plan_body_reference(counts, slots, range_tile, range_st):
    """plan_body of csrc/ppg_policy.h over `counts` (one per env): (plan words [3], prefix sums, tile_env)."""
    counts = np.asarray(counts, dtype=np.int64)
    n_envs = len(counts)
    per = (n_envs + 1023) // 1024
    t = np.arange(1024)
    lo = np.minimum(t * per, n_envs)
    hi = np.minimum(lo + per, n_envs)
    s = np.array([counts[a:b].sum() for a, b in zip(lo, hi)], dtype=np.int64)
    part = np.cumsum(s)                                  # the inclusive Hillis-Steele scan
    prefix = np.zeros(n_envs, dtype=np.int64)
    for a, b, before in zip(lo, hi, part - s):           # thread t: before = part[t] - s, then its run
        for e in range(a, b):
            prefix[e] = before
            before += counts[e]
    all_ = int(part[1023])

    def tile_env_of(n):
        n = np.asarray(n, dtype=np.int64)
        # the last run whose first env's prefix sum (part[u - 1]) is <= n, then the last env of that run whose prefix sum is <= n
        ua = bisect_last(lambda mid: part[mid - 1] <= n, np.zeros_like(n), np.full_like(n, 1023))
        a = np.where(ua * per < n_envs, ua * per, n_envs - 1)
        b = np.minimum(a + per - 1, n_envs - 1)
        return bisect_last(lambda mid: prefix[mid] <= n, a, b)

    if range_tile > 0:
        S = range_st * ((all_ + slots * range_st - 1) // (slots * range_st))
        tpw = (S + range_tile - 1) // range_tile if S else 1
        tile = np.arange(slots * tpw)
        if all_ == 0:
            return [all_, S, tpw], prefix, np.zeros(len(tile), dtype=np.int64)
        n = np.minimum((tile // tpw) * S + (tile % tpw) * range_tile, all_ - 1)
        return [all_, S, tpw], prefix, tile_env_of(n)
    per_round = TILE * slots
    n_full = (all_ // per_round) * slots
    rest = all_ - n_full * TILE
    ts = max(32 * ((rest + 32 * slots - 1) // (32 * slots)), 32)
    tail = all_ - n_full * TILE
    n_tiles = n_full + (tail + ts - 1) // ts
    tile = np.arange(n_tiles)
    n = np.where(tile < n_full, tile * TILE, n_full * TILE + (tile - n_full) * ts)
    return [all_, n_full, ts], prefix, (tile_env_of(n) if n_tiles else np.zeros(0, dtype=np.int64))


def rows_plan(lib, sp, slots, capacity, count):
    n = ctypes.c_uint64()
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), slots, capacity, count, None, 0, ctypes.byref(n)) == 0
    words = np.full(n.value + 4, 0xDEADBEEF, dtype=np.uint32)
    m = ctypes.c_uint64()
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), slots, capacity, count, words.ctypes.data, n.value, ctypes.byref(m)) == 0
    assert m.value == n.value and (words[n.value:] == 0xDEADBEEF).all()
    return words[:n.value].astype(np.int64)


def tiles_of(head, slots, range_tile):
    """(tile, first sample, samples) of every tile the forward kernels visit: policy_main (tile mode) / the share loop of the
    direct-head and pipeline kernels (range mode)."""
    N = head[0]
    out = []
    if range_tile > 0:
        share, tpw = head[1], head[2]
        for w in range(slots):
            begin, end = w * share, min(w * share + share, N)
            for j in range(tpw):
                n0 = begin + j * range_tile
                if n0 >= end:
                    break
                out.append((w * tpw + j, n0, min(end - n0, range_tile)))
        return out
    n_full, ts = head[1], head[2]
    n_tiles = n_full + (N - n_full * TILE + ts - 1) // ts
    for tile in range(n_tiles):
        size = TILE if tile < n_full else ts
        n0 = tile * TILE if tile < n_full else n_full * TILE + (tile - n_full) * ts
        out.append((tile, n0, min(N - n0, size)))
    return out


@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("family", (0, 1, 2, 3))
def test_rows_plan_equals_plan_body_and_reaches_every_row_once(lib, networks, family, slots, capacity):
    shape, sp, keep, d = networks[family]
    range_tile, range_st = range_mode_of(lib, family, sp, d)
    n_envs = (capacity + CH - 1) // CH
    for count in counts_of(capacity):
        clamped = min(max(count, 0), capacity)
        counts = np.clip(clamped - np.arange(n_envs) * CH, 0, CH)
        head, prefix, tile_env = plan_body_reference(counts, slots, range_tile, range_st)
        words = rows_plan(lib, sp, slots, capacity, count)
        where = (shape, slots, capacity, count)
        assert len(words) == HDR + n_envs + len(tile_env), where
        assert list(words[:HDR]) == head, where
        assert (words[HDR:HDR + n_envs] == prefix).all(), where
        got_env = words[HDR + n_envs:]
        assert (got_env == tile_env).all(), where
        # the walk of the forward kernels over the words the library returned
        pre = words[HDR:HDR + n_envs]
        tiles = tiles_of(list(words[:HDR]), slots, range_tile)
        reached = []
        n_slots = slots * head[2] if range_tile > 0 else len(got_env)
        for tile, n0, nt in tiles:
            n = n0 + np.arange(nt)
            lo = np.full(nt, got_env[tile])
            while True:   # phase_conv: while (lo + 1 < n_envs && plan[PLAN_HDR + 1 + lo] <= n) ++lo;
                step = (lo + 1 < n_envs) & (pre[np.minimum(lo + 1, n_envs - 1)] <= n)
                if not step.any():
                    break
                lo = lo + step
            if range_tile > 0:   # the direct-head kernels: the last env with prefix <= n between this tile's first env and the next tile's
                hi = np.full(nt, got_env[tile + 1] if tile + 1 < n_slots else n_envs - 1)
                e2 = bisect_last(lambda mid: pre[mid] <= n, np.full(nt, got_env[tile]), hi)
                assert (e2 == lo).all(), where
            row = n - pre[lo]
            assert ((row >= 0) & (row < CH)).all(), where
            reached.append(lo * CH + row)   # the address index: obs + (b * cap + row) * row_bytes with cap = CH
            assert (reached[-1] == n).all(), where
        reached = np.concatenate(reached) if reached else np.zeros(0, dtype=np.int64)
        assert len(reached) == clamped and (np.sort(reached) == np.arange(clamped)).all(), where


def test_rows_plan_refuses_what_no_plan_exists_for(lib, networks):
    _, sp, _, _ = networks[3]
    n = ctypes.c_uint64()
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), 0, 100, 10, None, 0, ctypes.byref(n)) == -1
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), 4, -1, 10, None, 0, ctypes.byref(n)) == -1
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), 4, (1 << 30) + 1, 10, None, 0, ctypes.byref(n)) == -1
    assert lib.ppg_policy_rows_plan(None, 4, 100, 10, None, 0, ctypes.byref(n)) == -1
    bad = _abi.PpgPolicySpec()
    assert lib.ppg_policy_rows_plan(ctypes.byref(bad), 4, 100, 10, None, 0, ctypes.byref(n)) == -1
    # a negative count is no rows; the size is reported without a buffer
    assert lib.ppg_policy_rows_plan(ctypes.byref(sp), 4, 100, -3, None, 0, ctypes.byref(n)) == 0 and n.value >= HDR + 1
