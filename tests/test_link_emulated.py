"""`ppg_link` (csrc/ppg_link.h) and predpreygrass_amd.trajectory through the kernel source compiled for the CPU wave emulator:
every pair of consecutive outputs against a numpy join of the row_id tables, returns / GAE against a per-agent-name recursion.
The same scenarios run on the GPU in test_link_gpu.py."""
import os
import subprocess
import sys

import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import link_cases as cases
from tests.emu_backend import library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


def make_walls(cfg, B, **kw):
    env = make_rq(cfg, B, walls=True, **kw)
    return env.set_walls(cases.WALLS)


@pytest.mark.parametrize("cfg,prey_cap,calls", [(cases.CFG_BASE_Q1, 64, 100), (cases.CFG_BASE, 128, 100), (cases.CFG_BASE_Q4, 256, 60)])
def test_link_base_family(cfg, prey_cap, calls):
    env = make(cfg, B, prey_capacity=prey_cap, seed=11)
    assert (env.pred_capacity, env.prey_capacity) == (64, prey_cap)
    seen = cases.link_vs_id_join(env, calls)
    if prey_cap == 256:   # rows of the third prey register were linked
        assert seen["prey_rows"] > 128, seen


def test_link_128_predator_rows_births_cross_row_64():
    env = make(cases.CFG_P2, B, pred_capacity=128, prey_capacity=256, seed=7)
    assert cases.link_vs_id_join(env, 90)["pred_rows"] > 64


def test_link_second_generation():
    cases.link_vs_id_join(make_rq(cases.CFG_RQ, B, seed=5), 100)


def test_link_walls():
    cases.link_vs_id_join(make_walls(cases.CFG_RQ, B, seed=6), 80)


def test_link_drive():
    env = make(cases.CFG_DRIVE, B, seed=9)
    assert env.obs_channels_pred > 4
    cases.link_vs_id_join(env, 80)


def test_link_across_rollout():
    cases.link_across_rollout(make(cases.CFG_BASE, B, seed=2), n_rounds=12, K=5)


@pytest.mark.parametrize("family", ["base", "second_generation"])
def test_returns_and_gae_vs_agent_names(family):
    env = make(cases.CFG_BASE, B, seed=3) if family == "base" else make_rq(cases.CFG_RQ, B, seed=4)
    cases.returns_vs_names(env, 70, 0.97)


def test_invalidation():
    cases.invalidation(make(cases.CFG_BASE, B, seed=1))
    cases.invalidation(make_rq(cases.CFG_RQ, B, seed=1), set_placement=False)


def test_sub_batches_forward_link():
    from predpreygrass_amd.subbatch import SubBatchedPredPreyGrass
    env = SubBatchedPredPreyGrass(cases.CFG_BASE, batch_size=4, n_sub=2, device="cpu", _library=library())
    env.reset()
    env.link()
    env.step(random_actions=True)
    maps = env.link()
    assert len(maps) == 2 and all(bool((p >= 0).any()) and tuple(p.shape) == (2, e.S) for (p, n), e in zip(maps, env.subs))


_SAN_CODE = (
    "import sys; sys.path.insert(0, %r)\n"
    "from tests.emu_backend import library\n"
    "from tests import link_cases as cases\n"
    "from predpreygrass_amd.batched import BatchedPredPreyGrass\n"
    "from predpreygrass_amd.red_queen import BatchedRedQueen\n"
    "lib = library(sanitize=%r)\n"
    "mk = lambda cfg, B, **kw: BatchedPredPreyGrass(cfg, batch_size=B, _library=lib, **kw)\n"
    "cases.link_vs_id_join(mk(cases.CFG_BASE_Q1, 2, prey_capacity=64, seed=11), 70)\n"
    "cases.link_vs_id_join(mk(cases.CFG_P2, 2, pred_capacity=128, prey_capacity=256, seed=7), 50, need=('birth', 'death'))\n"
    "cases.link_vs_id_join(BatchedRedQueen(cases.CFG_RQ, batch_size=2, _library=lib, seed=5), 40, need=('birth',))\n"
    "cases.invalidation(mk(cases.CFG_BASE, 2, seed=1))\n"
    "print('SAN-CLEAN')\n")


def test_link_clean_under_address_sanitizer():
    from tests.emu_backend import asan_runtime, build
    rt = asan_runtime()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("gcc has no libasan.so here")
    build(sanitize="address")
    code = _SAN_CODE % (ROOT, "address")
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", PYTHONMALLOC="malloc")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1800, env=env)
    assert out.returncode == 0 and "SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


def test_link_clean_under_ubsan():
    code = _SAN_CODE % (ROOT, True)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0 and "SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
