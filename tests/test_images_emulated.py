"""`ppg_pack` (csrc/ppg_pack.h) and `ppg_fetch` (csrc/ppg_fetch.h) through the kernel source compiled for the CPU wave emulator, at
every observation geometry of tests/image_cases.py: every image against a plain numpy reference built from the layout text of
include/ppg.h.  All handle sets run on all geometries here too (the images are small).  The same cases run on the GPU in
test_images_gpu.py."""
import os
import subprocess
import sys

import pytest

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import image_cases as cases
from tests.emu_backend import library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, _library=library(), **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, _library=library(), **kw)


BACKEND = cases.Backend(make, make_rq, lambda: None)
_sources = {}


def source(gid):
    """The stepped 130-env handle of a geometry; kept for the geometries the fetch test needs again."""
    if gid in _sources:
        return _sources[gid]
    src = cases.source(BACKEND, gid)
    if gid in cases.FETCH_GEOMETRIES:
        _sources[gid] = src
    return src


@pytest.mark.parametrize("gid", list(cases.GEOMETRIES))
def test_pack_geometry(gid):
    reached = cases.pack_matrix(BACKEND, gid, source(gid))
    print({k: sorted(v) for k, v in reached.items()})


@pytest.mark.parametrize("gid", cases.FETCH_GEOMETRIES)
def test_fetch_geometry(gid):
    print(cases.fetch_matrix(BACKEND, gid, source(gid)))


def test_pack_refuses_bad_calls():
    cases.pack_refusals(BACKEND)


def test_pack_env_without_predator_rows():
    assert cases.pack_env_without_predators(BACKEND) <= 50


_SAN_CODE = (
    "import sys; sys.path.insert(0, %r)\n"
    "from tests.emu_backend import library\n"
    "from tests import image_cases as cases\n"
    "from predpreygrass_amd.batched import BatchedPredPreyGrass\n"
    "from predpreygrass_amd.red_queen import BatchedRedQueen\n"
    "def backend(lib):\n"
    "    return cases.Backend(lambda cfg, B, **kw: BatchedPredPreyGrass(cfg, batch_size=B, _library=lib, **kw),\n"
    "                         lambda cfg, B, **kw: BatchedRedQueen(cfg, batch_size=B, _library=lib, **kw), lambda: None)\n"
    "cases.everything(backend(library(sanitize=True)), step_bk=backend(library()))\n"
    "print('SAN-CLEAN')\n")


def test_images_clean_under_ubsan():
    """The whole pack and fetch matrix against the build that traps on a misaligned access (and on every other undefined behaviour).
    The envs are stepped by the plain build and copied into handles of the trapping one: the step kernels have their own legs."""
    out = subprocess.run([sys.executable, "-c", _SAN_CODE % ROOT], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0 and "SAN-CLEAN" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
