"""`ppg_pack` (kernels ppg_pack_scan / ppg_pack_rows) and `ppg_fetch` (kernel ppg_fetch_rows) on the MI355X: the cases of
tests/image_cases.py, which test_images_emulated.py runs through the wave emulator -- every handle set, flag set and fetch range at
every observation geometry, against a plain numpy reference."""
import pytest
import torch

from predpreygrass_amd.batched import BatchedPredPreyGrass
from predpreygrass_amd.red_queen import BatchedRedQueen
from tests import image_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make(cfg, B, **kw):
    return BatchedPredPreyGrass(cfg, batch_size=B, device=DEV, **kw)


def make_rq(cfg, B, **kw):
    return BatchedRedQueen(cfg, batch_size=B, device=DEV, **kw)


BACKEND = cases.Backend(make, make_rq, torch.cuda.synchronize)
_sources = {}


def source(gid):
    if gid in _sources:
        return _sources[gid]
    src = cases.source(BACKEND, gid)
    if gid in cases.FETCH_GEOMETRIES:
        _sources[gid] = src
    return src


@pytest.mark.parametrize("gid", list(cases.GEOMETRIES))
def test_pack_geometry_on_gpu(gid):
    reached = cases.pack_matrix(BACKEND, gid, source(gid))
    print({k: sorted(v) for k, v in reached.items()})


@pytest.mark.parametrize("gid", cases.FETCH_GEOMETRIES)
def test_fetch_geometry_on_gpu(gid):
    print(cases.fetch_matrix(BACKEND, gid, source(gid)))


def test_pack_refuses_bad_calls_on_gpu():
    cases.pack_refusals(BACKEND)


def test_pack_env_without_predator_rows_on_gpu():
    assert cases.pack_env_without_predators(BACKEND) <= 50
