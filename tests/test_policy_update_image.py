"""ppg_policy_update without a device: the weight image ppg_policy_create_spec uploads (ppg_policy_image: PACKED) against the same image
made the update's way (REPACKED: the repack map and the word function the kernel calls, run on the CPU over a buffer pre-filled with
0xA5) -- byte for byte, over every shape that picks another path of the pack functions (tests/policy_update_cases.py) --, the image's
sections against ppg_policy_pack, the map's own properties, and a negative control through a NumPy restatement of "apply the map"."""
import ctypes

import numpy as np
import pytest

from predpreygrass_amd import _abi
from tests.policy_update_cases import SHAPES, SRC_CONV_B, SRC_N, make_spec

HDR = _abi.POLICY_MAP_HEADER
N_ARRAYS, ARRAY_FC, ARRAY_CONV1X, ARRAY_SLOTS = 11, 6, 9, 10   # the arrays of the image, in order (include/ppg.h: ppg_policy_image)
TAIL = 1 << 29


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    return _abi.bind(ctypes.CDLL(g.build_hip()))


def image(lib, spec, what, dtype=np.uint8):
    n = ctypes.c_uint64(0)
    assert lib.ppg_policy_image(ctypes.byref(spec), what, None, 0, ctypes.byref(n)) == 0, lib.ppg_policy_last_error(None)
    out = np.zeros(n.value, dtype=np.uint8)
    assert lib.ppg_policy_image(ctypes.byref(spec), what, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) == 0
    return out.view(dtype)


def pack(lib, spec, what):
    """ppg_policy_pack's words, or None where it refuses `what` for this network."""
    n = ctypes.c_uint64(0)
    if lib.ppg_policy_pack(ctypes.byref(spec), what, None, 0, ctypes.byref(n)) != 0:
        return None
    out = np.zeros(n.value, dtype=np.uint16)
    assert lib.ppg_policy_pack(ctypes.byref(spec), what, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)) == 0
    return out


def bf16_bits(v):
    """float32 -> bfloat16 bits, to nearest even (finite values)."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def apply_map(m, tensors, buf):
    """The update in NumPy: every word the map covers is written into `buf` (uint8, the image's size), nothing else."""
    W, n_bias, bias_off = int(m[1]), int(m[2]), int(m[4])
    e = m[HDR:HDR + W + n_bias].astype(np.int64)
    base, flat = np.zeros(SRC_N + 1, dtype=np.int64), []
    for t in range(SRC_N):
        flat.append(np.zeros(0, np.float32) if tensors[t] is None else tensors[t].ravel())
        base[t + 1] = base[t] + flat[-1].size
    flat = np.concatenate(flat + [np.zeros(1, np.float32)])
    t = ((e >> 24) & 31) - 1
    v = flat[np.where(e != 0, base[t] + (e & 0xFFFFFF), flat.size - 1)]
    head = (bf16_bits(v).astype(np.uint32) << 16).view(np.float32)
    v = np.where(e & TAIL != 0, v - head, v).astype(np.float32)
    buf[:2 * W] = bf16_bits(v[:W]).view(np.uint8)
    buf[bias_off:bias_off + 4 * n_bias] = v[W:].view(np.uint8)
    return buf


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-C{s[1]}-R{s[2]}-conv{len(s[3])}x{s[3][-1]}-head{len(s[4])}-{s[5]}-A{s[6]}")
def test_the_updates_image_equals_the_image_create_uploads(lib, shape):
    """REPACKED == PACKED byte for byte (a word the map forgot would still hold 0xA5); the sections of the image are what
    ppg_policy_pack returns for the layers, the slot table's section is PACK_SLOTS' (untouched by the update); the map names every
    element of every parameter at least once, no index outside its tensor, nothing inside the slot table; and the NumPy restatement
    of the update gives the same bytes -- with ONE entry redirected it does not, so the equality can fail."""
    spec, tensors = make_spec(shape, seed=len(shape[3]) * 1000 + shape[2])
    packed, repacked = image(lib, spec, _abi.POLICY_IMAGE_PACKED), image(lib, spec, _abi.POLICY_IMAGE_REPACKED)
    m = image(lib, spec, _abi.POLICY_IMAGE_MAP, np.int32)
    assert packed.size == repacked.size and np.array_equal(packed, repacked), np.flatnonzero(packed != repacked)[:8]

    # ---- the header, and the sections against ppg_policy_pack
    W, n_bias, total, bias_off = (int(x) for x in m[1:5])
    off, words = m[5:5 + N_ARRAYS].astype(np.int64), m[16:16 + N_ARRAYS].astype(np.int64)
    assert m[0] == HDR and m.size == HDR + W + n_bias and total == packed.size and n_bias == 560 and bias_off + 4 * n_bias == total
    assert W % 128 == 0 and 2 * W == off[ARRAY_SLOTS] and (off % 256 == 0).all() and bias_off % 256 == 0
    ends = np.append(off[1:], bias_off)
    assert (off + 2 * words <= ends).all() and (ends - off - 2 * words < 256).all()
    section = lambda l: packed[off[l]:off[l] + 2 * words[l]].view(np.uint16)
    layout, C, R, chans, hiddens, flatten, A = shape
    for l in range(len(chans)):
        assert np.array_equal(section(l), pack(lib, spec, l)), l
    for l in range(len(chans), 6):
        assert words[l] == 0
    c1x = pack(lib, spec, _abi.POLICY_PACK_CONV1X)
    assert (words[ARRAY_CONV1X] == 0) if c1x is None else np.array_equal(section(ARRAY_CONV1X), c1x)
    assert (c1x is None) == ((R if layout == "hwc" else C) > 9)
    if not hiddens:
        assert np.array_equal(section(ARRAY_FC), pack(lib, spec, _abi.POLICY_PACK_HEAD))
    slots = pack(lib, spec, _abi.POLICY_PACK_SLOTS)
    assert (words[ARRAY_SLOTS] == 0) if slots is None else np.array_equal(section(ARRAY_SLOTS), slots)
    assert np.array_equal(repacked[off[ARRAY_SLOTS]:bias_off], packed[off[ARRAY_SLOTS]:bias_off])
    pad = np.ones(total, dtype=bool)   # the bytes between the arrays are zero in both
    for l in range(N_ARRAYS):
        pad[off[l]:off[l] + 2 * words[l]] = False
    pad[bias_off:] = False
    assert not packed[pad].any()

    # ---- the map
    e = m[HDR:].astype(np.int64)
    assert (e >= 0).all() and (e >> 30 == 0).all()
    used = e[e != 0]
    t, idx = ((used >> 24) & 31) - 1, used & 0xFFFFFF
    for k in range(SRC_N):
        mine = idx[t == k]
        if tensors[k] is None:
            assert mine.size == 0, k
            continue
        assert mine.max() < tensors[k].size, k                                                  # every index inside its tensor
        assert np.array_equal(np.unique(mine), np.arange(tensors[k].size)), k                   # every element used
    tails = used[used & TAIL != 0]
    assert tails.size and (((tails >> 24) & 31) - 1 >= SRC_CONV_B).all() and (((tails >> 24) & 31) - 1 < SRC_CONV_B + 6).all()
    assert not (e[W:] & TAIL).any()                                                             # the bias block copies

    # ---- the restatement, and the negative control
    assert np.array_equal(apply_map(m, tensors, np.full(total, 0xA5, np.uint8))[:2 * W], packed[:2 * W])
    assert np.array_equal(apply_map(m, tensors, np.full(total, 0xA5, np.uint8))[bias_off:], packed[bias_off:])
    bad = m.copy()
    plain = np.flatnonzero((e[:W] != 0) & (e[:W] & TAIL == 0))
    where = HDR + int(plain[plain.size // 2])
    k, i = ((int(bad[where]) >> 24) & 31) - 1, int(bad[where]) & 0xFFFFFF
    j = (i + 1) % tensors[k].size
    assert bf16_bits(tensors[k].ravel()[i]) != bf16_bits(tensors[k].ravel()[j])
    bad[where] = ((k + 1) << 24) | j
    assert not np.array_equal(apply_map(bad, tensors, np.full(total, 0xA5, np.uint8))[:2 * W], packed[:2 * W])


def test_ppg_policy_image_refuses_what_it_cannot_make(lib):
    spec, _ = make_spec(SHAPES[0])
    n = ctypes.c_uint64(0)
    assert lib.ppg_policy_image(ctypes.byref(spec), 3, None, 0, ctypes.byref(n)) == -1
    assert lib.ppg_policy_image(None, _abi.POLICY_IMAGE_PACKED, None, 0, ctypes.byref(n)) == -1
    assert lib.ppg_policy_image(ctypes.byref(spec), _abi.POLICY_IMAGE_PACKED, None, 0, None) == -1
    m = image(lib, spec, _abi.POLICY_IMAGE_MAP, np.int32)
    spec.conv_w[0] = None                        # the map does not read the weights; the images need them
    assert np.array_equal(image(lib, spec, _abi.POLICY_IMAGE_MAP, np.int32), m)
    assert lib.ppg_policy_image(ctypes.byref(spec), _abi.POLICY_IMAGE_REPACKED, None, 0, ctypes.byref(n)) == -1
    spec.obs_range = 16
    assert lib.ppg_policy_image(ctypes.byref(spec), _abi.POLICY_IMAGE_MAP, None, 0, ctypes.byref(n)) == -1
    # a buffer that is too small gets nothing, the size is still reported
    spec, _ = make_spec(SHAPES[0])
    small = np.full(64, 7, dtype=np.uint8)
    assert lib.ppg_policy_image(ctypes.byref(spec), _abi.POLICY_IMAGE_PACKED, small.ctypes.data_as(ctypes.c_void_p), 64, ctypes.byref(n)) == 0
    assert n.value > 64 and (small == 7).all()
    # ppg_policy_update refuses a NULL policy before it looks at anything else
    assert lib.ppg_policy_update(None, ctypes.byref(spec), None) == -1 and b"NULL" in lib.ppg_policy_last_error(None)
