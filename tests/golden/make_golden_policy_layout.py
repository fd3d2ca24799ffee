#!/usr/bin/env python3
"""Generate tests/golden/policy_layout.npz: what the policy's device-free host code (ppg_policy_describe, ppg_policy_pack) answers for
every network shape, recorded from a library built at a known-good commit, so that a later restructuring of that host code is pinned
to it word for word (tests/test_policy_layout_golden.py recomputes `compute(lib)` from the current library and compares).  The committed
file comes from the library of commit bf9351b, the last one in which create, describe and pack each restated the layout.

Recorded, each under the environments ENVS (the two creation-time switches the host code reads):
  describe_<env>  [spec][13]  return code + the 12 words of ppg_policy_describe over the spec grid of
                              tests/test_abi.py::test_policy_kernel_choice_and_lds_layout_for_every_shape
  slots_<env>     [spec][3]   return code, length and CRC32 of the PPG_POLICY_PACK_SLOTS table (every family-3 spec has one)
and once, under the default environment:
  frag_<case>     [what][3]   return code, length and CRC32 of ppg_policy_pack for every layer code WHATS; weights from a seeded generator

    python tests/golden/make_golden_policy_layout.py [library]     (default: the library of this tree, built if stale)
"""
from __future__ import annotations

import ctypes
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from predpreygrass_amd import _abi  # noqa: E402

PATH = os.path.join(HERE, "policy_layout.npz")
ENVS = {"default": {}, "pipe0": {"PPG_POLICY_PIPE": "0"}, "slots0": {"PPG_POLICY_SLOTS": "0"}}
WHATS = (-1, 0, 1, 2, 3, 4, 5, 6, 7, _abi.POLICY_PACK_CONV1X, 150, _abi.POLICY_PACK_HEAD, _abi.POLICY_PACK_SLOTS, 301)
# (layout, C, R, conv channels, head widths): the six cases of test_weight_fragments_restated_in_numpy_equal_a_plain_convolution,
# then one network with two hidden head layers and one with one
FRAGMENT_CASES = [("hwc", 4, 9, (16, 32, 64), (9,)), ("hwc", 4, 7, (16, 32, 64), (9,)), ("chw", 4, 9, (16, 32, 64), (9,)),
                  ("hwc", 5, 9, (16, 32, 64, 64), (9,)), ("hwc", 4, 5, (12, 20, 40), (9,)), ("chw", 6, 5, (16, 24), (9,)),
                  ("hwc", 4, 9, (16, 32, 64), (256, 256, 9)), ("chw", 4, 7, (16, 32, 64), (96, 9))]


def grid():
    """(layout, C, R, n_conv, n_fc, n_actions) of every spec of the describe grid, in the order of the test in tests/test_abi.py."""
    return [(layout, C, R, n_conv, n_fc, n_actions)
            for layout in (_abi.POLICY_LAYOUT_CHW, _abi.POLICY_LAYOUT_HWC) for C in range(4, 9) for R in range(1, 16)
            for n_conv in range(1, 7) for n_fc, n_actions in ((1, 5), (1, 9), (1, 16), (1, 17), (1, 25), (2, 9), (3, 9))
            if n_fc == 1 or n_conv == 3]


def make_spec(layout, C, R, chans, widths, weights):
    """weights(n) -> a float32 array of n values that stays alive as long as the caller keeps it."""
    sp = _abi.PpgPolicySpec()
    sp.obs_channels, sp.obs_range, sp.n_actions, sp.layout, sp.flatten = C, R, widths[-1], layout, _abi.POLICY_FLATTEN_NHWC
    sp.n_conv, sp.n_fc = len(chans), len(widths)
    hwc = layout == _abi.POLICY_LAYOUT_HWC
    cin = R if hwc else C
    for l, c in enumerate(chans):
        sp.conv_out[l], sp.conv_w[l], sp.conv_b[l] = c, weights(c * cin * 9).ctypes.data, weights(c).ctypes.data
        cin = c
    fin = (C if hwc else R) * R * chans[-1]
    for l, c in enumerate(widths):
        sp.fc_out[l], sp.fc_w[l], sp.fc_b[l] = c, weights(c * fin).ctypes.data, weights(c).ctypes.data
        fin = c
    return sp


def pack(lib, sp, what):
    """(return code, words, CRC32 of the words) of ppg_policy_pack; a refused `what` gives (rc, 0, 0)."""
    n = ctypes.c_uint64(0)
    rc = lib.ppg_policy_pack(ctypes.byref(sp), what, None, 0, ctypes.byref(n))
    if rc != 0:
        return rc, 0, 0
    out = np.zeros(n.value, dtype=np.uint16)
    rc = lib.ppg_policy_pack(ctypes.byref(sp), what, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n))
    assert rc == 0 and n.value == len(out)
    return 0, len(out), zlib.crc32(out.tobytes())


def compute(lib):
    """Every recorded array, from `lib` (a bound ctypes library).  Sets and restores the switches of ENVS in os.environ."""
    zeros = np.zeros(32 * 15 * 15 * 64, dtype=np.float32)   # (the largest tensor of the grid: 32 actions' worth of a 15 x 15 x 64 flatten)
    specs = [make_spec(layout, C, R, ([16, 32, 64] + [64] * 3)[:n_conv], [256] * (n_fc - 1) + [n_actions], lambda n: zeros)
             for layout, C, R, n_conv, n_fc, n_actions in grid()]
    res = {"grid": np.array(grid(), dtype=np.int32)}
    saved = {k: os.environ.pop(k, None) for k in ("PPG_POLICY_PIPE", "PPG_POLICY_SLOTS")}
    try:
        for env, switches in ENVS.items():
            os.environ.update(switches)
            d = np.zeros((len(specs), 13), dtype=np.int64)
            s = np.zeros((len(specs), 3), dtype=np.int64)
            for i, sp in enumerate(specs):
                out = (ctypes.c_int32 * 12)()
                d[i, 0] = lib.ppg_policy_describe(ctypes.byref(sp), out, 12)
                d[i, 1:] = out[:]
                s[i] = pack(lib, sp, _abi.POLICY_PACK_SLOTS)
            res["describe_" + env], res["slots_" + env] = d, s
            for k in switches:
                del os.environ[k]
        for k, (layout, C, R, chans, widths) in enumerate(FRAGMENT_CASES):
            rng = np.random.default_rng(1000 + k)
            keep = []

            def weights(n):
                keep.append(rng.uniform(-1.0, 1.0, n).astype(np.float32))
                return keep[-1]
            sp = make_spec(_abi.POLICY_LAYOUT_HWC if layout == "hwc" else _abi.POLICY_LAYOUT_CHW, C, R, chans, widths, weights)
            res[f"frag_{k}"] = np.array([pack(lib, sp, what) for what in WHATS], dtype=np.int64)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        import __graft_entry__ as g
        path = g.build_hip()
    res = compute(_abi.bind(ctypes.CDLL(path)))
    np.savez_compressed(PATH, **res)
    fam = res["describe_default"][:, 1][res["describe_default"][:, 0] == 0]
    print(f"{PATH}: {len(res['grid'])} specs, families {np.bincount(fam, minlength=4).tolist()}, "
          f"{int((res['slots_default'][:, 0] == 0).sum())} slot tables, {os.path.getsize(PATH) / 1024:.0f} KiB")
