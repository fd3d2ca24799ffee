"""The policy's device-free host code, pinned word for word: kernel family, LDS layout, slot tables and weight fragments of every
network shape must equal what tests/golden/policy_layout.npz recorded (tests/golden/make_golden_policy_layout.py says from where)."""
import ctypes

import numpy as np

from predpreygrass_amd import _abi
from tests.golden import make_golden_policy_layout as golden


def test_describe_slot_tables_and_fragments_equal_the_recorded_ones():
    import __graft_entry__ as g
    got = golden.compute(_abi.bind(ctypes.CDLL(g.build_hip())))
    want = np.load(golden.PATH)
    assert sorted(got) == sorted(want.files)
    assert len(got["grid"]) > 4000 and {"describe_" + e for e in golden.ENVS} | {"slots_" + e for e in golden.ENVS} <= set(got)
    for name in sorted(got):
        assert got[name].shape == want[name].shape, name
        differ = np.nonzero((got[name] != want[name]).reshape(len(got[name]), -1).any(axis=1))[0]
        assert len(differ) == 0, (name, len(differ), differ[:5].tolist(), got[name][differ[:2]].tolist(), want[name][differ[:2]].tolist())
    # what the file is expected to hold: every family, a table exactly for the pipeline's networks (whatever PPG_POLICY_PIPE says)
    d, s = want["describe_default"], want["slots_default"]
    fam3 = (d[:, 0] == 0) & (d[:, 1] == 3)
    assert all(((d[:, 0] == 0) & (d[:, 1] == f)).any() for f in range(4)) and fam3.sum() > 100
    assert np.array_equal(s[:, 0] == 0, fam3) and (s[fam3, 1] > 0).all()
    assert not (want["describe_pipe0"][:, 1] == 3).any() and np.array_equal(want["slots_pipe0"], s)
    assert np.array_equal((want["describe_slots0"][:, 0] == 0) & (want["describe_slots0"][:, 1] == 3), fam3)
