"""TEST-ONLY: the network shapes the weight-image tests cover (tests/test_policy_update_image.py; tests/policy_update_san_main.cpp holds
the same list) and a `ppg_policy_spec` with random normal host weights for one of them.

Every shape picks another path of the pack functions (csrc/ppg_policy_pack.h): channels-last with R <= 8 (one input-channel block),
R = 9 (the ninth channel of the pipeline's first convolution), R > 9 (no such fragments), R > 8 (two blocks); channel-first with 1-8
channels; 1-6 convolutions with narrow channels (padding lanes); no hidden head layer (the head and its per-wavefront copy), one, two,
narrow ones; both flatten orders; 1-32 actions (one or two action tiles, a padded logits tile)."""
import numpy as np

from predpreygrass_amd import _abi

# (layout, C, R, conv channels, hidden head layers, flatten, actions)
SHAPES = [
    ("hwc", 4, 7, (16, 32, 64), (), "nhwc", 9),
    ("hwc", 4, 9, (16, 32, 64), (), "nhwc", 9),
    ("hwc", 4, 11, (16, 32, 64), (), "nhwc", 9),
    ("hwc", 5, 15, (16, 32, 64), (), "nhwc", 17),
    ("hwc", 1, 3, (5,), (), "nhwc", 1),
    ("hwc", 8, 9, (5, 12), (), "nchw", 25),
    ("chw", 4, 9, (16, 32, 64), (), "nchw", 9),
    ("chw", 5, 7, (5, 12, 40), (), "nhwc", 32),
    ("chw", 1, 3, (16, 32, 64, 64), (), "nchw", 9),
    ("chw", 8, 5, (16, 24, 40, 64, 64), (), "nchw", 17),
    ("hwc", 4, 7, (8, 16, 32, 64, 64, 64), (), "nhwc", 9),
    ("chw", 4, 11, (16, 32, 64), (), "nhwc", 25),
    ("hwc", 4, 9, (16, 32, 64), (256, 256), "nhwc", 9),
    ("hwc", 4, 7, (16, 32, 64), (256,), "nhwc", 9),
    ("hwc", 5, 11, (16, 32, 64), (96, 160), "nchw", 17),
    ("chw", 4, 9, (16, 32, 64), (256, 256), "nchw", 9),
    ("chw", 4, 15, (16, 32, 64), (96, 160), "nhwc", 32),
    ("hwc", 8, 15, (5, 12, 40), (256,), "nhwc", 25),
    ("hwc", 1, 3, (16, 32, 64), (256, 256), "nchw", 1),
]

# source tensor numbers of a map entry (include/ppg.h: PPG_POLICY_IMAGE_MAP)
SRC_CONV_W, SRC_CONV_B, SRC_FC_W, SRC_FC_B, SRC_N = 0, 6, 12, 15, 18


def make_spec(shape, seed=0):
    """(spec, tensors): tensors[t] = the float32 array of source tensor t (None: the shape has no such layer); the spec points into them."""
    layout, C, R, chans, hiddens, flatten, A = shape
    rng = np.random.default_rng(seed)
    cin, positions = (R, C * R) if layout == "hwc" else (C, R * R)
    sp = _abi.PpgPolicySpec()
    sp.obs_channels, sp.obs_range, sp.n_actions = C, R, A
    sp.layout = _abi.POLICY_LAYOUT_HWC if layout == "hwc" else _abi.POLICY_LAYOUT_CHW
    sp.flatten = _abi.POLICY_FLATTEN_NHWC if flatten == "nhwc" else _abi.POLICY_FLATTEN_NCHW
    sp.n_conv, sp.n_fc = len(chans), len(hiddens) + 1
    tensors = [None] * SRC_N
    for l, c in enumerate(chans):
        tensors[SRC_CONV_W + l] = rng.standard_normal((c, cin, 3, 3)).astype(np.float32)
        tensors[SRC_CONV_B + l] = rng.standard_normal(c).astype(np.float32)
        sp.conv_out[l], sp.conv_w[l], sp.conv_b[l] = c, tensors[SRC_CONV_W + l].ctypes.data, tensors[SRC_CONV_B + l].ctypes.data
        cin = c
    fin = cin * positions
    for l, n in enumerate((*hiddens, A)):
        tensors[SRC_FC_W + l] = rng.standard_normal((n, fin)).astype(np.float32)
        tensors[SRC_FC_B + l] = rng.standard_normal(n).astype(np.float32)
        sp.fc_out[l], sp.fc_w[l], sp.fc_b[l] = n, tensors[SRC_FC_W + l].ctypes.data, tensors[SRC_FC_B + l].ctypes.data
        fin = n
    return sp, tensors
