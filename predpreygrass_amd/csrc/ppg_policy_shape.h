// ppg_policy_shape.h -- the shape rules of a ppg_policy_spec, device-free and free of the policy kernels: ppg_policy_create_spec /
// ppg_policy_describe (ppg_policy_host.h) and ppg_net_* (ppg_learner_host.h, also in the CPU test build) accept the same networks and refuse
// the others with the same words.
#pragma once

#include <stdarg.h>
#include <stdio.h>

#include "../../include/ppg.h"

static int ppg_policy_shape_fail(char *msg, size_t n, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, n, fmt, ap);
    va_end(ap);
    return PPG_EINVAL;
}

// PPG_OK, or PPG_EINVAL with the reason in msg[n].  need_weights: also require the weight pointers.
static int ppg_policy_shape_check(const ppg_policy_spec &sp, bool need_weights, char *msg, size_t n) {
    const int layout = sp.layout, R = sp.obs_range, n_actions = sp.n_actions, C = sp.obs_channels;
    if (layout != PPG_POLICY_LAYOUT_CHW && layout != PPG_POLICY_LAYOUT_HWC) return ppg_policy_shape_fail(msg, n, "unknown layout %d", layout);
    if (sp.flatten != PPG_POLICY_FLATTEN_NCHW && sp.flatten != PPG_POLICY_FLATTEN_NHWC) return ppg_policy_shape_fail(msg, n, "unknown flatten order %d", sp.flatten);
    if (R < 1 || R > 15) return ppg_policy_shape_fail(msg, n, "obs_range %d outside 1..15", R);
    if (C < 1 || C > 8) return ppg_policy_shape_fail(msg, n, "obs_channels %d outside 1..8", C);
    if (n_actions < 1 || n_actions > 32) return ppg_policy_shape_fail(msg, n, "n_actions %d outside 1..32", n_actions);
    if (sp.n_conv < 1 || sp.n_conv > PPG_POLICY_MAX_CONV) return ppg_policy_shape_fail(msg, n, "n_conv %d outside 1..%d", sp.n_conv, PPG_POLICY_MAX_CONV);
    if (sp.n_fc < 1 || sp.n_fc > PPG_POLICY_MAX_FC) return ppg_policy_shape_fail(msg, n, "n_fc %d outside 1..%d", sp.n_fc, PPG_POLICY_MAX_FC);
    for (int l = 0; l < sp.n_conv; ++l) {
        const int lim = l == 0 ? 16 : l == 1 ? 32 : 64;
        if (sp.conv_out[l] < 1 || sp.conv_out[l] > lim)
            return ppg_policy_shape_fail(msg, n, "convolution %d has %d output channels: the kernels take up to 16 / 32 / 64 / 64 ...", l + 1, sp.conv_out[l]);
        if (need_weights && (!sp.conv_w[l] || !sp.conv_b[l])) return ppg_policy_shape_fail(msg, n, "a convolution weight pointer is NULL");
    }
    for (int l = 0; l < sp.n_fc; ++l) {
        if (need_weights && (!sp.fc_w[l] || !sp.fc_b[l])) return ppg_policy_shape_fail(msg, n, "a linear weight pointer is NULL");
        if (l + 1 < sp.n_fc && (sp.fc_out[l] < 1 || sp.fc_out[l] > 256))
            return ppg_policy_shape_fail(msg, n, "hidden head layer %d has %d features: the kernels take up to 256", l + 1, sp.fc_out[l]);
    }
    if (sp.fc_out[sp.n_fc - 1] != n_actions) return ppg_policy_shape_fail(msg, n, "the last linear layer has %d outputs, n_actions is %d", sp.fc_out[sp.n_fc - 1], n_actions);
    if (sp.n_fc > 1 && sp.n_conv != 3) return ppg_policy_shape_fail(msg, n, "a head with hidden layers needs exactly three convolutions (found %d)", sp.n_conv);
    if (sp.n_fc > 1 && layout != PPG_POLICY_LAYOUT_HWC && C != 4)
        return ppg_policy_shape_fail(msg, n, "channel-first networks with hidden head layers read 4-channel rows (found %d)", C);
    return PPG_OK;
}
