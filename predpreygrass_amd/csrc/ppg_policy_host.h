// ppg_policy_host.h -- the host side of policy inference (include/ppg.h: ppg_policy_*): struct ppg_policy, the shape rules and the
// device-free layout, create / pack / image / update / describe, the diagnostic builds' launch plumbing, act, evaluate and rows_plan.
// The kernels it launches and their parameter blocks are ppg_policy.h's (namespace ppgpol); ppg_hip.hip includes this file behind it.
#pragma once

#include "ppg_policy.h"
#include "ppg_policy_shape.h"

struct ppg_policy {
    int32_t device, R, n_actions, layout, cin;
    int32_t obs_channels;  // C of the (C,R,R) rows this network reads
    int32_t direct;        // 1: no hidden head layer, ppg_policy_direct.h (2: with more than three convolutions); 0: the FC chain
    int32_t nch16;         // more than 8 input channels into conv1
    int32_t pipe;          // direct == 1 only: the two-role pipeline kernels (ppg_policy_pipe.h), 512 threads per workgroup
    uint64_t macs;         // real multiply-accumulates per observation
    ppgpol::PolParams base;
    void *dev_weights;     // one allocation: fragments + biases
    __bf16 *xg;            // scratch slots (FC chain only)
    float *lgs;            // logits rows of the tiles in flight (direct path only)
    bool xg_is_spread;     // (from ppg_alloc_spread)
    uint32_t *plan;        // [PLAN_HDR + plan_envs] header + prefix sums, then the first env of every tile
    int32_t plan_envs;
    size_t plan_words;     // words the buffer was allocated with (it depends on the species' row capacity too)
    // ppg_policy_evaluate's own plan (never ppg_policy_act's: an evaluate between two acts must move nothing a captured act reads) and
    // the scratch its forward launch stores the action bytes into; sized for the largest capacity seen
    uint32_t *rows_plan;
    int8_t *rows_actions;
    int64_t rows_capacity;
    uint32_t *pre_g;       // the fused launch's prefix sums in memory (PolParams2::pre_g), [2][FUSED_MAX_ENVS]; owned by the prey's policy
    int32_t grid;
    int32_t lds_bytes;
    hipStream_t side;      // ppg_policy_act with both species: the predators' launch runs beside the prey's (fork / join by events)
    hipEvent_t fork, join;
    // ppg_policy_update: the shape the policy was created with (weight pointers NULL), where each array lies in dev_weights, and the
    // repack map on the device (allocated by the first update, freed by ppg_policy_destroy)
    ppg_policy_spec shape;
    ppg_policy_image_layout image;
    int32_t *map_dev;
    int32_t cus;
    char err[256];
};

static char g_ppg_policy_error[256] = "";

static int ppg_policy_fail(ppg_policy *p, int code, const char *fmt, ...) {
    char *dst = p ? p->err : g_ppg_policy_error;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 256, fmt, ap);
    va_end(ap);
    return code;
}

// ppg_policy_act with two policies: a failure is also reported through ppg_policy_last_error(NULL), whichever of them it came from
static int ppg_policy_mirror(const ppg_policy *p, int rc) {
    if (rc != PPG_OK) memcpy(g_ppg_policy_error, p->err, sizeof g_ppg_policy_error);
    return rc;
}

#define PPG_POL_TRY(p, call)                                                                              \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return ppg_policy_fail(p, PPG_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

extern "C" {

int ppg_policy_create_spec(int32_t device, const ppg_policy_spec *spec, ppg_policy **out);

int ppg_policy_create_layout(int32_t device, int32_t obs_range, int32_t n_actions, int32_t layout, const ppg_policy_weights *w,
                             ppg_policy **out) {
    if (!w || !out) return ppg_policy_fail(nullptr, PPG_EINVAL, "null argument");
    ppg_policy_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.obs_channels = 4; sp.obs_range = obs_range; sp.n_actions = n_actions; sp.layout = layout; sp.flatten = PPG_POLICY_FLATTEN_NCHW;
    sp.n_conv = 3; sp.conv_out[0] = 16; sp.conv_out[1] = 32; sp.conv_out[2] = 64;
    sp.n_fc = 3; sp.fc_out[0] = 256; sp.fc_out[1] = 256; sp.fc_out[2] = n_actions;
    for (int l = 0; l < 3; ++l) { sp.conv_w[l] = w->conv_w[l]; sp.conv_b[l] = w->conv_b[l]; sp.fc_w[l] = w->fc_w[l]; sp.fc_b[l] = w->fc_b[l]; }
    return ppg_policy_create_spec(device, &sp, out);
}

int ppg_policy_create(int32_t device, int32_t obs_range, int32_t n_actions, const ppg_policy_weights *w, ppg_policy **out) {
    return ppg_policy_create_layout(device, obs_range, n_actions, PPG_POLICY_LAYOUT_CHW, w, out);
}

int ppg_policy_destroy(ppg_policy *p);

// diagnostic switch: environment variable PPG_POLICY_PIPE=0 at creation time sends a network the pipeline would take to the one-role
// direct-head kernels instead (tests compare the two bit for bit)
static bool ppg_pipe_enabled() {
    const char *e = getenv("PPG_POLICY_PIPE");
    return !(e && e[0] == '0' && e[1] == 0);
}
// The pipeline's SLOT TABLE (ppg_policy_direct.h: dconv_cells): the ST * P positions of a sub-group in an order in which slot n's cell of
// the padded image -- 16-byte cell number sample * stride_cells + (y + 1) * Wp + x + 1 -- is congruent to n modulo 16.  A 32-slot MFMA
// tile then is, bank-wise, a run of 32 consecutive cells: ds_read_b128's sixteen-lane groups and the stores' eight-lane groups touch every
// bank once.  Possible iff no residue class holds more than two cells per tile; which classes the cells fall into depends on the
// sample stride (ppg_pipe_layout tries the eight strides that keep the head's reads conflict-free).  Returns false if some class is
// too full (the table is then the plain order: slot n = position n).
static bool ppg_slot_table(int ST, int IH, int IW, int stride_elems, std::vector<uint16_t> &tab) {
    const int P = IH * IW, Wp = IW + 1, tiles = (ST * P + 31) / 32, per_class = 2 * tiles, stride_cells = stride_elems / 8;
    std::vector<std::vector<uint16_t>> cls(16);
    for (int s = 0; s < ST; ++s)
        for (int p = 0; p < P; ++p) {
            const int y = p / IW, x = p % IW;
            cls[(s * stride_cells + (y + 1) * Wp + x + 1) & 15].push_back((uint16_t)(s << 8 | p));
        }
    bool ok = true;
    for (int r = 0; r < 16; ++r) ok = ok && (int)cls[r].size() <= per_class;
    tab.assign((size_t)32 * tiles, 0xFFFFu);
    if (!ok) {
        for (int n = 0; n < ST * P; ++n) tab[n] = (uint16_t)((n / P) << 8 | (n % P));
        return false;
    }
    // slot 16 k + r <- the k-th cell of class r, the classes' cells in (sample, position) order: a tile's two halves then hold
    // neighbouring positions, and the first sub-group-of-a-share's short last sub-group leaves whole slots empty rather than scattered
    for (int r = 0; r < 16; ++r)
        for (size_t k = 0; k < cls[r].size(); ++k) tab[16 * k + r] = cls[r][k];
    return true;
}

// samples per sub-group of the direct-head kernels, at most st_max: the most samples per round of position tiles (four wavefronts take a
// tile of 32 positions each); of equal scores the largest
static int ppg_subgroup_samples(int st_max, int P) {
    int st = st_max;
    double best = 0.0;
    for (int c = st_max; c >= 1; --c) {
        const int tiles = (c * P + 31) / 32, rounds = (tiles + 3) / 4;
        const double score = (double)c / rounds;
        if (score > best * 1.0001) { best = score; st = c; }
    }
    return st;
}

// LDS layout of the two-role pipeline kernels (ppg_policy_pipe.h) for rows of C x R x R elements read as P positions; blk = elements of
// one channel block of a sample's padded image, f_elems = elements of an area F.  Device-free (ppg_policy_describe, CPU tests).
static bool ppg_pipe_layout_at(int C, int R, int P, int blk, int f_elems, int tail_slack, ppgpol::PolParams &K, int *lds_bytes, int stride);
static bool ppg_pipe_layout(int C, int R, int P, int blk, int f_elems, int tail_slack, ppgpol::PolParams &K, int *lds_bytes,
                            std::vector<uint16_t> *slot_tab = nullptr) {
    int stride = 10 * blk + 2 * f_elems;
    while (((stride / 2) % 64) % 8 != 4) stride += 8;   // consecutive samples 16 bytes x an odd number apart in the banks: the head's
                                                        // sixteen sample columns read conflict-free
    // ... and of the eight such strides modulo 256 bytes the first for which the slot table exists (ppg_slot_table: whether a tile's
    // cells can be spread over all bank groups depends on where consecutive samples' images start)
    std::vector<uint16_t> tab;
    const char *sw = getenv("PPG_POLICY_SLOTS");   // diagnostic switch: PPG_POLICY_SLOTS=0 at creation time keeps the plain order (A/B runs)
    for (int k = 0; k < 8 && !(sw && sw[0] == '0' && sw[1] == 0); ++k) {
        if (!ppg_pipe_layout_at(C, R, P, blk, f_elems, tail_slack, K, lds_bytes, stride + 16 * k)) break;
        if (ppg_slot_table(K.ST, P / R, R, K.sample_stride, tab)) {
            if (slot_tab) *slot_tab = tab;
            K.slot_tiles = (int)tab.size() / 32;
            return true;
        }
    }
    if (!ppg_pipe_layout_at(C, R, P, blk, f_elems, tail_slack, K, lds_bytes, stride)) return false;
    if (ppg_slot_table(K.ST, P / R, R, K.sample_stride, tab)) {   // (PPG_POLICY_SLOTS=0 and this stride happens to admit a table: not wanted)
        tab.assign(tab.size(), 0xFFFFu);
        for (int n = 0; n < K.ST * P; ++n) tab[n] = (uint16_t)((n / P) << 8 | (n % P));
    }
    if (slot_tab) *slot_tab = tab;
    K.slot_tiles = (int)tab.size() / 32;
    return true;
}
static bool ppg_pipe_layout_at(int C, int R, int P, int blk, int f_elems, int tail_slack, ppgpol::PolParams &K, int *lds_bytes, int stride) {
    const int fixed_p = 2 * 4096 + 64 + 2048 + 1024 + tail_slack;   // partial sums x 2, role B's counter, Gumbel noise x 2, dconv's dummy slots (64 lanes)
    const int row_bf16 = C * R * R * 2;   // bytes of a bfloat16 row; the area `raw` takes ST of them when they are whole 8-byte chunks
    const bool chunks = row_bf16 % 8 == 0;
    int st_cap = (160 * 1024 - fixed_p - 128 * 16) / (stride * 2 + (chunks ? row_bf16 : 0));   // (at least 128 samples of table)
    if (st_cap > 16) st_cap = 16;
    while (st_cap > 1 && st_cap * P > 256) --st_cap;   // a role-B thread stages one position
    if (st_cap < 1 || P > 256) return false;
    {
        const int st = ppg_subgroup_samples(st_cap, P);
        int raw_bytes = chunks ? (st * row_bf16 + 15) / 16 * 16 : 0;
        const int cpr = row_bf16 / 8;   // 8-byte chunks per row; the role-B threads cover floor(256 / cpr) samples per load
        K.pipe_slots = chunks && cpr <= 256 ? 256 / cpr : 0;
        K.pipe_ni = K.pipe_slots ? (st + K.pipe_slots - 1) / K.pipe_slots : 0;
        if (K.pipe_ni > ppgpol::PIPE_CHUNKS) K.pipe_ni = 0;   // (that many chunk registers per thread)
        if (!K.pipe_ni) raw_bytes = 0;
        K.pipe_magic = K.pipe_ni ? (uint32_t)((0x100000000ull + cpr - 1) / cpr) : 0u;
        int cap_tab = (160 * 1024 - fixed_p - raw_bytes - st * stride * 2) / 16;
        if (cap_tab > 2048) cap_tab = 2048;
        K.ST = st;
        K.range_tile = st * (cap_tab / st);
        K.off_x = 0; K.pipe_x1 = 4 * blk; K.off_y = 8 * blk; K.off_f = 10 * blk; K.pipe_f1 = K.off_f + f_elems;
        K.sample_stride = stride;
        K.pipe_red = K.range_tile * 16;
        K.pipe_raw = K.pipe_red + 2 * 4096 + 64 + 2048;
        K.pipe_img = K.pipe_raw + raw_bytes + 1024;
        *lds_bytes = K.pipe_img + st * stride * 2 + tail_slack;
    }
    return true;
}

// The shape rules of ppg_policy_create_spec, device-free: shared with ppg_policy_describe so that the description of a network exists
// exactly when the network can be created.  need_weights: also require the weight pointers.  (The rules themselves:
// ppg_policy_shape.h, which ppg_net_* share.)
static int ppg_policy_check_spec(const ppg_policy_spec &sp, bool need_weights) {
    char msg[256];
    if (ppg_policy_shape_check(sp, need_weights, msg, sizeof msg) != PPG_OK) return ppg_policy_fail(nullptr, PPG_EINVAL, "%s", msg);
    return PPG_OK;
}

// Everything the SHAPE of a network decides, device-free: ppg_policy_create_spec builds what this says, ppg_policy_describe prints it and
// ppg_policy_pack(PPG_POLICY_PACK_SLOTS) returns its slot table.
struct ppg_policy_layout {
    int family;                       // 0: the FC chain; 1: direct head; 2: direct head behind more than three convolutions; 3: the two-role pipeline
    int threads;                      // per workgroup
    int lds_bytes;                    // dynamic LDS of a workgroup
    int wgs_per_cu;                   // 1: a workgroup takes a whole CU's LDS (grid = CUs); 2: half of it (grid = 2 x CUs)
    ppgpol::PolParams K;              // the geometry only, the rest zero: Wp, Wp2, flat_c, kflat_steps, head_mt, ST, range_tile, off_*, sample_stride, pipe_*, slot_tiles
    std::vector<uint16_t> slot_tab;   // family 3: ppg_slot_table
};

// sp: a spec ppg_policy_check_spec accepts.  allow_pipe = false sends a network of the two-role pipeline to the one-role direct-head
// kernels instead.  PPG_EINVAL: the image is too large for one sample in LDS.
static int ppg_policy_layout_of(const ppg_policy_spec &sp, bool allow_pipe, ppg_policy_layout &L) {
    const int R = sp.obs_range, C = sp.obs_channels, hwc = sp.layout == PPG_POLICY_LAYOUT_HWC;
    // the image the convolutions run on: R x R with C channels, or (channels-last) C x R with R channels
    const int IH = hwc ? C : R, IW = R, CIN = hwc ? R : C, P = IH * IW;
    ppgpol::PolParams &K = L.K;
    memset(&K, 0, sizeof K);
    L.slot_tab.clear();
    L.threads = 256;
    if (sp.n_fc > 1) {
        // FC chain.  LDS: tile table + max(activation images of ST samples, H, FC1 staging); ST as large as 2 workgroups per CU (80 KB each) allow
        K.Wp = IW + 2; K.Wp2 = (IH + 2) * (IW + 2);
        const int per_sample = 6 * K.Wp2 * 8 * 2;                       // X (4 blocks) + Y (2 blocks), bytes
        const int h_bytes = ppgpol::TILE * ppgpol::HSTRIDE * 2;
        int st = (78 * 1024 - ppgpol::TILE * 16) / per_sample;
        if (st < 1) st = 1;
        if (st > 16) st = 16;
        while (st > 1 && st * P > 512) --st;   // the staging of a sub-group gives every thread at most two positions
        K.ST = st;
        const int img = st * per_sample, fc1_stage = 3 * ppgpol::FC1_BUF;
        int overlay = img > h_bytes ? img : h_bytes;
        if (fc1_stage > overlay) overlay = fc1_stage;
        L.family = 0; L.wgs_per_cu = 2; L.lds_bytes = ppgpol::TILE * 16 + overlay;
        return PPG_OK;
    }
    // direct head: area F is [position][flat_c channels], read by the head in k-steps of 32 features, 16 actions per tile
    K.flat_c = (sp.conv_out[sp.n_conv - 1] + 7) / 8 * 8; K.kflat_steps = (P * K.flat_c + 31) / 32; K.head_mt = (sp.n_actions + 15) / 16;
    // LDS region of a sample: X (4 blocks) | Y (2 blocks) | F | [D0 | D1] -- padded pitch W + 1 (ppg_policy_direct.h)
    K.Wp = IW + 1; K.Wp2 = (IH + 2) * (IW + 1) + 1;
    const int blk = K.Wp2 * 8, f_elems = K.kflat_steps * 32 + 8;   // (+ 8: consecutive samples' fragments fall into different banks)
    K.off_x = 0; K.off_y = 4 * blk; K.off_f = 6 * blk; K.off_d0 = K.off_f + f_elems; K.off_d1 = K.off_d0 + 8 * blk;
    K.sample_stride = K.off_f + f_elems + (sp.n_conv > 3 ? 8 * blk : 0) + (sp.n_conv > 4 ? 8 * blk : 0);
    const int tail_slack = 18 * 32 * 2;   // bytes behind the last sample's region: the head's unconditional fragment reads end there
    // the two-role pipeline (ppg_policy_pipe.h): three convolutions, up to 16 actions, a wavefront's quarter of the head's k-steps in 18
    // fragments, up to nine input channels (Conv1X); region of a sample: X0 | X1 (4 blocks each) | Y (2 blocks) | F0 | F1
    if (allow_pipe && sp.n_conv == 3 && K.head_mt == 1 && (K.kflat_steps + 3) / 4 <= 18 && CIN <= 9 &&
        ppg_pipe_layout(C, R, P, blk, f_elems, tail_slack, K, &L.lds_bytes, &L.slot_tab)) {
        L.family = 3; L.threads = 512; L.wgs_per_cu = 1;
        return PPG_OK;
    }
    const int fixed = ppgpol::TILE * 16 + K.head_mt * 4096 + 4096 + tail_slack;   // table, partial logits, dconv's dummy slots
    int st_max = (160 * 1024 - fixed) / (K.sample_stride * 2);   // one workgroup per CU with all of its LDS (ppg_policy_direct.h)
    if (st_max > 16) st_max = 16;                // (the head's 16 sample columns)
    while (st_max > 1 && st_max * P > 512) --st_max;   // a thread stages at most two positions
    if (st_max < 1)
        return ppg_policy_fail(nullptr, PPG_EINVAL, "a %d x %d image with %d convolutions needs %d bytes of LDS per sample: too large", IH, IW, sp.n_conv, K.sample_stride * 2);
    const int st = ppg_subgroup_samples(st_max, P);
    K.ST = st;
    K.range_tile = st * (ppgpol::TILE / st);   // whole sub-groups per tile
    L.family = sp.n_conv > 3 ? 2 : 1; L.wgs_per_cu = 1; L.lds_bytes = fixed + st * K.sample_stride * 2;
    return PPG_OK;
}

int ppg_policy_create_spec(int32_t device, const ppg_policy_spec *spec, ppg_policy **out) {
    if (!spec || !out) return ppg_policy_fail(nullptr, PPG_EINVAL, "null argument");
    const ppg_policy_spec &sp = *spec;
    const int layout = sp.layout, R = sp.obs_range, n_actions = sp.n_actions, C = sp.obs_channels;
    {
        const int rc = ppg_policy_check_spec(sp, true);
        if (rc != PPG_OK) return rc;
    }
    const int hwc = layout == PPG_POLICY_LAYOUT_HWC;
    const int IH = hwc ? C : R, IW = R, CIN = hwc ? R : C, P = IH * IW, K1 = 64 * P;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return ppg_policy_fail(nullptr, PPG_ENODEV, "device %d not available", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ppg_policy_fail(nullptr, PPG_ENODEV, "ppg_policy needs a gfx950 device (MI355X)");
    ppg_policy_layout L;
    {
        const int rc = ppg_policy_layout_of(sp, ppg_pipe_enabled(), L);
        if (rc != PPG_OK) return rc;
    }
    ppg_policy_fragments F;
    ppg_policy_fragments_of(sp, F);
    ppg_policy *p = new (std::nothrow) ppg_policy();
    if (!p) return ppg_policy_fail(nullptr, PPG_ENOMEM, "out of host memory");
    memset(p, 0, sizeof *p);   // (every failure below: ppg_policy_destroy frees what exists by then)
    p->device = device; p->R = R; p->n_actions = n_actions; p->layout = layout; p->cin = CIN; p->obs_channels = C;
    p->direct = L.family == 3 ? 1 : L.family;
    p->pipe = L.family == 3;
    p->nch16 = CIN > 8;
    p->lds_bytes = L.lds_bytes;
    p->grid = L.wgs_per_cu * prop.multiProcessorCount;
    p->cus = prop.multiProcessorCount;
    p->shape = sp;
    for (int l = 0; l < PPG_POLICY_MAX_CONV; ++l) p->shape.conv_w[l] = p->shape.conv_b[l] = nullptr;
    for (int l = 0; l < PPG_POLICY_MAX_FC; ++l) p->shape.fc_w[l] = p->shape.fc_b[l] = nullptr;
#ifdef PPG_EXPERIMENTS
    if (const char *g = getenv("PPG_POLICY_GRID")) p->grid = L.wgs_per_cu == 2 && atoi(g) > 0 ? atoi(g) : p->grid;   // resident workgroups
#endif
    {   // real multiply-accumulates per observation
        uint64_t m = 0;
        int ci = CIN;
        for (int l = 0; l < sp.n_conv; ++l) { m += (uint64_t)P * sp.conv_out[l] * 9 * ci; ci = sp.conv_out[l]; }
        int fi = P * sp.conv_out[sp.n_conv - 1];
        for (int l = 0; l < sp.n_fc; ++l) { m += (uint64_t)fi * sp.fc_out[l]; fi = sp.fc_out[l]; }
        p->macs = m;
    }
    const int NF = PPG_FRAG_N;
    p->image = ppg_policy_image_layout_of(F, L.slot_tab.size());
    const size_t *off = p->image.off, total = p->image.total;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&p->dev_weights, total) != hipSuccess) {
        (void)ppg_policy_destroy(p);
        return ppg_policy_fail(nullptr, PPG_EHIP, "hipMalloc of %zu bytes of weights failed", total);
    }
    std::vector<unsigned char> stage(total);
    ppg_policy_image_assemble(F, p->image, L.slot_tab.data(), stage.data());
    if (hipMemcpy(p->dev_weights, stage.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)ppg_policy_destroy(p);
        return ppg_policy_fail(nullptr, PPG_EHIP, "upload of the weights failed");
    }
    ppgpol::PolParams &K = p->base;
    K = L.K;
    K.magic_P = (uint32_t)(((1u << ppgpol::DIV_SHIFT) + P - 1) / P);
    K.magic_R = (uint32_t)(((1u << ppgpol::DIV_SHIFT) + IW - 1) / IW);
    K.R = R; K.P = P; K.K1 = K1; K.n_actions = n_actions;
    K.IH = IH; K.IW = IW; K.cin = CIN; K.obs_elems = C * R * R;
    K.n_conv = sp.n_conv;
    for (int l = 0; l < sp.n_conv; ++l) K.cout_blocks[l] = (sp.conv_out[l] + 7) / 8;
    K.n_hidden = L.family == 0 ? sp.n_fc - 1 : 0;
    // observation element [a][b][c] of the (C,R,R) row: channel-first = (channel a, position b * R + c); channels-last = (position
    // a * R + b, channel c)
    K.c_stride = hwc ? 1 : R * R; K.p_stride = hwc ? R : 1;
    const unsigned char *dw = (const unsigned char *)p->dev_weights;
    K.wc1 = (const ppgpol::bf16x8 *)(dw + off[0]); K.wc2 = (const ppgpol::bf16x8 *)(dw + off[1]);
    K.wc3 = (const ppgpol::bf16x8 *)(dw + off[2]);
    for (int l = 3; l < PPG_POLICY_MAX_CONV; ++l) K.wcd[l - 3] = (const ppgpol::bf16x8 *)(dw + off[l]);
    K.w1 = (const ppgpol::bf16x8 *)(dw + off[PPG_FRAG_FC]); K.w2 = (const ppgpol::bf16x8 *)(dw + off[PPG_FRAG_FC + 1]); K.w3 = (const ppgpol::bf16x8 *)(dw + off[PPG_FRAG_FC + 2]);
    K.wh = K.w1; K.whw = K.w2;
    const float *db = (const float *)(dw + off[NF]);   // (the convolutions' biases ride in their fragments)
    K.b1 = db; K.b2 = db + 256; K.b3 = db + 512; K.bh = db + 512;
    K.wc1x = (const ppgpol::bf16x8 *)(dw + off[PPG_FRAG_CONV1X]); K.bc1x = db + 544;
    K.slot_tab = (const uint16_t *)(dw + off[PPG_FRAG_SLOTS]);
    // the family's scratch (the pipeline has none)
    if (L.family == 1 || L.family == 2) {
        const size_t lgs_bytes = (size_t)p->grid * ppgpol::TILE * 16 * K.head_mt * 4;
        if (hipMalloc((void **)&p->lgs, lgs_bytes) != hipSuccess || hipMemset(p->lgs, 0, lgs_bytes) != hipSuccess) {
            (void)ppg_policy_destroy(p);
            return ppg_policy_fail(nullptr, PPG_EHIP, "hipMalloc of %zu bytes of scratch failed", lgs_bytes);
        }
        K.lgs = p->lgs;
    } else if (L.family == 0) {
        const size_t xg_bytes = (size_t)p->grid * ppgpol::TILE * K1 * 2;
        // the scratch slots: 512 concurrent sequential streams, written by conv3 and read back by FC1 -- on spread physical pages like the
        // env's observation tensors where the virtual-memory calls work
        constexpr int xg_spread = 16;
        void *xg_ptr = nullptr;
        p->xg_is_spread = xg_spread > 1 && ppg_alloc_spread(device, (uint64_t)xg_bytes, xg_spread, 0x5850u + (uint64_t)R, &xg_ptr) == PPG_OK;
        if (p->xg_is_spread) p->xg = (__bf16 *)xg_ptr;
        if ((!p->xg_is_spread && hipMalloc((void **)&p->xg, xg_bytes) != hipSuccess) || hipMemset(p->xg, 0, xg_bytes) != hipSuccess) {
            (void)ppg_policy_destroy(p);
            return ppg_policy_fail(nullptr, PPG_EHIP, "hipMalloc of %zu bytes of scratch failed", xg_bytes);
        }
        K.xg = p->xg;
    }
    *out = p;
    return PPG_OK;
}

int ppg_policy_pack(const ppg_policy_spec *spec, int32_t what, uint16_t *out, uint64_t capacity, uint64_t *n_words) {
    if (!spec || !n_words) return ppg_policy_fail(nullptr, PPG_EINVAL, "null argument");
    const ppg_policy_spec &sp = *spec;
    const int rc = ppg_policy_check_spec(sp, true);
    if (rc != PPG_OK) return rc;
    const int CIN = sp.layout == PPG_POLICY_LAYOUT_HWC ? sp.obs_range : sp.obs_channels;
    ppg_policy_fragments F;
    int which;
    if (what == PPG_POLICY_PACK_SLOTS) {   // (whatever PPG_POLICY_PIPE says)
        ppg_policy_layout L;
        if (ppg_policy_layout_of(sp, true, L) != PPG_OK || L.family != 3)
            return ppg_policy_fail(nullptr, PPG_EINVAL, "PPG_POLICY_PACK_SLOTS: not a network of the two-role pipeline");
        which = PPG_FRAG_SLOTS;
        F.f[which].swap(L.slot_tab);
    } else {
        if (what >= 0 && what < sp.n_conv) {
            which = what;
        } else if (what == PPG_POLICY_PACK_CONV1X) {
            if (CIN > 9) return ppg_policy_fail(nullptr, PPG_EINVAL, "the pipeline's first convolution takes up to nine input channels (found %d)", CIN);
            which = PPG_FRAG_CONV1X;
        } else if (what == PPG_POLICY_PACK_HEAD) {
            if (sp.n_fc != 1) return ppg_policy_fail(nullptr, PPG_EINVAL, "PPG_POLICY_PACK_HEAD: the network has hidden head layers");
            which = PPG_FRAG_FC;
        } else {
            return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_pack: unknown layer %d", what);
        }
        ppg_policy_fragments_of(sp, F);
    }
    const std::vector<uint16_t> &f = F.f[which];
    *n_words = f.size();
    if (out && capacity >= f.size()) memcpy(out, f.data(), f.size() * 2);
    return PPG_OK;
}

int ppg_policy_image(const ppg_policy_spec *spec, int32_t what, void *out, uint64_t capacity, uint64_t *n_bytes) {
    if (!spec || !n_bytes) return ppg_policy_fail(nullptr, PPG_EINVAL, "null argument");
    const ppg_policy_spec &sp = *spec;
    if (what != PPG_POLICY_IMAGE_PACKED && what != PPG_POLICY_IMAGE_REPACKED && what != PPG_POLICY_IMAGE_MAP)
        return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_image: unknown image kind %d", what);
    int rc = ppg_policy_check_spec(sp, what != PPG_POLICY_IMAGE_MAP);
    if (rc != PPG_OK) return rc;
    ppg_policy_layout L;
    if ((rc = ppg_policy_layout_of(sp, ppg_pipe_enabled(), L)) != PPG_OK) return rc;
    std::vector<int32_t> map;
    std::vector<unsigned char> image;
    ppg_policy_image_layout I;
    if (what != PPG_POLICY_IMAGE_PACKED) ppg_policy_map_of(sp, L.slot_tab.size(), map, I);
    if (what != PPG_POLICY_IMAGE_MAP) {
        ppg_policy_fragments F;
        ppg_policy_fragments_of(sp, F);
        const ppg_policy_image_layout P = ppg_policy_image_layout_of(F, L.slot_tab.size());
        image.resize(P.total);
        ppg_policy_image_assemble(F, P, L.slot_tab.data(), image.data());
        if (what == PPG_POLICY_IMAGE_REPACKED) {   // of the packed image only the slot table's section survives
            if (I.total != P.total || I.off[PPG_FRAG_SLOTS] != P.off[PPG_FRAG_SLOTS] || I.off[PPG_FRAG_N] != P.off[PPG_FRAG_N])
                return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_image: the map and the fragments disagree about the image's layout");
            memset(image.data(), 0xA5, I.off[PPG_FRAG_SLOTS]);
            memset(image.data() + I.off[PPG_FRAG_N], 0xA5, I.total - I.off[PPG_FRAG_N]);
            const ppg_policy_sources S = ppg_policy_sources_of(sp);
            ppg_policy_repack_cpu(map.data(), S.t, image.data());
        }
    }
    const void *from = what == PPG_POLICY_IMAGE_MAP ? (const void *)map.data() : (const void *)image.data();
    *n_bytes = what == PPG_POLICY_IMAGE_MAP ? (uint64_t)map.size() * 4 : (uint64_t)image.size();
    if (out && capacity >= *n_bytes) memcpy(out, from, (size_t)*n_bytes);
    return PPG_OK;
}

// the first field in which spec `b` differs from the shape `a` (NULL: none); `va` / `vb` get the two values
static const char *ppg_policy_shape_diff(const ppg_policy_spec &a, const ppg_policy_spec &b, int *va, int *vb) {
    static char name[32];
#define PPG_SHAPE_FIELD(f) if (a.f != b.f) { *va = a.f; *vb = b.f; return #f; }
    PPG_SHAPE_FIELD(obs_channels) PPG_SHAPE_FIELD(obs_range) PPG_SHAPE_FIELD(n_actions) PPG_SHAPE_FIELD(layout) PPG_SHAPE_FIELD(flatten)
    PPG_SHAPE_FIELD(n_conv) PPG_SHAPE_FIELD(n_fc)
#undef PPG_SHAPE_FIELD
    for (int l = 0; l < a.n_conv; ++l)
        if (a.conv_out[l] != b.conv_out[l]) { *va = a.conv_out[l]; *vb = b.conv_out[l]; snprintf(name, sizeof name, "conv_out[%d]", l); return name; }
    for (int l = 0; l < a.n_fc; ++l)
        if (a.fc_out[l] != b.fc_out[l]) { *va = a.fc_out[l]; *vb = b.fc_out[l]; snprintf(name, sizeof name, "fc_out[%d]", l); return name; }
    return nullptr;
}

int ppg_policy_update(ppg_policy *p, const ppg_policy_spec *spec, void *stream) {
    if (!p) return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_update: the policy is NULL");
    if (!spec) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_update: spec is NULL");
    const ppg_policy_spec &sp = *spec;
    int was = 0, is = 0;
    if (const char *field = ppg_policy_shape_diff(p->shape, sp, &was, &is))
        return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_update: %s is %d, the policy was created with %d", field, is, was);
    for (int l = 0; l < sp.n_conv; ++l)
        if (!sp.conv_w[l] || !sp.conv_b[l]) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_update: a weight pointer of convolution %d is NULL", l + 1);
    for (int l = 0; l < sp.n_fc; ++l)
        if (!sp.fc_w[l] || !sp.fc_b[l]) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_update: a weight pointer of linear layer %d is NULL", l + 1);
    const size_t W = p->image.off[PPG_FRAG_SLOTS] / 2, n_bias = p->image.n_bias;
    if (!p->map_dev) {   // the first update of this policy: build the map and upload it (blocks; not inside a stream capture)
        std::vector<int32_t> map;
        ppg_policy_image_layout I;
        ppg_policy_map_of(p->shape, p->image.words[PPG_FRAG_SLOTS], map, I);
        if (I.total != p->image.total || I.off[PPG_FRAG_SLOTS] != p->image.off[PPG_FRAG_SLOTS] || I.off[PPG_FRAG_N] != p->image.off[PPG_FRAG_N])
            return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_update: the map and the policy disagree about the image's layout");
        const size_t bytes = (W + n_bias) * sizeof(int32_t);
        int32_t *dev = nullptr;
        PPG_POL_TRY(p, hipSetDevice(p->device));
        PPG_POL_TRY(p, hipMalloc((void **)&dev, bytes));
        if (hipMemcpy(dev, map.data() + PPG_MAP_HEADER, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dev);
            return ppg_policy_fail(p, PPG_EHIP, "ppg_policy_update: upload of the repack map failed");
        }
        p->map_dev = dev;
    }
    ppgpol::RepackParams K;
    const ppg_policy_sources S = ppg_policy_sources_of(sp);
    for (int t = 0; t < PPG_SRC_N; ++t) K.src[t] = S.t[t];
    K.map = p->map_dev;
    K.image = (ppgpol::u32x4_t *)p->dev_weights;
    K.bias = (float *)((unsigned char *)p->dev_weights + p->image.off[PPG_FRAG_N]);
    K.n_units = (uint32_t)(W / 8); K.n_bias = (uint32_t)n_bias;
    const uint32_t need = (K.n_units + K.n_bias + 255u) / 256u, most = 8u * (uint32_t)p->cus;   // (eight workgroups of 256 fill a CU's wavefront slots)
    hipLaunchKernelGGL(ppgpol::ppg_policy_repack, dim3(need < most ? need : most), dim3(256), 0, (hipStream_t)stream, K);
    PPG_POL_TRY(p, hipGetLastError());
    return PPG_OK;
}

int ppg_policy_describe(const ppg_policy_spec *spec, int32_t *out, int32_t n) {
    if (!spec || !out || n < 1) return PPG_EINVAL;
    ppg_policy_layout L;
    if (ppg_policy_check_spec(*spec, false) != PPG_OK || ppg_policy_layout_of(*spec, ppg_pipe_enabled(), L) != PPG_OK) return PPG_EINVAL;
    const ppgpol::PolParams &K = L.K;
    int32_t v[12] = {L.family, K.ST, L.lds_bytes, L.threads, 0, 0, 0, 0, 0, 0, 0, 0};
    if (L.family == 3) {   // the pipeline's areas: samples of table, bytes of a sample's region, row loads, byte offsets, bytes of the row area
        v[4] = K.range_tile; v[5] = K.sample_stride * 2; v[6] = K.pipe_ni; v[7] = K.pipe_slots;
        v[8] = K.pipe_red; v[9] = K.pipe_raw; v[10] = K.pipe_img; v[11] = K.pipe_img - 1024 - K.pipe_raw;
    }
    for (int i = 0; i < n && i < 12; ++i) out[i] = v[i];
    return PPG_OK;
}

int ppg_policy_destroy(ppg_policy *p) {
    if (!p) return PPG_OK;
    if (p->dev_weights) (void)hipFree(p->dev_weights);
    if (p->xg) { if (p->xg_is_spread) (void)ppg_free_spread(p->xg); else (void)hipFree(p->xg); }
    if (p->plan) (void)hipFree(p->plan);
    if (p->rows_plan) (void)hipFree(p->rows_plan);
    if (p->rows_actions) (void)hipFree(p->rows_actions);
    if (p->pre_g) (void)hipFree(p->pre_g);
    if (p->lgs) (void)hipFree(p->lgs);
    if (p->map_dev) (void)hipFree(p->map_dev);
    if (p->side) (void)hipStreamDestroy(p->side);
    if (p->fork) (void)hipEventDestroy(p->fork);
    if (p->join) (void)hipEventDestroy(p->join);
    delete p;
    return PPG_OK;
}

uint64_t ppg_policy_macs_per_observation(const ppg_policy *p) { return p ? p->macs : 0; }

const char *ppg_policy_last_error(const ppg_policy *p) { return p ? p->err : g_ppg_policy_error; }

// the plan buffer of a policy: [PLAN_HDR + envs] header + prefix sums, then the first env of every tile
static int ppg_policy_ensure_plan(ppg_policy *p, int total, int cap) {
    size_t max_tiles = ((size_t)total * cap + 31) / 32 + 1;   // (tiles of 32 samples are the smallest the plan picks)
    if (p->direct) {   // range mode: grid x tiles-per-workgroup slots, some of them empty
        const size_t share = ((size_t)total * cap + p->grid - 1) / p->grid + (size_t)p->base.ST;
        const size_t slots = (size_t)p->grid * ((share + p->base.range_tile - 1) / p->base.range_tile + 1);
        if (slots > max_tiles) max_tiles = slots;
    }
    // the tile list starts right behind the prefix sums of `total` envs: a buffer is reused only for the same env count and at most
    // the tile slots it was sized for (handles with the same env count but a larger row capacity need more slots: ADVICE r4)
    const size_t words = (size_t)(ppgpol::PLAN_HDR + total) + max_tiles;
    if (p->plan && p->plan_envs == total && p->plan_words >= words) return PPG_OK;
    if (p->plan) (void)hipFree(p->plan);
    p->plan = nullptr;
    p->plan_envs = 0; p->plan_words = 0;
    PPG_POL_TRY(p, hipMalloc((void **)&p->plan, words * 4));
    p->plan_envs = total;
    p->plan_words = words;
    return PPG_OK;
}
// ... and where a parameter block (PolParams or PlanParams) finds the two parts of such a buffer
extern "C++" template <class Params, class Word>
static void ppg_policy_bind_plan(Params &K, Word *plan, int n_envs) {
    K.plan = plan;
    K.tile_env = plan + ppgpol::PLAN_HDR + n_envs;
}

// the plan mode of a policy's forward kernels as the plan kernels take it: range_tile > 0 = range mode with sub-groups of range_st
static void ppg_policy_plan_mode(int direct, const ppgpol::PolParams &K, uint32_t &range_tile, uint32_t &range_st) {
    range_tile = direct ? (uint32_t)K.range_tile : 0u;
    range_st = (uint32_t)K.ST;
}

// The plan launch's parameters for policy `p` over the envs a filled block K lists: the species' row-count word of env_state, p's grid
// and plan mode, p's plan buffer (ppg_policy_ensure_plan has sized it for these envs).
static ppgpol::PlanParams ppg_policy_plan_params(const ppg_policy *p, int word, const ppgpol::PolParams &K) {
    ppgpol::PlanParams L;
    memset(&L, 0, sizeof L);
    L.n_handles = K.n_handles; L.n_envs = K.n_envs; L.word = word;
    L.slots = p->grid;
    uint32_t range_tile, range_st;
    ppg_policy_plan_mode(p->direct, p->base, range_tile, range_st);
    L.range_tile = (int32_t)range_tile; L.range_st = (int32_t)range_st;
    memcpy(L.env_base, K.env_base, sizeof L.env_base);
    memcpy(L.env_state, K.env_state, sizeof L.env_state);
    ppg_policy_bind_plan(L, p->plan, K.n_envs);
    return L;
}

// ---- the diagnostic builds' part of the launch path ----
// ppg_policy_run and ppg_policy_run_fused call ppg_policy_diag_before() ahead of their launches and ppg_policy_diag_after() behind the
// hipGetLastError() that follows them: arm, launch, hipGetLastError, check or write.  The product build's versions are empty.
#if defined(PPG_PIPE_DEBUG) || defined(PPG_EXPERIMENTS) || defined(PPG_DIRECT_PROFILE)
#ifdef PPG_PIPE_DEBUG
// diagnostic build: status words the pipeline kernels' bounded waits report into; checked (with a device synchronisation) after every
// launch.  PPG_PIPE_DEBUG_INJECT=1 (tests): pretend a report, to exercise the path that turns it into an error.
static uint32_t *g_pipe_status_host = nullptr;
static int ppg_pipe_debug_arm(ppg_policy *p) {
    if (!g_pipe_status_host) {
        PPG_POL_TRY(p, hipMalloc((void **)&g_pipe_status_host, 32));
        PPG_POL_TRY(p, hipMemcpyToSymbol(HIP_SYMBOL(ppgpol::g_pipe_status), &g_pipe_status_host, sizeof(uint32_t *)));
    }
    PPG_POL_TRY(p, hipMemset(g_pipe_status_host, 0, 32));
    return PPG_OK;
}
static int ppg_pipe_debug_check(ppg_policy *p) {
    uint32_t st[8];
    PPG_POL_TRY(p, hipDeviceSynchronize());
    PPG_POL_TRY(p, hipMemcpy(st, g_pipe_status_host, 32, hipMemcpyDeviceToHost));
    if (getenv("PPG_PIPE_DEBUG_INJECT")) { st[0] = 1; st[1] = 7; st[2] = 5; st[3] = 11; st[4] = 12; }
    if (st[0])
        return ppg_policy_fail(p, PPG_EHIP, "pipeline barrier: %u wavefront(s) gave up waiting; first: workgroup %u wavefront %u saw counter %u, wanted %u",
                               st[0], st[1], st[2], st[3], st[4]);
    return PPG_OK;
}
#endif

#if defined(PPG_EXPERIMENTS) || defined(PPG_DIRECT_PROFILE)
// diagnostic builds: a device buffer that ONE launch of a kind fills with stamps -- allocated (zeroed) at the first launch with $path_env
// set, handed to launch number $run_env (default 300), and after that launch written to the file "$path_env.<suffix>"
struct ppg_policy_dump {
    const char *path_env, *run_env;
    unsigned long long *buf;
    int runs;
    bool armed;   // the launch being prepared is the one
};
static int ppg_policy_dump_arm(ppg_policy *p, ppg_policy_dump &d, size_t bytes, void **slot) {   // *slot: the parameter block's pointer
    const char *path = getenv(d.path_env), *at = getenv(d.run_env);
    if (path && !d.buf) {
        PPG_POL_TRY(p, hipMalloc((void **)&d.buf, bytes));
        PPG_POL_TRY(p, hipMemset(d.buf, 0, bytes));
        PPG_POL_TRY(p, hipDeviceSynchronize());
    }
    d.armed = path && ++d.runs == (at ? atoi(at) : 300);
    *slot = d.armed ? d.buf : nullptr;
    return PPG_OK;
}
static int ppg_policy_dump_write(ppg_policy *p, const ppg_policy_dump &d, size_t bytes, const char *suffix) {
    if (!d.buf) return PPG_OK;
    PPG_POL_TRY(p, hipDeviceSynchronize());
    std::vector<unsigned long long> host(bytes / 8);
    PPG_POL_TRY(p, hipMemcpy(host.data(), d.buf, bytes, hipMemcpyDeviceToHost));
    char name[512];
    snprintf(name, sizeof name, "%s.%s", getenv(d.path_env), suffix);
    if (FILE *f = fopen(name, "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
    return PPG_OK;
}
#endif
#ifdef PPG_EXPERIMENTS   // PPG_POLICY_TIMELINE=<file prefix>: per-tile phase stamps of launch number PPG_POLICY_TIMELINE_RUN of each species -> <prefix>.{pred,prey}
static ppg_policy_dump g_ppg_timeline[2] = {{"PPG_POLICY_TIMELINE", "PPG_POLICY_TIMELINE_RUN"}, {"PPG_POLICY_TIMELINE", "PPG_POLICY_TIMELINE_RUN"}};
#endif
#ifdef PPG_DIRECT_PROFILE   // per-wavefront phase cycles of launch number PPG_DIRECT_PROFILE_RUN -> $PPG_DIRECT_PROFILE_FILE.{pred,prey,fused}
static ppg_policy_dump g_ppg_direct_profile[3] = {{"PPG_DIRECT_PROFILE_FILE", "PPG_DIRECT_PROFILE_RUN"}, {"PPG_DIRECT_PROFILE_FILE", "PPG_DIRECT_PROFILE_RUN"},
                                                  {"PPG_DIRECT_PROFILE_FILE", "PPG_DIRECT_PROFILE_RUN"}};
// [workgroup][wavefront][16] (the pipeline kernels have eight wavefronts, the others use the first half)
static size_t ppg_direct_profile_bytes(const ppg_policy *p) { return (size_t)p->grid * 8 * 16 * 8; }
#endif
#ifdef PPG_EXPERIMENTS
static size_t ppg_timeline_bytes(const ppgpol::PolParams &K, int total) { return (((size_t)total * K.cap + 31) / 32 + 1) * 512; }   // [tile][64] stamps
#endif
// launch: 0 the predators' launch, 1 the prey's, 2 the fused launch of both (K: the prey's block, K_also: the predators')
static int ppg_policy_diag_before(ppg_policy *p, int launch, int total, ppgpol::PolParams &K, ppgpol::PolParams *K_also) {
    int rc = PPG_OK;
#ifdef PPG_EXPERIMENTS
    if (launch < 2 && (rc = ppg_policy_dump_arm(p, g_ppg_timeline[launch], ppg_timeline_bytes(K, total), (void **)&K.timeline)) != PPG_OK) return rc;
#endif
#ifdef PPG_DIRECT_PROFILE   // (the FC chain's kernels write no profile: K.xg is their scratch)
    if (p->direct) {
        if ((rc = ppg_policy_dump_arm(p, g_ppg_direct_profile[launch], ppg_direct_profile_bytes(p), (void **)&K.xg)) != PPG_OK) return rc;
        if (K_also) K_also->xg = K.xg;
    }
#endif
#ifdef PPG_PIPE_DEBUG
    if (p->direct && (rc = ppg_pipe_debug_arm(p)) != PPG_OK) return rc;
#endif
    (void)launch; (void)total; (void)K; (void)K_also;
    return rc;
}
static int ppg_policy_diag_after(ppg_policy *p, int launch, int total, const ppgpol::PolParams &K) {
    int rc = PPG_OK;
#ifdef PPG_PIPE_DEBUG
    if (p->direct && (rc = ppg_pipe_debug_check(p)) != PPG_OK) return rc;
#endif
#ifdef PPG_DIRECT_PROFILE
    static const char *const suffix[3] = {"pred", "prey", "fused"};
    if (p->direct && g_ppg_direct_profile[launch].armed)
        if ((rc = ppg_policy_dump_write(p, g_ppg_direct_profile[launch], ppg_direct_profile_bytes(p), suffix[launch])) != PPG_OK) return rc;
#endif
#ifdef PPG_EXPERIMENTS
    for (int sp = 0; sp < 2 && launch == 0 && g_ppg_timeline[0].armed; ++sp)   // (the predators' launch is the second of a step: it writes both species' stamps)
        if ((rc = ppg_policy_dump_write(p, g_ppg_timeline[sp], ppg_timeline_bytes(K, total), sp ? "prey" : "pred")) != PPG_OK) return rc;
#endif
    (void)launch; (void)total; (void)K;
    return rc;
}
#else
static inline int ppg_policy_diag_before(ppg_policy *, int, int, ppgpol::PolParams &, ppgpol::PolParams *) { return PPG_OK; }
static inline int ppg_policy_diag_after(ppg_policy *, int, int, const ppgpol::PolParams &) { return PPG_OK; }
#endif

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the process-global kernel symbol, not of a policy: two live policies that
// share a kernel (say two pipe8 policies with different windows) need different amounts.  A running maximum per kernel is kept and raised
// right before the launch that needs more; the return code is checked.
static int ppg_policy_reserve_lds(ppg_policy *p, const void *fn, int bytes) {
    static const void *fns[256];   // (kernel, device): the attribute belongs to the code object loaded on a device
    static int devs[256], have[256];
    static int n_fns = 0;
    int i = 0;
    while (i < n_fns && !(fns[i] == fn && devs[i] == p->device)) ++i;
    if (i == n_fns) {
        if (n_fns == 256) return ppg_policy_fail(p, PPG_EHIP, "internal: more than 256 (policy kernel, device) pairs");
        fns[n_fns] = fn; devs[n_fns] = p->device; have[n_fns] = 0; ++n_fns;
    }
    if (have[i] >= bytes) return PPG_OK;
    PPG_POL_TRY(p, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have[i] = bytes;
    return PPG_OK;
}

// What every call sets in its copy of p->base whatever its rows come from -- species, row dtype, sampling and its key, the logits, the
// env count behind the last handle -- and the switch to the policy's device.
static int ppg_policy_fill_call(ppg_policy *p, ppgpol::PolParams &K, int species, int obs_dtype, uint32_t flags, uint64_t seed, float *logits,
                                int n_handles, int total) {
    K.species = species; K.obs_f32 = obs_dtype; K.sample = (flags & PPG_POLICY_SAMPLE) ? 1 : 0;
    K.seed_lo = (uint32_t)seed ^ (species ? 0x9E3779B9u : 0u); K.seed_hi = (uint32_t)(seed >> 32);
    K.seed_dev = (flags & PPG_POLICY_SEED_ON_DEVICE) ? (const uint64_t *)(uintptr_t)seed : nullptr;
    K.n_handles = n_handles;
    for (int k = n_handles; k <= ppgpol::MAX_HANDLES; ++k) K.env_base[k] = total;
    K.n_envs = total;
    K.logits = logits;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != p->device) PPG_POL_TRY(p, hipSetDevice(p->device));
    return PPG_OK;
}

// The per-call part of a species' parameter block: what the handles, the action tensors and the flags decide (no plan, no launch).
static int ppg_policy_fill(ppg_policy *p, int species, ppg_handle *const *handles, int32_t n, int8_t *const *actions, uint32_t flags,
                           uint64_t seed, float *logits, ppgpol::PolParams &K, int &total) {
    ppg_handle *h0 = handles[0];
    const int R = species ? h0->base.Rq : h0->base.Rp;
    if (R != p->R) return ppg_policy_fail(p, PPG_EINVAL, "the policy was created for %dx%d observations, the %s observe %dx%d", p->R, p->R,
                                          species ? "prey" : "predators", R, R);
    if (p->n_actions != 9 && !h0->gen2) return ppg_policy_fail(p, PPG_EINVAL, "the base env has 9 actions, the policy %d", p->n_actions);
    K = p->base;
    K.S = h0->base.S; K.cap = species ? h0->base.cap_prey : h0->base.cap_pred; K.slot0 = species ? h0->base.cap_pred : 0;
    total = 0;
    for (int k = 0; k < n; ++k) {
        const ppg_handle *h = handles[k];
        if (!h) return ppg_policy_fail(p, PPG_EINVAL, "handle %d is NULL", k);
        const int channels = h->drive ? 4 + h->cfg.n_drive[species] : (h->gen2 && h->cfg2.walls && h->cfg2.include_visibility_channel) ? 5 : 4;
        if (channels != p->obs_channels)
            return ppg_policy_fail(p, PPG_EINVAL, "the policy reads %d-channel observations, handle %d writes %d channels", p->obs_channels, k, channels);
        if ((species ? h->base.Rq : h->base.Rp) != R || h->base.S != K.S || h->base.obs_f32 != h0->base.obs_f32 || h->device != p->device)
            return ppg_policy_fail(p, PPG_EINVAL, "handle %d has another geometry / dtype / device than handle 0", k);
        if (!actions[k]) return ppg_policy_fail(p, PPG_EINVAL, "actions[%d] is NULL", k);
        K.env_base[k] = total;
        total += h->batch;
        K.env_state[k] = h->bufs.env_state;
        K.obs[k] = (const unsigned char *)(species ? h->bufs.obs_prey : h->bufs.obs_pred);
        K.actions[k] = actions[k];
    }
    return ppg_policy_fill_call(p, K, species, h0->base.obs_f32, flags, seed, logits, n, total);
}

static int ppg_policy_forward(ppg_policy *p, const ppgpol::PolParams &K, void *stream);

// also_plan_for: the OTHER species' policy whose plan this call's plan launch computes as well (ppg_policy_plan2); skip_plan: this
// species' plan was computed by the other call
static int ppg_policy_run(ppg_policy *p, int species, ppg_handle *const *handles, int32_t n, int8_t *const *actions, uint32_t flags,
                          uint64_t seed, float *logits, void *stream, ppg_policy *also_plan_for = nullptr, bool skip_plan = false) {
    ppg_handle *h0 = handles[0];
    ppgpol::PolParams K;
    int total = 0;
    int rc = ppg_policy_fill(p, species, handles, n, actions, flags, seed, logits, K, total);
    if (rc != PPG_OK) return rc;
    if (K.obs_f32 == 3)
        return ppg_policy_fail(p, PPG_EINVAL, "observation rows in the cell layout (obs_dtype 3) need the one-launch form: both species' pipeline policies in one ppg_policy_act call");
    if ((rc = ppg_policy_ensure_plan(p, total, K.cap)) != PPG_OK) return rc;
    ppg_policy_bind_plan(K, p->plan, total);
    const int word[2] = {PPG_ENV_N_PRED_ROWS, PPG_ENV_N_PREY_ROWS};
    const ppgpol::PlanParams L = ppg_policy_plan_params(p, word[species], K);
    if ((rc = ppg_policy_diag_before(p, species, total, K, nullptr)) != PPG_OK) return rc;
    if (also_plan_for) {   // the other species' plan in the same launch: same envs, its row-count word, its buffers, its grid
        ppg_policy *o = also_plan_for;
        rc = ppg_policy_ensure_plan(o, total, species ? h0->base.cap_pred : h0->base.cap_prey);
        if (rc != PPG_OK) { memcpy(p->err, o->err, sizeof p->err); return rc; }
        hipLaunchKernelGGL(ppgpol::ppg_policy_plan2, dim3(2), dim3(1024), 0, (hipStream_t)stream, L, ppg_policy_plan_params(o, word[!species], K));
    } else if (!skip_plan) {
        hipLaunchKernelGGL(p->direct ? ppgpol::ppg_policy_plan : ppgpol::ppg_policy_plan_small, dim3(1), dim3(1024), 0, (hipStream_t)stream, L);
    }
    if ((rc = ppg_policy_forward(p, K, stream)) != PPG_OK) return rc;   // (its hipGetLastError() speaks for the plan launch too)
    return ppg_policy_diag_after(p, species, total, K);
}

// the single-species forward launch of a filled parameter block: the kernel family, input-channel variant and row dtype pick the kernel
static int ppg_policy_forward(ppg_policy *p, const ppgpol::PolParams &K, void *stream) {
    int rc;
    typedef void (*fwd_fn)(const ppgpol::PolParams);
    const fwd_fn fwd[3][3] = {{ppgpol::ppg_policy_forward_f64, ppgpol::ppg_policy_forward_f32, ppgpol::ppg_policy_forward_bf16},
                              {ppgpol::ppg_policy_forward_hwc8_f64, ppgpol::ppg_policy_forward_hwc8_f32, ppgpol::ppg_policy_forward_hwc8_bf16},
                              {ppgpol::ppg_policy_forward_hwc16_f64, ppgpol::ppg_policy_forward_hwc16_f32, ppgpol::ppg_policy_forward_hwc16_bf16}};
    const int dt = K.obs_f32 == 2 ? 2 : K.obs_f32 ? 1 : 0;
    if (p->direct) {
        const fwd_fn dir[4][3] = {{ppgpol::ppg_policy_direct8_f64, ppgpol::ppg_policy_direct8_f32, ppgpol::ppg_policy_direct8_bf16},
                                  {ppgpol::ppg_policy_direct16_f64, ppgpol::ppg_policy_direct16_f32, ppgpol::ppg_policy_direct16_bf16},
                                  {ppgpol::ppg_policy_deep8_f64, ppgpol::ppg_policy_deep8_f32, ppgpol::ppg_policy_deep8_bf16},
                                  {ppgpol::ppg_policy_deep16_f64, ppgpol::ppg_policy_deep16_f32, ppgpol::ppg_policy_deep16_bf16}};
        const fwd_fn pipe[2][3] = {{ppgpol::ppg_policy_pipe8_f64, ppgpol::ppg_policy_pipe8_f32, ppgpol::ppg_policy_pipe8_bf16},
                                   {ppgpol::ppg_policy_pipe16_f64, ppgpol::ppg_policy_pipe16_f32, ppgpol::ppg_policy_pipe16_bf16}};
        const fwd_fn fn = p->pipe ? pipe[p->nch16 ? 1 : 0][dt] : dir[(p->direct == 2 ? 2 : 0) + (p->nch16 ? 1 : 0)][dt];
        if ((rc = ppg_policy_reserve_lds(p, (const void *)fn, p->lds_bytes)) != PPG_OK) return rc;
        hipLaunchKernelGGL(fn, dim3((unsigned)p->grid), dim3(p->pipe ? 512 : 256), (size_t)p->lds_bytes, (hipStream_t)stream, K);
    } else {
        const int variant = p->layout == PPG_POLICY_LAYOUT_HWC ? (p->cin > 8 ? 2 : 1) : 0;
        if ((rc = ppg_policy_reserve_lds(p, (const void *)fwd[variant][dt], p->lds_bytes)) != PPG_OK) return rc;
        hipLaunchKernelGGL(fwd[variant][dt], dim3((unsigned)p->grid), dim3(256), (size_t)p->lds_bytes, (hipStream_t)stream, K);
    }
    PPG_POL_TRY(p, hipGetLastError());
    return PPG_OK;
}

// diagnostic switch: environment variable PPG_POLICY_FUSED=0 sends a call with both species' pipeline policies through the two
// forward launches + plan launch of rounds 2-4 instead of the one fused launch (tests compare the two bit for bit)
static bool ppg_fused_enabled() {
    const char *e = getenv("PPG_POLICY_FUSED");
    return !(e && e[0] == '0' && e[1] == 0);
}

static int ppg_env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return (e && atoi(e) > 0) ? atoi(e) : dflt;
}

// Both species' pipeline policies in ONE launch and no plan launch (ppg_policy_pipe.h: fused_main).  Returns 1 if this call cannot
// take that path (the caller then runs the separate launches), PPG_OK after the launch, or an error.
static int ppg_policy_run_fused(ppg_policy *pred, ppg_policy *prey, ppg_handle *const *handles, int32_t n, int8_t *const *actions,
                                uint32_t flags, uint64_t seed, float *logits_pred, float *logits_prey, void *stream) {
    ppgpol::PolParams2 K2;
    int total_q = 0, total_p = 0;
    int rc = ppg_policy_fill(prey, 1, handles, n, actions, flags, seed, logits_prey, K2.q, total_q);
    if (rc != PPG_OK) return ppg_policy_mirror(prey, rc);
    rc = ppg_policy_fill(pred, 0, handles, n, actions, flags, seed, logits_pred, K2.p, total_p);
    if (rc != PPG_OK) return ppg_policy_mirror(pred, rc);
    const int lds = prey->lds_bytes > pred->lds_bytes ? prey->lds_bytes : pred->lds_bytes;
    const int img = K2.q.pipe_img > K2.p.pipe_img ? K2.q.pipe_img : K2.p.pipe_img;
    K2.scratch_off = (img + 15) / 16 * 16;
    if (total_q > ppgpol::FUSED_MAX_ENVS || K2.scratch_off + ppgpol::FUSED_PART_WORDS * 4 + 8 * total_q > lds) return 1;
    K2.q.plan = K2.p.plan = nullptr; K2.q.tile_env = K2.p.tile_env = nullptr;
    if (!prey->pre_g) PPG_POL_TRY(prey, hipMalloc((void **)&prey->pre_g, (size_t)2 * ppgpol::FUSED_MAX_ENVS * 4));
    K2.pre_g = prey->pre_g;
    // cycles per pipeline iteration of either network (measured on the reference's shapes, profiles/r04-r05; PPG_POLICY_ITER_Q / _P:
    // experiments): only their RATIO matters -- it decides how many workgroups serve which species
    K2.iter_q = ppg_env_int("PPG_POLICY_ITER_Q", 7500);
    K2.iter_p = ppg_env_int("PPG_POLICY_ITER_P", 8500);
    typedef void (*fused_fn)(const ppgpol::PolParams2);
    const fused_fn fn[2][2][3] = {
        {{ppgpol::ppg_policy_pipe2_8_8_f64, ppgpol::ppg_policy_pipe2_8_8_f32, ppgpol::ppg_policy_pipe2_8_8_bf16},
         {ppgpol::ppg_policy_pipe2_8_16_f64, ppgpol::ppg_policy_pipe2_8_16_f32, ppgpol::ppg_policy_pipe2_8_16_bf16}},
        {{ppgpol::ppg_policy_pipe2_16_8_f64, ppgpol::ppg_policy_pipe2_16_8_f32, ppgpol::ppg_policy_pipe2_16_8_bf16},
         {ppgpol::ppg_policy_pipe2_16_16_f64, ppgpol::ppg_policy_pipe2_16_16_f32, ppgpol::ppg_policy_pipe2_16_16_bf16}}};
    const int dt = K2.q.obs_f32 == 2 ? 2 : K2.q.obs_f32 ? 1 : 0;
    const fused_fn f = fn[prey->nch16 ? 1 : 0][pred->nch16 ? 1 : 0][dt];
    if ((rc = ppg_policy_reserve_lds(prey, (const void *)f, lds)) != PPG_OK) return ppg_policy_mirror(prey, rc);
    if ((rc = ppg_policy_diag_before(prey, 2, total_q, K2.q, &K2.p)) != PPG_OK) return ppg_policy_mirror(prey, rc);
    hipLaunchKernelGGL(f, dim3((unsigned)prey->grid), dim3(512), (size_t)lds, (hipStream_t)stream, K2);
    PPG_POL_TRY(prey, hipGetLastError());
    return ppg_policy_mirror(prey, ppg_policy_diag_after(prey, 2, total_q, K2.q));
}

int ppg_policy_act(ppg_policy *pred, ppg_policy *prey, ppg_handle *const *handles, int32_t n, int8_t *const *actions,
                   uint32_t flags, uint64_t seed, float *logits_pred, float *logits_prey, void *stream) {
    ppg_policy *any = pred ? pred : prey;
    if (!any) return PPG_EINVAL;
    if (!handles || !actions || n < 1 || n > ppgpol::MAX_HANDLES || !handles[0]) return ppg_policy_fail(any, PPG_EINVAL, "bad handle list");
    if (flags & ~(PPG_POLICY_SAMPLE | PPG_POLICY_SEED_ON_DEVICE)) return ppg_policy_fail(any, PPG_EINVAL, "unknown policy flags 0x%x", flags);
    for (int32_t k = 0; k < n; ++k)   // (the policy kernels read 64 predator rows per env)
        if (handles[k] && handles[k]->base.cap_pred != 64)
            return ppg_policy_mirror(any, ppg_policy_fail(any, PPG_EINVAL, "handle %d has %d predator rows; the policy kernels take handles with 64", k,
                                                          handles[k]->base.cap_pred));
    if (pred && prey && pred->pipe && prey->pipe && pred->device == prey->device && pred->grid == prey->grid && ppg_fused_enabled()) {
        const int rc = ppg_policy_run_fused(pred, prey, handles, n, actions, flags, seed, logits_pred, logits_prey, stream);
        if (rc != 1) return rc;
    }
    if (flags & PPG_POLICY_SEED_ON_DEVICE)
        return ppg_policy_fail(any, PPG_EINVAL, "PPG_POLICY_SEED_ON_DEVICE is for the one-launch form: both species' pipeline policies on one device");
    // The predators are few (a third of the chip's workgroup slots at 4096 envs): their launch goes to a side stream that is
    // forked from and joined back into `stream` with events, so that it fills the CUs the prey launch leaves idle.
    void *pred_stream = stream;
    // (direct-head networks: every workgroup needs a whole CU's LDS, so the two launches cannot share CUs -- a side stream only adds two
    //  cross-stream event waits; they run back to back on the caller's stream)
    const bool side = pred && prey && !(pred->direct && prey->direct);
    if (side) {
        if (!pred->side) {
            PPG_POL_TRY(pred, hipStreamCreateWithFlags(&pred->side, hipStreamNonBlocking));
            PPG_POL_TRY(pred, hipEventCreateWithFlags(&pred->fork, hipEventDisableTiming));
            PPG_POL_TRY(pred, hipEventCreateWithFlags(&pred->join, hipEventDisableTiming));
        }
        PPG_POL_TRY(pred, hipEventRecord(pred->fork, (hipStream_t)stream));
        PPG_POL_TRY(pred, hipStreamWaitEvent(pred->side, pred->fork, 0));
        pred_stream = pred->side;
    }
    const bool one_plan = pred && prey && !side;   // (same stream: the prey call's plan launch computes the predators' plan too)
    if (prey) {
        const int rc = ppg_policy_run(prey, 1, handles, n, actions, flags, seed, logits_prey, stream, one_plan ? pred : nullptr);
        if (rc != PPG_OK) return ppg_policy_mirror(prey, rc);
    }
    if (pred) {
        const int rc = ppg_policy_run(pred, 0, handles, n, actions, flags, seed, logits_pred, pred_stream, nullptr, one_plan);
        if (rc != PPG_OK) return ppg_policy_mirror(pred, rc);
    }
    if (side) {
        PPG_POL_TRY(pred, hipEventRecord(pred->join, pred->side));
        PPG_POL_TRY(pred, hipStreamWaitEvent((hipStream_t)stream, pred->join, 0));
    }
    return PPG_OK;
}

// The network over a dense row tensor (include/ppg.h).  The rows are one "handle" of ceil(capacity / CH) pseudo-envs with S = cap = CH
// and slot0 = 0: the forward kernels' addresses are then linear in the sample number (ppg_policy_plan.h).  The kernels, their constant
// parameters (p->base) and their selection are ppg_policy_run's; the plan comes from ppg_policy_plan_rows into a buffer of its own.
int ppg_policy_evaluate(ppg_policy *p, const ppg_policy_rows *rows, void *stream) {
    if (!p) return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_evaluate: the policy is NULL");
    if (!rows) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_evaluate: rows is NULL");
    const ppg_policy_rows &r = *rows;
    if (r.capacity < 0 || r.capacity > PPG_ROWS_MAX)
        return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_evaluate: capacity %lld is outside [0, %lld]", (long long)r.capacity, (long long)PPG_ROWS_MAX);
    if (r.obs_dtype == 3) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_evaluate: rows in the cell layout (obs_dtype 3) are not taken");
    if (r.obs_dtype < 0 || r.obs_dtype > 2)
        return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_evaluate: unknown obs_dtype %d (0 float64, 1 float32, 2 bfloat16)", r.obs_dtype);
    if (r.capacity > 0 && (!r.obs || !r.out)) return ppg_policy_fail(p, PPG_EINVAL, "ppg_policy_evaluate: %s is NULL", r.obs ? "out" : "obs");
    if (r.capacity == 0 || (!r.count_dev && r.count <= 0)) return PPG_OK;
    const uint32_t n_envs = ppg_rows_envs(r.capacity);
    ppgpol::PolParams K = p->base;   // (no env_state, and obs / actions of handle 0 only: the rest stays NULL)
    const int rc = ppg_policy_fill_call(p, K, 0, r.obs_dtype, 0u, 0u, r.out, 1, (int)n_envs);
    if (rc != PPG_OK) return rc;
    uint32_t range_tile, range_st;
    ppg_policy_plan_mode(p->direct, p->base, range_tile, range_st);
    if (r.capacity > p->rows_capacity) {   // (grows only: a call at a smaller capacity lays its plan out inside the same buffer)
        if (p->rows_plan) (void)hipFree(p->rows_plan);
        if (p->rows_actions) (void)hipFree(p->rows_actions);
        p->rows_plan = nullptr; p->rows_actions = nullptr; p->rows_capacity = 0;
        const size_t words = (size_t)ppgpol::PLAN_HDR + ppg_rows_envs(r.capacity) + ppg_rows_max_tile_words(r.capacity, (uint32_t)p->grid, range_tile, range_st);
        PPG_POL_TRY(p, hipMalloc((void **)&p->rows_plan, words * 4));
        PPG_POL_TRY(p, hipMalloc((void **)&p->rows_actions, (size_t)ppg_rows_envs(r.capacity) * PPG_ROWS_CH));
        p->rows_capacity = r.capacity;
    }
    ppgpol::RowsPlanParams L;
    L.capacity = r.capacity; L.count = r.count; L.count_dev = r.count_dev;
    L.slots = (uint32_t)p->grid; L.range_tile = range_tile; L.range_st = range_st;
    L.plan = p->rows_plan;
    K.S = K.cap = (int32_t)PPG_ROWS_CH; K.slot0 = 0;
    K.env_base[0] = 0;
    K.obs[0] = (const unsigned char *)r.obs;
    K.actions[0] = p->rows_actions;
    ppg_policy_bind_plan(K, p->rows_plan, (int)n_envs);
    const size_t tile_words = ppg_rows_max_tile_words(r.capacity, (uint32_t)p->grid, range_tile, range_st);
    const size_t items = tile_words > n_envs ? tile_words : (size_t)n_envs;
    const size_t blocks = (items + 255) / 256;
    hipLaunchKernelGGL(ppgpol::ppg_policy_plan_rows, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, L);
    return ppg_policy_forward(p, K, stream);
}

int ppg_policy_rows_plan(const ppg_policy_spec *spec, int32_t slots, int64_t capacity, int64_t count, uint32_t *out,
                         uint64_t capacity_words, uint64_t *n_words) {
    if (!spec || !n_words) return ppg_policy_fail(nullptr, PPG_EINVAL, "null argument");
    int rc = ppg_policy_check_spec(*spec, false);
    if (rc != PPG_OK) return rc;
    ppg_policy_layout L;
    if ((rc = ppg_policy_layout_of(*spec, ppg_pipe_enabled(), L)) != PPG_OK) return rc;
    uint32_t range_tile, range_st;
    ppg_policy_plan_mode(L.family != 0, L.K, range_tile, range_st);
    if (!ppg_rows_plan_cpu(capacity, count, slots, (int32_t)range_tile, (int32_t)range_st, out, capacity_words, n_words))
        return ppg_policy_fail(nullptr, PPG_EINVAL, "ppg_policy_rows_plan: slots %d / capacity %lld: slots >= 1, capacity in [0, %lld]", slots,
                               (long long)capacity, (long long)PPG_ROWS_MAX);
    return PPG_OK;
}

}  // extern "C"
