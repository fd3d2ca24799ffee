// ppg_learner_host.h -- the host side of the learner calls (include/ppg.h): ppg_pack, ppg_fetch, ppg_link, ppg_record,
// ppg_record_obs, ppg_record_logp, ppg_backward, ppg_backward_samples, ppg_ppo_loss and ppg_net_bytes / ppg_net_forward /
// ppg_net_backward -- their argument checks, parameter blocks and launches.  The kernels are the headers included below; the handle,
// the env-side calls and the backend seam are ppg_host.h, which includes this file at its end.
#pragma once

#include "ppg_pack.h"
#include "ppg_fetch.h"
#include "ppg_link.h"
#include "ppg_record.h"
#include "ppg_backward.h"
#include "ppg_obs_store.h"
#include "ppg_logp.h"
#include "ppg_ppo.h"
#include "ppg_net.h"
#include "ppg_policy_shape.h"

// the two launches of ppg_pack (ppg_pack.h)
static int backend_pack(ppg_handle *h, const ppg::PackParams &K, void *stream);
// the launch of ppg_fetch (ppg_fetch.h)
static int backend_fetch(ppg_handle *h, const ppg::FetchParams &K, void *stream);
// the launches of ppg_link (ppg_link.h), ppg_record (ppg_record.h), ppg_record_obs (ppg_obs_store.h: two), ppg_record_logp
// (ppg_logp.h: two), ppg_backward and ppg_backward_samples (ppg_backward.h), ppg_ppo_loss (ppg_ppo.h: two), ppg_net_forward (ppg_net.h:
// one launch of K.G workgroups of NET_THREADS threads with lds_bytes of dynamic LDS) and ppg_net_backward (two)
static int backend_link(ppg_handle *h, const ppg::LinkParams &K, void *stream);
static int backend_record(ppg_handle *h, const ppg::RecordParams &K, void *stream);
static int backend_record_obs(ppg_handle *h, const ppg::ObsStoreParams &K, void *stream);
static int backend_record_logp(ppg_handle *h, const ppg::LogpParams &K, void *stream);
static int backend_backward(ppg_handle *h, const ppg::BackwardParams &K, void *stream);
static int backend_backward_samples(ppg_handle *h, const ppg::BackwardSamplesParams &K, void *stream);
static int backend_ppo_loss(ppg_handle *h, const ppg::PpoParams &K, void *stream);
static int backend_net_forward(ppg_handle *h, const ppg::NetParams &K, int lds_bytes, void *stream);
static int backend_net_backward(ppg_handle *h, const ppg::NetParams &K, int lds_bytes, void *stream);
#ifdef PPG_WAVE_EMU
// CPU test build (tests/wave_emu): `grid` one-wave workgroups of Main with exactly LDS bytes each, as on the device.  These nine
// launches stand here, not next to the test backend's backend_pack / backend_fetch: a revision's test suite is also run against
// the sources of the revision after it, and its tests/wave_emu/ppg_emu.cpp defines only the launches that existed when it was written.
template <class P, void (*Main)(const P &, unsigned char *), int LDS>
static int ppg_emu_rows(const P &K, int grid) {
    for (int b = 0; b < grid; ++b)
        wv::run_block([](void *arg) { Main(*(const P *)arg, wv::emu().lds); }, (void *)&K, b, LDS, 1);
    return PPG_OK;
}
template <class P, void (*Main)(const P &)>   // (a main that takes no LDS)
static int ppg_emu_rows(const P &K, int grid) {
    for (int b = 0; b < grid; ++b) wv::run_block([](void *arg) { Main(*(const P *)arg); }, (void *)&K, b, 16, 1);
    return PPG_OK;
}
static int backend_link(ppg_handle *, const ppg::LinkParams &K, void *) { return ppg_emu_rows<ppg::LinkParams, ppg::link_main, ppg::LINK_LDS_BYTES>(K, K.batch); }
static int backend_record(ppg_handle *, const ppg::RecordParams &K, void *) {
    return ppg_emu_rows<ppg::RecordParams, ppg::record_main, ppg::LINK_LDS_BYTES>(K, K.batch);
}
static int backend_record_obs(ppg_handle *, const ppg::ObsStoreParams &K, void *) {
    ppg_emu_rows<ppg::ObsStoreParams, ppg::obs_scan_main, ppg::ROWS_SCAN_LDS_BYTES>(K, 1);
    return ppg_emu_rows<ppg::ObsStoreParams, ppg::obs_rows_main>(K, K.batch);
}
static int backend_record_logp(ppg_handle *, const ppg::LogpParams &K, void *) {
    ppg_emu_rows<ppg::LogpParams, ppg::logp_scan_main, ppg::ROWS_SCAN_LDS_BYTES>(K, 1);
    return ppg_emu_rows<ppg::LogpParams, ppg::logp_rows_main>(K, K.batch);
}
static int backend_backward(ppg_handle *, const ppg::BackwardParams &K, void *) {
    return ppg_emu_rows<ppg::BackwardParams, ppg::backward_main, ppg::BACKWARD_LDS_BYTES>(K, K.batch);
}
static int backend_backward_samples(ppg_handle *, const ppg::BackwardSamplesParams &K, void *) {
    return ppg_emu_rows<ppg::BackwardSamplesParams, ppg::backward_samples_main, ppg::BACKWARD_LDS_BYTES>(K, K.batch);
}
static int backend_ppo_loss(ppg_handle *, const ppg::PpoParams &K, void *) {
    ppg_emu_rows<ppg::PpoParams, ppg::ppo_count_main>(K, K.G);
    return ppg_emu_rows<ppg::PpoParams, ppg::ppo_rows_main, ppg::PPO_LDS_BYTES>(K, K.G);
}
// (four-wave workgroups with exactly lds_bytes of LDS each)
static int backend_net_forward(ppg_handle *, const ppg::NetParams &K, int lds_bytes, void *) {
    for (int b = 0; b < K.G; ++b)
        wv::run_block([](void *arg) { ppg::net_forward_main(*(const ppg::NetParams *)arg, wv::emu().lds); }, (void *)&K, b, (size_t)lds_bytes, ppg::NET_WAVES);
    return PPG_OK;
}
static int backend_net_backward(ppg_handle *, const ppg::NetParams &K, int lds_bytes, void *) {
    for (int b = 0; b < K.G; ++b)
        wv::run_block([](void *arg) { ppg::net_backward_main(*(const ppg::NetParams *)arg, wv::emu().lds); }, (void *)&K, b, (size_t)lds_bytes, ppg::NET_WAVES);
    for (int b = 0; b < (K.n_params + ppg::NET_THREADS - 1) / ppg::NET_THREADS; ++b)
        wv::run_block([](void *arg) { ppg::net_reduce_main(*(const ppg::NetParams *)arg); }, (void *)&K, b, 16, ppg::NET_WAVES);
    return PPG_OK;
}
#endif

// ---- argument checks more than one call makes: `fn` is the calling function's name, each stands where the caller's own lines stood ----
static int ppg_check_horizon(ppg_handle *h, const char *fn, int32_t horizon) {
    if (horizon < 1) return ppg_fail(h, PPG_EINVAL, "%s: horizon %d < 1", fn, horizon);
    return PPG_OK;
}

// the step argument of a recording call (ppg_rows.h: RecordedStep): `step` is the index, or with the call's on-device flag (named
// `flag`) the address of the device word
template <int BIAS>
static int ppg_step_arg(ppg_handle *h, const char *fn, const char *flag, bool on_device, uint64_t step, int32_t horizon,
                        ppg::RecordedStep<BIAS> &at) {
    if (on_device && !step) return ppg_fail(h, PPG_EINVAL, "%s: %s with a NULL address", fn, flag);
    if (!on_device && step >= (uint64_t)horizon)
        return ppg_fail(h, PPG_EINVAL, "%s: step %llu outside [0, %d)", fn, (unsigned long long)step, horizon);
    at.T = horizon; at.step_on_device = on_device;
    at.step = on_device ? 0 : (int32_t)step;
    at.step_dev = on_device ? (const int32_t *)(uintptr_t)step : nullptr;
    return PPG_OK;
}

// a sample store's capacities, and its slot table's int32 sample index
static int ppg_check_store(ppg_handle *h, const char *fn, const ppg_obs_store *st) {
    for (int s = 0; s < 2; ++s)
        if (st->capacity[s] < 0 || st->capacity[s] > INT32_MAX)
            return ppg_fail(h, PPG_EINVAL, "%s: capacity[%d] = %lld outside [0, 2^31)", fn, s, (long long)st->capacity[s]);
    if ((uint64_t)st->horizon * (uint64_t)h->batch * (uint64_t)h->base.S > (uint64_t)INT32_MAX)
        return ppg_fail(h, PPG_EINVAL, "%s: horizon %d x %d envs x %d rows does not fit the int32 sample index", fn, st->horizon, h->batch, h->base.S);
    return PPG_OK;
}

static int ppg_check_backward_inputs(ppg_handle *h, const char *fn, const double *reward, const int16_t *next_row, const uint8_t *in_use,
                                     const uint8_t *terminated, const uint8_t *truncated) {
    if (!reward || !next_row || !in_use || !terminated || !truncated) return ppg_fail(h, PPG_EINVAL, "%s: an input pointer is NULL", fn);
    return PPG_OK;
}

// the backward kernels' instantiations: 2 .. 6 row registers per lane
static int ppg_check_backward_rows(ppg_handle *h, const char *fn) {
    const int S = h->base.S;
    if (S % 64 != 0 || S < 128 || S * 8 * 3 > ppg::BACKWARD_LDS_BYTES)
        return ppg_fail(h, PPG_EINVAL, "%s: %d rows per env (needs a multiple of 64 in 128..%d)", fn, S, ppg::BACKWARD_MAX_ROWS);
    return PPG_OK;
}

// the head of a parameter block whose kernel walks the handle's row tables (LinkParams / RecordParams, ObsStoreParams, LogpParams)
template <class Params>
static void ppg_row_block(const ppg_handle *h, Params &K) {
    K.batch = h->batch; K.S = h->base.S; K.cap_pred = h->base.cap_pred; K.cap_prey = h->base.cap_prey;
    K.env_state = h->bufs.env_state;
}

extern "C" {

static int ppg_pack_geometry(const ppg_handle *h, uint32_t flags, int &blk_p, int &blk_q, int &src_elem, int &dst_elem) {
    const ppg::KParams &P = h->base;
    const bool drive = h->drive != 0;
    const int channels = (h->gen2 && h->cfg2.walls && h->cfg2.include_visibility_channel) ? 5 : 4;
    blk_p = (drive ? 4 + P.n_drive[0] : channels) * P.Rp * P.Rp;
    blk_q = (drive ? 4 + P.n_drive[1] : channels) * P.Rq * P.Rq;
    if (flags & PPG_PACK_NO_OBS) blk_p = blk_q = 0;   // an image without observation sections
    src_elem = P.obs_f32 == 2 ? 2 : P.obs_f32 ? 4 : 8;
    dst_elem = ((flags & PPG_PACK_F32) && src_elem == 8) ? 4 : src_elem;
    return PPG_OK;
}

uint64_t ppg_pack_bytes(const ppg_handle *h, int32_t n_envs, int64_t n_pred_rows, int64_t n_prey_rows, uint32_t flags) {
    if (!h || n_envs < 0 || n_pred_rows < 0 || n_prey_rows < 0) return 0;
    int bp, bq, se, de;
    ppg_pack_geometry(h, flags, bp, bq, se, de);
    return ppg::pack_layout((uint64_t)n_envs, (uint64_t)n_pred_rows, (uint64_t)n_prey_rows, (uint64_t)bp, (uint64_t)bq, (uint64_t)de).total;
}

int ppg_pack(ppg_handle *const *handles, int32_t n, void *out, uint64_t capacity, uint32_t flags, void *stream) {
    if (!handles || n < 1 || !handles[0]) return PPG_EINVAL;
    ppg_handle *h0 = handles[0];
    if (n > PPG_PACK_MAX_HANDLES) return ppg_fail(h0, PPG_EINVAL, "ppg_pack takes at most %d handles", PPG_PACK_MAX_HANDLES);
    if (!out || ((uintptr_t)out & 15u)) return ppg_fail(h0, PPG_EINVAL, "out must be a 16-byte aligned device pointer");
    if (flags & ~(PPG_PACK_F32 | PPG_PACK_NO_OBS)) return ppg_fail(h0, PPG_EINVAL, "unknown pack flags 0x%x", flags);
    ppg::PackParams K;
    memset(&K, 0, sizeof K);
    ppg_pack_geometry(h0, flags, K.blk_pred, K.blk_prey, K.src_elem, K.dst_elem);
    K.S = h0->base.S; K.cap_pred = h0->base.cap_pred; K.cap_prey = h0->base.cap_prey;
    K.n_handles = n;
    int total = 0;
    for (int k = 0; k < n; ++k) {
        const ppg_handle *h = handles[k];
        if (!h) return ppg_fail(h0, PPG_EINVAL, "handle %d is NULL", k);
        int bp, bq, se, de;
        ppg_pack_geometry(h, flags, bp, bq, se, de);
        if (bp != K.blk_pred || bq != K.blk_prey || se != K.src_elem || h->base.S != K.S || h->base.cap_pred != K.cap_pred || h->device != h0->device)
            return ppg_fail(h0, PPG_EINVAL, "handle %d has another geometry / device than handle 0", k);
        K.env_base[k] = total;
        total += h->batch;
        K.env_state[k] = h->bufs.env_state; K.row_id[k] = h->bufs.row_id; K.row_reward[k] = h->bufs.row_reward;
        K.row_flags[k] = h->bufs.row_flags;
        K.obs_pred[k] = (const unsigned char *)h->bufs.obs_pred; K.obs_prey[k] = (const unsigned char *)h->bufs.obs_prey;
    }
    for (int k = n; k <= PPG_PACK_MAX_HANDLES; ++k) K.env_base[k] = total;
    K.n_envs = total;
    K.capacity = capacity;
    K.out = (unsigned char *)out;
    // the header, the env words and the row offsets are always written: the caller learns the size an overflowing image needs
    const uint64_t fixed = ppg::pack_layout((uint64_t)total, 0, 0, 0, 0, 4).id_p;
    if (capacity < fixed) return ppg_fail(h0, PPG_EINVAL, "capacity %llu is below the fixed part of the image (%llu bytes for %d envs)",
                                          (unsigned long long)capacity, (unsigned long long)fixed, total);
    return backend_pack(h0, K, stream);
}

static void ppg_fetch_geometry(const ppg_handle *h, uint32_t &rec, uint32_t &bp, uint32_t &bq) {
    ppg_state_field f[16];
    const int n = ppg_state_fields(h, f);
    uint64_t r = 0;
    for (int i = 0; i < n; ++i) r += (f[i].bytes + 7) / 8 * 8;
    rec = (uint32_t)((r + 15) / 16 * 16);
    int blk_p, blk_q, se, de;
    ppg_pack_geometry(h, 0, blk_p, blk_q, se, de);
    bp = (uint32_t)(blk_p * se); bq = (uint32_t)(blk_q * se);
}

uint64_t ppg_fetch_bytes(const ppg_handle *h, int32_t n_envs, int64_t n_pred_rows, int64_t n_prey_rows) {
    if (!h || n_envs < 0 || n_pred_rows < 0 || n_prey_rows < 0) return 0;
    uint32_t rec, bp, bq;
    ppg_fetch_geometry(h, rec, bp, bq);
    return sizeof(ppg_fetch_header) + (uint64_t)n_envs * rec + (uint64_t)n_pred_rows * bp + (uint64_t)n_prey_rows * bq + (uint64_t)n_envs * 32;
}

int ppg_fetch(ppg_handle *h, int32_t env0, int32_t n_envs, void *host, uint64_t capacity, void *stream) {
    if (!h) return PPG_EINVAL;
    if (!host || ((uintptr_t)host & 15u)) return ppg_fail(h, PPG_EINVAL, "host must be a 16-byte aligned host pointer");
    if (env0 < 0 || n_envs < 1 || env0 + n_envs > h->batch) return ppg_fail(h, PPG_EINVAL, "envs [%d, %d) not in 0..%d", env0, env0 + n_envs, h->batch);
    ppg::FetchParams K;
    memset(&K, 0, sizeof K);
    ppg_fetch_geometry(h, K.record_bytes, K.blk_pred_bytes, K.blk_prey_bytes);
    const uint64_t fixed = sizeof(ppg_fetch_header) + (uint64_t)n_envs * K.record_bytes;
    if (capacity < fixed) return ppg_fail(h, PPG_EINVAL, "capacity %llu is below the fixed part of the image (%llu bytes for %d envs)",
                                          (unsigned long long)capacity, (unsigned long long)fixed, n_envs);
    ppg_state_field f[16];
    K.n_fields = ppg_state_fields(h, f);
    for (int i = 0; i < K.n_fields; ++i) { K.field[i] = (const unsigned char *)f[i].base; K.field_bytes[i] = (uint32_t)f[i].bytes; }
    K.env0 = env0; K.n_envs = n_envs;
    K.env_state = h->bufs.env_state;
    K.obs_pred = (const unsigned char *)h->bufs.obs_pred; K.obs_prey = (const unsigned char *)h->bufs.obs_prey;
    K.cap_pred = h->base.cap_pred; K.cap_prey = h->base.cap_prey;
    K.capacity = capacity;
    if (h->fetch_cap < capacity) {   // the staging buffer grows with the largest image asked for
        if (h->fetch_dev) { const int rc = backend_sync(h, stream); if (rc != PPG_OK) return rc; backend_free(h, h->fetch_dev); }
        h->fetch_dev = nullptr; h->fetch_cap = 0;
        const int rc = backend_alloc(h, (void **)&h->fetch_dev, (size_t)capacity);
        if (rc != PPG_OK) return rc;
        h->fetch_cap = capacity;
    }
    K.out = h->fetch_dev;
    int rc = backend_fetch(h, K, stream);
    if (rc != PPG_OK) return rc;
    // ONE transfer in the common case: as many bytes as the last image took plus a margin (births add rows); the header then says
    // whether a second transfer has to bring the rest
    uint64_t first = h->fetch_hint ? h->fetch_hint : capacity;
    if (first < fixed) first = fixed;
    if (first > capacity) first = capacity;
    rc = backend_copy(h, host, h->fetch_dev, (size_t)first, false, stream);
    if (rc == PPG_OK) rc = backend_sync(h, stream);
    if (rc != PPG_OK) return rc;
    const ppg_fetch_header *H = (const ppg_fetch_header *)host;
    if (H->magic != PPG_FETCH_MAGIC) return ppg_fail(h, PPG_EHIP, "ppg_fetch: the image has no header (magic 0x%x)", H->magic);
    if (!H->overflow && H->bytes_used > first) {
        rc = backend_copy(h, (unsigned char *)host + first, h->fetch_dev + first, (size_t)(H->bytes_used - first), false, stream);
        if (rc == PPG_OK) rc = backend_sync(h, stream);
        if (rc != PPG_OK) return rc;
    }
    h->fetch_hint = H->bytes_used + H->bytes_used / 4 + 4096;
    return PPG_OK;
}

// the parameter block of a link launch (ppg_link, ppg_record); allocates the snapshot on first use
static int ppg_link_params(ppg_handle *h, ppg::LinkParams &K, int16_t *prev_row, int16_t *next_row) {
    const size_t B = (size_t)h->batch, S = (size_t)h->base.S;
    if (!h->link_dev) h->link_valid = 0;   // nothing in it yet: this call writes -1 everywhere and takes the first snapshot
    if (int rc = ppg_first_use(h, h->link_dev, (B * S + B + 2 * B) * sizeof(int32_t))) return rc;
    ppg_row_block(h, K);
    K.valid = h->link_valid;
    K.row_id = h->bufs.row_id; K.row_flags = h->bufs.row_flags;
    K.snap_id = h->link_dev; K.snap_episode = h->link_dev + B * S; K.snap_rows = h->link_dev + B * S + B;
    K.prev_row = prev_row; K.next_row = next_row;
    return PPG_OK;
}

int ppg_link(ppg_handle *h, int16_t *prev_row, int16_t *next_row, void *stream) {
    if (!h) return PPG_EINVAL;
    ppg::LinkParams K;
    memset(&K, 0, sizeof K);
    int rc = ppg_link_params(h, K, prev_row, next_row);
    if (rc != PPG_OK) return rc;
    rc = backend_link(h, K, stream);
    if (rc == PPG_OK) h->link_valid = 1;
    return rc;
}

int ppg_record(ppg_handle *h, const ppg_record_buffers *buf, uint64_t step, uint32_t flags, int16_t *prev_row, int16_t *next_row,
               void *stream) {
    if (!h) return PPG_EINVAL;
    if (!buf) return ppg_fail(h, PPG_EINVAL, "ppg_record: buf is NULL");
    if (!buf->reward || !buf->in_use || !buf->terminated || !buf->truncated || !buf->next_row)
        return ppg_fail(h, PPG_EINVAL, "ppg_record: a buffer of ppg_record_buffers is NULL");
    if (int rc = ppg_check_horizon(h, "ppg_record", buf->horizon)) return rc;
    if (flags & ~PPG_RECORD_STEP_ON_DEVICE) return ppg_fail(h, PPG_EINVAL, "ppg_record: unknown flag bits 0x%x", flags);
    ppg::RecordParams K;
    memset((void *)&K, 0, sizeof K);
    int rc = ppg_step_arg(h, "ppg_record", "PPG_RECORD_STEP_ON_DEVICE", (flags & PPG_RECORD_STEP_ON_DEVICE) != 0, step, buf->horizon, K);
    if (rc != PPG_OK) return rc;
    const int S = h->base.S;
    if (S % 64 != 0 || S < 64 || S > ppg::LINK_MAX_ROWS)   // the kernel's row registers: S / 64 per lane
        return ppg_fail(h, PPG_EINVAL, "ppg_record: %d rows per env (needs a multiple of 64 up to %d)", S, ppg::LINK_MAX_ROWS);
    rc = ppg_link_params(h, K, prev_row, next_row);
    if (rc != PPG_OK) return rc;
    K.row_reward = (const uint64_t *)h->bufs.row_reward; K.reward = (uint64_t *)buf->reward;
    K.in_use = buf->in_use; K.terminated = buf->terminated; K.truncated = buf->truncated; K.traj_next = buf->next_row;
    rc = backend_record(h, K, stream);
    if (rc == PPG_OK) h->link_valid = 1;
    return rc;
}

int ppg_record_obs(ppg_handle *h, const ppg_obs_store *st, uint64_t step, uint32_t flags, const int8_t *actions, void *stream) {
    if (!h) return PPG_EINVAL;
    if (!st) return ppg_fail(h, PPG_EINVAL, "ppg_record_obs: st is NULL");
    if (!st->slot || !st->cursor || !st->sample[0] || !st->sample[1] || !st->obs[0] || !st->obs[1])
        return ppg_fail(h, PPG_EINVAL, "ppg_record_obs: slot, cursor, a sample[] or an obs[] of ppg_obs_store is NULL");
    if (int rc = ppg_check_horizon(h, "ppg_record_obs", st->horizon)) return rc;
    if (int rc = ppg_check_store(h, "ppg_record_obs", st)) return rc;
    if (!st->action[0] != !st->action[1]) return ppg_fail(h, PPG_EINVAL, "ppg_record_obs: only one of the two action[] pointers is set");
    if (flags & ~(PPG_OBS_STEP_ON_DEVICE | PPG_OBS_F32)) return ppg_fail(h, PPG_EINVAL, "ppg_record_obs: unknown flag bits 0x%x", flags);
    ppg::ObsStoreParams K;
    memset((void *)&K, 0, sizeof K);   // ((void *): a block with a base -- RecordedStep -- is trivially copyable but not standard-layout)
    if (int rc = ppg_step_arg(h, "ppg_record_obs", "PPG_OBS_STEP_ON_DEVICE", (flags & PPG_OBS_STEP_ON_DEVICE) != 0, step, st->horizon, K)) return rc;
    ppg_pack_geometry(h, (flags & PPG_OBS_F32) ? PPG_PACK_F32 : 0u, K.blk[0], K.blk[1], K.src_elem, K.dst_elem);
    if ((flags & PPG_OBS_F32) && K.src_elem < 4)
        return ppg_fail(h, PPG_EINVAL, "ppg_record_obs: PPG_OBS_F32 on a handle with %d-byte observation elements", K.src_elem);
    if (int rc = ppg_first_use(h, h->obs_base_dev, (size_t)h->batch * 2 * sizeof(int64_t))) return rc;
    ppg_row_block(h, K);
    K.src[0] = (const unsigned char *)h->bufs.obs_pred; K.src[1] = (const unsigned char *)h->bufs.obs_prey;
    for (int s = 0; s < 2; ++s) {
        K.dst[s] = (unsigned char *)st->obs[s]; K.capacity[s] = st->capacity[s];
        K.sample[s] = st->sample[s]; K.action[s] = st->action[s];
    }
    K.slot = st->slot; K.cursor = st->cursor; K.base = h->obs_base_dev;
    K.actions = st->action[0] ? actions : nullptr;
    return backend_record_obs(h, K, stream);
}

int ppg_record_logp(ppg_handle *h, const ppg_obs_store *st, const ppg_logp_store *out, uint64_t step, uint32_t flags,
                    const float *logits_pred, const float *logits_prey, const int8_t *actions, void *stream) {
    if (!h) return PPG_EINVAL;
    if (!st || !out || !actions) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: st, out or actions is NULL");
    if (!st->slot) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: slot of ppg_obs_store is NULL");
    if (int rc = ppg_check_horizon(h, "ppg_record_logp", st->horizon)) return rc;
    if (int rc = ppg_check_store(h, "ppg_record_logp", st)) return rc;
    const float *logits[2] = {logits_pred, logits_prey};
    for (int s = 0; s < 2; ++s) {
        if (!logits[s]) continue;
        if (!out->logp[s]) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: logp[%d] is NULL but the species' logits are given", s);
        if (out->n_actions[s] < 1 || out->n_actions[s] > 32)
            return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: n_actions[%d] = %d outside 1..32", s, out->n_actions[s]);
    }
    if (!out->entropy[0] != !out->entropy[1]) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: only one of the two entropy[] pointers is set");
    if (!out->dist[0] != !out->dist[1]) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: only one of the two dist[] pointers is set");
    if (flags & ~PPG_LOGP_STEP_ON_DEVICE) return ppg_fail(h, PPG_EINVAL, "ppg_record_logp: unknown flag bits 0x%x", flags);
    ppg::LogpParams K;
    memset((void *)&K, 0, sizeof K);   // ((void *): as in ppg_record_obs)
    if (int rc = ppg_step_arg(h, "ppg_record_logp", "PPG_LOGP_STEP_ON_DEVICE", (flags & PPG_LOGP_STEP_ON_DEVICE) != 0, step, st->horizon, K)) return rc;
    if (!logits[0] && !logits[1]) return PPG_OK;   // both species skipped
    if (int rc = ppg_first_use(h, h->logp_off_dev, (size_t)h->batch * 2 * sizeof(int32_t))) return rc;
    ppg_row_block(h, K);
    for (int s = 0; s < 2; ++s) {
        K.logits[s] = logits[s]; K.n_actions[s] = out->n_actions[s]; K.capacity[s] = st->capacity[s];
        K.logp[s] = out->logp[s]; K.entropy[s] = out->entropy[s]; K.dist[s] = (uint32_t *)out->dist[s];
    }
    K.slot = st->slot; K.actions = actions; K.off = h->logp_off_dev;
    return backend_record_logp(h, K, stream);
}

int ppg_backward(ppg_handle *h, int32_t n_steps, const double *reward, const int16_t *next_row, const uint8_t *in_use,
                 const uint8_t *terminated, const uint8_t *truncated, const void *values, int32_t values_dtype, double gamma, double lam,
                 double *returns, double *advantages, void *stream) {
    if (!h) return PPG_EINVAL;
    if (n_steps < 1) return ppg_fail(h, PPG_EINVAL, "ppg_backward: n_steps %d < 1", n_steps);
    if (int rc = ppg_check_backward_inputs(h, "ppg_backward", reward, next_row, in_use, terminated, truncated)) return rc;
    if (!returns && !advantages) return ppg_fail(h, PPG_EINVAL, "ppg_backward: returns and advantages are both NULL");
    if (advantages && !values) return ppg_fail(h, PPG_EINVAL, "ppg_backward: advantages need values");
    if (values && values_dtype != PPG_F64 && values_dtype != PPG_F32)
        return ppg_fail(h, PPG_EINVAL, "ppg_backward: values_dtype %d is neither PPG_F64 nor PPG_F32", values_dtype);
    if (int rc = ppg_check_backward_rows(h, "ppg_backward")) return rc;
    ppg::BackwardParams K;
    memset(&K, 0, sizeof K);
    K.batch = h->batch; K.S = h->base.S; K.T = n_steps;
    K.values_f32 = values && values_dtype == PPG_F32; K.prefetch = h->backward_prefetch;
    K.reward = reward; K.next_row = next_row; K.in_use = in_use; K.terminated = terminated; K.truncated = truncated;
    K.values = advantages ? values : nullptr;
    K.gamma = gamma; K.gl = gamma * lam;
    K.returns = returns; K.advantages = advantages;
    return backend_backward(h, K, stream);
}

int ppg_backward_samples(ppg_handle *h, int32_t n_steps, const double *reward, const int16_t *next_row, const uint8_t *in_use,
                         const uint8_t *terminated, const uint8_t *truncated, const ppg_obs_store *st, const ppg_sample_targets *tg,
                         int32_t values_dtype, double gamma, double lam, void *stream) {
    if (!h) return PPG_EINVAL;
    if (!st || !tg) return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: st or tg is NULL");
    if (!st->slot) return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: slot of ppg_obs_store is NULL");
    if (int rc = ppg_check_backward_inputs(h, "ppg_backward_samples", reward, next_row, in_use, terminated, truncated)) return rc;
    if (n_steps < 1 || n_steps > st->horizon)
        return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: n_steps %d outside [1, horizon %d]", n_steps, st->horizon);
    if (int rc = ppg_check_store(h, "ppg_backward_samples", st)) return rc;
    if (!tg->advantage[0] != !tg->advantage[1])
        return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: only one of the two advantage[] pointers is set");
    if (!tg->returns[0] != !tg->returns[1])
        return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: only one of the two returns[] pointers is set");
    if (!tg->advantage[0] && !tg->returns[0]) return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: advantage[] and returns[] are both NULL");
    if (tg->stats && !tg->advantage[0]) return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: stats need advantage[]");
    if ((tg->values[0] || tg->values[1]) && values_dtype != PPG_F64 && values_dtype != PPG_F32)
        return ppg_fail(h, PPG_EINVAL, "ppg_backward_samples: values_dtype %d is neither PPG_F64 nor PPG_F32", values_dtype);
    if (int rc = ppg_check_backward_rows(h, "ppg_backward_samples")) return rc;
    ppg::BackwardSamplesParams K;
    memset(&K, 0, sizeof K);
    K.batch = h->batch; K.S = h->base.S; K.T = n_steps; K.cap_pred = h->base.cap_pred;
    K.values_f32 = values_dtype == PPG_F32; K.prefetch = h->backward_samples_prefetch;
    K.reward = reward; K.next_row = next_row; K.in_use = in_use; K.terminated = terminated; K.truncated = truncated;
    K.slot = st->slot;
    for (int s = 0; s < 2; ++s) {
        K.capacity[s] = (int32_t)st->capacity[s];
        K.values[s] = tg->advantage[0] ? tg->values[s] : nullptr;   // (returns alone do not depend on V)
        K.advantage[s] = tg->advantage[s]; K.returns[s] = tg->returns[s];
    }
    K.gamma = gamma; K.gl = gamma * lam;
    K.stats = tg->stats;
    return backend_backward_samples(h, K, stream);
}

int ppg_ppo_loss(ppg_handle *h, const ppg_ppo_batch *mb, float *grad_logits, float *grad_values, double *partial, void *stream) {
    if (!h) return PPG_EINVAL;
    if (!mb) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: mb is NULL");
    if (!mb->logits || !mb->action || !mb->logp || !mb->advantage)
        return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: logits, action, logp or advantage of ppg_ppo_batch is NULL");
    if (!grad_logits || !partial) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: grad_logits or partial is NULL");
    if (mb->M < 1 || mb->M > INT32_MAX) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: M = %lld outside [1, INT32_MAX]", (long long)mb->M);
    if (mb->A < 1 || mb->A > ppg::PPO_MAX_ACTIONS) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: A = %d outside 1..32", mb->A);
    if (mb->capacity < 0 || mb->capacity > INT32_MAX)
        return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: capacity = %lld outside [0, INT32_MAX]", (long long)mb->capacity);
    if (!mb->values != !mb->value_target) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: only one of values and value_target is set");
    if (grad_values && !mb->values) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: grad_values without values");
    if (mb->kl_coeff != 0.0 && !mb->dist) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: kl_coeff != 0 needs dist");
    if (!(mb->clip >= 0.0 && mb->clip < INFINITY)) return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: clip = %g is negative or not finite", mb->clip);
    if (!(mb->vf_clip >= 0.0 && mb->vf_clip < INFINITY))
        return ppg_fail(h, PPG_EINVAL, "ppg_ppo_loss: vf_clip = %g is negative or not finite", mb->vf_clip);
    ppg::PpoParams K;
    memset(&K, 0, sizeof K);
    K.M = mb->M; K.capacity = mb->capacity; K.A = mb->A;
    K.G = (int32_t)((mb->M + ppg::PPO_CHUNK - 1) / ppg::PPO_CHUNK);
    K.index = mb->index; K.logits = mb->logits; K.values = mb->values;
    K.action = mb->action; K.logp = mb->logp; K.dist = mb->dist; K.advantage = mb->advantage; K.value_target = mb->value_target;
    K.adv_norm = mb->adv_norm;
    K.clip_lo = 1.0 - mb->clip; K.clip_hi = 1.0 + mb->clip;
    K.vf_clip = mb->vf_clip; K.vf_coeff = mb->vf_coeff; K.ent_coeff = mb->ent_coeff; K.kl_coeff = mb->kl_coeff;
    K.grad_logits = grad_logits; K.grad_values = grad_values; K.partial = partial;
    return backend_ppo_loss(h, K, stream);
}

// ---- ppg_net_*: the geometry a network's shape decides (device-free), the argument checks, the launches ------------------------------
// The checks in front of ppg::net_layout (ppg_net.h): K's geometry for M rows and `groups` workgroups (0: automatic); *lds_bytes: dynamic
// LDS of a workgroup.
// PPG_EINVAL with the reason in msg[256].
static int ppg_net_layout(const ppg_policy_spec &sp, int64_t M, int32_t groups, ppg::NetParams &K, int *lds_bytes, char *msg) {
    memset(&K, 0, sizeof K);
    if (int rc = ppg_policy_shape_check(sp, false, msg, 256)) return rc;
    if (M < 1 || M > (1 << 24)) return ppg_policy_shape_fail(msg, 256, "M = %lld outside [1, 2^24]", (long long)M);
    if (groups < 0) return ppg_policy_shape_fail(msg, 256, "groups = %d is negative", groups);
    *lds_bytes = ppg::net_layout(sp, M, groups, K);
    return PPG_OK;
}

static void ppg_net_sizes(const ppg::NetParams &K, uint64_t out[4]) {
    out[0] = (uint64_t)K.M * (uint64_t)K.ws_row * 4; out[1] = (uint64_t)K.G * (uint64_t)K.n_params * 4;
    out[2] = (uint64_t)K.n_params; out[3] = (uint64_t)K.TS;
}

int ppg_net_bytes(const ppg_policy_spec *spec, int64_t M, int32_t groups, uint64_t out[4]) {
    if (!spec || !out) return ppg_fail(nullptr, PPG_EINVAL, "ppg_net_bytes: spec or out is NULL");
    ppg::NetParams K;
    int lds = 0;
    char msg[256];
    if (ppg_net_layout(*spec, M, groups, K, &lds, msg) != PPG_OK) return ppg_fail(nullptr, PPG_EINVAL, "ppg_net_bytes: %s", msg);
    ppg_net_sizes(K, out);
    return PPG_OK;
}

// what ppg_net_forward and ppg_net_backward check alike, and what both launch with: the parameter block, a workgroup's dynamic LDS, and
// the sizes of ppg_net_bytes for this call's geometry (computed here, once)
struct ppg_net_call { ppg::NetParams K; int lds_bytes; uint64_t need[4]; };
static int ppg_net_params(ppg_handle *h, const char *fn, bool forward, const ppg_policy_spec *spec, const ppg_net_batch *mb, ppg_net_call &c) {
    ppg::NetParams &K = c.K;
    if (!spec) return ppg_fail(h, PPG_EINVAL, "%s: spec is NULL", fn);
    if (!mb) return ppg_fail(h, PPG_EINVAL, "%s: mb is NULL", fn);
    char msg[256];
    if (ppg_net_layout(*spec, mb->M, mb->groups, K, &c.lds_bytes, msg) != PPG_OK) return ppg_fail(h, PPG_EINVAL, "%s: %s", fn, msg);
    ppg_net_sizes(K, c.need);
    if (ppg_policy_shape_check(*spec, true, msg, sizeof msg) != PPG_OK) return ppg_fail(h, PPG_EINVAL, "%s: %s", fn, msg);
    if (mb->capacity < 0 || mb->capacity > INT32_MAX)
        return ppg_fail(h, PPG_EINVAL, "%s: capacity = %lld outside [0, INT32_MAX]", fn, (long long)mb->capacity);
    if (mb->obs_dtype < 0 || mb->obs_dtype > 2) return ppg_fail(h, PPG_EINVAL, "%s: unknown obs_dtype %d", fn, mb->obs_dtype);
    if (!mb->obs && mb->capacity > 0) return ppg_fail(h, PPG_EINVAL, "%s: obs of ppg_net_batch is NULL", fn);
    if (forward && !mb->out) return ppg_fail(h, PPG_EINVAL, "%s: out of ppg_net_batch is NULL", fn);
    if (!mb->workspace) return ppg_fail(h, PPG_EINVAL, "%s: workspace of ppg_net_batch is NULL", fn);
    if (mb->workspace_bytes < c.need[0])
        return ppg_fail(h, PPG_EINVAL, "%s: workspace_bytes = %llu, %lld rows need %llu", fn, (unsigned long long)mb->workspace_bytes,
                        (long long)mb->M, (unsigned long long)c.need[0]);
    K.capacity = mb->capacity; K.obs_dtype = mb->obs_dtype; K.obs = mb->obs; K.index = mb->index;
    K.out = mb->out; K.workspace = mb->workspace;
    for (int l = 0; l < spec->n_conv; ++l) { K.conv_w[l] = spec->conv_w[l]; K.conv_b[l] = spec->conv_b[l]; }
    for (int l = 0; l < spec->n_fc; ++l) { K.fc_w[l] = spec->fc_w[l]; K.fc_b[l] = spec->fc_b[l]; }
    return PPG_OK;
}

int ppg_net_forward(ppg_handle *h, const ppg_policy_spec *spec, const ppg_net_batch *mb, void *stream) {
    if (!h) return PPG_EINVAL;
    ppg_net_call c;
    if (int rc = ppg_net_params(h, "ppg_net_forward", true, spec, mb, c)) return rc;
    return backend_net_forward(h, c.K, c.lds_bytes, stream);
}

int ppg_net_backward(ppg_handle *h, const ppg_policy_spec *spec, const ppg_net_batch *mb, const float *grad_out,
                     const ppg_policy_spec *grads, float *partial, uint64_t partial_bytes, void *stream) {
    if (!h) return PPG_EINVAL;
    const char *fn = "ppg_net_backward";
    ppg_net_call c;
    if (int rc = ppg_net_params(h, fn, false, spec, mb, c)) return rc;
    ppg::NetParams &K = c.K;
    if (!grad_out) return ppg_fail(h, PPG_EINVAL, "%s: grad_out is NULL", fn);
    if (!grads) return ppg_fail(h, PPG_EINVAL, "%s: grads is NULL", fn);
    if (!partial) return ppg_fail(h, PPG_EINVAL, "%s: partial is NULL", fn);
    if (partial_bytes < c.need[1])
        return ppg_fail(h, PPG_EINVAL, "%s: partial_bytes = %llu, %d workgroups of %d parameters need %llu", fn,
                        (unsigned long long)partial_bytes, K.G, K.n_params, (unsigned long long)c.need[1]);
    int seg = 0;
    for (int l = 0; l < spec->n_conv; ++l) { K.grad[seg++] = (float *)grads->conv_w[l]; K.grad[seg++] = (float *)grads->conv_b[l]; }
    for (int l = 0; l < spec->n_fc; ++l) { K.grad[seg++] = (float *)grads->fc_w[l]; K.grad[seg++] = (float *)grads->fc_b[l]; }
    for (int q = 0; q < seg; ++q)
        if (!K.grad[q]) return ppg_fail(h, PPG_EINVAL, "%s: a gradient pointer of grads is NULL", fn);
    K.grad_out = grad_out; K.partial = partial;
    return backend_net_backward(h, K, c.lds_bytes, stream);
}

}  // extern "C"
