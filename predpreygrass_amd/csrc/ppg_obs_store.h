// ppg_obs_store.h -- ppg_record_obs of include/ppg.h: the observation rows in use of the handle's last call, appended to a compact
// per-species sample store on the device, with the (t, b, r) each slot holds and the action taken from it one call later.
//
// Two launches, both written against the wave primitives of wave.h (the CPU test build runs the same source):
//   obs_scan  one wavefront: exclusive prefix sums of the two per-env row counts over B (rows_scan of ppg_rows.h), plus the cursor
//             -> absolute per-env slot bases in a library-owned [B,2] int64 scratch, then the four cursor words.  The only writer of
//             the cursor: no atomics.
//   obs_rows  one wavefront per env: slot[t] of its S rows, the sample words and PPG_ACTION_UNSET of the rows it stores, the actions
//             of step t - 1 through slot[t-1], and the observation copies.
// The rows in use of an env are the FIRST n rows of its region of the observation tensor, and their slots are consecutive, so an
// env's observations are two contiguous copies (predators, prey), each cut where the store's capacity ends.
// Both kernels request the step index t the same way (ppg_rows.h: RecordedStep); with t outside [0, T) neither writes anything.
// A slot number becomes an address only after 0 <= k < capacity was checked -- the bases come from the
// scratch, slot[t-1] from the caller: both are device memory.
// Ordinary vector loads / stores and LDS accesses only.
#pragma once

#include <stdint.h>

#include "ppg_rows.h"

namespace ppg {

struct ObsStoreParams : RecordedStep<0> {   // the device word holds t; T = the horizon: slot is [T,B,S]
    int32_t batch, S, cap_pred, cap_prey;
    const int32_t *env_state;
    const unsigned char *src[2];   // obs_pred / obs_prey of the handle
    int32_t blk[2];                // elements per observation block
    int32_t src_elem, dst_elem;    // bytes per element in the env buffers / in the store (float64 -> float32: 8 / 4)
    unsigned char *dst[2];
    int64_t capacity[2];
    int32_t *sample[2];
    int8_t *action[2];          // both NULL, or both set
    int32_t *slot;
    int64_t *cursor;            // [4]: stored {pred, prey}, dropped {pred, prey}
    int64_t *base;              // library-owned [B,2]: slot of the env's first row in use, per species
    const int8_t *actions;      // [B,S] of the handle's last step, or NULL
};

// 16 bytes of a source that is only known to be 4-byte aligned (the loads of the shifted copy below), 8 bytes likewise
struct __attribute__((packed, aligned(4))) ObsLoad16 { uint32_t a, b, c, d; };
struct alignas(16) ObsStore16 { uint32_t a, b, c, d; };
struct __attribute__((packed, aligned(8))) ObsLoadD2 { double x, y; };
struct alignas(16) ObsStoreF4 { float x, y, z, w; };

// ---- launch 1: one wavefront ------------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void obs_scan_main(const KP &K, unsigned char *lds) {
    const int ln = wv::lane();
    const bool live = step_in_horizon(K, recorded_step(K));
    int64_t cur[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {   // the cursor as a slot number: inside [0, capacity] whatever the word holds
        const int64_t c = K.cursor[s];
        cur[s] = c < 0 ? 0 : c > K.capacity[s] ? K.capacity[s] : c;
    }
    auto count = [&](int e, int s) { return (uint32_t)rows_in_use(K, K.env_state + (size_t)e * PPG_ENV_WORDS, s); };
    const RowScan r = rows_scan(K.batch, lds, count);
    rows_scan_each(r, count, [&](int e, uint32_t bp, uint32_t bq) {
        // a step index outside [0, T): bases at the capacity, with which obs_rows (which checks t itself) could store no row
        K.base[2 * e] = live ? cur[0] + (int64_t)bp : K.capacity[0];
        K.base[2 * e + 1] = live ? cur[1] + (int64_t)bq : K.capacity[1];
    });
    if (ln == 0 && live) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t end = cur[s] + (int64_t)r.total[s], kept = end < K.capacity[s] ? end : K.capacity[s];
            const int64_t dropped = K.cursor[2 + s];
            K.cursor[s] = kept;
            K.cursor[2 + s] = dropped + (end - kept);
        }
    }
}

// `bytes` bytes from src to dst (contiguous), this wavefront's 64 lanes together.  All three multiples of 4: a head of up to three
// words brings the DESTINATION to 16 bytes, then 16 bytes per lane (stores aligned, loads as aligned as the source then is: the
// destination of a run starts slot * block bytes into the store, 8 bytes for a bfloat16 1x1 window, 72 for 3x3), then the last words.
// Anything else byte by byte.
PPG_DEVICE void obs_copy(const unsigned char *src, unsigned char *dst, uint64_t bytes, int ln) {
    const uint64_t dst_addr = (uint64_t)(uintptr_t)dst, src_addr = (uint64_t)(uintptr_t)src;
    if (((dst_addr | src_addr | bytes) & 3u) != 0) {
        for (uint64_t i = (uint64_t)ln; i < bytes; i += 64) dst[i] = src[i];
        return;
    }
    uint64_t head = (16u - (dst_addr & 15u)) & 15u;
    if (head > bytes) head = bytes;
    if ((uint64_t)ln < (head >> 2)) ((uint32_t *)dst)[ln] = ((const uint32_t *)src)[ln];
    const ObsLoad16 *s = (const ObsLoad16 *)(src + head);
    ObsStore16 *d = (ObsStore16 *)(dst + head);
    const uint64_t n16 = (bytes - head) >> 4;
    uint64_t i = (uint64_t)ln;
    for (; i + 192 < n16; i += 256) {   // four loads in flight per lane
        const ObsLoad16 v0 = s[i], v1 = s[i + 64], v2 = s[i + 128], v3 = s[i + 192];
        ObsStore16 w0, w1, w2, w3;
        w0.a = v0.a; w0.b = v0.b; w0.c = v0.c; w0.d = v0.d; w1.a = v1.a; w1.b = v1.b; w1.c = v1.c; w1.d = v1.d;
        w2.a = v2.a; w2.b = v2.b; w2.c = v2.c; w2.d = v2.d; w3.a = v3.a; w3.b = v3.b; w3.c = v3.c; w3.d = v3.d;
        d[i] = w0; d[i + 64] = w1; d[i + 128] = w2; d[i + 192] = w3;
    }
    for (; i < n16; i += 64) { const ObsLoad16 v = s[i]; ObsStore16 w; w.a = v.a; w.b = v.b; w.c = v.c; w.d = v.d; d[i] = w; }
    const uint64_t done = head + (n16 << 4), tail = (bytes - done) >> 2;
    if ((uint64_t)ln < tail) ((uint32_t *)(dst + done))[ln] = ((const uint32_t *)(src + done))[ln];
}

// n float64 elements from src to dst as float32 (round to nearest even): a head of up to three elements brings the destination to
// 16 bytes, then four elements per lane, then the last ones
PPG_DEVICE void obs_copy_f32(const double *src, float *dst, uint64_t n, int ln) {
    uint64_t head = ((16u - ((uint64_t)(uintptr_t)dst & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    if ((uint64_t)ln < head) dst[ln] = (float)src[ln];
    const ObsLoadD2 *s = (const ObsLoadD2 *)(src + head);
    ObsStoreF4 *d = (ObsStoreF4 *)(dst + head);
    const uint64_t n4 = (n - head) >> 2;
    uint64_t i = (uint64_t)ln;
    for (; i + 64 < n4; i += 128) {   // four loads in flight per lane
        const ObsLoadD2 a0 = s[2 * i], a1 = s[2 * i + 1], b0 = s[2 * i + 128], b1 = s[2 * i + 129];
        ObsStoreF4 f, g;
        f.x = (float)a0.x; f.y = (float)a0.y; f.z = (float)a1.x; f.w = (float)a1.y;
        g.x = (float)b0.x; g.y = (float)b0.y; g.z = (float)b1.x; g.w = (float)b1.y;
        d[i] = f; d[i + 64] = g;
    }
    for (; i < n4; i += 64) {
        const ObsLoadD2 a0 = s[2 * i], a1 = s[2 * i + 1];
        ObsStoreF4 f;
        f.x = (float)a0.x; f.y = (float)a0.y; f.z = (float)a1.x; f.w = (float)a1.y;
        d[i] = f;
    }
    const uint64_t done = head + (n4 << 2);
    if ((uint64_t)ln < n - done) dst[done + ln] = (float)src[done + ln];
}

// ---- launch 2: one wavefront per env ------------------------------------------------------------------------------
template <class KP>
PPG_DEVICE void obs_rows_main(const KP &K) {
    const int b = PPG_BLOCK_INDEX();
    if (b >= K.batch) return;
    const int ln = wv::lane();
    const int64_t t = recorded_step(K);
    if (!step_in_horizon(K, t)) return;   // a replay past the horizon: nothing
    const int S = K.S;
    const int32_t *es = K.env_state + (size_t)b * PPG_ENV_WORDS;
    const size_t step = (size_t)K.batch * S, at = (size_t)t * step + (size_t)b * S;
    const bool with_actions = K.actions && K.action[0] && t > 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {   // predators, then prey: rows [first, first + cap) of the env
        const int first = s ? K.cap_pred : 0, cap = s ? K.cap_prey : K.cap_pred;
        const int n = rows_in_use(K, es, s);
        const int64_t base = K.base[2 * b + s], capacity = K.capacity[s];
        int32_t *sample = K.sample[s];
        int8_t *action = K.action[s];
        for (int j = ln; j < cap; j += 64) {
            const int64_t k = base + j;
            const bool stored = j < n && k >= 0 && k < capacity;
            K.slot[at + first + j] = stored ? (int32_t)k : -1;
            if (stored) {
                sample[k] = (int32_t)(at + first + j);
                if (action) action[k] = (int8_t)PPG_ACTION_UNSET;
            }
        }
        if (with_actions) {   // the actions the step behind this output was given answer the observations of step t - 1
            for (int j = ln; j < cap; j += 64) {
                const int64_t k = K.slot[at - step + first + j];
                if (k >= 0 && k < capacity) action[k] = K.actions[(size_t)b * S + first + j];
            }
        }
        int64_t room = capacity - base;   // rows of this env the store still takes
        if (base < 0 || room < 0) room = 0;
        const uint64_t rows = (uint64_t)(room < n ? room : n);
        if (rows == 0) continue;
        const uint64_t blk = (uint64_t)K.blk[s];
        const unsigned char *src = K.src[s] + (uint64_t)b * cap * blk * K.src_elem;
        unsigned char *dst = K.dst[s] + (uint64_t)base * blk * K.dst_elem;
        if (K.src_elem == K.dst_elem) obs_copy(src, dst, rows * blk * K.src_elem, ln);
        else obs_copy_f32((const double *)src, (float *)dst, rows * blk, ln);
    }
}

}  // namespace ppg
