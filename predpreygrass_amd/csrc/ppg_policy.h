// ppg_policy.h -- policy inference next to the env (include/ppg.h: ppg_policy_*).
//
// The network the reference trains for each species (base_environment/tune_ppo_base_environment.py:106-141):
//     (4,R,R) observation -> conv3x3(C->16) ReLU -> conv3x3(16->32) ReLU -> conv3x3(32->64) ReLU   ("same" padding, stride 1)
//                         -> flatten -> Linear(64 P -> 256) ReLU -> Linear(256 -> 256) ReLU -> Linear(256 -> n_actions)
// in either of the two ways a (4,R,R) Box can be read as an image (include/ppg.h: PPG_POLICY_LAYOUT_*): channel-first -- an R x R
// image with C = 4 channels, P = R^2 positions -- or channels-last, which is how RLlib's CNN encoder reads a 3-D Box ([H, W, C]:
// a 4 x R image with C = R channels, P = 4 R positions).  The kernels work on an IH x IW image with CIN channels;
// evaluated for every agent row in use, reading the observation rows where ppg_step wrote them and writing one int8 action per
// row.  gfx950 only: every layer is a GEMM on the matrix cores, v_mfma_f32_32x32x16_bf16 (bf16 operands, fp32 accumulate).
//
// ORIENTATION (all six layers): M = output features / channels (the A operand = weights), N = samples or positions (the B
// operand = activations).  In the 32x32 result a lane holds ONE column (sample / position, = lane & 31) and 16 of the 32 rows:
// register 4g+i of lane half h = lane >> 5 is MFMA row i + 8g + 4h.  Which output feature an MFMA row computes is free -- it is
// decided by the order in which the host packs the weight rows -- so row i + 8g + 4h is given feature 16h + 4g + i of its
// 32-feature tile: a lane's 16 registers are then 16 CONSECUTIVE features (32 bytes of bf16), written by two 16-byte stores
// into an activation image whose inner dimension is the feature index -- exactly the 16-byte-per-lane B fragment the next
// layer reads (k = 8h + j: eight consecutive features).
//
// ONE persistent launch per species.  A workgroup (4 wavefronts) takes tiles of 128 samples:
//   A. convolutions in sub-groups of ST samples: activations live in LDS as [sample][channel block of 8][padded position][8]
//      bf16 with a zero halo ring (so the nine taps of the implicit GEMM are plain offsets); each wavefront keeps the layer's
//      weight fragments in registers (conv3: 144 VGPRs) and walks over 32-position tiles.  conv3 writes its output to the
//      workgroup's scratch slot in HBM/L2 as X[sample][row tile][position][32]  (= the K order the repacked FC1 weights expect).
//   B. FC1 over the whole tile (K = 64 R^2): weight fragments stream from L2, X fragments from the scratch slot (the slot was
//      written by this workgroup and is re-read after a workgroup barrier + ONE agent-scope acquire that drops stale L1 lines);
//      ReLU -> H[sample][256] in LDS.   C. FC2 from H, result back into H.   D. logits (M = actions padded to 32), the two
//      lane halves exchange their rows, argmax or Gumbel-max sampling, int8 store into actions[b][slot].
// The sample list is never materialised: a one-wavefront plan kernel writes exclusive prefix sums of the per-env row counts and
// each tile resolves sample -> (handle, env, row) by bisection.
// This file is device code only: the parameter blocks, the plan kernels, the FC-chain kernels, ppg_policy_repack and, included at its
// end, the direct-head and pipeline kernels.  The host side -- struct ppg_policy and the ppg_policy_* C ABI -- is ppg_policy_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>
#include <vector>

#include "ppg_policy_pack.h"
#include "ppg_policy_plan.h"

namespace ppgpol {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
#define GLOBAL_AS __attribute__((address_space(1)))   // pointers known to be global memory: global_* instead of flat_* instructions

constexpr int TILE = (int)PPG_PLAN_TILE;   // samples per workgroup tile (128)
constexpr int HSTRIDE = 264;      // H[sample][256 + 8] bf16: rows 528 B apart -> conflict-free 16-byte fragment reads
constexpr int MAX_HANDLES = PPG_PACK_MAX_HANDLES;
constexpr int PLAN_HDR = PPG_PLAN_HDR;     // words in front of the prefix sums of PolParams::plan (3)

struct PolParams {
    // geometry
    int32_t R, P, Wp, Wp2;        // window side of the observation; image positions IH*IW; padded row pitch IW+2; (IH+2)*(IW+2)
    int32_t IH, IW, cin;          // the image the convolutions run on and its real input channels
    int32_t c_stride, p_stride;   // observation element of (channel c, position p) = c * c_stride + p * p_stride
    int32_t obs_elems;            // elements per observation row: 4 R^2
    int32_t K1;                   // 64 * P
    int32_t ST;                   // samples per convolution sub-group
    int32_t n_actions;
    int32_t species;              // 0 predators, 1 prey
    int32_t obs_f32;
    int32_t sample;               // PPG_POLICY_SAMPLE
    uint32_t seed_lo, seed_hi;
    const uint64_t *seed_dev;     // PPG_POLICY_SEED_ON_DEVICE: the key is read from here by the kernel (seed_lo / seed_hi unused)
    // weights in fragment order (device, bf16) and the head's biases (float; the convolutions' ride in their fragments)
    const bf16x8 *wc1, *wc2, *wc3, *w1, *w2, *w3;
    const float *b1, *b2, *b3;
    // envs
    int32_t n_handles, n_envs;
    int32_t env_base[MAX_HANDLES + 1];
    const int32_t *env_state[MAX_HANDLES];
    const unsigned char *obs[MAX_HANDLES];   // obs_pred or obs_prey of handle k
    int8_t *actions[MAX_HANDLES];
    int32_t S, cap, slot0;        // rows per env of the action tensor; row capacity of this species; its first slot
    // scratch
    const uint32_t *plan;         // [0] = total rows of this species, [1] = number of FULL tiles (128 samples, whole rounds of the
                                  // resident workgroups), [2] = samples per tile of the last round (32 / 64 / 96 / 128),
                                  // [PLAN_HDR + e] = exclusive prefix sum of env e
    const uint32_t *tile_env;     // [tile] = env of the tile's first sample
    uint32_t magic_P, magic_R;    // ceil(2^18 / P), ceil(2^18 / IW): div_small()
    __bf16 *xg;                   // [gridDim.x][TILE][K1]
    float *logits;                // optional [rows][n_actions]
    // hidden layers of the head (phase_head): 2 = FC1, FC2, logits; 1 = FC1, logits
    int32_t n_hidden;
    // ---- direct-head networks (ppg_policy_direct.h) ----
    int32_t n_conv;               // convolution layers
    int32_t cout_blocks[PPG_POLICY_MAX_CONV];   // real output channel blocks (of 8) per layer
    int32_t off_x, off_y, off_f, off_d0, off_d1;   // element offsets of the areas in a sample's LDS region
    int32_t sample_stride;        // elements per sample region
    int32_t flat_c;               // channels per position of area F (8 * cout_blocks[n_conv - 1])
    int32_t kflat_steps;          // k-steps of 32 features of the head: ceil(P * flat_c / 32)
    int32_t head_mt;              // 16-row tiles of actions: 1 or 2
    const bf16x8 *wcd[PPG_POLICY_MAX_CONV - 3];   // fragments of the convolutions behind the third (64 -> 64 channels)
    const bf16x8 *wh;             // head fragments [action tile][k-step][lane]
    const bf16x8 *whw;            // the same of action tile 0 per wavefront: [wavefront][18][lane], zeros behind a wavefront's share of k-steps
    const float *bh;              // head bias [32]
    float *lgs;                   // library-owned [gridDim.x][TILE][16 head_mt]: a workgroup's logits of its current tile
    int32_t range_tile;           // samples per tile inside a workgroup's share (PlanParams::range_tile)
    // the two-role pipeline (ppg_policy_pipe.h): element offsets of the second X / F area in a sample's region; byte offsets of the
    // partial-sum buffers (+ role B's barrier counter) and of the images in LDS
    int32_t pipe_x1, pipe_f1, pipe_red, pipe_img;
    int32_t pipe_raw, pipe_ni;    // bfloat16 rows of a multiple of 8 bytes: byte offset of the LDS area that takes a sub-group's rows as they
    uint32_t pipe_magic;          // lie in HBM, 8-byte loads per role-B thread and sub-group (0: one load per channel), ceil(2^32 / chunks per row),
    int32_t pipe_slots;           // samples whose chunks the 256 role-B threads cover at once: floor(256 / chunks per row)
    const uint16_t *slot_tab;     // the pipeline's slot table [32 slot_tiles]: sample << 8 | position of a sub-group's slot (0xFFFF: none);
    int32_t slot_tiles;           // ppg_slot_table
    const bf16x8 *wc1x;           // conv1 of the pipeline as three 16x16x32 fragments [ky][lane][8] (ppg_policy_pipe.h: Conv1X); its bias [16]
    const float *bc1x;
#ifdef PPG_EXPERIMENTS
    unsigned long long *timeline; // diagnostic builds: [tile][64] = workgroup, hardware id, samples, 4 wall-clock stamps (10 ns units); [8 + 12 wave + i] cycles of wave in step i of the convolutions, [56 + 2 wave + i] FC1 wait / barrier cycles
#endif
};

struct PlanParams {
    int32_t n_handles, n_envs, word;   // word: PPG_ENV_N_PRED_ROWS / PPG_ENV_N_PREY_ROWS
    int32_t slots;                     // workgroups the forward launch keeps resident (its grid)
    int32_t range_tile, range_st;      // direct-head kernels: > 0 = RANGE MODE -- every workgroup gets one contiguous share of the samples (a
                                       // multiple of range_st = its sub-group size), cut into tiles of range_tile samples (a multiple too)
    int32_t env_base[MAX_HANDLES + 1];
    const int32_t *env_state[MAX_HANDLES];
    uint32_t *plan;
    uint32_t *tile_env;
};

template <class P>
__device__ __forceinline__ int handle_of(P env_base, int n_handles, int e) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < MAX_HANDLES; ++q) k += (q < n_handles && e >= env_base[q]) ? 1 : 0;
    return k;
}

// Exclusive prefix sums of one env_state word over the concatenated envs of all handles, and for every 128-sample tile the env
// its first sample belongs to.  One workgroup of 1024 threads: thread t sums a contiguous run of envs, the 1024 partial sums are
// scanned in LDS, then every thread bisects for its tiles.
// LDS_SUMS = false (ppg_policy_plan_small, the FC-chain policies): the per-env sums go through memory only and the kernel needs 4 KB of
// LDS -- those policies' forward kernels fill every CU to within 4 KB (two workgroups of 78 KB), and the OTHER species' plan runs on
// a side stream beside them: with 36 KB it found no CU to run on until a forward workgroup finished (fc256: 0.80 -> 0.89 ms per step).
template <bool LDS_SUMS>
__device__ __forceinline__ void plan_body(const PlanParams &K) {
    __shared__ uint32_t part[1024];
    // Up to PLAN_LDS_ENVS envs the per-env prefix sums stay in LDS as well and a thread keeps its run's counts in registers: ONE trip to
    // memory per launch (the counts) instead of four dependent ones (counts, counts again, two bisection steps over the sums just
    // written) -- the plan is a 1024-thread chain in front of every policy step (14 -> 9 us at 4096 envs).
    constexpr int PLAN_LDS_ENVS = 8192, PLAN_RUN = PLAN_LDS_ENVS / 1024;
    __shared__ uint32_t env_pre[LDS_SUMS ? PLAN_LDS_ENVS : 1];
    const int t = (int)threadIdx.x;
    const int per = (K.n_envs + 1023) / 1024;
    const bool in_lds = LDS_SUMS && K.n_envs <= PLAN_LDS_ENVS;
    const int lo = t * per < K.n_envs ? t * per : K.n_envs, hi = (lo + per) < K.n_envs ? (lo + per) : K.n_envs;
    // (the handle's env_state pointer by scalar comparisons: indexed with a per-lane handle number it is a vector load from the
    //  parameter block, one more dependent trip)
    auto count_of = [&](int e) -> uint32_t {
        const int32_t *base = K.env_state[0];
        int eb = 0;
#pragma unroll
        for (int q = 1; q < MAX_HANDLES; ++q) {
            const bool in = q < K.n_handles && e >= K.env_base[q];
            base = in ? K.env_state[q] : base;
            eb = in ? K.env_base[q] : eb;
        }
        return (uint32_t)base[(size_t)(e - eb) * PPG_ENV_WORDS + K.word];
    };
    uint32_t cnt[PLAN_RUN];
    uint32_t s = 0;
    if (in_lds) {
#pragma unroll
        for (int i = 0; i < PLAN_RUN; ++i) cnt[i] = (i < per && lo + i < hi) ? count_of(lo + i) : 0u;
#pragma unroll
        for (int i = 0; i < PLAN_RUN; ++i) s += cnt[i];
    } else {
        for (int e = lo; e < hi; ++e) s += count_of(e);
    }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t before = part[t] - s;
    const uint32_t all = part[1023];
    if (in_lds) {
#pragma unroll
        for (int i = 0; i < PLAN_RUN; ++i)
            if (i < per && lo + i < hi) {
                K.plan[PLAN_HDR + lo + i] = before;
                env_pre[lo + i] = before;
                before += cnt[i];
            }
    } else {
        for (int e = lo; e < hi; ++e) {
            K.plan[PLAN_HDR + e] = before;
            before += count_of(e);
        }
    }
    // exclusive prefix sum of env `e` as the bisections below read it
    auto prefix_of = [&](int e) -> uint32_t { return in_lds ? env_pre[e] : __builtin_nontemporal_load(&K.plan[PLAN_HDR + e]); };
    if (K.range_tile > 0) {
        // RANGE MODE: workgroup w owns samples [w S, (w + 1) S), S = the per-workgroup share rounded up to whole sub-groups, as tiles of
        // range_tile samples -- every workgroup the same number of FULL sub-groups (whole rounds of 128-sample tiles + a short last round
        // leave most of the chip idle in the last round and cut a two-sample sub-group off every tile: 7 % at the benchmark's 132 k prey)
        // (the arithmetic: ppg_policy_plan.h, shared with ppg_policy_plan_rows)
        const uint32_t slots = (uint32_t)K.slots, tsz = (uint32_t)K.range_tile;
        const ppg_plan_range rg = ppg_plan_range_of(all, slots, (uint32_t)K.range_st, tsz);
        const uint32_t S = rg.share, tpw = rg.tpw;
        if (t == 0) { K.plan[0] = all; K.plan[1] = S; K.plan[2] = tpw; }
        __threadfence_block();
        __syncthreads();
        const int n_slots = (int)(slots * tpw);
        for (int tile = t; tile < n_slots; tile += 1024) {
            uint32_t n = ppg_plan_range_slot((uint32_t)tile, S, tpw, tsz);
            if (all == 0u) { K.tile_env[tile] = 0u; continue; }
            n = ppg_plan_range_clamp(n, all);    // (an empty tile slot: behind every sample of the tiles in front of it -- keeps the list monotone)
            int ua = 0, ub = 1023;
            while (ua < ub) {
                const int mid = (ua + ub + 1) >> 1;
                if (part[mid - 1] <= n) ua = mid; else ub = mid - 1;
            }
            int a = ua * per < K.n_envs ? ua * per : K.n_envs - 1, b = (a + per - 1) < (K.n_envs - 1) ? (a + per - 1) : (K.n_envs - 1);
            while (a < b) {
                const int mid = (a + b + 1) >> 1;
                if (prefix_of(mid) <= n) a = mid; else b = mid - 1;
            }
            K.tile_env[tile] = (uint32_t)a;
        }
        return;
    }
    // Tiles: as many whole ROUNDS of 128-sample tiles as the resident workgroups (slots) can be given (the FC1 weights are re-read
    // once per tile, so tiles are as large as the accumulators allow), then ONE last round in which the remaining samples are
    // spread over the slots in tiles of 32 / 64 / 96 / 128.  A last round of a few full tiles would take as long as any other
    // round while most of the chip idles: at the benchmark's 134 k prey rows, 1047 tiles of 128 on 512 slots are 2.04 rounds and
    // cost three; 1024 + 92 tiles of 32 cost two and a short one.
    // (the arithmetic: ppg_policy_plan.h, shared with ppg_policy_plan_rows)
    const ppg_plan_tiles tl = ppg_plan_tiles_of(all, (uint32_t)K.slots);
    const uint32_t n_full = tl.n_full, ts = tl.ts;
    if (t == 0) { K.plan[0] = all; K.plan[1] = n_full; K.plan[2] = ts; }
    __threadfence_block();
    __syncthreads();   // (the prefix sums are re-read below by other threads of this workgroup: same CU, written through L1)
    const int n_tiles = (int)ppg_plan_tile_count(all, n_full, ts);
    // exclusive prefix of thread u's run = part[u] - (its own sum) = part[u - 1]: the bisection first finds the RUN in LDS (ten steps, no
    // memory round trip), then the env inside the run (`per` <= a handful of prefix sums from memory)
    for (int tile = t; tile < n_tiles; tile += 1024) {
        const uint32_t n = ppg_plan_tile_first((uint32_t)tile, n_full, ts);
        int ua = 0, ub = 1023;
        while (ua < ub) {   // the last run whose first env's prefix sum (= the inclusive sum of the runs before it) is <= n
            const int mid = (ua + ub + 1) >> 1;
            if (part[mid - 1] <= n) ua = mid; else ub = mid - 1;
        }
        int a = ua * per < K.n_envs ? ua * per : K.n_envs - 1, b = (a + per - 1) < (K.n_envs - 1) ? (a + per - 1) : (K.n_envs - 1);
        while (a < b) {   // the last env of that run whose prefix sum is <= n
            const int mid = (a + b + 1) >> 1;
            if (prefix_of(mid) <= n) a = mid; else b = mid - 1;
        }
        K.tile_env[tile] = (uint32_t)a;
    }
}
extern "C" __global__ void __launch_bounds__(1024) ppg_policy_plan(const PlanParams K) { plan_body<true>(K); }
extern "C" __global__ void __launch_bounds__(1024) ppg_policy_plan_small(const PlanParams K) { plan_body<false>(K); }
// both species' plans in one launch (workgroup 0: A, workgroup 1: B): one launch and one dependent-load chain less per step
extern "C" __global__ void __launch_bounds__(1024) ppg_policy_plan2(const PlanParams A, const PlanParams B) {
    if (blockIdx.x == 0) plan_body<true>(A); else plan_body<true>(B);
}

// The plan of a DENSE ROW TENSOR (ppg_policy_evaluate; ppg_policy_plan.h, part 2): the words plan_body would write for pseudo-envs of
// PPG_POLICY_ROWS_CHUNK rows of which the first `count` rows are in use, in closed form -- no scan, no bisection, no item depends on
// another, so it is a plain grid-stride loop.  The count is an argument, or a device word read HERE (nothing is read back).
struct RowsPlanParams {
    int64_t capacity, count;
    const int64_t *count_dev;
    uint32_t slots, range_tile, range_st;
    uint32_t *plan;                    // [PLAN_HDR + envs] header + prefix sums, then the first env of every tile
};
extern "C" __global__ void __launch_bounds__(256) ppg_policy_plan_rows(const RowsPlanParams K) {
    const int64_t count = K.count_dev ? *K.count_dev : K.count;
    const ppg_rows_shape s = ppg_rows_shape_of(K.capacity, count, K.slots, K.range_tile, K.range_st);
    uint32_t *tile_env = K.plan + PLAN_HDR + s.n_envs;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < s.items; i += gridDim.x * 256u) ppg_rows_item(i, s, K.plan, tile_env);
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
    return v;
}

// ReLU + round 8 accumulator registers to bf16: round first (v_cvt_pk_bf16_f32, two values per instruction), then ReLU on the PACKED
// pair -- a bf16 with the sign bit set is a negative 16-bit integer, so one v_pk_max_i16 with 0 clears both halves.  (Same values
// as ReLU before rounding: a negative number rounds to a negative number or -0, a positive one is untouched.)  12 instructions per
// 8 values instead of 8 v_max + 4 conversions... and half the v_max: the epilogues are a fifth of the convolutions' time.
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16x8 relu_pack8(const f32x16 &a, int r0) {
    u32x4_t w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 f = {a[r0 + 2 * j], a[r0 + 2 * j + 1]};
        const s16x2 zero = {0, 0};
        const s16x2 q = __builtin_elementwise_max(__builtin_bit_cast(s16x2, __builtin_convertvector(f, bf16x2)), zero);
        w[j] = __builtin_bit_cast(uint32_t, q);
    }
    return __builtin_bit_cast(bf16x8, w);
}

// n / d for 0 <= n < 1024, 1 <= d <= 255 with ONE full-rate instruction pair: (n * ceil(2^18 / d)) >> 18 (v_mul_u32_u24; the 32-bit
// multiplies and v_mul_hi the position arithmetic used before are quarter rate).  Exact: the error term n * (d ceil(2^18 / d) - 2^18)
// stays below 2^18.  The other products of the position arithmetic are 24-bit multiplies too.
constexpr int DIV_SHIFT = 18;
__device__ __forceinline__ int div_small(int n, uint32_t magic) { return (int)(__umul24((uint32_t)n, magic) >> DIV_SHIFT); }

// The weight fragments of one convolution layer and, per k-step, the offset of this lane half's K block: in registers.
//   CBIN   channel blocks (of 8) of the input image: 1 (4 real channels), 2, 4        K = 9 taps x CBIN blocks
//   MT     32-row tiles of output channels: 1 (16 real for conv1 / 32 for conv2), 2 (conv3)
// The bias rides in the GEMM: K block Q (the first one behind the 9 taps x CBIN channel blocks) holds the bias, split into a bf16
// head and a bf16 remainder, against a constant B fragment {1, 1, 0, ...} -- no bias loads per position tile and no registers to
// keep it in.  For CBIN = 1 that block is the second half of the last tap's k-step (free); for CBIN = 2 / 4 it costs one more MFMA
// per tile (10 instead of 9 / 19 instead of 18).
template <int CBIN, int MT>
struct ConvW {
    static constexpr int Q = 9 * CBIN, KS = (Q + 2) / 2;       // k-steps incl. the bias block
    static constexpr int KS_BIAS = Q / 2, H_BIAS = Q & 1;      // the bias block is block Q = 2 * KS_BIAS + H_BIAS
    bf16x8 a[MT][KS];
    int koff1[CBIN == 1 ? KS : 1];   // CBIN == 1 only: the tap of a k-step depends on the lane half -> per-lane offsets
    template <class KP>
    __device__ __forceinline__ void load(const KP &K, const bf16x8 *wfrag, int lane, int mt_base = 0) {
        const int h = lane >> 5;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt][ks] = wfrag[((mt_base + mt) * KS + ks) * 64 + lane];
            if (CBIN == 1) {
                const int q = 2 * ks + h;
                const int tap = q < Q ? q : 0;        // (the bias block: its B fragment is a constant, any in-bounds address will do)
                koff1[ks] = ((tap / 3 - 1) * K.Wp + tap % 3 - 1) * 8;
            }
        }
    }
    // element offset of k-step ks relative to (image of the sample, padded position, channel block in_blk + h * [CBIN > 1]):
    // K block q = 2 ks + h = tap * CBIN + cb.  For CBIN = 2: tap = ks, cb = h; for CBIN = 4: tap = ks >> 1, cb = 2 (ks & 1) + h --
    // the lane half only selects the channel block, which the caller folds into the base address, the rest is wave-uniform.
    // `d23` (CBIN = 4) = element distance from the image block that holds channels 0-7 to the one that holds channels 16-23.
    template <class KP>
    __device__ __forceinline__ int offset(const KP &K, int ks, int d23) const {
        if (CBIN == 1) return koff1[ks];
        // (CBIN = 8, the 64 -> 64 layers of ppg_policy_direct.h: four pairs of channel blocks d23 apart, tap = ks >> 2)
        const int tap = CBIN == 2 ? ks : CBIN == 4 ? ks >> 1 : ks >> 2;
        const int pr = CBIN == 2 ? 0 : CBIN == 4 ? (ks & 1) : (ks & 3);
        return pr * d23 + ((tap / 3 - 1) * K.Wp + tap % 3 - 1) * 8;
    }
    // The fragments were requested by load(): wait for them HERE, once, and hide their origin from the compiler.  Its wait-count
    // bookkeeping cannot follow a load across a loop's back edge: left alone it puts s_waitcnt vmcnt(0) in front of the first MFMA
    // of every position-tile loop -- which on this hardware also waits for every STORE the wavefront has issued since (conv3's, to
    // the scratch slot: one memory round trip per sub-group).
    __device__ __forceinline__ void landed() {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                u32x4_t v = __builtin_bit_cast(u32x4_t, a[mt][ks]);
                __asm__ volatile("" : "+v"(v));
                a[mt][ks] = __builtin_bit_cast(bf16x8, v);
            }
    }
};

// One convolution layer over the `ns` samples of a sub-group, this wavefront's share of the 32-position tiles.
//   COUT_BLOCKS  channel blocks written: 2 (conv1), 4 (conv2), 8 (conv3)
//   TO_GLOBAL    conv3: the result goes to the scratch slot X[sample][position][64] instead of an LDS image
// The LDS image of a sample is six channel blocks of [padded position][8]; which of them a layer reads and writes rotates with
// the sub-group (phase_conv): `in_blk` = the block of input channels 0-7 (8-15 in the next one; conv3's 16-31 always in blocks 2, 3),
// `out_blk0` / `out_blk1` = where the lane halves h = 0 / 1 put output channels 16 h .. 16 h + 15 (two blocks each).
template <int CBIN, int MT, int COUT_BLOCKS, bool TO_GLOBAL, int BATCH = 0, class KP>
__device__ __forceinline__ void conv_layer(const KP &K, const ConvW<CBIN, MT> &W, __bf16 *img, int sample_stride, int in_blk,
                                           int out_blk0, int out_blk1, GLOBAL_AS __bf16 *xg_tile,
                                           int s_local0, int ns, int nt_first, int nt_step, int lane, int mt_base = 0) {
    constexpr int KS = ConvW<CBIN, MT>::KS;
    const int h = lane >> 5, col = lane & 31;
    const int n_pos = ns * K.P;
    const int n_tiles = (n_pos + 31) / 32;
    const __bf16 *in = img + (in_blk + (CBIN > 1 ? h : 0)) * K.Wp2 * 8;
    __bf16 *out = img + (h ? out_blk1 : out_blk0) * K.Wp2 * 8;
    const int d23 = (2 - in_blk) * K.Wp2 * 8;
    for (int nt = nt_first; nt < n_tiles; nt += nt_step) {
        const int n = 32 * nt + col;
        const bool valid = n < n_pos;
        const int nn = valid ? n : 0;
        const int s = div_small(nn, K.magic_P), p = nn - __mul24(s, K.P);
        const int y = div_small(p, K.magic_R), x = p - __mul24(y, K.IW);
        const int pidx = __mul24(y + 1, K.Wp) + (x + 1);
        const __bf16 *base = in + __mul24(s, sample_stride) + pidx * 8;
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
        // the B fragment of k-step ks (the bias block's: {1, 1, 0 ...} in the lane half that holds it, zeros in the other)
        auto fragment = [&](int ks) -> bf16x8 {
            constexpr int KSB = ConvW<CBIN, MT>::KS_BIAS, HB = ConvW<CBIN, MT>::H_BIAS;
            bf16x8 v;
            if (ks == KSB && CBIN > 1) {
                v = zero8();
                if (h == HB) { v[0] = (__bf16)1.0f; v[1] = (__bf16)1.0f; }
            } else {
                v = *(const bf16x8 *)(base + W.offset(K, ks, d23));
                if (ks == KSB && h == HB) { v = zero8(); v[0] = (__bf16)1.0f; v[1] = (__bf16)1.0f; }
            }
            return v;
        };
        if constexpr (BATCH == 0) {
            // all of the tile's B fragments are requested before the first MFMA: the LDS latency is paid once per tile, and while this
            // wavefront's MFMA chain runs the SIMD's other wavefront has the LDS to itself.  (A software-pipelined version -- fragment k
            // of tile t + 1 re-read right behind the MFMA of tile t that consumed it, MFMA / DS-read alternation pinned with
            // sched_group_barrier, no lgkmcnt stall left in the loop -- measured the same: 1.39 vs 1.40 ms under load, 4.84 vs 4.92 ms
            // with 64 workgroups alone on their CUs.  What a tile waits for is its epilogue and the barriers, not LDS.)
            bf16x8 b[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = fragment(ks);
            __builtin_amdgcn_sched_barrier(0);   // (keep the reads together: left alone, the scheduler re-pairs each with its MFMA)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W.a[mt][ks], b[ks], acc[mt], 0, 0, 0);
        } else {
            // conv3 (19 k-steps): the fragments come in batches of BATCH, batch n + 1 requested before the MFMAs of batch n -- two
            // batches of registers instead of 76, which is what lets the weights of all three layers stay in registers
            constexpr int NB = (KS + BATCH - 1) / BATCH;
            bf16x8 b[2][BATCH];
#pragma unroll
            for (int i = 0; i < BATCH; ++i) b[0][i] = fragment(i);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb + 1 < NB) {
#pragma unroll
                    for (int i = 0; i < BATCH; ++i) if ((nb + 1) * BATCH + i < KS) b[(nb + 1) & 1][i] = fragment((nb + 1) * BATCH + i);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < BATCH; ++i)
                    if (nb * BATCH + i < KS) {
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W.a[mt][nb * BATCH + i], b[nb & 1][i], acc[mt], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!valid) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 2; ++j) {   // this lane's channels 32 mt + 16 h + 8 j .. + 7 = channel block 4 mt + 2 h + j
                const bf16x8 v = relu_pack8(acc[mt], 8 * j);
                if (TO_GLOBAL) {
                    // scratch slot X[sample][row tile][position][32]: a wavefront's 32 positions x 32 channels are 2 KB contiguous
                    *(GLOBAL_AS bf16x8 *)(xg_tile + (((size_t)(s_local0 + s) * 2 + (mt_base + mt)) * K.P + p) * 32 + 16 * h + 8 * j) = v;
                } else if (4 * (mt_base + mt) + 2 * h + j < COUT_BLOCKS) {   // (conv1: 16 real output channels: the h = 0 half only)
                    *(bf16x8 *)(out + __mul24(s, sample_stride) + (j * K.Wp2 + pidx) * 8) = v;
                }
            }
    }
}

// FC1 over the tile: M = 256 output features (A = weight fragments), N = up to 128 samples (B = the scratch slot X[sample][K1]),
// K in chunks of 32.  Wavefront w owns the feature row tiles 2w, 2w + 1 and ALL column tiles (2 x NT accumulators), so the same
// code serves tiles of 64, 96 and 128 samples.
//  - X: every wavefront needs every column, so the chunk (128 x 64 B) goes through LDS, brought by LDS-DMA loads
//    (global_load_lds_dwordx4: no registers, 1 KB per wave instruction) into one of THREE buffers, two chunks ahead of the one
//    being computed.  An LDS-DMA writes lane l's 16 bytes at base + 16 l, so the image cannot be padded; instead the 16-byte pieces
//    of row n sit at position piece ^ ((n >> 2) & 3) -- the swizzle is applied to the SOURCE address of the copy -- which makes the
//    16-lane groups of the fragment reads conflict-free.
//  - W: a wavefront's four fragments of a chunk are its own (nobody else reads them), so they go from L2 straight into registers,
//    one chunk ahead (two register sets, the chunk loop is unrolled by two; K1 / 32 = 2 R^2 is even).  Through LDS they cost a
//    third of the LDS bandwidth of the phase, which was its bound: with two workgroups per CU the fragment reads + DMA writes of a
//    chunk took longer than its 16 MFMAs per wavefront.
// Loads complete in order, so "chunk c is here" is a count: a step requests W(c + 1) [4 loads] and then X(c + 2) [2 loads]; at the
// top of step c everything but the two X(c + 1) loads must have landed: s_waitcnt vmcnt(2).
constexpr int FC1_BUF = TILE * 64;                   // bytes per X buffer

// (Cache hints were tried for the scratch slot -- nt stores in conv3, nt on these loads, nt on the observation reads, so that the
// streaming data would not push FC1's weights out of L2: every combination was 5-10 % SLOWER.)
__device__ __forceinline__ void glds16(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)g, (void __attribute__((address_space(3))) *)l, 16, 0, 0);
}

__device__ __forceinline__ void fc1_issue_x(int K1, const __bf16 *xg_tile, unsigned char *stage, int c, int buf, int wave, int lane) {
    unsigned char *xb = stage + (size_t)buf * FC1_BUF;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i0 = (wave * 2 + j) * 64, i = i0 + lane;
        const int row = i >> 2, q = (i & 3) ^ ((row >> 2) & 3);
        glds16(xg_tile + (size_t)row * K1 + 32 * c + 8 * q, xb + (size_t)i0 * 16);
    }
}

// The weight loads are written as inline assembly ON PURPOSE: hipcc's wait-count bookkeeping cannot follow loads whose results
// are consumed one loop iteration later in a rotating register set -- it puts s_waitcnt vmcnt(0) in front of the first MFMA of
// every chunk, i.e. it waits for the loads it has just issued.  Loads it does not know about it does not wait for; the explicit
// s_waitcnt vmcnt(2) at the top of each step is what guarantees their arrival, and fc1_landed() (an empty asm that "redefines" the
// registers behind that wait) keeps every use of them below it.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void fc1_issue_w(const GLOBAL_AS bf16x8 *wlane, int c, u32x4 (&w)[2][2]) {
    const GLOBAL_AS bf16x8 *p0 = wlane + (size_t)c * 1024, *p1 = p0 + 512;   // k2 = 0 / 1: 8 KB apart; m = 1: + 1 KB
    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=v"(w[0][0]) : "v"(p0) : "memory");
    __asm__ volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(w[0][1]) : "v"(p0) : "memory");
    __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=v"(w[1][0]) : "v"(p1) : "memory");
    __asm__ volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(w[1][1]) : "v"(p1) : "memory");
}
__device__ __forceinline__ void fc1_landed(u32x4 (&w)[2][2]) {
    __asm__ volatile("" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[1][0]), "+v"(w[1][1]));
}

template <int NT>
__device__ __forceinline__ void fc1_compute(const unsigned char *xb, const u32x4 (&w)[2][2], f32x16 (&acc)[2][NT], int lane) {
    const int h = lane >> 5, col = lane & 31;
    // all 2 x NT fragments of the chunk are requested before its first MFMA (the LDS latency is paid once per chunk)
    bf16x8 x[2][NT];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
        const int q = 2 * k2 + h;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = 32 * t + col;
            x[k2][t] = *(const bf16x8 *)(xb + n * 64 + 16 * (q ^ ((n >> 2) & 3)));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[k2][m]), x[k2][t], acc[m][t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);   // (or the next step's wait + barrier are scheduled in front of these MFMAs: nothing hidden)
}

#ifdef PPG_EXPERIMENTS
struct FcTimes {   // diagnostic builds: cycles a wave spends in the chunk loop's wait / barrier / the rest
    long long t[3] = {0, 0, 0}, prev = 0;
    __device__ __forceinline__ void start() { prev = (long long)clock64(); }
    __device__ __forceinline__ void add(int i) { const long long now = (long long)clock64(); t[i] += now - prev; prev = now; }
};
#else
struct FcTimes {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void add(int) {}
};
#endif

// one chunk: wait for it, meet, request W(c + 1) and X(c + 2) (compile-time switches: with a run-time condition around the loads
// the compiler's own wait-count bookkeeping gives up at the join and drains ALL loads before the MFMAs), compute.
template <int NT, bool ISSUE_W, bool ISSUE_X>
__device__ __forceinline__ void fc1_step(const GLOBAL_AS bf16x8 *wlane, int K1, const __bf16 *xg_tile, unsigned char *stage, int c, int buf,
                                         u32x4 (&w_cur)[2][2], u32x4 (&w_next)[2][2], f32x16 (&acc)[2][NT], int wave, int lane, FcTimes &T) {
    if (ISSUE_W) __asm__ volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    fc1_landed(w_cur);
    T.add(0);
    __builtin_amdgcn_s_barrier();   // everybody's X copies of chunk c are in LDS, and everybody is done with chunk c - 1's buffer
    T.add(1);
    if (ISSUE_W) fc1_issue_w(wlane, c + 1, w_next);
    if (ISSUE_X) fc1_issue_x(K1, xg_tile, stage, c + 2, buf >= 1 ? buf - 1 : 2, wave, lane);
    fc1_compute<NT>(stage + (size_t)buf * FC1_BUF, w_cur, acc, lane);
    T.add(2);
}

template <int NT>
__device__ __forceinline__ void fc1_staged(const bf16x8 *w1, int K1, const __bf16 *xg_tile, unsigned char *stage, f32x16 (&acc)[2][NT],
                                           int wave, int lane, FcTimes &T) {
    const int n_chunks = K1 / 32;    // = 2 R^2: even, >= 18
    const GLOBAL_AS bf16x8 *wlane = (const GLOBAL_AS bf16x8 *)w1 + (2 * wave) * 64 + lane;
    u32x4 w[2][2][2];
    fc1_issue_x(K1, xg_tile, stage, 0, 0, wave, lane);
    fc1_issue_w(wlane, 0, w[0]);
    fc1_issue_x(K1, xg_tile, stage, 1, 1, wave, lane);
    int buf = 0;
    T.start();
    for (int c = 0; c + 2 < n_chunks; c += 2) {   // (chunk c uses LDS buffer c % 3 and register set c % 2)
        fc1_step<NT, true, true>(wlane, K1, xg_tile, stage, c, buf, w[0], w[1], acc, wave, lane, T);
        buf = buf == 2 ? 0 : buf + 1;
        fc1_step<NT, true, true>(wlane, K1, xg_tile, stage, c + 1, buf, w[1], w[0], acc, wave, lane, T);
        buf = buf == 2 ? 0 : buf + 1;
    }
    fc1_step<NT, true, false>(wlane, K1, xg_tile, stage, n_chunks - 2, buf, w[0], w[1], acc, wave, lane, T);
    buf = buf == 2 ? 0 : buf + 1;
    fc1_step<NT, false, false>(wlane, K1, xg_tile, stage, n_chunks - 1, buf, w[1], w[0], acc, wave, lane, T);
    __syncthreads();
}

// M = 256 output features from K = 16 * KSTEPS inputs held in LDS as bsrc[sample][...] (B fragments: 16 bytes at
// bsrc + sample * bstride + 16 ks + 8 h); the weight fragments come straight from L2, fetched two k-steps ahead of their use.
template <int KSTEPS, int NT>
__device__ __forceinline__ void fc_256(const bf16x8 *wfrag, const __bf16 *bsrc, size_t bstride, f32x16 (&acc)[2][NT], int wave, int lane) {
    const int h = lane >> 5, col = lane & 31;
    const __bf16 *b0 = bsrc + (size_t)col * bstride + 8 * h;
    const bf16x8 *wa = wfrag + (size_t)(2 * wave) * 64 + lane;
    bf16x8 w[3][2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int m = 0; m < 2; ++m) w[d][m] = wa[((size_t)d * 8 + m) * 64];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const int cur = ks % 3, nxt = (ks + 2) % 3;
        if (ks + 2 < KSTEPS) {
#pragma unroll
            for (int m = 0; m < 2; ++m) w[nxt][m] = wa[((size_t)(ks + 2) * 8 + m) * 64];
        }
        bf16x8 x[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = *(const bf16x8 *)(b0 + (size_t)(32 * t) * bstride + 16 * ks);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[cur][m], x[t], acc[m][t], 0, 0, 0);
    }
}

template <int NT>
__device__ __forceinline__ void fc_init(const float *bias, f32x16 (&acc)[2][NT], int wave, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b = *(const GLOBAL_AS f32x4 *)(bias + 32 * (2 * wave + m) + 16 * h + 4 * g);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[m][t][4 * g + i] = b[i];
        }
}

// ReLU(acc) -> H[sample][feature] (bf16, LDS): 32 bytes per lane and tile
template <int NT>
__device__ __forceinline__ void fc_store(const f32x16 (&acc)[2][NT], __bf16 *H, int wave, int lane) {
    const int h = lane >> 5, col = lane & 31;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                *(bf16x8 *)(H + (size_t)(32 * t + col) * HSTRIDE + 32 * (2 * wave + m) + 16 * h + 8 * j) = relu_pack8(acc[m][t], 8 * j);
}

__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// The parameter block is read in place from the kernarg segment (scalar loads at the use sites): by value it would sit in ~100
// SGPRs for the whole kernel.  The three phases of a tile are separate NON-INLINED functions: each gets its own register
// allocation (inlined into one body, hipcc hoists address arithmetic of every phase to the top of the tile loop and spills
// hundreds of registers -- scratch reloads then sit between the LDS-DMA loads of FC1 and force vmcnt(0) waits).
typedef const __attribute__((address_space(4))) PolParams *KPtr;
// Arguments of a non-inlined device function arrive in VECTOR registers: the compiler has to treat them (and everything loaded
// through them) as possibly different per lane -- vector loads of the parameters, loop bounds in VGPRs, exec-masked "divergent"
// loops, conservative s_waitcnt vmcnt(0) at every join.  So the phases make their arguments uniform again with v_readfirstlane,
// the kernarg pointer included (__builtin_amdgcn_kernarg_segment_ptr() is a null pointer inside a callee).
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uintptr_t uniform(uintptr_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uintptr_t)hi << 32) | lo;
}
template <class T>
__device__ __forceinline__ T *uniform(T *p) { return (T *)uniform((uintptr_t)p); }
__device__ __forceinline__ KPtr uniform(KPtr p) { return (KPtr)uniform((uintptr_t)p); }

// How phase A keeps the observation values it has requested for the next sub-group: in the rows' own element type (the
// conversion to bf16 -- via float, round to nearest even both times, as ppg_step's bfloat16 rows are made -- happens when they are
// written to LDS, one sub-group later); the 16-channel float64 variant converts to float at once (64 registers otherwise).
template <int OBS, int NCH>
struct ObsRaw {
    typedef typename std::conditional<OBS == 2, uint16_t, typename std::conditional<OBS == 1, float, double>::type>::type elem;
    // (bfloat16 rows travel as the zero-extended 16 bits in a register of their own: two 16-bit values in one register would be
    //  packed as soon as they are loaded, i.e. waited for)
    typedef typename std::conditional<OBS == 2, uint32_t, typename std::conditional<OBS == 0 && (NCH > 8), float, elem>::type>::type type;
    // (the empty asm pins the conversion -- and with it the wait for the load -- to the place where the value is staged: a pure
    //  function of a loaded value is otherwise scheduled right behind its load)
    static __device__ __forceinline__ __bf16 to_bf16(type v) {
        __asm__ volatile("" : "+v"(v));
        if constexpr (OBS == 2) return __builtin_bit_cast(__bf16, (uint16_t)v);
        else return (__bf16)(float)v;
    }
};


// ---- phase A: the tile's sample table, then the convolutions, ST samples at a time -> scratch slot X ----
// NCH = input channel slots a thread stages per position: 4 (channel-first: the four observation channels), 8 or 16 (channels-last:
// R <= 8 / R <= 15 channels); conv1 reads CB1 = 1 or 2 channel blocks of 8.
// OBS = element type of the observation rows: 0 float64, 1 float32, 2 bfloat16 (ppg_config.obs_dtype)
template <int OBS, int NCH>
__device__ __noinline__ void phase_conv(KPtr Kp, unsigned char *lds, int tile_, int n0_, int nt_samples_, __bf16 *xg_tile_) {
    constexpr int CB1 = NCH > 8 ? 2 : 1;
    const auto &K = *uniform(Kp);
    const int tile = uniform(tile_), n0 = uniform(n0_), nt_samples = uniform(nt_samples_);
    __bf16 *xg_tile = uniform(xg_tile_);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *tab = (unsigned long long *)lds;
    __bf16 *img = (__bf16 *)(lds + TILE * 16);
    const int blk = K.Wp2 * 8, sample_stride = 6 * blk;    // elements per channel block and per sample: six blocks of [padded position][8]
    const int img_elems = K.ST * sample_stride;
#ifdef PPG_EXPERIMENTS
    long long tacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = (long long)clock64();
#define PPG_TA(i) do { const long long now_ = (long long)clock64(); tacc[i] += now_ - tprev; tprev = now_; } while (0)
#else
#define PPG_TA(i) do { } while (0)
#endif
    // conv3: wavefronts 0, 1 compute output channels 0-31, wavefronts 2, 3 channels 32-63, each for every other position tile --
    // so a wavefront needs ONE row tile's weight fragments (76 registers).  With those of conv1 / conv2 (20 - 40 / 40 registers)
    // they stay in registers for the whole sample tile (requested here, awaited behind the table and the zero fill).
    ConvW<4, 1> w3c;
    ConvW<CB1, 1> w1c;
    ConvW<2, 1> w2c;
    w3c.load(K, K.wc3, lane, wave >> 1);
    w1c.load(K, K.wc1, lane);
    w2c.load(K, K.wc2, lane);
    // sample -> (handle, env, row): walk forward from the tile's first env (a tile spans a handful of envs)
    if (tid < TILE) {
        unsigned long long src = 0, dst = 0;
        if (tid < nt_samples) {
            const uint32_t n = (uint32_t)(n0 + tid);
            int lo = (int)K.tile_env[tile];
            while (lo + 1 < K.n_envs && K.plan[PLAN_HDR + 1 + lo] <= n) ++lo;
            const int e = lo, row = (int)(n - K.plan[PLAN_HDR + e]);
            const int k = handle_of(K.env_base, K.n_handles, e);
            const int b = e - K.env_base[k];
            src = (unsigned long long)(uintptr_t)(K.obs[k] + ((size_t)b * K.cap + row) * (size_t)K.obs_elems * (OBS == 2 ? 2 : OBS == 1 ? 4 : 8));
            dst = (unsigned long long)(uintptr_t)(K.actions[k] + (size_t)b * K.S + K.slot0 + row);
        }
        tab[2 * tid] = src;
        tab[2 * tid + 1] = dst;
    }
    // halo rings (and the unused channels of the input image) are zero and stay zero: only interiors are ever written
    for (int i = tid; i < img_elems / 8; i += 256) ((bf16x8 *)img)[i] = zero8();
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    w3c.landed();
    w1c.landed();
    w2c.landed();
    __syncthreads();
    GLOBAL_AS __bf16 *xg = (GLOBAL_AS __bf16 *)xg_tile;
    // The observation values of a sub-group are REQUESTED two sub-groups ahead and WRITTEN to LDS one sub-group ahead (`stage`, into
    // the image block conv1 will read), so neither wait meets anything young: on this hardware a wavefront's loads and stores
    // complete in issue order and share one counter, so waiting for a load also waits for every store issued before... and, as the
    // compiler cannot count the stores of a loop, for every one issued AFTER it too.  Here the youngest stores in front of a wait are
    // conv3's of the previous sub-group, two layers old.  (The values stay in the rows' element type until they are staged: a
    // conversion at request time would wait for the loads it has just issued.)  A thread stages at most two positions (ST * P <= 512).
    typedef typename ObsRaw<OBS, NCH>::type raw_t;
    raw_t pre[2][NCH];
    auto request = [&](int s0) {
        const int left = nt_samples - s0, ns = left < K.ST ? left : K.ST;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = tid + 256 * j;
#pragma unroll
            for (int c = 0; c < NCH; ++c) pre[j][c] = (raw_t)0;
            if (idx < ns * K.P) {
                const int s = div_small(idx, K.magic_P), p = idx - __mul24(s, K.P);
                typedef typename ObsRaw<OBS, NCH>::elem elem_t;   // bfloat16 rows: what ppg_step rounded is what conv1 gets, bit for bit
                const GLOBAL_AS elem_t *src = (const GLOBAL_AS elem_t *)(uintptr_t)tab[2 * (s0 + s)] + p * K.p_stride;
#pragma unroll
                for (int c = 0; c < NCH; ++c) if (NCH == 4 || c < K.cin) pre[j][c] = (raw_t)src[c * K.c_stride];
            }
        }
    };
    auto stage = [&](int s0, int in_blk) {
        const int left = nt_samples - s0, ns = left < K.ST ? left : K.ST;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = tid + 256 * j;
            if (idx < ns * K.P) {
                const int s = div_small(idx, K.magic_P), p = idx - __mul24(s, K.P);
                const int y = div_small(p, K.magic_R), x = p - __mul24(y, K.IW);
#pragma unroll
                for (int cb = 0; cb < CB1; ++cb) {
                    bf16x8 v = zero8();
#pragma unroll
                    for (int c = 0; c < (NCH < 8 ? NCH : 8); ++c) v[c] = ObsRaw<OBS, NCH>::to_bf16(pre[j][8 * cb + c]);
                    *(bf16x8 *)(img + __mul24(s, sample_stride) + ((in_blk + cb) * K.Wp2 + __mul24(y + 1, K.Wp) + (x + 1)) * 8) = v;
                }
            }
        }
    };
    // Which image blocks a layer uses alternates with the sub-group k, so that the NEXT sub-group's input can be staged while conv3
    // still reads its own:        conv1: in -> c1, c1 + 1     conv2: c1, c1 + 1 -> in, in + 1, 2, 3     conv3: in, in + 1, 2, 3 -> scratch slot
    // with (in, c1) = (4, 0) for even k and (0, 4) for odd k; the input of sub-group k + 1 goes to block c1 (+ 1) once conv2 is done.
    request(0);
    stage(0, 4);
    if (K.ST < nt_samples) request(K.ST);
    __syncthreads();
    PPG_TA(0);
    int in_blk = 4, c1_blk = 0;
    for (int s0 = 0; s0 < nt_samples; s0 += K.ST) {
        const int ns = (nt_samples - s0) < K.ST ? (nt_samples - s0) : K.ST;
        conv_layer<CB1, 1, 2, false>(K, w1c, img, sample_stride, in_blk, c1_blk, c1_blk, nullptr, 0, ns, wave, 4, lane);
        PPG_TA(3);
        __syncthreads();
        PPG_TA(4);
        conv_layer<2, 1, 4, false>(K, w2c, img, sample_stride, c1_blk, in_blk, 2, nullptr, 0, ns, wave, 4, lane);
        PPG_TA(5);
        __syncthreads();
        PPG_TA(6);
        if (s0 + K.ST < nt_samples) {
            stage(s0 + K.ST, c1_blk);
            PPG_TA(1);
            if (s0 + 2 * K.ST < nt_samples) request(s0 + 2 * K.ST);
        }
        PPG_TA(7);
        conv_layer<4, 1, 8, true, 5>(K, w3c, img, sample_stride, in_blk, 0, 0, xg, s0, ns, wave & 1, 2, lane, wave >> 1);
        PPG_TA(8);
        __syncthreads();
        PPG_TA(9);
        const int t_ = in_blk; in_blk = c1_blk; c1_blk = t_;
    }
    // rows of the scratch slot behind the last sample of a partial tile hold older data: finite bf16 values whose columns are
    // never stored.  (The slot is zero-filled at creation, so they are never NaN patterns.)
    // This workgroup's stores to its scratch slot are re-read by FC1: drain them, meet, drop stale L1 lines.
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef PPG_EXPERIMENTS
    PPG_TA(0);   // (the drain + acquire at the end goes with the start-up work)
    if (K.timeline && lane == 0)
        for (int i = 0; i < 10; ++i) K.timeline[(size_t)tile * 64 + 8 + 12 * wave + i] = (unsigned long long)tacc[i];
#endif
}

// ---- phase B: FC1 from the scratch slot, ReLU -> H ----
template <int NT>
__device__ __noinline__ void phase_fc1(KPtr Kp, unsigned char *lds, const __bf16 *xg_tile_, int tile_ = 0) {
    const auto &K = *uniform(Kp);
    FcTimes T;
    const __bf16 *xg_tile = uniform(xg_tile_);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char *overlay = lds + TILE * 16;
    f32x16 acc[2][NT];
    fc_init<NT>(K.b1, acc, wave, lane);
    fc1_staged<NT>(K.w1, K.K1, xg_tile, overlay, acc, wave, lane, T);   // (staging buffers overlay the images)
#ifdef PPG_EXPERIMENTS
    if (K.timeline && lane == 0) {   // [8 + 12 wave + 10 / 11] = wait / barrier cycles of the chunk loop, [56 + wave] = the rest of it
        unsigned long long *t = K.timeline + (size_t)uniform(tile_) * 64;
        t[8 + 12 * wave + 10] = (unsigned long long)T.t[0];
        t[8 + 12 * wave + 11] = (unsigned long long)T.t[1];
        t[56 + wave] = (unsigned long long)T.t[2];
    }
#endif
    __syncthreads();
    fc_store<NT>(acc, (__bf16 *)overlay, wave, lane);      // (so does H)
    __syncthreads();
}

// ---- phases C, D: FC2 from H back into H; logits; actions ----
template <int NT>
__device__ __noinline__ void phase_head(KPtr Kp, unsigned char *lds, int n0_, int nt_samples_) {
    const auto &K = *uniform(Kp);
    const int n0 = uniform(n0_), nt_samples = uniform(nt_samples_);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long *tab = (const unsigned long long *)lds;
    __bf16 *H = (__bf16 *)(lds + TILE * 16);
    if (K.n_hidden >= 2) {   // (one hidden layer: the logits come straight from FC1's output)
        f32x16 acc[2][NT];
        fc_init<NT>(K.b2, acc, wave, lane);
        fc_256<16, NT>(K.w2, H, (size_t)HSTRIDE, acc, wave, lane);
        __syncthreads();
        fc_store<NT>(acc, H, wave, lane);
        __syncthreads();
    }
    if (wave >= NT) return;   // (one 32-sample column tile per wavefront)
    // logits = W3 (actions padded to 32 rows) x H^T, one 32-sample column tile per wavefront
    const int h = lane >> 5, col = lane & 31;
    f32x16 lg;
#pragma unroll
    for (int r = 0; r < 16; ++r) lg[r] = K.b3[16 * h + r];
    const __bf16 *hb = H + (size_t)(32 * wave + col) * HSTRIDE + 8 * h;
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks)
        lg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(K.w3[ks * 64 + lane], *(const bf16x8 *)(hb + 16 * ks), lg, 0, 0, 0);
    // lane (h = 0) of a column holds the logits of actions 0-15, its partner lane + 32 those of actions 16-31
    float mine[16], other[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { mine[r] = lg[r]; other[r] = __shfl_xor(mine[r], 32, 64); }
    const int s_local = 32 * wave + col;
    if (h == 0 && s_local < nt_samples) {
        float logit[32];
#pragma unroll
        for (int r = 0; r < 16; ++r) { logit[r] = mine[r]; logit[16 + r] = other[r]; }
        if (K.logits) {
            float *lo = K.logits + (size_t)(n0 + s_local) * K.n_actions;
#pragma unroll
            for (int a = 0; a < 32; ++a) if (a < K.n_actions) lo[a] = logit[a];
        }
        int8_t *dst = (int8_t *)(uintptr_t)tab[2 * s_local + 1];
        // Philox counter of this agent = (global env index, row slot): recovered from where its action goes.  (Never the address
        // itself: the same seed must give the same actions whatever tensor they are written to.)
        uint32_t c_env = 0, c_slot = 0;
        if (K.sample) {
            int k = 0;
#pragma unroll
            for (int q = 1; q < MAX_HANDLES; ++q)
                if (q < K.n_handles && (uintptr_t)dst >= (uintptr_t)K.actions[q] &&
                    (uintptr_t)dst < (uintptr_t)K.actions[q] + (size_t)(K.env_base[q + 1] - K.env_base[q]) * (size_t)K.S) k = q;
            const uint32_t off = (uint32_t)((uintptr_t)dst - (uintptr_t)K.actions[k]);
            const uint32_t b = off / (uint32_t)K.S;
            c_env = (uint32_t)K.env_base[k] + b;
            c_slot = off - b * (uint32_t)K.S;
        }
        uint32_t rnd[4] = {0, 0, 0, 0};
        int best = 0;
        float bestv = -INFINITY;
#pragma unroll
        for (int a = 0; a < 32; ++a) {
            if (a >= K.n_actions) continue;
            float v = logit[a];
            if (K.sample) {   // Gumbel-max: argmax(logit - log(-log u)) ~ softmax(logits)
                if ((a & 3) == 0) philox(c_env, c_slot, (uint32_t)(a >> 2), 0x504F4C31u, K.seed_lo, K.seed_hi, rnd);
                const float u = (float)(rnd[a & 3] >> 9) * (1.0f / 8388608.0f) + (1.0f / 16777216.0f);   // 23 bits: 2^-24 <= u < 1, exactly
                v -= __logf(-__logf(u));
            }
            if (v > bestv) { bestv = v; best = a; }
        }
        *dst = (int8_t)best;
    }
}

template <int OBS, int NCH>
__device__ __forceinline__ void policy_main(KPtr Kp, unsigned char *lds) {
    const int N = (int)Kp->plan[0], n_full = (int)Kp->plan[1], ts = (int)Kp->plan[2];
    const int n_tiles = n_full + (N - n_full * TILE + ts - 1) / ts;
    __bf16 *xg_tile = Kp->xg + (size_t)blockIdx.x * TILE * Kp->K1;
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const int size = tile < n_full ? TILE : ts;
        const int n0 = tile < n_full ? tile * TILE : n_full * TILE + (tile - n_full) * ts;
        const int nt_samples = (N - n0) < size ? (N - n0) : size;
        __syncthreads();   // the previous tile's readers of H / the table are done
#ifdef PPG_EXPERIMENTS
        unsigned long long *tl = Kp->timeline ? Kp->timeline + (size_t)tile * 64 : nullptr;
        const bool stamp = tl && threadIdx.x == 0;
        if (stamp) { tl[0] = blockIdx.x; tl[1] = (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32); tl[2] = (unsigned)nt_samples; tl[3] = wall_clock64(); }
#define PPG_POL_STAMP(i) do { if (stamp) tl[i] = wall_clock64(); } while (0)
#else
#define PPG_POL_STAMP(i) do { } while (0)
#endif
        phase_conv<OBS, NCH>(Kp, lds, tile, n0, nt_samples, xg_tile);
        PPG_POL_STAMP(4);
        if (size <= 32) { phase_fc1<1>(Kp, lds, xg_tile, tile); PPG_POL_STAMP(5); phase_head<1>(Kp, lds, n0, nt_samples); }
        else if (size <= 64) { phase_fc1<2>(Kp, lds, xg_tile, tile); PPG_POL_STAMP(5); phase_head<2>(Kp, lds, n0, nt_samples); }
        else if (size <= 96) { phase_fc1<3>(Kp, lds, xg_tile, tile); PPG_POL_STAMP(5); phase_head<3>(Kp, lds, n0, nt_samples); }
        else { phase_fc1<4>(Kp, lds, xg_tile, tile); PPG_POL_STAMP(5); phase_head<4>(Kp, lds, n0, nt_samples); }
        PPG_POL_STAMP(6);
    }
}

#define PPG_POLICY_KERNEL(name, OBS, NCH)                                                        \
    extern "C" __global__ void __launch_bounds__(256, 2) name(const PolParams K) {               \
        extern __shared__ __attribute__((aligned(16))) unsigned char lds[];                      \
        policy_main<OBS, NCH>((KPtr)__builtin_amdgcn_kernarg_segment_ptr(), lds);                \
    }
PPG_POLICY_KERNEL(ppg_policy_forward_f64, 0, 4)          // channel-first: R x R image, 4 channels
PPG_POLICY_KERNEL(ppg_policy_forward_f32, 1, 4)
PPG_POLICY_KERNEL(ppg_policy_forward_bf16, 2, 4)
PPG_POLICY_KERNEL(ppg_policy_forward_hwc8_f64, 0, 8)     // channels-last: 4 x R image, R <= 8 channels
PPG_POLICY_KERNEL(ppg_policy_forward_hwc8_f32, 1, 8)
PPG_POLICY_KERNEL(ppg_policy_forward_hwc8_bf16, 2, 8)
PPG_POLICY_KERNEL(ppg_policy_forward_hwc16_f64, 0, 16)   // channels-last, 9 <= R <= 15 channels (two channel blocks into conv1)
PPG_POLICY_KERNEL(ppg_policy_forward_hwc16_f32, 1, 16)
PPG_POLICY_KERNEL(ppg_policy_forward_hwc16_bf16, 2, 16)

// ---- ppg_policy_update: float32 parameters in device memory -> the weight image, through the repack map (ppg_policy_pack.h) ----
// One launch per policy, grid-stride over the image's 16-byte units of eight bf16 words and, behind them, the floats of the bias block.
// A lane reads its unit's eight map entries (two 16-byte loads), gathers the eight parameters they name and writes the unit with one
// 16-byte store.  The table of source pointers is read in place from the kernarg segment (indexed per lane: by value it would be a
// private array).  No atomics, no LDS; latency-bound: a few dependent loads per lane, about a thousand workgroups for the largest image.
struct RepackParams {
    const float *src[PPG_SRC_N];   // DEVICE pointers (PPG_SRC_*); those of layers the shape does not have are in no map entry and never read
    const int32_t *map;            // [8 n_units + n_bias] entries (the map behind its header)
    u32x4_t *image;                // dev_weights: n_units units from its first byte on
    float *bias;                   // the bias block inside dev_weights
    uint32_t n_units, n_bias;
};
typedef int32_t i32x4_t __attribute__((ext_vector_type(4)));
extern "C" __global__ void __launch_bounds__(256) ppg_policy_repack(const RepackParams K) {
    const auto *Kp = (const __attribute__((address_space(4))) RepackParams *)__builtin_amdgcn_kernarg_segment_ptr();
    const float *const __attribute__((address_space(4))) *src = Kp->src;
    const uint32_t n = K.n_units + K.n_bias, stride = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        if (i < K.n_units) {
            const GLOBAL_AS i32x4_t *m = (const GLOBAL_AS i32x4_t *)K.map + 2 * (size_t)i;
            const i32x4_t e0 = m[0], e1 = m[1];
            const int32_t e[8] = {e0[0], e0[1], e0[2], e0[3], e1[0], e1[1], e1[2], e1[3]};
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = ppg_repack_fetch(e[j], src);   // (eight independent gathers, all in flight)
            u32x4_t v;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = (uint32_t)ppg_bf16_bits(ppg_repack_finish(e[2 * j], f[2 * j])) | (uint32_t)ppg_bf16_bits(ppg_repack_finish(e[2 * j + 1], f[2 * j + 1])) << 16;
            *((GLOBAL_AS u32x4_t *)K.image + i) = v;
        } else {
            const uint32_t k = i - K.n_units;
            K.bias[k] = ppg_repack_value(K.map[8 * (size_t)K.n_units + k], src);
        }
    }
}

}  // namespace ppgpol

#include "ppg_policy_direct.h"
#include "ppg_policy_pipe.h"
