// ppg_hip.hip -- libppg_hip.so: the gfx950 kernels and the HIP backend of include/ppg.h.
//
// Build (see __graft_entry__.build_hip): this unit and ppg_kernels.hip once per (PPG_TU_GEN, PPG_TU_NQ) pair, each with
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, then hipcc -shared -o libppg_hip.so *.o
// -ffp-contract=off: energies are IEEE float64 sums that must round exactly like CPython's.
#include <hip/hip_runtime.h>

#include "ppg_host.h"

// The kernels are compiled in separate translation units (ppg_kernels.hip, one per generation and prey-register
// count) so that the build runs in parallel; this unit holds the host side and only declares them (the register caps are ppg_kernels.hip's).
// kernel name: ppg_<mode>_[p2]q<prey registers>[g]   (g = generic observation geometry, descriptors in LDS; p2 = 128 predator rows);
// ppg2_* = second generation (two agent types, stochastic reproduction)
#define PPG_DECLARE_KERNEL(name) extern "C" __global__ void name(const ppg::KParams P);
#define PPG_K(name, NQ, MODE, FAST) PPG_DECLARE_KERNEL(name)
#define PPG_K2(name, NQ, MODE, FAST) PPG_DECLARE_KERNEL(name)
#define PPG_K3(name, NQ, MODE) PPG_DECLARE_KERNEL(name)
#define PPG_K4(name, NQ, MODE) PPG_DECLARE_KERNEL(name)
#define PPG_KW3(name, NQ, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KW4(name, NQ, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KW(name, NQ, FAST, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KW2(name, NQ, FAST, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KC(name, NQ, GEN2, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KC3(name, NQ) PPG_DECLARE_KERNEL(name)
#define PPG_KCM(name, NQ, GEN2) PPG_DECLARE_KERNEL(name)
#define PPG_KCH(name, NQ) PPG_DECLARE_KERNEL(name)
#define PPG_KCR(name, NQ, GEN2, NW) PPG_DECLARE_KERNEL(name)
#define PPG_KP(name, NQ, MODE) PPG_DECLARE_KERNEL(name)
#define PPG_KP2(name, NQ, MODE) PPG_DECLARE_KERNEL(name)
#include "ppg_kernel_list.h"

PPG_DEFINE_KERNELSC(1)
PPG_DEFINE_KERNELSC(2)
PPG_DEFINE_KERNELS(1)
PPG_DEFINE_KERNELS(2)
PPG_DEFINE_KERNELS(4)
PPG_DEFINE_KERNELS2(1)
PPG_DEFINE_KERNELS2(2)
PPG_DEFINE_KERNELS2(4)
PPG_DEFINE_KERNELS3(1)
PPG_DEFINE_KERNELS3(2)
PPG_DEFINE_KERNELS3(4)
PPG_DEFINE_KERNELS4(1)
PPG_DEFINE_KERNELS4(2)
PPG_DEFINE_KERNELS4(4)
PPG_DEFINE_KERNELSW(1)
PPG_DEFINE_KERNELSW(2)
PPG_DEFINE_KERNELSW(4)
PPG_DEFINE_KERNELSW2(1)
PPG_DEFINE_KERNELSW2(2)
PPG_DEFINE_KERNELSW2(4)
PPG_DEFINE_KERNELSP(2)
PPG_DEFINE_KERNELSP(4)
PPG_DEFINE_KERNELSP2(2)
PPG_DEFINE_KERNELSP2(4)

typedef void (*ppg_kernel_fn)(const ppg::KParams);

static ppg_kernel_fn pick_kernel_gen2(int nq, int mode, bool fast) {
    static const ppg_kernel_fn table[2][3][5] = {
        {{ppg2_step_q1g, ppg2_reset_q1g, ppg2_observe_q1g, ppg2_grid_q1g, ppg2_step_ord_q1g},
         {ppg2_step_q2g, ppg2_reset_q2g, ppg2_observe_q2g, ppg2_grid_q2g, ppg2_step_ord_q2g},
         {ppg2_step_q4g, ppg2_reset_q4g, ppg2_observe_q4g, ppg2_grid_q4g, ppg2_step_ord_q4g}},
        {{ppg2_step_q1, ppg2_reset_q1, ppg2_observe_q1, ppg2_grid_q1, ppg2_step_ord_q1},
         {ppg2_step_q2, ppg2_reset_q2, ppg2_observe_q2, ppg2_grid_q2, ppg2_step_ord_q2},
         {ppg2_step_q4, ppg2_reset_q4, ppg2_observe_q4, ppg2_grid_q4, ppg2_step_ord_q4}},
    };
    return table[fast ? 1 : 0][nq == 1 ? 0 : nq == 2 ? 1 : 2][mode];
}

static ppg_kernel_fn pick_kernel_walls(int nq, int mode) {
    if (mode == ppg::MODE_VIS) return nq == 1 ? ppg3_vis_q1 : nq == 2 ? ppg3_vis_q2 : ppg3_vis_q4;
    static const ppg_kernel_fn table[3][5] = {
        {ppg3_step_q1, ppg3_reset_q1, ppg3_observe_q1, ppg3_grid_q1, ppg3_step_ord_q1},
        {ppg3_step_q2, ppg3_reset_q2, ppg3_observe_q2, ppg3_grid_q2, ppg3_step_ord_q2},
        {ppg3_step_q4, ppg3_reset_q4, ppg3_observe_q4, ppg3_grid_q4, ppg3_step_ord_q4},
    };
    return table[nq == 1 ? 0 : nq == 2 ? 1 : 2][mode];
}

static ppg_kernel_fn pick_kernel_drive(int nq, int mode) {
    static const ppg_kernel_fn table[3][5] = {
        {ppg4_step_q1, ppg4_reset_q1, ppg4_observe_q1, ppg4_grid_q1, ppg4_step_ord_q1},
        {ppg4_step_q2, ppg4_reset_q2, ppg4_observe_q2, ppg4_grid_q2, ppg4_step_ord_q2},
        {ppg4_step_q4, ppg4_reset_q4, ppg4_observe_q4, ppg4_grid_q4, ppg4_step_ord_q4},
    };
    return table[nq == 1 ? 0 : nq == 2 ? 1 : 2][mode];
}

static ppg_kernel_fn pick_kernel(int nq, int mode, bool fast) {
    static const ppg_kernel_fn table[2][3][ppg::N_MODES] = {
        {{ppg_step_q1g, ppg_reset_q1g, ppg_observe_q1g, ppg_grid_q1g, ppg_step_ord_q1g, ppg_rollout_q1g, ppg_step_kick_q1g, ppg_step_ord_kick_q1g},
         {ppg_step_q2g, ppg_reset_q2g, ppg_observe_q2g, ppg_grid_q2g, ppg_step_ord_q2g, ppg_rollout_q2g, ppg_step_kick_q2g, ppg_step_ord_kick_q2g},
         {ppg_step_q4g, ppg_reset_q4g, ppg_observe_q4g, ppg_grid_q4g, ppg_step_ord_q4g, ppg_rollout_q4g, ppg_step_kick_q4g, ppg_step_ord_kick_q4g}},
        {{ppg_step_q1, ppg_reset_q1, ppg_observe_q1, ppg_grid_q1, ppg_step_ord_q1, ppg_rollout_q1, ppg_step_kick_q1, ppg_step_ord_kick_q1},
         {ppg_step_q2, ppg_reset_q2, ppg_observe_q2, ppg_grid_q2, ppg_step_ord_q2, ppg_rollout_q2, ppg_step_kick_q2, ppg_step_ord_kick_q2},
         {ppg_step_q4, ppg_reset_q4, ppg_observe_q4, ppg_grid_q4, ppg_step_ord_q4, ppg_rollout_q4, ppg_step_kick_q4, ppg_step_ord_kick_q4}},
    };
    return table[fast ? 1 : 0][nq == 1 ? 0 : nq == 2 ? 1 : 2][mode];
}

// 128 predator rows (ppg_kernel_list.h: PPG_DEFINE_KERNELSP / SP2): one wave per env, generic observation geometry, nq 2 or 4
static ppg_kernel_fn pick_kernel_p2(bool gen2, int nq, int mode) {
    static const ppg_kernel_fn base[2][ppg::N_MODES] = {
        {ppg_step_p2q2g, ppg_reset_p2q2g, ppg_observe_p2q2g, ppg_grid_p2q2g, ppg_step_ord_p2q2g, ppg_rollout_p2q2g, ppg_step_kick_p2q2g,
         ppg_step_ord_kick_p2q2g},
        {ppg_step_p2q4g, ppg_reset_p2q4g, ppg_observe_p2q4g, ppg_grid_p2q4g, ppg_step_ord_p2q4g, ppg_rollout_p2q4g, ppg_step_kick_p2q4g,
         ppg_step_ord_kick_p2q4g}};
    static const ppg_kernel_fn second[2][5] = {
        {ppg2_step_p2q2g, ppg2_reset_p2q2g, ppg2_observe_p2q2g, ppg2_grid_p2q2g, ppg2_step_ord_p2q2g},
        {ppg2_step_p2q4g, ppg2_reset_p2q4g, ppg2_observe_p2q4g, ppg2_grid_p2q4g, ppg2_step_ord_p2q4g}};
    return gen2 ? second[nq == 2 ? 0 : 1][mode] : base[nq == 2 ? 0 : 1][mode];
}

#define PPG_HIP_TRY(h, call)                                                                   \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return ppg_fail(h, PPG_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// make the handle's device the calling thread's current one
static int backend_use_device(ppg_handle *h) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != h->device) PPG_HIP_TRY(h, hipSetDevice(h->device));
    return PPG_OK;
}

static int backend_init(ppg_handle *h, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ppg_fail(h, PPG_ENODEV, "no HIP device visible");
    if (device < 0 || device >= n) return ppg_fail(h, PPG_ENODEV, "device %d not in 0..%d", device, n - 1);
    hipDeviceProp_t prop;
    PPG_HIP_TRY(h, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ppg_fail(h, PPG_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    PPG_HIP_TRY(h, hipSetDevice(device));
    PPG_HIP_TRY(h, hipMalloc((void **)&h->lut_dev, h->lut_host.size() * sizeof(uint32_t)));
    PPG_HIP_TRY(h, hipMemcpy(h->lut_dev, h->lut_host.data(), h->lut_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (h->coop_ok) {
        PPG_HIP_TRY(h, hipMalloc((void **)&h->coop_tab_dev, h->coop_tab_host.size() * sizeof(uint32_t)));
        PPG_HIP_TRY(h, hipMemcpy(h->coop_tab_dev, h->coop_tab_host.data(), h->coop_tab_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return PPG_OK;
}

static int backend_alloc(ppg_handle *h, void **out, size_t bytes) {
    if (int rc = backend_use_device(h)) return rc;
    PPG_HIP_TRY(h, hipMalloc(out, bytes));
    return PPG_OK;
}

static void backend_release(ppg_handle *h) {
    if (h->vis_dev) (void)hipFree(h->vis_dev);
    h->vis_dev = nullptr;
    if (h->lut_dev) (void)hipFree(h->lut_dev);
    h->lut_dev = nullptr;
    if (h->coop_tab_dev) (void)hipFree(h->coop_tab_dev);
    h->coop_tab_dev = nullptr;
    if (h->order_dev) (void)hipFree(h->order_dev);
    h->order_dev = nullptr;
    if (h->fetch_dev) (void)hipFree(h->fetch_dev);
    h->fetch_dev = nullptr;
    h->fetch_cap = 0;
}

static void backend_free(ppg_handle *, void *p) { (void)hipFree(p); }

// order[] = the envs sorted by descending key (rows weighted by observation size): a counting sort in ONE workgroup, O(B) for any
// batch size.  Keys are small (<= 64 * 8 + 256 * 8), so the histogram lives in LDS; envs with equal keys land in arbitrary order
// (atomics) -- the order only decides which workgroup steps which env, never a result.
#define PPG_RANK_BINS 2568
// resident != NULL: also *resident = the largest count of leading envs (env-index order) whose observation bytes, n_pred_rows * bytes_p
// + n_prey_rows * bytes_q each, fit `share` (KParams::resident_envs; ppg_rebalance) -- a block-wide scan over contiguous runs of envs.
extern "C" __global__ void __launch_bounds__(1024) ppg_rank_envs(const int32_t *env_state, int batch, int wp, int wq, int32_t *order,
                                                                 int32_t *resident, long long share, int bytes_p, int bytes_q) {
    __shared__ int32_t hist[PPG_RANK_BINS];
    __shared__ long long run_sum[1024];
    __shared__ int32_t n_fit;
    const int t = (int)threadIdx.x;
    for (int k = t; k < PPG_RANK_BINS; k += 1024) hist[k] = 0;
    __syncthreads();
    for (int i = t; i < batch; i += 1024) {
        int key = env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PRED_ROWS] * wp + env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PREY_ROWS] * wq;
        key = key < 0 ? 0 : (key >= PPG_RANK_BINS ? PPG_RANK_BINS - 1 : key);
        atomicAdd(&hist[key], 1);
    }
    __syncthreads();
    if (t < 64) {   // exclusive prefix over the bins in DESCENDING key order: one wavefront, 41 bins per lane
        const int per = (PPG_RANK_BINS + 63) / 64;
        const int hi = PPG_RANK_BINS - 1 - t * per;          // this lane's bins: hi, hi-1, ..., hi-per+1
        int sum = 0;
        for (int q = 0; q < per; ++q) if (hi - q >= 0) sum += hist[hi - q];
        int before = 0;
        for (int l = 0; l < 64; ++l) { const int v = __shfl(sum, l, 64); if (l < t) before += v; }
        for (int q = 0; q < per; ++q) if (hi - q >= 0) { const int c = hist[hi - q]; hist[hi - q] = before; before += c; }
    }
    __syncthreads();
    for (int i = t; i < batch; i += 1024) {
        int key = env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PRED_ROWS] * wp + env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PREY_ROWS] * wq;
        key = key < 0 ? 0 : (key >= PPG_RANK_BINS ? PPG_RANK_BINS - 1 : key);
        order[atomicAdd(&hist[key], 1)] = i;
    }
    if (!resident) return;   // (uniform: a kernel argument)
    const int per = (batch + 1023) / 1024, lo = t * per, hi = lo + per < batch ? lo + per : batch;   // this thread's run of envs
    auto env_bytes = [&](int i) {
        const int np = env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PRED_ROWS], nq = env_state[(size_t)i * PPG_ENV_WORDS + PPG_ENV_N_PREY_ROWS];
        return (long long)(np > 0 ? np : 0) * bytes_p + (long long)(nq > 0 ? nq : 0) * bytes_q;
    };
    long long mine = 0;
    for (int i = lo; i < hi; ++i) mine += env_bytes(i);
    run_sum[t] = mine;
    if (t == 0) n_fit = 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan of the 1024 run sums
        const long long add = t >= d ? run_sum[t - d] : 0;
        __syncthreads();
        run_sum[t] += add;
        __syncthreads();
    }
    long long acc = run_sum[t] - mine;   // bytes of the envs in front of this run
    int fit = 0;
    for (int i = lo; i < hi; ++i) { acc += env_bytes(i); fit += acc <= share; }   // (sums never decrease: the envs that fit are a prefix)
    if (fit) atomicAdd(&n_fit, fit);
    __syncthreads();
    if (t == 0) *resident = n_fit;
}

static int backend_rebalance(ppg_handle *h, int weight_pred, int weight_prey, void *stream) {
    if (int rc = backend_use_device(h)) return rc;
    if (!h->order_dev) PPG_HIP_TRY(h, hipMalloc((void **)&h->order_dev, (size_t)h->batch * sizeof(int32_t)));
    hipLaunchKernelGGL(ppg_rank_envs, dim3(1), dim3(1024), 0, (hipStream_t)stream,
                       (const int32_t *)h->bufs.env_state, (int)h->batch, weight_pred, weight_prey, h->order_dev,
                       h->resident_share >= 0 ? h->resident_dev : (int32_t *)nullptr, (long long)h->resident_share,
                       (int)h->resident_row_bytes[0], (int)h->resident_row_bytes[1]);
    PPG_HIP_TRY(h, hipGetLastError());
    return PPG_OK;
}

// ---- the learner-side kernels: one wavefront per workgroup, the parameter block by value ----------------------------------------
// ppg_pack / ppg_fetch / ppg_link / ppg_record / ppg_record_obs / ppg_record_logp / ppg_backward / ppg_backward_samples / ppg_ppo_loss
// (the four-wave kernels of ppg_net_forward / ppg_net_backward stand further down) (ppg_pack.h, ppg_fetch.h, ppg_link.h, ppg_record.h, ppg_obs_store.h, ppg_logp.h, ppg_backward.h, ppg_ppo.h)
#define PPG_ROWS_KERNEL(name, Params, main, lds_bytes)                                         \
    extern "C" __global__ void __launch_bounds__(64) name(const ppg::Params K) {              \
        __shared__ __attribute__((aligned(16))) unsigned char lds[lds_bytes];                  \
        ppg::main(*PPG_KERNARG_PTR(ppg::Params, K), lds);                                      \
    }
#define PPG_ROWS_KERNEL_NO_LDS(name, Params, main)                                             \
    extern "C" __global__ void __launch_bounds__(64) name(const ppg::Params K) { ppg::main(*PPG_KERNARG_PTR(ppg::Params, K)); }
PPG_ROWS_KERNEL(ppg_pack_scan, PackParams, pack_scan_main, ppg::ROWS_SCAN_LDS_BYTES)
PPG_ROWS_KERNEL_NO_LDS(ppg_pack_rows, PackParams, pack_rows_main)
PPG_ROWS_KERNEL(ppg_fetch_rows, FetchParams, fetch_main, 1024)
PPG_ROWS_KERNEL(ppg_link_rows, LinkParams, link_main, ppg::LINK_LDS_BYTES)
PPG_ROWS_KERNEL(ppg_record_rows, RecordParams, record_main, ppg::LINK_LDS_BYTES)
PPG_ROWS_KERNEL(ppg_obs_scan, ObsStoreParams, obs_scan_main, ppg::ROWS_SCAN_LDS_BYTES)
PPG_ROWS_KERNEL_NO_LDS(ppg_obs_rows, ObsStoreParams, obs_rows_main)
PPG_ROWS_KERNEL(ppg_logp_scan, LogpParams, logp_scan_main, ppg::ROWS_SCAN_LDS_BYTES)
PPG_ROWS_KERNEL_NO_LDS(ppg_logp_rows, LogpParams, logp_rows_main)
PPG_ROWS_KERNEL(ppg_backward_rows, BackwardParams, backward_main, ppg::BACKWARD_LDS_BYTES)
PPG_ROWS_KERNEL(ppg_backward_samples_rows, BackwardSamplesParams, backward_samples_main, ppg::BACKWARD_LDS_BYTES)
PPG_ROWS_KERNEL_NO_LDS(ppg_ppo_count, PpoParams, ppo_count_main)
PPG_ROWS_KERNEL(ppg_ppo_rows, PpoParams, ppo_rows_main, ppg::PPO_LDS_BYTES)

// `grid` one-wave workgroups of `kernel` on `stream`
template <class Params>
static int backend_launch_rows(ppg_handle *h, void (*kernel)(const Params), int grid, const Params &K, void *stream) {
    if (int rc = backend_use_device(h)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, K);
    PPG_HIP_TRY(h, hipGetLastError());
    return PPG_OK;
}

static int backend_pack(ppg_handle *h, const ppg::PackParams &K, void *stream) {
    if (int rc = backend_launch_rows(h, ppg_pack_scan, 1, K, stream)) return rc;
    return backend_launch_rows(h, ppg_pack_rows, K.n_envs, K, stream);
}
static int backend_fetch(ppg_handle *h, const ppg::FetchParams &K, void *stream) { return backend_launch_rows(h, ppg_fetch_rows, K.n_envs, K, stream); }
static int backend_link(ppg_handle *h, const ppg::LinkParams &K, void *stream) { return backend_launch_rows(h, ppg_link_rows, K.batch, K, stream); }
static int backend_record(ppg_handle *h, const ppg::RecordParams &K, void *stream) { return backend_launch_rows(h, ppg_record_rows, K.batch, K, stream); }
static int backend_record_obs(ppg_handle *h, const ppg::ObsStoreParams &K, void *stream) {
    if (int rc = backend_launch_rows(h, ppg_obs_scan, 1, K, stream)) return rc;
    return backend_launch_rows(h, ppg_obs_rows, K.batch, K, stream);
}
static int backend_record_logp(ppg_handle *h, const ppg::LogpParams &K, void *stream) {
    if (int rc = backend_launch_rows(h, ppg_logp_scan, 1, K, stream)) return rc;
    return backend_launch_rows(h, ppg_logp_rows, K.batch, K, stream);
}
static int backend_backward(ppg_handle *h, const ppg::BackwardParams &K, void *stream) { return backend_launch_rows(h, ppg_backward_rows, K.batch, K, stream); }
static int backend_backward_samples(ppg_handle *h, const ppg::BackwardSamplesParams &K, void *stream) {
    return backend_launch_rows(h, ppg_backward_samples_rows, K.batch, K, stream);
}
static int backend_ppo_loss(ppg_handle *h, const ppg::PpoParams &K, void *stream) {
    if (int rc = backend_launch_rows(h, ppg_ppo_count, K.G, K, stream)) return rc;
    return backend_launch_rows(h, ppg_ppo_rows, K.G, K, stream);
}


// ---- ppg_net_forward / ppg_net_backward (ppg_net.h): four-wave workgroups, dynamic LDS (two activation buffers of a tile) ------------
extern "C" __global__ void __launch_bounds__(ppg::NET_THREADS) ppg_net_fwd(const ppg::NetParams K) {
    PPG_DYNAMIC_LDS(lds);
    ppg::net_forward_main(*PPG_KERNARG_PTR(ppg::NetParams, K), lds);
}
extern "C" __global__ void __launch_bounds__(ppg::NET_THREADS) ppg_net_bwd(const ppg::NetParams K) {
    PPG_DYNAMIC_LDS(lds);
    ppg::net_backward_main(*PPG_KERNARG_PTR(ppg::NetParams, K), lds);
}
extern "C" __global__ void __launch_bounds__(ppg::NET_THREADS) ppg_net_reduce(const ppg::NetParams K) {
    ppg::net_reduce_main(*PPG_KERNARG_PTR(ppg::NetParams, K));
}

// which: 0 forward, 1 backward, 2 reduce.  More than 64 KB of dynamic LDS has to be allowed per kernel and device: done the first time a
// launch needs more than was allowed so far (a host call, remembered here), never again for that size -- a warmed launch only launches.
static int backend_net_launch(ppg_handle *h, int which, int grid, const ppg::NetParams &K, int lds_bytes, void *stream) {
    static void (*const kernels[3])(const ppg::NetParams) = {ppg_net_fwd, ppg_net_bwd, ppg_net_reduce};
    static int allowed[3][64];   // bytes allowed so far, per kernel and device (0: the default 64 KB)
    void (*kernel)(const ppg::NetParams) = kernels[which];
    if (int rc = backend_use_device(h)) return rc;
    int &have = allowed[which][h->device & 63];
    if (lds_bytes > 64 * 1024 && lds_bytes > have) {
        PPG_HIP_TRY(h, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        have = 160 * 1024;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(ppg::NET_THREADS), (size_t)lds_bytes, (hipStream_t)stream, K);
    PPG_HIP_TRY(h, hipGetLastError());
    return PPG_OK;
}
static int backend_net_forward(ppg_handle *h, const ppg::NetParams &K, int lds_bytes, void *stream) {
    return backend_net_launch(h, 0, K.G, K, lds_bytes, stream);
}
static int backend_net_backward(ppg_handle *h, const ppg::NetParams &K, int lds_bytes, void *stream) {
    if (int rc = backend_net_launch(h, 1, K.G, K, lds_bytes, stream)) return rc;
    return backend_net_launch(h, 2, (K.n_params + ppg::NET_THREADS - 1) / ppg::NET_THREADS, K, 0, stream);
}

static int backend_copy(ppg_handle *h, void *dst, const void *src, size_t bytes, bool to_device, void *stream) {
    if (int rc = backend_use_device(h)) return rc;
    PPG_HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, (hipStream_t)stream));
    return PPG_OK;
}

static int backend_sync(ppg_handle *h, void *stream) {
    PPG_HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    return PPG_OK;
}

static int backend_launch(ppg_handle *h, int mode, const ppg::KParams &P, void *stream) {
    // one workgroup = one wavefront = one environment
    if (int rc = backend_use_device(h)) return rc;
    const bool fast = P.nch_p <= 2 && P.nch_q <= 3;
    if (h->gen2 && mode > ppg::MODE_STEP_ORDERED && !(mode == ppg::MODE_VIS && h->cfg2.walls) &&
        !(mode == ppg::MODE_ROLLOUT && !h->cfg2.walls && P.coop_e > 0))
        return ppg_fail(h, PPG_EINVAL, "mode %d is not available for second-generation handles", mode);
    if (h->drive && mode > ppg::MODE_STEP_ORDERED) return ppg_fail(h, PPG_EINVAL, "mode %d is not available for the drive-conditioned variant", mode);
    ppg_kernel_fn fn = h->drive ? pick_kernel_drive(h->nq, mode) : !h->gen2 ? pick_kernel(h->nq, mode, fast)
                       : h->cfg2.walls ? pick_kernel_walls(h->nq, mode) : pick_kernel_gen2(h->nq, mode, fast);
    if (P.cap_pred > 64) {   // (ppg_validate_and_layout admits 128 predator rows for these forms only; ppg_wave_plan keeps them one-wave)
        if (h->drive || (h->gen2 && h->cfg2.walls) || h->nq < 2 || P.coop_e > 0 || h->plan.nw != 1)
            return ppg_fail(h, PPG_EINVAL, "no kernel for 128 predator rows with this configuration");
        fn = pick_kernel_p2(h->gen2 != 0, h->nq, mode);
    }
    unsigned block = 64, grid = (unsigned)h->batch;
    const ppg_wave_plan_t wp = h->plan;
    if ((mode == ppg::MODE_STEP || mode == ppg::MODE_ROLLOUT) && P.coop_e > 0) {   // cooperative kernels: coop_e envs per workgroup of wp.nw wavefronts
        static const ppg_kernel_fn c[4][2] = {{ppgc_step_q1, ppgc_step_q2}, {ppgc8_step_q1, ppgc8_step_q2}, {ppgc16_step_q1, ppgc16_step_q2},
                                              {ppgc6_step_q1, ppgc6_step_q2}};
        fn = c[wp.nw == 8 ? 1 : wp.nw == 16 ? 2 : wp.nw == 6 ? 3 : 0][h->nq == 1 ? 0 : 1];
        if (!h->gen2 && wp.nw == 4 && P.obs_f32 == 2 && ppg_coop_high_occupancy(h, wp.coop_e))   // bfloat16 rows: the 64-register build, 8 workgroups per CU
            fn = h->nq == 1 ? ppgch_step_q1 : ppgch_step_q2;
        if (h->gen2) fn = h->nq == 1 ? ppgc2_step_q1 : ppgc2_step_q2;   // (second generation: four-wave cooperative kernels)
        if (!P.ch0_map)   // three cell maps per env (ppg_planned_step_params chose that layout: four-wave step launches only)
            fn = h->gen2 ? (h->nq == 1 ? ppgcm2_step_q1 : ppgcm2_step_q2) : (h->nq == 1 ? ppgcm_step_q1 : ppgcm_step_q2);
        if (h->gen2 && h->cfg2.walls) fn = h->nq == 1 ? ppgc3_step_q1 : ppgc3_step_q2;   // (walls: three maps, rows written whole)
        if (mode == ppg::MODE_ROLLOUT)   // (ppg_rollout: the fused form of the four-wave cooperative kernels)
            fn = h->gen2 ? (h->nq == 1 ? ppgc2_rollout_q1 : ppgc2_rollout_q2) : (h->nq == 1 ? ppgc_rollout_q1 : ppgc_rollout_q2);
        block = 64u * (unsigned)wp.nw;
        grid = (unsigned)((h->batch + P.coop_e - 1) / P.coop_e);
        if (P.lds_bytes > 64 * 1024)
            PPG_HIP_TRY(h, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, P.lds_bytes));
    } else if (mode == ppg::MODE_STEP && wp.nw > 1) {   // several waves per env: wave 0 steps, all of them write the final observations
        const int qi = h->nq == 1 ? 0 : h->nq == 2 ? 1 : 2;
        if (h->drive) {
            static const ppg_kernel_fn w4[2][3] = {{ppgw4_step_q1, ppgw4_step_q2, ppgw4_step_q4}, {ppgwp4_step_q1, ppgwp4_step_q2, ppgwp4_step_q4}};
            fn = w4[wp.nw == 2 ? 1 : 0][qi];
        } else if (h->gen2 && h->cfg2.walls) {
            static const ppg_kernel_fn w3[2][3] = {{ppgw3_step_q1, ppgw3_step_q2, ppgw3_step_q4}, {ppgwp3_step_q1, ppgwp3_step_q2, ppgwp3_step_q4}};
            fn = w3[wp.nw == 2 ? 1 : 0][qi];
        } else if (wp.nw == 16) {
            static const ppg_kernel_fn w16[3] = {ppgw16_step_q1, ppgw16_step_q2, ppgw16_step_q4};
            fn = w16[qi];
        } else if (wp.nw == 2) {
            static const ppg_kernel_fn wpair[2][3] = {{ppgwp_step_q1g, ppgwp_step_q2g, ppgwp_step_q4g}, {ppgwp_step_q1, ppgwp_step_q2, ppgwp_step_q4}};
            fn = wpair[fast ? 1 : 0][qi];
        } else {
            static const ppg_kernel_fn w[2][2][2][3] = {
                {{{ppgw_step_q1g, ppgw_step_q2g, ppgw_step_q4g}, {ppgw_step_q1, ppgw_step_q2, ppgw_step_q4}},
                 {{ppgw2_step_q1g, ppgw2_step_q2g, ppgw2_step_q4g}, {ppgw2_step_q1, ppgw2_step_q2, ppgw2_step_q4}}},
                {{{ppgw8_step_q1g, ppgw8_step_q2g, ppgw8_step_q4g}, {ppgw8_step_q1, ppgw8_step_q2, ppgw8_step_q4}},
                 {{ppgw28_step_q1g, ppgw28_step_q2g, ppgw28_step_q4g}, {ppgw28_step_q1, ppgw28_step_q2, ppgw28_step_q4}}}};
            fn = w[wp.nw == 8 ? 1 : 0][h->gen2 ? 1 : 0][fast ? 1 : 0][qi];
        }
        block = 64u * (unsigned)wp.nw;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(block), (size_t)P.lds_bytes, (hipStream_t)stream, P);
    PPG_HIP_TRY(h, hipGetLastError());
    return PPG_OK;
}

// device buffers on physical pages spread over device memory (observation tensors; the policy kernels' scratch slots)
#include "ppg_spread.h"

// policy inference next to the env (MFMA kernels + their host side)
#include "ppg_policy.h"
#include "ppg_policy_host.h"
