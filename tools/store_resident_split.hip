// Calibration program (not product code): can a FIXED set of envs keep the 256 MiB Infinity Cache to itself across per-step launches
// if the other envs' observation stores are non-temporal?  The cooperative LAUNCH STRUCTURE of the headline step with no compute
// (store_patterns5's `slab` mode): two envs per four-wave workgroup, 1 KB pieces of 16 bytes per lane, float64 slabs [B, 64, 196]
// (predator rows) and [B, 128, 324] (prey rows), the benchmark's spread of row counts (about 94 KB per env, 386 MB per 4096-env
// step), three sub-batches on three streams, a transition-length delay in front of the stores.
//   ./a.out [B=4096] [steps=200] [rounds=5] [delay_us=21] [draws=1]
// variants, all in one process on the same buffers, interleaved round by round, timed with HIP events on the launch streams:
//   plain       every store as the step kernels do today
//   nt          every store through __builtin_nontemporal_store on the 16-byte vector
//   split X     the first M envs of every sub-batch plain, the others nt; M = the largest count of leading envs whose bytes stay
//               within X MiB * batch / envs in flight (so the three sub-batches share one budget of X MiB); always the same envs
//   only X      the plain envs of `split X` written and nothing else (that part with the cache to itself: the most split X can save)
//   splitsc X   split X with `global_store_dwordx4 ... sc0 sc1` in place of nt for the streamed part
// Output: one table, us per full step per variant (median and range over the rounds), and the go / stop line of the decision rule:
// go if the best split's median is below plain's by more than plain's range over its rounds.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef double d2 __attribute__((ext_vector_type(2)));
enum { PLAIN = 0, NT = 1, SC01 = 2, SKIP = 3 };

__device__ __forceinline__ void st16(double *p, double a, double b, int flavour) {   // (flavour is wave-uniform)
    d2 v; v.x = a; v.y = b;
    if (flavour == PLAIN) *(d2 *)p = v;
    else if (flavour == NT) __builtin_nontemporal_store(v, (d2 *)p);
    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}

// rows: [B][2] = predator rows, prey rows in use of each env.  Envs below M are written with flavour lo, the others with hi.
__global__ void __launch_bounds__(256) step_like(double *obs_p, double *obs_q, const int *rows, int B, int M, int lo, int hi,
                                                 int delay_ticks, int spread_ticks) {
    constexpr int E = 2, NW = 4, CAP_P = 64, BLK_P = 196, CAP_Q = 128, BLK_Q = 324;
    const int ln = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.x * E;
    if (w < E && b0 + w < B) {   // "transition": idle; its length grows with the env's rows like the real one
        const int n = rows[2 * (b0 + w)] + rows[2 * (b0 + w) + 1];
        const long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
        const long long want = delay_ticks + (long long)spread_ticks * n / 41;
        while (__builtin_amdgcn_s_memrealtime() - t0 < want) __builtin_amdgcn_s_sleep(32);
    }
    __syncthreads();
    int at = 0;
    for (int k = 0; k < E; ++k) {
        const int b = b0 + k;
        if (b >= B) break;
        const int flavour = b < M ? lo : hi;
        if (flavour == SKIP) continue;
        for (int part = 0; part < 2; ++part) {
            const int tot = rows[2 * b + part] * (part ? BLK_Q : BLK_P);   // (even, and at most cap * blk: inside the env's slab)
            double *base = part ? obs_q + (size_t)b * CAP_Q * BLK_Q : obs_p + (size_t)b * CAP_P * BLK_P;
            int first = w - at; if (first < 0) first += NW;
            for (int e = first * 128 + 2 * ln; e < tot; e += NW * 128) st16(base + e, (double)e, 1.0, flavour);
            at = (at + (tot + 127) / 128) % NW;
        }
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Variant { std::string name; int x_mib, lo, hi; std::vector<float> us; int m_total = 0; double plain_mb = 0, written_mb = 0; };

int main(int argc, char **argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 4096, steps = argc > 2 ? atoi(argv[2]) : 200, rounds = argc > 3 ? atoi(argv[3]) : 5;
    const double delay_us = argc > 4 ? atof(argv[4]) : 21.0;
    const int draws = argc > 5 ? atoi(argv[5]) : 1;
    constexpr int S = 3, E = 2, CAP_P = 64, BLK_P = 196, CAP_Q = 128, BLK_Q = 324;
    if (B < S || steps < 1 || rounds < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    printf("device %s, %d envs, %d sub-batches, %d steps x %d rounds per variant, delay %.1f us\n", prop.name, B, S, steps, rounds, delay_us);

    // the benchmark's spread: 4..20 predator rows (mean 12) and 10..48 prey rows (mean 29) -> (12 * 196 + 29 * 324) * 8 = 94 KB per env
    std::vector<int> h(2 * (size_t)B);
    std::vector<size_t> env_bytes(B);
    unsigned s = 12345; size_t total_bytes = 0;
    for (int i = 0; i < B; ++i) {
        s = s * 1664525u + 1013904223u; h[2 * i] = 4 + (int)((s >> 8) % 17u);
        s = s * 1664525u + 1013904223u; h[2 * i + 1] = 10 + (int)((s >> 8) % 39u);
        env_bytes[i] = ((size_t)h[2 * i] * BLK_P + (size_t)h[2 * i + 1] * BLK_Q) * sizeof(double);
        total_bytes += env_bytes[i];
    }
    printf("one step writes %.1f MB (%.1f KB per env)\n", total_bytes / 1e6, total_bytes / 1e3 / B);
    int sub_lo[S + 1];
    for (int k = 0; k <= S; ++k) sub_lo[k] = (int)((long long)B * k / S);

    std::vector<Variant> vars;
    vars.push_back({"plain", -1, PLAIN, PLAIN});
    vars.push_back({"nt", 0, PLAIN, NT});
    const int xs[5] = {96, 128, 160, 192, 224};
    for (int x : xs) vars.push_back({"split " + std::to_string(x), x, PLAIN, NT});
    for (int x : xs) vars.push_back({"only " + std::to_string(x), x, PLAIN, SKIP});
    for (int x : xs) vars.push_back({"splitsc " + std::to_string(x), x, PLAIN, SC01});
    // M of every variant and sub-batch: the largest count of leading envs whose bytes fit x MiB * batch / envs in flight
    std::vector<std::vector<int>> m_of(vars.size(), std::vector<int>(S));
    for (size_t v = 0; v < vars.size(); ++v)
        for (int k = 0; k < S; ++k) {
            const int nb = sub_lo[k + 1] - sub_lo[k];
            int m = nb;
            if (vars[v].x_mib >= 0) {
                const size_t share = (size_t)((double)vars[v].x_mib * 1048576.0 * nb / B);
                size_t acc = 0; m = 0;
                while (m < nb && acc + env_bytes[sub_lo[k] + m] <= share) acc += env_bytes[sub_lo[k] + m++];
            }
            m_of[v][k] = m;
            vars[v].m_total += m;
            for (int i = 0; i < nb; ++i) {
                const int fl = i < m ? vars[v].lo : vars[v].hi;
                if (fl == PLAIN) vars[v].plain_mb += env_bytes[sub_lo[k] + i] / 1e6;
                if (fl != SKIP) vars[v].written_mb += env_bytes[sub_lo[k] + i] / 1e6;
            }
        }

    int *rows; CK(hipMalloc(&rows, h.size() * sizeof(int)));
    CK(hipMemcpy(rows, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
    hipStream_t st[S]; hipEvent_t ev0, ev1, done[S];
    for (int k = 0; k < S; ++k) { CK(hipStreamCreate(&st[k])); CK(hipEventCreateWithFlags(&done[k], hipEventDisableTiming)); }
    CK(hipEventCreate(&ev0)); CK(hipEventCreate(&ev1));
    const int ticks = (int)(delay_us * 100 * 0.6), spread = (int)(delay_us * 100 * 0.4);

    for (int draw = 0; draw < draws; ++draw) {
        double *obs_p, *obs_q;   // (a fresh pair of allocations per draw, not freed: the next draw gets other pages)
        CK(hipMalloc(&obs_p, (size_t)B * CAP_P * BLK_P * sizeof(double)));
        CK(hipMalloc(&obs_q, (size_t)B * CAP_Q * BLK_Q * sizeof(double)));
        for (auto &v : vars) v.us.clear();
        auto launch_all = [&](size_t v) {
            for (int k = 0; k < S; ++k) {
                const int lo = sub_lo[k], nb = sub_lo[k + 1] - lo;
                hipLaunchKernelGGL(step_like, dim3((nb + E - 1) / E), dim3(256), 0, st[k], obs_p + (size_t)lo * CAP_P * BLK_P,
                                   obs_q + (size_t)lo * CAP_Q * BLK_Q, rows + 2 * lo, nb, m_of[v][k], vars[v].lo, vars[v].hi, ticks, spread);
            }
        };
        for (int r = 0; r < rounds; ++r)
            for (size_t v = 0; v < vars.size(); ++v) {
                for (int i = 0; i < 20; ++i) launch_all(v);   // warm-up: also what makes the variant's plain part resident
                CK(hipDeviceSynchronize());
                // the window opens on stream 0, the other streams start behind it, and it closes when all three are done
                CK(hipEventRecord(ev0, st[0]));
                for (int k = 1; k < S; ++k) CK(hipStreamWaitEvent(st[k], ev0, 0));
                for (int i = 0; i < steps; ++i) launch_all(v);
                for (int k = 1; k < S; ++k) { CK(hipEventRecord(done[k], st[k])); CK(hipStreamWaitEvent(st[0], done[k], 0)); }
                CK(hipEventRecord(ev1, st[0]));
                CK(hipEventSynchronize(ev1));
                CK(hipGetLastError());
                float ms = 0; CK(hipEventElapsedTime(&ms, ev0, ev1));
                vars[v].us.push_back(ms / steps * 1e3f);
            }
        printf("\ndraw %d: us per full step (3 launches), median [min .. max] over %d rounds; TB/s = bytes written / median\n", draw, rounds);
        printf("%-12s %6s %9s %9s %8s %8s %8s %6s   rounds\n", "variant", "M", "plain MB", "all MB", "median", "min", "max", "TB/s");
        float plain_med = 0, plain_range = 0, best = 1e30f; std::string best_name;
        for (auto &v : vars) {
            std::vector<float> t = v.us; std::sort(t.begin(), t.end());
            const float med = t[t.size() / 2];
            printf("%-12s %6d %9.1f %9.1f %8.2f %8.2f %8.2f %6.2f  ", v.name.c_str(), v.m_total, v.plain_mb, v.written_mb, med, t.front(), t.back(),
                   v.written_mb * 1e6 / (med * 1e-6) / 1e12);
            for (float u : v.us) printf(" %.2f", u);
            printf("\n");
            if (v.name == "plain") { plain_med = med; plain_range = t.back() - t.front(); }
            if (v.name.rfind("split ", 0) == 0 && med < best) { best = med; best_name = v.name; }
        }
        printf("draw %d decision: plain %.2f us (range %.2f), best split '%s' %.2f us: %s\n", draw, plain_med, plain_range, best_name.c_str(), best,
               plain_med - best > plain_range ? "GO" : "STOP");
        fflush(stdout);
    }
    return 0;
}
