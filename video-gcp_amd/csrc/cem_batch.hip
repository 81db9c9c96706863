// The per-iteration arithmetic of the flat CEM planner (planning.py: CEMPlanner.plan_batch) for K planning tasks at once: the population
// from unit noise, the elite pick and the refit of the K Gaussians (gcp/planning/cem/cem_planner.py:55-135, sampler.py:33-48).  One launch
// each over all tasks; nothing is read back between them.  Every result is defined as a fixed sequence of separately rounded float32
// operations, which the torch mirrors in planning.py repeat: the compiler may not contract a multiply and an add into an FMA in this
// file: it is built with -ffp-contract=off (csrc/sources.sh: GCPX_NO_CONTRACT; hipcc contracts by default, and the __fmul_rn / __fadd_rn
// intrinsics are plain operators to it).  `/` and sqrtf are the correctly rounded ones (hipcc's default for float32).
// Beside them what receding-horizon planning adds, which the reference's CEM does not have: the Gaussians a re-plan starts from
// (gcpx_cem_warm_start) and the population with carried elites and AR(1) noise along the steps (gcpx_cem_population_ex).
#include "common.h"

namespace {

constexpr int kPopCols = 1024;      // columns of one row a population workgroup covers: 4 per thread

// workgroup (row r = (k, j), chunk c): out[r][d] = clamp(mean[k][d] + std[k][d] * eps[r][d]) for the chunk's columns; out may be eps
__global__ void __launch_bounds__(256) cem_population_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                             const float* eps, const float clip, const int do_clip, float* out,
                                                             const int n, const int D, const int chunks) {
    const int r = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const int k = r / n;
    const float* m = mean + (size_t)k * D;
    const float* s = std_ + (size_t)k * D;
    const float* e = eps + (size_t)r * D;
    float* o = out + (size_t)r * D;
    const float lo = -clip;
#pragma unroll
    for (int u = 0; u < kPopCols / 256; ++u) {
        const int d = c * kPopCols + u * 256 + threadIdx.x;
        if (d >= D) break;
        float v = m[d] + s[d] * e[d];
        if (do_clip) {                                      // torch.clamp: min(max(v, -clip), clip); a NaN stays a NaN
            v = v < lo ? lo : v;
            v = v > clip ? clip : v;
        }
        o[d] = v;
    }
}

// ascending, order-preserving key of a score: -0.0 = +0.0, -inf < numbers < +inf < every NaN (all NaNs one key: among themselves by index)
__device__ __forceinline__ uint32_t score_key(const float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.f) return 0x80000000u;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// workgroup k: the keys of the task's n scores in LDS; the rank of score i in the stable ascending order is the number of j < i with
// key_j <= key_i plus the number of j > i with key_j < key_i (a permutation of 0 .. n-1: every output slot is written exactly once)
__global__ void __launch_bounds__(256) cem_elites_kernel(const float* __restrict__ scores, int32_t* __restrict__ idx,
                                                         float* __restrict__ elite_scores, const int n, const int n_elite) {
    __shared__ uint32_t keys[GCPX_CEM_MAX_N];
    const int k = blockIdx.x;
    const float* sc = scores + (size_t)k * n;
    for (int i = threadIdx.x; i < n; i += 256) keys[i] = score_key(sc[i]);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const uint32_t ki = keys[i];
        int rank = 0;
        for (int j = 0; j < i; ++j) rank += keys[j] <= ki;
        for (int j = i + 1; j < n; ++j) rank += keys[j] < ki;
        if (rank < n_elite) {
            idx[(size_t)k * n_elite + rank] = i;
            elite_scores[(size_t)k * n_elite + rank] = sc[i];
        }
    }
}

// thread (k, d): the task's elites in order, column d.  idx is only ever compared and, inside [0, n), multiplied into an address
__global__ void __launch_bounds__(256) cem_refit_kernel(const float* __restrict__ samples, const int32_t* __restrict__ idx,
                                                        float* __restrict__ mean, float* __restrict__ std_, float* __restrict__ best,
                                                        const int n, const int n_elite, const int D, const int blocks_d) {
    const int k = blockIdx.x / blocks_d;
    const int d = (blockIdx.x % blocks_d) * 256 + threadIdx.x;
    if (d >= D) return;
    const int32_t* e = idx + (size_t)k * n_elite;
    const float* x = samples + (size_t)k * n * D + d;
    const size_t o = (size_t)k * D + d;
    bool ok = true;
    for (int j = 0; j < n_elite; ++j) ok = ok && e[j] >= 0 && e[j] < n;
    if (!ok) {
        const float nan = __builtin_nanf("");
        mean[o] = nan; std_[o] = nan; best[o] = nan;
        return;
    }
    const float x0 = x[(size_t)e[0] * D];
    float acc = x0;
    for (int j = 1; j < n_elite; ++j) acc += x[(size_t)e[j] * D];
    const float cnt = (float)n_elite;
    const float mu = acc / cnt;
    float dv = x0 - mu;
    float sq = dv * dv;
    for (int j = 1; j < n_elite; ++j) {
        dv = x[(size_t)e[j] * D] - mu;
        sq = sq + dv * dv;
    }
    mean[o] = mu;
    std_[o] = sqrtf(sq / cnt);
    best[o] = x0;
}

// thread (k, d), d = t * A + a: the Gaussian a re-plan starts from.  Task k's previous plan moved up by s = shift[k] executed steps, a
// narrower std on the steps it covers, the cold start behind them (and everywhere for s < 0 or s >= S).  The one shifted load is made
// only where t + s < S, written as t < S - s (s >= 0 there: no overflow); prev of a task with s < 0 is never read.
__global__ void __launch_bounds__(256) cem_warm_start_kernel(const float* __restrict__ prev, const int32_t* __restrict__ shift,
                                                             const float init_std, const float warm, float* __restrict__ mean,
                                                             float* __restrict__ std_, const int S, const int A, const int blocks_d) {
    const int k = blockIdx.x / blocks_d;
    const int D = S * A;
    const int d = (blockIdx.x % blocks_d) * 256 + threadIdx.x;
    if (d >= D) return;
    const int s = shift[k];
    const size_t o = (size_t)k * D + d;
    if (s >= 0 && d / A < S - s) {
        mean[o] = prev[o + (size_t)s * A];
        std_[o] = warm;
    } else {
        mean[o] = 0.f;
        std_[o] = init_std;
    }
}

// thread (row r = (k, j), column group c): W columns a = c W .. c W + W - 1 of the row, walked along its S steps (the noise of a column is
// a chain over the steps).  Rows j < m are copies of rows of prev_pop, moved as 32-bit words; the others are the AR(1) noise turned into
// candidates with the expression of cem_population_kernel.  out may be eps: a thread reads an element before it writes it and touches
// no other thread's elements.
template <int W>
__global__ void __launch_bounds__(256) cem_population_ex_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                                const float* eps, const float clip, const int do_clip, const float rho,
                                                                const float c, const float* __restrict__ prev_pop,
                                                                const int32_t* __restrict__ prev_idx, const int m, const int n_prev,
                                                                float* out, const int n, const int S, const int A, const int G,
                                                                const int64_t threads) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= threads) return;
    const int64_t r = g / G;
    const int a0 = (int)(g % G) * W;
    const int k = (int)(r / n), j = (int)(r % n);
    const size_t D = (size_t)S * A;
    float* o = out + (size_t)r * D + a0;
    if (j < m) {                                            // idx is only ever compared and, inside [0, n_prev), multiplied into an address
        const int32_t* e = prev_idx + (size_t)k * m;
        bool ok = true;
        for (int i = 0; i < m; ++i) ok = ok && e[i] >= 0 && e[i] < n_prev;
        if (!ok) {
            const float nan = __builtin_nanf("");
            for (int t = 0; t < S; ++t)
#pragma unroll
                for (int w = 0; w < W; ++w) o[(size_t)t * A + w] = nan;
            return;
        }
        const uint32_t* src = reinterpret_cast<const uint32_t*>(prev_pop) + ((size_t)k * n_prev + e[j]) * D + a0;
        uint32_t* dst = reinterpret_cast<uint32_t*>(o);
        for (int t = 0; t < S; ++t)
#pragma unroll
            for (int w = 0; w < W; ++w) dst[(size_t)t * A + w] = src[(size_t)t * A + w];
        return;
    }
    const float* e = eps + (size_t)r * D + a0;
    const float* mu = mean + (size_t)k * D + a0;
    const float* sd = std_ + (size_t)k * D + a0;
    const float lo = -clip;
    const bool corr = rho != 0.f;                           // rho = 0: the noise is eps itself, not 0 * xi + 1 * eps (a NaN or Inf in eps
    float xi[W];                                            // stays in its own step)
    for (int t = 0; t < S; ++t) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const size_t i = (size_t)t * A + w;
            const float u = e[i];
            xi[w] = (t == 0 || !corr) ? u : (rho * xi[w]) + (c * u);
            float v = mu[i] + sd[i] * xi[w];
            if (do_clip) {
                v = v < lo ? lo : v;
                v = v > clip ? clip : v;
            }
            o[i] = v;
        }
    }
}

constexpr int64_t kMaxBlocks = (int64_t)1 << 30;

}  // namespace

extern "C" int gcpx_cem_warm_start(const float* prev, const int32_t* shift, float init_std, float warm_std, float* mean, float* std_,
                                   int32_t K, int32_t S, int32_t A, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(prev && shift && mean && std_, "null pointer");
    GCPX_CHECK_ARG(K > 0 && S > 0 && A > 0 && (int64_t)S * A <= INT32_MAX, "bad sizes");
    GCPX_CHECK_ARG(warm_std > 0.f && warm_std <= 1.f, "warm_std outside (0, 1]");
    const int blocks_d = (int)(((int64_t)S * A + 255) / 256);
    GCPX_CHECK_ARG((int64_t)K * blocks_d <= kMaxBlocks, "too many (task, column) blocks for one launch");
    const float warm = warm_std * init_std;
    hipLaunchKernelGGL(cem_warm_start_kernel, dim3((unsigned)((int64_t)K * blocks_d)), dim3(256), 0, stream, prev, shift, init_std, warm, mean,
                       std_, S, A, blocks_d);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_cem_population_ex(const float* mean, const float* std_, const float* eps, float clip, float rho, const float* prev_pop,
                                      const int32_t* prev_idx, int32_t m, int32_t n_prev, float* out, int32_t K, int32_t n, int32_t S,
                                      int32_t A, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(mean && std_ && eps && out, "null pointer");
    GCPX_CHECK_ARG(K > 0 && n > 0 && S > 0 && A > 0 && (int64_t)S * A <= INT32_MAX, "bad sizes");
    GCPX_CHECK_ARG(rho >= 0.f && rho < 1.f, "rho outside [0, 1)");
    GCPX_CHECK_ARG(m >= 0 && m <= n, "m outside [0, n]");
    const int64_t D = (int64_t)S * A;
    if (m > 0) {
        GCPX_CHECK_ARG(prev_pop && prev_idx, "null pointer (prev_pop, prev_idx with m > 0)");
        GCPX_CHECK_ARG(n_prev > 0 && m <= n_prev, "m > n_prev");
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(prev_pop), o0 = reinterpret_cast<uintptr_t>(out);
        GCPX_CHECK_ARG(p0 + (uint64_t)K * n_prev * D * sizeof(float) <= o0 || o0 + (uint64_t)K * n * D * sizeof(float) <= p0,
                       "out overlaps prev_pop");
    }
    // The split of a row over threads.  The noise of a column is a chain over the S steps, so a thread owns whole columns.  From A = 5 up,
    // one thread per (row, column): consecutive threads read consecutive floats of a step.  For A = 2 .. 4 (visual MPC plans 2 numbers
    // per step) one thread per row with its A columns in registers: a step of a row is then one contiguous 8 .. 16 byte piece per
    // thread, its A chains give the thread independent work, and the launch has A times fewer threads walking the steps.  This rests on
    // that reasoning alone: neither split has been timed against the other, and the launch is small beside the rollout that follows.
    const int W = (A >= 2 && A <= 4) ? A : 1;
    const int G = A / W;
    const int64_t threads = (int64_t)K * n * G;
    const int64_t blocks = (threads + 255) / 256;
    GCPX_CHECK_ARG(blocks <= kMaxBlocks, "population too large for one launch");
    const int do_clip = clip == clip && clip != __builtin_inff() && clip != -__builtin_inff();
    const float c = (float)sqrt(1.0 - (double)rho * (double)rho);
#define GCPX_CEM_POP_EX(W_)                                                                                                              \
    hipLaunchKernelGGL(cem_population_ex_kernel<W_>, dim3((unsigned)blocks), dim3(256), 0, stream, mean, std_, eps, clip, do_clip, rho, c, \
                       prev_pop, prev_idx, m, n_prev, out, n, S, A, G, threads)
    switch (W) {
        case 2: GCPX_CEM_POP_EX(2); break;
        case 3: GCPX_CEM_POP_EX(3); break;
        case 4: GCPX_CEM_POP_EX(4); break;
        default: GCPX_CEM_POP_EX(1); break;
    }
#undef GCPX_CEM_POP_EX
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_cem_population(const float* mean, const float* std_, const float* eps, float clip, float* out, int32_t K, int32_t n,
                                   int32_t D, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(mean && std_ && eps && out, "null pointer");
    GCPX_CHECK_ARG(K > 0 && n > 0 && D > 0, "bad sizes");
    const int chunks = (D + kPopCols - 1) / kPopCols;
    GCPX_CHECK_ARG((int64_t)K * n * chunks <= kMaxBlocks, "population too large for one launch");
    const int do_clip = clip == clip && clip != __builtin_inff() && clip != -__builtin_inff();
    hipLaunchKernelGGL(cem_population_kernel, dim3((unsigned)((int64_t)K * n * chunks)), dim3(256), 0, stream, mean, std_, eps, clip, do_clip,
                       out, n, D, chunks);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_cem_elites(const float* scores, int32_t* idx, float* elite_scores, int32_t K, int32_t n, int32_t n_elite, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(scores && idx && elite_scores, "null pointer");
    GCPX_CHECK_ARG(K > 0 && n > 0 && n_elite > 0 && K <= kMaxBlocks, "bad sizes");
    GCPX_CHECK_ARG(n_elite <= n, "n_elite > n");
    GCPX_CHECK_ARG(n <= GCPX_CEM_MAX_N, "n above GCPX_CEM_MAX_N (the scores of a task are staged in LDS)");
    hipLaunchKernelGGL(cem_elites_kernel, dim3(K), dim3(256), 0, stream, scores, idx, elite_scores, n, n_elite);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_cem_refit(const float* samples, const int32_t* idx, float* mean, float* std_, float* best, int32_t K, int32_t n,
                              int32_t n_elite, int32_t D, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(samples && idx && mean && std_ && best, "null pointer");
    GCPX_CHECK_ARG(K > 0 && n > 0 && n_elite > 0 && D > 0, "bad sizes");
    GCPX_CHECK_ARG(n_elite <= n, "n_elite > n");
    GCPX_CHECK_ARG(n <= GCPX_CEM_MAX_N, "n above GCPX_CEM_MAX_N");
    const int blocks_d = (D + 255) / 256;
    GCPX_CHECK_ARG((int64_t)K * blocks_d <= kMaxBlocks, "too many (task, column) blocks for one launch");
    hipLaunchKernelGGL(cem_refit_kernel, dim3((unsigned)((int64_t)K * blocks_d)), dim3(256), 0, stream, samples, idx, mean, std_, best, n,
                       n_elite, D, blocks_d);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
