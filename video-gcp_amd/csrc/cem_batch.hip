// The per-iteration arithmetic of the flat CEM planner (planning.py: CEMPlanner.plan_batch) for K planning tasks at once: the population
// from unit noise, the elite pick and the refit of the K Gaussians (gcp/planning/cem/cem_planner.py:55-135, sampler.py:33-48).  One launch
// each over all tasks; nothing is read back between them.  Every result is defined as a fixed sequence of separately rounded float32
// operations, which the torch mirrors in planning.py repeat: the compiler may not contract a multiply and an add into an FMA in this
// file: it is built with -ffp-contract=off (csrc/sources.sh: GCPX_NO_CONTRACT; hipcc contracts by default, and the __fmul_rn / __fadd_rn
// intrinsics are plain operators to it).  `/` and sqrtf are the correctly rounded ones (hipcc's default for float32).
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

constexpr int64_t kMaxBlocks = (int64_t)1 << 30;

}  // namespace

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
