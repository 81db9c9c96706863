// Top-of-N accumulation of the evaluation (video-gcp_amd/evaluation.py, Evaluator.eval): after prior sample n of N has been aligned
// and scored, this records its [B][3] metrics, keeps the index of the best sample per sequence and copies the frames of a sample that
// becomes best.  Counterpart of the reference's per-sample buffer update and best-sample bookkeeping on the host
// (gcp/evaluation/compute_metrics.py:89-120 eval_single / compute_metrics, :236-250 _is_better / _get_best_idxs).
//
// "Better" is the order np.argmin / np.argmax give over the samples 0..n: strictly lower (mse) or higher (psnr, ssim), so the first
// sample wins a tie; a NaN (a sequence with no frame left after the crop) beats any number, since both return the first NaN.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSelectThreads = 64;
constexpr int kMaxBlocksPerSeq = 64;

__device__ __forceinline__ bool better(const float v, const float cur, const bool lower) {
    if (isnan(v)) return !isnan(cur);
    return lower ? v < cur : v > cur;
}

// one thread per sequence: all[b][n][:] = metrics[b][:]; best[b] = n when sample n is better than the best of samples 0..n-1
__global__ void __launch_bounds__(kSelectThreads) topn_select_kernel(const float* __restrict__ metrics, const int B, const int n,
                                                                     const int N, const int comp, const int lower,
                                                                     float* __restrict__ all, int32_t* __restrict__ best) {
    const int b = blockIdx.x * kSelectThreads + threadIdx.x;
    if (b >= B) return;
    const float m0 = metrics[b * 3 + 0], m1 = metrics[b * 3 + 1], m2 = metrics[b * 3 + 2];
    float* row = all + ((size_t)b * N + n) * 3;
    row[0] = m0;
    row[1] = m1;
    row[2] = m2;
    const float v = comp == 0 ? m0 : (comp == 1 ? m1 : m2);
    if (n == 0) {
        best[b] = 0;
        return;
    }
    const int cur = best[b];
    if (cur < 0 || cur >= n || better(v, all[((size_t)b * N + cur) * 3 + comp], lower != 0)) best[b] = n;
}

__device__ __forceinline__ int frame_row(const int32_t* __restrict__ map, const int32_t* __restrict__ first,
                                         const int32_t* __restrict__ last, const int b, const int t, const int T, const int rows) {
    if (first && t < first[b]) return -1;
    if (last && t >= last[b]) return -1;
    const int r = map[(size_t)b * T + t];
    return r < rows ? r : -1;
}

// grid (x, B): sequences whose best is not sample n leave at once; the others copy, per destination frame, the pool frame its map names
// (zeros where there is none).  dst0 [B][T0] frames of the aligned set (map0 inside [first, last)), then dst1 [B][T1] (map1 only).
__global__ void __launch_bounds__(kThreads) topn_copy_kernel(const int32_t* __restrict__ best, const int n,
                                                             const float4* __restrict__ pool0, const int32_t* __restrict__ map0,
                                                             const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                                             const int rows0, const int T0, float4* __restrict__ dst0,
                                                             const float4* __restrict__ pool1, const int32_t* __restrict__ map1,
                                                             const int rows1, const int T1, float4* __restrict__ dst1,
                                                             const long long D4) {
    const int b = blockIdx.y;
    if (best[b] != n) return;
    const long long total = (long long)(T0 + T1) * D4;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const int f = (int)(i / D4);
        const long long k = i - (long long)f * D4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f < T0) {
            const int r = frame_row(map0, first, last, b, f, T0, rows0);
            if (r >= 0) v = pool0[(size_t)r * D4 + k];
            dst0[((size_t)b * T0 + f) * D4 + k] = v;
        } else {
            const int j = f - T0;
            const int r = frame_row(map1, nullptr, nullptr, b, j, T1, rows1);
            if (r >= 0) v = pool1[(size_t)r * D4 + k];
            dst1[((size_t)b * T1 + j) * D4 + k] = v;
        }
    }
}

}  // namespace

extern "C" int gcpx_topn_accumulate(const float* metrics, int32_t B, int32_t n, int32_t N, int32_t comp, int32_t lower_is_better,
                                    float* all, int32_t* best, const float* pool, int32_t pool_rows, const int32_t* frame_map,
                                    const int32_t* first, const int32_t* last, int32_t T, float* best_frames, const float* full_pool,
                                    int32_t full_rows, const int32_t* full_map, int32_t F, float* best_full, int64_t row_floats,
                                    void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(metrics && all && best, "null pointer");
    GCPX_CHECK_ARG(B > 0 && N > 0 && n >= 0 && n < N && comp >= 0 && comp < 3, "bad sizes");
    GCPX_CHECK_ARG(T >= 0 && F >= 0 && row_floats > 0 && (row_floats & 3) == 0, "bad frame sizes (rows of a multiple of 4 floats)");
    GCPX_CHECK_ARG(T == 0 || (pool && frame_map && best_frames && pool_rows >= 0), "aligned frame set incomplete");
    GCPX_CHECK_ARG(F == 0 || (full_pool && full_map && best_full && full_rows >= 0), "full frame set incomplete");
    GCPX_CHECK_ARG(((reinterpret_cast<uintptr_t>(pool) | reinterpret_cast<uintptr_t>(best_frames) |
                     reinterpret_cast<uintptr_t>(full_pool) | reinterpret_cast<uintptr_t>(best_full)) & 15) == 0,
                   "frames not 16-byte aligned");
    hipLaunchKernelGGL(topn_select_kernel, dim3((B + kSelectThreads - 1) / kSelectThreads), dim3(kSelectThreads), 0, stream, metrics, B,
                       n, N, comp, lower_is_better, all, best);
    if (T + F > 0) {
        const long long D4 = row_floats / 4;
        const long long per_seq = ((long long)(T + F) * D4 + kThreads - 1) / kThreads;
        const dim3 grid((unsigned)(per_seq < kMaxBlocksPerSeq ? per_seq : kMaxBlocksPerSeq), (unsigned)B);
        hipLaunchKernelGGL(topn_copy_kernel, grid, dim3(kThreads), 0, stream, best, n, reinterpret_cast<const float4*>(pool), frame_map,
                           first, last, pool_rows, T, reinterpret_cast<float4*>(best_frames), reinterpret_cast<const float4*>(full_pool),
                           full_map, full_rows, F, reinterpret_cast<float4*>(best_full), D4);
    }
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
