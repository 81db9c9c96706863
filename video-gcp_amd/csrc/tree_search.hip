// The per-decision steps of the hierarchical latent search (tree_latent_search.py: _dopt_subgoal, _dopt_children, _dbest_segment) for
// K planning tasks at once: int32 tables of (row, first, end) views into the rollout's latents, float32 latent rows.  Latency-bound
// glue: one workgroup per (task, candidate) for the row copies, one per task for the selections; nothing is read back between them.
#include "common.h"

namespace {

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// latent (row, frame) of lat [n_rows][T][nz4 float4]; both indices are clamped into the tensor: a table that is out of range reads
// another row, never memory outside `lat`
__device__ __forceinline__ const float4* lat_row(const float4* __restrict__ lat, const int row, const int frame, const int n_rows,
                                                 const int T, const int nz4) {
    return lat + ((size_t)clampi(row, 0, n_rows - 1) * T + clampi(frame, 0, T - 1)) * nz4;
}

// the goal latent of candidate (row, a, b) of task k: (goal row, frame), or the candidate's own last frame when goal row < 0
__device__ __forceinline__ const float4* goal_row(const float4* __restrict__ lat, const int32_t* __restrict__ goal, const int k,
                                                  const int row, const int b, const int n_rows, const int T, const int nz4) {
    const int gr = goal[2 * k], gf = goal[2 * k + 1];
    return gr < 0 ? lat_row(lat, row, b - 1, n_rows, T, nz4) : lat_row(lat, gr, gf, n_rows, T, nz4);
}

// workgroup r = (k, g): rows r and KG + r of both operand matrices
__global__ void __launch_bounds__(64) subgoal_rows_kernel(const float4* __restrict__ lat, const int32_t* __restrict__ views,
                                                          const int32_t* __restrict__ goal, float4* __restrict__ opa,
                                                          float4* __restrict__ opb, int32_t* __restrict__ mids, const int KG,
                                                          const int G, const int n_rows, const int T, const int nz4) {
    const int r = blockIdx.x, k = r / G;
    const int row = views[3 * r], a = views[3 * r + 1], b = views[3 * r + 2];
    const int m = b > a ? (b - a) / 2 : 0;
    const float4* start = lat_row(lat, row, a, n_rows, T, nz4);
    const float4* sub = lat_row(lat, row, a + m, n_rows, T, nz4);
    const float4* gl = goal_row(lat, goal, k, row, b, n_rows, T, nz4);
    for (int d = threadIdx.x; d < nz4; d += 64) {
        const float4 s = start[d], u = sub[d], g = gl[d];
        opa[(size_t)r * nz4 + d] = s;
        opb[(size_t)r * nz4 + d] = u;
        opa[((size_t)KG + r) * nz4 + d] = u;
        opb[((size_t)KG + r) * nz4 + d] = g;
    }
    if (threadIdx.x == 0) mids[r] = m;
}

// workgroup k: numpy's argmin of total = c1 (+ c2) over the candidates the mask admits, then the chosen row of `draw`
__global__ void __launch_bounds__(64) select_kernel(const float* __restrict__ c1, const float* __restrict__ c2,
                                                    const int32_t* __restrict__ mask, const float4* __restrict__ draw,
                                                    float4* __restrict__ best_z, int32_t* __restrict__ idx, float* __restrict__ cost,
                                                    const int G, const int zf4) {
    const int k = blockIdx.x;
    __shared__ int chosen;
    if (threadIdx.x == 0) {
        int best = -1;
        float bv = __builtin_inff();
        for (int g = 0; g < G; ++g) {
            if (mask && mask[k * G + g] == 0) continue;
            const float v = c2 ? c1[k * G + g] + c2[k * G + g] : c1[k * G + g];
            // np.argmin: the first NaN when there is one, else the first minimum
            if (best < 0) { best = g; bv = v; }
            else if (bv != bv) { }
            else if (v != v || v < bv) { best = g; bv = v; }
        }
        idx[k] = best;
        cost[k] = bv;
        chosen = best;
    }
    __syncthreads();
    if (draw && chosen >= 0) {
        const float4* src = draw + ((size_t)k * G + chosen) * zf4;
        for (int d = threadIdx.x; d < zf4; d += 64) best_z[(size_t)k * zf4 + d] = src[d];
    }
}

// one thread per (k, g)
__global__ void __launch_bounds__(64) split_views_kernel(const int32_t* __restrict__ views, const int dummy_row,
                                                         int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                         int32_t* __restrict__ left_goal, int32_t* __restrict__ short_,
                                                         const int KG, const int G) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= KG) return;
    int row = views[3 * r], a = views[3 * r + 1], b = views[3 * r + 2];
    const int is_short = b - a < 3;
    if (is_short) { row = dummy_row; a = 0; b = 3; }        // the stand-in [inf, 0, inf] (tree_optimizer.py:142-147)
    const int c = (b - a) / 2;
    left[3 * r] = row; left[3 * r + 1] = a; left[3 * r + 2] = a + c;
    right[3 * r] = row; right[3 * r + 1] = a + c; right[3 * r + 2] = b;
    short_[r] = is_short;
    if (r % G == 0) { left_goal[2 * (r / G)] = row; left_goal[2 * (r / G) + 1] = a + c; }
}

// workgroup r = (k, g): the view's frames, zero padded to tmax, its length and its goal latent
__global__ void __launch_bounds__(64) segment_windows_kernel(const float4* __restrict__ lat, const int32_t* __restrict__ views,
                                                             const int32_t* __restrict__ goal, float4* __restrict__ seg,
                                                             int32_t* __restrict__ lens, float4* __restrict__ goal_rows, const int G,
                                                             const int n_rows, const int T, const int tmax, const int nz4) {
    const int r = blockIdx.x, k = r / G;
    const int row = views[3 * r], a = views[3 * r + 1], b = views[3 * r + 2];
    const int len = clampi(b - a, 0, tmax);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < tmax; ++t) {
        const float4* src = lat_row(lat, row, a + t, n_rows, T, nz4);
        for (int d = threadIdx.x; d < nz4; d += 64) seg[((size_t)r * tmax + t) * nz4 + d] = t < len ? src[d] : zero;
    }
    const float4* gl = goal_row(lat, goal, k, row, b, n_rows, T, nz4);
    for (int d = threadIdx.x; d < nz4; d += 64) goal_rows[(size_t)r * nz4 + d] = gl[d];
    if (threadIdx.x == 0) lens[r] = len;
}

// one thread per task
__global__ void __launch_bounds__(64) short_alternative_kernel(const float* __restrict__ lc, const float* __restrict__ rc,
                                                               const float* __restrict__ sc, const int32_t* __restrict__ sidx,
                                                               float* __restrict__ cost, int32_t* __restrict__ use_short, const int K) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const float c = lc[k] + rc[k];
    const int use = sidx[k] >= 0 && (sc[k] < c || c != c);
    cost[k] = use ? sc[k] : c;
    use_short[k] = use;
}

constexpr int kMaxDim = 1 << 24;

}  // namespace

extern "C" int gcpx_tree_subgoal_rows(const float* lat, const int32_t* views, const int32_t* goal, float* opa, float* opb, int32_t* mids,
                                      int32_t K, int32_t G, int32_t n_rows, int32_t T, int32_t nz, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(lat && views && goal && opa && opb && mids, "null pointer");
    GCPX_CHECK_ARG(K > 0 && G > 0 && (int64_t)K * G <= kMaxDim && n_rows > 0 && T > 0 && nz > 0 && nz % 4 == 0, "bad sizes");
    hipLaunchKernelGGL(subgoal_rows_kernel, dim3(K * G), dim3(64), 0, stream, reinterpret_cast<const float4*>(lat), views, goal,
                       reinterpret_cast<float4*>(opa), reinterpret_cast<float4*>(opb), mids, K * G, G, n_rows, T, nz / 4);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_tree_select(const float* c1, const float* c2, const int32_t* mask, const float* draw, float* best_z, int32_t* idx,
                                float* cost, int32_t K, int32_t G, int32_t zf, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(c1 && idx && cost, "null pointer");
    GCPX_CHECK_ARG((draw == nullptr) == (best_z == nullptr), "draw and best_z go together");
    GCPX_CHECK_ARG(K > 0 && G > 0 && (int64_t)K * G <= kMaxDim && (!draw || (zf > 0 && zf % 4 == 0)), "bad sizes");
    hipLaunchKernelGGL(select_kernel, dim3(K), dim3(64), 0, stream, c1, c2, mask, reinterpret_cast<const float4*>(draw),
                       reinterpret_cast<float4*>(best_z), idx, cost, G, draw ? zf / 4 : 0);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_tree_split_views(const int32_t* views, int32_t dummy_row, int32_t* left, int32_t* right, int32_t* left_goal,
                                     int32_t* short_, int32_t K, int32_t G, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(views && left && right && left_goal && short_, "null pointer");
    GCPX_CHECK_ARG(K > 0 && G > 0 && (int64_t)K * G <= kMaxDim && dummy_row >= 0, "bad sizes");
    hipLaunchKernelGGL(split_views_kernel, dim3((K * G + 63) / 64), dim3(64), 0, stream, views, dummy_row, left, right, left_goal, short_,
                       K * G, G);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_tree_segment_windows(const float* lat, const int32_t* views, const int32_t* goal, float* seg, int32_t* lens,
                                         float* goal_rows, int32_t K, int32_t G, int32_t n_rows, int32_t T, int32_t tmax, int32_t nz,
                                         void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(lat && views && goal && seg && lens && goal_rows, "null pointer");
    GCPX_CHECK_ARG(K > 0 && G > 0 && (int64_t)K * G <= kMaxDim && n_rows > 0 && T > 0 && tmax > 0 && nz > 0 && nz % 4 == 0, "bad sizes");
    hipLaunchKernelGGL(segment_windows_kernel, dim3(K * G), dim3(64), 0, stream, reinterpret_cast<const float4*>(lat), views, goal,
                       reinterpret_cast<float4*>(seg), lens, reinterpret_cast<float4*>(goal_rows), G, n_rows, T, tmax, nz / 4);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_tree_short_alternative(const float* lc, const float* rc, const float* sc, const int32_t* sidx, float* cost,
                                           int32_t* use_short, int32_t K, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(lc && rc && sc && sidx && cost && use_short, "null pointer");
    GCPX_CHECK_ARG(K > 0 && K <= kMaxDim, "bad sizes");
    hipLaunchKernelGGL(short_alternative_kernel, dim3((K + 63) / 64), dim3(64), 0, stream, lc, rc, sc, sidx, cost, use_short, K);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
