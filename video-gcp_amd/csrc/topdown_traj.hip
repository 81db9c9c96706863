// State trajectories drawn on the nav datasets' top-down picture: Multiroom3dEnv.render_top_down (multiroom3d_env.py:151-183) for every
// logged sample in one launch.  The written spec is at gcpx_topdown_trajectories in include/gcpx.h; its definition is the numpy mirror
// visualization.render_trajectories_numpy.  Per canvas i and layer l, with m = min(len[i], P) points:
//     (x, y) -> (x, -y); all 2 m values divided by 27 when their max > 1 or their min < -1 (a NaN among them: neither holds, as in
//     numpy); + 0.5 * table_size; px = int(x * scale), py = S - int(y * scale)                            -- float32, nothing contracted
//     segment j = 0 .. m - 2 paints the pixels within thickness / 2 of it (exact int64 test), colour trunc(c * 0.5^hits * 255)
//     then the agent stamp on point 0 and the goal stamp on point m - 1
// and a later write wins.
//
// One workgroup = one 32 x 32 tile of one canvas; a thread owns four pixels of it (column tid & 31, rows (tid >> 5) + 8 r) from the
// background read to the store, so the paint order is the loop order.  Per layer the workgroup converts the points once into LDS
// (every workgroup of a canvas repeats the layer's max / min reduction: at most 2048 values), marks the segments whose bounding box,
// grown by the half thickness, meets the tile, and walks the m - 1 marks; only a marked segment is tested.  Every loop bound is an
// argument or a clamped length.  Byte stores of the vector unit only, no atomics.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kPix = (kTile * kTile) / kThreads;          // pixels per thread
constexpr int kStampMax = 31;
constexpr int kHit = 1 << 24;                             // bit of a segment's colour word: the segment may touch this tile

struct TrajLayers {
    gcpx_traj_layer l[GCPX_TRAJ_LAYERS_PER_LAUNCH];
};

// float32 product -> pixel offset: truncated toward zero; the float clamp keeps the conversion defined, the caller clamps again
__device__ __forceinline__ int trunc_clamped(const float v) { return (int)fminf(fmaxf(truncf(v), -1073741824.f), 1073741824.f); }

__device__ __forceinline__ int clamp_coord(const int v) { return min(max(v, -GCPX_TRAJ_COORD_LIMIT), GCPX_TRAJ_COORD_LIMIT); }

__device__ __forceinline__ uint32_t colour_byte(const float c) {
    const float v = truncf(c * 255.f);
    return (uint32_t)(v >= 255.f ? 255.f : (v > 0.f ? v : 0.f));          // a NaN gives 0
}

// the pixel (qx, qy) lies within thickness / 2 of the segment a -> b: the end-point cases by the sign of the projection, else the
// distance to the line, all in int64 (|coordinates| <= GCPX_TRAJ_COORD_LIMIT keeps 4 cross^2 below 2^63)
__device__ __forceinline__ bool covers(const int ax, const int ay, const int bx, const int by, const int qx, const int qy) {
    constexpr long long th2 = (long long)GCPX_TRAJ_THICKNESS * GCPX_TRAJ_THICKNESS;
    const long long dx = bx - ax, dy = by - ay, wx = qx - ax, wy = qy - ay;
    const long long dd = dx * dx + dy * dy, t = wx * dx + wy * dy;
    if (t <= 0) return 4 * (wx * wx + wy * wy) <= th2;
    if (t >= dd) {
        const long long ux = qx - bx, uy = qy - by;
        return 4 * (ux * ux + uy * uy) <= th2;
    }
    const long long cr = dx * wy - dy * wx;
    return 4 * cr * cr <= th2 * dd;
}

__global__ void __launch_bounds__(kThreads) topdown_trajectories_kernel(
    const uint8_t* __restrict__ bg, const int S, const int cw, const uint8_t* __restrict__ agent_stamp,
    const uint8_t* __restrict__ goal_stamp, const int k, const uint32_t agent_rgb, const uint32_t goal_rgb, const TrajLayers layers,
    const int n_layers, const int first, const float half_table, const float scale, uint8_t* __restrict__ out) {
    __shared__ int s_px[GCPX_TRAJ_MAX_POINTS], s_py[GCPX_TRAJ_MAX_POINTS];
    __shared__ uint32_t s_seg[GCPX_TRAJ_MAX_POINTS];      // segment j: colour | kHit; s_ok[j]: point j is finite
    __shared__ uint8_t s_ok[GCPX_TRAJ_MAX_POINTS];
    __shared__ uint8_t s_stamp[2][kStampMax * kStampMax];
    __shared__ float s_max[kThreads / 64], s_min[kThreads / 64];
    __shared__ int s_nan[kThreads / 64];
    const int tid = threadIdx.x;
    const int tiles = (S + kTile - 1) / kTile;
    const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
    const int i = blockIdx.y;
    const int x0 = tx * kTile, y0 = ty * kTile;
    const int qx = x0 + (tid & (kTile - 1)), qy0 = y0 + (tid >> 5);
    const int h = k >> 1;
    for (int e = tid; e < k * k; e += kThreads) {
        s_stamp[0][e] = agent_stamp[e] != 0;
        s_stamp[1][e] = goal_stamp[e] != 0;
    }
    // this thread's pixels: the unpadded picture (the first launch of a call) or what the launches before left
    uint32_t rgb[kPix];
    const int side = S + 2 * cw;
#pragma unroll
    for (int r = 0; r < kPix; ++r) {
        const int qy = qy0 + r * (kThreads / kTile);
        rgb[r] = 0;
        if (qx < S && qy < S) {
            const uint8_t* p = first ? bg + ((size_t)(qy + cw) * side + (qx + cw)) * 3 : out + (((size_t)i * S + qy) * S + qx) * 3;
            rgb[r] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
    }
    for (int li = 0; li < n_layers; ++li) {
        const gcpx_traj_layer& L = layers.l[li];
        const long long len = L.len_i64 ? reinterpret_cast<const long long*>(L.len)[i] : (long long)reinterpret_cast<const int32_t*>(L.len)[i];
        const int m = (int)(len < (long long)L.P ? len : (long long)L.P);
        if (m < 1) continue;                              // (uniform over the workgroup)
        const float* st = L.states + (long long)i * L.s_n;
        // max / min of the 2 m values after the y flip; a NaN switches the division off, as numpy's max() / min() return it
        float vmax = -INFINITY, vmin = INFINITY;
        int any_nan = 0;
        for (int p = tid; p < m; p += kThreads) {
            const float x = st[(long long)p * L.s_p], y = st[(long long)p * L.s_p + L.s_d] * -1.f;
            any_nan |= (x != x) | (y != y);
            vmax = fmaxf(vmax, fmaxf(x, y));
            vmin = fminf(vmin, fminf(x, y));
        }
        for (int o = 32; o > 0; o >>= 1) {
            vmax = fmaxf(vmax, __shfl_xor(vmax, o));
            vmin = fminf(vmin, __shfl_xor(vmin, o));
            any_nan |= __shfl_xor(any_nan, o);
        }
        __syncthreads();                                  // the layer before is done with the LDS
        if ((tid & 63) == 0) {
            s_max[tid >> 6] = vmax;
            s_min[tid >> 6] = vmin;
            s_nan[tid >> 6] = any_nan;
        }
        __syncthreads();
        bool divide = false, nan_seen = false;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            divide |= s_max[w] > 1.f || s_min[w] < -1.f;
            nan_seen |= s_nan[w] != 0;
        }
        divide = divide && !nan_seen;
        for (int p = tid; p < m; p += kThreads) {
            float x = st[(long long)p * L.s_p], y = st[(long long)p * L.s_p + L.s_d] * -1.f;
            if (divide) {                                 // correctly rounded, as numpy's float32 division
                x = (float)((double)x / 27.0);
                y = (float)((double)y / 27.0);
            }
            x = x + half_table;
            y = y + half_table;
            const float fx = x * scale, fy = y * scale;
            s_ok[p] = isfinite(fx) && isfinite(fy);
            s_px[p] = clamp_coord(trunc_clamped(fx));
            s_py[p] = clamp_coord(S - trunc_clamped(fy));
        }
        __syncthreads();
        // segment j: its colour (halved once per hit of the two index statements of nav_9rooms.py:46-49) and whether it can touch the tile
        const long long last = len - 1;
        for (int j = tid; j < m - 1; j += kThreads) {
            int hits = 0;
            if (L.dim_t) {
                bool here = false, next = false;
                for (int q = 0; q < L.K; ++q) {
                    const long long t = min((long long)L.dim_t[(long long)i * L.K + q], last);
                    here |= t == j;
                    next |= t == j + 1;
                }
                hits = (int)here + (int)next;
            }
            const float f = hits == 0 ? 1.f : (hits == 1 ? 0.5f : 0.25f);
            uint32_t w = colour_byte(L.color[0] * f) | colour_byte(L.color[1] * f) << 8 | colour_byte(L.color[2] * f) << 16;
            constexpr int g = (GCPX_TRAJ_THICKNESS + 1) / 2;
            const int ax = s_px[j], ay = s_py[j], bx = s_px[j + 1], by = s_py[j + 1];
            const bool hit = s_ok[j] && s_ok[j + 1] && max(ax, bx) + g >= x0 && min(ax, bx) - g < x0 + kTile && max(ay, by) + g >= y0 &&
                             min(ay, by) - g < y0 + kTile;
            s_seg[j] = w | (hit ? kHit : 0);
        }
        __syncthreads();
        for (int j = 0; j < m - 1; ++j) {
            const uint32_t w = s_seg[j];
            if (!(w & kHit)) continue;
            const int ax = s_px[j], ay = s_py[j], bx = s_px[j + 1], by = s_py[j + 1];
#pragma unroll
            for (int r = 0; r < kPix; ++r)
                if (covers(ax, ay, bx, by, qx, qy0 + r * (kThreads / kTile))) rgb[r] = w & 0xFFFFFF;
        }
        // render_pos_top_down(traj[0], traj[-1]): the agent's stamp on point 0, then the goal's on point m - 1
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int p = s ? m - 1 : 0;
            if (!s_ok[p]) continue;
            const int ex = qx - s_px[p] + h;
            if (ex < 0 || ex >= k) continue;
#pragma unroll
            for (int r = 0; r < kPix; ++r) {
                const int ey = qy0 + r * (kThreads / kTile) - s_py[p] + h;
                if (ey >= 0 && ey < k && s_stamp[s][ey * k + ex]) rgb[r] = s ? goal_rgb : agent_rgb;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kPix; ++r) {
        const int qy = qy0 + r * (kThreads / kTile);
        if (qx < S && qy < S) {
            uint8_t* p = out + (((size_t)i * S + qy) * S + qx) * 3;
            p[0] = (uint8_t)(rgb[r] & 255);
            p[1] = (uint8_t)((rgb[r] >> 8) & 255);
            p[2] = (uint8_t)((rgb[r] >> 16) & 255);
        }
    }
}

// out[i][j] = first maximum over t of w[i][df(j)][t], df(j) the depth-first position of breadth-first node j (a NaN counts as the
// maximum, as in numpy.argmax)
__global__ void __launch_bounds__(64) topdown_bottlenecks_kernel(const float* __restrict__ w, const int N, const int T, const int levels,
                                                                 const int n, const int K, int32_t* __restrict__ out) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n * K) return;
    const int i = e / K, j = e - i * K;
    const int l = 31 - __clz(j + 1), pos = j + 1 - (1 << l);
    const int df = (2 * pos + 1) * (1 << (levels - 1 - l)) - 1;
    const float* row = w + ((size_t)i * N + df) * T;
    float best = row[0];
    int at = 0;
    for (int t = 1; t < T; ++t) {
        const float v = row[t];
        if (best == best && (v > best || v != v)) {
            best = v;
            at = t;
        }
    }
    out[e] = at;
}

}  // namespace

extern "C" int gcpx_topdown_trajectories(const uint8_t* background, int32_t S, int32_t cw, const uint8_t* agent_stamp,
                                         const uint8_t* goal_stamp, int32_t k, int32_t agent_rgb, int32_t goal_rgb,
                                         const gcpx_traj_layer* layers, int32_t n_layers, int32_t n, int32_t state_dim,
                                         int32_t n_rooms, int32_t render_scale, uint8_t* out, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(background && agent_stamp && goal_stamp && out, "null background / stamp / output pointer");
    GCPX_CHECK_ARG(S > 0 && S <= GCPX_TRAJ_MAX_SIDE, "the picture's side S must be in [1, 2048]");
    GCPX_CHECK_ARG(cw >= 0 && cw <= 4096, "crop_window must be in [0, 4096]");
    GCPX_CHECK_ARG(k > 0 && (k & 1) == 1 && k <= kStampMax, "the stamp side k must be odd and at most 31");
    GCPX_CHECK_ARG(n > 0 && n <= 65535, "n canvases: 1 .. 65535");
    GCPX_CHECK_ARG(state_dim == 2, "state_dim must be 2 (x, y)");
    GCPX_CHECK_ARG(n_layers >= 0 && n_layers <= GCPX_TRAJ_MAX_LAYERS, "n_layers: 0 .. 64");
    GCPX_CHECK_ARG(n_layers == 0 || layers, "null layer table");
    GCPX_CHECK_ARG(n_rooms > 0 && render_scale > 0, "n_rooms and render_scale must be positive");
    for (int l = 0; l < n_layers; ++l) {
        GCPX_CHECK_ARG(layers[l].states && layers[l].len, "a layer's states / len pointer is null");
        GCPX_CHECK_ARG(layers[l].P > 0 && layers[l].P <= GCPX_TRAJ_MAX_POINTS, "a layer's P points per trajectory: 1 .. 1024");
        GCPX_CHECK_ARG(!layers[l].dim_t || (layers[l].K > 0 && layers[l].K <= GCPX_TRAJ_MAX_DIM), "dim_t: K must be in [1, 16]");
    }
    // 0.5 * table_size as the reference computes it in Python floats, rounded to float32 once where it meets the float32 states
    const float half_table = (float)(0.5 * ((1.0 / 3) * (double)(int)sqrt((double)n_rooms)));
    const int tiles = (S + kTile - 1) / kTile;
    const dim3 grid((unsigned)(tiles * tiles), (unsigned)n);
    int l0 = 0;
    do {                                                  // the launches of one stream run in order: a later layer still wins
        TrajLayers tab{};
        const int cnt = n_layers - l0 < GCPX_TRAJ_LAYERS_PER_LAUNCH ? n_layers - l0 : GCPX_TRAJ_LAYERS_PER_LAUNCH;
        for (int l = 0; l < cnt; ++l) tab.l[l] = layers[l0 + l];
        hipLaunchKernelGGL(topdown_trajectories_kernel, grid, dim3(kThreads), 0, stream, background, S, cw, agent_stamp, goal_stamp, k,
                           (uint32_t)agent_rgb & 0xFFFFFFu, (uint32_t)goal_rgb & 0xFFFFFFu, tab, cnt, l0 == 0 ? 1 : 0, half_table,
                           (float)render_scale, out);
        l0 += cnt;
    } while (l0 < n_layers);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_topdown_bottlenecks(const float* match_dist_df, int32_t B, int32_t N, int32_t T, int32_t levels, int32_t n, int32_t K,
                                        int32_t* out, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(match_dist_df && out, "null pointer");
    GCPX_CHECK_ARG(levels > 0 && levels <= 20 && N == (1 << levels) - 1, "N must be 2^levels - 1");
    GCPX_CHECK_ARG(B > 0 && T > 0 && n > 0 && n <= B, "bad sizes: 0 < n <= B, T > 0");
    GCPX_CHECK_ARG(K > 0 && K <= N && K <= GCPX_TRAJ_MAX_DIM, "K must be in [1, min(N, 16)]");
    hipLaunchKernelGGL(topdown_bottlenecks_kernel, dim3((unsigned)((n * K + 63) / 64)), dim3(64), 0, stream, match_dist_df, N, T, levels, n,
                       K, out);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
