// The nav data generator's expert: a probabilistic road map per trajectory (prm.py of the reference's PrmPolicy), for a batch of
// independent trajectories, one workgroup each.  The written spec is at gcpx_prm_* in include/gcpx.h; its definition is the numpy
// restatement nav_gen.prm_numpy / nav_gen.spline_numpy / nav_gen.sample_points_numpy.
//
//   gcpx_prm_sample_points   uniform draws in room / door boxes from a counter-based generator keyed (seed, trajectory key, draw)
//   gcpx_prm_roadmap         sample_points' obstacle filter (prm.py:229-257), then generate_roadmap / is_collision (:96-159)
//   gcpx_prm_shortest_path   dijkstra_planning (:162-226) as bounded Bellman-Ford sweeps
//   gcpx_prm_resample        splprep(s=0) / splev(linspace(0, 1, n_steps)) (prm_policy.py:173-185) and the recorded episode
//
// All geometry is float64 and nothing is contracted into an FMA: every decision is a threshold test (dist >= rr, d >= max_edge_len,
// dist <= rr) or an order of distances, which in double agree with the reference's except at ties.
//
// Roadmap: the node coordinates live in LDS (2 x GCPX_PRM_MAX_NODES doubles = 32 KiB).  A wave owns node i: its lanes walk all nodes 64
// at a time, test every candidate with d < max_edge_len for collision at once, and insert the survivors into a sorted list that lanes
// 0 .. n_knn - 1 hold in registers -- the first n_knn non-colliding neighbours in ascending distance, as the reference's early-exit loop
// finds them.  A candidate no nearer than a full list's last entry is not tested: it cannot enter.  The nearest obstacle point comes
// from a uniform grid over the cloud (cell > rr, built once per layout on the host): the 3 x 3 cells around the query hold every point
// within one cell size, so the value equals a brute-force scan whenever that is <= cell, and is > cell otherwise.
//
// Shortest path: tentative costs (as the bits of non-negative doubles, ordered like unsigned integers) and predecessors in LDS.  A sweep
// reads the costs of the nodes that improved, a barrier, then relaxes their out-edges with a 64-bit LDS atomic minimum: the fixed point
// does not depend on the order.  At most n sweeps, early exit when nothing changed.  Predecessor of j: the lowest i with
// cost[i] + w(i, j) == cost[j].  Every loop bound is an argument or a clamped count; every index read from memory is range-checked.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = GCPX_PRM_MAX_NODES / kThreads;        // nodes per thread of the path kernel

struct ObsGrid {
    const double* ox;                 // the cloud sorted by cell (row-major cells: cell = cy * gx + cx)
    const double* oy;
    const int32_t* cell_start;        // [gx * gy + 1]
    int n_obs, gx, gy;
    double x0, y0, cell;
};

// distance to the nearest obstacle point among the 3 x 3 cells around (x, y); +inf when they hold none
__device__ __forceinline__ double nearest_obstacle(const ObsGrid& g, const double x, const double y) {
    const double fx = floor((x - g.x0) / g.cell), fy = floor((y - g.y0) / g.cell);
    if (!(fx >= -1.0 && fx <= (double)g.gx && fy >= -1.0 && fy <= (double)g.gy)) return INFINITY;      // (a NaN lands here too)
    const int cx = (int)fx, cy = (int)fy;
    const int xa = max(cx - 1, 0), xb = min(cx + 1, g.gx - 1);
    double best = INFINITY;
    if (xb < xa) return best;
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, g.gy - 1); ++yy) {
        // the cells of one row are adjacent in the sorted cloud: one range
        const int s = max(g.cell_start[yy * g.gx + xa], 0), e = min(g.cell_start[yy * g.gx + xb + 1], g.n_obs);
        for (int k = s; k < e; ++k) {
            const double dx = g.ox[k] - x, dy = g.oy[k] - y;
            best = fmin(best, dx * dx + dy * dy);
        }
    }
    return sqrt(best);                // sqrt is monotone and correctly rounded: the minimum of the roots
}

// is_collision (prm.py:96-122) for an edge already known to have d < max_edge_len
__device__ __forceinline__ bool edge_collides(const ObsGrid& g, const double sx, const double sy, const double gx, const double gy,
                                              const double dx, const double dy, const double d, const double rr) {
    const double yaw = atan2(dy, dx);
    const int nstep = (int)fmin(rint(d / rr), (double)GCPX_PRM_MAX_EDGE_STEPS);     // Python's round: half to even
    const double ax = rr * cos(yaw), ay = rr * sin(yaw);
    double x = sx, y = sy;
    for (int i = 0; i < nstep; ++i) {
        if (nearest_obstacle(g, x, y) <= rr) return true;
        x += ax;                      // accumulated, as the reference does it
        y += ay;
    }
    return nearest_obstacle(g, gx, gy) <= rr;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {     // the splitmix64 output function
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// uniform in [0, 1): 53 bits of the hash of (seed, key, counter)
__device__ __forceinline__ double uniform01(const uint64_t seed, const uint64_t key, const uint64_t ctr) {
    return (double)(mix64(mix64(mix64(seed) ^ key) ^ ctr) >> 11) * 0x1.0p-53;
}

__global__ void __launch_bounds__(kThreads) prm_sample_kernel(const double* __restrict__ boxes, const int n_boxes,
                                                              const int32_t* __restrict__ pt_box, const int32_t* __restrict__ pt_off,
                                                              const int64_t* __restrict__ traj_key, const int32_t* __restrict__ draw0,
                                                              const int total_pts, const uint64_t seed, double* __restrict__ px,
                                                              double* __restrict__ py) {
    const int b = blockIdx.y;
    const int p0 = min(max(pt_off[b], 0), total_pts), p1 = min(max(pt_off[b + 1], p0), total_pts);
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= p1 - p0) return;
    const int bx = pt_box[p0 + p];
    if (bx < 0 || bx >= n_boxes) {                          // no such box: a NaN the caller cannot miss
        px[p0 + p] = NAN;
        py[p0 + p] = NAN;
        return;
    }
    const uint64_t draw = (uint64_t)((int64_t)draw0[b] + p);
    const double u = uniform01(seed, (uint64_t)traj_key[b], 2 * draw), v = uniform01(seed, (uint64_t)traj_key[b], 2 * draw + 1);
    px[p0 + p] = (u - 0.5) * boxes[4 * bx + 2] + boxes[4 * bx];          // _rand(2) * width + center (sampling_fcns.py:33)
    py[p0 + p] = (v - 0.5) * boxes[4 * bx + 3] + boxes[4 * bx + 1];
}

__global__ void __launch_bounds__(kThreads) prm_roadmap_kernel(const ObsGrid g, const double* __restrict__ px, const double* __restrict__ py,
                                                               const int32_t* __restrict__ pt_off, const double* __restrict__ start_goal,
                                                               const int total_pts, const int max_pts, const int cap, const int n_knn,
                                                               const double rr, const double max_len, uint8_t* __restrict__ kept,
                                                               int32_t* __restrict__ n_nodes, double* __restrict__ node_xy,
                                                               int32_t* __restrict__ adj) {
    __shared__ double s_x[GCPX_PRM_MAX_NODES], s_y[GCPX_PRM_MAX_NODES];
    __shared__ int s_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int p0 = min(max(pt_off[b], 0), total_pts), p1 = min(max(pt_off[b + 1], p0), total_pts);
    const int n_pts = min(p1 - p0, max_pts);               // max_pts + 2 <= cap <= GCPX_PRM_MAX_NODES (checked by the caller)
    // sample_points: keep a sample iff its nearest obstacle point is at >= rr; the kept keep their order
    int base = 0;
    for (int c0 = 0; c0 < n_pts; c0 += kThreads) {
        const int p = c0 + tid;
        bool keep = false;
        double x = 0., y = 0.;
        if (p < n_pts) {
            x = px[p0 + p];
            y = py[p0 + p];
            keep = nearest_obstacle(g, x, y) >= rr;
            kept[p0 + p] = keep ? 1 : 0;
        }
        const unsigned long long m = __ballot(keep);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) off += s_cnt[w];
            tot += s_cnt[w];
        }
        if (keep) {
            s_x[off + rank] = x;
            s_y[off + rank] = y;
        }
        base += tot;
        __syncthreads();
    }
    const int n = base + 2;                                 // start and goal: the last two nodes, unfiltered
    if (tid == 0) {
        s_x[base] = start_goal[4 * b];
        s_y[base] = start_goal[4 * b + 1];
        s_x[base + 1] = start_goal[4 * b + 2];
        s_y[base + 1] = start_goal[4 * b + 3];
        n_nodes[b] = n;
    }
    __syncthreads();
    double* nx = node_xy + (size_t)b * 2 * cap;
    for (int i = tid; i < cap; i += kThreads) {
        nx[i] = i < n ? s_x[i] : 0.;
        nx[cap + i] = i < n ? s_y[i] : 0.;
    }
    int32_t* ab = adj + (size_t)b * cap * n_knn;
    for (int e = n * n_knn + tid; e < cap * n_knn; e += kThreads) ab[e] = -1;
    // generate_roadmap: node i's first n_knn non-colliding neighbours in ascending distance
    for (int i = wave; i < n; i += kWaves) {
        const double xi = s_x[i], yi = s_y[i];
        double ld = INFINITY;                               // lane k < n_knn: the k-th entry of the sorted list
        int lj = -1;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            bool cand = false;
            double d = INFINITY;
            const double worst = __shfl(ld, n_knn - 1);     // +inf until the list is full
            if (j < n && j != i) {
                const double dx = s_x[j] - xi, dy = s_y[j] - yi;
                d = sqrt(dx * dx + dy * dy);
                if (d < max_len && d <= worst) cand = !edge_collides(g, xi, yi, s_x[j], s_y[j], dx, dy, d, rr);
            }
            unsigned long long m = __ballot(cand);
            while (m) {                                     // (uniform over the wave)
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const double cd = __shfl(d, src);
                const int cj = __shfl(j, src);
                const bool before = ld < cd || (ld == cd && lj >= 0 && lj < cj);      // a prefix of the lanes: the list is sorted
                const int pos = __popcll(__ballot(before));
                const double pd = __shfl_up(ld, 1);
                const int pj = __shfl_up(lj, 1);
                if (lane == pos) {
                    ld = cd;
                    lj = cj;
                } else if (lane > pos) {
                    ld = pd;
                    lj = pj;
                }
                if (lane >= n_knn) {
                    ld = INFINITY;
                    lj = -1;
                }
            }
        }
        if (lane < n_knn) ab[(size_t)i * n_knn + lane] = lj;
    }
}

__device__ __forceinline__ double edge_cost(const double dx, const double dy, const double power) {
    const double d = sqrt(dx * dx + dy * dy);
    return power == 2.0 ? d * d : pow(d, power);           // cost_fcn(d) = d ** cost_power
}

__global__ void __launch_bounds__(kThreads) prm_path_kernel(const double* __restrict__ node_xy, const int32_t* __restrict__ n_nodes,
                                                            const int32_t* __restrict__ adj, const int cap, const int n_knn,
                                                            const double power, int32_t* __restrict__ success,
                                                            int32_t* __restrict__ n_vert, int32_t* __restrict__ path,
                                                            double* __restrict__ cost) {
    __shared__ double s_x[GCPX_PRM_MAX_NODES], s_y[GCPX_PRM_MAX_NODES];
    __shared__ unsigned long long s_cost[GCPX_PRM_MAX_NODES];
    __shared__ int s_pred[GCPX_PRM_MAX_NODES];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = min(max(n_nodes[b], 0), cap);
    if (n < 2) {                                            // (uniform over the workgroup)
        if (tid == 0) success[b] = 0;
        return;
    }
    const double* nx = node_xy + (size_t)b * 2 * cap;
    const int32_t* ab = adj + (size_t)b * cap * n_knn;
    const unsigned long long inf_bits = (unsigned long long)__double_as_longlong(INFINITY);
    for (int i = tid; i < n; i += kThreads) {
        s_x[i] = nx[i];
        s_y[i] = nx[cap + i];
        s_cost[i] = i == n - 2 ? 0ull : inf_bits;
        s_pred[i] = 0x7fffffff;
    }
    __syncthreads();
    double pushed[kPer];                                    // the cost node tid + 256 r had when its edges were last relaxed
#pragma unroll
    for (int r = 0; r < kPer; ++r) pushed[r] = INFINITY;
    for (int sweep = 0; sweep < n; ++sweep) {
        double ci[kPer];
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int i = tid + r * kThreads;
            ci[r] = i < n ? __longlong_as_double((long long)s_cost[i]) : INFINITY;
        }
        __syncthreads();                                    // every cost of this sweep is read before any is lowered
        int changed = 0;
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int i = tid + r * kThreads;
            if (!(ci[r] < pushed[r])) continue;
            pushed[r] = ci[r];
            for (int k = 0; k < n_knn; ++k) {
                const int j = ab[(size_t)i * n_knn + k];
                if (j < 0 || j >= n) continue;
                const double c = ci[r] + edge_cost(s_x[j] - s_x[i], s_y[j] - s_y[i], power);
                if (!(c >= 0.)) continue;                   // a NaN does not enter
                const unsigned long long bits = (unsigned long long)__double_as_longlong(c);
                if (bits < atomicMin(&s_cost[j], bits)) changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    __syncthreads();
    // predecessor of j: the lowest i whose relaxed cost is j's final cost
    for (int i = tid; i < n; i += kThreads) {
        const double c0 = __longlong_as_double((long long)s_cost[i]);
        if (!(c0 < INFINITY)) continue;
        for (int k = 0; k < n_knn; ++k) {
            const int j = ab[(size_t)i * n_knn + k];
            if (j < 0 || j >= n || j == n - 2) continue;
            const double c = c0 + edge_cost(s_x[j] - s_x[i], s_y[j] - s_y[i], power);
            if ((unsigned long long)__double_as_longlong(c) == s_cost[j]) atomicMin(&s_pred[j], i);
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const double total = __longlong_as_double((long long)s_cost[n - 1]);
    int len = 1, v = n - 1;
    bool ok = total < INFINITY;
    while (ok && v != n - 2) {                              // at most n steps: a longer walk is a cycle of zero-length edges
        v = s_pred[v];
        ++len;
        ok = v >= 0 && v < n && len <= n;
    }
    if (!ok) {                                              // an unreachable goal is a normal result; the outputs keep their fill values
        success[b] = 0;
        return;
    }
    int32_t* pb = path + (size_t)b * cap;
    v = n - 1;
    for (int k = len - 1; k >= 0; --k) {
        pb[k] = v;
        v = s_pred[v];
    }
    n_vert[b] = len;
    cost[b] = total;
    success[b] = 1;
}

// One workgroup per trajectory: the interpolating cubic spline over the normalised cumulative chord length with not-a-knot ends -- what
// splprep(s=0) builds (interior knots u[2:-2]) -- as second derivatives M from one tridiagonal solve per coordinate, evaluated at
// linspace(0, 1, n_steps); then the recorded episode in the environment's units.
__global__ void __launch_bounds__(128) prm_resample_kernel(const double* __restrict__ node_xy, const int32_t* __restrict__ n_nodes,
                                                           const int32_t* __restrict__ path, const int32_t* __restrict__ n_vert,
                                                           const int32_t* __restrict__ n_steps, const double* __restrict__ start_goal,
                                                           const int cap, const int T, double* __restrict__ plan,
                                                           int32_t* __restrict__ ok_out, float* __restrict__ states,
                                                           float* __restrict__ actions, float* __restrict__ pad_mask) {
    __shared__ double s_u[GCPX_PRM_MAX_PATH], s_v[2][GCPX_PRM_MAX_PATH], s_M[2][GCPX_PRM_MAX_PATH], s_w[2][GCPX_PRM_MAX_PATH];
    __shared__ int s_ok;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int m = n_vert[b], n = min(max(n_nodes[b], 0), cap);
    const int ns = min(max(n_steps[b], 0), T);
    if (tid == 0) s_ok = (m >= 4 && m <= GCPX_PRM_MAX_PATH && m <= n && ns >= 2) ? 1 : 0;
    __syncthreads();
    if (s_ok) {
        const double* nx = node_xy + (size_t)b * 2 * cap;
        for (int k = tid; k < m; k += 128) {
            const int idx = path[(size_t)b * cap + k];
            if (idx < 0 || idx >= n) {
                s_ok = 0;
            } else {
                s_v[0][k] = nx[idx];
                s_v[1][k] = nx[cap + idx];
            }
        }
    }
    __syncthreads();
    if (s_ok && tid == 0) {                                 // cumulative chord length, normalised (FITPACK parcur)
        s_u[0] = 0.;
        bool good = true;
        for (int k = 1; k < m; ++k) {
            const double dx = s_v[0][k] - s_v[0][k - 1], dy = s_v[1][k] - s_v[1][k - 1];
            const double h = sqrt(dx * dx + dy * dy);
            good = good && h > 0.;                          // a repeated vertex: splprep raises
            s_u[k] = s_u[k - 1] + h;
        }
        const double total = s_u[m - 1];
        good = good && total > 0. && total < INFINITY;
        if (good) {
            for (int k = 1; k < m; ++k) s_u[k] = s_u[k] / total;
            for (int k = 1; k < m; ++k) good = good && s_u[k] > s_u[k - 1];
        }
        if (!good) s_ok = 0;
    }
    __syncthreads();
    if (s_ok && tid < 2) {                                  // Thomas on M[1 .. m - 2]; the not-a-knot rows are diagonally dominant
        const double* y = s_v[tid];
        double* M = s_M[tid];
        double* cp = s_w[tid];
        double prev_cp = 0., prev_dp = 0.;
        for (int i = 1; i <= m - 2; ++i) {
            const double hl = s_u[i] - s_u[i - 1], hr = s_u[i + 1] - s_u[i];
            double a = hl, bb = 2. * (hl + hr), c = hr;
            if (i == 1) {
                a = 0.;
                bb = 3. * hl + 2. * hr + hl * hl / hr;
                c = hr - hl * hl / hr;
            }
            if (i == m - 2) {                               // (m >= 4: never the row above)
                bb = 3. * hr + 2. * hl + hr * hr / hl;
                a = hl - hr * hr / hl;
                c = 0.;
            }
            const double r = 6. * ((y[i + 1] - y[i]) / hr - (y[i] - y[i - 1]) / hl);
            const double den = bb - a * prev_cp;
            prev_cp = c / den;
            prev_dp = (r - a * prev_dp) / den;
            cp[i] = prev_cp;
            M[i] = prev_dp;
        }
        for (int i = m - 3; i >= 1; --i) M[i] = M[i] - cp[i] * M[i + 1];
        const double h0 = s_u[1] - s_u[0], h1 = s_u[2] - s_u[1];
        const double hL = s_u[m - 1] - s_u[m - 2], hp = s_u[m - 2] - s_u[m - 3];
        M[0] = (1. + h0 / h1) * M[1] - (h0 / h1) * M[2];
        M[m - 1] = (1. + hL / hp) * M[m - 2] - (hL / hp) * M[m - 3];
    }
    __syncthreads();
    const int okv = s_ok;
    if (tid == 0) ok_out[b] = okv;
    double* pl = plan + (size_t)b * T * 2;
    double* ex = s_w[0];                                    // the plan, kept for the differences (the solve is done with s_w)
    double* ey = s_w[1];
    __syncthreads();
    for (int k = tid; k < T; k += 128) {
        double x = 0., y = 0.;
        if (okv && k < ns) {
            const double t = k == ns - 1 ? 1.0 : (double)k * (1.0 / (double)(ns - 1));           // numpy.linspace(0, 1, ns)
            int lo = 0, hi = m - 2;                         // the last i with u[i] <= t (the last interval at t = 1)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_u[mid] <= t) lo = mid; else hi = mid - 1;
            }
            const double h = s_u[lo + 1] - s_u[lo], A = s_u[lo + 1] - t, Bq = t - s_u[lo];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double Ml = s_M[c][lo], Mr = s_M[c][lo + 1], yl = s_v[c][lo], yr = s_v[c][lo + 1];
                const double val = Ml * (A * A * A) / (6. * h) + Mr * (Bq * Bq * Bq) / (6. * h) + (yl / h - Ml * h / 6.) * A +
                                   (yr / h - Mr * h / 6.) * Bq;
                if (c == 0) x = val; else y = val;
            }
        }
        pl[2 * k] = x;
        pl[2 * k + 1] = y;
        if (k < GCPX_PRM_MAX_PATH) {
            ex[k] = x * 27.0;                               // the environment's units: 27 (x, -y)
            ey[k] = (y * -1.0) * 27.0;
        }
    }
    __syncthreads();
    if (!states) return;
    // the recorded episode: ns plan states and the state after the zero action of the `done` step; actions = differences, then zero
    const float gx = (float)(start_goal[4 * b + 2] * 27.0), gy = (float)((start_goal[4 * b + 3] * -1.0) * 27.0);
    for (int k = tid; k <= T; k += 128) {
        float* st = states + ((size_t)b * (T + 1) + k) * 5;
        const bool live = okv && k <= ns;
        const int kk = min(k, ns - 1);
        float sx = 0.f, sy = 0.f, hd = 0.f;
        if (live) {
            sx = (float)ex[kk];
            sy = (float)ey[kk];
            const int k0 = min(kk, ns - 2);                 // heading: the direction of the step taken from this state (the last one repeats)
            hd = (float)atan2(ey[k0 + 1] - ey[k0], ex[k0 + 1] - ex[k0]);
        }
        st[0] = sx;
        st[1] = sy;
        st[2] = hd;
        st[3] = live ? gx : 0.f;
        st[4] = live ? gy : 0.f;
        pad_mask[(size_t)b * (T + 1) + k] = live ? 1.f : 0.f;
        if (k < T) {
            float* ac = actions + ((size_t)b * T + k) * 2;
            const bool step = okv && k < ns - 1;
            ac[0] = step ? (float)(ex[k + 1] - ex[k]) : 0.f;
            ac[1] = step ? (float)(ey[k + 1] - ey[k]) : 0.f;
        }
    }
}

}  // namespace

extern "C" int gcpx_prm_sample_points(const double* boxes, int32_t n_boxes, const int32_t* pt_box, const int32_t* pt_off,
                                      const int64_t* traj_key, const int32_t* draw0, int32_t B, int32_t total_pts, int32_t max_pts,
                                      int64_t seed, double* px, double* py, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(boxes && pt_box && pt_off && traj_key && draw0 && px && py, "null pointer");
    GCPX_CHECK_ARG(n_boxes > 0 && B > 0 && B <= 65535, "n_boxes > 0, B: 1 .. 65535");
    GCPX_CHECK_ARG(total_pts > 0 && max_pts > 0 && max_pts <= total_pts, "0 < max_pts <= total_pts");
    hipLaunchKernelGGL(prm_sample_kernel, dim3((unsigned)((max_pts + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, stream,
                       boxes, n_boxes, pt_box, pt_off, traj_key, draw0, total_pts, (uint64_t)seed, px, py);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_prm_roadmap(const double* obs_x, const double* obs_y, const int32_t* cell_start, int32_t n_obs, int32_t grid_x,
                                int32_t grid_y, double grid_x0, double grid_y0, double cell, const double* px, const double* py,
                                const int32_t* pt_off, const double* start_goal, int32_t B, int32_t total_pts, int32_t max_pts,
                                int32_t cap, int32_t n_knn, double rr, double max_edge_len, uint8_t* kept, int32_t* n_nodes,
                                double* node_xy, int32_t* adj, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(obs_x && obs_y && cell_start && px && py && pt_off && start_goal && kept && n_nodes && node_xy && adj, "null pointer");
    GCPX_CHECK_ARG(n_obs > 0 && grid_x > 0 && grid_y > 0 && (int64_t)grid_x * grid_y < (1 << 24), "bad obstacle grid sizes");
    GCPX_CHECK_ARG(rr > 0. && cell > rr, "the grid's cell must be larger than the robot radius rr > 0");
    GCPX_CHECK_ARG(max_edge_len > 0. && max_edge_len / rr <= (double)GCPX_PRM_MAX_EDGE_STEPS, "max_edge_len / rr: (0, 4096]");
    GCPX_CHECK_ARG(B > 0 && total_pts > 0 && max_pts > 0 && max_pts <= total_pts, "B > 0, 0 < max_pts <= total_pts");
    GCPX_CHECK_ARG(cap >= max_pts + 2 && cap <= GCPX_PRM_MAX_NODES, "cap: max_pts + 2 .. GCPX_PRM_MAX_NODES");
    GCPX_CHECK_ARG(n_knn > 0 && n_knn <= GCPX_PRM_MAX_KNN, "n_knn: 1 .. GCPX_PRM_MAX_KNN");
    ObsGrid g{obs_x, obs_y, cell_start, n_obs, grid_x, grid_y, grid_x0, grid_y0, cell};
    hipLaunchKernelGGL(prm_roadmap_kernel, dim3((unsigned)B), dim3(kThreads), 0, stream, g, px, py, pt_off, start_goal, total_pts, max_pts,
                       cap, n_knn, rr, max_edge_len, kept, n_nodes, node_xy, adj);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_prm_shortest_path(const double* node_xy, const int32_t* n_nodes, const int32_t* adj, int32_t B, int32_t cap,
                                      int32_t n_knn, double cost_power, int32_t* success, int32_t* n_vert, int32_t* path, double* cost,
                                      void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(node_xy && n_nodes && adj && success && n_vert && path && cost, "null pointer");
    GCPX_CHECK_ARG(B > 0 && cap >= 2 && cap <= GCPX_PRM_MAX_NODES, "B > 0, cap: 2 .. GCPX_PRM_MAX_NODES");
    GCPX_CHECK_ARG(n_knn > 0 && n_knn <= GCPX_PRM_MAX_KNN, "n_knn: 1 .. GCPX_PRM_MAX_KNN");
    GCPX_CHECK_ARG(cost_power > 0. && cost_power <= 16., "cost_power: (0, 16]");
    hipLaunchKernelGGL(prm_path_kernel, dim3((unsigned)B), dim3(kThreads), 0, stream, node_xy, n_nodes, adj, cap, n_knn, cost_power,
                       success, n_vert, path, cost);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_prm_resample(const double* node_xy, const int32_t* n_nodes, const int32_t* path, const int32_t* n_vert,
                                 const int32_t* n_steps, const double* start_goal, int32_t B, int32_t cap, int32_t T, double* plan,
                                 int32_t* ok, float* states, float* actions, float* pad_mask, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(node_xy && n_nodes && path && n_vert && n_steps && plan && ok, "null pointer");
    GCPX_CHECK_ARG(B > 0 && cap >= 4 && cap <= GCPX_PRM_MAX_NODES, "B > 0, cap: 4 .. GCPX_PRM_MAX_NODES");
    GCPX_CHECK_ARG(T >= 2 && T <= GCPX_PRM_MAX_PATH, "T: 2 .. GCPX_PRM_MAX_PATH");
    GCPX_CHECK_ARG((!states && !actions && !pad_mask) || (states && actions && pad_mask && start_goal),
                   "states, actions, pad_mask and start_goal come together or not at all");
    hipLaunchKernelGGL(prm_resample_kernel, dim3((unsigned)B), dim3(128), 0, stream, node_xy, n_nodes, path, n_vert, n_steps, start_goal,
                       cap, T, plan, ok, states, actions, pad_mask);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
