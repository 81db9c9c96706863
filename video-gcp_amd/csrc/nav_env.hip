// The maze environment of the control experiments: E independent episodes advanced by one step per launch, on the device.  The batched
// counterpart of TopdownMultiroom3dEnv.step / BaseMiniworldEnv.eval as GeneralAgent.rollout drives them (one episode at a time, on the
// host, in the reference).  gym-miniworld is absent, so the dynamics are this build's own; the written spec is at
// gcpx_nav_env_* in include/gcpx.h and its definition is the numpy restatement nav_env.step_numpy / nav_env.goal_dist_numpy.
//
//   gcpx_nav_env_reset   row 0 of the record: the start state, its distance to the goal and its pixel; path lengths zeroed
//   gcpx_nav_env_step    p' = p + a (one float32 add per coordinate); the move is rejected whole when the closed segment [p, p'] comes
//                        within the robot radius of a wall segment; heading, path length, goal distance and pixel of the new state
//
// One thread per episode: an episode tests ~30 (9 rooms) to ~100 (25 rooms) wall segments, which the workgroup stages in LDS once, and E
// is of the order of 100 -- the launch is latency, not throughput.  All geometry is float64 with nothing contracted into an FMA: the
// decisions are threshold tests on sums of products, which the numpy restatement evaluates in the same order, so both agree bit for bit.
// Every index read from a state is clamped before it addresses a table.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 64;

// squared distance from q to the closed segment [a, b]
__device__ __forceinline__ double point_segment_d2(const double qx, const double qy, const double ax, const double ay, const double bx,
                                                   const double by) {
    const double dx = bx - ax, dy = by - ay;
    const double l2 = dx * dx + dy * dy;
    double t = 0.;
    if (l2 > 0.) t = fmin(fmax(((qx - ax) * dx + (qy - ay) * dy) / l2, 0.), 1.);
    const double ex = qx - (ax + t * dx), ey = qy - (ay + t * dy);
    return ex * ex + ey * ey;
}

// squared distance between the closed segments [p, q] and [a, b]: 0 when they cross properly, else the least of the four end-point
// distances (segments that touch or overlap have an end point at distance 0)
__device__ __forceinline__ double segment_segment_d2(const double px, const double py, const double qx, const double qy, const double ax,
                                                     const double ay, const double bx, const double by) {
    const double ux = qx - px, uy = qy - py, vx = bx - ax, vy = by - ay;
    const double o1 = ux * (ay - py) - uy * (ax - px), o2 = ux * (by - py) - uy * (bx - px);
    const double o3 = vx * (py - ay) - vy * (px - ax), o4 = vx * (qy - ay) - vy * (qx - ax);
    const bool split_ab = (o1 > 0. && o2 < 0.) || (o1 < 0. && o2 > 0.);
    const bool split_pq = (o3 > 0. && o4 < 0.) || (o3 < 0. && o4 > 0.);
    if (split_ab && split_pq) return 0.;
    const double d0 = point_segment_d2(px, py, ax, ay, bx, by), d1 = point_segment_d2(qx, qy, ax, ay, bx, by);
    const double d2 = point_segment_d2(ax, ay, px, py, qx, qy), d3 = point_segment_d2(bx, by, px, py, qx, qy);
    return fmin(fmin(d0, d1), fmin(d2, d3));
}

struct Maze {
    int rps;                          // rooms per side
    double table_size;                // ROOM_SIZE * rps, as nav_layout computes it
    float half_table, render_scale;   // topdown_pixels' float32 constants
    int S, cw;
};

// comp_shortest_dist from a position in table coordinates: nav_env.goal_dist_numpy
__device__ __forceinline__ double goal_distance(const Maze& m, const double* __restrict__ tab, const double x, const double y) {
    if (!(x >= -0.5 && x <= 0.5 && y >= -0.5 && y <= 0.5)) return 10.;
    const double room = 1. / 3.;
    const double last = (double)(m.rps - 1);
    const double xr = fmin(fmax(floor((x + m.table_size / 2.) / room), 0.), last);
    const double yr = fmin(fmax(floor((y + m.table_size / 2.) / room), 0.), last);
    const int r = (int)xr * m.rps + (m.rps - 1) - (int)yr;
    const double dx = x - tab[3 * r], dy = y - tab[3 * r + 1], rest = tab[3 * r + 2];
    if (rest != rest) return 10.;     // the goal lies outside [-0.5, 0.5]
    const double d = sqrt(dx * dx + dy * dy);
    return rest < 0. ? d : d + rest;
}

// dataset.topdown_pixels for one state, in float32
__device__ __forceinline__ void pixel_of(const Maze& m, const float sx, const float sy, int32_t* __restrict__ out) {
    const float qx = sx / 27.0f + m.half_table, qy = (sy * -1.0f) / 27.0f + m.half_table;
    const float vx = truncf(qx * m.render_scale), vy = truncf(qy * m.render_scale);
    const double lim = 2147483647.;
    // a NaN or a value past int64 has no defined conversion in numpy either: such a state is painted nowhere (the renderer clamps)
    const double ox = vx == vx ? (double)vx + (double)m.cw : -lim - 1., oy = vy == vy ? (double)(m.S + m.cw) - (double)vy : -lim - 1.;
    out[0] = (int32_t)fmin(fmax(ox, -lim - 1.), lim);
    out[1] = (int32_t)fmin(fmax(oy, -lim - 1.), lim);
}

__global__ void __launch_bounds__(kThreads) nav_env_reset_kernel(const float* __restrict__ state, const double* __restrict__ goal_table,
                                                                 const Maze m, const int E, const int T, float* __restrict__ full_traj,
                                                                 double* __restrict__ path_len, double* __restrict__ goal_dist,
                                                                 int32_t* __restrict__ pix) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const float sx = state[3 * e], sy = state[3 * e + 1], sh = state[3 * e + 2];
    float* row = full_traj + (size_t)e * (T + 1) * 3;
    row[0] = sx;
    row[1] = sy;
    row[2] = sh;
    path_len[e] = 0.;
    goal_dist[(size_t)e * (T + 1)] = goal_distance(m, goal_table + (size_t)e * m.rps * m.rps * 3, (double)sx / 27., ((double)sy / 27.) * -1.);
    pixel_of(m, sx, sy, pix + 2 * e);
}

__global__ void __launch_bounds__(kThreads) nav_env_step_kernel(float* __restrict__ state, const float* __restrict__ action,
                                                                const double* __restrict__ walls, const int n_walls, const double radius,
                                                                const double* __restrict__ goal_table, const Maze m, const int E,
                                                                const int T, const int t, float* __restrict__ full_traj,
                                                                double* __restrict__ path_len, double* __restrict__ goal_dist,
                                                                uint8_t* __restrict__ blocked, int32_t* __restrict__ pix) {
    __shared__ double s_walls[GCPX_NAV_MAX_WALLS * 4];
    for (int i = threadIdx.x; i < 4 * n_walls; i += kThreads) s_walls[i] = walls[i];
    __syncthreads();
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const float sx = state[3 * e], sy = state[3 * e + 1], sh = state[3 * e + 2];
    const float ax = action[2 * e], ay = action[2 * e + 1];
    const float nx = sx + ax, ny = sy + ay;                 // the proposed state: one float32 add per coordinate
    bool hit = false;
    const bool moves = !(ax == 0.f && ay == 0.f);           // a zero action is free and keeps the heading
    if (moves) {
        hit = !(isfinite(nx) && isfinite(ny));              // a NaN or an overflow moves nowhere
        const double px = (double)sx / 27., py = ((double)sy / 27.) * -1.;
        const double qx = (double)nx / 27., qy = ((double)ny / 27.) * -1.;
        const double r2 = radius * radius;
        for (int k = 0; k < n_walls && !hit; ++k) {
            const double d2 = segment_segment_d2(px, py, qx, qy, s_walls[4 * k], s_walls[4 * k + 1], s_walls[4 * k + 2], s_walls[4 * k + 3]);
            hit = !(d2 > r2);
        }
    }
    float ox = sx, oy = sy, oh = sh;
    double len = 0.;
    if (moves && !hit) {
        const double dx = (double)nx - (double)sx, dy = (double)ny - (double)sy;
        ox = nx;
        oy = ny;
        oh = (float)atan2(dy, dx);
        len = sqrt(dx * dx + dy * dy);
    }
    state[3 * e] = ox;
    state[3 * e + 1] = oy;
    state[3 * e + 2] = oh;
    float* row = full_traj + ((size_t)e * (T + 1) + t + 1) * 3;
    row[0] = ox;
    row[1] = oy;
    row[2] = oh;
    blocked[(size_t)e * T + t] = hit ? 1 : 0;
    path_len[e] = path_len[e] + len;
    goal_dist[(size_t)e * (T + 1) + t + 1] =
        goal_distance(m, goal_table + (size_t)e * m.rps * m.rps * 3, (double)ox / 27., ((double)oy / 27.) * -1.);
    pixel_of(m, ox, oy, pix + 2 * e);
}

}  // namespace

extern "C" int gcpx_nav_env_reset(const float* state, const double* goal_table, int32_t rooms_per_side, double table_size, int32_t E, int32_t T,
                                  float half_table, float render_scale, int32_t S, int32_t cw, float* full_traj, double* path_len,
                                  double* goal_dist, int32_t* pix, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(state && goal_table && full_traj && path_len && goal_dist && pix, "null pointer");
    GCPX_CHECK_ARG(E >= 1 && E <= (1 << 20) && T >= 1 && T <= (1 << 20), "E, T: 1 .. 2^20");
    GCPX_CHECK_ARG(rooms_per_side >= 1 && rooms_per_side <= GCPX_NAV_MAX_ROOMS_PER_SIDE, "rooms_per_side: 1 .. GCPX_NAV_MAX_ROOMS_PER_SIDE");
    GCPX_CHECK_ARG(table_size > 0. && S > 0 && cw >= 0 && S <= 16384 && cw <= 16384, "table_size > 0, S: 1 .. 16384, cw: 0 .. 16384");
    const Maze m{rooms_per_side, table_size, half_table, render_scale, S, cw};
    hipLaunchKernelGGL(nav_env_reset_kernel, dim3((unsigned)((E + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, state, goal_table, m,
                       E, T, full_traj, path_len, goal_dist, pix);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_nav_env_step(float* state, const float* action, const double* walls, int32_t n_walls, double radius,
                                 const double* goal_table, int32_t rooms_per_side, double table_size, int32_t E, int32_t T, int32_t t,
                                 float half_table, float render_scale, int32_t S, int32_t cw, float* full_traj, double* path_len,
                                 double* goal_dist, uint8_t* blocked, int32_t* pix, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(state && action && walls && goal_table && full_traj && path_len && goal_dist && blocked && pix, "null pointer");
    GCPX_CHECK_ARG(E >= 1 && E <= (1 << 20) && T >= 1 && T <= (1 << 20), "E, T: 1 .. 2^20");
    GCPX_CHECK_ARG(t >= 0 && t < T, "t: 0 .. T - 1");
    GCPX_CHECK_ARG(n_walls >= 1 && n_walls <= GCPX_NAV_MAX_WALLS, "n_walls: 1 .. GCPX_NAV_MAX_WALLS");
    GCPX_CHECK_ARG(radius >= 0. && radius < INFINITY, "radius: finite, >= 0");
    GCPX_CHECK_ARG(rooms_per_side >= 1 && rooms_per_side <= GCPX_NAV_MAX_ROOMS_PER_SIDE, "rooms_per_side: 1 .. GCPX_NAV_MAX_ROOMS_PER_SIDE");
    GCPX_CHECK_ARG(table_size > 0. && S > 0 && cw >= 0 && S <= 16384 && cw <= 16384, "table_size > 0, S: 1 .. 16384, cw: 0 .. 16384");
    const Maze m{rooms_per_side, table_size, half_table, render_scale, S, cw};
    hipLaunchKernelGGL(nav_env_step_kernel, dim3((unsigned)((E + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, state, action, walls,
                       n_walls, radius, goal_table, m, E, T, t, full_traj, path_len, goal_dist, blocked, pix);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
