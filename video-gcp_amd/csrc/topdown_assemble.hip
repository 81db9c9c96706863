// Batch assembly for the nav datasets (MazeTopRenderedGlobalSplitVarLenVideoDataset, data_loader.py:299-319): every frame is a top-down
// picture of the maze drawn from the trajectory's states (multiroom3d_env.py:185-219), not a recorded image.  The host sends, per window
// frame, the agent's pixel in the padded static picture and, per sequence, the goal's (dataset.topdown_pixels); the picture itself, the two
// dot stamps and the resize tables stay on the device.  Per output frame t <= end_ind (s = min(t + chop, T - 1), csrc/batch_assemble.hip):
//     window  = background[cy - cw : cy + cw, cx - cw : cx + cw],  (cx, cy) = (max(cw, x_s), max(cw, y_s))   -- the clamp moves the crop only
//     window[agent stamp around (x_s, y_s)] = agent colour;  window[goal stamp around goal] = goal colour    -- in this order: the goal wins
//     frame t = lut[resize(window, 2cw -> H x W)]                                                           -- the passes of resize_passes.h
// A stamp pixel is painted where it falls inside the window; the window lies inside the padded picture (the host raises before it sends a
// crop that does not), so what the picture's border would clip is clipped as well.  Integer work only.
//
// One workgroup = one band of R output rows of one frame, as in resize_assemble_frames_kernel: the band's source rows of the window are
// copied into LDS (a thread moves 16 bytes: a row starts at any byte of the picture, so the up to five aligned dwords around them are
// shifted together; consecutive lanes read consecutive bytes of a row), the stamps overwrite them there, then the two passes run.
#include "resize_passes.h"

using namespace gcpx_resize;

namespace {

constexpr int kStampMax = 31;
constexpr int kWindowMin = 4, kWindowMax = 128;

constexpr int kStampPerThread = (kStampMax * kStampMax + kThreads - 1) / kThreads;

// one pixel of the staged rows [y_lo, y_lo + nrows) of the window, given in window coordinates; outside them nothing is written
__device__ __forceinline__ void paint_pixel(uint8_t* __restrict__ raw, const int wx, const int wy, const uint32_t rgb, const int D,
                                            const int y_lo, const int nrows) {
    const int ry = wy - y_lo;
    if (wx < 0 || wx >= D || ry < 0 || ry >= nrows) return;
    uint8_t* p = raw + (ry * D + wx) * 3;
    p[0] = (uint8_t)(rgb & 255);
    p[1] = (uint8_t)((rgb >> 8) & 255);
    p[2] = (uint8_t)((rgb >> 16) & 255);
}

__global__ void __launch_bounds__(kThreads) topdown_assemble_frames_kernel(
    const uint8_t* __restrict__ bg, const int side, const long long bg_bytes, const int cw, const uint8_t* __restrict__ agent_stamp,
    const uint8_t* __restrict__ goal_stamp, const int k, const uint32_t agent_rgb, const uint32_t goal_rgb,
    const int32_t* __restrict__ coords, const int32_t* __restrict__ goal, const int32_t* __restrict__ info, const float* __restrict__ lut,
    const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, const int32_t* __restrict__ ky, const int32_t* __restrict__ by,
    const int T, const int H, const int W, const int ksx, const int ksy, const int R, const int cap, float* __restrict__ traj,
    float* __restrict__ I0, float* __restrict__ Ig) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int D = 2 * cw;                         // the window's side: the resampler's Hs = Ws
    const ResizeLds L = resize_lds(D, W, ksx, ksy, R, cap);
    float* tab = reinterpret_cast<float*>(smem);
    int32_t* skx = reinterpret_cast<int32_t*>(smem) + 256;
    int32_t* sbx = skx + W * ksx;
    int32_t* sky = sbx + 2 * W;
    int32_t* sby = sky + R * ksy;
    uint8_t* raw = smem + L.raw_off;
    uint8_t* hres = smem + L.hres_off;
    const int tid = threadIdx.x;
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const int r0 = blockIdx.y * R, nr = min(R, H - r0);
    const int32_t* in = info + (size_t)b * kInfo;
    const int n_frames = min(in[0], T), chop = max(in[3], 0), zero_from = in[4], end_ind = in[5];
    const int s = min(t + chop, T - 1);
    const bool valid = t <= end_ind && t < zero_from && s < n_frames;     // only frames up to end_ind are rendered
    const int HW = H * W, W4 = W >> 2;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW + (size_t)r0 * W;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    float* dg = t == end_ind ? Ig + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    tab[tid] = lut[tid];
    if (!valid) {                                 // past end_ind the reference's frames are uint8 zeros: lut[0], nothing read
        store_pad_band(lut[0], nr, W4, HW, dst, d0, dg, tid);
        return;
    }
    for (int i = tid; i < W * ksx; i += kThreads) skx[i] = kx[i];
    for (int i = tid; i < 2 * W; i += kThreads) sbx[i] = bx[i];
    for (int i = tid; i < nr * ksy; i += kThreads) sky[i] = ky[r0 * ksy + i];
    for (int i = tid; i < 2 * nr; i += kThreads) sby[i] = by[2 * r0 + i];
    // the band's rows [y_lo, y_lo + nrows) of the window
    const int y_lo = min(max(by[2 * r0], 0), D - 1);
    const int nrows = min(min(max(by[2 * (r0 + nr - 1)] + by[2 * (r0 + nr - 1) + 1], y_lo + 1), D) - y_lo, cap);
    // a dot further than a stamp away from the picture paints nothing: bounding it keeps the index arithmetic inside int32
    const int32_t* xy = coords + ((size_t)b * T + s) * 2;
    const int ax = min(max(xy[0], -kStampMax), side + kStampMax), ay = min(max(xy[1], -kStampMax), side + kStampMax);
    const int gx = min(max(goal[2 * b], -kStampMax), side + kStampMax), gy = min(max(goal[2 * b + 1], -kStampMax), side + kStampMax);
    // first pixel of the crop (the upper clamp never acts on what the host sends: it keeps every read inside the picture)
    const int lx = min(max(ax, cw), side - cw) - cw, ly = min(max(ay, cw), side - cw) - cw;
    // this thread's entries of both stamps (entry tid + 256 j is bit j), in flight with the copy below
    uint32_t abits = 0, gbits = 0;
#pragma unroll
    for (int j = 0; j < kStampPerThread; ++j) {
        const int i = tid + j * kThreads;
        if (i < k * k) {
            abits |= (uint32_t)(agent_stamp[i] != 0) << j;
            gbits |= (uint32_t)(goal_stamp[i] != 0) << j;
        }
    }
    // the copy: a thread moves 16 bytes of the staged rows at a time, out of the up to five dwords of the picture that hold them
    const int rb = D * 3, nbytes = nrows * rb;
    {
        const long long row0 = ((long long)(ly + y_lo) * side + lx) * 3, pitch = (long long)side * 3;
        const int dr = (16 * kThreads) / rb, dc = 16 * kThreads - dr * rb;       // a step of 256 chunks in (row, byte of the row)
        int r = (16 * tid) / rb, c = 16 * tid - r * rb;
        for (int i = tid; i < (nbytes + 15) >> 4; i += kThreads) {
            const long long g = row0 + r * pitch + c;
            const int sh = (int)(g & 3);
            uint32_t w[4] = {0, 0, 0, 0};
            if (c + 16 <= rb && g - sh + (sh ? 20 : 16) <= bg_bytes) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(bg + (g - sh));
                uint32_t d[5] = {p[0], p[1], p[2], p[3], 0u};
                if (sh) d[4] = p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (uint32_t)sh);
            } else {                              // a chunk across rows of the window, or the last bytes of the picture
                for (int j = 0; j < 16 && 16 * i + j < nbytes; ++j) {
                    const int rj = (16 * i + j) / rb, cj = 16 * i + j - rj * rb;
                    w[j >> 2] |= (uint32_t)bg[row0 + rj * pitch + cj] << (8 * (j & 3));
                }
            }
            *reinterpret_cast<uint4*>(raw + 16 * i) = make_uint4(w[0], w[1], w[2], w[3]);
            r += dr;
            c += dc;
            if (c >= rb) {
                c -= rb;
                ++r;
            }
        }
    }
    __syncthreads();
    // the dots, in one pass: the goal is painted after the agent in the reference and wins where they overlap, so an entry of the
    // agent's stamp that the goal's stamp covers is left to the goal's entry (no two threads write one pixel)
    {
        const int h = k >> 1;
#pragma unroll
        for (int j = 0; j < kStampPerThread; ++j) {
            const int i = tid + j * kThreads;
            if (i >= k * k) break;
            const int dy = i / k, dx = i - dy * k;
            if ((gbits >> j) & 1) paint_pixel(raw, gx + dx - h - lx, gy + dy - h - ly, goal_rgb, D, y_lo, nrows);
            if ((abits >> j) & 1) {
                const int px = ax + dx - h, py = ay + dy - h;                    // in the picture
                const int ex = px - gx + h, ey = py - gy + h;                    // in the goal's stamp
                const bool covered = ex >= 0 && ex < k && ey >= 0 && ey < k && goal_stamp[ey * k + ex] != 0;
                if (!covered) paint_pixel(raw, px - lx, py - ly, agent_rgb, D, y_lo, nrows);
            }
        }
    }
    __syncthreads();
    resize_rows_any(ksx, raw, 0, hres, skx, sbx, nrows, D, W, tid);
    __syncthreads();
    resize_cols_store(hres, sky, sby, tab, y_lo, nrows, nr, W, ksy, HW, dst, d0, dg, tid);
}

}  // namespace

extern "C" int gcpx_topdown_assemble_batch(const uint8_t* background, int32_t side, int32_t cw, const uint8_t* agent_stamp,
                                           const uint8_t* goal_stamp, int32_t k, int32_t agent_rgb, int32_t goal_rgb, const int32_t* coords,
                                           const int32_t* goal, const int32_t* info, const float* lut, const int32_t* kx, const int32_t* bx,
                                           const int32_t* ky, const int32_t* by, const float* pad_in, const float* states_in,
                                           const float* actions_in, const float* states_mean, const float* states_den, int32_t B, int32_t T,
                                           int32_t H, int32_t W, int32_t ksx, int32_t ksy, int32_t state_dim, int32_t n_actions,
                                           float* traj_seq, float* I_0, float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind,
                                           float* states, float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(background && agent_stamp && goal_stamp && coords && goal, "null background / stamp / coordinate pointer");
    GCPX_CHECK_ARG(info && lut && pad_in && traj_seq && I_0 && I_g && pad_mask && end_ind && start_ind, "null pointer");
    GCPX_CHECK_ARG(kx && bx && ky && by, "null coefficient / bounds table");
    GCPX_CHECK_ARG(B > 0 && T > 1 && state_dim >= 0 && n_actions >= 0, "bad sizes");
    GCPX_CHECK_ARG(cw > 0 && 2 * cw >= kWindowMin && 2 * cw <= kWindowMax, "the window side 2 * cw must be in [4, 128]");
    const int D = 2 * cw;
    GCPX_CHECK_ARG(side >= D && side <= 16384, "the background's side must be in [2 * cw, 16384]");
    GCPX_CHECK_ARG(k > 0 && (k & 1) == 1 && k <= kStampMax, "the stamp side k must be odd and at most 31");
    GCPX_CHECK_ARG(H > 0 && W > 0 && H <= kResizeMaxSide && W <= kResizeMaxSide, "output sides must be in [1, 512]");
    GCPX_CHECK_ARG((W & 3) == 0, "output width must be a multiple of 4");
    GCPX_CHECK_ARG(D <= kResizeMaxScale * H && D <= kResizeMaxScale * W, "down-scaling by more than 8 is not supported");
    GCPX_CHECK_ARG(ksx == resize_ksize(D, W) && ksy == resize_ksize(D, H), "ksx / ksy are not the tap counts of these sizes");
    GCPX_CHECK_ARG(state_dim == 0 || (states_in && states), "states_in / states null with state_dim > 0");
    GCPX_CHECK_ARG(n_actions == 0 || (actions_in && actions), "actions_in / actions null with n_actions > 0");
    GCPX_CHECK_ARG(!states_mean == !states_den, "states_mean and states_den go together");
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(background) & 3) == 0, "background not 4-byte aligned");
    GCPX_CHECK_ARG(((reinterpret_cast<uintptr_t>(traj_seq) | reinterpret_cast<uintptr_t>(I_0) | reinterpret_cast<uintptr_t>(I_g)) & 15) == 0,
                   "outputs not 16-byte aligned");
    int cap = 0;
    ResizeLds L{};
    const int R = resize_choose_band(D, D, H, W, ksx, ksy, &cap, &L);
    GCPX_CHECK_ARG(R > 0, "one output row's source rows do not fit the LDS");
    const long long bg_bytes = (long long)side * side * 3;
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(topdown_assemble_frames_kernel, grid, dim3(kThreads), (size_t)L.total, stream, background, side, bg_bytes, cw,
                       agent_stamp, goal_stamp, k, (uint32_t)agent_rgb, (uint32_t)goal_rgb, coords, goal, info, lut, kx, bx, ky, by, T, H, W,
                       ksx, ksy, R, cap, traj_seq, I_0, I_g);
    launch_assemble_small(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask, end_ind,
                          start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
