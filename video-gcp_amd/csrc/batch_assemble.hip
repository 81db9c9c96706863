// Batch assembly of the data paths (video-gcp_amd/dataset.py, dataset_resident.py): uint8 frames plus a few integers per sequence -> the
// model's f32 inputs, written in place into the persistent buffers its launch plans read.  Three ideas, each written once:
//   the frames of a batch at the model's size    (assemble_frames_kernel),
//   the frames resized on the way                (resize_assemble_frames_kernel; topdown_assemble_frames_kernel renders them first),
//   pad mask, indices, states and actions        (assemble_small_kernel),
// over a sequence source (SlotSrc, ResidentSrc) that says where frame s of sequence b lives.
//
// The host mirrors the reference's per-item index logic (data_loader.py:131-211).  For output frame t (randomize_length's chop and
// repeat of the last frame, data_loader.py:191-211):
//     s = min(t + chop, T - 1);  value = (t < zero_from && s < n_frames) ? lut[raw[s]] : lut[0]
// lut is the 256-entry table of `np.arange(256, dtype=np.uint8).astype(np.float32) / 255 * 2 - 1` built on the host, so the values
// are the reference's bit for bit whatever the compiler flags; padded frames are uint8 0 in the reference and so become -1.0.
//
// SlotSrc (gcpx_assemble_batch, gcpx_resize_assemble_batch, gcpx_topdown_assemble_batch): the host uploads, per sequence, the frame
// window raw[offset : offset + T] (n_frames of them, the rest of the slot undefined) as row b of frames [B][T][H][W][3], the matching
// state / action windows and int32 info[8] = n_frames, n_states, n_actions, chop, zero_from, end_ind, -, -.
//
// ResidentSrc (gcpx_assemble_batch_resident, gcpx_resize_assemble_batch_resident): the frames of a whole split stay in HBM, all
// trajectories back to back, states and actions likewise rows of two resident f32 arrays; int64 info[8] per sequence (include/gcpx.h
// fixes the layout):
//     0 first frame of the window in the store      1 n_frames available from there within the trajectory
//     2 first state row                             3 n_states
//     4 first action row                            5 n_actions
//     6 chop                                        7 zero_from | end_ind << 32
// Addressing into the store is 64-bit.  A frame is read only when the time map says it is the sequence's own (s < n_frames: the bytes
// behind a short trajectory belong to the next one) and when it lies inside the store (first >= 0, first + s < store frames), so
// integers that do not belong to the store give a padded frame, never a wild read; the 16-byte staging loads of the resize form stop
// at store_bytes.
//
// The resize forms: frames stored at Hs x Ws != H x W.  Between the time map and the table lookup every frame goes through the
// reference's resize (data_loader.py:213-220), which is Pillow's 8-bit bilinear Image.resize: a horizontal and a vertical pass of
// integer arithmetic, each rounding to uint8, over int32 coefficient tables the host builds once in float64 (dataset.resize_coeffs).
// Integer only here, so the pixels are Pillow's whatever the compiler flags.
// Limits (invalid argument otherwise): sides of source and output in [1, 512], W a multiple of 4, Hs / H and Ws / W at most 8 (no limit on
// up-sampling inside the side limits), tap counts equal to Pillow's for the sizes, 16-byte aligned frames and images.
//
// The top-down form (MazeTopRenderedGlobalSplitVarLenVideoDataset, data_loader.py:299-319): every frame is a picture of the maze drawn
// from the trajectory's states (multiroom3d_env.py:185-219), not a recorded image.  The host sends, per window frame, the agent's pixel in
// the padded static picture and, per sequence, the goal's (dataset.topdown_pixels); the picture itself, the two dot stamps and the resize
// tables stay on the device.  Per output frame t <= end_ind:
//     window  = background[cy - cw : cy + cw, cx - cw : cx + cw],  (cx, cy) = (max(cw, x_s), max(cw, y_s))   -- the clamp moves the crop only
//     window[agent stamp around (x_s, y_s)] = agent colour;  window[goal stamp around goal] = goal colour    -- in this order: the goal wins
//     frame t = lut[resize(window, 2cw -> H x W)]
// A stamp pixel is painted where it falls inside the window; the window lies inside the padded picture (the host raises before it sends a
// crop that does not), so what the picture's border would clip is clipped as well.  Integer work only.
#include "resize_passes.h"

using namespace gcpx_resize;   // kThreads, kInfo, the band, the two passes of the resampler and the choice of the band

namespace {

// ---- where the sequences of a batch live ----------------------------------------------------------------------------------------

// One sequence under the time map.  Window position s is frame first + s, state row srow + s and action row arow + s of the source's
// arrays (64-bit); the counts are clamped to the window.
struct Seq {
    long long first, srow, arow;
    int n_frames, n_states, n_actions, chop, zero_from, end_ind;
};

// The two sources, the kernels' template parameter: how sequence b is read from the batch's info, and whether window frame s of it lies
// inside a source of n_frames frames.  The arrays themselves stay plain __restrict__ kernel arguments: pointers handed over inside a
// struct cost the resize kernel 11 VGPRs and a wave per SIMD.

// an uploaded slot: sequence b is row b of frames [B][T], states [B][T][S] and actions [B][T - 1][A]; every row exists
struct SlotSrc {
    using info_t = int32_t;
    static __device__ __forceinline__ Seq seq(const info_t* __restrict__ info, const int b, const int T) {
        const info_t* in = info + (size_t)b * kInfo;
        return {(long long)b * T, (long long)b * T, (long long)b * (T - 1), min(in[0], T), min(in[1], T), min(in[2], T - 1), max(in[3], 0),
                in[4], in[5]};
    }
    static __device__ __forceinline__ bool holds(const Seq&, const int, const long long) { return true; }
};

// a resident store: the info names the rows; a negative state / action row gives zero rows
struct ResidentSrc {
    using info_t = int64_t;
    static __device__ __forceinline__ Seq seq(const info_t* __restrict__ info, const int b, const int T) {
        const info_t* in = info + (size_t)b * kInfoResident;
        const long long srow = in[2], arow = in[4];
        return {in[0], srow, arow, (int)min((long long)in[1], (long long)T), srow < 0 ? 0 : (int)min((long long)in[3], (long long)T),
                arow < 0 ? 0 : (int)min((long long)in[5], (long long)(T - 1)), max((int)in[6], 0), (int)(in[7] & 0xffffffffll),
                (int)(in[7] >> 32)};
    }
    static __device__ __forceinline__ bool holds(const Seq& q, const int s, const long long n_frames) {
        return q.first >= 0 && q.first < n_frames - s;
    }
};

// output frame t of the sequence shows window frame s; true when that frame is the sequence's own and lies inside the source
template <class Src>
__device__ __forceinline__ bool frame_valid(const Seq& q, const int t, const int s, const long long n_frames) {
    return t < q.zero_from && s < q.n_frames && Src::holds(q, s, n_frames);
}

// ---- frames at the model's size -------------------------------------------------------------------------------------------------

// one thread = four consecutive pixels of one frame: 12 bytes read, one float4 written to each of the three channel planes
template <class Src>
__global__ void __launch_bounds__(kThreads) assemble_frames_kernel(const uint8_t* __restrict__ frames, const long long n_frames,
                                                                  const typename Src::info_t* __restrict__ info,
                                                                  const float* __restrict__ lut, const int T, const int HW,
                                                                  float* __restrict__ traj, float* __restrict__ I0,
                                                                  float* __restrict__ Ig) {
    __shared__ float tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const Seq q = Src::seq(info, b, T);
    const int s = min(t + q.chop, T - 1);
    const bool valid = frame_valid<Src>(q, t, s, n_frames);
    const uint8_t* from = frames + (size_t)(valid ? q.first + s : 0) * HW * 3;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW : nullptr;
    float* dg = t == q.end_ind ? Ig + (size_t)b * 3 * HW : nullptr;
    const float pad = tab[0];
    const int p0 = (blockIdx.y * kThreads + threadIdx.x) * 4;
    if (p0 >= HW) return;
    lut_quad_store(from, valid, tab, pad, HW, p0, dst, d0, dg);
}

// ---- pad mask, indices, states, actions -----------------------------------------------------------------------------------------

// one workgroup per sequence: pad mask, end / start index, states (standardised) and actions under the same time map as the frames
// (actions have T - 1 steps: the reference pads them to T and drops the last, so their "last frame" is T - 2)
template <class Src>
__global__ void __launch_bounds__(kThreads) assemble_small_kernel(
    const typename Src::info_t* __restrict__ info, const float* __restrict__ pad_in, const float* __restrict__ states_in,
    const float* __restrict__ actions_in, const float* __restrict__ mean, const float* __restrict__ den, const int T, const int S,
    const int A, float* __restrict__ pad_mask, int64_t* __restrict__ end_ind, int64_t* __restrict__ start_ind, float* __restrict__ states,
    float* __restrict__ actions) {
    const int b = blockIdx.x;
    const Seq q = Src::seq(info, b, T);
    if (threadIdx.x == 0) {
        end_ind[b] = q.end_ind;
        start_ind[b] = 0;
    }
    for (int i = threadIdx.x; i < T; i += kThreads) pad_mask[(size_t)b * T + i] = pad_in[(size_t)b * T + i];
    for (int i = threadIdx.x; i < T * S; i += kThreads) {
        const int t = i / S, k = i - t * S, s = min(t + q.chop, T - 1);
        float x = (t < q.zero_from && s < q.n_states) ? states_in[(size_t)(q.srow + s) * S + k] : 0.f;
        if (mean) x = __fdiv_rn(__fsub_rn(x, mean[k]), den[k]);
        states[((size_t)b * T + t) * S + k] = x;
    }
    for (int i = threadIdx.x; i < (T - 1) * A; i += kThreads) {
        const int t = i / A, k = i - t * A, s = min(t + q.chop, T - 2);
        actions[((size_t)b * (T - 1) + t) * A + k] =
            (t < q.zero_from && s < q.n_actions) ? actions_in[(size_t)(q.arow + s) * A + k] : 0.f;
    }
}

// ---- resize + assembly ------------------------------------------------------------------------------------------------------------

// one workgroup = R output rows (a band) of one output frame.  The band's `nrows` <= cap source rows are one contiguous run of bytes:
// 16-byte loads into LDS, horizontal pass LDS -> LDS as bytes (resize_rows),
// vertical pass out of LDS (one thread: four output columns of one row = 12 bytes per tap), table lookup, float4 stores.
// Every table entry is clamped to what was staged, so tables that do not belong to the sizes give a wrong picture, never a wild access.
template <class Src>
__global__ void __launch_bounds__(kThreads) resize_assemble_frames_kernel(
    const uint8_t* __restrict__ frames, const long long bytes, const long long n_frames, const typename Src::info_t* __restrict__ info,
    const float* __restrict__ lut, const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, const int32_t* __restrict__ ky,
    const int32_t* __restrict__ by, const int T, const int Hs, const int Ws, const int H, const int W, const int ksx, const int ksy,
    const int R, const int cap, float* __restrict__ traj, float* __restrict__ I0, float* __restrict__ Ig) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const Seq q = Src::seq(info, b, T);
    const int s = min(t + q.chop, T - 1);
    ResizeBand d = resize_band(smem, Hs, Ws, H, W, ksx, ksy, R, cap, b, t, T, q.end_ind, traj, I0, Ig);
    if (!resize_band_tables(d, frame_valid<Src>(q, t, s, n_frames), lut, kx, bx, ky, by, tid)) return;
    // the band's source rows [y_lo, y_lo + nrows) of frame first + s, staged with the tables under one barrier; no load at or past `bytes`
    const int row_bytes = Ws * 3;
    const long long a0 = ((q.first + s) * Hs + d.y_lo) * row_bytes;
    const int shift = stage_bytes(frames, a0, d.nrows * row_bytes, bytes, d.raw, tid);
    resize_band_store(d, shift, tid);
}

// ---- top-down rendering + resize + assembly ---------------------------------------------------------------------------------------

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

// One workgroup = one band of R output rows of one frame, as in resize_assemble_frames_kernel: the band's source rows of the window are
// copied into LDS (a thread moves 16 bytes: a row starts at any byte of the picture, so the up to five aligned dwords around them are
// shifted together; consecutive lanes read consecutive bytes of a row), the stamps overwrite them there, then the two passes run.
// The time map is the slot's (SlotSrc); there are no frames.
__global__ void __launch_bounds__(kThreads) topdown_assemble_frames_kernel(
    const uint8_t* __restrict__ bg, const int side, const long long bg_bytes, const int cw, const uint8_t* __restrict__ agent_stamp,
    const uint8_t* __restrict__ goal_stamp, const int k, const uint32_t agent_rgb, const uint32_t goal_rgb,
    const int32_t* __restrict__ coords, const int32_t* __restrict__ goal, const int32_t* __restrict__ info, const float* __restrict__ lut,
    const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, const int32_t* __restrict__ ky, const int32_t* __restrict__ by,
    const int T, const int H, const int W, const int ksx, const int ksy, const int R, const int cap, float* __restrict__ traj,
    float* __restrict__ I0, float* __restrict__ Ig) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int D = 2 * cw;                         // the window's side: the resampler's Hs = Ws
    const int tid = threadIdx.x;
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const Seq q = SlotSrc::seq(info, b, T);
    const int s = min(t + q.chop, T - 1);
    ResizeBand d = resize_band(smem, D, D, H, W, ksx, ksy, R, cap, b, t, T, q.end_ind, traj, I0, Ig);
    // only frames up to end_ind are rendered: past it the reference's frames are uint8 zeros
    if (!resize_band_tables(d, t <= q.end_ind && frame_valid<SlotSrc>(q, t, s, 0), lut, kx, bx, ky, by, tid)) return;
    uint8_t* raw = d.raw;
    const int y_lo = d.y_lo, nrows = d.nrows;     // the band's rows [y_lo, y_lo + nrows) of the window
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
                uint32_t v[5] = {p[0], p[1], p[2], p[3], 0u};
                if (sh) v[4] = p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], (uint32_t)sh);
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
    resize_band_store(d, 0, tid);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

template <class Src>
void launch_small(hipStream_t stream, const typename Src::info_t* info, const float* pad_in, const float* states_in,
                  const float* actions_in, const float* mean, const float* den, const int B, const int T, const int S, const int A,
                  float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states, float* actions) {
    hipLaunchKernelGGL(assemble_small_kernel<Src>, dim3(B), dim3(kThreads), 0, stream, info, pad_in, S ? states_in : nullptr,
                       A ? actions_in : nullptr, mean, den, T, S, A, pad_mask, end_ind, start_ind, states, actions);
}

bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

// The checks the entry points share, over the argument names they share (info, lut, pad_in, B, T, state_dim, n_actions, states_mean /
// states_den and the outputs).  Macros: GCPX_CHECK_ARG reports __func__, which has to be the public function's name.
// every form: `src` the frame source (the picture for the top-down form), `st` / `ac` where states and actions are read
#define GCPX_CHECK_ASSEMBLE(src, st, ac)                                                                                                  \
    GCPX_CHECK_ARG(src && info && lut && pad_in && traj_seq && I_0 && I_g && pad_mask && end_ind && start_ind, "null pointer");           \
    GCPX_CHECK_ARG(B > 0 && T > 1 && state_dim >= 0 && n_actions >= 0, "bad sizes");                                                      \
    GCPX_CHECK_ARG(state_dim == 0 || (st && states), #st " / states null with state_dim > 0");                                            \
    GCPX_CHECK_ARG(n_actions == 0 || (ac && actions), #ac " / actions null with n_actions > 0");                                          \
    GCPX_CHECK_ARG(!states_mean == !states_den, "states_mean and states_den go together")
// the resizing forms, Hs x Ws -> H x W: tables, limits, tap counts
#define GCPX_CHECK_RESIZE(Hs, Ws)                                                                                                         \
    GCPX_CHECK_ARG(kx && bx && ky && by, "null coefficient / bounds table");                                                              \
    GCPX_CHECK_ARG(Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hs <= kResizeMaxSide && Ws <= kResizeMaxSide && H <= kResizeMaxSide &&           \
                       W <= kResizeMaxSide, "source and output sides must be in [1, 512]");                                               \
    GCPX_CHECK_ARG((W & 3) == 0, "output width must be a multiple of 4");                                                                 \
    GCPX_CHECK_ARG(Hs <= kResizeMaxScale * H && Ws <= kResizeMaxScale * W, "down-scaling by more than 8 is not supported");               \
    GCPX_CHECK_ARG(ksx == resize_ksize(Ws, W) && ksy == resize_ksize(Hs, H), "ksx / ksy are not the tap counts of these sizes")
// the bands of a resizing launch: R rows each, cap source rows at the most, L the LDS (the limits above keep the worst case at 62 KB)
#define GCPX_CHOOSE_BAND(Hs, Ws)                                                                                                          \
    int cap = 0;                                                                                                                          \
    ResizeLds L{};                                                                                                                        \
    const int R = resize_choose_band(Hs, Ws, H, W, ksx, ksy, &cap, &L);                                                                   \
    GCPX_CHECK_ARG(R > 0, "one output row's source rows do not fit the LDS")

extern "C" int gcpx_assemble_batch(const uint8_t* frames, const int32_t* info, const float* lut, const float* pad_in,
                                   const float* states_in, const float* actions_in, const float* states_mean, const float* states_den,
                                   int32_t B, int32_t T, int32_t H, int32_t W, int32_t state_dim, int32_t n_actions, float* traj_seq,
                                   float* I_0, float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states,
                                   float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ASSEMBLE(frames, states_in, actions_in);
    GCPX_CHECK_ARG(H > 0 && W > 0, "bad sizes");
    const int HW = H * W;
    GCPX_CHECK_ARG((HW & 3) != 0 || aligned16(frames, traj_seq, I_0, I_g), "frames / outputs not 16-byte aligned");
    const dim3 grid((unsigned)(B * T), (unsigned)(((HW + 3) / 4 + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(assemble_frames_kernel<SlotSrc>, grid, dim3(kThreads), 0, stream, frames, (long long)B * T, info, lut, T, HW,
                       traj_seq, I_0, I_g);
    launch_small<SlotSrc>(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask,
                          end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_resize_assemble_batch(const uint8_t* frames, const int32_t* info, const float* lut, const int32_t* kx, const int32_t* bx,
                                          const int32_t* ky, const int32_t* by, const float* pad_in, const float* states_in,
                                          const float* actions_in, const float* states_mean, const float* states_den, int32_t B, int32_t T,
                                          int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t ksx, int32_t ksy, int32_t state_dim,
                                          int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask, int64_t* end_ind,
                                          int64_t* start_ind, float* states, float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ASSEMBLE(frames, states_in, actions_in);
    GCPX_CHECK_RESIZE(Hs, Ws);
    GCPX_CHECK_ARG(aligned16(frames, traj_seq, I_0, I_g), "frames / outputs not 16-byte aligned");
    GCPX_CHOOSE_BAND(Hs, Ws);
    const long long n_frames = (long long)B * T;
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(resize_assemble_frames_kernel<SlotSrc>, grid, dim3(kThreads), (size_t)L.total, stream, frames,
                       n_frames * Hs * Ws * 3, n_frames, info, lut, kx, bx, ky, by, T, Hs, Ws, H, W, ksx, ksy, R, cap, traj_seq, I_0, I_g);
    launch_small<SlotSrc>(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask,
                          end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_assemble_batch_resident(const uint8_t* store, int64_t store_bytes, const int64_t* info, const float* lut,
                                            const float* pad_in, const float* states_store, const float* actions_store,
                                            const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t H, int32_t W,
                                            int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask,
                                            int64_t* end_ind, int64_t* start_ind, float* states, float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ASSEMBLE(store, states_store, actions_store);
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(info) & 7) == 0, "info not 8-byte aligned");
    GCPX_CHECK_ARG(H > 0 && W > 0 && H <= kResizeMaxSide && W <= kResizeMaxSide, "sides must be in [1, 512]");
    const int HW = H * W;
    GCPX_CHECK_ARG(store_bytes >= (int64_t)HW * 3, "store_bytes holds less than one frame");
    GCPX_CHECK_ARG((HW & 3) != 0 || aligned16(store, traj_seq, I_0, I_g), "store / outputs not 16-byte aligned");
    const dim3 grid((unsigned)(B * T), (unsigned)(((HW + 3) / 4 + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(assemble_frames_kernel<ResidentSrc>, grid, dim3(kThreads), 0, stream, store, store_bytes / ((long long)HW * 3), info,
                       lut, T, HW, traj_seq, I_0, I_g);
    launch_small<ResidentSrc>(stream, info, pad_in, states_store, actions_store, states_mean, states_den, B, T, state_dim, n_actions,
                              pad_mask, end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_resize_assemble_batch_resident(const uint8_t* store, int64_t store_bytes, const int64_t* info, const float* lut,
                                                   const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by,
                                                   const float* pad_in, const float* states_store, const float* actions_store,
                                                   const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t Hs,
                                                   int32_t Ws, int32_t H, int32_t W, int32_t ksx, int32_t ksy, int32_t state_dim,
                                                   int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask,
                                                   int64_t* end_ind, int64_t* start_ind, float* states, float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ASSEMBLE(store, states_store, actions_store);
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(info) & 7) == 0, "info not 8-byte aligned");
    GCPX_CHECK_RESIZE(Hs, Ws);
    const long long frame_bytes = (long long)Hs * Ws * 3;
    GCPX_CHECK_ARG(store_bytes >= frame_bytes, "store_bytes holds less than one frame");
    GCPX_CHECK_ARG(aligned16(store, traj_seq, I_0, I_g), "store / outputs not 16-byte aligned");
    GCPX_CHOOSE_BAND(Hs, Ws);
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(resize_assemble_frames_kernel<ResidentSrc>, grid, dim3(kThreads), (size_t)L.total, stream, store,
                       (long long)store_bytes, store_bytes / frame_bytes, info, lut, kx, bx, ky, by, T, Hs, Ws, H, W, ksx, ksy, R, cap,
                       traj_seq, I_0, I_g);
    launch_small<ResidentSrc>(stream, info, pad_in, states_store, actions_store, states_mean, states_den, B, T, state_dim, n_actions,
                              pad_mask, end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

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
    GCPX_CHECK_ASSEMBLE(background, states_in, actions_in);
    GCPX_CHECK_ARG(cw > 0 && 2 * cw >= kWindowMin && 2 * cw <= kWindowMax, "the window side 2 * cw must be in [4, 128]");
    const int D = 2 * cw;
    GCPX_CHECK_ARG(side >= D && side <= 16384, "the background's side must be in [2 * cw, 16384]");
    GCPX_CHECK_ARG(k > 0 && (k & 1) == 1 && k <= kStampMax, "the stamp side k must be odd and at most 31");
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(background) & 3) == 0, "background not 4-byte aligned");
    GCPX_CHECK_RESIZE(D, D);
    GCPX_CHECK_ARG(aligned16(nullptr, traj_seq, I_0, I_g), "outputs not 16-byte aligned");
    GCPX_CHOOSE_BAND(D, D);
    const long long bg_bytes = (long long)side * side * 3;
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(topdown_assemble_frames_kernel, grid, dim3(kThreads), (size_t)L.total, stream, background, side, bg_bytes, cw,
                       agent_stamp, goal_stamp, k, (uint32_t)agent_rgb, (uint32_t)goal_rgb, coords, goal, info, lut, kx, bx, ky, by, T, H, W,
                       ksx, ksy, R, cap, traj_seq, I_0, I_g);
    launch_small<SlotSrc>(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask,
                          end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
