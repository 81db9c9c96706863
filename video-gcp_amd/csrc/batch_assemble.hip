// Batch assembly of the host-fed data path (video-gcp_amd/dataset.py): uploaded uint8 frames [B][T][H][W][3] plus a few integers per
// sequence -> the model's f32 inputs, written in place into the persistent buffers its launch plans read.
//
// The host mirrors the reference's per-item index logic (data_loader.py:131-211) and uploads, per sequence, the frame window
// raw[offset : offset + T] (n_frames of them, the rest of the slot undefined), the matching state / action windows and the pad mask.
// Here, for output frame t (randomize_length's chop and repeat of the last frame, data_loader.py:191-211):
//     s = min(t + chop, T - 1);  value = (t < zero_from && s < n_frames) ? lut[raw[s]] : lut[0]
// lut is the 256-entry table of `np.arange(256, dtype=np.uint8).astype(np.float32) / 255 * 2 - 1` built on the host, so the values
// are the reference's bit for bit whatever the compiler flags; padded frames are uint8 0 in the reference and so become -1.0.
//
// gcpx_resize_assemble_batch: the same assembly for frames stored at Hs x Ws != H x W.  Between the time map and the table lookup every
// frame goes through the reference's resize (data_loader.py:213-220), which is Pillow's 8-bit bilinear Image.resize: a horizontal and a
// vertical pass of integer arithmetic, each rounding to uint8, over int32 coefficient tables the host builds once in float64
// (dataset.resize_coeffs).  Integer only here, so the pixels are Pillow's whatever the compiler flags.
// Limits (invalid argument otherwise): sides of source and output in [1, 512], W a multiple of 4, Hs / H and Ws / W at most 8 (no limit on
// up-sampling inside the side limits), tap counts equal to Pillow's for the sizes, 16-byte aligned frames and images.
#include "resize_passes.h"

using namespace gcpx_resize;   // kThreads, kInfo, the two passes of the resampler and the choice of the band

namespace {

// one thread = four consecutive pixels of one frame: 12 bytes read, one float4 written to each of the three channel planes
__global__ void __launch_bounds__(kThreads) assemble_frames_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ info,
                                                                  const float* __restrict__ lut, const int T, const int HW,
                                                                  float* __restrict__ traj, float* __restrict__ I0,
                                                                  float* __restrict__ Ig) {
    __shared__ float tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const int32_t* in = info + (size_t)b * kInfo;
    const int n_frames = min(in[0], T), chop = max(in[3], 0), zero_from = in[4], end_ind = in[5];
    const int s = min(t + chop, T - 1);
    const bool valid = t < zero_from && s < n_frames;
    const uint8_t* src = frames + ((size_t)b * T + s) * HW * 3;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW : nullptr;
    float* dg = t == end_ind ? Ig + (size_t)b * 3 * HW : nullptr;
    const float pad = tab[0];
    const int p0 = (blockIdx.y * kThreads + threadIdx.x) * 4;
    if (p0 >= HW) return;
    lut_quad_store(src, valid, tab, pad, HW, p0, dst, d0, dg);
}

// one workgroup per sequence: pad mask, end / start index, states (standardised) and actions under the same time map as the frames
// (actions have T - 1 steps: the reference pads them to T and drops the last, so their "last frame" is T - 2)
__global__ void __launch_bounds__(kThreads) assemble_small_kernel(const int32_t* __restrict__ info, const float* __restrict__ pad_in,
                                                                 const float* __restrict__ states_in, const float* __restrict__ actions_in,
                                                                 const float* __restrict__ mean, const float* __restrict__ den,
                                                                 const int T, const int S, const int A, float* __restrict__ pad_mask,
                                                                 int64_t* __restrict__ end_ind, int64_t* __restrict__ start_ind,
                                                                 float* __restrict__ states, float* __restrict__ actions) {
    const int b = blockIdx.x;
    const int32_t* in = info + (size_t)b * kInfo;
    const int n_states = min(in[1], T), n_actions = min(in[2], T - 1), chop = max(in[3], 0), zero_from = in[4];
    if (threadIdx.x == 0) {
        end_ind[b] = in[5];
        start_ind[b] = 0;
    }
    for (int i = threadIdx.x; i < T; i += kThreads) pad_mask[(size_t)b * T + i] = pad_in[(size_t)b * T + i];
    for (int i = threadIdx.x; i < T * S; i += kThreads) {
        const int t = i / S, k = i - t * S, s = min(t + chop, T - 1);
        float x = (t < zero_from && s < n_states) ? states_in[((size_t)b * T + s) * S + k] : 0.f;
        if (mean) x = __fdiv_rn(__fsub_rn(x, mean[k]), den[k]);
        states[((size_t)b * T + t) * S + k] = x;
    }
    for (int i = threadIdx.x; i < (T - 1) * A; i += kThreads) {
        const int t = i / A, k = i - t * A, s = min(t + chop, T - 2);
        actions[((size_t)b * (T - 1) + t) * A + k] =
            (t < zero_from && s < n_actions) ? actions_in[((size_t)b * (T - 1) + s) * A + k] : 0.f;
    }
}

// ---- resize + assembly --------------------------------------------------------------------------------------------------------

// one workgroup = R output rows (a band) of one output frame.  The band's `nrows` <= cap source rows are one contiguous run of bytes:
// 16-byte loads into LDS, horizontal pass LDS -> LDS as bytes (resize_rows),
// vertical pass out of LDS (one thread: four output columns of one row = 12 bytes per tap), table lookup, float4 stores.
// Every table entry is clamped to what was staged, so tables that do not belong to the sizes give a wrong picture, never a wild access.
__global__ void __launch_bounds__(kThreads) resize_assemble_frames_kernel(
    const uint8_t* __restrict__ frames, const int32_t* __restrict__ info, const float* __restrict__ lut, const int32_t* __restrict__ kx,
    const int32_t* __restrict__ bx, const int32_t* __restrict__ ky, const int32_t* __restrict__ by, const int T, const int Hs, const int Ws,
    const int H, const int W, const int ksx, const int ksy, const int R, const int cap, const long long total_bytes,
    float* __restrict__ traj, float* __restrict__ I0, float* __restrict__ Ig) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ResizeLds L = resize_lds(Ws, W, ksx, ksy, R, cap);
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
    const bool valid = t < zero_from && s < n_frames;
    const int HW = H * W, W4 = W >> 2;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW + (size_t)r0 * W;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    float* dg = t == end_ind ? Ig + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    tab[tid] = lut[tid];
    if (!valid) {                                 // a padded frame resizes to zeros: lut[0], nothing read
        store_pad_band(lut[0], nr, W4, HW, dst, d0, dg, tid);
        return;
    }
    for (int i = tid; i < W * ksx; i += kThreads) skx[i] = kx[i];
    for (int i = tid; i < 2 * W; i += kThreads) sbx[i] = bx[i];
    for (int i = tid; i < nr * ksy; i += kThreads) sky[i] = ky[r0 * ksy + i];
    for (int i = tid; i < 2 * nr; i += kThreads) sby[i] = by[2 * r0 + i];
    // the band's source rows [y_lo, y_lo + nrows), staged with the tables under one barrier
    const int y_lo = min(max(by[2 * r0], 0), Hs - 1);
    const int nrows = min(min(max(by[2 * (r0 + nr - 1)] + by[2 * (r0 + nr - 1) + 1], y_lo + 1), Hs) - y_lo, cap);
    const int row_bytes = Ws * 3;
    const long long a0 = (((long long)b * T + s) * Hs + y_lo) * row_bytes;
    const int shift = stage_bytes(frames, a0, nrows * row_bytes, total_bytes, raw, tid);
    __syncthreads();
    // horizontal pass: hres[r][xx][c] for the nrows staged rows
    resize_rows_any(ksx, raw, shift, hres, skx, sbx, nrows, Ws, W, tid);
    __syncthreads();
    // vertical pass, conversion and stores
    resize_cols_store(hres, sky, sby, tab, y_lo, nrows, nr, W, ksy, HW, dst, d0, dg, tid);
}

}  // namespace

void gcpx_resize::launch_assemble_small(hipStream_t stream, const int32_t* info, const float* pad_in, const float* states_in,
                                        const float* actions_in, const float* mean, const float* den, const int B, const int T, const int S,
                                        const int A, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states, float* actions) {
    hipLaunchKernelGGL(assemble_small_kernel, dim3(B), dim3(kThreads), 0, stream, info, pad_in, S ? states_in : nullptr,
                       A ? actions_in : nullptr, mean, den, T, S, A, pad_mask, end_ind, start_ind, states, actions);
}

extern "C" int gcpx_assemble_batch(const uint8_t* frames, const int32_t* info, const float* lut, const float* pad_in,
                                   const float* states_in, const float* actions_in, const float* states_mean, const float* states_den,
                                   int32_t B, int32_t T, int32_t H, int32_t W, int32_t state_dim, int32_t n_actions, float* traj_seq,
                                   float* I_0, float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states,
                                   float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(frames && info && lut && pad_in && traj_seq && I_0 && I_g && pad_mask && end_ind && start_ind, "null pointer");
    GCPX_CHECK_ARG(B > 0 && T > 1 && H > 0 && W > 0 && state_dim >= 0 && n_actions >= 0, "bad sizes");
    GCPX_CHECK_ARG(state_dim == 0 || (states_in && states), "states_in / states null with state_dim > 0");
    GCPX_CHECK_ARG(n_actions == 0 || (actions_in && actions), "actions_in / actions null with n_actions > 0");
    GCPX_CHECK_ARG(!states_mean == !states_den, "states_mean and states_den go together");
    const int HW = H * W;
    GCPX_CHECK_ARG((HW & 3) != 0 || ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(traj_seq) |
                                      reinterpret_cast<uintptr_t>(I_0) | reinterpret_cast<uintptr_t>(I_g)) & 15) == 0,
                   "frames / outputs not 16-byte aligned");
    const dim3 grid((unsigned)(B * T), (unsigned)(((HW + 3) / 4 + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(assemble_frames_kernel, grid, dim3(kThreads), 0, stream, frames, info, lut, T, HW, traj_seq, I_0, I_g);
    launch_assemble_small(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask,
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
    GCPX_CHECK_ARG(frames && info && lut && pad_in && traj_seq && I_0 && I_g && pad_mask && end_ind && start_ind, "null pointer");
    GCPX_CHECK_ARG(kx && bx && ky && by, "null coefficient / bounds table");
    GCPX_CHECK_ARG(B > 0 && T > 1 && state_dim >= 0 && n_actions >= 0, "bad sizes");
    GCPX_CHECK_ARG(Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hs <= kResizeMaxSide && Ws <= kResizeMaxSide && H <= kResizeMaxSide &&
                       W <= kResizeMaxSide, "source and output sides must be in [1, 512]");
    GCPX_CHECK_ARG((W & 3) == 0, "output width must be a multiple of 4");
    GCPX_CHECK_ARG(Hs <= kResizeMaxScale * H && Ws <= kResizeMaxScale * W, "down-scaling by more than 8 is not supported");
    GCPX_CHECK_ARG(ksx == resize_ksize(Ws, W) && ksy == resize_ksize(Hs, H), "ksx / ksy are not the tap counts of these sizes");
    GCPX_CHECK_ARG(state_dim == 0 || (states_in && states), "states_in / states null with state_dim > 0");
    GCPX_CHECK_ARG(n_actions == 0 || (actions_in && actions), "actions_in / actions null with n_actions > 0");
    GCPX_CHECK_ARG(!states_mean == !states_den, "states_mean and states_den go together");
    GCPX_CHECK_ARG(((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(traj_seq) | reinterpret_cast<uintptr_t>(I_0) |
                     reinterpret_cast<uintptr_t>(I_g)) & 15) == 0, "frames / outputs not 16-byte aligned");
    int cap = 0;
    ResizeLds L{};
    const int R = resize_choose_band(Hs, Ws, H, W, ksx, ksy, &cap, &L);
    GCPX_CHECK_ARG(R > 0, "one output row's source rows do not fit the LDS");    // (the limits above keep the worst case at 62 KB)
    const long long total_bytes = (long long)B * T * Hs * Ws * 3;
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(resize_assemble_frames_kernel, grid, dim3(kThreads), (size_t)L.total, stream, frames, info, lut, kx, bx, ky, by, T,
                       Hs, Ws, H, W, ksx, ksy, R, cap, total_bytes, traj_seq, I_0, I_g);
    launch_assemble_small(stream, info, pad_in, states_in, actions_in, states_mean, states_den, B, T, state_dim, n_actions, pad_mask,
                          end_ind, start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
