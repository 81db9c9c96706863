// Batch assembly of the host-fed data path (video-gcp_amd/dataset.py): uploaded uint8 frames [B][T][H][W][3] plus a few integers per
// sequence -> the model's f32 inputs, written in place into the persistent buffers its launch plans read.
//
// The host mirrors the reference's per-item index logic (data_loader.py:131-211) and uploads, per sequence, the frame window
// raw[offset : offset + T] (n_frames of them, the rest of the slot undefined), the matching state / action windows and the pad mask.
// Here, for output frame t (randomize_length's chop and repeat of the last frame, data_loader.py:191-211):
//     s = min(t + chop, T - 1);  value = (t < zero_from && s < n_frames) ? lut[raw[s]] : lut[0]
// lut is the 256-entry table of `np.arange(256, dtype=np.uint8).astype(np.float32) / 255 * 2 - 1` built on the host, so the values
// are the reference's bit for bit whatever the compiler flags; padded frames are uint8 0 in the reference and so become -1.0.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInfo = 8;     // int32 per sequence: n_frames, n_states, n_actions, chop, zero_from, end_ind, -, -

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
    if ((HW & 3) == 0) {
        float4 v[3];
        if (valid) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(src + (size_t)p0 * 3);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];        // RGBR GBRG BRGB
            v[0] = make_float4(tab[w0 & 255], tab[(w0 >> 24) & 255], tab[(w1 >> 16) & 255], tab[(w2 >> 8) & 255]);
            v[1] = make_float4(tab[(w0 >> 8) & 255], tab[w1 & 255], tab[(w1 >> 24) & 255], tab[(w2 >> 16) & 255]);
            v[2] = make_float4(tab[(w0 >> 16) & 255], tab[(w1 >> 8) & 255], tab[w2 & 255], tab[(w2 >> 24) & 255]);
        } else {
            v[0] = v[1] = v[2] = make_float4(pad, pad, pad, pad);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            *reinterpret_cast<float4*>(dst + (size_t)c * HW + p0) = v[c];
            if (d0) *reinterpret_cast<float4*>(d0 + (size_t)c * HW + p0) = v[c];
            if (dg) *reinterpret_cast<float4*>(dg + (size_t)c * HW + p0) = v[c];
        }
    } else {
        for (int p = p0; p < min(p0 + 4, HW); ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = valid ? tab[src[(size_t)p * 3 + c]] : pad;
                dst[(size_t)c * HW + p] = x;
                if (d0) d0[(size_t)c * HW + p] = x;
                if (dg) dg[(size_t)c * HW + p] = x;
            }
        }
    }
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

}  // namespace

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
    hipLaunchKernelGGL(assemble_small_kernel, dim3(B), dim3(kThreads), 0, stream, info, pad_in, state_dim ? states_in : nullptr,
                       n_actions ? actions_in : nullptr, states_mean, states_den, T, state_dim, n_actions, pad_mask, end_ind,
                       start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
