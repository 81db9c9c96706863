// Batch assembly of the device-resident data path (video-gcp_amd/dataset_resident.py): the frames of a whole split stay in HBM as
// uint8, all trajectories back to back, and a batch is described by a few integers per sequence that say which window of which
// trajectory goes where.  The kernels of csrc/batch_assemble.hip with one difference: a sequence's frames are not row b of a freshly
// uploaded [B][T][H][W][3] slot but frames [first, first + n_frames) of the store, states and actions likewise rows of two resident
// f32 arrays.  Time map, resize, table lookup and the stores are the shared device functions of resize_passes.h, so the values are
// those of gcpx_assemble_batch / gcpx_resize_assemble_batch bit for bit.
//
// info int64 [B][8] per sequence (kInfoResident; include/gcpx.h fixes the layout):
//     0 first frame of the window in the store      1 n_frames available from there within the trajectory
//     2 first state row                             3 n_states
//     4 first action row                            5 n_actions
//     6 chop                                        7 zero_from | end_ind << 32
// Addressing into the store is 64-bit.  A frame is read only when the time map says it is the sequence's own (s < n_frames: the bytes
// behind a short trajectory belong to the next one) and when it lies inside the store (first >= 0, first + s < store frames), so
// integers that do not belong to the store give a padded frame, never a wild read; the 16-byte staging loads of the resize form stop
// at store_bytes.
#include "resize_passes.h"

using namespace gcpx_resize;

namespace {

struct ResidentSeq {
    long long first;
    int n_frames, chop, zero_from, end_ind;
};

__device__ __forceinline__ ResidentSeq resident_seq(const int64_t* __restrict__ in, const int T) {
    ResidentSeq q;
    q.first = in[0];
    q.n_frames = (int)min((long long)in[1], (long long)T);
    q.chop = max((int)in[6], 0);
    q.zero_from = (int)(in[7] & 0xffffffffll);
    q.end_ind = (int)(in[7] >> 32);
    return q;
}

// output frame t of the sequence shows window frame s; true when that frame is the sequence's own and lies inside the store
__device__ __forceinline__ bool resident_valid(const ResidentSeq& q, const int t, const int s, const long long store_frames) {
    return t < q.zero_from && s < q.n_frames && q.first >= 0 && q.first < store_frames - s;
}

// one thread = four consecutive pixels of one frame (assemble_frames_kernel of csrc/batch_assemble.hip)
__global__ void __launch_bounds__(kThreads) assemble_frames_resident_kernel(const uint8_t* __restrict__ store, const long long store_frames,
                                                                           const int64_t* __restrict__ info,
                                                                           const float* __restrict__ lut, const int T, const int HW,
                                                                           float* __restrict__ traj, float* __restrict__ I0,
                                                                           float* __restrict__ Ig) {
    __shared__ float tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int bt = blockIdx.x;
    const int b = bt / T, t = bt - b * T;
    const ResidentSeq q = resident_seq(info + (size_t)b * kInfoResident, T);
    const int s = min(t + q.chop, T - 1);
    const bool valid = resident_valid(q, t, s, store_frames);
    const uint8_t* src = store + (size_t)(valid ? q.first + s : 0) * HW * 3;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW : nullptr;
    float* dg = t == q.end_ind ? Ig + (size_t)b * 3 * HW : nullptr;
    const float pad = tab[0];
    const int p0 = (blockIdx.y * kThreads + threadIdx.x) * 4;
    if (p0 >= HW) return;
    lut_quad_store(src, valid, tab, pad, HW, p0, dst, d0, dg);
}

// one workgroup per sequence (assemble_small_kernel of csrc/batch_assemble.hip): states and actions are rows of the resident arrays
__global__ void __launch_bounds__(kThreads) assemble_small_resident_kernel(
    const int64_t* __restrict__ info, const float* __restrict__ pad_in, const float* __restrict__ states_store,
    const float* __restrict__ actions_store, const float* __restrict__ mean, const float* __restrict__ den, const int T, const int S,
    const int A, float* __restrict__ pad_mask, int64_t* __restrict__ end_ind, int64_t* __restrict__ start_ind, float* __restrict__ states,
    float* __restrict__ actions) {
    const int b = blockIdx.x;
    const int64_t* in = info + (size_t)b * kInfoResident;
    const ResidentSeq q = resident_seq(in, T);
    const long long srow = in[2], arow = in[4];
    const int n_states = srow < 0 ? 0 : (int)min((long long)in[3], (long long)T);
    const int n_actions = arow < 0 ? 0 : (int)min((long long)in[5], (long long)(T - 1));
    if (threadIdx.x == 0) {
        end_ind[b] = q.end_ind;
        start_ind[b] = 0;
    }
    for (int i = threadIdx.x; i < T; i += kThreads) pad_mask[(size_t)b * T + i] = pad_in[(size_t)b * T + i];
    for (int i = threadIdx.x; i < T * S; i += kThreads) {
        const int t = i / S, k = i - t * S, s = min(t + q.chop, T - 1);
        float x = (t < q.zero_from && s < n_states) ? states_store[(size_t)(srow + s) * S + k] : 0.f;
        if (mean) x = __fdiv_rn(__fsub_rn(x, mean[k]), den[k]);
        states[((size_t)b * T + t) * S + k] = x;
    }
    for (int i = threadIdx.x; i < (T - 1) * A; i += kThreads) {
        const int t = i / A, k = i - t * A, s = min(t + q.chop, T - 2);
        actions[((size_t)b * (T - 1) + t) * A + k] =
            (t < q.zero_from && s < n_actions) ? actions_store[(size_t)(arow + s) * A + k] : 0.f;
    }
}

// one workgroup = R output rows (a band) of one output frame (resize_assemble_frames_kernel of csrc/batch_assemble.hip)
__global__ void __launch_bounds__(kThreads) resize_assemble_frames_resident_kernel(
    const uint8_t* __restrict__ store, const long long store_bytes, const long long store_frames, const int64_t* __restrict__ info,
    const float* __restrict__ lut, const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, const int32_t* __restrict__ ky,
    const int32_t* __restrict__ by, const int T, const int Hs, const int Ws, const int H, const int W, const int ksx, const int ksy,
    const int R, const int cap, float* __restrict__ traj, float* __restrict__ I0, float* __restrict__ Ig) {
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
    const ResidentSeq q = resident_seq(info + (size_t)b * kInfoResident, T);
    const int s = min(t + q.chop, T - 1);
    const bool valid = resident_valid(q, t, s, store_frames);
    const int HW = H * W, W4 = W >> 2;
    float* dst = traj + ((size_t)b * T + t) * 3 * HW + (size_t)r0 * W;
    float* d0 = t == 0 ? I0 + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    float* dg = t == q.end_ind ? Ig + (size_t)b * 3 * HW + (size_t)r0 * W : nullptr;
    tab[tid] = lut[tid];
    if (!valid) {                                 // a padded frame resizes to zeros: lut[0], nothing read
        store_pad_band(lut[0], nr, W4, HW, dst, d0, dg, tid);
        return;
    }
    for (int i = tid; i < W * ksx; i += kThreads) skx[i] = kx[i];
    for (int i = tid; i < 2 * W; i += kThreads) sbx[i] = bx[i];
    for (int i = tid; i < nr * ksy; i += kThreads) sky[i] = ky[r0 * ksy + i];
    for (int i = tid; i < 2 * nr; i += kThreads) sby[i] = by[2 * r0 + i];
    // the band's source rows [y_lo, y_lo + nrows) of frame first + s of the store, staged with the tables under one barrier
    const int y_lo = min(max(by[2 * r0], 0), Hs - 1);
    const int nrows = min(min(max(by[2 * (r0 + nr - 1)] + by[2 * (r0 + nr - 1) + 1], y_lo + 1), Hs) - y_lo, cap);
    const int row_bytes = Ws * 3;
    const long long a0 = ((q.first + s) * Hs + y_lo) * row_bytes;
    const int shift = stage_bytes(store, a0, nrows * row_bytes, store_bytes, raw, tid);
    __syncthreads();
    resize_rows_any(ksx, raw, shift, hres, skx, sbx, nrows, Ws, W, tid);
    __syncthreads();
    resize_cols_store(hres, sky, sby, tab, y_lo, nrows, nr, W, ksy, HW, dst, d0, dg, tid);
}

void launch_small(hipStream_t stream, const int64_t* info, const float* pad_in, const float* states_store, const float* actions_store,
                  const float* mean, const float* den, const int B, const int T, const int S, const int A, float* pad_mask,
                  int64_t* end_ind, int64_t* start_ind, float* states, float* actions) {
    hipLaunchKernelGGL(assemble_small_resident_kernel, dim3(B), dim3(kThreads), 0, stream, info, pad_in, S ? states_store : nullptr,
                       A ? actions_store : nullptr, mean, den, T, S, A, pad_mask, end_ind, start_ind, states, actions);
}

}  // namespace

#define GCPX_CHECK_RESIDENT_COMMON()                                                                                                    \
    GCPX_CHECK_ARG(store && info && lut && pad_in && traj_seq && I_0 && I_g && pad_mask && end_ind && start_ind, "null pointer");       \
    GCPX_CHECK_ARG(B > 0 && T > 1 && state_dim >= 0 && n_actions >= 0, "bad sizes");                                                    \
    GCPX_CHECK_ARG(state_dim == 0 || (states_store && states), "states_store / states null with state_dim > 0");                        \
    GCPX_CHECK_ARG(n_actions == 0 || (actions_store && actions), "actions_store / actions null with n_actions > 0");                    \
    GCPX_CHECK_ARG(!states_mean == !states_den, "states_mean and states_den go together");                                              \
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(info) & 7) == 0, "info not 8-byte aligned")

extern "C" int gcpx_assemble_batch_resident(const uint8_t* store, int64_t store_bytes, const int64_t* info, const float* lut,
                                            const float* pad_in, const float* states_store, const float* actions_store,
                                            const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t H, int32_t W,
                                            int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask,
                                            int64_t* end_ind, int64_t* start_ind, float* states, float* actions, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_RESIDENT_COMMON();
    GCPX_CHECK_ARG(H > 0 && W > 0 && H <= kResizeMaxSide && W <= kResizeMaxSide, "sides must be in [1, 512]");
    const int HW = H * W;
    GCPX_CHECK_ARG(store_bytes >= (int64_t)HW * 3, "store_bytes holds less than one frame");
    GCPX_CHECK_ARG((HW & 3) != 0 || ((reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(traj_seq) |
                                      reinterpret_cast<uintptr_t>(I_0) | reinterpret_cast<uintptr_t>(I_g)) & 15) == 0,
                   "store / outputs not 16-byte aligned");
    const long long store_frames = store_bytes / ((long long)HW * 3);
    const dim3 grid((unsigned)(B * T), (unsigned)(((HW + 3) / 4 + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(assemble_frames_resident_kernel, grid, dim3(kThreads), 0, stream, store, store_frames, info, lut, T, HW, traj_seq,
                       I_0, I_g);
    launch_small(stream, info, pad_in, states_store, actions_store, states_mean, states_den, B, T, state_dim, n_actions, pad_mask, end_ind,
                 start_ind, states, actions);
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
    GCPX_CHECK_RESIDENT_COMMON();
    GCPX_CHECK_ARG(kx && bx && ky && by, "null coefficient / bounds table");
    GCPX_CHECK_ARG(Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hs <= kResizeMaxSide && Ws <= kResizeMaxSide && H <= kResizeMaxSide &&
                       W <= kResizeMaxSide, "source and output sides must be in [1, 512]");
    GCPX_CHECK_ARG((W & 3) == 0, "output width must be a multiple of 4");
    GCPX_CHECK_ARG(Hs <= kResizeMaxScale * H && Ws <= kResizeMaxScale * W, "down-scaling by more than 8 is not supported");
    GCPX_CHECK_ARG(ksx == resize_ksize(Ws, W) && ksy == resize_ksize(Hs, H), "ksx / ksy are not the tap counts of these sizes");
    const long long frame_bytes = (long long)Hs * Ws * 3;
    GCPX_CHECK_ARG(store_bytes >= frame_bytes, "store_bytes holds less than one frame");
    GCPX_CHECK_ARG(((reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(traj_seq) | reinterpret_cast<uintptr_t>(I_0) |
                     reinterpret_cast<uintptr_t>(I_g)) & 15) == 0, "store / outputs not 16-byte aligned");
    int cap = 0;
    ResizeLds L{};
    const int R = resize_choose_band(Hs, Ws, H, W, ksx, ksy, &cap, &L);
    GCPX_CHECK_ARG(R > 0, "one output row's source rows do not fit the LDS");
    const dim3 grid((unsigned)(B * T), (unsigned)((H + R - 1) / R));
    hipLaunchKernelGGL(resize_assemble_frames_resident_kernel, grid, dim3(kThreads), (size_t)L.total, stream, store, (long long)store_bytes,
                       store_bytes / frame_bytes, info, lut, kx, bx, ky, by, T, Hs, Ws, H, W, ksx, ksy, R, cap, traj_seq, I_0, I_g);
    launch_small(stream, info, pad_in, states_store, actions_store, states_mean, states_den, B, T, state_dim, n_actions, pad_mask, end_ind,
                 start_ind, states, actions);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
