// Scalar logs of the trainer (video-gcp_amd/scalar_log.py): the two statistics a logging step reads that no training kernel leaves behind.
//
//   gcpx_grad_segment_norms   log_gradients (base_model.py:139-146): torch.norm(p.grad) of every parameter, their mean and maximum, over
//                             the trainer's flat gradient vector
//   gcpx_kl_layerwise         TreeModule._log_outputs (tree_module.py:159-169): the KL error matrix averaged per tree level
// and the training guard's scan over the same tables (further down):
//   gcpx_grad_health          NanGradHook (base_trainer.py:20-66): NaN / +Inf / -Inf counts per parameter, the verdict, the optimizer's gate
//
// All are deterministic and bit-repeatable: every sum has a fixed shape, there is no atomic.
//
// Gradient norms.  The host cuts every counted segment into chunks of at most kChunk elements (scalar_log.grad_tables); stage 1 runs one
// workgroup per chunk.  A thread adds the squares of at most kSerial elements into one f32 accumulator (fmaf: one rounding per element),
// in the order it loads them -- 16-byte loads of elements 4 v .. 4 v + 3 for v = tid, tid + kThreads, ... where the chunk starts on a
// 16-byte boundary, the up to three elements behind the last whole quad by single loads, one per thread; single loads throughout where
// it does not.  The kThreads accumulators are then summed by a fixed tree of depth kTreeDepth: six butterfly steps across the wavefront,
// two levels over the four wavefronts in LDS.  Beside its sum a chunk reports whether any of its elements differs from zero.
// Stage 2, one workgroup, sums each segment's chunk partials in table order in f64 (exact to 2^-53 per term, so the f32 error of a norm is
// that of stage 1: relative <= (kSerial + kTreeDepth) 2^-24 on the sum of squares, half of it on the root, plus the one rounding of the
// f64 result to f32), takes the root, applies grad_scale and the clip coefficient, and walks the segments in index order for the mean,
// the maximum and the counts.
// A chunk is read only if it lies inside [0, n) and is no longer than kChunk: a wrong table gives a wrong number, never a wild access.
// The floats between segments are read by nobody.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = GCPX_GRAD_NORM_THREADS;
constexpr int kChunk = GCPX_GRAD_NORM_CHUNK;
constexpr int kSerial = GCPX_GRAD_NORM_SERIAL;
constexpr int kTreeDepth = GCPX_GRAD_NORM_TREE_DEPTH;
static_assert(kThreads == 256 && kChunk % (4 * kThreads) == 0 && kSerial == kChunk / kThreads + 1 && kTreeDepth == 6 + 2,
              "the constants of include/gcpx.h describe this kernel");

// sum over the 64 lanes, every lane gets the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ void __launch_bounds__(kThreads) chunk_sqsum_kernel(const float* __restrict__ grad, const long long n,
                                                               const gcpx_grad_chunk* __restrict__ chunks,
                                                               float* __restrict__ partial, const int n_chunks) {
    __shared__ float red[kThreads / 64];
    __shared__ int any[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gcpx_grad_chunk c = chunks[blockIdx.x];
    float acc = 0.f;
    bool nonzero = false;
    if (c.first >= 0 && c.length > 0 && c.length <= kChunk && c.first + c.length <= n) {      // (uniform over the workgroup)
        const float* g = grad + c.first;
        const int len = c.length;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const int nvec = len >> 2;
            const float4* g4 = reinterpret_cast<const float4*>(g);
            if (nvec == kChunk / 4) {                 // a full chunk: a fixed trip count, every load of the thread in flight at once
                float4 v[kChunk / 4 / kThreads];
#pragma unroll
                for (int i = 0; i < kChunk / 4 / kThreads; ++i) v[i] = g4[tid + i * kThreads];
#pragma unroll
                for (int i = 0; i < kChunk / 4 / kThreads; ++i) {
                    acc = fmaf(v[i].x, v[i].x, acc);
                    acc = fmaf(v[i].y, v[i].y, acc);
                    acc = fmaf(v[i].z, v[i].z, acc);
                    acc = fmaf(v[i].w, v[i].w, acc);
                    nonzero |= (v[i].x != 0.f) | (v[i].y != 0.f) | (v[i].z != 0.f) | (v[i].w != 0.f);
                }
            } else {
                for (int i = tid; i < nvec; i += kThreads) {
                    const float4 v = g4[i];
                    acc = fmaf(v.x, v.x, acc);
                    acc = fmaf(v.y, v.y, acc);
                    acc = fmaf(v.z, v.z, acc);
                    acc = fmaf(v.w, v.w, acc);
                    nonzero |= (v.x != 0.f) | (v.y != 0.f) | (v.z != 0.f) | (v.w != 0.f);
                }
                const int e = 4 * nvec + tid;         // the segment's tail: len % 4 single elements
                if (e < len) {
                    const float x = g[e];
                    acc = fmaf(x, x, acc);
                    nonzero |= x != 0.f;
                }
            }
        } else {
            for (int e = tid; e < len; e += kThreads) {
                const float x = g[e];
                acc = fmaf(x, x, acc);
                nonzero |= x != 0.f;
            }
        }
    }
    acc = wave_sum(acc);
    const bool wave_any = __any(nonzero);
    if (lane == 0) {
        red[wave] = acc;
        any[wave] = wave_any;
    }
    __syncthreads();
    if (tid == 0) {
        partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        partial[n_chunks + blockIdx.x] = (any[0] | any[1] | any[2] | any[3]) ? 1.f : 0.f;
    }
}

constexpr int kThreads2 = 1024;

__global__ void __launch_bounds__(kThreads2) segment_norm_kernel(const float* __restrict__ partial, const int n_chunks,
                                                                 const int32_t* __restrict__ seg_chunk0, const int n_seg,
                                                                 const float grad_scale, const float* __restrict__ clip_coef,
                                                                 float* __restrict__ seg_norm, float* __restrict__ stats) {
    __shared__ float tile[kThreads2];
    __shared__ int counted[kThreads2];
    const int tid = threadIdx.x;
    float coef = clip_coef ? clip_coef[0] : 1.f;
    coef = coef > 0.f ? coef : (coef < 0.f ? 0.f : 1.f);        // the optimizer state's slot: 0 = unset, < 0 = a coefficient of zero
    const double mul = (double)fabsf(grad_scale) * (double)coef;
    // thread 0 walks the segments in index order: these are its running values
    double sum = 0.0;
    float mx = -INFINITY;
    int n_counted = 0, n_nonfinite = 0;
    for (int s0 = 0; s0 < n_seg; s0 += kThreads2) {
        const int s = s0 + tid;
        if (s < n_seg) {
            const int c0 = max(seg_chunk0[s], 0), c1 = min(seg_chunk0[s + 1], n_chunks);
            double q = 0.0;
            bool nonzero = false;
            for (int c = c0; c < c1; ++c) {
                q += (double)partial[c];
                nonzero |= partial[n_chunks + c] != 0.f;
            }
            const float v = (float)(sqrt(q) * mul);
            seg_norm[s] = v;
            tile[tid] = v;
            counted[tid] = nonzero;
        }
        __syncthreads();
        if (tid == 0) {
            const int m = min(kThreads2, n_seg - s0);
            for (int i = 0; i < m; ++i) {
                if (!counted[i]) continue;
                const float v = tile[i];
                sum += (double)v;
                mx = (v != v || mx != mx) ? NAN : fmaxf(mx, v);           // torch.max: a NaN stays
                n_counted += 1;
                n_nonfinite += !(fabsf(v) <= 3.402823466e38f);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[0] = n_counted ? (float)(sum / (double)n_counted) : 0.f;
        stats[1] = n_counted ? mx : 0.f;
        stats[2] = (float)n_counted;
        stats[3] = (float)n_nonfinite;
    }
}

// ---------------------------------------------------------------------------------------------------
// layer-wise KL.  Kernel 1: one wavefront per (b, node): v = mean over nz of max(KL_elem, free_nats) -- the element loss.hip's
// kl_sequence sums; a lane adds the quads d = 4 lane, 4 (lane + 64), ... in order, then the butterfly.  Kernel 2: one wavefront per
// level l: entries e = b 2^l + j (node j of the level sits at depth-first position (2 j + 1) 2^(L-1-l) - 1), a lane adds the non-zero
// entries e = lane, lane + 64, ... and counts them, then the butterfly; sum / count (0 / 0 = NaN, as l[l != 0].mean() of no element).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) kl_node_mean_kernel(const float* __restrict__ qz, const float* __restrict__ pz, const int rows,
                                                           const int N, const int nz, const long long batch_stride,
                                                           const long long node_stride, const float free_nats,
                                                           float* __restrict__ node_v) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                     // (whole wavefronts leave: no barrier below)
    const int b = r / N, nd = r % N;
    const float* q = qz + (size_t)b * batch_stride + (size_t)nd * node_stride;
    const float* p = pz + (size_t)b * batch_stride + (size_t)nd * node_stride;
    float acc = 0.f;
    for (int d = 4 * lane; d < nz; d += 256) {
        const float4 mq = *reinterpret_cast<const float4*>(q + d), lq = *reinterpret_cast<const float4*>(q + nz + d);
        const float4 mp = *reinterpret_cast<const float4*>(p + d), lp = *reinterpret_cast<const float4*>(p + nz + d);
        const float mqa[4] = {mq.x, mq.y, mq.z, mq.w}, lqa[4] = {lq.x, lq.y, lq.z, lq.w};
        const float mpa[4] = {mp.x, mp.y, mp.z, mp.w}, lpa[4] = {lp.x, lp.y, lp.z, lp.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float diff = mqa[k] - mpa[k];
            const float kl = lpa[k] - lqa[k] + (expf(2.f * lqa[k]) + diff * diff) / (2.f * expf(2.f * lpa[k])) - 0.5f;
            acc += fmaxf(kl, free_nats);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) node_v[r] = acc / (float)nz;
}

__global__ void __launch_bounds__(1024) kl_level_mean_kernel(const float* __restrict__ node_v, const int B, const int L,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63, l = threadIdx.x >> 6;
    if (l >= L) return;
    const int N = (1 << L) - 1, per = 1 << l, sh = L - 1 - l;
    float acc = 0.f;
    int cnt = 0;
    for (int e = lane; e < B * per; e += 64) {
        const int b = e >> l, j = e & (per - 1);
        const float v = node_v[(size_t)b * N + (((2 * j + 1) << sh) - 1)];
        if (v != 0.f) {
            acc += v;
            cnt += 1;
        }
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) out[l] = acc / (float)cnt;
}

// ---------------------------------------------------------------------------------------------------
// Training guard (NanGradHook, base_trainer.py:20-66; the NaN total loss of base_gcp.py:302-303): gcpx_grad_health counts the NaN, +Inf
// and -Inf elements of every segment of a flat f32 vector, through the tables of the norms kernel above and in its shape.  An element
// is classified by its bit pattern alone (integer compares on the 32 bits: exponent all ones, mantissa zero or not, the sign), so
// denormals, -0 and +-FLT_MAX are finite whatever the float mode of the wavefront.  Stage 1, one workgroup per chunk: three integer
// counters per thread, the wavefront butterfly, the four wavefronts in LDS.  Stage 2, one workgroup: a thread sums the chunks of its
// segments, the workgroup reduces the totals, the number of bad segments and the first of them, thread 0 writes the summary and the
// gate.  Integer sums: the result does not depend on the schedule, there is no atomic.
// ---------------------------------------------------------------------------------------------------
struct BadCount { int nan, pinf, ninf; };

__device__ __forceinline__ void classify(const uint32_t u, BadCount& c) {
    c.nan += (u & 0x7fffffffu) > 0x7f800000u;
    c.pinf += u == 0x7f800000u;
    c.ninf += u == 0xff800000u;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ void __launch_bounds__(kThreads) chunk_health_kernel(const uint32_t* __restrict__ x, const long long n,
                                                                const gcpx_grad_chunk* __restrict__ chunks,
                                                                int32_t* __restrict__ partial) {
    __shared__ int red[kThreads / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gcpx_grad_chunk c = chunks[blockIdx.x];
    BadCount bc = {0, 0, 0};
    if (c.first >= 0 && c.length > 0 && c.length <= kChunk && c.first + c.length <= n) {      // (uniform over the workgroup)
        const uint32_t* g = x + c.first;
        const int len = c.length;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const int nvec = len >> 2;
            const uint4* g4 = reinterpret_cast<const uint4*>(g);
            if (nvec == kChunk / 4) {                 // a full chunk: a fixed trip count, every load of the thread in flight at once
                uint4 v[kChunk / 4 / kThreads];
#pragma unroll
                for (int i = 0; i < kChunk / 4 / kThreads; ++i) v[i] = g4[tid + i * kThreads];
#pragma unroll
                for (int i = 0; i < kChunk / 4 / kThreads; ++i) {
                    classify(v[i].x, bc);
                    classify(v[i].y, bc);
                    classify(v[i].z, bc);
                    classify(v[i].w, bc);
                }
            } else {
                for (int i = tid; i < nvec; i += kThreads) {
                    const uint4 v = g4[i];
                    classify(v.x, bc);
                    classify(v.y, bc);
                    classify(v.z, bc);
                    classify(v.w, bc);
                }
                const int e = 4 * nvec + tid;         // the segment's tail: len % 4 single elements
                if (e < len) classify(g[e], bc);
            }
        } else {
            for (int e = tid; e < len; e += kThreads) classify(g[e], bc);
        }
    }
    bc.nan = wave_sum_int(bc.nan);
    bc.pinf = wave_sum_int(bc.pinf);
    bc.ninf = wave_sum_int(bc.ninf);
    if (lane == 0) {
        red[wave][0] = bc.nan;
        red[wave][1] = bc.pinf;
        red[wave][2] = bc.ninf;
    }
    __syncthreads();
    if (tid < 3) partial[3 * (size_t)blockIdx.x + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ void __launch_bounds__(kThreads2) segment_health_kernel(const int32_t* __restrict__ partial, const int n_chunks,
                                                                   const int32_t* __restrict__ seg_chunk0, const int n_seg,
                                                                   const uint32_t* __restrict__ extra, const int n_extra,
                                                                   int32_t* __restrict__ seg_bad, int32_t* __restrict__ summary,
                                                                   float* __restrict__ gate) {
    __shared__ int red[kThreads2 / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this thread's share: [0..2] element counts, [3] bad segments, [4] bad extra scalars; the first bad segment apart (a minimum)
    int acc[5] = {0, 0, 0, 0, 0};
    int first = 0x7fffffff;
    for (int s = tid; s < n_seg; s += kThreads2) {
        const int c0 = max(seg_chunk0[s], 0), c1 = min(seg_chunk0[s + 1], n_chunks);
        int q[3] = {0, 0, 0};
        for (int c = c0; c < c1; ++c) {
            q[0] += partial[3 * (size_t)c];
            q[1] += partial[3 * (size_t)c + 1];
            q[2] += partial[3 * (size_t)c + 2];
        }
        seg_bad[3 * (size_t)s] = q[0];
        seg_bad[3 * (size_t)s + 1] = q[1];
        seg_bad[3 * (size_t)s + 2] = q[2];
        acc[0] += q[0];
        acc[1] += q[1];
        acc[2] += q[2];
        if (q[0] | q[1] | q[2]) {                     // (counts are >= 0)
            acc[3] += 1;
            first = min(first, s);
        }
    }
    for (int e = tid; e < n_extra; e += kThreads2) acc[4] += (extra[e] & 0x7f800000u) == 0x7f800000u;
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[k] = wave_sum_int(acc[k]);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) first = min(first, __shfl_xor(first, m));
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[wave][k] = acc[k];
        red[wave][5] = first;
    }
    __syncthreads();
    if (tid == 0) {
        int tot[5] = {0, 0, 0, 0, 0};
        int f = 0x7fffffff;
        for (int w = 0; w < kThreads2 / 64; ++w) {
            for (int k = 0; k < 5; ++k) tot[k] += red[w][k];
            f = min(f, red[w][5]);
        }
        const int verdict = (tot[3] > 0 || tot[4] > 0) ? 1 : 0;
        summary[0] = tot[0];
        summary[1] = tot[1];
        summary[2] = tot[2];
        summary[3] = tot[3];
        summary[4] = tot[3] > 0 ? f : -1;
        summary[5] = tot[4];
        summary[6] = verdict;
        summary[7] += verdict;
        if (gate) gate[0] = verdict ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" int gcpx_grad_segment_norms(const float* grad, int64_t n, const gcpx_grad_chunk* chunks, int32_t n_chunks,
                                       const int32_t* seg_chunk0, int32_t n_seg, float grad_scale, const float* clip_coef,
                                       float* partial, int64_t n_partial, float* seg_norm, float* stats, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(grad && chunks && seg_chunk0 && partial && seg_norm && stats, "null pointer");
    GCPX_CHECK_ARG(n > 0 && n_chunks > 0 && n_seg > 0 && n_seg <= n_chunks, "sizes must be positive, and every segment has a chunk");
    GCPX_CHECK_ARG(n_partial >= 2 * (int64_t)n_chunks, "partial must hold 2 * n_chunks floats");
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 3) == 0 && (reinterpret_cast<uintptr_t>(chunks) & 7) == 0, "misaligned pointer");
    hipLaunchKernelGGL(chunk_sqsum_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, stream, grad, (long long)n, chunks, partial,
                       n_chunks);
    hipLaunchKernelGGL(segment_norm_kernel, dim3(1), dim3(kThreads2), 0, stream, partial, n_chunks, seg_chunk0, n_seg, grad_scale,
                       clip_coef, seg_norm, stats);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_grad_health(const float* x, int64_t n, const gcpx_grad_chunk* chunks, int32_t n_chunks, const int32_t* seg_chunk0,
                                int32_t n_seg, const float* extra, int32_t n_extra, int32_t* partial, int64_t n_partial, int32_t* seg_bad,
                                int32_t* summary, float* gate, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(x && chunks && seg_chunk0 && partial && seg_bad && summary, "null pointer");
    GCPX_CHECK_ARG(n > 0 && n_chunks > 0 && n_seg > 0 && n_seg <= n_chunks, "sizes must be positive, and every segment has a chunk");
    GCPX_CHECK_ARG(n < (1ll << 31), "more than 2^31 - 1 elements: the counts are 32-bit");
    GCPX_CHECK_ARG(n_extra >= 0 && (n_extra == 0 || extra), "n_extra scalars need a pointer");
    GCPX_CHECK_ARG(n_partial >= 3 * (int64_t)n_chunks, "partial must hold 3 * n_chunks integers");
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(chunks) & 7) == 0 &&
                       ((reinterpret_cast<uintptr_t>(extra) | reinterpret_cast<uintptr_t>(gate)) & 3) == 0, "misaligned pointer");
    hipLaunchKernelGGL(chunk_health_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, stream, reinterpret_cast<const uint32_t*>(x),
                       (long long)n, chunks, partial);
    hipLaunchKernelGGL(segment_health_kernel, dim3(1), dim3(kThreads2), 0, stream, partial, n_chunks, seg_chunk0, n_seg,
                       reinterpret_cast<const uint32_t*>(extra), n_extra, seg_bad, summary, gate);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

extern "C" int gcpx_kl_layerwise(const float* qz, const float* pz, int32_t B, int32_t L, int32_t nz, int64_t batch_stride,
                                 int64_t node_stride, float free_nats, float* node_v, float* out, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(qz && pz && node_v && out && B > 0 && nz > 0, "null pointer / bad sizes");
    GCPX_CHECK_ARG(L >= 1 && L <= 16, "hierarchy levels must be in [1, 16]");
    GCPX_CHECK_ARG(nz % 4 == 0 && batch_stride % 4 == 0 && node_stride % 4 == 0, "nz and the strides must be multiples of 4");
    GCPX_CHECK_ARG(((reinterpret_cast<uintptr_t>(qz) | reinterpret_cast<uintptr_t>(pz)) & 15) == 0, "q_z / p_z not 16-byte aligned");
    const long long N = (1ll << L) - 1;
    GCPX_CHECK_ARG((long long)B * N < (1ll << 30), "too many nodes");
    const int rows = (int)(B * N);
    hipLaunchKernelGGL(kl_node_mean_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, qz, pz, rows, (int)N, nz,
                       (long long)batch_stride, (long long)node_stride, free_nats, node_v);
    hipLaunchKernelGGL(kl_level_mean_kernel, dim3(1), dim3(1024), 0, stream, node_v, B, L, out);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
