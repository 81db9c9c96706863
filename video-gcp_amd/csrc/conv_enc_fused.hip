// The first two encoder blocks of 64 x 64 frames in one launch: 3 -> 16 channels (64 x 64 -> 32 x 32, bias + LeakyReLU) and 16 -> 32
// channels (32 x 32 -> 16 x 16, split-f16), the 32 x 32 x 16 map between them kept in LDS.
//
// There is no BatchNorm between the two layers, so as two launches (conv4x4s2_image_lds_kernel<64>, conv_enc.hip, and
// conv4x4s2_split_kernel<16, 32, 32, 1, 2, 2, false>, conv_enc_split.hip) the map — 64 KB per frame, 84 MB for the 1280 frames of a
// c2 trajectory batch — is written to HBM and read back only because the layers are two kernels.  Here a persistent workgroup loops
// over its frames; per frame
//   1. the image planes are in LDS in the layout of conv4x4s2_image_lds_kernel (zero border stored);
//   2. the map is formed with that kernel's products in that kernel's order — mfma16 over (ci, ky), bias, LeakyReLU — and written as
//      f32 straight into the frame layout of conv4x4s2_split_kernel (80 bytes per pixel); the frame's largest magnitude is taken
//      while the values are in registers, and the map is stored to HBM as well when the caller has a reader for it;
//   3. from there on the steps of conv4x4s2_split_kernel: power-of-two scale, in-place conversion to two f16 pieces, 8 k-steps x 3
//      MFMAs per accumulator in the same order, the same epilogue.  Every value is bit-identical to the two launches.
// The two regions together are 139 KB: one workgroup, one wavefront per SIMD, per CU — nothing else is resident to overlap with.  The
// 16 -> 32 weight fragments of a wavefront (64 VGPRs) and both biases stay in registers for the whole launch, and the first layer reads
// the operands of four pixel groups before their MFMAs.  A form that requested the NEXT frame's image into registers at the top of a
// frame and stored it into the image region (dead once the map is formed) behind the MFMA phase measured 68.5 against 70.4 us for the
// 1280-frame pass with overlapping ranges (profiles/enc_fused.txt): not kept, the frame's image is staged at the top of its iteration.
// BatchNorm partial sums: row f of stats_partial holds frame f alone, reduced as conv4x4s2_split_kernel reduces its one-frame
// workgroups (F <= rows, which the launch requires), so the rows are those of the two launches; rows from F on are zeroed.
#include "common.h"

#include <cstdlib>

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma32h(h8 a, h8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

struct EncFusedCfg {
    static constexpr int HIMG = 64, HIN = 32, HOUT = 16, CIN = 16, COUT = 32, CT = 2;
    static constexpr int WP = 2, WC = 2, PGW = 8, NSTEP = 8;            // as EncSplitCfg<16, 32, 32, 1, 2, 2, false>
    static constexpr int PIXB = CIN * 4 + 16, FRAME_PIX = HIN * HIN, FRAME_BYTES = FRAME_PIX * PIXB;
    static constexpr int PITCH = HIMG + 8, ROWS = HIMG + 2, PLANE = ROWS * PITCH, IMG_BYTES = 3 * PLANE * 4;      // as ImgLdsCfg<64>
    static constexpr int RED_BYTES = WP * 2 * COUT * 4;
    static constexpr int LDS_BYTES = FRAME_BYTES + IMG_BYTES + RED_BYTES;
    static constexpr int F4 = 3 * HIMG * HIMG / 4, NPF = F4 / 256;      // float4 of an image, per thread
    static_assert(FRAME_BYTES == 81920 && IMG_BYTES == 57024 && F4 % 256 == 0 && LDS_BYTES <= 160 * 1024, "layout");
};

// A0: the map is stored to a0_out as well; STATS: a.stats_partial is set
template <bool A0, bool STATS>
__global__ void __launch_bounds__(256) conv4x4s2_image_fused_kernel(const float* __restrict__ x, const float* __restrict__ w0pk,
                                                                    const float* __restrict__ bias0, const int act0,
                                                                    float* __restrict__ a0_out, const gcpx_conv_args a, const int nrows) {
    using Cfg = EncFusedCfg;
    constexpr int HIMG = Cfg::HIMG, HIN = Cfg::HIN, HOUT = Cfg::HOUT, COUT = Cfg::COUT, CT = Cfg::CT, WP = Cfg::WP, PGW = Cfg::PGW;
    constexpr int PIXB = Cfg::PIXB, FRAME_PIX = Cfg::FRAME_PIX, NSTEP = Cfg::NSTEP, PITCH = Cfg::PITCH, PLANE = Cfg::PLANE;
    constexpr int F4 = Cfg::F4, NPF = Cfg::NPF;
    extern __shared__ float4 encf_smem4[];
    char* lds = reinterpret_cast<char*>(encf_smem4);                                // the 32 x 32 x 16 map, then its two f16 pieces
    float* img = reinterpret_cast<float*>(lds + Cfg::FRAME_BYTES);                  // three planes of the 64 x 64 image
    float* red = reinterpret_cast<float*>(lds + Cfg::FRAME_BYTES + Cfg::IMG_BYTES); // [WP][2][COUT]
    float* wmax = reinterpret_cast<float*>(lds + Cfg::CIN * 4);                     // the 4 per-wavefront maxima: pad bytes of pixel 0
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave % WP, wc = wave / WP;
    const int j = lane & 15, q = lane >> 4;
    const int F = a.F, G = gridDim.x;
    // LeakyReLU or nothing, without a branch: x > 0 ? x : x * 1 is x
    const float slope0 = act0 == GCPX_ACT_LRELU ? 0.2f : 1.f, slope1 = a.out_act == GCPX_ACT_LRELU ? 0.2f : 1.f;

    // zero border of the image planes: rows 0 and HIMG + 1, columns 3 and HIMG + 4 of every row (written once: staging never touches them)
    for (int i = tid; i < 3 * 2 * PITCH; i += 256) {
        const int pl = i / (2 * PITCH), r = (i / PITCH) % 2, c = i % PITCH;
        img[pl * PLANE + (r ? HIMG + 1 : 0) * PITCH + c] = 0.f;
    }
    for (int i = tid; i < 3 * Cfg::ROWS * 2; i += 256) {
        const int pl = i / (Cfg::ROWS * 2), r = (i / 2) % Cfg::ROWS, c = (i & 1) ? HIMG + 4 : 3;
        img[pl * PLANE + r * PITCH + c] = 0.f;
    }
    // rows of stats_partial without a frame
    if (STATS && tid < 2 * COUT)
        for (int r = F + (int)blockIdx.x; r < nrows; r += G) a.stats_partial[(size_t)r * 2 * COUT + tid] = 0.f;

    // operands that stay in registers for the whole launch: both layers' weight fragments and biases
    float w0[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) w0[t] = w0pk[t * 64 + lane];
    const float4 bv0 = *reinterpret_cast<const float4*>(bias0 + q * 4);
    // packed pieces of the second layer: [NSTEP][CT][2][64] x 16 B
    h8 w1[NSTEP][2];
    {
        const char* wbase = reinterpret_cast<const char*>(a.wpk_split) + (size_t)wc * 2048 + lane * 16;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            w1[s][0] = *reinterpret_cast<const h8*>(wbase + (size_t)s * CT * 2048);
            w1[s][1] = *reinterpret_cast<const h8*>(wbase + (size_t)s * CT * 2048 + 1024);
        }
    }
    const int c1 = wc * 16 + q * 4;                         // this lane's 4 output channels of the second layer
    const float4 bv1 = *reinterpret_cast<const float4*>(a.bias + c1);
    const int ew = a.w_split_log2_dev ? __builtin_amdgcn_readfirstlane(*a.w_split_log2_dev) : a.w_split_log2;

    // per pixel group of this wavefront: byte offset of input pixel (2 oy - 1, 2 ox - 1), tap validity (bit ky: row, bit 4 + kx: column)
    int base[PGW], pin_[PGW];
    unsigned vmask[PGW];
#pragma unroll
    for (int pt = 0; pt < PGW; ++pt) {
        const int pin = (wp + pt * WP) * 16 + j;
        const int oy = pin / HOUT, ox = pin % HOUT;
        pin_[pt] = pin;
        base[pt] = ((2 * oy - 1) * HIN + 2 * ox - 1) * PIXB;
        unsigned m = 0;
        for (int k = 0; k < 4; ++k) {
            if (2 * oy - 1 + k >= 0 && 2 * oy - 1 + k < HIN) m |= 1u << k;
            if (2 * ox - 1 + k >= 0 && 2 * ox - 1 + k < HIN) m |= 16u << k;
        }
        vmask[pt] = m;
    }

    auto img_off = [&](const int i) __attribute__((always_inline)) {           // float offset of float4 i of a frame in the planes
        const int pl = i / (HIMG * HIMG / 4), rem = i % (HIMG * HIMG / 4);
        const int y = rem / (HIMG / 4), x4 = rem % (HIMG / 4);
        return pl * PLANE + (y + 1) * PITCH + 4 + 4 * x4;
    };
    const f32x4* x4p = reinterpret_cast<const f32x4*>(x);
    // every load above has landed: inside the loop nothing then waits on the previous frame's stores for the sake of these registers
    __builtin_amdgcn_s_waitcnt(0x0f70);                     // vmcnt(0)

    for (int f = blockIdx.x; f < F; f += G) {
        {
            // the frame's image (f32x4, a native vector type: an array of float4 structs is copied through scratch)
            const f32x4* src = x4p + (size_t)f * F4;
            f32x4 v[NPF];
#pragma unroll
            for (int k = 0; k < NPF; ++k) v[k] = src[k * 256 + tid];
#pragma unroll
            for (int k = 0; k < NPF; ++k) *reinterpret_cast<f32x4*>(img + img_off(k * 256 + tid)) = v[k];
        }
        __syncthreads();                                    // the image is staged (the previous frame's operand reads were done at its end)

        // first layer: same products in the same order as conv4x4s2_image_lds_kernel; lane (j, q) of k-step (ci, ky) reads
        // x[ci][2 oy - 1 + ky][2 ox_j - 1 + q] = row 2 oy + ky, column 3 + 2 ox + q of plane ci
        // Four pixel groups at a time, their 48 operands read before the first MFMA: with one wavefront per SIMD nothing else covers
        // an LDS latency, and the four accumulators are independent chains
        float amax = 0.f;
#pragma unroll
        for (int gi = 0; gi < FRAME_PIX / 64; gi += 4) {
            float b[4][12];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = ((gi + u) * 4 + wave) * 16 + j;
                const int oy = p / HIN, ox = p % HIN;
                const float* bp = img + (2 * oy) * PITCH + 3 + 2 * ox + q;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                    for (int ky = 0; ky < 4; ++ky) b[u][ci * 4 + ky] = bp[ci * PLANE + ky * PITCH];
            }
            f32x4 acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 12; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = mfma16(w0[t], b[u][t], acc[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = ((gi + u) * 4 + wave) * 16 + j;
                f32x4 v = acc[u];
                v[0] += bv0.x; v[1] += bv0.y; v[2] += bv0.z; v[3] += bv0.w;
                v[0] = lrelu(v[0], slope0); v[1] = lrelu(v[1], slope0); v[2] = lrelu(v[2], slope0); v[3] = lrelu(v[3], slope0);
                *reinterpret_cast<f32x4*>(lds + p * PIXB + 16 * q) = v;
                if constexpr (A0) *reinterpret_cast<f32x4*>(a0_out + ((size_t)f * FRAME_PIX + p) * 16 + q * 4) = v;
                amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
        if (lane == 0) wmax[wave] = amax;
        __syncthreads();                                    // the map is complete; the image region is dead
        amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        int ex = 14 + 127 - (int)((__float_as_uint(amax) >> 23) & 0xff);            // amax 2^ex in [2^14, 2^15)
        ex = __builtin_amdgcn_readfirstlane(amax > 0.f ? max(-100, min(min(100, 126 - ew), ex)) : min(100, 126 - ew));
        const float sx2 = __uint_as_float((unsigned)(127 + ex) << 23);
        // in place: 8 consecutive channels of a pixel (32 B of f32) -> [8 first pieces | 8 second pieces]
#pragma unroll
        for (int i = tid; i < FRAME_PIX * 2; i += 256) {
            const int c8 = i % 2, pix = i / 2;
            char* p = lds + pix * PIXB + 32 * c8;
            const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 16);
            const float fv[8] = {v0.x * sx2, v0.y * sx2, v0.z * sx2, v0.w * sx2, v1.x * sx2, v1.y * sx2, v1.z * sx2, v1.w * sx2};
            h8 p1, p2;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p1[e] = (_Float16)fv[e];
                p2[e] = (_Float16)fmaf((float)p1[e], -1.f, fv[e]);
            }
            *reinterpret_cast<h8*>(p) = p1;
            *reinterpret_cast<h8*>(p + 16) = p2;
        }
        __syncthreads();

        f32x4 acc[PGW];
#pragma unroll
        for (int pt = 0; pt < PGW; ++pt) acc[pt] = f32x4{0, 0, 0, 0};
        // k-step s of lane (j, q): tap 2 s + (q >> 1), 8-channel group q & 1.  An out-of-image tap reads pixel 0 and is replaced by zero
        auto load_b = [&](const int step, h8 (&b)[PGW][2]) __attribute__((always_inline)) {
            const int tap = 2 * step + (q >> 1), grp = q & 1;
            const int ky = tap >> 2, kx = tap & 3;
            const int tapoff = (ky * HIN + kx) * PIXB + grp * 32;
#pragma unroll
            for (int pt = 0; pt < PGW; ++pt) {
                const bool ok = ((vmask[pt] >> ky) & 1u) && ((vmask[pt] >> (4 + kx)) & 1u);
                const char* p = lds + (ok ? base[pt] + tapoff : 0);
                const h8 t0 = *reinterpret_cast<const h8*>(p), t1 = *reinterpret_cast<const h8*>(p + 16);
                const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                b[pt][0] = ok ? t0 : z;
                b[pt][1] = ok ? t1 : z;
            }
        };
        // small terms first: they are added to the accumulator while it is still small
        auto mm = [&](const int step, const h8 (&b)[PGW][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int pt = 0; pt < PGW; ++pt) acc[pt] = mfma32h(w1[step][1], b[pt][0], acc[pt]);
#pragma unroll
            for (int pt = 0; pt < PGW; ++pt) acc[pt] = mfma32h(w1[step][0], b[pt][1], acc[pt]);
#pragma unroll
            for (int pt = 0; pt < PGW; ++pt) acc[pt] = mfma32h(w1[step][0], b[pt][0], acc[pt]);
        };
        // two operand sets in ping-pong: the LDS reads of step s + 1 are in flight during the 24 MFMAs of step s
        h8 bA[PGW][2], bB[PGW][2];
        load_b(0, bA);
#pragma unroll
        for (int step = 0; step < NSTEP; step += 2) {
            load_b(step + 1, bB);
            mm(step, bA);
            if (step + 2 < NSTEP) load_b(step + 2, bA);
            mm(step + 1, bB);
        }
        const float inv = __uint_as_float((unsigned)(127 - ex - ew) << 23);
        f32x4 st1 = f32x4{0, 0, 0, 0}, st2 = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int pt = 0; pt < PGW; ++pt) {
            float* op = a.out + ((size_t)f * HOUT * HOUT + pin_[pt]) * COUT;
            f32x4 v = acc[pt];
            v[0] = fmaf(v[0], inv, bv1.x); v[1] = fmaf(v[1], inv, bv1.y); v[2] = fmaf(v[2], inv, bv1.z); v[3] = fmaf(v[3], inv, bv1.w);
            v[0] = lrelu(v[0], slope1); v[1] = lrelu(v[1], slope1); v[2] = lrelu(v[2], slope1); v[3] = lrelu(v[3], slope1);
            *reinterpret_cast<f32x4*>(op + c1) = v;
            if constexpr (STATS) {
                // explicit FMAs in frame order: conv4x4s2_split_kernel's `st2 += v * v` across its loop compiles to this chain, and a
                // contraction the compiler is free to choose here (which product of v0 v0 + v1 v1 is fused) would change the last bit
                st1 += v;
#pragma unroll
                for (int r = 0; r < 4; ++r) st2[r] = fmaf(v[r], v[r], st2[r]);
            }
        }
        if constexpr (STATS) {
            // the frame's partial sums: lanes of a row, then the WP wavefronts that share channels
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s1 = row16_sum(st1[r]);
                const float s2 = row16_sum(st2[r]);
                if (j == 0) {
                    red[(wp * 2 + 0) * COUT + c1 + r] = s1;
                    red[(wp * 2 + 1) * COUT + c1 + r] = s2;
                }
            }
        }
        __syncthreads();                                    // this frame's operand reads and sums are done
        if (STATS && tid < 2 * COUT) {
            const int which = tid / COUT, c = tid % COUT;
            float sum = 0.f;
#pragma unroll
            for (int w_ = 0; w_ < WP; ++w_) sum += red[(w_ * 2 + which) * COUT + c];
            a.stats_partial[((size_t)f * 2 + which) * COUT + c] = sum;
        }
    }
}

bool fused_shape_ok(const gcpx_conv_args* a, int Himg, int Wimg) {
    return a && Himg == 64 && Wimg == 64 && a->nsrc == 1 && a->src[0].frame_div == 1 && a->src[0].C == 16 && !a->src[0].scale &&
           !a->src[0].shift && a->src[0].act == GCPX_ACT_NONE && a->Cin == 16 && a->Cout == 32 && a->out_pitch == 32 && a->Hin == 32 &&
           a->Win == 32 && a->Hout == 16 && a->Wout == 16 && a->wpk_split && a->split_layout == GCPX_SPLIT_PLAIN && a->F > 0 &&
           a->F <= gcpx_conv4x4s2_grid() && !a->src_row_map && !a->addend;
}

}  // namespace

extern "C" int gcpx_conv4x4s2_image_fused_grid(void) { return gcpx_conv_grid() / 2; }

extern "C" int gcpx_conv4x4s2_image_fused_supported(const gcpx_conv_args* a, int32_t Himg, int32_t Wimg) {
    return fused_shape_ok(a, Himg, Wimg) ? 1 : 0;
}

extern "C" int gcpx_conv4x4s2_image_fused(const float* x, const float* w0pk, const float* bias0, int32_t act0, float* a0_out,
                                          const gcpx_conv_args* a, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(a != nullptr && x && w0pk && bias0, "null pointer");
    GCPX_CHECK_ARG(fused_shape_ok(a, 64, 64), "not a problem gcpx_conv4x4s2_image_fused_supported accepts");
    GCPX_CHECK_ARG(a->bias && a->out, "null bias / out");
    GCPX_CHECK_ARG(act0 == GCPX_ACT_NONE || act0 == GCPX_ACT_LRELU, "act0 must be NONE or LRELU");
    using Cfg = EncFusedCfg;
    const int form = (a0_out ? 1 : 0) + (a->stats_partial ? 2 : 0);
    const auto kern = form == 0 ? conv4x4s2_image_fused_kernel<false, false> : form == 1 ? conv4x4s2_image_fused_kernel<true, false>
                    : form == 2 ? conv4x4s2_image_fused_kernel<false, true> : conv4x4s2_image_fused_kernel<true, true>;
    static bool attr_set[4] = {false, false, false, false};
    if (!attr_set[form]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
        if (e != hipSuccess) {
            gcpx_set_error("conv4x4s2 image (fused): hipFuncSetAttribute(%d B): %s", Cfg::LDS_BYTES, hipGetErrorString(e));
            return GCPX_ERR_HIP;
        }
        attr_set[form] = true;
    }
    int grid = gcpx_conv4x4s2_image_fused_grid();
    if (grid > a->F) grid = a->F;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), Cfg::LDS_BYTES, stream, x, w0pk, bias0, act0, a0_out, *a, gcpx_conv4x4s2_grid());
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
