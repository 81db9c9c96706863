// The whole inference-mode encoder of one frame inside one workgroup: gcpx_encode_frames.
//
// Encoder.forward with running BatchNorm statistics (oracle/gcp_model_oracle.py: encoder, training=False) as the closed-loop policy
// calls it at gcp/planning/planner_policy.py:222-227 of the reference, for F frames in one launch.  The conv blocks of conv_enc*.hip
// share one power-of-two scale among the frames a workgroup stages (conv_enc_split.hip), so their result for a frame depends on its
// batch-mates in the last bits.  Here a frame's latent depends on that frame and the weights only:
//   * one workgroup (4 wavefronts) owns one frame from the image to the latent and strides over the grid when F exceeds it;
//   * exact f32: f32 operands, f32 accumulation (v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain; plain fmaf in the first layer, K = 48,
//     and in the head, one output row);
//   * the summation order of every output value is a function of (layer, pixel, channel) alone: which wavefront computes a tile, the
//     frame's index, F and the grid size do not enter it.
// Activations live in LDS in two regions used in turn (NHWC maps, C + 4 floats per pixel) and never go to global memory:
//   region 0: the staged NCHW frame -> pyramid-0's map -> (64 x 64: pyramid-2's map)
//   region 1: the input layer's map -> pyramid-1's map
//   32 x 32: 12 KB + 20 KB;  64 x 64: 48 KB + 80 KB = 128 KB of the CU's 160 KB (dynamic LDS, limit raised at the first launch).
// Weights come from global memory (the blob of packing.pack_encoder_frames, 0.7 MB at 32 x 32 / nz_enc 128, 1.7 MB at 64 x 64), in
// fragment order for the MFMA layers; they stay in L2 across the workgroups.
// Out-of-image taps contribute zeros and are never formed into an address; frames at or beyond F are never read or written.
#include "common.h"

namespace {

constexpr int NGF = 16;

// float offsets inside the blob (video-gcp_amd/packing.py: encoder_frames_layout is the same arithmetic)
//   input    w [48 (ci, ky, kx)][16], bias [16]
//   pyramid  w [16 taps][Cin/16][Cout/16][64][4] (packing.pack_conv4x4), bias, scale, shift [Cout]
//   head     w [nz][16 c_top (y, x, c)], bias [nz]
constexpr int IN_FLOATS = 48 * NGF + NGF;
constexpr int pyr_floats(int cin) { return 16 * cin * 2 * cin + 3 * 2 * cin; }
constexpr int pyr_off(int i) { return i == 0 ? IN_FLOATS : pyr_off(i - 1) + pyr_floats(NGF << (i - 1)); }

template <int S>
struct EncFramesCfg {
    static constexpr int NPYR = S == 64 ? 3 : 2;
    static constexpr int CTOP = NGF << NPYR;
    static constexpr int R0 = 3 * S * S;                           // floats of region 0: the frame
    static constexpr int R1 = (S / 2) * (S / 2) * (NGF + 4);       // floats of region 1: the input layer's map
    static constexpr int LDS_BYTES = (R0 + R1) * 4;
    static constexpr int HEAD_OFF = pyr_off(NPYR);
    static_assert((S / 4) * (S / 4) * (2 * NGF + 4) <= R0 && (S / 8) * (S / 8) * (4 * NGF + 4) <= R1 && 16 * (CTOP + 4) <= R0, "regions");
};

// input: 4x4, stride 2, pad 1, 3 -> 16, bias, LeakyReLU on plain FMAs (K = 48 does not pay an MFMA tile's set-up).  Thread (c = tid & 15,
// tid >> 4) owns channel c of every 16th pixel: its 48 weights w[k][c] stay in registers over all frames (w48), and an output value is ONE
// fmaf chain over k = (ci, ky, kx).  The 16 lanes of a pixel read the same LDS word (a broadcast).
template <int S>
__device__ __forceinline__ void input_layer(const float* __restrict__ img, float* __restrict__ omap, const float (&w48)[48], const float bias,
                                            const float slope, const int tid) {
    constexpr int HO = S / 2, CP = NGF + 4;
    const int c = tid & 15;
#pragma unroll 1
    for (int p = tid >> 4; p < HO * HO; p += 16) {
        const int oy = p / HO, ox = p % HO;
        float acc = 0.f;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
                const int iy = 2 * oy - 1 + ky;
                const bool rok = iy >= 0 && iy < S;
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    const int ix = 2 * ox - 1 + kx;
                    const bool ok = rok && ix >= 0 && ix < S;
                    const float v = img[ok ? (ci * S + iy) * S + ix : 0];
                    acc = fmaf(ok ? v : 0.f, w48[(ci * 4 + ky) * 4 + kx], acc);      // conv zero padding stays exactly zero
                }
            }
        }
        omap[p * CP + c] = lrelu(acc + bias, slope);
    }
}

// pyramid-i: 4x4, stride 2, pad 1, CIN -> COUT = 2 CIN on f32 MFMA tiles of 16 pixels x 16 channels, K = 16 CIN in the order
// (tap, channel); then + bias, fmaf(raw, scale, shift), LeakyReLU.  The COUT / 16 channel tiles go over WC wavefronts, the pixel groups
// over the other WP: a weight fragment fetched once feeds the PGW pixel groups of its wavefront.
template <int CIN, int HIN>
__device__ __forceinline__ void pyramid_layer(const float* __restrict__ imap, float* __restrict__ omap, const float* __restrict__ wl,
                                              const float slope, const int lane, const int wave) {
    constexpr int COUT = 2 * CIN, HOUT = HIN / 2, NG = HOUT * HOUT / 16, CT = COUT / 16, NCG = CIN / 16, CINP = CIN + 4, COUTP = COUT + 4;
    constexpr int WC = CT < 4 ? CT : 4, WP = 4 / WC, CTW = CT / WC, PGW = NG / WP;
    static_assert((HOUT * HOUT) % 16 == 0 && NG % WP == 0 && PGW >= 1 && CT % WC == 0, "tiling");
    const int wc = wave % WC, wp = wave / WC;
    const int j = lane & 15, q = lane >> 4;
    const float4* wbase = reinterpret_cast<const float4*>(wl) + wc * CTW * 64 + lane;
    const float* bias = wl + 16 * CIN * COUT;
    const float* scale = bias + COUT;
    const float* shift = scale + COUT;

    // per pixel group of this wavefront: offset of input pixel (2 oy - 1, 2 ox - 1) + this lane's 4-channel slice (used only where the
    // tap is inside the image), tap validity (bit ky: row, bit 4 + kx: column)
    int base[PGW], pix[PGW];
    unsigned vmask[PGW];
#pragma unroll
    for (int pt = 0; pt < PGW; ++pt) {
        const int p = (wp * PGW + pt) * 16 + j;
        const int oy = p / HOUT, ox = p % HOUT;
        pix[pt] = p;
        base[pt] = ((2 * oy - 1) * HIN + 2 * ox - 1) * CINP + 4 * q;
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (2 * oy - 1 + k >= 0 && 2 * oy - 1 + k < HIN) m |= 1u << k;
            if (2 * ox - 1 + k >= 0 && 2 * ox - 1 + k < HIN) m |= 16u << k;
        }
        vmask[pt] = m;
    }
    f32x4 acc[CTW][PGW];
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
        for (int pt = 0; pt < PGW; ++pt) acc[ct][pt] = f32x4{0, 0, 0, 0};

#pragma unroll 1
    for (int ky = 0; ky < 4; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const int tapoff = (ky * HIN + kx) * CINP;
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) {
                float4 w[CTW], b[PGW];
                const float4* wp_ = wbase + (((ky * 4 + kx) * NCG + cg) * CT) * 64;
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) w[ct] = wp_[ct * 64];
#pragma unroll
                for (int pt = 0; pt < PGW; ++pt) {
                    const bool ok = ((vmask[pt] >> ky) & 1u) && ((vmask[pt] >> (4 + kx)) & 1u);
                    const float4 t = *reinterpret_cast<const float4*>(imap + (ok ? base[pt] + tapoff + cg * 16 : 4 * q));
                    b[pt] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
#pragma unroll
                    for (int pt = 0; pt < PGW; ++pt) {
                        acc[ct][pt] = mfma16(w[ct].x, b[pt].x, acc[ct][pt]);
                        acc[ct][pt] = mfma16(w[ct].y, b[pt].y, acc[ct][pt]);
                        acc[ct][pt] = mfma16(w[ct].z, b[pt].z, acc[ct][pt]);
                        acc[ct][pt] = mfma16(w[ct].w, b[pt].w, acc[ct][pt]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct) {
        const int c = (wc * CTW + ct) * 16 + q * 4;
        const float4 bv = *reinterpret_cast<const float4*>(bias + c);
        const float4 sc = *reinterpret_cast<const float4*>(scale + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c);
#pragma unroll
        for (int pt = 0; pt < PGW; ++pt) {
            const f32x4 v = acc[ct][pt];
            *reinterpret_cast<float4*>(omap + pix[pt] * COUTP + c) =
                make_float4(lrelu(fmaf(v[0] + bv.x, sc.x, sh.x), slope), lrelu(fmaf(v[1] + bv.y, sc.y, sh.y), slope),
                            lrelu(fmaf(v[2] + bv.z, sc.z, sh.z), slope), lrelu(fmaf(v[3] + bv.w, sc.w, sh.w), slope));
        }
    }
}

// head: 4x4 valid over the 4 x 4 x CTOP map + bias = one row of K = 16 CTOP products per output channel.  The 64 lanes of a wavefront
// split K (lane l: k = l, l + 64, ... in one fmaf chain), then one xor butterfly 32, 16, ... 1; a wavefront takes 4 channels at a time.
template <int CTOP>
__device__ __forceinline__ void head_layer(const float* __restrict__ imap, const float* __restrict__ wl, float* __restrict__ orow,
                                           const int nz, const int lane, const int wave) {
    constexpr int K = 16 * CTOP, CP = CTOP + 4, NI = K / 64;
    float a[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int k = lane + 64 * i;
        a[i] = imap[(k / CTOP) * CP + k % CTOP];
    }
    const float* bias = wl + (size_t)nz * K;
    for (int g = wave; g < nz / 4; g += 4) {
        const float* wr = wl + (size_t)g * 4 * K + lane;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] = fmaf(a[i], wr[c * K + 64 * i], s[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s[c] += __shfl_xor(s[c], d);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) orow[g * 4 + c] = s[c] + bias[g * 4 + c];
        }
    }
}

template <int S>
__global__ void __launch_bounds__(256) encode_frames_kernel(const float* __restrict__ x, const float* __restrict__ blob, float* __restrict__ out,
                                                            const long long out_stride, const int F, const int nz, const float slope) {
    using Cfg = EncFramesCfg<S>;
    extern __shared__ float4 encf_smem4[];
    float* r0 = reinterpret_cast<float*>(encf_smem4);
    float* r1 = r0 + Cfg::R0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int F4 = 3 * S * S / 4;
    float w48[48];                                              // the input layer's weights of this thread's channel
#pragma unroll
    for (int k = 0; k < 48; ++k) w48[k] = blob[k * NGF + (tid & 15)];
    const float b_in = blob[48 * NGF + (tid & 15)];
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        __syncthreads();                                        // the previous frame's reads of both regions are done
        const float4* src = reinterpret_cast<const float4*>(x) + (size_t)f * F4;
        for (int i = tid; i < F4; i += 256) reinterpret_cast<float4*>(r0)[i] = src[i];
        __syncthreads();
        input_layer<S>(r0, r1, w48, b_in, slope, tid);
        __syncthreads();
        pyramid_layer<NGF, S / 2>(r1, r0, blob + pyr_off(0), slope, lane, wave);
        __syncthreads();
        pyramid_layer<2 * NGF, S / 4>(r0, r1, blob + pyr_off(1), slope, lane, wave);
        __syncthreads();
        float* orow = out + (size_t)f * out_stride;
        if constexpr (S == 64) {
            pyramid_layer<4 * NGF, S / 8>(r1, r0, blob + pyr_off(2), slope, lane, wave);
            __syncthreads();
            head_layer<Cfg::CTOP>(r0, blob + Cfg::HEAD_OFF, orow, nz, lane, wave);
        } else {
            head_layer<Cfg::CTOP>(r1, blob + Cfg::HEAD_OFF, orow, nz, lane, wave);
        }
    }
}

template <int S>
int launch_encode_frames(const float* x, const float* blob, float* out, long long out_stride, int F, int nz, float slope,
                         hipStream_t stream) {
    using Cfg = EncFramesCfg<S>;
    auto kern = encode_frames_kernel<S>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
        if (e != hipSuccess) {
            gcpx_set_error("encode_frames: hipFuncSetAttribute(%d B): %s", Cfg::LDS_BYTES, hipGetErrorString(e));
            return GCPX_ERR_HIP;
        }
        attr_set = true;
    }
    int grid = gcpx_conv_grid() / 2 * (160 * 1024 / Cfg::LDS_BYTES);      // as many workgroups as fit the CUs' LDS at once
    if (grid > F) grid = F;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), Cfg::LDS_BYTES, stream, x, blob, out, out_stride, F, nz, slope);
    return GCPX_OK;
}

}  // namespace

extern "C" int gcpx_encode_frames(const float* images, const float* weights, float* out, int64_t out_stride, int32_t F, int32_t S,
                                  int32_t ngf, int32_t nz_enc, float leaky_slope, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(images && weights && out, "null pointer");
    GCPX_CHECK_ARG(F > 0, "F <= 0");
    GCPX_CHECK_ARG(S == 32 || S == 64, "unsupported image size: S must be 32 or 64");
    GCPX_CHECK_ARG(ngf == NGF, "unsupported width: ngf must be 16");
    GCPX_CHECK_ARG(nz_enc > 0 && nz_enc <= 256 && nz_enc % 16 == 0, "unsupported latent width: nz_enc must be a multiple of 16, at most 256");
    GCPX_CHECK_ARG(out_stride >= nz_enc, "out_stride < nz_enc");
    GCPX_CHECK_ARG(((uintptr_t)images & 15) == 0 && ((uintptr_t)weights & 15) == 0, "images and weights must be 16-byte aligned");
    const int st = S == 64 ? launch_encode_frames<64>(images, weights, out, out_stride, F, nz_enc, leaky_slope, stream)
                           : launch_encode_frames<32>(images, weights, out, out_stride, F, nz_enc, leaky_slope, stream);
    if (st != GCPX_OK) return st;
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
