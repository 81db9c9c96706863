// Low-resolution decoder up-blocks (pyramid-2: 128 -> 64 @4x4 -> 8x8, pyramid-1: 64 (+ 64) -> 32 @8x8 -> 16x16) in split-f16 with the tap
// products taken BEFORE the bilinear x2 (GCPX_SPLIT_LOWRES).  The upsample acts on space only, a conv tap mixes channels only:
//
//     out[co, p] = b[co] + sum_t 1[p + t inside] Up(Y_t)[co, p + t],      Y_t = W_t x      (a 1x1 conv on the SOURCE grid)
//
// so the nine Y_t run on the f16 matrix pipe at source resolution — a quarter of the MFMAs of conv3x3_up32_split_kernel — and the
// interpolation + 3x3 shift-sum run on Cout channels in f32 VALU, separably:
//
//     Z_ty[sy, px] = sum_tx 1[px + tx inside] sum_sx ux(px + tx, sx) Y_(ty,tx)[sy, sx]          (6 FMA per value)
//     out[py, px]  = b + sum_ty 1[py + ty inside] sum_sy uy(py + ty, sy) Z_ty[sy, px]          (6 FMA per value)
//
// Both stages are register-tiled in half-runs (half_run below): a thread reads the Hin / 2 + 1 source samples that one half of an output
// row (column) depends on, for the three taps, ONCE — 3 (Hin / 2 + 1) - 1 float4 from LDS — and forms the Hin adjacent outputs of that
// half from registers: 14 reads for 8 values at Hin = 8, 8 for 4 at Hin = 4, where one value at a time took 6 reads each.  The second
// half of a row is the mirror image of the first (x -> W - 1 - x, tx -> 2 - tx), so both run the same code with the border rules and
// bilinear weights folded at compile time; only the base address and the sign of the stride differ per thread.
//
// One unit of work = one frame (two at 4x4: 32 source pixels).  A workgroup has 3 CT wavefronts; wavefront (tx, ct) owns the three (ty, tx) taps of channel tile ct
// and keeps their A fragments — the PLAIN up32 pack, [chunk][tap][CT][2][64] x 16 B — in registers for the whole persistent loop: no
// weight traffic after the prologue.  The B fragments (the frame's activations, two f16 planes per 32-channel chunk) come from LDS and
// each serves nine MFMAs.  One power-of-two scale per (frame, chunk), following the chunks with the exact accumulator rescale of
// conv3x3_up32_split_kernel: the bound of split_mfma.h holds per frame.
#include "common.h"
#include "split_mfma.h"

namespace {

template <int CT, int HIN, int NCHUNK, int FPU>
struct LowresCfg {
    static constexpr int NW = 3 * CT, NT = NW * 64;
    static constexpr int NPIX = HIN * HIN, UPIX = FPU * NPIX, NPG = UPIX / 16, WOUT = 2 * HIN, HOUT = 2 * HIN;
    static constexpr int COUT = CT * 16, CIN = NCHUNK * 32, C4 = COUT / 4, Q4 = CIN / 4;
    static constexpr int YS = COUT + 4;                                        // floats per pixel of Y: + 4 keeps the MFMA lanes' stores off each other's banks
    static constexpr int PLANE_BYTES = UPIX * 64;                              // one f16 piece of one chunk: 32 channels x 2 B per pixel
    static constexpr int PLANES_BYTES = NCHUNK * 2 * PLANE_BYTES;
    static constexpr int Y_BYTES = 9 * UPIX * YS * 4;                          // [tap][unit pixel][YS] f32
    static constexpr int Z_BYTES = FPU * 3 * HIN * WOUT * COUT * 4;            // [frame][ty][source row][output column][COUT] f32
    static constexpr int PZ_BYTES = PLANES_BYTES > Z_BYTES ? PLANES_BYTES : Z_BYTES;      // the planes are dead when Z is written: one region
    static constexpr int TAB_BYTES = (2 * CIN + COUT) * 4;                     // BatchNorm scale / shift per input channel, bias
    static constexpr int STAT_BYTES = NT * 8 * 4;                              // a thread's running sum / sum of squares of its channel quad
    static constexpr int LDS_BYTES = PZ_BYTES + Y_BYTES + 64 + TAB_BYTES + STAT_BYTES;      // (64: the chunk maxima)
    static constexpr int NSLOT = UPIX * Q4;                                    // float4 staging slots of a unit
    static constexpr int NS = (NSLOT + NT - 1) / NT;
    // half-runs: a row of Z is two runs of HIN output columns, a column of the output two runs of HIN output rows
    static constexpr int NH = 2 * FPU * 3 * HIN * C4;                          // half-runs of the horizontal stage: one per thread
    static constexpr int NV = 2 * FPU * WOUT * C4;                             // half-runs of the vertical stage: the first 2/3 of the threads
    static_assert(NT % C4 == 0 && NT % Q4 == 0, "a thread keeps one channel quad of the input and one of the output");
    static_assert(NH == NT && NV <= NT && NV % 64 == 0, "one horizontal half-run per thread; whole wavefronts in the vertical stage");
    static_assert(NV * HIN * 16 <= Y_BYTES, "a finished unit may wait in the Y buffer");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// sources and weights of the bilinear x2 (align_corners = False) at output index h of an axis with n source samples
__device__ __forceinline__ void up_taps(const int h, const int n, int& s0, int& s1, float& w0, float& w1) {
    const int s = h >> 1;
    const bool odd = h & 1;
    s0 = odd ? s : max(s - 1, 0);
    s1 = odd ? min(s + 1, n - 1) : s;
    w0 = odd ? 0.75f : 0.25f;
    w1 = 1.f - w0;
}

// One half-run of either interpolation stage, in the half's own coordinates (outputs r = 0 .. HIN - 1 from its border inwards):
//     o[r] = sum_k 1[r + k - 1 >= 0] (w0 L_k[s0] + w1 L_k[s1]),   (s0, s1, w0, w1) = up_taps(r + k - 1)
// p[k] points at sample 0 of tap k (the mirrored half passes tap 2 - k and its last sample), ss is the stride between samples in
// floats (negative in the mirrored half).  r + k - 1 <= HIN stays inside the axis, so only the near border clamps; sample HIN / 2 of
// tap 0 is never used.  Everything but the addresses folds at compile time.
// TAPWISE (the instances with 96 registers of resident weights): one tap's samples in registers at a time, not all three.
template <int HIN, bool TAPWISE>
__device__ __forceinline__ void half_run(const float* const (&p)[3], const int ss, float4 (&o)[HIN]) {
    constexpr int NS1 = HIN / 2 + 1;
    int dep = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // (TAPWISE: the tap's addresses are made to depend on the previous tap's sums, which keeps its reads behind that arithmetic)
        if (TAPWISE && k > 0) {
#pragma unroll
            for (int r = k > 1 ? 0 : 1; r < HIN; ++r) asm volatile("" : "+v"(dep) : "v"(o[r].x), "v"(o[r].w));
        }
        const float* pk = p[k] + dep;
        float4 L[NS1];
#pragma unroll
        for (int s = 0; s < NS1; ++s)
            if (k > 0 || s < NS1 - 1) L[s] = *reinterpret_cast<const float4*>(pk + s * ss);
#pragma unroll
        for (int r = 0; r < HIN; ++r) {
            const int h = r + k - 1;
            if (h >= 0) {
                int s0, s1; float w0, w1;
                up_taps(h, HIN, s0, s1, w0, w1);
                const float4 A = L[s0], B = L[s1];
                const float4 t = make_float4(w0 * A.x + w1 * B.x, w0 * A.y + w1 * B.y, w0 * A.z + w1 * B.z, w0 * A.w + w1 * B.w);
                if (k == 0 || (k == 1 && r == 0)) o[r] = t;                  // (the first tap inside the axis)
                else { o[r].x += t.x; o[r].y += t.y; o[r].z += t.z; o[r].w += t.w; }
            }
        }
    }
}

template <int CT, int HIN, int NCHUNK, int FPU>
__global__ void __launch_bounds__(3 * CT * 64, 1) conv3x3_lowres_kernel(const gcpx_conv_args a, const int stat_rows) {
    using Cfg = LowresCfg<CT, HIN, NCHUNK, FPU>;
    constexpr int NT = Cfg::NT, NPIX = Cfg::NPIX, UPIX = Cfg::UPIX, NPG = Cfg::NPG, WOUT = Cfg::WOUT, HOUT = Cfg::HOUT, COUT = Cfg::COUT;
    constexpr int C4 = Cfg::C4, Q4 = Cfg::Q4, NS = Cfg::NS, NSLOT = Cfg::NSLOT, NV = Cfg::NV;
    constexpr int PLANE = Cfg::PLANE_BYTES, YS = Cfg::YS, FS = HOUT * WOUT * COUT;
    // 48 registers of resident weights leave room to hold a finished half-run and its addend in registers; 96 do not
    constexpr bool REG_RICH = CT * NCHUNK <= 4, AB_EARLY = REG_RICH;
    extern __shared__ float4 smem4[];
    char* planes = reinterpret_cast<char*>(smem4);                               // [chunk][piece][unit pixel][32] f16
    float* Z = reinterpret_cast<float*>(smem4);                                  // (the same bytes, one phase later)
    float* Y = reinterpret_cast<float*>(planes + Cfg::PZ_BYTES);
    unsigned* smax = reinterpret_cast<unsigned*>(planes + Cfg::PZ_BYTES + Cfg::Y_BYTES);
    // the per-channel constants and the running statistics live in LDS, not in registers: beside 96 registers of resident weights
    // (64 output channels, 3 wavefronts per SIMD) every lane constant carried through the unit loop is a spill
    float* bnS = reinterpret_cast<float*>(smax + 16);
    float* bnT = bnS + Cfg::CIN;
    float* biasT = bnT + Cfg::CIN;
    float4* stat = reinterpret_cast<float4*>(biasT + COUT);                      // [NT][2]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, q = lane >> 4;
    const int tx = wave % 3, ct = wave / 3;
    const int F = a.F;
    const int ew = a.w_split_log2_dev ? __builtin_amdgcn_readfirstlane(*a.w_split_log2_dev) : a.w_split_log2;

    // this wavefront's A fragments: taps (ty, tx) of channel tile ct, every chunk, both pieces — resident
    h8 wreg[3][NCHUNK][2];
    {
        const char* wbase = reinterpret_cast<const char*>(a.wpk_split) + lane * 16;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int ch = 0; ch < NCHUNK; ++ch) {
                const char* wp = wbase + (size_t)(((ch * 9 + ty * 3 + tx) * CT + ct) * 2048);
                wreg[ty][ch][0] = *reinterpret_cast<const h8*>(wp);
                wreg[ty][ch][1] = *reinterpret_cast<const h8*>(wp + 1024);
            }
    }
    if (tid < NCHUNK) smax[tid] = 0u;

    // a thread stages the same input channel quad in every slot (NT % Q4 == 0): its source, BatchNorm affine and activation are fixed,
    // and it keeps one output channel quad through both interpolation stages (NT % C4 == 0).  Like the stages' index algebra these are
    // derived again in every unit from an opaque copy of the thread index, not carried in registers beside the resident weights
    const int c0 = a.src[0].C;
    for (int c = tid; c < Cfg::CIN; c += NT) {
        const gcpx_conv_src& sr = c < c0 ? a.src[0] : a.src[1];
        const int cl = c < c0 ? c : c - c0;
        bnS[c] = sr.scale ? sr.scale[cl] : 1.f;
        bnT[c] = sr.scale ? sr.shift[cl] : 0.f;
    }
    if (tid < COUT) biasT[tid] = a.bias[tid];
    stat[tid * 2] = stat[tid * 2 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 pre[NS];
    auto issue_loads = [&](const int f0, const int t) {
        const int cgq = (t % Q4) * 4;
        const bool first = cgq < c0;
        const float* sptr = (first ? a.src[0].ptr : a.src[1].ptr) + (first ? cgq : cgq - c0);
        const int srcC = first ? a.src[0].C : a.src[1].C;
        // (frame -> source frame on the scalar unit: a unit has FPU frames and two sources, a thread picks)
        int sf[FPU];
#pragma unroll
        for (int fl = 0; fl < FPU; ++fl) {
            const int f = min(f0 + fl, F - 1);                            // (a unit's frames behind the last repeat it: computed, never stored)
            const int q0 = f / a.src[0].frame_div, q1 = a.nsrc > 1 ? f / a.src[1].frame_div : 0;
            sf[fl] = first ? q0 : q1;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int idx = t + NT * k;
            pre[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (NSLOT % NT == 0 || idx < NSLOT) {
                const int up = idx / Q4;
                int fs = sf[0];
#pragma unroll
                for (int fl = 1; fl < FPU; ++fl) fs = up / NPIX == fl ? sf[fl] : fs;
                pre[k] = *reinterpret_cast<const float4*>(sptr + ((size_t)fs * NPIX + up % NPIX) * srcC);
            }
        }
    };
    // A unit's output is stored one iteration late, behind the NEXT unit's staging: the memory counter is in order, so stores issued
    // right before the loop's back-edge would have to complete before the staging may touch the prefetched input; issued behind the
    // staging they are older than the next prefetch and long complete when it is waited for (conv3x3_up16_fold_kernel does the same)
    // Until then a half-run waits where the vertical stage left it, in its thread's registers, or (the instances with 96 registers
    // of resident weights) in LDS, in the Y buffer: dead behind the horizontal stage, and every thread reads back what it wrote itself.
    float4 keep[HIN];
    float4* O = reinterpret_cast<float4*>(Y);
    int pf0 = -1;
    auto store_out = [&](const int t) __attribute__((always_inline)) {
        if (t < NV) {
            const int px = (t / C4) % WOUT, fl = (t / (C4 * WOUT)) % FPU, hv = t / (C4 * WOUT * FPU);
            if (pf0 + fl < F) {
                float* op = a.out + (size_t)(pf0 + fl) * FS + ((hv ? HOUT - 1 : 0) * WOUT + px) * COUT + (t % C4) * 4;
                const int os = hv ? -WOUT * COUT : WOUT * COUT;
#pragma unroll
                for (int r = 0; r < HIN; ++r) *reinterpret_cast<float4*>(op + r * os) = REG_RICH ? keep[r] : O[r * NV + t];
            }
        }
    };

    const int nunits = (F + FPU - 1) / FPU;
    int u = blockIdx.x;
    if (u < nunits) issue_loads(u * FPU, tid);
    __syncthreads();

    for (; u < nunits; u += gridDim.x) {
        const int f0 = u * FPU;
        // (index algebra that is the same in every unit is recomputed from an opaque copy of the thread index: a few VALU instructions
        // per use; hoisted out of the unit loop it would pin ~100 registers beside the resident weights)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        // ---- registers -> BatchNorm affine + LeakyReLU of the producer; largest magnitude of every chunk over the unit ----
        const int cgq = (tl % Q4) * 4, chq = cgq >> 5;
        const float slope = (cgq < c0 ? a.src[0].act : a.src[1].act) == GCPX_ACT_LRELU ? 0.2f : 1.f;
        float4 v[NS];
        float m = 0.f;
        const float4 bn_s = *reinterpret_cast<const float4*>(bnS + cgq), bn_t = *reinterpret_cast<const float4*>(bnT + cgq);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            float4 t = pre[k];
            t.x = fmaf(t.x, bn_s.x, bn_t.x); t.y = fmaf(t.y, bn_s.y, bn_t.y); t.z = fmaf(t.z, bn_s.z, bn_t.z); t.w = fmaf(t.w, bn_s.w, bn_t.w);
            t.x = t.x > 0.f ? t.x : t.x * slope; t.y = t.y > 0.f ? t.y : t.y * slope;
            t.z = t.z > 0.f ? t.z : t.z * slope; t.w = t.w > 0.f ? t.w : t.w * slope;
            if (!(NSLOT % NT == 0 || tl + NT * k < NSLOT)) t = make_float4(0.f, 0.f, 0.f, 0.f);
            v[k] = t;
            m = fmaxf(m, fmaxf(fmaxf(fabsf(t.x), fabsf(t.y)), fmaxf(fabsf(t.z), fabsf(t.w))));
        }
        // (lanes l, l ^ 1, l ^ 2, l ^ 4 stage quads of the same 32-channel chunk: one LDS atomic per 8 lanes)
        // (ds_swizzle in bit mode, lane ^ 1, 2, 4: no lane-address registers to carry)
        m = fmaxf(m, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(m), 0x041f)));
        m = fmaxf(m, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(m), 0x081f)));
        m = fmaxf(m, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(m), 0x101f)));
        if ((lane & 7) == 0) atomicMax(&smax[chq], __float_as_uint(m));         // non-negative floats order like their bit patterns
        if (pf0 >= 0) store_out(tl);
        __syncthreads();                                                    // maxima complete; the previous unit's Z reads are done
        // the scale follows the chunks: a chunk with larger values than any before lowers it (the accumulators are rescaled, exact), a
        // chunk with smaller values keeps it.  amax 2^ec in [2^14, 2^15)
        int exr[NCHUNK];
#pragma unroll
        for (int ch = 0; ch < NCHUNK; ++ch) {
            const float amax = __uint_as_float(smax[ch]);
            int ec = 14 + 127 - (int)((__float_as_uint(amax) >> 23) & 0xff);
            ec = __builtin_amdgcn_readfirstlane(amax > 0.f ? max(-100, min(min(100, 126 - ew), ec)) : min(100, 126 - ew));
            exr[ch] = ch == 0 ? ec : min(ec, exr[ch - 1]);
        }
        // ---- two f16 planes per chunk in B-fragment order ----
        {
            int ex = exr[0];
#pragma unroll
            for (int c = 1; c < NCHUNK; ++c) ex = chq == c ? exr[c] : ex;
            const float sc = __uint_as_float((unsigned)(127 + ex) << 23);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int idx = tl + NT * k;
                if (NSLOT % NT == 0 || idx < NSLOT) {
                    float4 s = v[k];
                    s.x *= sc; s.y *= sc; s.z *= sc; s.w *= sc;
                    h4 p1, p2;
                    p1[0] = (_Float16)s.x; p1[1] = (_Float16)s.y; p1[2] = (_Float16)s.z; p1[3] = (_Float16)s.w;
                    p2[0] = (_Float16)(s.x - (float)p1[0]); p2[1] = (_Float16)(s.y - (float)p1[1]);
                    p2[2] = (_Float16)(s.z - (float)p1[2]); p2[3] = (_Float16)(s.w - (float)p1[3]);
                    char* dst = planes + chq * 2 * PLANE + (idx / Q4) * 64 + (cgq & 31) * 2;
                    *reinterpret_cast<h4*>(dst) = p1;
                    *reinterpret_cast<h4*>(dst + PLANE) = p2;
                }
            }
        }
        __syncthreads();                                                    // planes complete, every thread has read the maxima
        if (tl < NCHUNK) smax[tl] = 0u;
        // bias + the sequence's share of the conv (its skip channels, convolved once per sequence: gcpx_conv_args.addend) for this
        // thread's vertical half-run.  Where the registers allow it (AB_EARLY: 48 registers of resident weights) it is requested here,
        // BEFORE the next unit's input, so that the in-order memory counter lets the vertical stage wait for the addend alone; for the
        // same reason the prefetch below is issued on every path (a workgroup's last unit fetches itself again, from L2: never used).
        // The other instances fetch it in the vertical stage's epilogue, one output row at a time
        // (frame -> addend frame on the scalar unit, as in issue_loads)
        auto addend_frame = [&](const int fl) __attribute__((always_inline)) {
            int q = 0;
            if (a.addend) {
#pragma unroll
                for (int g = 0; g < FPU; ++g) {
                    const int qg = min(f0 + g, F - 1) / a.addend_frame_div;
                    q = fl == g ? qg : q;
                }
            }
            return q;
        };
        float4 ab[HIN];
        auto issue_addend = [&](const int t) __attribute__((always_inline)) {
            if (t < NV) {
                const float4 bq = *reinterpret_cast<const float4*>(biasT + (t % C4) * 4);
#pragma unroll
                for (int r = 0; r < HIN; ++r) ab[r] = bq;
                if (a.addend) {
                    const int px = (t / C4) % WOUT, fl = (t / (C4 * WOUT)) % FPU, hv = t / (C4 * WOUT * FPU);
                    const float* ap = a.addend + (size_t)addend_frame(fl) * FS + ((hv ? HOUT - 1 : 0) * WOUT + px) * COUT + (t % C4) * 4;
                    const int os = hv ? -WOUT * COUT : WOUT * COUT;
#pragma unroll
                    for (int r = 0; r < HIN; ++r) {
                        const float4 ad = *reinterpret_cast<const float4*>(ap + r * os);
                        ab[r].x += ad.x; ab[r].y += ad.y; ab[r].z += ad.z; ab[r].w += ad.w;
                    }
                }
            }
        };
        if (AB_EARLY) issue_addend(tl);
        // the next unit arrives behind this one's arithmetic
        issue_loads((u + (int)gridDim.x < nunits ? u + (int)gridDim.x : u) * FPU, tl);

        // ---- Y_(ty,tx) = W_(ty,tx) x on the source grid: NCHUNK x NPG x 3 taps x 3 MFMAs, small terms first ----
        f32x4 acc[3][NPG];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int pg = 0; pg < NPG; ++pg) acc[ty][pg] = f32x4{0, 0, 0, 0};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ch = 0; ch < NCHUNK; ++ch) {
            if (ch > 0 && exr[ch] != exr[ch - 1]) {
                const float r = __uint_as_float((unsigned)(127 + exr[ch] - exr[ch - 1]) << 23);
#pragma unroll
                for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                    for (int pg = 0; pg < NPG; ++pg) acc[ty][pg] *= r;
            }
#pragma unroll
            for (int pg = 0; pg < NPG; ++pg) {
                const char* bp = planes + ch * 2 * PLANE + (pg * 16 + (tl & 15)) * 64 + ((tl >> 4) & 3) * 16;
                const h8 b1 = *reinterpret_cast<const h8*>(bp);
                const h8 b2 = *reinterpret_cast<const h8*>(bp + PLANE);
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][pg] = mfma32h(wreg[ty][ch][1], b1, acc[ty][pg]);
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][pg] = mfma32h(wreg[ty][ch][0], b2, acc[ty][pg]);
#pragma unroll
                for (int ty = 0; ty < 3; ++ty) acc[ty][pg] = mfma32h(wreg[ty][ch][0], b1, acc[ty][pg]);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        {
            const float inv = __uint_as_float((unsigned)(127 - exr[NCHUNK - 1] - ew) << 23);          // scale back: exact
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int pg = 0; pg < NPG; ++pg) {
                    const f32x4 y = acc[ty][pg] * inv;
                    *reinterpret_cast<float4*>(Y + ((ty * 3 + tx) * UPIX + pg * 16 + (tl & 15)) * YS + ct * 16 + ((tl >> 4) & 3) * 4) = make_float4(y[0], y[1], y[2], y[3]);
                }
        }
        __syncthreads();                                                    // Y complete, the planes are free
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const int c4o = (tv % C4) * 4;

        // ---- horizontal: interpolate + shift-sum over tx.  A column outside the image is the conv's zero padding ----
        // thread = (half, frame, ty, source row, channel quad): HIN output columns of Z_ty[sy, .] from the half's border inwards
        {
            int t = tv / C4;
            const int sy = t % HIN; t /= HIN;
            const int ty = t % 3; t /= 3;
            const int fl = t % FPU, h = t / FPU;
            const float* yb = Y + ((ty * 3 + (h ? 2 : 0)) * UPIX + fl * NPIX + sy * HIN + (h ? HIN - 1 : 0)) * YS + c4o;
            const int ts = h ? -UPIX * YS : UPIX * YS;
            const float* const yp[3] = {yb, yb + ts, yb + 2 * ts};
            float4 z[HIN];
            half_run<HIN, !REG_RICH>(yp, h ? -YS : YS, z);
            float* zp = Z + (((fl * 3 + ty) * HIN + sy) * WOUT + (h ? WOUT - 1 : 0)) * COUT + c4o;
            const int zs = h ? -COUT : COUT;
#pragma unroll
            for (int r = 0; r < HIN; ++r) *reinterpret_cast<float4*>(zp + r * zs) = z[r];
        }
        __syncthreads();                                                    // Z complete

        // ---- vertical: interpolate + shift-sum over ty, bias + addend, BatchNorm partial sums; the result waits in registers for the next staging ----
        // thread = (half, frame, output column, channel quad): HIN output rows of that column from the half's border inwards
        if (tv < NV) {
            int t = tv / C4;
            const int px = t % WOUT; t /= WOUT;
            const int fl = t % FPU, hv = t / FPU;
            const float* zb = Z + (((fl * 3 + (hv ? 2 : 0)) * HIN + (hv ? HIN - 1 : 0)) * WOUT + px) * COUT + c4o;
            const int ts = hv ? -HIN * WOUT * COUT : HIN * WOUT * COUT;
            const float* const zq[3] = {zb, zb + ts, zb + 2 * ts};
            float4 o[HIN];
            half_run<HIN, !REG_RICH>(zq, hv ? -WOUT * COUT : WOUT * COUT, o);
            const float4 bq = *reinterpret_cast<const float4*>(biasT + c4o);
            const float* ap = a.addend + (size_t)addend_frame(fl) * FS + ((hv ? HOUT - 1 : 0) * WOUT + px) * COUT + c4o;
            const int os = hv ? -WOUT * COUT : WOUT * COUT;
            f32x4 st1, st2;
#pragma unroll
            for (int r = 0; r < HIN; ++r) {
                float4 b = AB_EARLY ? ab[r] : bq;
                if (!AB_EARLY && a.addend) {
                    __builtin_amdgcn_sched_barrier(0);                      // (one row's addend in registers, not all HIN)
                    const float4 ad = *reinterpret_cast<const float4*>(ap + r * os);
                    b.x += ad.x; b.y += ad.y; b.z += ad.z; b.w += ad.w;
                }
                const f32x4 v4 = f32x4{o[r].x + b.x, o[r].y + b.y, o[r].z + b.z, o[r].w + b.w};
                if (REG_RICH) keep[r] = make_float4(v4[0], v4[1], v4[2], v4[3]);
                else O[r * NV + tv] = make_float4(v4[0], v4[1], v4[2], v4[3]);
                st1 = r == 0 ? v4 : st1 + v4;
                st2 = r == 0 ? v4 * v4 : st2 + v4 * v4;
            }
            if (f0 + fl < F) {                                              // (a frame behind the last repeats it: computed, never counted or stored)
                const float4 s1 = stat[tv * 2], s2 = stat[tv * 2 + 1];
                stat[tv * 2] = make_float4(s1.x + st1[0], s1.y + st1[1], s1.z + st1[2], s1.w + st1[3]);
                stat[tv * 2 + 1] = make_float4(s2.x + st2[0], s2.y + st2[1], s2.z + st2[2], s2.w + st2[3]);
            }
        }
        pf0 = f0;
    }
    if (pf0 >= 0) store_out(tid);

    if (a.stats_partial) {
        __syncthreads();
        const float* red = reinterpret_cast<const float*>(stat);            // [NT][2][4]
        if (tid < 2 * COUT) {
            const int which = tid / COUT, c = tid % COUT;
            float sum = 0.f;
#pragma unroll 4
            for (int m = 0; m < NT / C4; ++m) sum += red[((c >> 2) + C4 * m) * 8 + which * 4 + (c & 3)];
            a.stats_partial[((size_t)blockIdx.x * 2 + which) * COUT + c] = sum;
            // rows of the workgroups the exact kernel's grid has and this launch does not: no work, zero sums
            for (int r = blockIdx.x + gridDim.x; r < stat_rows; r += gridDim.x) a.stats_partial[((size_t)r * 2 + which) * COUT + c] = 0.f;
        }
    }
}

template <int CT, int HIN, int NCHUNK, int FPU>
int launch_lowres(const gcpx_conv_args* a, hipStream_t stream, int rows) {
    using Cfg = LowresCfg<CT, HIN, NCHUNK, FPU>;
    auto kern = conv3x3_lowres_kernel<CT, HIN, NCHUNK, FPU>;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
        if (e != hipSuccess) {
            gcpx_set_error("conv3x3 lowres: hipFuncSetAttribute(%d B LDS): %s", Cfg::LDS_BYTES, hipGetErrorString(e));
            return GCPX_ERR_HIP;
        }
        attr_set = true;
    }
    // one workgroup per CU (registers and LDS allow no more): every workgroup pays the weight prologue once
    // (rows = the exact kernel's grid = rows of stats_partial: with statistics no workgroup may lie behind them)
    const int nunits = (a->F + FPU - 1) / FPU;
    int grid = gcpx_conv_grid() / 2;
    if (a->stats_partial && grid > rows) grid = rows;
    if (grid > nunits) grid = nunits;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::NT), Cfg::LDS_BYTES, stream, *a, rows);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}

// the kernel instance that takes the problem, or -1
int lowres_variant(const gcpx_conv_args* a) {
    if (!a || !a->upsample || !a->wpk_split || !a->out || !a->bias) return -1;
    if (a->split_layout != GCPX_SPLIT_PLAIN && a->split_layout != GCPX_SPLIT_LOWRES) return -1;
    if (a->head_mode != GCPX_HEAD_RAW || a->out_act != GCPX_ACT_NONE || a->out_pitch != a->Cout) return -1;
    if (a->src_row_map || a->raw_row_map || a->bwd_r) return -1;
    if (a->Hin != a->Win || a->Hout != 2 * a->Hin || a->Wout != 2 * a->Win || a->F <= 0) return -1;
    if (a->nsrc != 1 && a->nsrc != 2) return -1;
    int cin = 0;
    for (int s = 0; s < a->nsrc; ++s) {
        if (!a->src[s].ptr || a->src[s].C <= 0 || a->src[s].C % 16 || a->src[s].frame_div <= 0) return -1;
        cin += a->src[s].C;
    }
    if (cin != a->Cin) return -1;
    if (a->addend && a->addend_frame_div <= 0) return -1;
    if (a->Cout == 64 && a->Hin == 4 && a->Cin == 128) return 0;
    if (a->Cout == 32 && a->Hin == 8 && a->Cin == 64) return 1;
    if (a->Cout == 32 && a->Hin == 8 && a->Cin == 128) return 2;
    if (a->Cout == 32 && a->Hin == 4 && a->Cin == 128) return 3;
    return -1;
}

}  // namespace

extern "C" int gcpx_conv3x3_lowres_supported(const gcpx_conv_args* a) { return lowres_variant(a) >= 0 ? 1 : 0; }

// called by gcpx_launch_up32_split for GCPX_SPLIT_LOWRES; rows = gcpx_conv3x3_grid(a), the rows of stats_partial
int gcpx_launch_lowres(const gcpx_conv_args* a, hipStream_t stream, int rows) {
    switch (lowres_variant(a)) {
        case 0: return launch_lowres<4, 4, 4, 2>(a, stream, rows);
        case 1: return launch_lowres<2, 8, 2, 1>(a, stream, rows);
        case 2: return launch_lowres<2, 8, 4, 1>(a, stream, rows);
        case 3: return launch_lowres<2, 4, 4, 2>(a, stream, rows);
    }
    gcpx_set_error("conv3x3 lowres: GCPX_SPLIT_LOWRES on a problem gcpx_conv3x3_lowres_supported refuses (up=%d Cin=%d Cout=%d Hin=%d)",
                   a->upsample, a->Cin, a->Cout, a->Hin);
    return GCPX_ERR_UNSUPPORTED;
}
