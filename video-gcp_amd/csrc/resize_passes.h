// The two integer passes of the 8-bit bilinear resampler (Pillow's Image.resize, see video-gcp_amd/dataset.py) as device functions over a
// band of source rows staged in LDS, the band itself (ResizeBand: LDS carve-up, tables, where the rows go), the host-side choice of the
// band, and the staging loads and the conversion of frames that need no resize.  Shared by the kernels of csrc/batch_assemble.hip
// (recorded frames from an uploaded slot or from a resident store; frames rendered top-down from states), so that all do one arithmetic.
#pragma once
#include <algorithm>

#include "common.h"

namespace gcpx_resize {

constexpr int kThreads = 256;
constexpr int kInfo = 8;     // int32 per sequence: n_frames, n_states, n_actions, chop, zero_from, end_ind, -, -
constexpr int kInfoResident = 8;   // int64 per sequence of the resident forms (include/gcpx.h fixes the layout)
constexpr int kPrecisionBits = 22;            // Pillow's PRECISION_BITS for 8-bit channels
constexpr int kResizeMaxSide = 512;
constexpr int kResizeMaxScale = 8;
constexpr int kResizeLdsTarget = 24 * 1024;   // per workgroup when a band can be made that small: six workgroups to a CU
constexpr int kResizeLdsMax = 64 * 1024;

// taps per output sample of one axis: Pillow's (int)ceil(support) * 2 + 1, support = max(n_in / n_out, 1)
inline int resize_ksize(const int n_in, const int n_out) {
    return (n_in <= n_out ? 1 : (n_in + n_out - 1) / n_out) * 2 + 1;
}

// source rows output rows [r0, r1) read, by the host table's own float64 arithmetic (dataset.resize_coeffs)
inline int resize_span(const int n_in, const int n_out, const int r0, const int r1) {
    const double scale = (double)n_in / n_out, support = scale < 1.0 ? 1.0 : scale;
    int lo = (int)((r0 + 0.5) * scale - support + 0.5), hi = (int)((r1 - 1 + 0.5) * scale + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
    return hi - lo;
}

// LDS of one workgroup: lut f32[256] | kx i32[W * ksx] | bx i32[2 W] | ky i32[R * ksy] | by i32[2 R] | raw u8 | hres u8
struct ResizeLds {
    int raw_off, raw_cap, hres_off, total;
};
__host__ __device__ inline ResizeLds resize_lds(const int Ws, const int W, const int ksx, const int ksy, const int R, const int cap) {
    ResizeLds l;
    l.raw_off = ((256 + W * ksx + 2 * W + R * ksy + 2 * R) * 4 + 15) & ~15;
    l.raw_cap = (cap * Ws * 3 + 32) & ~15;    // the band's source rows from the 16-byte boundary below their first byte
    l.hres_off = l.raw_off + l.raw_cap;
    l.total = l.hres_off + ((cap * W * 3 + 15) & ~15) + 64;    // + what zero-weight taps of the last row may read (resize_rows)
    return l;
}

__device__ __forceinline__ int clip8(const int acc) { return min(max(acc >> kPrecisionBits, 0), 255); }

// The horizontal pass of one band.  A thread keeps one output column xx (kThreads / W rows are in flight; all columns in turn when
// W >= kThreads): first source column, tap count and the KS coefficients stay in registers while it walks down the staged rows.  The
// 3 KS bytes a row contributes are read as the ND aligned dwords around them and shifted down to the first byte (v_alignbyte), a third
// of the LDS reads that byte loads take.  Taps past the count have coefficient 0; what they read lies inside the workgroup's LDS (at
// most 4 ND <= 56 bytes past the staged rows: hres and the slack behind it) and is multiplied by it.
template <int KS>
__device__ __forceinline__ void resize_rows(const uint8_t* __restrict__ raw, const int shift, uint8_t* __restrict__ hres,
                                            const int32_t* __restrict__ skx, const int32_t* __restrict__ sbx, const int nrows,
                                            const int Ws, const int W, const int tid) {
    constexpr int ND = (3 * KS + 3) / 4 + 1;
    const bool wide = W >= kThreads;
    const int rp = wide ? 1 : kThreads / W, rr = wide ? 0 : tid / W;
    if (rr >= rp) return;
    const int row_bytes = Ws * 3, hrow = W * 3;
    const uint32_t* raw32 = reinterpret_cast<const uint32_t*>(raw);
    for (int xx = wide ? tid : tid - rr * W; xx < W; xx += kThreads) {
        const int xmin = min(max(sbx[2 * xx], 0), Ws - 1);
        const int cnt = min(max(sbx[2 * xx + 1], 0), min(KS, Ws - xmin));
        int k[KS];
#pragma unroll
        for (int x = 0; x < KS; ++x) k[x] = x < cnt ? skx[xx * KS + x] : 0;
        int o = shift + rr * row_bytes + xmin * 3;
        uint8_t* q = hres + rr * hrow + xx * 3;
        for (int r = rr; r < nrows; r += rp, o += rp * row_bytes, q += rp * hrow) {
            const uint32_t* d = raw32 + (o >> 2);
            uint32_t w[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) w[i] = d[i];
#pragma unroll
            for (int i = 0; i + 1 < ND; ++i) w[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], (uint32_t)(o & 3));
            int a[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
#pragma unroll
            for (int j = 0; j < 3 * KS; ++j) a[j % 3] += __mul24((int)((w[j >> 2] >> (8 * (j & 3))) & 255), k[j / 3]);
            q[0] = (uint8_t)clip8(a[0]);
            q[1] = (uint8_t)clip8(a[1]);
            q[2] = (uint8_t)clip8(a[2]);
        }
    }
}

// the horizontal pass for a run-time tap count (2 * kResizeMaxScale + 1 at the most)
__device__ __forceinline__ void resize_rows_any(const int ksx, const uint8_t* __restrict__ raw, const int shift, uint8_t* __restrict__ hres,
                                                const int32_t* __restrict__ skx, const int32_t* __restrict__ sbx, const int nrows,
                                                const int Ws, const int W, const int tid) {
    switch (ksx) {
        case 3: resize_rows<3>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 5: resize_rows<5>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 7: resize_rows<7>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 9: resize_rows<9>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 11: resize_rows<11>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 13: resize_rows<13>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        case 15: resize_rows<15>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;
        default: resize_rows<17>(raw, shift, hres, skx, sbx, nrows, Ws, W, tid); break;   // 2 * kResizeMaxScale + 1
    }
}

// Bytes [a0, a0 + nbytes) of `src` into LDS by 16-byte loads from the 16-byte boundary below a0 (src itself is 16-byte aligned); returns
// a0 & 15, the offset of byte a0 in `raw`.  `total_bytes` is the size of what src points to: its last bytes are read one by one, nothing
// at or past its end.
__device__ __forceinline__ int stage_bytes(const uint8_t* __restrict__ src, const long long a0, const int nbytes,
                                           const long long total_bytes, uint8_t* __restrict__ raw, const int tid) {
    const int shift = (int)(a0 & 15);
    const long long abase = a0 - shift;
    const int nvec = (shift + nbytes + 15) >> 4;
    for (int v = tid; v < nvec; v += kThreads) {
        const long long g = abase + 16ll * v;
        uint4 x;
        if (g + 16 <= total_bytes) {
            x = *reinterpret_cast<const uint4*>(src + g);
        } else {                              // the last bytes of the whole slot: no read past its end
            uint32_t w[4] = {0, 0, 0, 0};
            for (int j = 0; j < 16; ++j)
                if (g + j < total_bytes) w[j >> 2] |= (uint32_t)src[g + j] << (8 * (j & 3));
            x = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(raw + 16 * v) = x;
    }
    return shift;
}

// Pixels [p0, p0 + 4) of one frame stored at the model's size: 12 bytes of `src` (read when `valid`, else the pixel is `pad`) through
// the table to one float4 of each of the three channel planes of dst (and of d0 / dg when the frame is also I_0 / I_g).  H * W % 4 == 0
// takes three dword loads (src is then 4-byte aligned), any other size single bytes.
__device__ __forceinline__ void lut_quad_store(const uint8_t* __restrict__ src, const bool valid, const float* __restrict__ tab,
                                               const float pad, const int HW, const int p0, float* __restrict__ dst,
                                               float* __restrict__ d0, float* __restrict__ dg) {
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

// a band of a frame that is not valid under the time map: lut[0] everywhere, nothing read
__device__ __forceinline__ void store_pad_band(const float pad, const int nr, const int W4, const int HW, float* __restrict__ dst,
                                               float* __restrict__ d0, float* __restrict__ dg, const int tid) {
    const float4 v = make_float4(pad, pad, pad, pad);
    for (int i = tid; i < nr * W4; i += kThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            *reinterpret_cast<float4*>(dst + (size_t)c * HW + 4 * i) = v;
            if (d0) *reinterpret_cast<float4*>(d0 + (size_t)c * HW + 4 * i) = v;
            if (dg) *reinterpret_cast<float4*>(dg + (size_t)c * HW + 4 * i) = v;
        }
    }
}

// The vertical pass of one band out of LDS (one thread: four output columns of one row = 12 bytes per tap), table lookup, float4 stores
// to the three channel planes of dst (and of d0 / dg when the frame is also I_0 / I_g).  hres holds the horizontal result of source rows
// [y_lo, y_lo + nrows); every table entry is clamped to them.
__device__ __forceinline__ void resize_cols_store(const uint8_t* __restrict__ hres, const int32_t* __restrict__ sky,
                                                  const int32_t* __restrict__ sby, const float* __restrict__ tab, const int y_lo,
                                                  const int nrows, const int nr, const int W, const int ksy, const int HW,
                                                  float* __restrict__ dst, float* __restrict__ d0, float* __restrict__ dg, const int tid) {
    const int W4 = W >> 2;
    const int dy = kThreads / W4, dgp = kThreads - dy * W4;
    int yy = tid / W4, g = tid - yy * W4;
    const int hrow4 = (W * 3) >> 2;
    while (yy < nr) {
        const int ymin = min(max(sby[2 * yy], y_lo), y_lo + nrows - 1);
        const int cnt = min(max(sby[2 * yy + 1], 0), min(ksy, y_lo + nrows - ymin));
        const uint32_t* q = reinterpret_cast<const uint32_t*>(hres) + (ymin - y_lo) * hrow4 + g * 3;
        const int32_t* k = sky + yy * ksy;
        int a[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) a[j] = 1 << (kPrecisionBits - 1);
        for (int y = 0; y < cnt; ++y) {
            const int kk = k[y];
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
            q += hrow4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] += __mul24((int)((w0 >> (8 * j)) & 255), kk);
                a[4 + j] += __mul24((int)((w1 >> (8 * j)) & 255), kk);
                a[8 + j] += __mul24((int)((w2 >> (8 * j)) & 255), kk);
            }
        }
        const size_t o = (size_t)yy * W + 4 * g;
#pragma unroll
        for (int c = 0; c < 3; ++c) {         // bytes RGBR GBRG BRGB: channel c of pixel j is byte 3 j + c
            const float4 v = make_float4(tab[clip8(a[c])], tab[clip8(a[3 + c])], tab[clip8(a[6 + c])], tab[clip8(a[9 + c])]);
            *reinterpret_cast<float4*>(dst + (size_t)c * HW + o) = v;
            if (d0) *reinterpret_cast<float4*>(d0 + (size_t)c * HW + o) = v;
            if (dg) *reinterpret_cast<float4*>(dg + (size_t)c * HW + o) = v;
        }
        g += dgp;
        yy += dy;
        if (g >= W4) {
            g -= W4;
            ++yy;
        }
    }
}

// the bands: the fewest equal bands of output rows whose source rows and horizontal result fit the LDS target, else single rows inside
// the LDS limit.  Returns R (0: one output row's source rows do not fit), with the most source rows of a band in *cap.
inline int resize_choose_band(const int Hs, const int Ws, const int H, const int W, const int ksx, const int ksy, int* cap, ResizeLds* L) {
    for (int nb = 1; nb <= H; ++nb) {
        const int r = (H + nb - 1) / nb;
        int c = 0;
        for (int r0 = 0; r0 < H; r0 += r) c = std::max(c, resize_span(Hs, H, r0, std::min(r0 + r, H)));
        *L = resize_lds(Ws, W, ksx, ksy, r, c);
        if (L->total <= (r > 1 ? kResizeLdsTarget : kResizeLdsMax)) {
            *cap = c;
            return r;
        }
    }
    return 0;
}

// One workgroup of a resizing kernel: the band of output rows [r0, r0 + nr) of one output frame.  Its parts of the LDS (ResizeLds), the
// source rows [y_lo, y_lo + nrows) the band reads and where its rows go: dst in traj_seq, d0 / dg in I_0 / I_g when the frame is also
// that (else null).  A kernel makes it (resize_band), loads lut and tables (resize_band_tables), stages the source rows into `raw` its own
// way and ends with resize_band_store.
struct ResizeBand {
    float* tab;
    int32_t *skx, *sbx, *sky, *sby;
    uint8_t *raw, *hres;
    int Hs, Ws, W, ksx, ksy, cap, HW, r0, nr, y_lo, nrows;
    float *dst, *d0, *dg;
};

// the band blockIdx.y of output frame t of sequence b (source Hs x Ws, output H x W, R rows to a band, at most cap source rows)
__device__ __forceinline__ ResizeBand resize_band(uint8_t* smem, const int Hs, const int Ws, const int H, const int W, const int ksx,
                                                  const int ksy, const int R, const int cap, const int b, const int t, const int T,
                                                  const int end_ind, float* traj, float* I0, float* Ig) {
    const ResizeLds L = resize_lds(Ws, W, ksx, ksy, R, cap);
    ResizeBand d;
    d.tab = reinterpret_cast<float*>(smem);
    d.skx = reinterpret_cast<int32_t*>(smem) + 256;
    d.sbx = d.skx + W * ksx;
    d.sky = d.sbx + 2 * W;
    d.sby = d.sky + R * ksy;
    d.raw = smem + L.raw_off;
    d.hres = smem + L.hres_off;
    d.Hs = Hs, d.Ws = Ws, d.W = W, d.ksx = ksx, d.ksy = ksy, d.cap = cap, d.HW = H * W;
    d.r0 = blockIdx.y * R;
    d.nr = min(R, H - d.r0);
    d.dst = traj + ((size_t)b * T + t) * 3 * d.HW + (size_t)d.r0 * W;
    d.d0 = t == 0 ? I0 + (size_t)b * 3 * d.HW + (size_t)d.r0 * W : nullptr;
    d.dg = t == end_ind ? Ig + (size_t)b * 3 * d.HW + (size_t)d.r0 * W : nullptr;
    return d;
}

// lut and the band's tables into LDS, y_lo / nrows from the bounds table; no barrier: the caller's staged bytes go under the same one.
// A frame that is not valid resizes to zeros: the band is lut[0], no table or frame is read, and the result is false (nothing left to do).
__device__ __forceinline__ bool resize_band_tables(ResizeBand& d, const bool valid, const float* lut, const int32_t* kx, const int32_t* bx,
                                                   const int32_t* ky, const int32_t* by, const int tid) {
    d.tab[tid] = lut[tid];
    if (!valid) {
        store_pad_band(lut[0], d.nr, d.W >> 2, d.HW, d.dst, d.d0, d.dg, tid);
        return false;
    }
    for (int i = tid; i < d.W * d.ksx; i += kThreads) d.skx[i] = kx[i];
    for (int i = tid; i < 2 * d.W; i += kThreads) d.sbx[i] = bx[i];
    for (int i = tid; i < d.nr * d.ksy; i += kThreads) d.sky[i] = ky[d.r0 * d.ksy + i];
    for (int i = tid; i < 2 * d.nr; i += kThreads) d.sby[i] = by[2 * d.r0 + i];
    const int last = d.r0 + d.nr - 1;
    d.y_lo = min(max(by[2 * d.r0], 0), d.Hs - 1);
    d.nrows = min(min(max(by[2 * last] + by[2 * last + 1], d.y_lo + 1), d.Hs) - d.y_lo, d.cap);
    return true;
}

// tables and source rows (byte `shift` of raw is the first) are written: horizontal pass LDS -> LDS, vertical pass, conversion, stores
__device__ __forceinline__ void resize_band_store(const ResizeBand& d, const int shift, const int tid) {
    __syncthreads();
    resize_rows_any(d.ksx, d.raw, shift, d.hres, d.skx, d.sbx, d.nrows, d.Ws, d.W, tid);
    __syncthreads();
    resize_cols_store(d.hres, d.sky, d.sby, d.tab, d.y_lo, d.nrows, d.nr, d.W, d.ksy, d.HW, d.dst, d.d0, d.dg, tid);
}

}  // namespace gcpx_resize
