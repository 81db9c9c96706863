// Picture logs (video-gcp_amd/image_log.py): one launch composes a whole panel -- a [n][H_c][W_c][3] canvas, channel-last as PNG rows
// want it -- out of f32 tensors that already live on the device, from a device table of tile descriptors (gcpx_panel_tile).
//
// It replaces the reference's host loops over nodes and samples (logger.py:114-182 "TODO vectorize", visualization.py:232-262,327-400,
// 485-497): where a node's tile goes is a device integer (node_t), so the host never has to read it.
//
// One workgroup = kSeg pixels of one canvas row.  The row segment lives in LDS; element e (pixel e / 3, channel e % 3) is owned by
// thread e % kThreads for the whole kernel: the background fill, every descriptor in table order and the write-out of the f32 canvas.
// So when two tiles land on the same pixels the later descriptor wins, and the gamma strips add in table order, whatever the hardware
// does: there is no atomic and no race to lose.  The descriptor loops are uniform over the workgroup (scalar tests); only the copy of a
// tile that crosses this row diverges.  Reads are three runs of consecutive floats per wave (one per channel plane); writes are
// consecutive dwords (f32) or dwords of four packed bytes (uint8).
// Every source read is checked against the element count the caller gave for its slot, every index against its count, and every write
// is clipped to the canvas: a wrong table gives a wrong picture, never a wild access.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSeg = 1024;                    // canvas pixels per workgroup: 12 KB of LDS

struct PanelSrcs {
    const void* p[GCPX_PANEL_MAX_SRCS];
    long long n[GCPX_PANEL_MAX_SRCS];
};

__device__ __forceinline__ long long load_int(const void* p, const long long i, const bool is64) {
    return is64 ? (long long)reinterpret_cast<const int64_t*>(p)[i] : (long long)reinterpret_cast<const int32_t*>(p)[i];
}

__global__ void __launch_bounds__(kThreads) panel_compose_kernel(const gcpx_panel_tile* __restrict__ tab, const int n_tiles,
                                                                 const PanelSrcs S, const int Hc, const int Wc, const float background,
                                                                 const int post_rescale, float* __restrict__ out_f32,
                                                                 uint8_t* __restrict__ out_u8) {
    __shared__ float row[kSeg * 3];
    const int tid = threadIdx.x;
    const int seg0 = blockIdx.x * kSeg, segw = min(kSeg, Wc - seg0);
    const int y = blockIdx.y, n = blockIdx.z;
    const int ne = segw * 3;
    for (int e = tid; e < ne; e += kThreads) row[e] = background;
    for (int d = 0; d < n_tiles; ++d) {
        const gcpx_panel_tile t = tab[d];
        if (t.kind < GCPX_PANEL_IMAGE || t.kind > GCPX_PANEL_FILL || t.h <= 0 || t.w <= 0) continue;
        const bool needs_src = t.kind != GCPX_PANEL_FILL;
        if (needs_src && (t.src < 0 || t.src >= GCPX_PANEL_MAX_SRCS || !S.p[t.src])) continue;
        const float* src = needs_src ? reinterpret_cast<const float*>(S.p[t.src]) : nullptr;
        const long long src_n = needs_src ? S.n[t.src] : 0;
        const bool has_idx = t.index >= 0 && t.index < GCPX_PANEL_MAX_SRCS && S.p[t.index];
        const bool has_len = t.length >= 0 && t.length < GCPX_PANEL_MAX_SRCS && S.p[t.length];
        if ((t.index >= 0 && !has_idx) || (t.length >= 0 && !has_len)) continue;
        const int tile_w = max(t.tile_w, 1);
        {   // the rows and canvases the whole descriptor can reach: most descriptors are left here
            const int rb = (t.nb - 1) * t.r_b, rf = (t.nf - 1) * t.r_f, qb = (t.nb - 1) * t.n_b, qf = (t.nf - 1) * t.n_f;
            if (t.nb <= 0 || t.nf <= 0) continue;
            if (y < t.r0 + min(rb, 0) + min(rf, 0) || y >= t.r0 + max(rb, 0) + max(rf, 0) + t.h) continue;
            if (n < t.n0 + min(qb, 0) + min(qf, 0) || n > t.n0 + max(qb, 0) + max(qf, 0)) continue;
        }
        for (int b = 0; b < t.nb; ++b) {
            long long iv = 0;
            if (has_idx) {
                const long long ii = (long long)t.index_off + (long long)b * t.index_stride;
                if (ii < 0 || ii >= S.n[t.index]) continue;
                iv = load_int(S.p[t.index], ii, (t.flags & GCPX_PANEL_INDEX_I64) != 0);
                if (iv < 0 || iv >= t.index_count) continue;
            }
            long long len = LLONG_MAX;
            if (has_len) {
                if (b >= S.n[t.length]) continue;
                len = load_int(S.p[t.length], b, (t.flags & GCPX_PANEL_LENGTH_I64) != 0);
                if (t.flags & GCPX_PANEL_LENGTH_STRICT) len -= 1;
            }
            const bool idx_is_frame = has_idx && (t.flags & GCPX_PANEL_INDEX_FRAME);
            const int col_add = (has_idx && !idx_is_frame) ? (int)iv * t.w : 0;
            // the frames of sample b that can touch (n, y): one candidate when frames step through canvases, the few whose rows hold
            // y when they step down the canvas, every frame otherwise (frames side by side in one row)
            int f_lo = 0, f_hi = t.nf - 1;
            if (t.n_f > 0) {
                const int q = n - t.n0 - b * t.n_b;
                if (q < 0 || q % t.n_f != 0) continue;
                f_lo = f_hi = q / t.n_f;
            } else if (t.r_f > 0) {
                const int q = y - t.r0 - b * t.r_b;                  // rows [f r_f, f r_f + h) hold q
                f_lo = q - t.h + 1 <= 0 ? 0 : (q - t.h + t.r_f) / t.r_f;
                f_hi = q < 0 ? -1 : q / t.r_f;
            }
            f_lo = max(f_lo, 0);
            f_hi = min(f_hi, t.nf - 1);
            for (int f = f_lo; f <= f_hi; ++f) {
                if (t.n0 + b * t.n_b + f * t.n_f != n) continue;
                const int r = t.r0 + b * t.r_b + f * t.r_f;
                if (y < r || y >= r + t.h) continue;
                const int c = t.c0 + b * t.c_b + f * t.c_f + col_add;
                const int x_lo = max(c, seg0), x_hi = min(c + t.w, seg0 + segw);
                if (x_lo >= x_hi) continue;
                const int e_lo = (x_lo - seg0) * 3, e_hi = (x_hi - seg0) * 3;
                const long long fs = idx_is_frame ? iv : (long long)f;
                const float keep = (long long)f <= len ? 1.f : 0.f;
                const long long base = t.off + (long long)b * t.s_b + fs * t.s_f;
                // the elements of [e_lo, e_hi) this thread owns: e = tid (mod kThreads)
                for (int e = e_lo + ((tid - e_lo) & (kThreads - 1)); e < e_hi; e += kThreads) {
                    const int px = e / 3, ch = e - 3 * px;
                    const int dx = seg0 + px - c;
                    if (t.kind == GCPX_PANEL_FILL) {
                        row[e] = t.fill;
                        continue;
                    }
                    const long long si = t.kind == GCPX_PANEL_IMAGE ? base + (long long)ch * t.s_c + (long long)(y - r) * t.s_y + dx
                                                                    : base + (long long)(dx / tile_w) * t.s_c;
                    if (si < 0 || si >= src_n) continue;
                    float v = src[si];
                    if (t.kind == GCPX_PANEL_GREY_ADD) {
                        row[e] = __fadd_rn(row[e], v);
                    } else {
                        if (has_len) v = __fmul_rn(v, keep);                                          // mask_extra: x * 0 past the end
                        if (t.flags & GCPX_PANEL_RESCALE) v = __fmul_rn(__fadd_rn(v, 1.f), 0.5f);     // (x + 1) / 2
                        row[e] = v;
                    }
                }
            }
        }
    }
    if (post_rescale)
        for (int e = tid; e < ne; e += kThreads) row[e] = __fmul_rn(__fadd_rn(row[e], 1.f), 0.5f);
    const size_t o = (((size_t)n * Hc + y) * Wc + seg0) * 3;
    if (out_f32)
        for (int e = tid; e < ne; e += kThreads) out_f32[o + e] = row[e];
    if (out_u8) {
        __syncthreads();                           // a packed dword holds elements of four owners
        // uint8 = trunc(clip(x, 0, 1) * 255)
        if ((Wc & 3) == 0) {                       // rows and segments start on dwords (kSeg * 3 is a multiple of 4)
            uint32_t* q = reinterpret_cast<uint32_t*>(out_u8 + o);
            for (int i = tid; i < ne / 4; i += kThreads) {
                uint32_t w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w |= (uint32_t)(int)__fmul_rn(fminf(fmaxf(row[4 * i + j], 0.f), 1.f), 255.f) << (8 * j);
                q[i] = w;
            }
        } else {
            for (int e = tid; e < ne; e += kThreads)
                out_u8[o + e] = (uint8_t)(int)__fmul_rn(fminf(fmaxf(row[e], 0.f), 1.f), 255.f);
        }
    }
}

}  // namespace

extern "C" int gcpx_panel_compose(const gcpx_panel_tile* tiles, int32_t n_tiles, const void* const* srcs, const int64_t* src_elems,
                                  int32_t n_srcs, int32_t n, int32_t H_c, int32_t W_c, float background, int32_t post_rescale,
                                  float* canvas_f32, uint8_t* canvas_u8, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    GCPX_CHECK_ARG(n_tiles >= 0 && (tiles || n_tiles == 0), "null tile table");
    GCPX_CHECK_ARG(n_srcs >= 0 && n_srcs <= GCPX_PANEL_MAX_SRCS && (n_srcs == 0 || (srcs && src_elems)),
                   "n_srcs must be in [0, GCPX_PANEL_MAX_SRCS] with srcs and src_elems given");
    GCPX_CHECK_ARG(n > 0 && H_c > 0 && W_c > 0 && n <= 65535 && H_c <= 65535, "canvas sizes must be in [1, 65535]");
    GCPX_CHECK_ARG((long long)n * H_c * W_c * 3 < (1ll << 31), "canvas too large");
    GCPX_CHECK_ARG(canvas_f32 || canvas_u8, "no output canvas");
    GCPX_CHECK_ARG((reinterpret_cast<uintptr_t>(canvas_u8) & 3) == 0 && (reinterpret_cast<uintptr_t>(canvas_f32) & 3) == 0,
                   "canvas not 4-byte aligned");
    PanelSrcs S{};
    for (int i = 0; i < n_srcs; ++i) {
        GCPX_CHECK_ARG(src_elems[i] >= 0 && (srcs[i] || src_elems[i] == 0), "null source with a non-zero element count");
        S.p[i] = srcs[i];
        S.n[i] = src_elems[i];
    }
    const dim3 grid((unsigned)((W_c + kSeg - 1) / kSeg), (unsigned)H_c, (unsigned)n);
    hipLaunchKernelGGL(panel_compose_kernel, grid, dim3(kThreads), 0, stream, tiles, n_tiles, S, H_c, W_c, background, post_rescale,
                       canvas_f32, canvas_u8);
    GCPX_CHECK_LAUNCH();
    return GCPX_OK;
}
