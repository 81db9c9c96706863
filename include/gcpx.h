/*
 * gcpx.h — C-ABI of libgcpx.so: the MI355X (gfx950) hot path of the goal-conditioned hierarchical video
 * predictor (gcp_tree).  Plain pointers and sizes only; every pointer marked "dev" is a device (HBM) pointer
 * owned by the caller.  The library allocates nothing on the hot path and never synchronises; every launch
 * is enqueued on the caller's stream.  Every function returns 0 on success, a negative gcpx_status otherwise;
 * gcpx_last_error() gives the text.
 *
 * The reference (orybkin/video-gcp, mounted at /root/reference) has no FFI/plugin layer — its boundary is
 * Python duck typing.  Each entry point therefore cites the reference call site whose device
 * work it replaces.
 */
#ifndef GCPX_H
#define GCPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCPX_VERSION 1

typedef enum gcpx_status {
    GCPX_OK = 0,
    GCPX_ERR_INVALID_ARG = -1,
    GCPX_ERR_UNSUPPORTED = -2,
    GCPX_ERR_HIP = -3,
    GCPX_ERR_COMM = -4
} gcpx_status;

typedef enum gcpx_act { GCPX_ACT_NONE = 0, GCPX_ACT_LRELU = 1, GCPX_ACT_TANH = 2 } gcpx_act;

int gcpx_version(void);
const char* gcpx_last_error(void);
/* number of workgroups a persistent conv launch will use (size of the stats_partial first dim) */
int gcpx_conv_grid(void);

/* ---------------------------------------------------------------------------------------------------
 * Convolution stacks.
 *   replaces blox.torch.encoder_decoder.Encoder / DecoderModule as called at
 *   gcp/prediction/models/base_gcp.py:188,208-209 (encoder) and
 *   gcp/prediction/models/tree/tree_dense_rec.py:42 (decoder.decode_seq over all tree nodes).
 * Activations are fp32 NHWC [F][H][W][C].  A conv's input is the channel concatenation of up to two sources
 * (decoder features ++ skip activations of I_0, broadcast over the node axis with frame_div); each source is
 * passed RAW (pre-normalisation) with the per-channel affine (BatchNorm folded to scale/shift) and
 * LeakyReLU applied while the tile is staged ("normalise on load").
 * ------------------------------------------------------------------------------------------------- */
typedef struct gcpx_conv_src {
    const float* ptr;    /* dev: NHWC [F / frame_div][Hin][Win][C] */
    const float* scale;  /* dev: [C] or NULL (identity) */
    const float* shift;  /* dev: [C] or NULL */
    int32_t C;           /* channels of this source (multiple of 16) */
    int32_t frame_div;   /* source frame = f / frame_div (1 = per-frame; N = broadcast over N nodes) */
    int32_t act;         /* gcpx_act applied after the affine */
    int32_t _pad;
} gcpx_conv_src;

typedef enum gcpx_head_mode {
    GCPX_HEAD_RAW = 0,      /* store conv output NHWC [F][H][W][CT*16] (kernel channel order), + bias, + out_act */
    GCPX_HEAD_DLM_MEAN = 1, /* discrete-logistic-mixture mean -> images NCHW [F][3][H][W]; nothing else written */
    GCPX_HEAD_DLM_BOTH = 2, /* both of the above */
    GCPX_HEAD_TANH_NCHW = 3, /* gaussian head: tanh(first 3 channels) -> images NCHW */
    GCPX_HEAD_DLM_NLL = 4,  /* mixture mean -> images, and for every frame f with raw_row_map[f] >= 0 the discretised-logistic-mixture
                               negative log-likelihood of target row raw_row_map[f] (decoder.nll on the matched frames,
                               frame_binding.py:88-99), evaluated in the epilogue: nll_partial[i][row] = sum over the pixels of item i
                               (4 rows x 16 columns; (H / 4) * (W / 16) items per frame) — reduce over i with gcpx_reduce_partials.
                               No raw parameters are stored.  Split-f16 head only (wpk_split set) */
    GCPX_HEAD_DLM_NLL_GRAD = 5 /* training forward: as GCPX_HEAD_DLM_NLL, and row raw_row_map[f] of `out` ([rows][H][W][112]) receives
                               d (nll_scale * nll_row_weight[row] * NLL) / d parameters — what gcpx_dlm_nll_bwd computes from stored
                               parameters.  Rows no frame maps to are not written (zero them: gcpx_zero_unmapped_rows) */
} gcpx_head_mode;

typedef struct gcpx_conv_args {
    gcpx_conv_src src[2];
    int32_t nsrc;
    int32_t F;              /* output frames */
    int32_t Hin, Win;       /* source spatial size */
    int32_t Hout, Wout;     /* output spatial size (2x source when upsample, 1/2 for the stride-2 encoder conv) */
    int32_t Cin;            /* sum of source channels */
    int32_t Cout;           /* real output channels; stored channel pitch is out_pitch */
    int32_t out_pitch;      /* floats between consecutive pixels of `out` */
    int32_t upsample;       /* 1: bilinear x2 (align_corners=False) before the 3x3 conv */
    int32_t out_act;        /* gcpx_act in the epilogue (layers without a norm) */
    int32_t head_mode;      /* gcpx_head_mode (conv3x3 only) */
    const float* wpk;       /* dev: weights in MFMA fragment order (see video-gcp_amd/packing.py) */
    const float* bias;      /* dev: [CT*16], zero padded */
    float* out;             /* dev: NHWC raw output (may be NULL for GCPX_HEAD_DLM_MEAN) */
    float* images;          /* dev: NCHW [F][3][H][W] for the head modes that produce images */
    float* stats_partial;   /* dev: [gcpx_conv3x3_grid(a) or gcpx_conv4x4s2_grid()][2][CT*16] per-workgroup sum / sum-of-squares of the
                               raw output for training-mode BatchNorm, or NULL */
    const int32_t* raw_row_map; /* dev: [F] or NULL (output head only): frame f stores its raw parameters at row
                               raw_row_map[f] of `out`, or not at all when the entry is negative — only the nodes matched
                               to a ground-truth frame need their distribution parameters (frame_binding.py:91-92) */
    const int32_t* src_row_map; /* dev: [F] or NULL (non-upsampling convs and gcpx_conv_stage): frame f reads source frame
                               src_row_map[f]; a negative entry reads zeros (backward of the matched-frame gather) */
    const int32_t* src_row_frames; /* dev: [n_src_rows] or NULL: the inverse of src_row_map (row r is read by frame src_row_frames[r]).
                               Optional accelerator for the plain 3x3 conv: the kernel then walks the rows that exist instead of
                               testing every frame, and zero-fills the frames whose src_row_map entry is negative up front */
    int32_t n_src_rows;
    int32_t w_split_log2;   /* with wpk_split: the power of two the packed weights were scaled by (the kernel undoes it) */
    const void* wpk_split;  /* dev or NULL: the same weights as two f16 pieces in 16x16x32 fragment order
                               (packing.pack_dlm_head_split / pack_conv3x3_split).  When set, kernels that have a split-f16 form run
                               it: f32-equivalent results (error of the order of one f32 rounding per product) on the f16 matrix
                               pipes, see csrc/split_mfma.h.  NULL selects the exact f32 MFMA kernels */
    const int32_t* w_split_log2_dev; /* dev or NULL: when set, the scale exponent is read from here instead of w_split_log2
                               (weights re-split on the device after every optimizer step, gcpx_split_pack) */
    int32_t split_layout;   /* layout of wpk_split: GCPX_SPLIT_PLAIN (the conv's own 3x3 taps) or GCPX_SPLIT_ROWFOLD (upsampling blocks
                               with 32 -> 16 channels: the vertical half of the bilinear x2 folded into the weights, see
                               gcpx_fold_upsample_weights) */
    int32_t nll_rows;       /* GCPX_HEAD_DLM_NLL: rows of nll_target / row pitch of nll_partial */
    const float* nll_target; /* dev: NCHW [nll_rows][3][H][W] ground-truth frames in [-1, 1] (traj_seq) */
    float* nll_partial;     /* dev: [(H / 4) * (W / 16)][nll_rows]; rows no frame maps to are not written */
    const float* nll_row_weight; /* dev: [nll_rows] or NULL (GCPX_HEAD_DLM_NLL_GRAD): per-row factor of the gradient (pad_mask) */
    float nll_scale;        /* GCPX_HEAD_DLM_NLL_GRAD: d total / d nll_bt = w_rec / (B * prod(traj_seq.shape[1:])) (base_gcp.py:299-301) */
    int32_t _pad3;
    float* images_rows;     /* dev or NULL (split-f16 mixture heads): NCHW [rows][3][H][W]; every frame f with raw_row_map[f] >= 0 stores its
                               image at that row as well — the matched / kept frames in sequence order (tree_dense_rec.py:56-60,
                               tree.py:62-65) without a gather pass behind the head.  Rows no frame maps to are not written */
    int64_t images_rows_dup; /* != 0: a second copy of those rows at images_rows + images_rows_dup (floats) */
    /* Data gradient of a 16-channel layer with the NEXT step of the backward pass in its epilogue (split-f16 plain 3x3 conv with 16
       output channels, out_pitch 16): the layer whose output gradient this conv produces is BatchNorm + LeakyReLU(0.2) of the raw
       tensor bwd_r [F][H][W][16], so the kernel stores  g = conv * (bwd_scale * r + bwd_shift > 0 ? 1 : 0.2)  and leaves the
       per-workgroup sums of g and of g * (r - bwd_mean) * bwd_rstd in stats_partial [gcpx_conv3x3_grid(a)][2][16] — what gcpx_act_bwd
       (up = 0, no add) computes in a pass of its own over the same tensors.  NULL: plain data gradient */
    const float* bwd_r;
    const float *bwd_scale, *bwd_shift, *bwd_mean, *bwd_rstd;
    /* Upsampling blocks with 32 / 64 output channels in split-f16 (conv3x3_up32_split_kernel), and with Cout == 16 the 16-channel
       row-folded block only (GCPX_SPLIT_ROWFOLD16, conv3x3_up16_fold16_kernel: F must be a multiple of addend_frame_div): a raw NHWC tensor
       [F / addend_frame_div][Hout][Wout][out_pitch] added to the conv's result (before the BatchNorm partial sums and the store), frame f
       reading frame f / addend_frame_div.  The decoder concatenates the skip activations of I_0 — the same for the N nodes of a sequence
       — to every node's features (tree_dense_rec.py:42 -> blox ConvDecoder with skips); a conv is linear in its input channels, so the
       skip half is convolved ONCE per sequence and arrives here, and the per-node launch walks the node's own channels only.  NULL: none */
    const float* addend;
    int32_t addend_frame_div;
    int32_t _pad4;
} gcpx_conv_args;

/* GCPX_SPLIT_HEAD32: the 100-channel mixture head's weights in 32x32x16 A-fragment order [9 taps][4 tiles][2 pieces][64][8]
   (packing.pack_head32_split / head32_index) for csrc/conv3x3_head32.hip — modes GCPX_HEAD_DLM_MEAN / _NLL / _NLL_GRAD only */
/* GCPX_SPLIT_ROWFOLD16: the row-folded weights of a 16 -> 16 channel upsampling block, two horizontal taps per k-step
   (packing.pack_conv3x3_fold16 / conv3x3_fold16_index over the [24][16][Cin] scratch of gcpx_fold_upsample_weights): the node half / the
   skip half of additional_conv_layer once the skip half is hoisted (gcpx_conv_args.addend) */
/* GCPX_SPLIT_LOWRES: the PLAIN pack of a 32 / 64-output-channel upsampling block (byte-identical: packing.pack_conv3x3_split32), run by
   csrc/conv3x3_lowres.hip — the nine tap products on the SOURCE grid, bilinear x2 and 3x3 shift-sum behind them in f32.  Same contract
   as the PLAIN launch (sources, bias, addend, raw store, stats_partial rows); only for problems gcpx_conv3x3_lowres_supported accepts */
typedef enum gcpx_split_layout { GCPX_SPLIT_PLAIN = 0, GCPX_SPLIT_ROWFOLD = 1, GCPX_SPLIT_HEAD32 = 2, GCPX_SPLIT_ROWFOLD16 = 3,
                                 GCPX_SPLIT_LOWRES = 4 } gcpx_split_layout;

/* decoder block: (bilinear x2 upsample +) 3x3 conv, pad 1.  gcpx_conv3x3_grid(a) = number of workgroups that launch
   will use = rows of a->stats_partial (a->stats_partial must already be non-NULL in the query if it will be). */
int gcpx_conv3x3(const gcpx_conv_args* a, void* stream);
int gcpx_conv3x3_grid(const gcpx_conv_args* a);
/* 1 when the block has a GCPX_SPLIT_LOWRES form (upsampling, split-f16 PLAIN-compatible pack, raw store at pitch Cout, and one of
   128 -> 64 @4x4, 64 -> 32 @8x8, 128 -> 32 @8x8, 128 -> 32 @4x4), else 0.  split_layout may be PLAIN or LOWRES in the query */
int gcpx_conv3x3_lowres_supported(const gcpx_conv_args* a);
/* encoder block: 4x4 conv, stride 2, pad 1 (NHWC sources); its stats_partial has gcpx_conv4x4s2_grid() rows */
int gcpx_conv4x4s2(const gcpx_conv_args* a, void* stream);
int gcpx_conv4x4s2_grid(void);
/* first encoder block: same conv on the NCHW 3-channel image tensor the model API receives.
   x: dev NCHW [F][3][Hin][Win]; out NHWC [F][Hin/2][Win/2][Cout] with bias + out_act applied. */
int gcpx_conv4x4s2_image(const float* x, const float* wpk, const float* bias, float* out,
                         int32_t F, int32_t Hin, int32_t Win, int32_t Cout, int32_t out_act, void* stream);
/* Dispatch queries: what gcpx_conv4x4s2 / gcpx_conv4x4s2_image would launch for these arguments, without launching anything (no HIP
   call besides the one-time read of the device's CU count; 256 CUs are assumed without a device).  Each entry point takes form,
   frames per workgroup and grid from the same host function as its query, under the same environment switches, read on every call:
   GCPX_ENC_NOSPLIT (ignore split weights), GCPX_ENC_DIRECT (no LDS form), GCPX_ENC_FPB (frames per workgroup of the LDS and split
   forms, when in 1 .. the shape's maximum), GCPX_ENC_IMAGE_DIRECT.  Both return the argument errors the launch would.
   out4 = {form, fpb, grid, nblk}: fpb = frames a workgroup of the LDS / split form stages (0 for the direct kernels); nblk = the blocks
   the grid's workgroups loop over: groups of fpb frames, or for the direct kernels groups of 16 (Cout 32) / 8 pixel groups of 16
   output pixels.  out2 = {form, grid}. */
typedef enum gcpx_enc_form_id {
    GCPX_ENC_FORM_DIRECT = 0,        /* conv4x4s2_kernel: operands straight from global memory, any frame shape */
    GCPX_ENC_FORM_LDS = 1,           /* conv4x4s2_lds_kernel: exact f32, fpb frames staged in LDS */
    GCPX_ENC_FORM_SPLIT = 2,         /* conv4x4s2_split_kernel (csrc/conv_enc_split.hip): split-f16, fpb frames staged in LDS */
    GCPX_ENC_FORM_IMAGE_DIRECT = 3,  /* conv4x4s2_image_kernel */
    GCPX_ENC_FORM_IMAGE_LDS = 4      /* conv4x4s2_image_lds_kernel: 32 x 32 and 64 x 64 images, one frame per workgroup and trip */
} gcpx_enc_form_id;
int gcpx_conv4x4s2_form(const gcpx_conv_args* a, int32_t* out4);
int gcpx_conv4x4s2_image_form(int32_t F, int32_t Hin, int32_t Win, int32_t* out2);
/* the first TWO encoder blocks of 64 x 64 frames in one launch (csrc/conv_enc_fused.hip): gcpx_conv4x4s2_image(x, w0pk, bias0, ., a->F,
   64, 64, 16, act0) followed by gcpx_conv4x4s2(a) on its result, the 32 x 32 x 16 map between them kept in LDS.  `a` describes the
   second block as for gcpx_conv4x4s2 (16 -> 32 channels, 32 x 32 -> 16 x 16, split-f16 weights in the PLAIN layout, one source without
   affine or activation); a->src[0].ptr is not read.  a0_out: dev [F][32][32][16] or NULL — the map is stored there as well, for the
   callers that have another reader of it.  a->out, a0_out and rows 0 .. F - 1 of a->stats_partial (row f = frame f; may be NULL) hold the
   bits the two launches leave; rows F .. gcpx_conv4x4s2_grid() - 1 are zeroed.  Nothing at or beyond frame F is read or written.
   _supported: 1 when (a, image size) is such a problem (and F <= gcpx_conv4x4s2_grid()), else 0 — the caller then makes the two
   launches; _grid: workgroups of a launch with at least that many frames (a workgroup loops over frames blockIdx, blockIdx + grid, ...) */
int gcpx_conv4x4s2_image_fused(const float* x, const float* w0pk, const float* bias0, int32_t act0, float* a0_out,
                               const gcpx_conv_args* a, void* stream);
int gcpx_conv4x4s2_image_fused_supported(const gcpx_conv_args* a, int32_t Himg, int32_t Wimg);
int gcpx_conv4x4s2_image_fused_grid(void);

/* BatchNorm statistics -> (scale, shift):  scale = gamma * rsqrt(var + eps), shift = beta - mean * scale.
   partial: dev [n_partial][2][pitch] (fp32 partial sums written by the conv / gemm epilogues); column n
   < (pitch / C) * C belongs to channel n % C, the columns behind those whole replicas are padding and are not read (pitch >= C);
   count = elements per channel.  If running_mean/var are non-NULL they are updated with `momentum` (training). */
int gcpx_bn_finalize(const float* partial, int32_t n_partial, int32_t pitch, int32_t C, double count,
                     const float* gamma, const float* beta, float eps, float* scale, float* shift,
                     float* running_mean, float* running_var, float momentum, float* mean_out, float* rstd_out,
                     void* stream);   /* mean_out / rstd_out: [C] batch statistics kept for the backward pass, or NULL */
/* n standard-normal numbers (Philox4x32-10 + Box-Muller) into out (16-byte aligned); state: dev uint64 [2] = {seed, offset}, the offset
   advanced by a second launch behind the draw, so a replayed graph draws fresh numbers.  Replaces the torch.randn behind
   Gaussian.sample() (tree_module.py:79-94) for models that draw their latent noise themselves. */
int gcpx_randn(float* out, int64_t n, uint64_t* state, void* stream);
/* eval-mode fold: scale/shift from running statistics */
int gcpx_bn_fold(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                 float eps, int32_t C, float* scale, float* shift, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Row GEMM with gathered, concatenated inputs:  out[r, :] = epi( concat_s X_s[map_s(r), :] @ W^T + bias ).
 *   replaces the Linear/LSTMCell/Conv1d/ConvTranspose(1x1->4x4)/Conv(4x4 valid) launches issued from
 *   gcp/prediction/models/tree/tree_lstm.py:43-49 (split_linear merge + HiddenStatePredictorModel),
 *   gcp/prediction/models/base_gcp.py:199 (ConvSeqEncodingModule) and the encoder head / decoder input.
 * Row r = (b, j), b = r / rpb, j = r % rpb.  A source row is ptr + b*sb + (j+shift)*sr  (zeros when j+shift is
 * outside [0, rpb)), or ptr + rowidx[r]*sr when rowidx is given (batchwise_index gather, inference.py:27-33).
 * ------------------------------------------------------------------------------------------------- */
typedef struct gcpx_row_src {
    const float* ptr;
    const int32_t* rowidx;  /* dev: [M] absolute row indices, or NULL */
    const float* scale;     /* dev: per-channel affine on load, channel = k % cmod; NULL = identity */
    const float* shiftv;
    int64_t sb, sr;         /* strides in floats */
    int32_t width;          /* K extent of this source (multiple of 16) */
    int32_t shift;          /* row shift inside the batch (conv1d taps) */
    int32_t act;
    int32_t cmod;
} gcpx_row_src;

typedef enum gcpx_gemm_epi {
    GCPX_EPI_NONE = 0,
    GCPX_EPI_LRELU = 1,
    GCPX_EPI_LSTM = 2,   /* N = 4H gate-interleaved (n = 4u+g, g in i,f,g,o): writes h, c; see below */
    GCPX_EPI_GAUSS_SAMPLE = 3 /* gcpx_gemm_group only — not a GEMM: out[r, n] = mu + exp(log_sigma) * eps with [mu | log_sigma] = the 2N-wide
                            rows of src[0] and eps = the N-wide rows of src[1] (Gaussian.sample / reparametrize, sequential.py:52): lets
                            the draw of the next VRNN step ride in a launch of this step instead of being a launch of its own */
} gcpx_gemm_epi;

struct gcpx_lstm_bwd_args;
typedef struct gcpx_gemm_args {
    gcpx_row_src src[6];
    int32_t nsrc;
    int32_t M, N, K, rpb;
    const float* wpk;       /* dev: [K/16][N/16][64][4] fragment-packed W[N][K] */
    const float* bias;      /* dev: [N] or NULL */
    float* out;             /* dev: row r at out + b*ob + j*orow (NONE / LRELU) */
    int64_t ob, orow;
    int32_t epi;
    int32_t nbatch;         /* 0/1: single problem; >1: blockIdx.z = b runs the same M x N x K problem with every source
                               pointer advanced by b*z_src_off, weights by b*z_w_off, bias by b*z_bias_off and out by
                               b*z_out_off floats (the 2*n_lstm_layers split_linear projections in one launch) */
    float* stats_partial;   /* dev: [gcpx_gemm_row_blocks(M, N)][2][N] per-row-block sum / sum of squares
                               of the output columns (training-mode BatchNorm), or NULL */
    /* LSTM epilogue: c' = sig(f)*c + sig(i)*tanh(g); h' = sig(o)*tanh(c') */
    const float* c_prev;    /* row r at c_prev + r*c_prev_stride */
    int64_t c_prev_stride;
    float* h_out;           /* row r at h_out + b*hb + j*hrow ; c_out likewise */
    float* c_out;
    int64_t hb, hrow;
    float* h_copy;          /* optional dense copy of h: row r at h_copy + r*H (input of the next layer) */
    int64_t z_src_off, z_w_off, z_bias_off, z_out_off;
    float* gates_out;       /* LSTM epilogue, optional: activated gates [M][H][4] = (i, f, g, o) kept for the backward pass */
    const void* wpk_split;  /* dev or NULL: the same weights as two f16 pieces, [K/32][N/16][2][64][8] (packing.pack_gemm_split; batch b at
                               byte offset b * z_w_off * 4).  When set, problems with enough rows to be bound by the f32 MFMA rate run
                               the split-f16 kernel (csrc/gemm_split.hip): f32-equivalent results, see split_mfma.h */
    const int32_t* w_split_log2_dev; /* dev or NULL: [nbatch] powers of two the packed pieces were scaled by; NULL = w_split_log2 */
    int32_t w_split_log2;
    int32_t _pad_split;
    void* x_planes;         /* dev or NULL: workspace for the activations as two f16 pieces in fragment order + x_exp [padded rows] row
                               exponents (sizes: gcpx_gemm_planes_workspace).  When set (with wpk_split) problems with many rows run as a
                               conversion pass + an LDS-DMA fed GEMM (csrc/gemm_planes.hip); same results class as the split kernel */
    int32_t* x_exp;
    int64_t x_planes_bytes; /* size of the x_planes allocation (checked against the problem) */
    const struct gcpx_lstm_bwd_args* lstm_bwd;
                            /* DEVICE copy of a gcpx_lstm_bwd_args, or NULL (GCPX_EPI_NONE, single problem, dense rows r = b*rpb + j of the
                               M rows the cell backward has too): the epilogue runs the LSTM cell backward of the layer this GEMM feeds —
                               output column u < H of row r IS that cell's d h from above, so dgates / dc_prev of (r, u) are written next
                               to out[r, u] and the separate gcpx_lstm_bwd launch (one of two per layer on a latency-bound chain)
                               disappears.  dh_dense of the struct is ignored; columns >= H (the d h_prev half of a [dx | dh] GEMM) are
                               plain outputs.  Same arithmetic as gcpx_lstm_bwd. */
} gcpx_gemm_args;

int gcpx_gemm(const gcpx_gemm_args* a, void* stream);
/* workspace of gcpx_gemm_args.x_planes / x_exp for an M x K activation matrix (x nbatch): bytes of the planes, number of int32 exponents */
int gcpx_gemm_planes_workspace(int32_t M, int32_t K, int32_t nbatch, int64_t* planes_bytes, int64_t* n_exp);
/* Several independent small-M problems (those gcpx_gemm runs as split-K 16 x 16 tiles) in ONE launch: the same layer of the
   prior / inference / generator nets of a VRNN step (sequential.py:49-54), or independent GEMMs of a tree level.
   gcpx_gemm_group_dims validates a HOST table of n (<= 16) problems (GCPX_ERR_UNSUPPORTED when one is not in that regime) and
   fills dims [n][4] + the grid size; the caller uploads table and dims once and replays gcpx_gemm_group. */
int gcpx_gemm_group_dims(const gcpx_gemm_args* host_table, int32_t n, int32_t* dims, int32_t* total_blocks);
int gcpx_gemm_group(const gcpx_gemm_args* dev_table, const int32_t* dev_dims, int32_t n, int32_t total_blocks, void* stream);
/* number of row blocks gcpx_gemm uses for an M x N problem (first dim of stats_partial) */
int gcpx_gemm_row_blocks(int32_t M, int32_t N);
/* Dispatch query: what gcpx_gemm would launch for these arguments, without launching anything (no HIP call besides the one-time
   read of the device's CU count; 256 CUs are assumed without a device).  out6 = {form, PR, CR, grid x, grid y, grid z}: PR x CR
   is the block of 16 x 16 tiles a wavefront (GCPX_GEMM_FORM_TILE) or a split-K workgroup (GCPX_GEMM_FORM_SPLIT_K) owns; PR, CR and
   the grid's x, y are 0 for the split-f16 and planes kernels, which tile on their own.  gcpx_gemm takes its launch from the same
   host function, under the same environment switches (GCPX_GEMM_TILE, GCPX_GEMM_NOKS, GCPX_GEMM_NO_KS_BLOCKS).  Returns the argument
   errors gcpx_gemm would. */
typedef enum gcpx_gemm_form_id {
    GCPX_GEMM_FORM_TILE = 0,      /* one-wavefront blocks: csrc/gemm_tile.h, KS = false */
    GCPX_GEMM_FORM_SPLIT_K = 1,   /* four wavefronts split K over one block: csrc/gemm_tile.h, KS = true */
    GCPX_GEMM_FORM_SPLIT_F16 = 2, /* csrc/gemm_split.hip */
    GCPX_GEMM_FORM_PLANES = 3     /* csrc/gemm_planes.hip */
} gcpx_gemm_form_id;
int gcpx_gemm_form(const gcpx_gemm_args* a, int32_t* out6);

/* ---------------------------------------------------------------------------------------------------
 * Fused Predictor MLP:  input(in->mid, LReLU), n_mid x (mid->mid, GroupNorm(8), LReLU), head(mid->out).
 *   replaces blox.torch.subnetworks.Predictor as called at tree_module.py:77 (prior), inference.py:35
 *   (posterior), tree_module.py:105 (MLP LSTM initialiser), misc.py:48 (length), frame_binding.py:71
 *   (existence), base_gcp.py:256 (state regressor), inverse_mdl.py:126 and cost_mdl.py:63.
 * One wavefront owns 16 rows end to end; hidden activations never leave LDS.
 * GCPX_MLP_GAUSS: out = 2*nz, mu = out[:nz], log_sigma = out[nz:]; additionally z = mu + exp(log_sigma) * eps
 * (Gaussian.sample / reparametrize, tree_module.py:79-94).
 * ------------------------------------------------------------------------------------------------- */
typedef enum gcpx_mlp_epi { GCPX_MLP_PLAIN = 0, GCPX_MLP_GAUSS = 1,
                             GCPX_MLP_TANH = 2 /* out = tanh(head): the non-LSTM subgoal predictor, tree_module.py:109-110 */ } gcpx_mlp_epi;

typedef struct gcpx_mlp_args {
    gcpx_row_src src[6];
    int32_t nsrc;
    int32_t M, rpb;
    int32_t in_dim, mid, n_mid, out_dim;
    const float* w_in;      /* dev: fragment-packed [in_dim/16][mid/16][64][4] */
    const float* b_in;      /* [mid] */
    const float* w_mid;     /* dev: n_mid x fragment-packed [mid/16][mid/16][64][4] */
    const float* b_mid;     /* [n_mid][mid] */
    const float* gn_gamma;  /* [n_mid][mid] */
    const float* gn_beta;   /* [n_mid][mid] */
    const float* w_out;     /* dev: fragment-packed [mid/16][out_pad/16][64][4] */
    const float* b_out;     /* [out_pad] */
    float gn_eps;
    float lrelu_slope;
    int32_t epi;
    int32_t out_split;      /* columns per output block (0 = out_dim): n -> block n / out_split */
    float* out;             /* row r, col n at out + (n/out_split)*oblk + b*ob + j*orow + n % out_split */
    int64_t ob, orow, oblk;
    /* GAUSS */
    const float* eps;       /* row r at eps + b*eb + j*erow, [nz] */
    int64_t eb, erow;
    float* z;               /* row r at z + b*zb + j*zrow, [nz] */
    int64_t zb, zrow;
    float* save;            /* optional, training: hidden activations kept for the backward pass, dense rows:
                               [0]: a_0 = LReLU(input layer) [M][mid]; then per hidden layer l: u_l (pre-GroupNorm) [M][mid]
                               and a_l (post GroupNorm + LReLU) [M][mid]  ->  (1 + 2*n_mid) * M * mid floats */
} gcpx_mlp_args;

int gcpx_mlp(const gcpx_mlp_args* a, void* stream);
/* Several independent Predictors of the same hidden width in ONE launch: the prior next to the posterior of a tree level
   (tree_module.py:77 + inference.py:27-35), the latent-space heads of run_auxilliary_models (base_gcp.py:234-262).
   gcpx_mlp_group_dims validates a HOST table of n (<= 16) problems and fills dims [n][4] = {first block, row blocks, head
   splits, 0} + the grid size; the caller uploads table and dims once (plan build) and replays gcpx_mlp_group. */
int gcpx_mlp_group_dims(const gcpx_mlp_args* host_table, int32_t n, int32_t* dims, int32_t* total_blocks);
int gcpx_mlp_group(const gcpx_mlp_args* dev_table, const int32_t* dev_dims, int32_t n, int32_t total_blocks, int32_t mid,
                   void* stream);
/* The same launch carrying one row GEMM (a HOST gcpx_gemm_args, plain epilogue) as additional workgroups: a level of the tree in front
   of its recurrent cell — prior + posterior Predictors (tree_module.py:77, inference.py:27-35) and the split_linear merge of the
   parents' hidden states (tree_lstm.py:43-48) depend on the previous level only, not on each other.  Results are those of
   gcpx_mlp_group + gcpx_gemm.  gcpx_mlp_group_gemm_supported: 1 when the GEMM's tiling and the group's size have a combined kernel
   (hidden width 128, at most one workgroup per CU, GEMM not on the split-f16 kernel); otherwise launch the two separately. */
int gcpx_mlp_group_gemm_supported(const gcpx_gemm_args* g, int32_t total_blocks, int32_t mid);
int gcpx_mlp_group_gemm(const gcpx_mlp_args* dev_table, const int32_t* dev_dims, int32_t n, int32_t total_blocks, int32_t mid,
                        const gcpx_gemm_args* g, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Balanced frame binding — integer bookkeeping, bit-exact with
 *   gcp/prediction/models/tree/frame_binding.py:42-65 (BalancedBinding, torch-1.3 Long/Long truncation),
 *   gcp/prediction/models/tree/frame_binding.py:28-34 (argmax gather) and
 *   gcp/evaluation/evaluation_matching.py:192-206 (BalancedEvalBinding.get_all_samples).
 * Tree nodes are addressed by depth-first position p in [0, N) (N = 2^L - 1).
 *   node_t      [B][N]  timestep of node p (int32)
 *   leave       [B][N]  1 if the node is kept (its c_n_prime row is non-zero)
 *   frame2node  [B][T]  depth-first position matched to frame t; for padded frames the ROOT (argmax of an
 *                       all-zero column = bf index 0)
 *   etilde_row  [L-level blocks, bf order: level l holds B*2^l entries, b-major]  b*T + node timestep:
 *               absolute row of inf_enc_seq[B*T] gathered for the posterior (inference.py:27-33)
 *   seq_len     [B]     end_ind + 1
 *   node2row    [B][N]  b*T + timestep for kept nodes, -1 otherwise (row of the matched-frame arrays; may be NULL)
 * ------------------------------------------------------------------------------------------------- */
int gcpx_balanced_binding(const int64_t* end_ind, int32_t B, int32_t L, int32_t T, int32_t* node_t,
                          int32_t* leave, int32_t* frame2node, int32_t* etilde_row, int32_t* seq_len,
                          int32_t* node2row, void* stream);

/* out[b][t] = src[b][idx[b][t] + idx_offset] for rows of `row_floats` floats (matched / pruned sequences);
   src has N rows per batch element; rows with idx < 0 are zero-filled (pad_sequence, base_gcp.py:242). */
int gcpx_gather_rows(const float* src, const int32_t* idx, float* out, int32_t B, int32_t T, int32_t N,
                     int32_t idx_offset, int64_t row_floats, void* stream);
/* gcpx_gather_rows for the rows its producer has NOT written: rows r with written[r] >= 0 are left untouched (the output head stores
   the frames matched to a row itself, gcpx_conv_args.images_rows; what remains are the padded rows: zeros, or the frame idx names) */
int gcpx_gather_rows_rest(const float* src, const int32_t* idx, float* out, int32_t B, int32_t T, int32_t N, int32_t idx_offset,
                          int64_t row_floats, const int32_t* written, void* stream);
/* Learned pairwise cost over a rollout (LearnedCostEstimate, gcp/planning/cem/cost_fcn.py:88-95):
   gcpx_seq_pairs builds the "next" operand nxt[i][t] = lat[i][t+1] (t+1 < len_i) else goal[i] (goal == NULL: the
   sequence's own last latent, row 0 when len_i <= 0); the cost MLP runs on (lat, nxt) rows; gcpx_masked_row_sum adds the first len_i
   per-step costs of every candidate.  Both clamp len_i to T (lat and vals have T rows per candidate); a non-positive length sums to 0. */
int gcpx_seq_pairs(const float* lat, const int32_t* lengths, const float* goal, float* nxt, int32_t n, int32_t T,
                   int32_t nz, void* stream);
int gcpx_masked_row_sum(const float* vals, const int32_t* lengths, float* out, int32_t n, int32_t T, void* stream);
/* Hand-written planner costs over padded device rollouts (CostFcn subclasses, gcp/planning/cem/cost_fcn.py:10-77): x [n][T][ld]
   (the first D columns of a row are used), lengths [n], goal row of candidate i at goal + i*goal_stride (0: one goal for all) -> out [n].
   kind 0 EuclideanDistance, 1 EuclideanPathLength (dense only), 2 StepPathLength, 3 L2ImageCost (D = the image columns);
   final_step_weight multiplies the last step, dense = sum over steps instead of the last step's value (cost_fcn.py:16-23). */
int gcpx_rollout_cost(const float* x, int64_t ld, const int32_t* lengths, const float* goal, int64_t goal_stride, float* out, int32_t n,
                      int32_t T, int32_t D, int32_t kind, int32_t dense, float final_step_weight, void* stream);
/* dst[b][r] = src[b][r] for r < rows, rows of row_floats floats, independent batch strides (in rows): assembling
   images = cat(I_0, decoded) of the sequential model (sequential.py:57) without a torch.cat */
int gcpx_copy_rows(const float* src, float* dst, int32_t B, int32_t rows, int64_t row_floats, int64_t src_batch_rows,
                   int64_t dst_batch_rows, void* stream);
/* Gaussian.sample() for a recurrent cell's [mu | log_sigma] rows: z = mu + exp(log_sigma) * eps, rows r = (b, j) at
   base + b*{m,e,z}b + j*{m,e,z}r  (VRNN step of sequential.py:51-54) */
int gcpx_gauss_sample(const float* muls, int64_t mb, int64_t mr, const float* eps, int64_t eb, int64_t er, float* z,
                      int64_t zb, int64_t zr, int32_t M, int32_t rpb, int32_t nz, void* stream);
/* idx[b][t] = t (t <= end_ind[b]) else -1; seq_len[b] = end_ind[b] + 1: prefix selection of the sequential model
   (sequential.py:88-93,130-131) in the same form as gcpx_compact_index */
int gcpx_seq_index(const int64_t* end_ind, int32_t B, int32_t T, int32_t* idx, int32_t* seq_len, void* stream);
/* graph-capturable memset(0) (recurrent state reset, lstm_init='zero') */
int gcpx_fill_zero(void* ptr, int64_t nbytes, void* stream);
/* compaction of kept nodes: dst_idx[b][k] = k-th depth-first position with leave==1 (k < seq_len[b]), else -1 */
int gcpx_compact_index(const int32_t* leave, int32_t B, int32_t N, int32_t T, int32_t* dst_idx, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Losses (deterministic reductions).
 *   gcpx_dlm_nll:  decoder.nll(matched distr, traj_seq) of frame_binding.py:88-99 for the discrete-logistic-mixture head:
 *                  params [rows][npix][pitch] in the head kernel's channel order, target NCHW [rows][3][npix];
 *                  nll_out[row] = sum over pixels of the negative log-likelihood; rows whose row_weight (pad_mask) is 0
 *                  are skipped and report 0.
 *   gcpx_gauss_nll: the same for the gaussian head (mu = images).
 *   gcpx_kl_gauss: KLDivLoss2(q_z, p_z) of inference.py:38-43: per batch element, sum over nodes and dims of
 *                  max(KL, free_nats); q/p rows are [mu | log_sigma] at base + b*batch_stride + n*node_stride.
 *   gcpx_loss_combine: length CE (misc.py:53-56), existence BCE (frame_binding.py:80-86), state L2
 *                  (base_gcp.py:281-286), the weighted total of get_total_loss (base_gcp.py:294-304).
 *                  out[0..8] = dense_img_rec, kl, len_pred, existence_predictor, state_regression, total, nll,
 *                  action_reconst (inverse_mdl.py:181-191), cost_estimation (cost_mdl.py:59-62).
 * ------------------------------------------------------------------------------------------------- */
typedef struct gcpx_loss_args {
    const float* nll_bt;          /* [B*T] */
    const float* pad_mask;        /* [B*T] */
    const float* kl_b;            /* [B] or NULL */
    const float* len_logits;      /* [B][T] or NULL */
    const int64_t* end_ind;       /* [B] */
    const float* existence;       /* [B][N] logits or NULL */
    const int32_t* leave;         /* [B][N] */
    const float* regressed_state; /* [B][T][state_dim] or NULL */
    const float* state_target;    /* [B][T][state_dim] or NULL */
    const int32_t* seq_len;       /* [B] */
    float* out;                   /* [16] */
    int32_t B, T, N, state_dim;
    float w_rec, w_kl, w_len, w_exist, w_state;
    float total_div;
    /* inverse model, sampled pair (inverse_mdl.py:136-191): action_pred [B][n_actions] against actions[b][inv_t0[b]] */
    const float* action_pred;     /* [B][n_actions] or NULL */
    const float* action_seq;      /* inputs.actions [B][T-1][n_actions] */
    const int64_t* inv_t0;        /* [B] */
    /* cost model (cost_mdl.py:42-62): cost_pred [B] against the ground-truth path cost [B] */
    const float* cost_pred;       /* [B] or NULL */
    const float* cost_target;     /* [B] */
    int32_t n_actions;
    float w_action, w_cost;
    /* weights of the state regression when they differ from pad_mask (gcp_sequential: pad_mask above is the reconstruction
       weight with frame 0 zeroed, sequential.py:63-66, while the regressor still sees frame 0, base_gcp.py:281-286); NULL = pad_mask */
    const float* state_mask;      /* [B*T] or NULL */
    /* KL weight under a schedule (kl_weight_burn_in, base_gcp.py:121-128: the weight ramps from 0 to its target over the first
       iterations): when set, the weight is read from this device scalar instead of w_kl, so a captured graph sees the current value */
    const float* w_kl_dev;
} gcpx_loss_args;

int gcpx_dlm_nll(const float* params, const float* target, const float* row_weight, float* nll_out, int32_t rows,
                 int32_t npix, int32_t pitch, int32_t n_mix, void* stream);
int gcpx_gauss_nll(const float* mu, const float* target, const float* log_sigma, float* nll_out, int32_t rows,
                   int32_t nelem, void* stream);
int gcpx_kl_gauss(const float* qz, const float* pz, int32_t B, int32_t N, int32_t nz, int64_t batch_stride,
                  int64_t node_stride, float free_nats, const float* node_weight /* b*weight_bstride + n, or NULL */,
                  int64_t weight_bstride, float* kl_out, void* stream);
int gcpx_loss_combine(const gcpx_loss_args* a, void* stream);
/* The same in two launches for a forward whose serial tail matters: gcpx_loss_pre = gcpx_kl_gauss (same arguments) + the five terms
   that need no decoded frame (length cross entropy, existence BCE, state / action / cost regression -> out[2], [3], [4], [7], [8]),
   one launch that can be issued before the decoder; gcpx_loss_final = reconstruction + KL sums and the weighted total
   (base_gcp.py:264-304) from nll_bt, kl_b and those five values. */
int gcpx_loss_pre(const gcpx_loss_args* a, const float* qz, const float* pz, int32_t N, int32_t nz, int64_t batch_stride,
                  int64_t node_stride, float free_nats, const float* node_weight, int64_t weight_bstride, float* kl_out, void* stream);
int gcpx_loss_final(const gcpx_loss_args* a, void* stream);


/* ---------------------------------------------------------------------------------------------------
 * Auxiliary models, training-time paths, and the sampled sequence length (csrc/aux.hip).
 * ------------------------------------------------------------------------------------------------- */
/* InverseModel.sample_offsets (inverse_mdl.py:84-104) + CostModel._general_cost's index draws (cost_mdl.py:105-107) from four
   uniform numbers per sequence, u [4][B] in [0,1):  inv_t0 in {0..end_ind-temp_dist}, inv_t1 = inv_t0 + {1..temp_dist},
   cost_start in {0..end_ind-1}, cost_end in {cost_start+1..end_ind}.  (The reference draws with np.random; callers that
   want its exact stream feed the indices instead.) */
int gcpx_aux_sample_indices(const int64_t* end_ind, const float* u, int32_t B, int32_t temp_dist, int64_t* inv_t0, int64_t* inv_t1,
                            int64_t* cost_start, int64_t* cost_end, void* stream);
/* the same from four STANDARD-NORMAL numbers per sequence, n [4][B] (u = Phi(n) is uniform on (0, 1)): the draws then come out of the
   one generator launch that also fills the latent noise of Gaussian.sample(), and this launch sits inside the forward's graph */
int gcpx_aux_sample_indices_gauss(const int64_t* end_ind, const float* n, int32_t B, int32_t temp_dist, int64_t* inv_t0, int64_t* inv_t1,
                                  int64_t* cost_start, int64_t* cost_end, void* stream);
/* rows [4][B] (int32): absolute rows b*T + inv_t0, b*Wd + inv_t1, b*Wd + cost_start, b*Wd + cost_end — the gather-on-load
   sources of `inv_mdl.action_pred(enc_traj_seq[b,t0], model_enc_seq[b,t1])` (inverse_mdl.py:149-169) and
   `cost_mdl.cost_pred(model_enc_seq[b,start], model_enc_seq[b,end])` (cost_mdl.py:108-109, :50) */
int gcpx_aux_index_rows(const int64_t* inv_t0, const int64_t* inv_t1, const int64_t* cost_start, const int64_t* cost_end, int32_t B,
                        int32_t T, int32_t Wd, int32_t* rows, void* stream);
/* ground-truth cost of CostModel._general_cost with EuclideanPathLength(dense_cost=True) (cost_mdl.py:110-111,
   cost_fcn.py:14-21,49-54): out[b] = sum_{t=start}^{end-1} sum_row || x[b,t+1,row,:] - x[b,t,row,:] ||_2 over x [B][T][rows][row_len]
   (images: rows = 3*H, row_len = W).  partial: scratch [B][rows]. */
int gcpx_path_cost(const float* x, const int64_t* start_idx, const int64_t* end_idx, int32_t B, int32_t T, int32_t rows,
                   int32_t row_len, float* partial, float* out, void* stream);
/* get_end_ind under val_mode(pred_length=True) (base_gcp.py:219-226): end_ind[b] = max(min_len, inverse CDF of
   softmax(logits[b]) at u[b]) — the OneHotCategorical draw (misc.py:49) with the uniform number fed in */
int gcpx_sample_length(const float* logits, const float* u, int32_t B, int32_t T, int32_t min_len, int64_t* end_ind, void* stream);


/* ---------------------------------------------------------------------------------------------------
 * Evaluation metrics (csrc/metrics.hip): mse / psnr / ssim of generated against ground-truth sequences —
 * Evaluator.compute_metrics (gcp/evaluation/compute_metrics.py:123-130; blox.torch.evaluation is absent, spec in
 * video-gcp_amd/evaluation.py).  tgt [B][T][C][H][W] in [-1,1]; est: a pool of frames [R][C][H][W]; frame_map [B*T] = pool
 * frame compared with target frame (b, t) (negative: skipped; NULL: identity); per sequence the frames t in [first[b], last[b])
 * are averaged (the harness crops the two conditioning frames).  Skipped means left out of the average: such a frame adds to no sum
 * and is not counted, so the three values are those of the remaining frames of the range; a sequence with no frame left (an empty
 * range, or every frame of it skipped) reports NaN three times.  scratch: 2*B*T*C doubles.  out [B][3] = mse, psnr, ssim.
 * ------------------------------------------------------------------------------------------------- */
int gcpx_image_metrics(const float* est, const float* tgt, const int32_t* frame_map, const int32_t* first, const int32_t* last,
                       int32_t B, int32_t T, int32_t C, int32_t H, int32_t W, double* scratch, float* out, void* stream);

/* Top-of-N accumulation (csrc/topn.hip), one launch pair per prior sample n of N: the per-sample buffer update and best-sample
 * bookkeeping of Evaluator.eval_single / _is_better / _get_best_idxs (gcp/evaluation/compute_metrics.py:89-120,236-250), called by
 * Evaluator.eval inside ModelTrainer.val (gcp/prediction/train.py:205-210).
 *   metrics [B][3] (gcpx_image_metrics' out) -> all[b][n][:]; best[b] = n when metrics[b][comp] is better than the best of samples 0..n-1
 *   (strictly lower if lower_is_better, else strictly higher; a NaN beats any number: np.argmin / np.argmax order), best[b] = 0 at n = 0.
 *   When sample n becomes best, its frames are copied: best_frames[b][t] = pool[frame_map[b*T + t]] for first[b] <= t < last[b]
 *   (first / last NULL: no bound), best_full[b][j] = full_pool[full_map[b*F + j]]; a negative or >= *_rows row gives a zero frame.
 *   Frames are rows of row_floats floats (a multiple of 4, 16-byte aligned).  T = 0 / F = 0: no such set (its pointers may be NULL). */
int gcpx_topn_accumulate(const float* metrics, int32_t B, int32_t n, int32_t N, int32_t comp, int32_t lower_is_better, float* all,
                         int32_t* best, const float* pool, int32_t pool_rows, const int32_t* frame_map, const int32_t* first,
                         const int32_t* last, int32_t T, float* best_frames, const float* full_pool, int32_t full_rows,
                         const int32_t* full_map, int32_t F, float* best_full, int64_t row_floats, void* stream);


/* ===================================================================================================
 * Training step: explicit backward pass, optimizer.
 *   replaces `losses.total.value.backward(); optimizer.step()` of gcp/prediction/train.py:155-163 (torch autograd +
 *   blox.torch.radam.RAdam, gcp_builder.py:178-179).  There is no autograd here: every gradient is a launch.
 * Data gradients of Linear / conv layers reuse gcpx_gemm / gcpx_conv3x3 with transposed weight packs.
 * ================================================================================================= */

/* ---- weight gradients: dW[n][k] = sum_r dY[r][n] * X[r][k] ---- */
typedef enum gcpx_wgrad_mode {
    GCPX_WG_ROWS = 0,      /* X row r at x + b*sb + (j+shift)*sr (b = r / rpb, j = r % rpb; zero outside [0,rpb)) or x + rowidx[r]*sr */
    GCPX_WG_CONV1D = 1,    /* k = (tap, ci), 3 taps along j: X[r][k] = x[b][j + tap - 1][ci] */
    GCPX_WG_CONV3X3 = 2,   /* k = (tap, ci): rows are pixels (f, y, x) of an NHWC [F][H][W][Cin] tensor, pad 1 */
    GCPX_WG_CONV4X4S2 = 3  /* k = (tap, ci), 16 taps: rows are output pixels (f, oy, ox) of the stride-2 conv over NHWC [F][H][W][Cin] */
} gcpx_wgrad_mode;
typedef enum gcpx_wgrad_map {
    GCPX_WMAP_LINEAR = 0,  /* dst[n*ldw + k_off + k] */
    GCPX_WMAP_CONV = 1,    /* k = (tap, ci): dst[(n_map[n]*Cin + ci)*ntap + tap]   (torch conv weight [Cout][Cin][taps]) */
    GCPX_WMAP_CONVT = 2    /* n = (tap, co), k = ci: dst[(k*Cout + co)*ntap + tap] (ConvTranspose2d weight [Cin][Cout][taps]) */
} gcpx_wgrad_map;

typedef struct gcpx_wgrad_args {
    const float* dy;        /* dev: [R][ldy] output gradient rows (dense) */
    const float* x;         /* dev: input operand (see mode) */
    const int32_t* rowidx;  /* ROWS: absolute row gather, or NULL */
    const int32_t* frame_map; /* conv modes: X frame = frame_map[f] (negative: zeros), or NULL */
    const float* scale;     /* per-channel affine + activation applied to X on load (channel = k % cmod, or ci), or NULL */
    const float* shiftv;
    float* out;             /* direct: dW[n*ldw + k_off + k]; partial: [nsplit][n_valid][K] */
    int64_t ldy, sb, sr, ldw;
    int64_t dy_sb;          /* 0: dy rows are dense (row r at dy + r*ldy); else row (b, j) at dy + b*dy_sb + j*ldy, b = r / dy_rpb */
    int32_t R, N, n_valid;  /* rows; columns of dy to read (N % 4 == 0 when > 16); rows of dW to write */
    int32_t K, mode, Cin, H, W, rpb, shift, act, cmod;
    int32_t k_off, accumulate, partial, nsplit;
    int32_t dy_rpb;
    int32_t nbatch;         /* > 1 (direct mode): blockIdx.z = b runs the same problem with dy advanced by b*z_dy_off, x by b*z_x_off,
                               out by b*z_out_off and dbias by b*z_bias_off floats (the 2*n_lstm_layers split_linear projections) */
    float* dbias;           /* optional (direct mode): dbias[n] (+)= sum_r dy[r][n], fused bias gradient */
    float* dbias2;          /* optional second destination of the same sums (LSTM b_ih / b_hh; not batched) */
    int64_t z_dy_off, z_x_off, z_out_off, z_bias_off;
    int32_t split_f16;      /* != 0: a direct-mode ROWS problem of whole 128 x 128 blocks of dW with >= 256 plain rows runs on the f16 matrix
                               pipes with f32-equivalent arithmetic (csrc/wgrad_rows_split.hip: both operands split into two f16 pieces in
                               the kernel, three MFMAs per product, f32 accumulate); everything else, and 0, runs the exact f32 kernel */
    int32_t _pad_split;
} gcpx_wgrad_args;

int gcpx_wgrad(const gcpx_wgrad_args* a, void* stream);
/* Grouped launch of up to 64 independent direct-mode problems that use the same kernel variant (the small per-level weight gradients of
   tree_module.py:67-114 / tree_lstm.py:43-49): gcpx_wgrad_classify gives the variant and workgroup count of one problem (host query);
   tab: DEVICE copy of the descriptors, block_start: DEVICE [nprob] first workgroup of each problem, total_blocks = their sum.
   The problems must write disjoint outputs. */
int gcpx_wgrad_classify(const gcpx_wgrad_args* a, int32_t row_split, int32_t* variant, int32_t* nblocks);   /* row_split: -1 = this problem's own heuristic, 0 / 1 = force */
int gcpx_wgrad_group(const gcpx_wgrad_args* tab, const int32_t* block_start, int32_t nprob, int32_t total_blocks, int32_t variant,
                     void* stream);
int gcpx_wgrad_reduce(const float* partial, int32_t nsplit, int32_t N, int32_t K, float* dst, int32_t map_mode, int32_t Cin,
                      int32_t ntap, int32_t Cout, const int32_t* n_map, int64_t ldw, int32_t k_off, int32_t accumulate,
                      void* stream);
/* LDS-tiled weight gradient of a 3x3 conv (pad 1): dy [F*H*W][ldy] (Cout rounded up to 16 columns are read), u NHWC
   [F][H][W][Cin]; writes partial [grid][ceil16(Cout)][9*Cin] (k = tap*Cin + ci), one row block per persistent workgroup,
   to be combined by gcpx_wgrad_reduce(map CONV).  H, W powers of two, W in {8, 16, 32k}. */
int gcpx_wgrad_conv3x3(const float* dy, int32_t ldy, const float* u, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                       float* partial, int32_t grid, void* stream);
/* The same contract on the f16 matrix pipes with f32-equivalent arithmetic (csrc/wgrad_conv_split.hip: both operands split into two
   f16 pieces in the kernel, three MFMAs per product, f32 accumulate, running power-of-two scales per workgroup).  Shapes it does not
   cover run on gcpx_wgrad_conv3x3. */
int gcpx_wgrad_conv3x3_split(const float* dy, int32_t ldy, const float* u, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                             float* partial, int32_t grid, void* stream);
/* The same for an UPSAMPLING block with 16 output channels, reading the block's own low-resolution sources: `a` is the block's forward
   descriptor as gcpx_conv_stage takes it (src / nsrc / F / Hin / Win / Hout / Wout / Cin, upsample = 1, no src_row_map); the kernel forms
   the bilinear x2 of the concatenated, normalised + activated sources per tile, so the operand tensor gcpx_conv_stage would write
   (additional_conv_layer at c2: 1.07 GB per step, read back by the weight gradient) never exists.  GCPX_ERR_UNSUPPORTED (nothing
   launched) when the shape has no fused form: Cout <= 16, Cin % 32 == 0, source widths % 16 == 0, W in {8, 16, 32 k}. */
int gcpx_wgrad_conv3x3_split_up(const float* dy, int32_t ldy, const gcpx_conv_args* a, int32_t Cout, float* partial, int32_t grid,
                                void* stream);
/* ... and for a NON-upsampling conv whose operand is LeakyReLU(0.2)(scale * x + shift) of a raw tensor x [Fx][H][W][Cin] read through a
   frame map (operand frame f = frame frame_map[f] of x; a negative entry must carry a zero dy): the output head's weight gradient reads
   the last decoder block's raw output at the matched nodes — the gathered, activated copy gcpx_conv_stage would write (335 MB at c2)
   never exists.  frame_map, or scale + shift, may be NULL.  bias_partial (optional; the 112-column head form only): [grid][112]
   per-workgroup column sums of dy over every pixel = the bias gradient, from the same staged tiles (sum over the grid with
   gcpx_wgrad_reduce): no gcpx_colsum pass over dy (2.35 GB at c2). */
int gcpx_wgrad_conv3x3_split_src(const float* dy, int32_t ldy, const float* x, const int32_t* frame_map, const float* scale,
                                 const float* shift, int32_t F, int32_t H, int32_t W, int32_t Cin, int32_t Cout, float* partial,
                                 float* bias_partial, int32_t grid, void* stream);
/* bias gradient: dst[n] (+)= sum_r dy[r][n] (rows addressed like gcpx_wgrad_args.dy); dst2 = optional second destination
   (LSTM b_ih and b_hh); with nsplit > 1 the row range is split and partial [nsplit][N] is written instead of dst */
int gcpx_colsum(const float* dy, int64_t ldy, int32_t R, int32_t N, int32_t dy_rpb, int64_t dy_sb, int32_t nsplit, float* partial,
                float* dst, float* dst2, int32_t accumulate, void* stream);
/* dst[i] (+)= sum_{p < n} partial[p*stride + i], i < len (per-workgroup partial sums of norm parameters) */
int gcpx_reduce_partials(const float* partial, int32_t n, int64_t stride, int32_t len, float* dst, int32_t accumulate, void* stream);

/* ---- LSTM cell backward (HiddenStatePredictorModel inside tree_lstm.py:43-49) ---- */
typedef struct gcpx_lstm_bwd_args {
    const float* gates;     /* [M][H][4] activated gates saved by the forward (gcpx_gemm_args.gates_out) */
    const float* c_prev;    /* row r at c_prev + r*c_prev_stride */
    const float* c_new;     /* row (b, j) at c_new + b*pb + j*prow */
    const float* dh_dense;  /* [M] rows at dh_dense + r*dh_stride: gradient from the layer above, or NULL */
    const float* dh_pos;    /* gradient w.r.t. the stored hidden state h (from the children), at dh_pos + b*pb + j*prow, or NULL */
    const float* dc_pos;    /* same for the stored cell state c, or NULL */
    float* dgates;          /* [M][4H] pre-activation gate gradients, torch gate-major order (i | f | g | o) */
    float* dc_prev;         /* row r at dc_prev + r*dcp_stride */
    int64_t c_prev_stride, pb, prow, dh_stride, dcp_stride;
    int32_t M, H, rpb, _pad;
} gcpx_lstm_bwd_args;
int gcpx_lstm_bwd(const gcpx_lstm_bwd_args* a, void* stream);

/* ---- Predictor MLP pieces ---- */
/* GroupNorm + LeakyReLU backward on dense rows: du = dGN(u) applied to da * lrelu'; partial: [gcpx_gn_bwd_blocks(M)][2][C]
   per-workgroup sums of (d gamma, d beta) */
int gcpx_gn_lrelu_bwd(const float* u, const float* da, const float* gamma, const float* beta, float* du, float* partial,
                      int32_t M, int32_t C, int32_t groups, float eps, float slope, void* stream);
int gcpx_gn_bwd_blocks(int32_t M);
/* Fused data-gradient chain of one Predictor MLP (mirror of gcpx_mlp; backward of tree_module.py:77 / inference.py:27-35, which
   the reference gets from autograd): dout [M][ldo] -> head^T -> (GroupNorm + LReLU backward -> mid_l^T) x n_mid -> LReLU
   backward -> per input split dx_i = du0 @ W_in[:, split i].  `save` = the buffer gcpx_mlp_args.save filled in the forward.
   Writes every du_l ([M][mid]; operands of the weight-gradient GEMMs), the per-workgroup GroupNorm parameter sums
   gn_partial[l] [gcpx_mlp_bwd_blocks(M)][2][mid] (reduce with gcpx_reduce_partials) and the dx_i rows (b, j) at
   out + b*ob + j*orow (b = r / rpb).  wT_*: gcpx_gemm packs of the transposed weights. */
typedef struct gcpx_mlp_bwd_dx {
    const float* wT;        /* pack of W_in[:, split]^T: [mid / 16][width / 16][64][4] */
    float* out;
    int64_t ob, orow;
    int32_t width, _pad;
} gcpx_mlp_bwd_dx;
typedef struct gcpx_mlp_bwd_args {
    const float* dout;
    const float* save;
    const float* wT_out;    /* [out_pad / 16][mid / 16][64][4] */
    const float* wT_mid[4];
    const float* gn_gamma[4];
    const float* gn_beta[4];
    float* du[5];           /* du[0]: input layer (after its LReLU backward); du[1 + l]: hidden layer l */
    float* gn_partial[4];
    gcpx_mlp_bwd_dx dx[4];
    int64_t ldo;
    int32_t M, rpb, mid, n_mid, out_pad, ndx;
    float gn_eps, lrelu_slope;
} gcpx_mlp_bwd_args;
int gcpx_mlp_bwd(const gcpx_mlp_bwd_args* a, void* stream);
/* nprob (<= GCPX_MLP_BWD_GROUP_MAX) Predictors of one hidden width whose chains are independent, in ONE launch (blockIdx.y = the
   Predictor; tab: HOST array, copied into the kernel arguments): a tree level's posterior and prior share the level's latency-bound
   chain.  Bit for bit what one gcpx_mlp_bwd per Predictor writes. */
#define GCPX_MLP_BWD_GROUP_MAX 4
int gcpx_mlp_bwd_group(const gcpx_mlp_bwd_args* tab, int32_t nprob, void* stream);
int gcpx_mlp_bwd_blocks(int32_t M);
/* dx[r][c] = dy[r][c] * (1 - y[r][c]^2), backward of y = tanh(u) (GCPX_MLP_TANH; tree_module.py:109-110): dy and y rows (b, j) at
   base + b*sb + j*sr, dx dense [B*rpb][width] */
int gcpx_tanh_bwd_rows(const float* dy, const float* y, float* dx, int64_t sb, int64_t sr, int32_t B, int32_t rpb, int32_t width,
                       void* stream);
/* dx[i] = dy[i] * (a[i] > 0 ? 1 : slope) */
int gcpx_lrelu_bwd(const float* a, const float* dy, float* dx, int64_t n, float slope, void* stream);

/* ---- latent variables ---- */
/* d KL(q||p) (inference.py:38-43): writes d q / d p rows ([mu | log_sigma]) at the same addresses as qz / pz rows */
int gcpx_kl_bwd(const float* qz, const float* pz, float* dqz, float* dpz, int32_t B, int32_t N, int32_t nz, int64_t batch_stride,
                int64_t node_stride, float free_nats, float coef, void* stream);
/* the same with a per-node weight (the flat VRNN's KL term carries pad_mask[:, 1:], sequential.py:63-66):
   gradient rows scaled by node_weight[b * weight_bstride + n] */
int gcpx_kl_bwd_weighted(const float* qz, const float* pz, float* dqz, float* dpz, int32_t B, int32_t N, int32_t nz, int64_t batch_stride,
                         int64_t node_stride, float free_nats, float coef, const float* node_weight, int64_t weight_bstride, void* stream);
/* the general form with the scheduled part of the weight in device memory: gradient rows scaled by coef * (*coef_dev) (* node_weight
   when given) — the KL weight burn-in (base_gcp.py:121-128) */
int gcpx_kl_bwd_scheduled(const float* qz, const float* pz, float* dqz, float* dpz, int32_t B, int32_t N, int32_t nz, int64_t batch_stride,
                          int64_t node_stride, float free_nats, float coef, const float* node_weight, int64_t weight_bstride,
                          const float* coef_dev, void* stream);
/* one tree level: dq_out[r] = dqz_pos[r] + [dz, dz * exp(log_sigma_q) * eps] (reparametrised sample backward,
   tree_module.py:86-94), dp_out[r] = dpz_pos[r]; rows r = (b, j) of the level; *_pos at base + b*pb + j*prow;
   dz = dz0[r*ldz0 ..] (+ dz1[r*ldz1 ..]); eps at eps + b*eb + j*erow */
int gcpx_latent_bwd(const float* dqz_pos, const float* dpz_pos, const float* qz_pos, int64_t pb, int64_t prow, const float* eps,
                    int64_t eb, int64_t erow, const float* dz0, int64_t ldz0, const float* dz1, int64_t ldz1, float* dq_out,
                    float* dp_out, int32_t M, int32_t rpb, int32_t nz, void* stream);

/* gradients of one level's inputs accumulated into the parents' slots of a position-layout buffer (the backward of
   tree_utils.py:37-44 interleave + the context broadcast of tree_module.py:97-101) */
typedef struct gcpx_tree_accum_src {
    const float* ptr;       /* dense [B*n][ld] */
    int64_t ld;
    int32_t off_left, off_right, off_ctx0, off_ctxg;   /* column offsets of the e_l / e_r / e_0 / e_g parts, -1 = absent */
    int32_t dst_col;        /* column offset inside the destination row */
    int32_t _pad;
} gcpx_tree_accum_src;
typedef struct gcpx_tree_accum_args {
    gcpx_tree_accum_src src[6];
    float* dst;             /* slot 0 of batch element 0 */
    int64_t dst_sb;         /* floats between batch elements */
    int64_t slot_stride;    /* floats between consecutive parent slots of this level */
    int32_t nsrc, B, n, width;
} gcpx_tree_accum_args;
int gcpx_tree_accum(const gcpx_tree_accum_args* a, void* stream);
/* backward of the posterior's batchwise_index gather (inference.py:27-33): out[b][t] = sum over nodes p with node_t[b][p] == t
   of det[b][p] (rows of nz floats at det + b*db + p*dp) */
int gcpx_timestep_scatter(const float* det, int64_t db, int64_t dp, const int32_t* node_t, float* out, int32_t B, int32_t N,
                          int32_t T, int32_t nz, void* stream);

/* dst row (b, j) at dst + b*dst_sb + j*dst_sr  +=  src1[r] (+ src2[r]), dense sources [B*rpb][width] */
int gcpx_add_rows(float* dst, int64_t dst_sb, int64_t dst_sr, const float* src1, const float* src2, int32_t B, int32_t rpb,
                  int32_t width, void* stream);
/* rows (b, j), j < rpb, of `width` floats between two strided layouts (row at base + b*sb + j*sr): mode 0 dst = src, 1 dst += src,
   2 dst[b] += sum over j of src[b][j] (dst_sr unused; fixed summation order).  Gradient bookkeeping of the recurrent rollout
   (sequential.py:49-54 backward): x_t / context slices of the per-step embedding gradients */
int gcpx_rows_strided(float* dst, int64_t dst_sb, int64_t dst_sr, const float* src, int64_t src_sb, int64_t src_sr, int32_t B, int32_t rpb,
                      int32_t width, int32_t mode, void* stream);
/* rows r of `row_floats` floats with row2frame[r] < 0 are set to zero (rows of the matched-frame gradient no decoded frame maps to:
   padded frames t > end_ind; the head kernel in GCPX_HEAD_DLM_NLL_GRAD mode writes only mapped rows) */
int gcpx_zero_unmapped_rows(float* ptr, int64_t row_floats, const int32_t* row2frame, int32_t rows, void* stream);
/* out[b][t] = idx[b][t] + b*stride (per-sequence node index -> absolute frame index) */
int gcpx_index_offset(const int32_t* idx, int32_t* out, int32_t B, int32_t T, int32_t stride, void* stream);
/* inv[r] = i for every i < n with fwd[i] = r >= 0 (fwd injective on its non-negative entries), -1 for rows nobody maps to:
   the src_row_frames companion of a src_row_map (gcpx_conv_args) */
int gcpx_index_inverse(const int32_t* fwd, int32_t n, int32_t* inv, int32_t n_inv, void* stream);

/* ---- conv stacks ---- */
/* gradient w.r.t. the raw (pre-norm) output of a layer from the gradient w.r.t. its activated output:
   dy = (T(da) + add) * act'(scale*r + shift), where T is identity, the transposed bilinear x2 upsample (up = 1) and / or
   the sum over `fsum` consecutive frames (backward of the skip broadcast); with mean/rstd also the per-workgroup partial
   sums [gcpx_act_bwd_blocks()][2][C] of (dy, dy * x_hat) the BatchNorm backward needs. */
typedef struct gcpx_actbwd_args {
    const float* da;        /* NHWC [F*fsum][H*(1+up)][W*(1+up)][ldc], channels c_off .. c_off+C */
    const float* add;       /* [F][H][W][C] or NULL */
    const float* r;         /* [F][H][W][C] raw output (or activated output when scale == NULL) or NULL (no activation) */
    const float* scale;
    const float* shift;
    const float* mean;      /* [C] batch statistics, or NULL (no norm: no partial sums) */
    const float* rstd;
    float* dy;              /* [F][H][W][C] */
    float* stats_partial;
    int64_t ldc;
    int32_t c_off, up, fsum, act, F, H, W, C;
} gcpx_actbwd_args;
int gcpx_act_bwd(const gcpx_actbwd_args* a, void* stream);
int gcpx_act_bwd_blocks(void);
/* gcpx_act_bwd (up = 1, fsum = 1) for the channels a->c_off .. + a->C of an upsampling decoder block's input gradient AND, from the same pass
   over the tensor, the skip-connection half: ds [F / rpb][H][W][Cs] = sum over the rpb frames of a sequence of the (bilinear-transposed)
   channels c_off_s .. + Cs (the two gcpx_act_bwd launches of training.py's decoder backward, tree_dense_rec.py:42 / base_gcp.py:190) */
int gcpx_act_skip_bwd(const gcpx_actbwd_args* a, float* ds, int32_t c_off_s, int32_t Cs, int32_t rpb, void* stream);
/* BatchNorm backward, second half: coef[0..C) = gamma*rstd, coef[C..2C) = mean(dy), coef[2C..3C) = mean(dy*x_hat);
   d gamma / d beta written (accumulated) to the gradient buffers */
int gcpx_bn_bwd_finalize(const float* partial, int32_t n_partial, int32_t C, double count, const float* gamma, const float* rstd,
                         float* coef, float* dgamma, float* dbeta, int32_t accumulate, void* stream);
/* dr = coef0 * (dy - coef1 - x_hat * coef2), in place over dy; channel = index % C */
int gcpx_bn_bwd_apply(float* dy, const float* r, const float* mean, const float* rstd, const float* coef, int64_t n, int32_t C,
                      void* stream);
/* materialise the (upsampled, concatenated, normalised + activated) input of a 3x3 conv block for its weight gradient:
   uses src / nsrc / F / Hin / Win / Hout / Wout / Cin / upsample / src_row_map / out of gcpx_conv_args; out NHWC [F][Hout][Wout][Cin] */
int gcpx_conv_stage(const gcpx_conv_args* a, void* stream);
/* backward of the stride-2 4x4 conv w.r.t. its input: dx[f][iy][ix][ci] = sum of the (at most 4) taps of
   dcol [F*H/2*W/2][16*Cin] (k = (tap, ci)) that touched the pixel */
int gcpx_col2im4x4s2(const float* dcol, float* dx, int32_t F, int32_t H, int32_t W, int32_t Cin, void* stream);
/* im2col of the NCHW 3-channel image for the first encoder conv's weight gradient: col [F*H/2*W/2][48], k = (ci, ky, kx) */
int gcpx_im2col_image(const float* x, float* col, int32_t F, int32_t H, int32_t W, void* stream);
/* Weight + bias gradient of the encoder's first layer (4x4 stride-2 pad-1 conv on the NCHW image, LeakyReLU, no norm) in one launch:
   (da + add) * slope(r) against the image patches (csrc/wgrad_image.hip; replaces gcpx_act_bwd + gcpx_im2col_image + gcpx_wgrad +
   gcpx_colsum for that layer).  da / add (or NULL) / r: NHWC [F][S/2][S/2][16]; image [F][3][S][S]; partial [grid][16*48 + 16]
   (weights [co][ci*16 + ky*4 + kx], then the bias), to be summed by gcpx_reduce_partials(stride 784). */
int gcpx_wgrad_image4x4s2(const float* da, const float* add, const float* r, const float* image, int32_t F, int32_t S, float* partial,
                          int32_t grid, void* stream);

/* ---- loss gradients ---- */
/* d NLL / d params of the discretised logistic mixture (same layouts as gcpx_dlm_nll); row gradient scaled by
   row_weight[row] * scale; rows with weight 0 are zero-filled.  colsum (optional): [rows][pitch] per-row sums over the
   pixels of dparams (the output head's bias gradient, summed over rows by gcpx_colsum).  nll_out (optional): [rows] the same
   values gcpx_dlm_nll writes — the training step evaluates loss and gradient in ONE pass over the 2.3 GB of parameters */
int gcpx_dlm_nll_bwd(const float* params, const float* target, const float* row_weight, float scale, float* dparams, float* colsum,
                     float* nll_out, int32_t rows, int32_t npix, int32_t pitch, int32_t n_mix, void* stream);
/* The same for the gaussian head, whose likelihood is taken of mu = tanh(y) (GCPX_HEAD_TANH_NCHW): mu, target NCHW [rows][C][npix],
   log_sigma one device scalar (decoder.log_sigma).  dy [rows][npix][pitch] = d (scale * row_weight[row] * NLL) / d y, the head's
   PRE-tanh output, in the pixel-record layout the head's weight / data gradient launches read: slot c < C =
   scale * w_row * (mu - x) * exp(-2 log_sigma) * (1 - mu^2), slots C .. pitch-1 = 0; rows with weight 0 are zero-filled
   (row_weight NULL: every weight 1).  colsum (optional): [rows][pitch] per-row sums of dy over the pixels (the head's bias gradient,
   summed over rows by gcpx_colsum).  nll_out (optional): [rows] what gcpx_gauss_nll reports, for rows of weight 0 too.
   dls_rows [rows]: scale * w_row * sum over the row of (1 - ((x - mu) * exp(-log_sigma))^2), the rows' contributions to
   d total / d log_sigma (sum them with gcpx_reduce_partials).  All sums in a fixed order, no atomics.
   Shape contract: 1 <= C <= 4 and C <= pitch; pitch % 4 == 0, pitch <= 256; npix % 64 == 0; npix * pitch < 2^31.  Anything else
   returns GCPX_ERR_INVALID_ARG and launches nothing. */
int gcpx_gauss_nll_bwd(const float* mu, const float* target, const float* row_weight, const float* log_sigma, float scale, float* dy,
                       float* colsum, float* nll_out, float* dls_rows, int32_t rows, int32_t C, int32_t npix, int32_t pitch,
                       void* stream);
/* d total / d logits of the length CE, existence BCE and state L2 heads (same arguments as gcpx_loss_combine);
   dlen [B][ceil16(T)] (pad columns zero), dexist [B*N][16] (column 0), dstate [B*T][16] (columns < state_dim); NULL outputs are skipped */
int gcpx_loss_heads_bwd(const gcpx_loss_args* a, float* dlen, float* dexist, float* dstate, void* stream);
/* same for the inverse-model and cost-model L2 heads: daction [B][16] (columns < n_actions), dcost [B][16] (column 0) */
int gcpx_loss_aux_heads_bwd(const gcpx_loss_args* a, float* daction, float* dcost, void* stream);

/* ---- parameters ---- */
/* dst[i] = theta[idx0[i]] (+ theta[idx1[i]]), negative index = 0: every fragment-packed weight arena is a gather of the
   canonical flat parameter vector (video-gcp_amd/packing.py), refreshed once per optimizer step.  idx0 / idx1 / dst 16-byte aligned;
   n is any positive count: four elements per thread, and the last n % 4 go through a scalar tail (every call site of
   video-gcp_amd/weights.py passes a multiple of 4, its arena leaves being padded to one) */
int gcpx_repack(const float* theta, const int32_t* idx0, const int32_t* idx1, float* dst, int64_t n, void* stream);
/* the same, held to max_blocks 256-thread workgroups (0 = no limit): see gcpx_optim_range */
int gcpx_repack_blocks(const float* theta, const int32_t* idx0, const int32_t* idx1, float* dst, int64_t n, int32_t max_blocks, void* stream);
/* split-f16 weights from the flat parameter vector (one launch per tensor, after gcpx_repack): v[i] = theta[idx[i]] (negative = 0),
   e = 14 - floor(log2 max|v|) (0 when all zero), *log2_out = e, and the two f16 pieces of v[i] 2^e in the layout the split kernels
   read: out[((i / 512) * 2 + p) * 512 + i % 512], p = 0 (rn16(v 2^e)) and 1 (rn16 of the remainder); n % 512 == 0.  Same pieces as
   packing.split_f16 on the host */
int gcpx_split_pack(const float* theta, const int32_t* idx, int32_t n, void* out, int32_t* log2_out, void* stream);
/* The same for several tensors in one launch (one workgroup per tensor; csrc/split_pack.hip): tab = DEVICE array of descriptors */
typedef struct gcpx_split_pack_desc {
    const float* src;        /* flat parameter vector (or the folded weights of a row-folded block) */
    const int32_t* idx;      /* [n] gather indices into src, -1 = zero */
    void* out;               /* [n / 512][2][512] f16 */
    int32_t* log2_out;       /* exponent of the tensor */
    int32_t n, _pad;
} gcpx_split_pack_desc;
int gcpx_split_pack_group(const gcpx_split_pack_desc* tab, int32_t nprob, void* stream);
/* The same result, bit for bit, from two launches with 32 workgroups per tensor (largest magnitudes first, then the pieces): the form
   the trainer runs behind every optimizer step.  scratch: DEVICE [nprob] uint32, overwritten */
int gcpx_split_pack_group2(const gcpx_split_pack_desc* tab, int32_t nprob, uint32_t* scratch, void* stream);
/* Row-folded weights of an upsampling decoder block (bilinear x2, align_corners=False, then 3x3 conv, pad 1 — DecoderModule's
   pyramid / additional_conv_layer blocks, blox; called through gcp/prediction/models/tree/tree_dense_rec.py:42).  Output row
   2 y + py of the block reads the three low-resolution rows y - 1, y, y + 1 (clamped) of the horizontally interpolated input with
   weights that are fixed linear combinations of the conv's three tap rows:
       py = 0:  [0.75 W0 + 0.25 W1,  0.25 W0 + 0.75 W1 + 0.75 W2,  0.25 W2]
       py = 1:  [0.25 W0,  0.75 W0 + 0.75 W1 + 0.25 W2,  0.25 W1 + 0.75 W2]
   and the conv's zero padding above row 0 / below the last row is restored by the correction sets -W0 (on the clamped row above)
   and -W2 (on the clamped row below).  w: dev [Cout][Cin][3][3]; out: dev f32 [24][Cout][Cin], set t = py 9 + dyl 3 + tx for
   t < 18, 18 + tx = -W0[tx], 21 + tx = -W2[tx]; sums formed in float64 in tap-row order (bit-identical to packing.fold_up_weights). */
int gcpx_fold_upsample_weights(const float* w, int32_t Cout, int32_t Cin, float* out, void* stream);
/* The optimizer state is four floats: state[0] = step counter (a float: exact to 2^24 steps, where it stays), state[1] = this step's
   gradient-clipping coefficient: > 0 the coefficient, 0 = unset = 1 (a zeroed state means "no clipping"), < 0 = the coefficient is
   ZERO (gcpx_grad_clip_coef writes -1 when the norm overflowed to inf or max_norm / norm underflowed: the gradient does not enter the
   step, as clip_grad_norm_ scales it to 0; stored as 0 it would read as unset and the exploded gradient would be applied whole),
   state[2] = the norm gcpx_grad_clip_coef measured, state[3] = the GATE.  With state[3] != 0 every step entry point below
   (gcpx_radam_step, gcpx_optim_step, gcpx_optim_range, whatever kind and tick) returns at kernel entry: theta, m, v and state[0] keep
   their bits.  gcpx_grad_health writes the gate (1 = this step's gradient or loss is not finite, 0 = clean) on every call; a caller
   without a guard leaves it 0, and every result is then what it was before the slot had a meaning.
   The scalar coefficients of a step (beta1^t, beta2^t, RAdam's sma_max, sma and rectification term, Adam's bias corrections) are
   formed in double from the float hyperparameters and the counter and rounded to float once: they are correct to float32 rounding for
   every beta2 < 1 and t <= 2^24, and RAdam's sma >= 5 switch is the double-precision decision.  The element-wise arithmetic is float32. */
/* RAdam (Liu et al. 2019; blox.torch.radam.RAdam as used by gcp_builder.py:178-179): state[0] = step counter (float),
   incremented by this call; rectified update when the variance is tractable (rho_t > 5), momentum SGD otherwise */
int gcpx_radam_step(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, float* state, int64_t n, float lr,
                    float beta1, float beta2, float eps, float grad_scale, void* stream);
/* The trainer's other optimizers (gcp_builder.py:174-186; torch.optim.Adam / RMSprop / SGD formulas): kind 1 = adam (p1, p2 = betas),
   2 = rmsprop (p1 = momentum, p2 = alpha), 3 = sgd (p1 = momentum).  m / v: the optimizer's two state vectors; state[0] = step
   counter (incremented), state[1] = gradient-clipping coefficient applied to the (scaled) gradient (0 = unset = 1, < 0 = zero; set per
   step by gcpx_grad_clip_coef; gcpx_radam_step applies it too). */
int gcpx_optim_step(float* theta, const float* grad, float* m, float* v, float* state, int64_t n, int32_t kind, float lr, float p1,
                    float p2, float eps, float grad_scale, void* stream);
/* One slice of an optimizer step: kind 0 = RAdam (p1, p2 = betas), 1 .. 3 as gcpx_optim_step, over n elements of the four vectors;
   state[0] is incremented only when tick != 0.  A trainer whose gradient becomes final slice by slice (the tree levels of the backward
   pass, leaves first) applies each slice while the rest is still being differentiated and ticks with the last one: every slice of a
   step must read the same counter, so all tick == 0 calls of a step are ordered before its tick != 0 call.  The same arithmetic per
   element as gcpx_radam_step / gcpx_optim_step (a step cut into slices gives the same bits as one call).  max_blocks > 0 holds the
   launch to that many 256-thread workgroups: a slice applied beside the backward's critical chain must leave it the chip (a full
   grid's wavefronts fill every CU and stretched the chain's 40 us GEMMs to 100 us). */
int gcpx_optim_range(float* theta, const float* grad, float* m, float* v, float* state, int64_t n, int32_t kind, float lr, float p1,
                     float p2, float eps, float grad_scale, int32_t tick, int32_t max_blocks, void* stream);
/* gradient_clip (gcp_builder.py:186 -> blox get_clipped_optimizer; spec here: torch.nn.utils.clip_grad_norm_ over all parameters):
   state[2] = || grad_scale * grad ||_2, state[1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0; -1 when that coefficient
   is exactly 0, see the state above: a float32 sum of squares that overflows gives norm = inf).  partial: [n_partial] scratch
   (deterministic two-stage sum: workgroup b adds the squares of elements b 256 + i + k 256 n_partial per thread i, then a tree;
   one workgroup adds the partials the same way). */
int gcpx_grad_clip_coef(const float* grad, int64_t n, float grad_scale, float max_norm, float* partial, int32_t n_partial, float* state,
                        void* stream);
/* Gradient accumulation over the micro-batches of one optimizer step (the trainer's accumulate=k; no reference counterpart: k
   micro-batches stand for the k replicas of nn.DataParallel, gcp_builder.py:71-78).  assign = 0: dst[i] = dst[i] + src[i]; assign = 1:
   dst[i] = src[i] (the first micro-step of a cycle: no separate zero pass).  Exactly one float32 addition per element, nothing
   contracted: the result does not depend on how a vector is cut into slices, and NaN / +-Inf propagate (gcpx_grad_health reads the
   sum).  dst and src are any 4-byte aligned, non-overlapping slices (the bucket ranges of the flat gradient start anywhere): both
   16-byte aligned takes four elements per access, two accesses in flight; the remainder and unaligned slices a scalar loop.  Nothing
   outside [dst, dst + n) is written.  max_blocks as in gcpx_optim_range (0 = full grid).  n = 0 is a no-op that returns 0.
   Memory bound: 12 n bytes of traffic (8 n with assign). */
int gcpx_grad_accumulate(float* dst, const float* src, int64_t n, int32_t assign, int32_t max_blocks, void* stream);
/* Exponential moving average of the weights (the trainer's ema_decay; no reference counterpart).  With omd = 1.0f - decay formed once
   in float32 (exact for decay >= 0.5, Sterbenz), per element: d = theta[i] - ema[i] (one float32 rounding), ema[i] = fmaf(omd, d, ema[i])
   (one rounding); nothing else is contracted or reassociated, so the result does not depend on how a vector is cut into calls, and
   NaN / +-Inf propagate (the training guard, not this kernel, keeps them out).  gate: NULL = always update; otherwise one device float
   read at kernel entry, non-zero = return having written nothing (the trainer passes opt_state + 3: a step gcpx_grad_health closed
   moves the average no more than it moves theta or the moments).  ema and theta are any 4-byte aligned, non-overlapping slices: both
   16-byte aligned takes four elements per access, two accesses in flight; the last n % 4 elements and unaligned slices a scalar loop.
   Nothing outside [ema, ema + n) is written.  max_blocks as in gcpx_optim_range (0 = full grid).  n = 0 returns 0 and launches
   nothing.  decay outside (0, 1) or NaN, n < 0, a null ema or theta with n > 0: GCPX_ERR_INVALID_ARG before any HIP call.
   Memory bound: 12 n bytes of traffic. */
int gcpx_ema_update(float* ema, const float* theta, int64_t n, float decay, const float* gate, int32_t max_blocks, void* stream);
/* Exchanges [a, a + n) and [b, b + n) as 32-bit words (the trainer's ema_weights(): theta <-> average): NaN payloads and -0 keep
   their bits.  Alignment, max_blocks, n = 0 and the argument checks as in gcpx_ema_update; nothing outside the two ranges is
   written; overlapping ranges are the caller's error.  Memory bound: 16 n bytes of traffic. */
int gcpx_swap_f32(float* a, float* b, int64_t n, int32_t max_blocks, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * hipGraph helpers: capture a launch sequence once, replay it per step.
 * ------------------------------------------------------------------------------------------------- */
int gcpx_graph_begin(void* stream);
int gcpx_graph_end(void* stream, void** graph_exec);
int gcpx_graph_launch(void* graph_exec, void* stream);
int gcpx_graph_destroy(void* graph_exec);

/* side streams for the independent branches of the forward (the I_0 / I_g encoder passes, the per-level
   split_linear merge and prior next to the posterior chain, the aux heads next to the decoder).  Under
   gcpx_graph_begin/_end a gcpx_event_record on the capturing stream followed by gcpx_stream_wait_event on a side
   stream forks the capture; the reverse joins it, so the branches become parallel paths of the hipGraph. */
int gcpx_stream_create(void** stream);
/* level < 0: highest priority of the device, 0: middle, > 0: lowest (side lanes that must not delay the critical chain) */
int gcpx_stream_create_priority(void** stream, int level);
int gcpx_stream_destroy(void* stream);
int gcpx_stream_wait_event(void* stream, void* ev);

/* event timing on the caller's stream (bench.py measures the dominant kernel with these) */
int gcpx_event_create(void** ev);
int gcpx_event_create_sync(void** ev);   /* ordering only: no timing, device-scope release (lane fork / join) */
int gcpx_event_record(void* ev, void* stream);
int gcpx_event_elapsed_ms(void* start, void* stop, float* ms);
int gcpx_event_destroy(void* ev);

/* ===================================================================================================
 * Adaptive (soft-DTW) frame binding + attentive inference — the long-horizon configuration
 *   (experiments/prediction/base_configs/gcp_adaptive.py:6-11: matching_type='dtw_image', attentive_inference=True).
 * ================================================================================================= */

/* Masked single-query multi-head attention of the attentive posterior
 *   (blox MultiheadAttention as called at adaptive_binding/attentive_inference.py:81; q / k / v already projected):
 *   row r = (b, j), b = r / rpb:  score[h][t] = q[r][h] . k[b][t][h] / sqrt(dk / heads) / temperature[0],
 *   frames outside [start_ind[b], end_ind[b]] masked out, softmax over t, out[r][h] = sum_t a[h][t] v[b][t][h].
 *   q [M][dk], k [B][T][dk], v [B][T][nz], out [M][nz] dense; att [M][T] = head-averaged weights or NULL;
 *   start_ind NULL = 0.  Caller's contract: end_ind[b] in [0, inf) — an end_ind at or beyond T is clamped to T - 1; start_ind[b] >= 0.
 *   Keys and values outside the window are never used (the value rows outside it are not read).
 *   A row whose window is empty (start_ind[b] > end_ind[b], or start_ind[b] >= T) is a softmax over nothing: every element of
 *   out[r] and att[r] is NaN, what the reference's masking (scores outside the window at -inf, then softmax) gives; the other
 *   rows of the launch are not affected. */
int gcpx_attention(const float* q, const float* k, const float* v, const int64_t* start_ind, const int64_t* end_ind,
                   const float* temperature, float* out, float* att, int32_t M, int32_t rpb, int32_t T, int32_t dk, int32_t nz,
                   int32_t heads, void* stream);

/* batch_cdist(x, y, reduction='sum') of adaptive.py:44 / binding_loss.py:24 (blox.torch.ops.batch_cdist): squared L2 distance
 *   out[b][n][t] = max(0, |x[b][n]|^2 + |y[b][t]|^2 - 2 x[b][n] . y[b][t]),  x [B][N][K], y [B][T][K], K % 32 == 0.
 *   f32 MFMA GEMM with gcpx_cdist_splits(K) deterministic split-K partials: partial [splits][B][N][T], xnorm [B*N], ynorm [B*T]
 *   are caller-owned scratch. */
int gcpx_cdist_splits(int64_t K);
int gcpx_cdist(const float* x, const float* y, int32_t B, int32_t N, int32_t T, int64_t K, float* partial, float* xnorm,
               float* ynorm, float* out, void* stream);
/* gcpx_cdist with x read where it lies: row (b, n) is the K floats at x + b * x_sb + n * x_sr (strides in floats, multiples of 4,
 *   x 16-byte aligned; x_sr >= K, and a batch element's rows end before the next one's begin).  y, the scratch and out as above;
 *   the same kernels in the same order, so with x_sb = N * K, x_sr = K the result has the bits of gcpx_cdist.
 *   Call site: forward_plan.py, the `matching` block with matching_type = 'dtw_latent' (adaptive.py:45-47: the cost between
 *   tree.df.e_g_prime and enc_traj_seq) — the node latents in position layout, node n at slot n + 1: x = E + nz_enc,
 *   x_sb = (2^L + 1) * nz_enc, x_sr = nz_enc, K = nz_enc; no gathered copy. */
int gcpx_cdist_strided(const float* x, int64_t x_sb, int64_t x_sr, const float* y, int32_t B, int32_t N, int32_t T, int64_t K,
                       float* partial, float* xnorm, float* ynorm, float* out, void* stream);

/* soft_dtw(cost / temp, end_ind) + normalize(w, 1) of adaptive.py:50-58 (probabilistic_dtw.py:11-122), float64 inside:
 *   cost[b][n][t] = (dsum[b][n][t] / D) / temp[0]  ('mean' reduction of the cdist, then the matching temperature);
 *   w[b][n][t] = P(node n is aligned with frame t) under the Gibbs distribution over monotone alignments without horizontal
 *   moves that start at (0, 0) and end at (N-1, end_ind[b]), divided by max(sum over nodes, 1e-7).  Depth-first node order.
 *   acc: caller-owned scratch, float64 [2*B][N][T] (forward and backward accumulators, both in the orientation of dsum; -inf where
 *   no alignment reaches).  Every cell of acc and w is written; columns beyond end_ind[b] of w are exact zeros.
 *   Needs N >= T, T <= 1024 (GCPX_ERR_UNSUPPORTED beyond, nothing written).
 *   Caller's contract: end_ind[b] in [0, T-1].  It is used as a column index without a check; a value outside is an out-of-bounds
 *   read.  The same holds for gcpx_soft_dtw_dtemp. */
int gcpx_soft_dtw(const float* dsum, float D, const float* temp, const int64_t* end_ind, int32_t B, int32_t N, int32_t T,
                  double* acc, float* w, void* stream);

/* d loss / d temp of a LEARNED matching temperature (hyperparameters.py:132 learn_matching_temp = True; adaptive.py:19-21 keeps
 * `temp` trainable, adaptive.py:51 divides the detached cost by it inside the autograd graph): the averaging criterion
 * (binding_loss.py:24-35)  coef * sum_{b,n,t} w[b][n][t] * pad[b][t] * (0.5 dsum exp(-2 ls) + D (ls + 0.5 log 2 pi))  differentiated
 * through w = normalize(soft_dtw(cost / temp)) in forward mode along the alignment lattice, float64 inside.
 *   acc: the [2*B][N][T] accumulators gcpx_soft_dtw left for the same dsum / temp / end_ind;
 *   tangent [2*B][N][T] and partial [B]: caller-owned float64 scratch;  dtemp[0] += the gradient. */
int gcpx_soft_dtw_dtemp(const float* dsum, float D, const float* temp, const int64_t* end_ind, const double* acc,
                        const float* pad_mask, const float* log_sigma, float coef, int32_t B, int32_t N, int32_t T,
                        double* tangent, double* partial, float* dtemp, void* stream);
/* The same with the lattice cost and the criterion's per-cell value taken from two matrices: the alignment runs over
 *   cost[b][n][t] = (cost_dsum / cost_D) / temp[0] (acc: what gcpx_soft_dtw left for cost_dsum / cost_D), the criterion is
 *   coef * sum w * pad * (0.5 loss_dsum exp(-2 ls) + loss_D (ls + 0.5 log 2 pi)).  Same float64 sweep and summation order:
 *   with loss_dsum == cost_dsum and loss_D == cost_D the result has the bits of gcpx_soft_dtw_dtemp.
 *   Call site: backward_plan.py, "bw.dtw_dtemp" with matching_type = 'dtw_latent' and learn_matching_temp (the matching costs
 *   latents, adaptive.py:45-47; LossAveragingCriterion.loss still weighs image distances, binding_loss.py:24). */
int gcpx_soft_dtw_dtemp_split(const float* cost_dsum, float cost_D, const float* loss_dsum, float loss_D, const float* temp,
                              const int64_t* end_ind, const double* acc, const float* pad_mask, const float* log_sigma, float coef,
                              int32_t B, int32_t N, int32_t T, double* tangent, double* partial, float* dtemp, void* stream);

/* Bookkeeping on the matching distribution w [B][N = 2^L - 1][T] (depth-first):
 *   frame2node [B][T]  depth-first position of argmax over nodes, first maximum in BREADTH-first order
 *                      (tree.bf.match_dist.argmax(1), frame_binding.py:30; all-zero column -> root)
 *   matched_idx [B][T] the same for t <= end_ind[b], -1 beyond (get_matched_pruned_seqs, base_gcp.py:358-366), or NULL
 *   best_t [B][N]      argmax over frames (adaptive.py:119); entropy [B][N] = -sum p log p; p_n [B][N] = clamp(sum p, 0, 1)
 *                      (tree_module.py:145-147) */
int gcpx_match_stats(const float* w, const int64_t* end_ind, int32_t B, int32_t L, int32_t T, int32_t* frame2node,
                     int32_t* matched_idx, int32_t* best_t, float* entropy, float* p_n, void* stream);

/* AdaptiveBinding.prune_sequence (adaptive.py:62-77): node p > 0 is dropped when sigmoid(dist[b][p-1]) > threshold.
 *   leave [B][N]; kept_idx [B][N] = depth-first positions of kept nodes then -1; count [B]; target [B][N-1] (or NULL) =
 *   best_t[p] == best_t[p-1], the BCE target of adaptive.py:118-122. */
int gcpx_distance_prune(const float* dist, float threshold, const int32_t* best_t, int32_t B, int32_t N, int32_t* leave,
                        int32_t* kept_idx, int32_t* count, int32_t* target, void* stream);

/* LossAveragingCriterion.loss (binding_loss.py:19-42) before pad_mask / batch mean:
 *   nll_bt[b][t] = sum_n w[b][n][t] * (0.5 * dsum[b][n][t] * exp(-log_sigma)^2 + D * (log_sigma + 0.5 log 2 pi)) */
int gcpx_averaging_nll(const float* dsum, const float* w, const float* log_sigma, float D, int32_t B, int32_t N, int32_t T,
                       float* nll_bt, void* stream);

/* LossAveragingCriterion.get_soft_estimates (binding_loss.py:44-58): out[b][t][:] = sum_n w[b][n][t] * x[b][n][:], rows of D floats */
int gcpx_soft_average(const float* w, const float* x, float* out, int32_t B, int32_t N, int32_t T, int64_t D, void* stream);

/* Evaluation alignment: basic_dtw + _traceback of gcp/evaluation/dtw_utils.py:77-95,201-218 (the C version is
 *   gcp/evaluation/cutils.pyx:22-29) as used by DTWEvalBinding.get_single_matches (gcp/evaluation/evaluation_matching.py:133-146).
 *   cost [B][N][T] float32 (mean squared distance estimate n vs target t); sequence b uses rows < n_len[b] and columns < t_len[b]
 *   (NULL = N / T).  acc [B][N][T] float64 accumulated cost; inds [B][T] = for every target frame the estimate with the smallest
 *   accumulated cost among the path cells of its column (-1 beyond t_len); path [B][2][N+T] = (rows | columns) from the END of
 *   the path to its start, path_len [B]; dist [B] = acc[n-1][t-1] / (n + t).
 *   Caller's contract: 1 <= n_len[b] <= N and 1 <= t_len[b] <= T (not checked).  Cells of acc outside n_len[b] x t_len[b] and
 *   entries of path beyond path_len[b] are not written. */
int gcpx_dtw_align(const float* cost, const int32_t* n_len, const int32_t* t_len, int32_t B, int32_t N, int32_t T, double* acc,
                   int32_t* inds, int32_t* path, int32_t* path_len, double* dist, void* stream);

/* ---- backward of the adaptive path (training step of config c5) ---- */
/* d images of LossAveragingCriterion.loss (binding_loss.py:19-42), the matching weights being constants (adaptive.py:50 detaches):
 *   dimg[b][n][:] = coef * exp(-2 log_sigma) * (images[b][n][:] * sum_t wp - sum_t wp[b][n][t] * traj[b][t][:]),  wp = w * pad_mask;
 *   dlog_sigma[0] += coef * sum w * pad * (D - dsum * exp(-2 log_sigma)).  coef = d total / d (per-sequence loss value). */
int gcpx_averaging_nll_bwd(const float* w, const float* pad_mask, const float* images, const float* traj, const float* dsum,
                           const float* log_sigma, float coef, int32_t B, int32_t N, int32_t T, int64_t D, float* dimg,
                           float* dlog_sigma, void* stream);
/* backward of the mixture mean (`images` of the discrete-logistic-mixture head): params / dparams [rows][npix][pitch] in the head's
 *   slot order, dimg NCHW [rows][3][npix]; colsum [rows][pitch] (per-frame column sums for the bias gradient) or NULL.
 *   used_slots = pitch: every slot of dparams is written (zeros where the mean does not depend on the parameter: the log-scales);
 *   used_slots = 8 * n_mix: only slots 0 .. 8 n_mix - 1 are read and written (the green / blue log-scales and the padding behind them
 *   carry no gradient) — for a head backward that walks the leading 8 n_mix channels only (gcpx_conv3x3 with Cin < src[0].C,
 *   gcpx_wgrad_conv3x3_split_src with Cout = 8 n_mix); slots >= used_slots of dparams are left untouched, of colsum written as 0 */
int gcpx_dlm_mean_bwd(const float* params, const float* dimg, float* dparams, float* colsum, int32_t rows, int32_t npix, int32_t pitch,
                      int32_t n_mix, int32_t used_slots, void* stream);
/* backward of gcpx_attention (one head): from d_out [M][nz] and the saved weights att [M][T]:
 *   dS [M][T] (scratch, gradient w.r.t. the scaled scores), dq [M][dk], dtemp_row [M] (per-row terms of d temperature),
 *   dK [B][T] rows of dk floats with leading dimension ldk, dV [B][T] rows of nz floats with leading dimension ldv
 *   (gradients of the projected keys / values summed over the rows of a sequence). */
int gcpx_attention_bwd(const float* q, const float* k, const float* v, const float* att, const float* d_out, const int64_t* end_ind,
                       const float* temperature, float* dS, float* dq, float* dtemp_row, float* dK, int64_t ldk, float* dV, int64_t ldv,
                       int32_t M, int32_t rpb, int32_t T, int32_t dk, int32_t nz, void* stream);
/* backward of gcpx_attention with `heads` heads (blox MultiheadAttention as called at adaptive_binding/attentive_inference.py:81;
 *   hyperparameters.py:24 n_attention_heads).  The forward keeps only the head-averaged weights, which carry no gradient (they are
 *   logged) and are the softmax of no head: the probabilities of head h are computed again from q, k, end_ind and the temperature, by
 *   the forward's own arithmetic.  With dh = dk / heads, vh = nz / heads, per head h:
 *     a = softmax over [0, end_ind[b]] of q_h . k_h[t] / sqrt(dh) / temp,  dA[t] = dO_h . V_h[t],  dS = a * (dA - sum_t a dA),
 *     dq_h = sum_t dS[t] k_h[t] / (sqrt(dh) temp),  dK_h[b][t] = sum_j dS[(b, j)][t] q_h[(b, j)] / (sqrt(dh) temp),
 *     dV_h[b][t] = sum_j a[(b, j)][t] dO_h[(b, j)],  dtemp_row[r] = - sum_h sum_t dS[t] score[t] / temp.
 *   Arguments as gcpx_attention_bwd, except: no att; stats [M][heads][2] scratch (maximum and sum of each softmax, written by the
 *   row launch for the key / value launch); dS [M][heads][T] scratch.  Every element of dq, dtemp_row and of the [B][T] rows of
 *   dK / dV is written (zeros past end_ind).  Sums run in a fixed order, no atomics; with heads = 1 the results have the bits of
 *   gcpx_attention_bwd.  T <= 4096; head widths multiples of 4, dh / 4 and vh / 4 divisors of 256; rpb * heads <= 8192. */
int gcpx_attention_bwd_heads(const float* q, const float* k, const float* v, const float* d_out, const int64_t* end_ind,
                             const float* temperature, float* stats, float* dS, float* dq, float* dtemp_row, float* dK, int64_t ldk,
                             float* dV, int64_t ldv, int32_t M, int32_t rpb, int32_t T, int32_t dk, int32_t nz, int32_t heads,
                             void* stream);
/* Row layer-norm without affine between the attention layers (F.layer_norm(x, x.shape[1:]) at attentive_inference.py:82-83;
 *   hyperparameters.py:25 n_attention_layers): y[r] = (s - mean(s)) / sqrt(var(s) + eps), s = x[r] (+ add[r] if add is not NULL),
 *   biased variance; x, add, y dense [M][W], W a multiple of 4 up to 1024; rstd [M] = 1 / sqrt(var + eps) for the backward, or NULL. */
int gcpx_row_layernorm(const float* x, const float* add, float* y, float* rstd, int32_t M, int32_t W, float eps, void* stream);
/* its backward from the saved y and rstd: dx[r] = rstd[r] * (dy[r] - mean(dy[r]) - y[r] * mean(dy[r] * y[r])); with an addend the
 *   same dx is the gradient of both summands */
int gcpx_row_layernorm_bwd(const float* dy, const float* y, const float* rstd, float* dx, int32_t M, int32_t W, void* stream);
/* Sum of `nblocks` column blocks lying side by side: dst[r][c] = ((src[r][c] + src[r][width + c]) + src[r][2 width + c]) + ...,
 *   r < rows, c < width; src rows have leading dimension ld >= nblocks * width, dst rows ldd >= width.  float32, one thread per
 *   element adds the blocks left to right (no atomics: the order is fixed).  dst may be block 0 of src; nothing else is written.
 *   Call site: backward_plan.py, "bw.attn.ksum" / "bw.attn.vsum" — tied tree levels (untied_layers = False) share the projected
 *   keys / values of an attention layer, whose gradient is the sum over the levels of what gcpx_attention_bwd(_heads) wrote for
 *   each level into a block of its own, the blocks laid out in the order the backward walks the levels (level L - 1 first). */
int gcpx_add_col_blocks(const float* src, int64_t ld, int32_t nblocks, float* dst, int64_t ldd, int64_t rows, int32_t width,
                        void* stream);

/* ---- collectives of the data-parallel paths: RCCL over xGMI, one communicator per process (one process
 *   per GPU), enqueued on the caller's stream, no synchronisation.  Replaces nn.DataParallel's gradient reduce
 *   (/root/reference/gcp/prediction/training/gcp_builder.py:71-78) and the per-GPU split of planning work (gcp/planning/run.py:108-120:
 *   here the costs of one sharded CEM population are gathered).  The Python host reaches the same RCCL through torch.distributed
 *   (video-gcp_amd/dist.py); these entry points serve a binder without torch.  RCCL is resolved at run time (GCPX_ERR_COMM when absent). */
#define GCPX_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (GCPX_COMM_ID_BYTES bytes) to hand to every rank by any host channel */
int gcpx_comm_unique_id(void* id_out);
/* every rank (its GPU current): *comm = communicator of `world` ranks */
int gcpx_comm_init(void** comm, int32_t rank, int32_t world, const void* id);
/* in-place sum of buf[0..n) over the ranks (the flat fp32 gradient or one of its buckets; 1 / world is folded into gcpx_optim_step) */
int gcpx_comm_allreduce(void* comm, float* buf, int64_t n, void* stream);
/* recv[r * n .. (r + 1) * n) = rank r's send[0..n)  (the candidates' costs of a sharded CEM population) */
int gcpx_comm_allgather(void* comm, const float* send, float* recv, int64_t n, void* stream);
int gcpx_comm_destroy(void* comm);

/* ---- host-fed data path (video-gcp_amd/dataset.py): assembly of one uploaded batch into the model's f32 inputs, in place.
 *   frames  uint8 [B][T][H][W][3]: per sequence the window raw[offset : offset + T] of its recorded frames (first n_frames valid);
 *   info    int32 [B][8]: n_frames, n_states, n_actions, chop, zero_from, end_ind, 0, 0 (the host's draws, data_loader.py:131-211);
 *   lut     f32 [256]: the reference's uint8 -> [-1, 1] conversion (data_loader.py:222) as a table; pad_in f32 [B][T];
 *   states_in f32 [B][T][state_dim], actions_in f32 [B][T-1][n_actions]: windows like the frames (null when the size is 0);
 *   states_mean / states_den f32 [state_dim] (both null: no standardisation): states = (s - mean) / den, den = 1e-6 + std.
 *   Output frame t reads window frame s = min(t + chop, T - 1) when t < zero_from and s < n_frames, else uint8 0 (-> lut[0] = -1).
 *   Writes traj_seq [B][T][3][H][W], I_0 / I_g [B][3][H][W] (frames 0 / end_ind), pad_mask [B][T], end_ind / start_ind int64 [B],
 *   states [B][T][state_dim], actions [B][T-1][n_actions].  H * W % 4 == 0 needs 16-byte aligned frames and images. */
int gcpx_assemble_batch(const uint8_t* frames, const int32_t* info, const float* lut, const float* pad_in, const float* states_in,
                        const float* actions_in, const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t H,
                        int32_t W, int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask,
                        int64_t* end_ind, int64_t* start_ind, float* states, float* actions, void* stream);

/* The same assembly for frames stored at Hs x Ws != H x W: between the time map and the conversion every frame is resized as the
 *   reference's preprocess_images does (data_loader.py:213-220, resize_video(images, (img_sz, img_sz)); taken to be Pillow's 8-bit
 *   bilinear Image.resize, see video-gcp_amd/dataset.py): a horizontal, then a vertical pass, each rounding to uint8,
 *       out[xx] = clip((2^21 + sum_{x < bx[xx][1]} in[bx[xx][0] + x] * kx[xx][x]) >> 22, 0, 255)   (int32; likewise ky / by down a column),
 *   over tables the host computes once per size pair in float64 (dataset.resize_coeffs) -- integer arithmetic only on the device.
 *   frames  uint8 [B][T][Hs][Ws][3];  kx int32 [W][ksx], bx int32 [W][2] (first source column, tap count), ky int32 [H][ksy],
 *   by int32 [H][2];  ksx = 2 * ceil(max(Ws / W, 1)) + 1, ksy likewise.  A pass whose lengths agree gets its (identity) table like any other.
 *   A frame that is not valid under the time map is lut[0] without a read, as in gcpx_assemble_batch; every other argument and every
 *   output is that function's, the images at H x W.
 *   Limits (GCPX_ERR_INVALID_ARG otherwise): all four sides in [1, 512], W % 4 == 0, Hs <= 8 H and Ws <= 8 W, ksx / ksy as above,
 *   frames and images 16-byte aligned. */
int gcpx_resize_assemble_batch(const uint8_t* frames, const int32_t* info, const float* lut, const int32_t* kx, const int32_t* bx,
                               const int32_t* ky, const int32_t* by, const float* pad_in, const float* states_in, const float* actions_in,
                               const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t Hs, int32_t Ws, int32_t H,
                               int32_t W, int32_t ksx, int32_t ksy, int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0,
                               float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states, float* actions,
                               void* stream);

/* The same two assemblies over a split whose frames stay on the device (video-gcp_amd/dataset_resident.py: ResidentStore holds them,
 *   ResidentLoader._launch calls these where HostFedLoader._launch calls gcpx_assemble_batch / gcpx_resize_assemble_batch on a
 *   freshly uploaded slot).  No frame, state or action bytes are uploaded per batch: a sequence is a window of the store.
 *   store   uint8, store_bytes of them: every trajectory's frames [n_i][H][W][3] ([n_i][Hs][Ws][3] in the resize form) back to back,
 *           no padding between trajectories; 16-byte aligned (the plain form with H * W % 4 != 0 takes any alignment);
 *   states_store f32 [sum n_i][state_dim], actions_store f32 [sum (n_i - 1)][n_actions] (null when the size is 0);
 *   info    int64 [B][8], 8-byte aligned, per sequence:
 *             [0] index in the store (in frames) of the window's first frame, [1] n_frames the trajectory has from there on,
 *             [2] first state row, [3] n_states from there on, [4] first action row, [5] n_actions from there on,
 *             [6] chop, [7] zero_from | end_ind << 32 (both non-negative and below 2^31);
 *   lut, pad_in, states_mean / states_den, the tables and every output: as in gcpx_assemble_batch / gcpx_resize_assemble_batch.
 *   Output frame t reads frame [0] + s of the store, s = min(t + chop, T - 1), when t < zero_from and s < min(n_frames, T), else it
 *   is lut[0] and nothing is read: the frames behind a short trajectory are another trajectory's and never stand in for padding.
 *   States and actions read rows [2] + s and [4] + s under the same map (actions: T - 1 steps, s clamped to T - 2).  All addressing
 *   into the store is 64-bit.  No byte outside [store, store + store_bytes) is read whatever info holds: a window that starts below
 *   the store or reaches past its last whole frame is padding, and the 16-byte staging loads of the resize form stop at store_bytes.
 *   The row bases of states and actions are the caller's to keep inside their arrays (a negative base reads nothing).
 *   Limits (GCPX_ERR_INVALID_ARG otherwise, nothing launched): no null store / info / lut / pad_in / output, store_bytes at least one
 *   frame, sides in [1, 512]; the resize form has the limits of gcpx_resize_assemble_batch (W % 4 == 0, Hs <= 8 H, Ws <= 8 W, ksx / ksy
 *   the tap counts of the sizes, no null table). */
int gcpx_assemble_batch_resident(const uint8_t* store, int64_t store_bytes, const int64_t* info, const float* lut, const float* pad_in,
                                 const float* states_store, const float* actions_store, const float* states_mean, const float* states_den,
                                 int32_t B, int32_t T, int32_t H, int32_t W, int32_t state_dim, int32_t n_actions, float* traj_seq,
                                 float* I_0, float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states,
                                 float* actions, void* stream);
int gcpx_resize_assemble_batch_resident(const uint8_t* store, int64_t store_bytes, const int64_t* info, const float* lut, const int32_t* kx,
                                        const int32_t* bx, const int32_t* ky, const int32_t* by, const float* pad_in,
                                        const float* states_store, const float* actions_store, const float* states_mean,
                                        const float* states_den, int32_t B, int32_t T, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                                        int32_t ksx, int32_t ksy, int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0,
                                        float* I_g, float* pad_mask, int64_t* end_ind, int64_t* start_ind, float* states, float* actions,
                                        void* stream);

/* The assembly for the nav datasets, whose frames are not recorded images but top-down pictures of the maze drawn from the states
 *   (MazeTopRenderedGlobalSplitVarLenVideoDataset.process_data_dict, /root/reference/gcp/datasets/data_loader.py:299-319, calling
 *   Multiroom3dEnv.render_pos_top_down, gcp/planning/infra/envs/miniworld_env/multiroom3d/multiroom3d_env.py:185-219).  Called by
 *   video-gcp_amd/dataset.py: topdown_assemble_into (HostFedLoader._launch).
 *   background  uint8 [side][side][3]: the static picture padded by cw zeros on every side, after the reference's * 255 truncation;
 *   agent_stamp / goal_stamp  uint8 [k][k] (non-zero: painted), k odd, entry [k / 2][k / 2] on the point; agent_rgb / goal_rgb: the dot
 *   colours as r | g << 8 | b << 16;  coords int32 [B][T][2]: (x, y) of the agent in the padded picture for the frames of the window
 *   states[offset : offset + T] (first n_frames = info[b][0] valid), goal int32 [B][2]: (x, y) of the goal (dataset.topdown_pixels).
 *   Output frame t reads window frame s = min(t + chop, T - 1) when t <= end_ind, t < zero_from and s < n_frames (else lut[0], nothing
 *   read: the reference renders frames up to end_ind and leaves zeros behind them, whatever zero_from says for states and actions):
 *       the 2cw x 2cw block of the picture whose first pixel is (max(cw, x) - cw, max(cw, y) - cw), rows by y and columns by x,
 *       with the agent stamp's colour written around (x, y), then the goal stamp's around the goal (the goal wins), both clipped to the
 *       block (which lies inside the picture: the caller checks max(cw, x) + cw <= side, likewise y; the device clamps the block into the
 *       picture, so a caller that does not check gets a wrong picture, never a wild read),
 *   then resized 2cw -> H x W with the two integer passes of gcpx_resize_assemble_batch over its tables for (Hs, Ws) = (2cw, 2cw), and
 *   converted through lut.  info, lut, the tables, the auxiliary windows and every output are that function's.
 *   Limits (GCPX_ERR_INVALID_ARG otherwise, nothing launched): no null table, background, stamp or coordinate pointer, 2cw in [4, 128],
 *   side in [2cw, 16384], k odd and <= 31, H and W in [1, 512], W % 4 == 0, 2cw <= 8 H and 8 W, ksx / ksy the tap counts of the sizes,
 *   background 4-byte and images 16-byte aligned. */
int gcpx_topdown_assemble_batch(const uint8_t* background, int32_t side, int32_t cw, const uint8_t* agent_stamp, const uint8_t* goal_stamp,
                                int32_t k, int32_t agent_rgb, int32_t goal_rgb, const int32_t* coords, const int32_t* goal,
                                const int32_t* info, const float* lut, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                                const int32_t* by, const float* pad_in, const float* states_in, const float* actions_in,
                                const float* states_mean, const float* states_den, int32_t B, int32_t T, int32_t H, int32_t W, int32_t ksx,
                                int32_t ksy, int32_t state_dim, int32_t n_actions, float* traj_seq, float* I_0, float* I_g, float* pad_mask,
                                int64_t* end_ind, int64_t* start_ind, float* states, float* actions, void* stream);

/* ---- picture logs (video-gcp_amd/image_log.py): a whole panel composed by one launch out of f32 tensors on the device.
 *   Replaces the host loops of the reference's logger: HierarchyLogger.log_hierarchy_image (logger.py:114-182), log_loss_gif
 *   (logger.py:236-253), log_dense_gif / log_rows_gif + make_gif (logger.py:214-234, visualization.py:485-497), plot_balanced_tree
 *   (visualization.py:232-262), plot_val_tree (:327-362), plot_gt_matching_overview (:365-400) and plot_greyscale_dist (:51-55).
 *   The canvas is [n][H_c][W_c][3] (channel-last), first filled with `background`; then the tiles are applied IN TABLE ORDER (a later
 *   tile overwrites an earlier one on the pixels they share: the reference's sequential assignment), then, if post_rescale, every
 *   element becomes (x + 1) / 2 (logger.py:180).  A tile descriptor emits, for sample b < nb and frame f < nf, one h x w rectangle at
 *       canvas index n0 + b n_b + f n_f,  row r0 + b r_b + f r_f,  column c0 + b c_b + f c_f  (+ index[b] * w, see below)
 *   clipped to the canvas.  Kinds:
 *     GCPX_PANEL_IMAGE     pixel (yy, xx) of channel ch = src[off + b s_b + f s_f + ch s_c + yy s_y + xx]  (channel-first f32 frames)
 *     GCPX_PANEL_GREY      all three channels = src[off + b s_b + f s_f + (xx / tile_w) s_c]: nearest-tile expansion of a row of values
 *     GCPX_PANEL_GREY_ADD  the same value ADDED to what the canvas holds (f32, table order): the gamma strips of logger.py:132-148
 *     GCPX_PANEL_FILL      the constant `fill`
 *   src / index / length are slots of the `srcs` array (-1: none); src_elems[slot] is the element count of that array and every read
 *   is checked against it (an out-of-range read leaves the pixel as it was).
 *   index  (int32, or int64 with GCPX_PANEL_INDEX_I64): v = index[index_off + b index_stride]; the rectangle of sample b is skipped
 *          unless 0 <= v < index_count; v * w is added to the column (a node's matched time step, logger.py:145-154), or, with
 *          GCPX_PANEL_INDEX_FRAME, v replaces f in the SOURCE address (batchwise_index, visualization.py:359).
 *   length (int32, or int64 with GCPX_PANEL_LENGTH_I64; IMAGE / GREY): frames f > length[b] are multiplied by 0 (mask_extra,
 *          logger.py:160-161, get_pad_mask utils.py:30-50); with GCPX_PANEL_LENGTH_STRICT frames f >= length[b] (pad_sequence's zeros).
 *   GCPX_PANEL_RESCALE (IMAGE / GREY): (x + 1) / 2 (imgtensor2np, visualization.py:113), after the mask.
 *   Outputs (either may be null, not both): canvas_f32, and canvas_u8 = trunc(clip(x, 0, 1) * 255), this build's own conversion.
 *   The pointers of `srcs` travel as kernel arguments, so a cached device table serves every logging step; the host arrays are read
 *   before the call returns.  Nothing is allocated, nothing synchronises. */
#define GCPX_PANEL_MAX_SRCS 16
#define GCPX_PANEL_IMAGE 0
#define GCPX_PANEL_GREY 1
#define GCPX_PANEL_GREY_ADD 2
#define GCPX_PANEL_FILL 3
#define GCPX_PANEL_RESCALE 1
#define GCPX_PANEL_LENGTH_STRICT 2
#define GCPX_PANEL_INDEX_FRAME 4
#define GCPX_PANEL_INDEX_I64 8
#define GCPX_PANEL_LENGTH_I64 16
typedef struct gcpx_panel_tile {
    int32_t kind, src, index, length, flags;
    int32_t nb, nf;                    /* samples, frames */
    int32_t h, w, tile_w;              /* rectangle in pixels; GREY kinds: pixels per value */
    int32_t n0, n_b, n_f;              /* canvas index of (b, f) */
    int32_t r0, r_b, r_f;              /* top row */
    int32_t c0, c_b, c_f;              /* left column */
    int32_t index_off, index_stride, index_count;
    float fill;
    int32_t _pad;
    int64_t off, s_b, s_f, s_c, s_y;   /* source offset and strides in elements */
} gcpx_panel_tile;
int gcpx_panel_compose(const gcpx_panel_tile* tiles, int32_t n_tiles, const void* const* srcs, const int64_t* src_elems, int32_t n_srcs,
                       int32_t n, int32_t H_c, int32_t W_c, float background, int32_t post_rescale, float* canvas_f32,
                       uint8_t* canvas_u8, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * State trajectories on the top-down map (video-gcp_amd/image_log.py, visualization.render_trajectories_numpy; csrc/topdown_traj.hip):
 * Multiroom3dEnv.render_top_down (multiroom3d_env.py:151-183) for n canvases at once.
 *
 * gcpx_topdown_trajectories: out uint8 [n][S][S][3].  background: the padded picture uint8 [S + 2 cw][S + 2 cw][3] of
 *   topdown_assets.npz; the drawing surface is its unpadded middle [cw : cw + S]^2 (the reference renders these pictures from an
 *   environment without crop_window).  agent_stamp / goal_stamp: [k][k] bytes (non-zero = painted), k odd and at most 31;
 *   agent_rgb / goal_rgb: r | g << 8 | b << 16.  layers [n_layers]: a host array, read before the call returns.  Layer l of canvas i:
 *     points     m = min(len[i], P) (len = end_ind + 1, int32 or int64 as len_i64 says); m < 1 paints nothing.  Point p is
 *                states[i * s_n + p * s_p + {0, s_d}] (element strides).
 *     pixels     in float32, nothing contracted: y *= -1; if the maximum of the 2 m values is > 1 or their minimum < -1 (a NaN among
 *                them: neither, as numpy's max / min return it) every value is divided by 27 (correctly rounded); then
 *                + (float)(0.5 * table_size), table_size = (1 / 3) * int(sqrt(n_rooms)); fx = x * render_scale, fy = y * render_scale;
 *                px = int(fx), py = S - int(fy), truncated toward zero.  A point whose fx or fy is not finite is skipped: no segment
 *                ends in it, no stamp is centred on it.  px and py are clamped to [-GCPX_TRAJ_COORD_LIMIT, GCPX_TRAJ_COORD_LIMIT],
 *                which with S <= GCPX_TRAJ_MAX_SIDE keeps the test below inside int64 (the reference raises on such a point).
 *     segments   j = 0 .. m - 2, from point j to point j + 1, covers pixel q when q lies within GCPX_TRAJ_THICKNESS / 2 of it, decided
 *                in int64 on integer coordinates: d = b - a, w = q - a, t = w . d; t <= 0: 4 |w|^2 <= thickness^2; t >= |d|^2:
 *                4 |q - b|^2 <= thickness^2; else 4 (d x w)^2 <= thickness^2 |d|^2.
 *     colour     trunc(c * f * 255) per channel of color[3], clamped to [0, 255]; f = 0.5^hits, hits = [j in D] + [j + 1 in D], D = the
 *                set {min(dim_t[i][q], len[i] - 1), q < K} (nav_9rooms.py:46-49: `color_seq[t] *= 0.5`, `color_seq[t - 1] *= 0.5`, each
 *                once per distinct t; t = 0 dims the unused last entry through the index -1).  dim_t NULL: f = 1.  Negative values of
 *                dim_t are ignored.
 *     order      the background; then per layer the segments in order, the agent stamp centred on point 0, the goal stamp centred on
 *                point m - 1 (clipped at the picture's border).  A later write wins.  Every pixel belongs to one thread for the whole
 *                launch; GCPX_TRAJ_LAYERS_PER_LAUNCH layers go into one launch, more layers into further launches on the same stream.
 *   Limits (GCPX_ERR_INVALID_ARG): S <= GCPX_TRAJ_MAX_SIDE, 1 <= P <= GCPX_TRAJ_MAX_POINTS, n_layers <= GCPX_TRAJ_MAX_LAYERS,
 *   K <= GCPX_TRAJ_MAX_DIM, k odd and <= 31, state_dim == 2.  Nothing is allocated, nothing synchronises.
 *
 * gcpx_topdown_bottlenecks: out int32 [n][K], out[i][j] = the first maximum over t of match_dist_df[i][df(j)][:] for the breadth-first
 *   nodes j < K of the depth-first tensor [B][N = 2^levels - 1][T] (`tree.bf.match_dist.argmax(2)[:, :7]`, nav_9rooms.py:42); a NaN
 *   counts as the maximum, as in numpy.argmax.  One launch. */
#define GCPX_TRAJ_MAX_SIDE 2048
#define GCPX_TRAJ_MAX_POINTS 1024
#define GCPX_TRAJ_MAX_LAYERS 64
#define GCPX_TRAJ_LAYERS_PER_LAUNCH 8
#define GCPX_TRAJ_MAX_DIM 16
#define GCPX_TRAJ_THICKNESS 4
#define GCPX_TRAJ_COORD_LIMIT 16384
typedef struct gcpx_traj_layer {
    const float* states;
    int64_t s_n, s_p, s_d;             /* element strides of [n][P][2] */
    const void* len;                   /* [n] */
    const int32_t* dim_t;              /* [n][K] or NULL */
    float color[3];
    int32_t len_i64;                   /* len is int64 (else int32) */
    int32_t K;
    int32_t P;                         /* points per trajectory of `states` */
} gcpx_traj_layer;
int gcpx_topdown_trajectories(const uint8_t* background, int32_t S, int32_t cw, const uint8_t* agent_stamp, const uint8_t* goal_stamp,
                              int32_t k, int32_t agent_rgb, int32_t goal_rgb, const gcpx_traj_layer* layers, int32_t n_layers, int32_t n,
                              int32_t state_dim, int32_t n_rooms, int32_t render_scale, uint8_t* out, void* stream);
int gcpx_topdown_bottlenecks(const float* match_dist_df, int32_t B, int32_t N, int32_t T, int32_t levels, int32_t n, int32_t K,
                             int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Scalar logs (video-gcp_amd/scalar_log.py; csrc/train_stats.hip).
 *
 * gcpx_grad_segment_norms: log_gradients (base_model.py:139-146): `torch.norm(p.grad)` of every parameter with a gradient, their mean
 *   and maximum.  grad: the trainer's flat f32 gradient of n elements, laid out like theta (segments on 16-byte boundaries, any
 *   length).  chunks [n_chunks]: every counted segment cut into pieces of at most GCPX_GRAD_NORM_CHUNK elements, the pieces of one
 *   segment adjacent; seg_chunk0 [n_seg + 1]: the first chunk of every segment (a prefix sum; seg_chunk0[n_seg] = n_chunks).  Both
 *   tables live on the device and are built once per model (scalar_log.grad_tables).  Only the elements the chunks name are read, and
 *   a chunk outside [0, n) or longer than GCPX_GRAD_NORM_CHUNK is skipped.
 *   seg_norm[s] = |grad_scale| * coef * || segment s ||_2, with grad_scale as gcpx_grad_clip_coef takes it (1 / world when the buffer
 *   holds the ranks' sum) and coef = *clip_coef (NULL or a value of 0: 1; a negative value: 0) -- the clipping coefficient the step kernels apply to the
 *   gradient they read, where the reference's clip_grad_norm_ has scaled p.grad itself before it is logged.
 *   A segment whose elements are all exactly zero is NOT counted (this build's `p.grad is None`: a parameter off the graph gets no
 *   gradient write and keeps the zeros of the step's clear).  stats[0..3] = mean of the counted norms, their maximum (a NaN stays, as in
 *   torch.max), the number counted, the number of counted norms that are not finite; mean and maximum are 0 when nothing is counted.
 *   partial: caller's scratch of n_partial >= 2 * n_chunks floats.  Two launches on `stream`; nothing is allocated, nothing
 *   synchronises.  Deterministic and bit-repeatable: a thread of the 256 of a chunk's workgroup adds at most GCPX_GRAD_NORM_SERIAL
 *   squares into one f32 accumulator, a fixed tree of depth GCPX_GRAD_NORM_TREE_DEPTH adds the accumulators, and the chunks of a segment
 *   are added in table order in f64; the root and the scale are applied in f64 and rounded to f32 once.  So the relative error of a
 *   norm is at most (GCPX_GRAD_NORM_SERIAL + GCPX_GRAD_NORM_TREE_DEPTH + 2) / 2 * 2^-24 (as long as no square leaves the f32 range:
 *   elements below 1e-19 or above 1e19 in magnitude underflow / overflow, as they do in torch.norm of an f32 tensor).
 *
 * gcpx_kl_layerwise: the layer-wise KL of TreeModule._log_outputs (tree_module.py:159-169).  q_z / p_z rows [mu | log_sigma] at
 *   base + b * batch_stride + n * node_stride for the N = 2^L - 1 nodes in depth-first order, as gcpx_kl_gauss reads them.
 *   node_v[b * N + n] = mean over the nz latent dimensions of max(KL_elem, free_nats), KL_elem being the element gcpx_kl_gauss sums;
 *   out[l] = mean of node_v over (b, the 2^l nodes of level l) counting only entries != 0, NaN when none remain (`l[l != 0].mean()`).
 *   The level of depth-first position p is L - 1 - ctz(p + 1).  Two launches on `stream`, fixed summation order. */
#define GCPX_GRAD_NORM_THREADS 256
#define GCPX_GRAD_NORM_CHUNK 16384
#define GCPX_GRAD_NORM_SERIAL (GCPX_GRAD_NORM_CHUNK / GCPX_GRAD_NORM_THREADS + 1)
#define GCPX_GRAD_NORM_TREE_DEPTH 8
typedef struct gcpx_grad_chunk {
    int64_t first;                     /* first element of the chunk in the flat vector */
    int32_t seg;                       /* the segment it belongs to */
    int32_t length;                    /* 1 .. GCPX_GRAD_NORM_CHUNK */
} gcpx_grad_chunk;
int gcpx_grad_segment_norms(const float* grad, int64_t n, const gcpx_grad_chunk* chunks, int32_t n_chunks, const int32_t* seg_chunk0,
                            int32_t n_seg, float grad_scale, const float* clip_coef, float* partial, int64_t n_partial, float* seg_norm,
                            float* stats, void* stream);
int gcpx_kl_layerwise(const float* qz, const float* pz, int32_t B, int32_t L, int32_t nz, int64_t batch_stride, int64_t node_stride,
                      float free_nats, float* node_v, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Training guard (video-gcp_amd/health.py; csrc/train_stats.hip).
 *
 * gcpx_grad_health: NanGradHook (base_trainer.py:20-66: every parameter's gradient is tested between backward() and optimizer.step(),
 *   the bad ones are named and training stops before the weights are touched) and the NaN total loss of base_gcp.py:302-303, on the
 *   device.  x: a flat f32 vector of n < 2^31 elements, walked through the tables of gcpx_grad_segment_norms (chunks, seg_chunk0: only
 *   the elements the chunks name are read; a chunk outside [0, n) or longer than GCPX_GRAD_NORM_CHUNK is skipped).  extra: n_extra
 *   device scalars tested beside it (the loss terms and their total), or NULL / 0.
 *   An element is classified by its bits: exponent all ones and mantissa != 0 -> NaN (either sign, any payload), exponent all ones and
 *   mantissa 0 -> +Inf or -Inf by the sign; everything else, denormals, -0 and +-FLT_MAX included, is finite.
 *   seg_bad [n_seg][3] = NaN, +Inf, -Inf elements of every segment.  summary [8]: [0..2] their totals, [3] number of segments with a
 *   count > 0, [4] the first such segment or -1, [5] number of extra scalars that are NaN or +-Inf, [6] the verdict: 1 when [3] or [5]
 *   is > 0, else 0, [7] a running count: incremented by the verdict on every call (the caller zeroes it once).
 *   gate: NULL, or a float that receives verdict ? 1 : 0 on EVERY call (a clean call re-opens it): slot 3 of the optimizer state.
 *   partial: caller's scratch of n_partial >= 3 * n_chunks int32.  Two launches on `stream`, no atomic, nothing allocated, nothing
 *   synchronises; integer sums, so the result does not depend on the schedule. */
int gcpx_grad_health(const float* x, int64_t n, const gcpx_grad_chunk* chunks, int32_t n_chunks, const int32_t* seg_chunk0, int32_t n_seg,
                     const float* extra, int32_t n_extra, int32_t* partial, int64_t n_partial, int32_t* seg_bad, int32_t* summary,
                     float* gate, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Nav data generator: the PRM expert of the reference's data collection (video-gcp_amd/nav_gen.py; csrc/prm.hip).  One workgroup per
 * trajectory, a batch of B independent trajectories per call.  All geometry is float64, nothing contracted.  Ragged inputs: the points
 * of trajectory b are px / py [pt_off[b] .. pt_off[b + 1]) of total_pts, at most max_pts of them; per-trajectory outputs have a fixed
 * capacity of `cap` nodes, max_pts + 2 <= cap <= GCPX_PRM_MAX_NODES.  start_goal [B][4] = (sx, sy, gx, gy).  Every launch is on
 * `stream`; nothing is allocated, nothing synchronises.  The numpy restatements nav_gen.sample_points_numpy, prm_numpy and
 * spline_numpy are the definitions.
 *
 * gcpx_prm_sample_points: the sample points of PrmPolicy._sample_points (prm_policy.py:99-124) from RoomSampler2d's boxes
 *   (sampling_fcns.py:27-45): point p of trajectory b lies in box pt_box[p] of boxes [n_boxes][4] = (centre x, centre y, width x,
 *   width y):  (u - 0.5) * width + centre, u in [0, 1) = 53 bits of mix64(mix64(mix64(seed) ^ traj_key[b]) ^ c), mix64 the splitmix64
 *   output function, c = 2 * draw for x and 2 * draw + 1 for y, draw = draw0[b] + (p - pt_off[b]).  A trajectory's points depend on
 *   (seed, its key, its draws) alone, not on the batch.  The generator is this build's own: np.random is not mirrored.  A box index
 *   outside [0, n_boxes) gives NaN.
 *
 * gcpx_prm_roadmap: sample_points with `sampled_points` given (prm.py:229-257), then generate_roadmap / is_collision (:96-159).
 *   kept [total_pts]: 1 iff the sample's nearest obstacle point is at distance >= rr.  Nodes of b: its kept samples in order, then
 *   start, then goal; n_nodes[b] = their number n; node_xy [B][2][cap] (x row, y row; 0 past n).  adj [B][cap][n_knn]: row i = the
 *   first n_knn nodes j != i in ascending d = sqrt(dx^2 + dy^2) (ties: lower j) whose edge does not collide, -1 past the list and in
 *   rows >= n.  An edge collides if d >= max_edge_len, or if one of the rint(d / rr) points starting at node i and advanced by repeated
 *   addition of (rr cos yaw, rr sin yaw), yaw = atan2(dy, dx), or the point j itself, has an obstacle point at distance <= rr.
 *   The cloud enters as a uniform grid built once per layout (nav_gen.obstacle_grid): obs_x / obs_y [n_obs] sorted by cell
 *   (cell = cy * grid_x + cx, c. = floor((. - grid_.0) / cell)), cell_start [grid_x * grid_y + 1]; cell > rr, so the 3 x 3 cells around
 *   a query hold every point within rr and the decisions equal a brute-force scan's.
 *
 * gcpx_prm_shortest_path: dijkstra_planning (prm.py:162-226): the shortest directed path from node n - 2 to node n - 1 over adj under
 *   cost d ** cost_power, costs summed from the start.  Bounded Bellman-Ford sweeps (at most n, early exit when nothing changed); the
 *   predecessor of j is the lowest i with cost[i] + w(i, j) == cost[j].  success[b] = 1, n_vert[b], path [B][cap] (vertex indices
 *   start .. goal) and cost[b]; when the goal is unreachable (or n < 2) success[b] = 0 and the other outputs are NOT written.
 *
 * gcpx_prm_resample: PrmPolicy._plan's resampling (prm_policy.py:173-185) and the recorded episode.  plan [B][T][2] (float64, the
 *   planner's units): the cubic spline that interpolates the n_vert[b] path vertices over the normalised cumulative chord length with
 *   not-a-knot ends -- splprep(s=0) -- evaluated at linspace(0, 1, ns), ns = clamp(n_steps[b], 0, T); rows >= ns are 0.  ok[b] = 0
 *   (and a zero plan) when n_vert[b] is outside [4, GCPX_PRM_MAX_PATH], a vertex repeats (splprep raises), an index is out of range
 *   or ns < 2.  states / actions / pad_mask (all three or none; float32): states [B][T + 1][5] = (x, y, heading, goal x, goal y) in
 *   the environment's units 27 * (x, -y) (the inverse of multiroom3d_env.py:196-199) for the ns plan states and the state after the
 *   `done` step's zero action (prm_policy.py:82-90), heading = atan2 of the step taken from the state; actions [B][T][2] = the ns - 1
 *   state differences (transform_plan, multiroom3d_env.py:141-144), then zeros; pad_mask [B][T + 1] = get_pad_mask(ns, T)
 *   (hdf5_saver.py:39-53).  Rows past the episode, and everything of a trajectory with ok = 0, are 0. */
#define GCPX_PRM_MAX_NODES 2048
#define GCPX_PRM_MAX_KNN 32
#define GCPX_PRM_MAX_PATH 1024
#define GCPX_PRM_MAX_EDGE_STEPS 4096
int gcpx_prm_sample_points(const double* boxes, int32_t n_boxes, const int32_t* pt_box, const int32_t* pt_off, const int64_t* traj_key,
                           const int32_t* draw0, int32_t B, int32_t total_pts, int32_t max_pts, int64_t seed, double* px, double* py,
                           void* stream);
int gcpx_prm_roadmap(const double* obs_x, const double* obs_y, const int32_t* cell_start, int32_t n_obs, int32_t grid_x, int32_t grid_y,
                     double grid_x0, double grid_y0, double cell, const double* px, const double* py, const int32_t* pt_off,
                     const double* start_goal, int32_t B, int32_t total_pts, int32_t max_pts, int32_t cap, int32_t n_knn, double rr,
                     double max_edge_len, uint8_t* kept, int32_t* n_nodes, double* node_xy, int32_t* adj, void* stream);
int gcpx_prm_shortest_path(const double* node_xy, const int32_t* n_nodes, const int32_t* adj, int32_t B, int32_t cap, int32_t n_knn,
                           double cost_power, int32_t* success, int32_t* n_vert, int32_t* path, double* cost, void* stream);
int gcpx_prm_resample(const double* node_xy, const int32_t* n_nodes, const int32_t* path, const int32_t* n_vert, const int32_t* n_steps,
                      const double* start_goal, int32_t B, int32_t cap, int32_t T, double* plan, int32_t* ok, float* states,
                      float* actions, float* pad_mask, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The maze environment of the control experiments (video-gcp_amd/nav_env.py, control.py; csrc/nav_env.hip): E independent episodes
 * advanced together, one launch per step -- what GeneralAgent.rollout does one episode at a time on the host through
 * TopdownMultiroom3dEnv.step (gcp/planning/infra/agent/general_agent.py, .../multiroom3d/multiroom3d_env.py) and BaseMiniworldEnv.eval
 * (base_miniworld_env.py:29-40).  gym-miniworld is absent: the dynamics are this build's own, defined by the numpy
 * restatements nav_env.step_numpy and nav_env.goal_dist_numpy.  One thread per episode; float64 geometry, nothing contracted; every
 * launch is on `stream`, nothing is allocated, nothing synchronises.
 *
 * Units: state [E][3] = (x, y, heading) float32 in the environment's units, 27 * (x, -y) of the table coordinates the layout uses
 *   (the inverse of multiroom3d_env.py:196-199); a position in table coordinates is ((double)x / 27, -((double)y / 27)).
 * walls [n_walls][4] float64 = (x0, y0, x1, y1): nav_layout.wall_segments centred on (0, 0) as Layout centres its cloud.
 * goal_table [E][rooms_per_side^2][3] float64, built by the host at reset (nav_env.goal_table): row r of episode e serves a position in
 *   room r (Layout.coords2ridx): (first door centre x, y, length from that door over the remaining door centres of
 *   plan_room_seq(r, goal room) to the goal); the goal room's row is (goal x, goal y, -1); every row's third entry is NaN when a
 *   coordinate of the goal lies outside [-0.5, 0.5].
 *   goal distance of a position p = 10 when a coordinate of p lies outside [-0.5, 0.5] or the row's third entry is NaN; else
 *   |p - (row x, y)| + max(third entry, 0): PrmPolicy.compute_shortest_path (prm_policy.py:198-216).  The room coordinates
 *   floor((c + table_size / 2) / (1 / 3)) are clamped to [0, rooms_per_side - 1].
 * pix [E][2] int32: dataset.topdown_pixels of the position (float32: (x, -y) / 27 + half_table, times render_scale, truncated;
 *   (v_x + cw, S + cw - v_y)), what gcpx_topdown_assemble_batch takes as the agent's pixel.
 *
 * gcpx_nav_env_reset: full_traj [E][T + 1][3] row 0 = state, path_len [E] (float64) = 0, goal_dist [E][T + 1] (float64) entry 0, pix.
 *
 * gcpx_nav_env_step: step t of T.  action [E][2] float32.  Proposed position p' = p + a, one float32 add per coordinate.
 *   a == (0, 0): the move is free, nothing changes.  Otherwise the move is BLOCKED iff p' is not finite or the closed segment [p, p']
 *   (table coordinates) comes within `radius` of a wall: for some wall NOT (d2 > radius^2), d2 = 0 when the two segments cross properly
 *   (both orientation tests strictly of opposite sign), else the least of the four squared end-point-to-segment distances.  A blocked
 *   move is rejected whole: position and heading stay.  A free move: position p', heading (float)atan2(dy, dx) of the step
 *   (float64 differences of the float32 coordinates, environment units).
 *   Written: state; full_traj row t + 1; blocked [E][T] entry t (1 / 0); path_len[e] += the Euclidean length of the step taken (0 when
 *   blocked; environment units); goal_dist entry t + 1 and pix of the new position.
 *
 * GCPX_ERR_INVALID_ARG, nothing launched: a null pointer, E or T outside [1, 2^20], t outside [0, T), n_walls outside
 *   [1, GCPX_NAV_MAX_WALLS], rooms_per_side outside [1, GCPX_NAV_MAX_ROOMS_PER_SIDE], radius negative or not finite, table_size <= 0,
 *   S outside [1, 16384], cw outside [0, 16384]. */
#define GCPX_NAV_MAX_WALLS 1024
#define GCPX_NAV_MAX_ROOMS_PER_SIDE 16
int gcpx_nav_env_reset(const float* state, const double* goal_table, int32_t rooms_per_side, double table_size, int32_t E, int32_t T,
                       float half_table, float render_scale, int32_t S, int32_t cw, float* full_traj, double* path_len, double* goal_dist,
                       int32_t* pix, void* stream);
int gcpx_nav_env_step(float* state, const float* action, const double* walls, int32_t n_walls, double radius, const double* goal_table,
                      int32_t rooms_per_side, double table_size, int32_t E, int32_t T, int32_t t, float half_table, float render_scale,
                      int32_t S, int32_t cw, float* full_traj, double* path_len, double* goal_dist, uint8_t* blocked, int32_t* pix,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The hierarchical latent search for K planning tasks at once (video-gcp_amd/tree_latent_search.py:
 * BatchedDeviceTreeLatentOptimizer; csrc/tree_search.hip): the per-decision steps of
 * HierarchicalTreeLatentOptimizer (gcp/planning/tree_optimizer.py), each one launch over all tasks.  Which level is drawn, optimised
 * and how the population is laid out does not depend on the task, so K tasks share one walk; only these tables differ per task.
 *
 * lat [n_rows][T][nz] float32: the rollout's latents, rows k*n .. k*n+n-1 of task k, then one stand-in row [inf, 0, inf, 0 ...] for a
 *   rollout too short to split (tree_optimizer.py:142-147).  nz % 4 == 0.
 * views [K][G][3] int32 = (row, a, b): candidate g of task k is lat[row][a:b].
 * goal [K][2] int32 = (row, frame); row < 0: every candidate's own last frame b - 1 (the raw goal image, tree_optimizer.py:99-101).
 * Row and frame indices are clamped into `lat` before they are used.  Every launch is on `stream`; nothing is allocated or read back.
 *
 * gcpx_tree_subgoal_rows (tree_optimizer.py:92-105): the operands of both pair costs of every candidate, m = (b - a) / 2:
 *   opa, opb [2][K][G][nz]: opa[0] = lat[row][a], opb[0] = opa[1] = lat[row][a + m], opb[1] = the goal latent; mids [K][G] = m.
 * gcpx_tree_select (tree_optimizer.py:106-110, 81-82, 179): per task total[g] = c1[k][g] + c2[k][g] (one float32 add; c2 NULL: c1),
 *   numpy's argmin over the candidates with mask[k][g] != 0 (mask NULL: all): the first NaN when there is one, else the first minimum
 *   -> idx [K], cost [K]; no candidate: idx = -1, cost = +inf.  draw [K][G][zf] != NULL: best_z [K][zf] = the chosen row (zf % 4 == 0).
 * gcpx_tree_split_views (tree_optimizer.py:142-155): short [K][G] = (b - a < 3); such a candidate becomes (dummy_row, 0, 3); then
 *   c = (b - a) / 2, left = (row, a, a + c), right = (row, a + c, b), left_goal [K][2] = (row, a + c) of the task's candidate 0.
 * gcpx_tree_segment_windows (tree_optimizer.py:79-84, 175-180): seg [K*G][tmax][nz] = lat[row][a:b] zero padded, lens [K*G] =
 *   min(b - a, tmax), goal_rows [K*G][nz]: what gcpx_seq_pairs / gcpx_masked_row_sum take.
 * gcpx_tree_short_alternative (tree_optimizer.py:157-163): c = lc[k] + rc[k] (one float32 add); use_short[k] = sidx[k] >= 0 and
 *   (sc[k] < c or isnan(c)); cost[k] = use_short ? sc[k] : c.
 *
 * GCPX_ERR_INVALID_ARG, nothing launched: a null pointer (c2, mask, draw with best_z may be NULL), a size <= 0, K*G > 2^24,
 *   nz or zf not a multiple of 4, dummy_row < 0. */
int gcpx_tree_subgoal_rows(const float* lat, const int32_t* views, const int32_t* goal, float* opa, float* opb, int32_t* mids,
                           int32_t K, int32_t G, int32_t n_rows, int32_t T, int32_t nz, void* stream);
int gcpx_tree_select(const float* c1, const float* c2, const int32_t* mask, const float* draw, float* best_z, int32_t* idx, float* cost,
                     int32_t K, int32_t G, int32_t zf, void* stream);
int gcpx_tree_split_views(const int32_t* views, int32_t dummy_row, int32_t* left, int32_t* right, int32_t* left_goal, int32_t* short_,
                          int32_t K, int32_t G, void* stream);
int gcpx_tree_segment_windows(const float* lat, const int32_t* views, const int32_t* goal, float* seg, int32_t* lens, float* goal_rows,
                              int32_t K, int32_t G, int32_t n_rows, int32_t T, int32_t tmax, int32_t nz, void* stream);
int gcpx_tree_short_alternative(const float* lc, const float* rc, const float* sc, const int32_t* sidx, float* cost, int32_t* use_short,
                                int32_t K, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The flat CEM loop for K planning tasks at once (video-gcp_amd/planning.py: CEMPlanner.plan_batch; csrc/cem_batch.hip): the
 * per-iteration arithmetic of CEMPlanner.__call__ / _get_best_rollouts (gcp/planning/cem/cem_planner.py:55-135) and of
 * FlatCEMSampler.sample / fit (gcp/planning/cem/sampler.py:33-48), each one launch over all tasks.  K Gaussians mean, std [K][D] over
 * samples of D = n_steps * action_dim floats (no alignment asked of D), n candidates per task, float32 throughout.  Every float operation
 * below is rounded on its own (nothing is contracted to an FMA), in the order written, so the torch mirrors in planning.py
 * (cem_population_torch, cem_elites_torch, cem_refit_torch) give the same bits.  Every launch is on `stream`; nothing is allocated or
 * read back.
 *
 * gcpx_cem_population (sampler.py:40-42: np.random.normal(loc=mean, scale=std) = mean + std * eps, then np.clip):
 *   out[k][j][d] = clamp(mean[k][d] + std[k][d] * eps[k][j][d], -clip, clip), eps standard-normal numbers; a non-finite clip: no clamp.
 *   A NaN stays a NaN.  One pass over the population; out may be eps (in place).
 * gcpx_cem_elites (cem_planner.py:129-130: np.argsort(scores)[:n_elite], stable): per task the first n_elite entries of the stable
 *   ascending order of scores [K][n] -> idx int32 [K][n_elite], elite_scores [K][n_elite] = the scores at idx.  Ties go to the lower
 *   index, -0.0 == +0.0, -inf and +inf are ordered, every NaN comes after every number and NaNs among themselves by index.  One workgroup
 *   per task, the task's scores staged in LDS, each score ranked by counting: n <= GCPX_CEM_MAX_N.
 * gcpx_cem_refit (sampler.py:44-46: np.mean / np.std(axis=0) of the elites; cem_planner.py:81: best_samples[:1]): with e_j = idx[k][j],
 *   x_j = samples[k][e_j][d]:  mean[k][d] = (((x_0 + x_1) + x_2) + ...) / n_elite;  std[k][d] = sqrt(((q_0 + q_1) + ...) / n_elite),
 *   q_j = (x_j - mean) * (x_j - mean) (the population std, two passes);  best[k][d] = x_0.  One thread per (task, column).  Every idx is
 *   range-checked before it is used: a task with an index outside [0, n) gets NaN in all three outputs, no load is made through it.
 *
 * GCPX_ERR_INVALID_ARG, nothing launched: a null pointer, a size <= 0, n_elite > n, n > GCPX_CEM_MAX_N (elites, refit), or more
 *   than 2^30 workgroups (K n ceil(D / 1024) for the population, K ceil(D / 256) for the refit). */
#define GCPX_CEM_MAX_N 8192     /* candidates per task: 32 KB of LDS keys in gcpx_cem_elites */
int gcpx_cem_population(const float* mean, const float* std, const float* eps, float clip, float* out, int32_t K, int32_t n, int32_t D,
                        void* stream);
int gcpx_cem_elites(const float* scores, int32_t* idx, float* elite_scores, int32_t K, int32_t n, int32_t n_elite, void* stream);
int gcpx_cem_refit(const float* samples, const int32_t* idx, float* mean, float* std, float* best, int32_t K, int32_t n, int32_t n_elite,
                   int32_t D, void* stream);

/* Receding-horizon additions to the loop above (CEMPlanner(noise_rho, keep_elites, warm_std), plan_batch(warm=); the reference's CEM has
 * none of them; iCEM, Pinneri et al. 2020).  A sample is S steps of A values, D = S * A, a population [K][n][S][A].  The same rule: every
 * float operation rounded on its own, in the order written; mirrors cem_warm_start_torch, cem_population_ex_torch.
 *
 * gcpx_cem_warm_start: the Gaussian a re-plan starts from.  prev [K][S][A] the previous best sample of each task, shift int32 [K] the
 *   steps executed since.  Task k with s = shift[k]: s < 0 (no previous plan): mean = 0, std = init_std.  Otherwise, where t + s < S:
 *   mean[k][t] = prev[k][t + s], std = warm_std * init_std (one float32 product, formed once); behind that, t + s >= S: mean = 0,
 *   std = init_std (so s >= S is a cold start).  No load is made through a shifted index outside [0, S), prev of a task with s < 0 is not
 *   read, a NaN in prev stays a NaN.  One thread per (task, column).
 * gcpx_cem_population_ex: gcpx_cem_population with carried rows and temporally correlated noise.
 *   rows j < m:  out[k][j] = prev_pop[k][prev_idx[k][j]], prev_pop [K][n_prev][S][A], prev_idx int32 [K][m]: copied as 32-bit words,
 *     not clamped and not re-noised.  Every index is range-checked before it is used: a task with an index outside [0, n_prev) gets NaN
 *     in its m carried rows, no load is made through it.  m == 0: prev_pop, prev_idx and n_prev are not looked at (may be null / 0).
 *   rows j >= m: xi_0 = eps_0, xi_t = (rho * xi_{t-1}) + (c * eps_t) along the steps of each column, c = (float) sqrt(1 - (double) rho *
 *     rho) formed once on the host: unit variance at every step.  out = clamp(mean + std * xi, -clip, clip) as in gcpx_cem_population.
 *     rho == 0: xi = eps, the bits of gcpx_cem_population (nothing is multiplied by 0).
 *   out may be eps (in place; rows < m of eps are not read); it may not overlap prev_pop.  A thread owns whole columns of a row: one
 *   column for A = 1 and A >= 5, all A of them for A = 2 .. 4.
 *
 * GCPX_ERR_INVALID_ARG, nothing launched: a null pointer, a size <= 0 or S * A >= 2^31, m < 0, m > n, m > n_prev, rho outside [0, 1) or
 *   NaN, warm_std outside (0, 1] or NaN, out overlapping prev_pop, more than 2^30 workgroups. */
int gcpx_cem_warm_start(const float* prev, const int32_t* shift, float init_std, float warm_std, float* mean, float* std, int32_t K,
                        int32_t S, int32_t A, void* stream);
int gcpx_cem_population_ex(const float* mean, const float* std, const float* eps, float clip, float rho, const float* prev_pop,
                           const int32_t* prev_idx, int32_t m, int32_t n_prev, float* out, int32_t K, int32_t n, int32_t S, int32_t A,
                           void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The inference-mode encoder of F frames in one launch, each frame on its own (csrc/enc_frames.hip): what the closed-loop policy
 * computes one frame per call, gcp/planning/planner_policy.py:222-227 (`self.planner.encoder(img)[0][:, :, 0, 0]`), for the frames of
 * all episodes at once (video-gcp_amd/model.py: GCPTreeModel.encode_frames; control.py --batch_encode 1).
 *
 * images [F][3][S][S] float32 NCHW in [-1, 1], 16-byte aligned; row f of the result, nz_enc floats, is written to
 * out + f * out_stride (floats; out_stride >= nz_enc).  weights: the blob of packing.pack_encoder_frames (16-byte aligned):
 *   input    w [48 (ci, ky, kx)][16], bias [16]                                         4x4, stride 2, pad 1, bias, LeakyReLU
 *   pyramid  w [16 taps][Cin/16][Cout/16][64][4], bias, scale, shift [Cout]  each     conv + bias, fmaf(raw, scale, shift), LeakyReLU
 *   head     w [nz_enc][16 c_top (y, x, c)], bias [nz_enc]                              4x4 valid + bias
 * with scale / shift the BatchNorm's running statistics folded as gcpx_bn_fold folds them, leaky_slope the LeakyReLU's slope.
 * Exact f32 (f32 operands and accumulation).  The summation order of every output value is a function of (layer, pixel, channel)
 * alone: a frame's row has the same bits whatever F, the frame's index or the grid.  Out-of-image taps contribute zeros and are never
 * formed into an address; nothing at or beyond frame F is read or written.  One launch on `stream`; every argument is passed by value
 * or points into memory the caller keeps: no host synchronisation is needed afterwards.
 *
 * GCPX_ERR_INVALID_ARG, no HIP call made: a null pointer, F <= 0, S other than 32 or 64, ngf other than 16, nz_enc not a multiple of 16
 *   or above 256, out_stride < nz_enc, a misaligned images / weights pointer.  There is no fallback to gcpx_conv4x4s2. */
int gcpx_encode_frames(const float* images, const float* weights, float* out, int64_t out_stride, int32_t F, int32_t S, int32_t ngf,
                       int32_t nz_enc, float leaky_slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCPX_H */
