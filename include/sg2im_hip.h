/*
 * sg2im_hip.h -- C ABI of libsg2im_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels behind the
 * scene-graph -> image G+D training step.
 *
 * The reference (ashual/scene_generation) has no FFI: its hot path dispatches PyTorch ops.  Each entry
 * point below replaces the op group a reference call site dispatches (cited per function, paths
 * relative to /root/reference/scene_generation/).  The only caller is the Python host layer
 * (scene_generation_amd/ops/, ctypes); INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - caller owns every buffer (incl. workspace); no allocation, no host sync, no stream creation inside
 *   - all pointers are DEVICE pointers unless the name ends in _host; tensors are dense row-major,
 *     images NCHW fp32, indices int64 (graph/crop) or int32 (CSR / segment offsets / plans)
 *   - `stream` is a hipStream_t passed as void*; every launch goes to that stream, in order
 *   - return 0 = OK; <0 = argument error detected before launch; >0 = hipError_t from the launch
 *     sg_last_error_string() describes the last non-zero return on the calling thread
 *   - thread-safe for distinct streams.  Global state, all of it: the opt-in profiler (sg_prof_*), the shape-table cache
 *     (sg_plan_cache_*: mutex-guarded) and the option table (sg_set_option: atomic ints, initialised once at load time)
 */
#ifndef SG2IM_HIP_H
#define SG2IM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sgStream;

/* activation codes fused into epilogues */
enum { SG_ACT_NONE = 0, SG_ACT_RELU = 1, SG_ACT_LEAKY = 2, SG_ACT_TANH = 3, SG_ACT_SIGMOID = 4 };
/* scalar loss kinds (sg_loss_fwd / sg_loss_bwd) */
enum { SG_LOSS_MSE_CONST = 0, SG_LOSS_MSE = 1, SG_LOSS_L1 = 2, SG_LOSS_BCE_LOGITS_CONST = 3,
       SG_LOSS_MEAN = 4,               /* sum a_i                      (wgan_*_loss, losses.py:93-112) */
       SG_LOSS_MSE_SIGMOID_CONST = 5,  /* (sigmoid(a_i) - target)^2    (lsgan_*_loss, losses.py:115-132) */
       SG_LOSS_BCE_PROB_CONST = 6 };   /* nn.BCELoss vs a constant     (GANLoss(use_lsgan=False), losses.py:147) */
#define SG_WSUM_MAX 32
/* return code of an index operand outside its range (the reference raises IndexError: graph.py:79-80, model.py:131) */
#define SG_ERR_INDEX (-2)

int sg_version(void);
const char* sg_last_error_string(void);
/* Tuning / debugging switches (which kernel variant or threshold a launch plan uses; results stay within the tolerances of
 * the parity suite for every setting).  Each switch has a compiled-in default and is initialised ONCE, when the library is
 * loaded, from the environment variable SG_<NAME> (upper case) if that is set; afterwards the library never reads the
 * environment.  sg_set_option stores atomically: launches planned after the call see the new value.  Names:
 * sg_option_name(0 .. sg_num_options()-1).  Returns -1 for an unknown name. */
int sg_num_options(void);
const char* sg_option_name(int index);
int sg_option_default(int index);
int sg_get_option(const char* name, int* value);
int sg_set_option(const char* name, int value);
/* device bytes held by the shape-table cache; drop it (synchronises the tables' build events) */
size_t sg_plan_cache_bytes(void);
int sg_plan_cache_clear(void);
/* What launches SHARE on the current device (a host query for tests; it adds no option, changes no launch and is never called on
 * the training path).  Launches outside a stream capture draw their ticket counters from a ring of their own (device, stream),
 * created by the first such launch of that stream; captured launches draw from one region per device that is handed out once.  A
 * launch leaves every counter it drew at zero.  Before the ring of ``stream`` exists its three fields read 0, and before the
 * device's first eager request for a counter every counter field does.  ``count_nonzero`` != 0: synchronises the device, copies
 * every counter of the device (the capture region and the rings of all its streams) to the host and counts those that are not 0. */
typedef struct sgRuntimeState {
  int ring_size, ring_at, ring_laps;        /* the eager ring `stream` draws from: size, next index, wraps so far */
  int captured_size, captured_used;         /* capture region of the current device */
  int counters_nonzero;                     /* -1 unless asked for */
  size_t tail_bytes, tail_captured_bytes;   /* scratch of (device, stream); scratch shared by captured launches */
  int tail_retired;                         /* outgrown scratch buffers still held */
} sgRuntimeState;
int sg_runtime_state(sgStream stream, int count_nonzero, sgRuntimeState* out);

/* ---------------------------------------------------------------------------------------------
 * Convolution family = implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain).
 * Replaces nn.Conv2d / nn.ConvTranspose2d (+ the nn.ReflectionPad2d, Interpolate(x2, nearest) and
 * torch.cat((layout, img), 1) feeding them) at generators.py:20-27,68-89, layers.py:160-180,251-270,
 * discriminators.py:137-158,215-234 and trainer.py:246,250,328.
 * Every GEMM family of the convolutions runs from one host-side plan function that a host-only query reports (tile, loaders,
 * mask, split, reduce -- under the current options, launching nothing): sg_conv2d_fwd_plan (forward gathers: sg_conv2d_fwd,
 * _fwd_sparse, _fwd_perimage), sg_conv2d_tgather_plan (transposed gathers), sg_conv2d_wgrad_plan (weight gradients) and
 * sg_conv2d_wino_plan (Winograd).  The vector-ALU kernels report theirs the same way: sg_conv2d_head_plan (one output channel) and
 * sg_conv2d_smallm_plan (ReflectionPad(3) + 7x7 to <= 4 channels).
 * A desc with reflection padding must satisfy pad < H*upsample, pad < W*upsample and (OH-1)*stride + KS <= H*upsample + 2*pad
 * (the same for the width): the gathers mirror a coordinate once.  Every entry point refuses any other (as torch refuses it).
 * ------------------------------------------------------------------------------------------- */
typedef struct sgConvDesc {
  int32_t N;            /* images */
  int32_t C1, C2;       /* input channels taken from x1 / x2 (channel concat folded into the gather; C2=0 if none) */
  int32_t H, W;         /* stored input spatial size */
  int32_t Cout;
  int32_t KS;           /* square kernel: 1, 3, 4 or 7 */
  int32_t stride;       /* 1 or 2 */
  int32_t pad;
  int32_t pad_reflect;  /* 0 zero padding, 1 reflection padding (nn.ReflectionPad2d folded in) */
  int32_t upsample;     /* 1, or 2 = nearest x2 upsample of the input folded in (layers.py:304-314) */
  int32_t OH, OW;       /* output spatial size */
  int32_t out_pad;      /* conv-transpose only: output_padding */
  int32_t x2_broadcast; /* 1: x2 is [N, C2] and is broadcast over H x W (the one-hot class map of discriminators.py:107-110) */
} sgConvDesc;

/* scratch the caller must provide (kind 0: conv / convT forward, 1: conv / convT dgrad, 2: conv / convT wgrad) */
size_t sg_conv2d_ws_bytes(const sgConvDesc* d, int kind);
/* y[N,Cout,OH,OW] = act(conv(x) + bias) ; w [Cout, C1+C2, KS, KS] */
int sg_conv2d_fwd(const sgConvDesc* d, const float* x1, const float* x2, const float* w, const float* bias,
                  float* y, int act, float slope, void* ws, size_t ws_bytes, sgStream stream);
/* gx[N, c_end-c_begin, Hg, Wg]: gradient w.r.t. input channels [c_begin, c_end) of the *padded/upsampled*
 * logical input: Hg = H*upsample + (pad_reflect ? 2*pad : 0).  Fold with sg_pad_upsample_bwd. */
int sg_conv2d_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, int c_begin, int c_end,
                    void* ws, size_t ws_bytes, sgStream stream);
/* Same gathers with PER-IMAGE weights wimg / gwimg [N, Cout, L, KS, KS] (position j of image n's list <-> channel
   chan_list[n][j]): the factored form of a conv over a masks_to_layout() layout, whose channels are linear combinations of
   the per-object sampled-mask planes (layout = sum_o vecs[o] (x) S_o, reference layout.py:85-86), so
   conv(layout) = sum_o (sum_c vecs[o][c] W[:, c]) * S_o: the "channels" become the <= 9 objects of the image. */
int sg_conv2d_fwd_perimage(const sgConvDesc* d, const float* x1, const float* x2, const float* wimg, const float* bias,
                           const int32_t* chan_list, const int32_t* chan_cnt, int L, float* y, int act, float slope,
                           void* ws, size_t ws_bytes, sgStream stream);
/* (reflection-padded 7x7 stride-1 convs: sg_conv2d_sparse_ws_bytes(d, L, 2) includes room for reflect-padded copies of the listed
   planes, which the weight gradient then gathers from -- option wgrad_padded; a smaller workspace that still holds the gather
   route's bytes is accepted and runs the gather route, same result bit for bit) */
int sg_conv2d_wgrad_perimage(const sgConvDesc* d, const float* gy, const float* x1, const float* x2,
                             const int32_t* chan_list, const int32_t* chan_cnt, int L, float* gwimg, void* ws,
                             size_t ws_bytes, sgStream stream);
/* Data gradient w.r.t. the ACTUAL [N, c_end-c_begin, H, W] input of ReflectionPad2d(1) + 3x3 stride-1 conv (the
   ResnetBlock convs, reference layers.py:251-270): the reflection fold is applied to gy (one pre-folded copy per tap)
   instead of computing the gradient on the padded (H+2)x(W+2) grid and folding it with sg_pad_upsample_bwd. */
int sg_conv2d_dgrad_folded_supported(const sgConvDesc* d);
size_t sg_conv2d_dgrad_folded_ws_bytes(const sgConvDesc* d);
int sg_conv2d_dgrad_folded(const sgConvDesc* d, const float* gy, const float* w, float* gx, int c_begin, int c_end,
                           void* ws, size_t ws_bytes, sgStream stream);
/* gw[Cout, C1+C2, KS, KS] (+ gb[Cout] if non-null) */
int sg_conv2d_wgrad(const sgConvDesc* d, const float* gy, const float* x1, const float* x2, float* gw, float* gb,
                    void* ws, size_t ws_bytes, sgStream stream);
/* Channel-sparse variants for a layer whose input is a masks_to_layout() layout (reference model.py:165-168 and
   layout.py:64-93: per image only the one-hot planes of the classes present and the dense representation block are
   non-zero).  chan_list [N, L] int32: ascending concat-channel ids (over x1|x2) that may be non-zero in image n, the
   first chan_cnt[n] (<= L) entries are used; every other channel of that image MUST be all-zero or the result
   differs from sg_conv2d_fwd / sg_conv2d_wgrad.  Same outputs as the dense calls (different summation order).
   The workspace of sg_conv2d_fwd_sparse and sg_conv2d_fwd_perimage must be 16-byte aligned (they build compact per-image weight
   rows in it and read them as float4); a misaligned one is refused before anything is launched. */
size_t sg_conv2d_sparse_ws_bytes(const sgConvDesc* d, int L, int kind /* 0 fwd, 2 wgrad */);
int sg_conv2d_fwd_sparse(const sgConvDesc* d, const float* x1, const float* x2, const float* w, const float* bias,
                         const int32_t* chan_list, const int32_t* chan_cnt, int L, float* y, int act, float slope,
                         void* ws, size_t ws_bytes, sgStream stream);
int sg_conv2d_wgrad_sparse(const sgConvDesc* d, const float* gy, const float* x1, const float* x2,
                           const int32_t* chan_list, const int32_t* chan_cnt, int L, float* gw, float* gb,
                           void* ws, size_t ws_bytes, sgStream stream);
/* Winograd F(2x2, 3x3) forward / data gradient / weight gradient for 3x3 stride-1 pad-1 convs (reflection padding: the
   ResnetBlock convs, layers.py:251-270; zero padding: the VGG19 convs of VGGLoss, losses.py:183-198, and -- behind the folded
   nearest x2 upsample -- mask_net, generators.py:20-22) with >= 128 channels on both sides, whose channel counts and tile count
   N*(OH/2)*(OW/2) are all multiples of 128 (other counts, mask_net's 192 channels among them, run the direct kernels): 2.25x
   fewer MACs; fp32 throughout, results agree with
   sg_conv2d_fwd / _dgrad / _wgrad to fp32 rounding (gb via sg_channel_sum). */
int sg_conv2d_wino_supported(const sgConvDesc* d);
size_t sg_conv2d_wino_ws_bytes(const sgConvDesc* d);
/* ut_save (optional, sg_conv2d_wino_ut_floats(d) floats): the forward also writes the filter transform with the channel
   roles swapped -- what sg_conv2d_wino_dgrad of the SAME conv multiplies with (ut_saved): the weights are transformed once
   per step instead of once per direction. */
size_t sg_conv2d_wino_ut_floats(const sgConvDesc* d);
/* v_save / ytp_save (optional, sg_conv2d_wino_v_floats(d) / sg_conv2d_wino_ytp_floats(d) floats; 0 = not applicable to this
   desc): the forward keeps its input transform V[16][P][C1], the data gradient its gradient transform Ytp[16][P][Cout], and
   sg_conv2d_wino_wgrad of the SAME conv in the same step, given both (v_saved, ytp_saved), runs its 16 GEMMs straight on them
   instead of transforming x and gy a second time. */
size_t sg_conv2d_wino_v_floats(const sgConvDesc* d);
size_t sg_conv2d_wino_ytp_floats(const sgConvDesc* d);
int sg_conv2d_wino_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y, int act,
                       float slope, float* ut_save, float* v_save, void* ws, size_t ws_bytes, sgStream stream);
int sg_conv2d_wino_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, const float* v_saved,
                         const float* ytp_saved, void* ws, size_t ws_bytes, sgStream stream);
/* gx [N, C1, H, W] (all input channels): Winograd on the padded gradient grid + reflection fold */
int sg_conv2d_wino_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, const float* ut_saved,
                         float* ytp_save, void* ws, size_t ws_bytes, sgStream stream);
/* ReflectionPad(1) + Conv3x3 + InstanceNorm2d(affine=False) [+ ReLU / LeakyReLU] [+ residual] of a ResnetBlock (layers.py:251-270,
 * 296) on the Winograd F(4x4,3x3) path, fused at both ends of the batched GEMMs (sg_conv2d_wino_in_supported: 8x8 .. 16x16 planes,
 * channels multiples of 128, tile count a multiple of 64):
 *   forward : output transform + bias + InstanceNorm + activation + skip in one launch; ypre = the conv result (kept for the
 *             backward), out = act((ypre - mean) * rstd) + skip, mean / rstd [N * Cout]
 *   backward: InstanceNorm's backward and the gradient transform in one launch (gconv = the conv's gy: its weight gradient
 *             is sg_conv2d_wino_wgrad(d, gconv, x, gw, v_saved, ytp_saved)); gx is computed when non-NULL; gb [Cout], when
 *             non-NULL, receives the conv's bias gradient = sum of gconv over images and pixels (per-image plane sums from the
 *             same launch, added over the images in ascending order by one small launch; NULL: the caller runs
 *             sg_channel_sum(gconv)).  ut_save / v_save / ytp_save as in sg_conv2d_wino_fwd / _dgrad.
 * Same arithmetic as sg_conv2d_wino_fwd + sg_instnorm_fwd / sg_instnorm_bwd + sg_conv2d_wino_dgrad up to the order of the
 * per-plane sums. */
int sg_conv2d_wino_in_supported(const sgConvDesc* d);
int sg_conv2d_wino_fwd_instnorm(const sgConvDesc* d, const float* x, const float* w, const float* bias, const float* skip,
                                float* ypre, float* out, float* mean, float* rstd, float eps, int act, float slope,
                                float* ut_save, float* v_save, void* ws, size_t ws_bytes, sgStream stream);
int sg_conv2d_wino_dgrad_instnorm(const sgConvDesc* d, const float* gout, const float* ypre, const float* mean, const float* rstd,
                                  int act, float slope, const float* w, float* gconv, float* gx, float* gb,
                                  const float* ut_saved, float* ytp_save, void* ws, size_t ws_bytes, sgStream stream);
/* bf16-operand path of the same ResnetBlock convs (ReflectionPad2d(1) + Conv2d(C, C, 3), stride 1), the opt-in mixed-precision
 * trunk of GlobalGenerator: every product of the forward / data-gradient / weight-gradient GEMMs takes its operands rounded to
 * bf16 (round to nearest even), the sums are fp32 (v_mfma_f32_16x16x32_bf16); x, y, w, bias and all gradients stay fp32 NCHW.
 * Supported (sg_conv3x3r_bf16_supported): C1 == Cout, C1 % 64 == 0 (64 .. 4096), C2 == 0, KS 3, stride 1, pad 1, pad_reflect,
 * no upsample, H, W >= 2, OH == H, OW == W.  Other shapes return -1 ("unsupported shape").  ws: sg_conv3x3r_bf16_ws_bytes(d)
 * (one size for all three calls).  Deterministic (split-K slices are reduced in a fixed order); no allocation, no host sync.
 *   fwd  : y [N, Cout, H, W] = conv(reflectpad1(x), w) + bias (bias may be NULL)
 *   dgrad: gx [N, C1, H, W], the reflection fold included
 *   wgrad: gw [Cout, C1, 3, 3]; gb [Cout] = channel sum of gy (fp32, sg_channel_sum) when non-NULL */
int sg_conv3x3r_bf16_supported(const sgConvDesc* d);
size_t sg_conv3x3r_bf16_ws_bytes(const sgConvDesc* d);
int sg_conv3x3r_bf16_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y, void* ws,
                         size_t ws_bytes, sgStream stream);
int sg_conv3x3r_bf16_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, void* ws, size_t ws_bytes,
                           sgStream stream);
int sg_conv3x3r_bf16_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, float* gb, void* ws,
                           size_t ws_bytes, sgStream stream);
/* The GEMM stage of the Winograd convs on its own (the transforms of layers.py:251-270's convs aside):
 *   c[m][z*cols + j] = sum_k a[z][m][k] * b[z*cols + j][k],   z < nbatch   (both operands K-contiguous, fp32 MFMA)
 * tile: 0 = 128x128, 1 = 64x128, 2 = 64x64, 3 = 64x64 with 16-deep k-tiles; M, cols multiples of the tile, K of 32.  Exposed for
 * micro-benchmarks of candidate Winograd forms (tools/bench_wino_gemm.py: the F(4x4,3x3) study) and for tests. */
int sg_batched_gemm_nt(const float* a, const float* b, float* c, int nbatch, int M, int cols, int K, int tile,
                       sgStream stream);
/* Winograd F(2x2, 4x4) for the stride-1 4x4 convs of the PatchGANs (reference discriminators.py:221-228:
   nn.Conv2d(nf_prev, nf, kernel_size=4, stride=1, padding=2), 256 -> 512 channels: the largest layer of the discriminator steps):
   KS 4, stride 1, zero padding 0..3, one source, C1 and Cout multiples of 128, >= 256 output tiles.  25 multiplies per 2x2
   output tile and channel pair instead of 64; fp32 throughout, results agree with sg_conv2d_fwd / _dgrad / _wgrad to fp32
   rounding (asserted at the same tolerances; gb via sg_channel_sum).  ws: sg_conv2d_wino24_ws_bytes. */
int sg_conv2d_wino24_supported(const sgConvDesc* d);
size_t sg_conv2d_wino24_ws_bytes(const sgConvDesc* d);
int sg_conv2d_wino24_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y, int act,
                         float slope, void* ws, size_t ws_bytes, sgStream stream);
int sg_conv2d_wino24_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, void* ws, size_t ws_bytes,
                           sgStream stream);
int sg_conv2d_wino24_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, void* ws, size_t ws_bytes,
                           sgStream stream);
/* host-only query of THE launch plan of a Winograd entry point (sg_conv2d_wino_* / sg_conv2d_wino24_* launch exactly this; the
 * query reports it): which form, kernels and GEMM tiles run for this desc under the current options.  Never touches the device.
 *   entry       SG_WINO_*: the entry point
 *   align_mask  SG_WA_* bits of the operands whose address is 16-byte aligned: X (x), W (w), Y (y; ypre / out / skip of the fused
 *               forward), GY (gy; gout / ypre / gconv of the fused backward), GX (gx), GW (gw)
 *   saved_mask  SG_WS_* bits of the saved operands passed: UT (ut_save / ut_saved), V (v_save / v_saved), YTP (ytp_save / ytp_saved)
 * Returns non-zero for a bad entry, a null plan, an unsupported desc and for what the entry point itself rejects before its
 * first launch: an unaligned operand on an F(4x4,3x3) shape or on a fused entry, a saved operand the desc cannot use.
 *   form        SG_WF_F23_GENERIC: F(2x2,3x3) over the (padded) grid -- every forward and weight gradient that is not F(4x4,3x3),
 *               and the data gradient on the padded gradient grid followed by sg_pad_upsample_bwd; SG_WF_F23_ADJOINT: the data
 *               gradient over the output tiles + reflection fold; SG_WF_F43: F(4x4,3x3); SG_WF_F24: F(2x2,4x4)
 *   P / Ps      tiles of the forward / weight gradient and the columns their GEMM runs on (padded to whole tiles)
 *   Pd / Pds    the same for the data gradient (F23 generic on a reflect desc: the (H/2+1) x (W/2+1) tiles of the padded grid)
 *   in_kernel   transform of the entry's moving operand (x: forward, gy: data gradient; both: a weight gradient that rebuilds its
 *               operands): SG_WK_IN_LDS (small planes staged in LDS) or SG_WK_IN_GENERAL; SG_WK_NONE: weight gradient on saved operands
 *   wt_kernel   filter transform: SG_WK_WT_LDS, SG_WK_WT_PLAIN, SG_WK_NONE (saved operand used; weight gradient)
 *   fold_kernel data gradient: SG_WK_FOLD_CELLS / SG_WK_FOLD_WALK (F23 adjoint), SG_WK_FOLD_F43, SG_WK_FOLD_PAD_UPSAMPLE
 *               (sg_pad_upsample_bwd behind the generic form), SG_WK_NONE
 *   bm x bn     GEMM tile;  nsub: k-tile depth / 16;  kfold: chunk of the channel sum (0 = one chain, 128, 256);
 *   pipe        main loop of the 128x128 K-contiguous GEMM (option wino_pipe: 1 or 2), 0 elsewhere
 *   wgrad_src   weight gradient: SG_WSRC_SAVED (GEMM over the x-contiguous saved operands) or SG_WSRC_REBUILT; 0 elsewhere
 *   norm_tiles  fused entries: tiles per thread of the output transform + InstanceNorm kernel (1 or 4); 0 elsewhere
 *   TH .. Pc    F(2x2,4x4): tile grid of the output (TH x TW) and of the input (THd x TWd), k-chunks S of Pc tiles each
 * Not reported: the F(4x4,3x3) tail split (option w43_tail_split) -- it depends on the CU count. */
enum { SG_WINO_FWD = 0, SG_WINO_DGRAD = 1, SG_WINO_WGRAD = 2, SG_WINO_FWD_INSTNORM = 3, SG_WINO_DGRAD_INSTNORM = 4,
       SG_WINO24_FWD = 5, SG_WINO24_DGRAD = 6, SG_WINO24_WGRAD = 7 };
enum { SG_WA_X = 1, SG_WA_W = 2, SG_WA_Y = 4, SG_WA_GY = 8, SG_WA_GX = 16, SG_WA_GW = 32, SG_WA_ALL = 63 };
enum { SG_WS_UT = 1, SG_WS_V = 2, SG_WS_YTP = 4 };
enum { SG_WF_UNSUPPORTED = 0, SG_WF_F23_GENERIC = 1, SG_WF_F23_ADJOINT = 2, SG_WF_F43 = 3, SG_WF_F24 = 4 };
enum { SG_WK_NONE = 0, SG_WK_IN_LDS = 1, SG_WK_IN_GENERAL = 2, SG_WK_WT_LDS = 1, SG_WK_WT_PLAIN = 2,
       SG_WK_FOLD_CELLS = 1, SG_WK_FOLD_WALK = 2, SG_WK_FOLD_F43 = 3, SG_WK_FOLD_PAD_UPSAMPLE = 4 };
enum { SG_WSRC_SAVED = 1, SG_WSRC_REBUILT = 2 };
typedef struct sgWinoPlan {
  int32_t form;
  int32_t P, Ps, Pd, Pds;
  int32_t in_kernel, wt_kernel, fold_kernel;
  int32_t bm, bn, nsub, kfold, pipe;
  int32_t wgrad_src, norm_tiles;
  int32_t TH, TW, THd, TWd, S, Pc;
} sgWinoPlan;
int sg_conv2d_wino_plan(const sgConvDesc* d, int entry, int align_mask, int saved_mask, sgWinoPlan* plan);
/* Direct (vector-ALU) kernels for ReflectionPad2d(3) + Conv2d(C, Cout <= 4, 7) [+ act]: the generator's RGB head
   (reference generators.py:88-90).  Same results as sg_conv2d_fwd / sg_conv2d_wgrad (gb via sg_channel_sum).
   Alignment: the forward stores y, and the weight gradient loads gy, four pixels at a time (W % 4 == 0 keeps every row on the
   vector grid): y (forward) and gy (weight gradient) must be 16-byte aligned, and both entry points refuse any other address on
   the host, before a launch.
   sg_conv2d_smallm_plan (host only, launches nothing; the launchers run from the same function):
     entry    SG_SMALLM_FWD or SG_SMALLM_WGRAD
     MO       the instantiation: output rows per thread (3 for Cout == 3, else 4; rows >= Cout repeat row Cout - 1, never stored)
     grid_x, grid_y, grid_z   forward: 64-column tiles x 16-row tiles x images;  weight gradient: channels x images x 1
     col_blocks, row_blocks   weight gradient: blocks of 128 columns x 16 rows each workgroup walks (forward: 1 x 1)
     iters    forward: channel pairs each of the two thread groups walks, (C1 + 1) / 2;  idle_last: 1 when the second group has
              no channel in the last one (odd C1);  both 0 for the weight gradient */
enum { SG_SMALLM_FWD = 0, SG_SMALLM_WGRAD = 2 };
typedef struct sgSmallmPlan {
  int32_t MO;
  int32_t grid_x, grid_y, grid_z;
  int32_t col_blocks, row_blocks;
  int32_t iters, idle_last;
} sgSmallmPlan;
int sg_conv2d_smallm_supported(const sgConvDesc* d);
size_t sg_conv2d_smallm_ws_bytes(const sgConvDesc* d);
int sg_conv2d_smallm_plan(const sgConvDesc* d, int entry, sgSmallmPlan* plan);
int sg_conv2d_smallm_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y, int act,
                         float slope, sgStream stream);
int sg_conv2d_smallm_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, void* ws, size_t ws_bytes,
                           sgStream stream);
/* Direct (vector-ALU) kernels for SINGLE-output-channel convs with zero padding, stride 1, KS in {1,3,4}: the PatchGAN score
   heads (reference discriminators.py:152-158,232-234) and the 1x1 head of mask_net (generators.py:27).  Memory-bound
   reductions; channel chunks / images are combined in a fixed order.  ws: sg_conv2d_head_ws_bytes.  gb via sg_channel_sum.
   No alignment is required: the forward's 1x1 stream kernel reads x and writes y as float4 and runs only where both are 16-byte
   aligned (the LDS-staged kernel takes the call otherwise).
   sg_conv2d_head_plan (host only, launches nothing; the launchers run from the same function): what sg_conv2d_head_fwd / _dgrad /
   _wgrad (entry SG_HEAD_*) launches for this desc.  x_mod16, y_mod16: the addresses of x and y modulo 16 (0, 4, 8 or 12; they
   matter to the forward only).  Returns non-zero for a desc sg_conv2d_head_supported refuses.
     kind        SG_HEAD_STREAM: the 1x1 stream kernel (forward; KS 1, pad 0, H*W % 4 == 0, x and y aligned);  SG_HEAD_STAGED: the
                 LDS-staged kernels
     CH          channels per workgroup (staged; from the LDS budget, at most 16), or the 8 channels a stream thread loads together
     chunks      workgroups (staged) / load groups (stream) along the channels;  last_chunk: the channels of the last one
     lds_bytes   dynamic LDS of the entry's launch (0 for the stream kernel)
     Q_full, Q_last   weight gradient: the pixel parts (1, 2, 4, 8 or 16) a full and the last chunk split the plane into; else 0 */
enum { SG_HEAD_FWD = 0, SG_HEAD_DGRAD = 1, SG_HEAD_WGRAD = 2 };
enum { SG_HEAD_STREAM = 1, SG_HEAD_STAGED = 2 };
typedef struct sgHeadPlan {
  int32_t kind, CH, chunks, last_chunk;
  int32_t lds_bytes, Q_full, Q_last;
} sgHeadPlan;
int sg_conv2d_head_supported(const sgConvDesc* d);
size_t sg_conv2d_head_ws_bytes(const sgConvDesc* d);
int sg_conv2d_head_plan(const sgConvDesc* d, int entry, int x_mod16, int y_mod16, sgHeadPlan* plan);
int sg_conv2d_head_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y, int act,
                       float slope, void* ws, size_t ws_bytes, sgStream stream);
int sg_conv2d_head_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, sgStream stream);
int sg_conv2d_head_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, void* ws, size_t ws_bytes,
                         sgStream stream);
/* nn.ConvTranspose2d(k3,s2,p1,op1) : w [Cin, Cout, KS, KS]; desc.H,W = input size, OH,OW = output size */
int sg_convT2d_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y,
                   void* ws, size_t ws_bytes, sgStream stream);
int sg_convT2d_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, void* ws, size_t ws_bytes,
                     sgStream stream);
int sg_convT2d_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, float* gb,
                     void* ws, size_t ws_bytes, sgStream stream);
/* host-only query of the launch plan of a transposed gather (csrc/igemm_kn1.hip): what sg_convT2d_fwd, sg_conv2d_dgrad on the
 * channel window [c_begin, c_end) or sg_conv2d_dgrad_folded launches for this desc, from the same functions the launchers use,
 * under the current options (tile, splits, fixedtap, ...).  Never touches the device.  ws_mod16: the workspace address modulo 16
 * (0, 4, 8 or 12); ws_bytes: its size, 0 = what the entry point's own *_ws_bytes query returns (a smaller one can
 * switch split-K off).  The channel window is ignored for SG_TG_CONVT_FWD.
 *   route   SG_TG_PLAIN : one GEMM over all KS*KS taps (stride 1, 1x1 kernels, the folded form): ncls = 1, taps[0] = KS*KS,
 *                         PH/PW[0] = the whole pixel grid, ph0 = pw0 = 0
 *           SG_TG_PARITY: stride 2, KS >= 3: one GEMM per non-empty parity class, in launch order; class c reduces over
 *                         taps[c] taps (K[c] = channels * taps[c]) and writes pixels (ph0[c] + 2i, pw0[c] + 2j), i < PH[c], j < PW[c]
 *   loader  SG_TG_TABLE : taps from the k-table;  SG_TG_FIXED: taps fixed per thread (LoadFixedKN)
 *   a_vec   1: the weight matrix is read as float4, 0: scalar
 *   bm x bn the tile;  splits: split-K slabs (1 = none);  M: rows of the GEMM
 * Not reported (they depend on the CU count): the parity split (option par_split) and the tail split (w43_tail_split). */
enum { SG_TG_CONVT_FWD = 0, SG_TG_CONV_DGRAD = 1, SG_TG_DGRAD_FOLDED = 2 };
enum { SG_TG_PLAIN = 0, SG_TG_PARITY = 1 };
enum { SG_TG_TABLE = 0, SG_TG_FIXED = 1 };
typedef struct sgTGatherPlan {
  int32_t route, ncls;
  int32_t taps[4], PH[4], PW[4], ph0[4], pw0[4], K[4];
  int32_t loader, a_vec, bm, bn, splits, M;
} sgTGatherPlan;
int sg_conv2d_tgather_plan(const sgConvDesc* d, int entry, int c_begin, int c_end, int ws_mod16, size_t ws_bytes,
                           sgTGatherPlan* plan);
/* host-only query of THE launch plan of a weight-gradient GEMM (csrc/igemm_nk.hip: the launcher runs from the same function,
 * nk_launch_plan in csrc/igemm_core.h): what sg_conv2d_wgrad, sg_conv2d_wgrad_sparse, sg_conv2d_wgrad_perimage or sg_convT2d_wgrad
 * launches for this desc under the current options (wgrad_xcd, wgrad_rowsum, wgrad_padded).  Never touches the device.
 *   entry    SG_WG_*: the entry point;  L: length of the channel lists (SG_WG_SPARSE / SG_WG_PERIMAGE; ignored otherwise)
 *   a_mod16  address modulo 16 of the GEMM's A operand (gy; x for SG_WG_CONVT): 0, 4, 8 or 12
 *   ws_bytes the workspace offered (a short one can shrink the split, drop the XCD padding, the fused bias gradient or the
 *            padded planes).  Returns non-zero where the entry point itself would (bad desc, workspace too small, ...).
 *   form     SG_WG_TAP: tap-major columns [tap][cpad channels] (LoadTapNK);  SG_WG_GATHER: (channel, tap) columns of a few-channel
 *            input (LoadGatherNK);  SG_WG_PADDED: the same columns gathered from reflect-padded planes (LoadPaddedNK)
 *   bm x bn  the tile;  cpad: channels padded to whole column tiles (0 unless SG_WG_TAP)
 *   a_vec    1: A is read as float4 (LoadPixKVec), 0: scalar (LoadPixK)
 *   two      1: the tap loader reads two sources;  nomask: 1: the mask-free tap loader runs
 *   kchunk   k range (image x pixel) of one chunk;  chunks: chunks that hold pixels;  grid_z: chunks launched (after padding
 *            with empty chunks to a multiple of 8 for XCD pinning; N x S for per-image chunks)
 *   xcd      0: off, 1: the chunks are pinned to XCDs, 2: per-image chunks pinned to XCDs
 *   reduce   SG_WR_*: what runs behind the GEMM: nothing (it stored the result), slab_reduce, slab_reduce_wide, the un-permuting
 *            reduce of the tap-major slabs, the scatter of the per-image slabs through the inverse channel lists, the per-image
 *            copy, or the reduce over the chunks of each image
 *   rowsum_fused  1: a bias gradient asked for (gb != NULL) comes from the A loader's row sums, 0: from sg_channel_sum
 *   ws_needed     workspace bytes the GEMM and its reduce read or write (slabs, row sums, inverse lists, padded planes) */
enum { SG_WG_CONV = 0, SG_WG_SPARSE = 1, SG_WG_PERIMAGE = 2, SG_WG_CONVT = 3 };
enum { SG_WG_TAP = 0, SG_WG_GATHER = 1, SG_WG_PADDED = 2 };
enum { SG_WR_NONE = 0, SG_WR_SLAB = 1, SG_WR_WIDE = 2, SG_WR_UNPERMUTE = 3, SG_WR_SPARSE = 4, SG_WR_PERIMAGE = 5, SG_WR_GROUP = 6 };
typedef struct sgWgradPlan {
  int32_t form, bm, bn, cpad;
  int32_t a_vec, two, nomask;
  int32_t kchunk, chunks, grid_z, xcd;
  int32_t reduce, rowsum_fused, reserved;
  int64_t ws_needed;
} sgWgradPlan;
int sg_conv2d_wgrad_plan(const sgConvDesc* d, int entry, int L, int a_mod16, size_t ws_bytes, sgWgradPlan* plan);
/* host-only query of THE launch plan of a forward gather (csrc/igemm_kn0.hip: the launchers run from the same functions, kn_plan
 * and kn_sparse_plan in csrc/igemm_core.h): what sg_conv2d_fwd, sg_conv2d_fwd_sparse or sg_conv2d_fwd_perimage launches for this
 * desc under the current options (tile, t128_min, tile3, tile3_min, split_target, split_kmin, splits, fixedtap).  Never touches
 * the device.  Returns non-zero exactly where the entry point itself would for the same desc, L and workspace (the checks are one
 * function): bad desc, L outside (0, C1 + C2] for the list entries, a workspace below the entry's minimum or, for the list entries,
 * not 16-byte aligned -- and for a null plan, an unknown entry or a mod16 argument that is not 0, 4, 8 or 12.
 *   entry    SG_FW_*: the entry point;  L: length of the channel lists (SG_FW_SPARSE / SG_FW_PERIMAGE; ignored otherwise)
 *   w_mod16, y_mod16, ws_mod16  addresses modulo 16 of the weights, the result and the workspace (w_mod16 is ignored for the list
 *            entries: their weights are copied into compact rows first)
 *   ws_bytes the workspace offered (one that holds only the k-table switches split-K off)
 *   bm x bn  the tile;  a_vec 1: the weight rows are read as float4 (always, for the compact rows of the list entries), 0: scalar
 *   loader   SG_FW_TABLE: taps from the k-table (LoadGatherKN);  SG_FW_FIXED: taps fixed per thread (LoadFixedKN)
 *   two      1: the gather reads two sources;  bcast: 1: the second is a row per sample;  nomask: 1: the mask-free table loader runs
 *   K        the reduced extent: Cin * KS * KS, or the padded compact K of the list entries (L * KS * KS rounded up to 16)
 *   splits   split-K slabs (1 = none);  kchunk: k range of one slab (K when unsplit)
 *   reduce   SG_FR_*: what adds the slabs: nothing, the float4 reduce, or the scalar one (result or workspace misaligned, or
 *            OH * OW not a multiple of 4)
 *   batched  1: one GEMM per image over its own compact weights and k extent (the list entries: tiles never straddle images)
 *   ws_needed  workspace bytes the entry point requires for this plan (k-table area + slabs, or the list entries' tables)
 * Not reported (it depends on the CU count): the tail split (options w43_tail_split, tail_smax, tail_ktmin), which runs the
 * tiles of a ragged last round of an unsplit launch as k-pieces. */
enum { SG_FW_CONV = 0, SG_FW_SPARSE = 1, SG_FW_PERIMAGE = 2 };
enum { SG_FW_TABLE = 0, SG_FW_FIXED = 1 };          /* LoadGatherKN / LoadFixedKN */
enum { SG_FR_NONE = 0, SG_FR_VEC = 1, SG_FR_SCALAR = 2 };
typedef struct sgFwdPlan {
  int32_t bm, bn, a_vec, loader, two, bcast, nomask;
  int32_t K, splits, kchunk, reduce, batched;       /* K: Cin*KS*KS, or the padded compact K of the sparse forms */
  int64_t ws_needed;
} sgFwdPlan;
int sg_conv2d_fwd_plan(const sgConvDesc* d, int entry, int L, int w_mod16, int y_mod16, int ws_mod16, size_t ws_bytes,
                       sgFwdPlan* plan);
/* Interpolate(x2, nearest) + Conv2d(C, Cout, 3, padding=1) (mask_net, reference generators.py:20-21, layers.py:304-314) as a
 * SUB-PIXEL transposed convolution: every output pixel (2i+a, 2j+b) only sees a 2x2 neighbourhood of the stored input, with
 * the 3x3 taps that land on the same source pixel summed -- conv3x3(up2(x); w) == convT(k4, s2, p1)(x; wt) with
 *   wt[ci][co][kh][kw] = sum_{i in R(kh)} sum_{j in R(kw)} w[co][ci][i][j],  R(0)={2} R(1)={1,2} R(2)={0,1} R(3)={0}
 * i.e. 16 instead of 36 multiply-adds per (input pixel, channel pair).  sg_upconv3_fold_weights builds wt; forward, data and
 * weight gradient are sg_convT2d_{fwd,dgrad,wgrad} on a (KS=4, stride 2, pad 1) desc; sg_upconv3_unfold_wgrad is the adjoint
 * of the fold: gw[co][ci][i][j] = sum_{kh: i in R(kh)} sum_{kw: j in R(kw)} gwt[ci][co][kh][kw]. */
int sg_upconv3_fold_weights(const float* w, float* wt, int Cout, int Cin, sgStream stream);
int sg_upconv3_unfold_wgrad(const float* gwt, float* gw, int Cout, int Cin, sgStream stream);
/* fold a dgrad taken w.r.t. the reflect-padded and/or x2-upsampled logical input back onto the stored
 * input: gx[NC,H,W] = sum of gp[NC, H*up+2p, W*up+2p] over reflected / replicated positions */
int sg_pad_upsample_bwd(const float* gp, float* gx, int NC, int H, int W, int pad, int upsample, sgStream stream);
/* per-channel sum over (N, HW): bias gradients.  ws (optional, sg_channel_sum_ws_bytes) enables the two-stage form */
size_t sg_channel_sum_ws_bytes(int C);
int sg_channel_sum(const float* g, float* out, int N, int C, int HW, void* ws, size_t ws_bytes, sgStream stream);
/* host-only query of sg_channel_sum's launch plan (what it launches, from the same function): *S = slices of the two-stage
 * form, 1 = the single-stage kernel.  ws_bytes = 0 stands for "no workspace". */
int sg_channel_sum_plan(int N, int C, int HW, size_t ws_bytes, int* S);

/* ---------------------------------------------------------------------------------------------
 * Dense layers (nn.Linear inside build_mlp layers.py:215-231, generators.py:45, discriminators.py:23-27)
 * ------------------------------------------------------------------------------------------- */
int sg_linear_fwd(const float* x, const float* w, const float* b, float* y, int rows, int in_f, int out_f,
                  int act, float slope, sgStream stream);                 /* y = act(x w^T + b) */
int sg_linear_bwd_data(const float* gy, const float* w, float* gx, int rows, int in_f, int out_f, sgStream stream);
int sg_linear_bwd_weight(const float* gy, const float* x, float* gw, float* gb, int rows, int in_f, int out_f,
                         sgStream stream);
/* host-only query of a dense layer's launch plan (the three entry points above launch from the same function, under the
 * current options linear_skinny / linear_nsub).  entry: SG_LINEAR_*.  The GEMM is C[M][N] = sum_k A(m, k) B(n, k) with
 *   fwd: A = x, B = w, K = in_f;   bwd_data: A = gy, B = w, K = out_f;   bwd_weight: A = gy, B = x, K = rows
 * a_align / b_align: alignment in bytes (16, 8 or 4) of the address of A / B.
 *   *kind   SG_LIN_SKINNY: skinny_gemm_kernel<AV, BV> on 32x32 tiles with (AV, BV) = (*a_form, *b_form), *bm = *bn = 32, *nsub = 1
 *           SG_LIN_TILED : the LDS-tiled kernel on *bm x *bn tiles (64x64, or 32x128 when M <= 32), k-tiles 16 * *nsub deep
 *   *a_form / *b_form  how the operand is read: SG_LIN_ROWMAJOR = elem(x, k) = p[k*ld + x] (w of bwd_data, both operands of
 *           bwd_weight); otherwise rows of k -- skinny: 4 / 2 / 1 floats per load; tiled: SG_LIN_KVEC (float4 loads with a masked
 *           tail; needs K % 4 == 0 and 16-byte alignment of every K-contiguous operand) or SG_LIN_KSCALAR */
enum { SG_LINEAR_FWD = 0, SG_LINEAR_BWD_DATA = 1, SG_LINEAR_BWD_WEIGHT = 2 };
enum { SG_LIN_SKINNY = 0, SG_LIN_TILED = 1 };
enum { SG_LIN_ROWMAJOR = 0, SG_LIN_KSCALAR = 1, SG_LIN_KVEC = 4 };
int sg_linear_plan(int entry, int rows, int in_f, int out_f, int a_align, int b_align, int* kind, int* a_form, int* b_form,
                   int* bm, int* bn, int* nsub);
/* gx = gy * act'(.) evaluated from the activation OUTPUT y (relu / leaky / tanh / sigmoid) */
int sg_act_bwd(const float* y, const float* gy, float* gx, int64_t n, int act, float slope, sgStream stream);
int sg_act_fwd(const float* x, float* y, int64_t n, int act, float slope, sgStream stream);

/* ---------------------------------------------------------------------------------------------
 * Graph convolution (graph.py:58-122) + embeddings (model.py:131-132)
 * ------------------------------------------------------------------------------------------- */
/* destination-major CSR of the 2T (pass, t) entries: pass 0 = subject column, pass 1 = object column,
 * entries of a row ordered (pass, t ascending) == the order CPU scatter_add applies them (graph.py:98-101).
 * csr_off[O+1], csr_ent[2T] (t | pass<<30).
 * Zero-length calls (here and below: T = 0 triples, n = 0 indices, rows = 0, B = 0 boxes) are valid: the operands that are
 * indexed by the empty dimension may be null (a tensor without elements has no storage) and the other outputs are still
 * written -- csr_off all zero, sg_embedding_bwd's g_table and sg_crop_bbox_bwd's g_feats zero-filled.  sg_segment_sum takes
 * no count: its src must be valid whenever the CSR holds an entry. */
int sg_build_csr(const int64_t* edges /*T,2*/, int T, int O, int32_t* csr_off, int32_t* csr_ent, sgStream stream);
/* Range check of an index operand on the device: 0 if lo <= idx[i] < hi for every i < n, else SG_ERR_INDEX with the first
 * offending position and value in sg_last_error_string() -- what the reference's indexing raises as IndexError
 * (obj_vecs[s_idx], graph.py:79-80; nn.Embedding, model.py:131-132; feats[bbox_to_feats], bilinear.py:36).  Synchronises the
 * stream (a debugging aid, not part of the hot path); inside a stream capture it returns 0 unchecked.  The kernels
 * themselves do NOT validate indices: with the option check_indices = 1 (sg_set_option / SG_CHECK_INDICES=1) sg_build_csr
 * checks its edges this way, and the host mirror checks objs / obj_to_img / bbox_to_feats before the launches that use them. */
int sg_check_indices(const int64_t* idx, int64_t n, int64_t lo, int64_t hi, const char* what, sgStream stream);
/* out[t] = [obj[s_t], pred[t], obj[o_t]]  (graph.py:79-84) */
int sg_gather_concat_fwd(const float* obj, const float* pred, const int64_t* edges, float* out,
                         int T, int Do, int Dp, sgStream stream);
/* y[t] = act([obj[s_t], pred[t], obj[o_t]] W^T + b): the gather of graph.py:79-84 and the first nn.Linear (+ReLU) of net1
 * (graph.py:58-60,86) in ONE launch -- the A loader of the register-streaming GEMM reads the node / edge feature rows directly,
 * the (T, 2 Do + Dp) matrix is never written.  W: [out_f][2 Do + Dp].  Graphs too large for that kernel (the same size rule
 * as sg_linear_fwd) take gather + GEMM through ws (sg_gconv_gather_linear_ws_bytes: 0 for the fused form). */
size_t sg_gconv_gather_linear_ws_bytes(int T, int Do, int Dp, int out_f);
int sg_gconv_gather_linear_fwd(const float* obj, const float* pred, const int64_t* edges, const float* w, const float* b,
                               float* y, int T, int Do, int Dp, int out_f, int act, float slope, void* ws, size_t ws_bytes,
                               sgStream stream);
/* dst[i, :] = (sum over CSR entries e of row i of src[t_e, col_off[pass_e] : +width]) / (avg ? max(deg_i,1) : 1)
 * forward pool: src=new_t, col_off={0, H+Dout}; gather backward: src=g_cur_t, col_off={0, Do+Dp}. Bit-exact
 * w.r.t. sequential CPU scatter_add (deterministic, no atomics). */
int sg_segment_sum(const float* src, int src_ld, int col_off0, int col_off1, int width, const int32_t* csr_off,
                   const int32_t* csr_ent, float* dst, int O, int avg, sgStream stream);
/* g_new_t[t] = [g_pooled[s_t]/cnt_s, g_new_p[t], g_pooled[o_t]/cnt_o]  (dual of the pool, graph.py:89-116) */
int sg_pool_bwd(const float* g_pooled, const float* g_new_p, const int64_t* edges, const int32_t* csr_off,
                float* g_new_t, int T, int H, int Dout, int avg, sgStream stream);
int sg_embedding_fwd(const float* table, const int64_t* idx, float* out, int n, int dim, sgStream stream);
int sg_embedding_bwd(const float* g, const int64_t* idx, float* g_table, int n, int num_rows, int dim, sgStream stream);
/* strided 2-D copy: dst[r, dst_off : dst_off+width] = src[r, src_off : src_off+width] (concat / split glue) */
int sg_copy_cols(const float* src, int src_ld, int src_off, float* dst, int dst_ld, int dst_off, int rows, int width,
                 sgStream stream);
int sg_one_hot(const int64_t* idx, float* out, int n, int classes, int ld, int col_off, sgStream stream);

/* ---------------------------------------------------------------------------------------------
 * Normalisation / pooling (nn.InstanceNorm2d, nn.BatchNorm2d, nn.AvgPool2d(3,2,1,count_include_pad=False),
 * GlobalAvgPool layers.py:82-85)
 * ------------------------------------------------------------------------------------------- */
/* y = act((x-mean)*rstd) [+ skip]; biased variance per (n,c) plane, eps inside sqrt (layers.py:296) */
int sg_instnorm_fwd(const float* x, const float* skip, float* y, float* mean, float* rstd, int NC, int HW, float eps,
                    int act, float slope, sgStream stream);
int sg_instnorm_bwd(const float* x, const float* gy, const float* mean, const float* rstd, float* gx, int NC, int HW,
                    int act, float slope, sgStream stream);
/* host-only query of the InstanceNorm launch plan (sg_instnorm_fwd / _bwd launch from the same function, under the current
 * option instnorm_reg): *kind one of SG_IN_*, *G / *E the kernel's template arguments -- threads per plane and values (reg) or
 * float4s (vec) per thread; three-pass / big: threads per plane and 0.  aligned16: every operand pointer 16-byte aligned. */
enum { SG_IN_THREE_PASS_WAVE = 0, SG_IN_THREE_PASS_BLOCK = 1, SG_IN_REG = 2, SG_IN_VEC = 3, SG_IN_BIG = 4 };
int sg_instnorm_plan(int bwd, int HW, int aligned16, int* kind, int* G, int* E);
/* training: batch stats (biased var) + running-stat update (unbiased var, momentum) + num_batches_tracked++;
   ws (sg_batchnorm_ws_bytes) holds the per-slice partial statistics of the multi-workgroup reduction */
size_t sg_batchnorm_ws_bytes(int N, int C, int HW);
int sg_batchnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean,
                     float* save_rstd, float* running_mean, float* running_var, int64_t* num_batches, int N, int C,
                     int HW, float eps, float momentum, int training, int act, float slope, void* ws, size_t ws_bytes,
                     sgStream stream);
/* beta is needed to rebuild the pre-activation gamma*z+beta for the fused activation mask */
int sg_batchnorm_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                     const float* save_rstd, float* gx, float* ggamma, float* gbeta, int N, int C, int HW, int training,
                     int act, float slope, void* ws, size_t ws_bytes, sgStream stream);
/* host-only query of the BatchNorm launch plan (sg_batchnorm_fwd / _bwd launch from the same functions): *S statistics slices
 * per channel, *apply_form 1 = per-plane apply kernels, 0 = one thread per element, *stats_two_pass 1 = the statistics kernel
 * reads its (longest) slices twice instead of holding them in registers */
int sg_batchnorm_plan(int N, int C, int HW, int* S, int* apply_form, int* stats_two_pass);
int sg_avgpool3s2_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, sgStream stream);
int sg_avgpool3s2_bwd(const float* gy, float* gx, int NC, int H, int W, int OH, int OW, sgStream stream);
/* nn.MaxPool2d(2, 2) of the VGG19 feature extractor behind VGGLoss (losses.py:179-224; torchvision vgg19.features[4,9,18,27]):
 * y [NC, H/2, W/2]; _bwd routes gy to the first maximum of each window (recomputed from x), zero elsewhere */
int sg_maxpool2_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream);
int sg_maxpool2_bwd(const float* x, const float* gy, float* gx, int NC, int H, int W, sgStream stream);
/* build_cnn's 'P<k>' layers for any window (layers.py:181-189): nn.MaxPool2d(k, k) (avg = 0; _bwd recomputes the first
 * maximum of each window from x) / nn.AvgPool2d(k, k) (avg = 1; x may be null in _bwd).  y [NC, H/k, W/k] */
int sg_pool2d_fwd(const float* x, float* y, int NC, int H, int W, int k, int avg, sgStream stream);
int sg_pool2d_bwd(const float* x, const float* gy, float* gx, int NC, int H, int W, int k, int avg, sgStream stream);
/* nn.ReplicationPad2d(pad) of ResnetBlock(padding_type='replicate') (layers.py:245-246,258-259) and its adjoint (gp is the
 * gradient on the padded grid [NC, H+2pad, W+2pad]; deterministic gather, no atomics) */
int sg_replicate_pad_fwd(const float* x, float* y, int NC, int H, int W, int pad, sgStream stream);
int sg_replicate_pad_bwd(const float* gp, float* gx, int NC, int H, int W, int pad, sgStream stream);
int sg_gap_fwd(const float* x, float* y, int NC, int HW, sgStream stream);
int sg_gap_bwd(const float* gy, float* gx, int NC, int HW, sgStream stream);
int sg_upsample2_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream);   /* nearest x2 */
int sg_reflect_pad_fwd(const float* x, float* y, int NC, int H, int W, int pad, sgStream stream);
int sg_concat_channels(const float* a, const float* b, float* out, int N, int Ca, int Cb, int HW, sgStream stream);
/* Conv over [x1 || cond row expanded over the grid] with the broadcast source folded into a per-(n, m, tap) term
 * (MultiscaleMaskDiscriminator.singleD_forward, discriminators.py:107-110: cat([feat, cond.expand(...)], 1) -> Conv2d):
 *   y = conv(x1, W[:, :C1]) + sum_{taps inside the plane at (oh, ow)} P[n][m][tap],  P = cond x W2r^T (sg_linear_fwd).
 * split_w: W [M][C1+C2][R] -> W1 [M][C1][R], W2r [M*R][C2];  merge_w: its adjoint (a NULL source reads as zeros);
 * bias_act: y[NM][OH][OW] = act(y + window sum of P[NM][KS*KS]) in place;  window_sums: its adjoint, gP[NM][KS*KS] (KS 1, 3, 4) */
int sg_cond_conv_split_w(const float* w, float* w1, float* w2r, int M, int C1, int C2, int R, sgStream stream);
int sg_cond_conv_merge_w(const float* gw1, const float* gw2r, float* gw, int M, int C1, int C2, int R, sgStream stream);
int sg_cond_conv_bias_act(float* y, const float* p, int NM, int OH, int OW, int H, int W, int KS, int stride, int pad,
                          int act, float slope, sgStream stream);
int sg_cond_conv_window_sums(const float* g, float* gp, int NM, int OH, int OW, int H, int W, int KS, int stride, int pad,
                             sgStream stream);

/* ---------------------------------------------------------------------------------------------
 * Layout scatter and bilinear crops (layout.py:64-155, bilinear.py:67-130)
 * ------------------------------------------------------------------------------------------- */
/* grid_sample geometry of the bilinear operators below (masks_to_layout, crop_bbox): 0 (default) = align_corners=False,
 * what torch >= 1.3 executes for the reference's calls (layout.py:51,86,88; bilinear.py:130); 1 = align_corners=True, the
 * default of the PyTorch 1.0 the reference was written for (requirements.txt:8) -- needed to run its released checkpoints
 * with the geometry they were trained with.  Process-wide switch (the second piece of global state next to the profiler). */
int sg_set_legacy_align_corners(int on);
int sg_get_legacy_align_corners(void);
/* seg_off[N+1] from a sorted, gap-free obj_to_img */
int sg_segment_offsets(const int64_t* obj_to_img, int O, int N, int32_t* seg_off, sgStream stream);
/* out[n,d,h,w] = sum_{o in image n, ascending} vecs[o,d] * bilinear(mask_o, box_o)(h,w)   (align_corners=False,
 * zeros padding); masks int64 0/1 (gt) or fp32 (predicted); never materialises (O,D,H,W). */
int sg_masks_to_layout_fwd(const float* vecs, const float* boxes, const void* masks, int masks_i64,
                           const int32_t* seg_off, float* out, int N, int O, int D, int M, int H, int W, int avg,
                           int max_per_image /* hint: objects per image the LDS tile is provisioned for; 0 = default */,
                           sgStream stream);
/* test-mode compositing (layout.py:87-92,157-169): per image, objects are visited in ascending mass
 * (sum over d,h,w of vecs[o,d]*sampled_mask_o[h,w]; ties by index) and a pixel takes vecs[o]*sampled_mask_o of the
 * first visited object whose sampled mask exceeds 0.5 (zero if none).  Inference only: no backward. */
size_t sg_masks_to_layout_test_ws_bytes(int O);
int sg_masks_to_layout_test_fwd(const float* vecs, const float* boxes, const void* masks, int masks_i64,
                                const int32_t* seg_off, float* out, void* ws, size_t ws_bytes, int N, int O, int D, int M,
                                int H, int W, int avg, sgStream stream);
/* The FACTORED form of the test-mode compositing: every pixel belongs to at most one object, so the layout is
 * vecs[winner(p)] * value(p).  Same inputs, visiting order and arithmetic as sg_masks_to_layout_test_fwd (vecs are needed for the
 * masses only); instead of the D channels it writes
 *   Z [N, J, H, W]    Z[n, j, p] = value(p) if j == plane_idx[winner(p)] else 0   (EVERY element is written: no fill needed)
 *   winner [N, H, W]  int32 global object index, -1 where no object's sampled mask exceeds 0.5
 *   value [N, H, W]   the winner's sampled mask (divided by the image's object count under avg), 0 where nobody wins; may be null
 * plane_idx [O]: the plane (0 <= plane < J) of every object inside its image.  vecs[winner] * value is bit-identical to the
 * output of sg_masks_to_layout_test_fwd.  ws >= sg_masks_to_layout_test_planes_ws_bytes(O).  Inference only. */
size_t sg_masks_to_layout_test_planes_ws_bytes(int O);
int sg_masks_to_layout_test_planes(const float* vecs, const float* boxes, const void* masks, int masks_i64,
                                   const int32_t* seg_off, const int64_t* plane_idx, float* Z, int32_t* winner, float* value,
                                   void* ws, size_t ws_bytes, int N, int O, int D, int J, int M, int H, int W, int avg,
                                   sgStream stream);
/* imagenet_deprocess_batch (data/utils.py:17-51) on the device.  imgs (N, C, H, W) fp32 -> out_f32 (N, C, H, W) in [0, 255] and / or
 * out_u8 (N, H, W, C) uint8 (either may be null, not both).  In IEEE fp32, in this order: y = x / 2 + 0.5; with rescale, per image
 * over all channels lo = min y, hi = max y, y = (y - lo) / (hi - lo); v = clamp(y * 255, 0, 255); uint8 = (uint8)(v + 0.5f).
 * A constant image under rescale (hi == lo) gives NaN in out_f32, as the reference does, and 0 in out_u8; so does a NaN input.
 * ws >= sg_deprocess_images_ws_bytes(N, H, W) when rescale != 0 (per-(image, chunk) min / max partials); N <= 65535. */
size_t sg_deprocess_images_ws_bytes(int N, int H, int W);
int sg_deprocess_images(const float* imgs, float* out_f32, uint8_t* out_u8, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                        int rescale, sgStream stream);
/* The label map of a test-mode layout as a picture (scripts/sample_images.py:156-160) without the dense layout:
 * rgb[n, e, p] = colors[objs[winner[n, p]], e] * value[n, p] (0 where winner < 0), then the whole batch times 255 / (its maximum).
 * winner / value as written by sg_masks_to_layout_test_planes, objs [O] int64 class ids, colors [num_colors, 3] fp32,
 * rgb [N, 3, H, W] fp32.  An all-zero batch gives NaN, as the reference's 0 * (255 / 0) does.  ws >= sg_layout_rgb_ws_bytes. */
size_t sg_layout_rgb_ws_bytes(int N, int H, int W);
int sg_layout_rgb(const int32_t* winner, const float* value, const int64_t* objs, const float* colors, float* rgb, void* ws,
                  size_t ws_bytes, int N, int O, int num_colors, int H, int W, sgStream stream);
/* ---- segmented k-means for the appearance bank (kmeans.hip; scene_generation_amd/bank.py) -----------------------------------
 * Many independent k-means problems in one launch.  x [P, D] fp32 with every class's rows contiguous, offsets [C + 1] int32 (CSR).
 * Every per-problem array has a leading restart dimension R (R = 1: none): centers [R, C, K, D], labels / mind2 [R, P], the
 * per-class arrays [R, C].  Class c uses the first k_c = min(n_c, K) rows of its block of centers; a class without rows does no
 * work.  Supported: 1 <= D <= SG_KMEANS_MAX_D, 1 <= K <= SG_KMEANS_MAX_K, R <= 65535, P * R < 2^31 (checked, rc -1).
 * tiles [T, 2] int32 = (class, first row relative to the class's start) cuts every class into pieces of at most SG_KMEANS_TILE rows,
 * ascending per class; tile_off [C + 1] = CSR of the tiles per class.  Results of a class depend on the class's own rows only and
 * are bit-identical from run to run (no floating-point atomics).
 * state [R, C] (may be null: every class runs): 0 running, 1 finished, 2 converged, final pass outstanding.  With final_pass = 0
 * the classes with state != 0 are skipped; with final_pass = 1 those with state == 1 are. */
#define SG_KMEANS_MAX_D 128
#define SG_KMEANS_MAX_K 256
#define SG_KMEANS_TILE 1024
/* labels[i] = argmin_j |x_i - c_j|^2 over the class's k_c centres (a tie: the lowest j), mind2[i] = that distance (direct form, fp32).
 * ADDS to changed [R, C] the number of rows whose label differs from the one found in labels, and to acount [R, C, K] the rows per
 * centre (integer atomics); sg_kmeans_update clears both. */
int sg_kmeans_assign(const float* x, const int32_t* offsets, const int32_t* tiles, const float* centers, const int32_t* state,
                     int32_t* labels, float* mind2, int32_t* changed, int32_t* acount, int P, int C, int K, int D, int R, int T,
                     int final_pass, sgStream stream);
/* centers[c, j] = mean of the class's rows labelled j (a centre without rows keeps its value), counts [R, C, K], inertia [R, C] =
 * sum of mind2, shift [R, C] = sum of squared centre movement; n_iter [R, C] += 1; state: 1 if changed == 0, else 2 if k_c == 1 or
 * shift <= tolvar[c] (tolvar [C], may be null), else 0; changed and acount (either may be null) are cleared.  final_pass = 1:
 * counts and inertia only, state = 1.  ws >= sg_kmeans_update_ws_bytes(T, K, D, R). */
size_t sg_kmeans_update_ws_bytes(int T, int K, int D, int R);
int sg_kmeans_update(const float* x, const int32_t* offsets, const int32_t* tiles, const int32_t* tile_off, const int32_t* labels,
                     const float* mind2, float* centers, int32_t* counts, float* inertia, float* shift, const float* tolvar,
                     int32_t* state, int32_t* n_iter, int32_t* changed, int32_t* acount, void* ws, size_t ws_bytes, int P, int C,
                     int K, int D, int R, int T, int final_pass, sgStream stream);
/* Empty clusters, between assign and update: per centre of a running class with acount == 0 (ascending), the class's row with the
 * largest mind2 (a tie: the lowest row) among the rows whose centre holds more than one row takes that centre's label. */
int sg_kmeans_relocate(const int32_t* offsets, const int32_t* state, int32_t* labels, const float* mind2, const int32_t* acount,
                       int P, int C, int K, int R, sgStream stream);
/* Round ``round`` of k-means++ seeding (one trial per round) for every class with round < k_c: round 0 picks row floor(u * n_c);
 * round t updates mind2 with the centre of round t - 1 and picks the first row whose running sum of mind2 exceeds u * total (a row
 * at distance zero from a chosen centre is never picked).  u [R, C, K] fp32 in [0, 1); the picked row goes to centers[c, round]
 * and its class-relative index to picks [R, C, K].  ws >= sg_kmeans_pp_step_ws_bytes(T, R) (the tiles' sums). */
size_t sg_kmeans_pp_step_ws_bytes(int T, int R);
int sg_kmeans_pp_step(const float* x, const int32_t* offsets, const int32_t* tiles, const int32_t* tile_off, const float* u,
                      float* centers, float* mind2, int32_t* picks, void* ws, size_t ws_bytes, int P, int C, int K, int D, int R,
                      int T, int round, sgStream stream);
/* ---- scene graphs from layouts (scenegraph.hip; scene_generation_amd/scenegraph.py) ------------------------------------------
 * What CocoSceneGraphDataset.__getitem__ derives from a layout in Python loops (data/coco.py:323-416), as launches over the
 * collated batch: boxes [O, 4] fp32 (x0, y0, x1, y1), masks [O, M, M] int64 (masks_i64 = 1; an element is set when == 1) or
 * fp32 (set when > 0.5f), centers [O, 2] fp32.  Every decision is an exact function of fp32 inputs; the only sums are integer
 * sums, so results do not depend on any order and are bit-identical from run to run.  Predicates in the vocabulary order of
 * coco.py:18,206: 0 __in_image__, 1 left of, 2 right of, 3 above, 4 below, 5 inside, 6 surrounding. */
#define SG_SCENEGRAPH_MAX_M 256
#define SG_SCENEGRAPH_MAX_P 64
/* coco.py:326-341: the mean of the box's linspace coordinates over the set mask elements.  count[o] = number of set elements;
 * with Sx / Sy the sums of the set elements' column / row indices, in fp64 from the fp32 box and rounded to fp32 once:
 *   cx = x0 + (x1 - x0) * Sx / (count * (M - 1)),  cy likewise;  count == 0: the fp32 box centre 0.5f * (x0 + x1)
 *   (coco.py:335-337);  M == 1: (x0, y0), the start of a one-step torch.linspace.  1 <= M <= SG_SCENEGRAPH_MAX_M. */
int sg_object_centers(const float* boxes, const void* masks, int masks_i64, float* centers, int32_t* count, int O, int M,
                      sgStream stream);
/* coco.py:296-297,347-348 (and the __image__ row of coco.py:315, model.py:246-249, which needs no special case), in fp64 with
 * round-half-to-even like Python's round():
 *   size_idx = clamp(rint((S - 1) * double(x1 - x0) * double(y1 - y0)), 0, S - 1)   (the differences taken in fp32)
 *   loc_idx  = clamp(rint(double(cx) * (g - 1)), 0, g - 1) + g * clamp(rint(double(cy) * (g - 1)), 0, g - 1)
 * onehot [O, S + g * g] fp32 (may be null): every element is written. */
int sg_object_attributes(const float* boxes, const float* centers, int32_t* size_idx, int32_t* loc_idx, float* onehot, int O,
                         int S, int g, sgStream stream);
/* coco.py:368-385 for T (subject, object) pairs of global object ids: surrounding, else inside (strict comparisons of the boxes),
 * else the angle class of the centre difference (dx, dy) in fp32 -- as comparisons that equal the reference's math.atan2
 * thresholds: dx < 0 && |dy| <= |dx| left of, else dy < 0 && |dy| > |dx| above, else dy > 0 && |dy| >= |dx| below, else right
 * of.  Element t of s / o is read at s[t * idx_stride], p is written at p[t * p_stride] (1, 1: plain arrays; 3, 3 with
 * s = triples, o = triples + 2, p = triples + 1: the columns of a [T, 3] array).  An id outside [0, O) gives p = -1. */
int sg_pair_predicates(const float* boxes, const float* centers, const int64_t* s, const int64_t* o, int idx_stride, int64_t* p,
                       int p_stride, int T, int O, sgStream stream);
/* The random partner draw of coco.py:358-366 and the collate order of coco.py:406-413,501-547, driven by a table of uniforms.
 * Image n owns the objects seg_off[n] .. seg_off[n + 1] - 1, the last of which is its __image__ object, and the triples
 * tri_off[n] .. tri_off[n + 1] - 1.  With k = its number of real objects, every real object i (ascending) draws r partners,
 *   j = min(int(double(u[o, q, 0]) * (k - 1)), k - 2), j += (j >= i);  subject = i if u[o, q, 1] > 0.5f else j   (o = seg_off[n] + i)
 * with the derived predicate (sg_pair_predicates); then the k triples (i, 0, last).  k < 2: only those (coco.py:359-361), so
 * tri_off[n + 1] - tri_off[n] must be k + (k >= 2 ? k * r : 0) (an image whose count differs is left unwritten).  u [O, r, 2]
 * fp32 in [0, 1), triples [T, 3] / triple_to_img [T] int64 with T = tri_off[N]. */
int sg_draw_pairs(const int32_t* seg_off, const int32_t* tri_off, const float* u, const float* boxes, const float* centers,
                  int64_t* triples, int64_t* triple_to_img, int N, int O, int T, int r, sgStream stream);
/* How many triples a layout honours: ADDS to counts [P, 2] int64 (the caller zeroes it once; integer atomics), for every triple
 * with 1 <= p < P, counts[p, 0] += 1 and counts[p, 1] += (the predicate derived as in sg_pair_predicates == p).  Row 0 and
 * triples with ids outside [0, O) are left alone.  P <= SG_SCENEGRAPH_MAX_P. */
int sg_triple_agreement(const int64_t* triples, const float* boxes, const float* centers, int64_t* counts, int T, int O, int P,
                        sgStream stream);
/* The same for the attribute block attrs [O, S + g * g] fp32 (a bit is set when > 0.5f): ADDS to counts [2, 2] int64
 * counts[0, 0] += objects whose size block has exactly one bit set, counts[0, 1] += those whose bit is size_idx[o];
 * counts[1, :] likewise for the location block and loc_idx.  Rows without a set bit count for nothing. */
int sg_attribute_agreement(const float* attrs, const int32_t* size_idx, const int32_t* loc_idx, int64_t* counts, int O, int S,
                           int g, sgStream stream);
/* ---- size and location attributes from class statistics (attributes.hip; scene_generation_amd/attributes.py) --------------------
 * The two ends of the reference's attribute sampler: the per-class counts of scripts/create_attributes_file.py and the draw of
 * --sample_attributes (data/coco_panoptic.py:336-340,389-391,432-449,468-521).  All integers.  S = size_len, g = grid side (cell =
 * col + g * row), A = S + g * g; predicates as above, opposites 1<->2, 3<->4, 5<->6; class image_class is the __image__ object.
 *
 * Statistics: counts [C, A] int64.  A row of attrs [O, A] fp32 contributes its FIRST set bit (> 0.5f) of the size block and of the
 * location block, independently; a block without a bit contributes nothing.  Rows of class image_class
 * (create_attributes_file.py:127) and of classes outside [0, C) are skipped.  The call ADDS (integer atomics: exact whatever the
 * order), so a dataset is accumulated batch by batch. */
int sg_attribute_histogram(const int64_t* objs, const float* attrs, int64_t* counts, int O, int C, int S, int g, int image_class,
                           sgStream stream);
/* draw(w, allowed, u) over int64 weights w_c = hist_c * allowed_c: if their sum is 0 (a class never seen, or never seen in the
 * allowed cells; a class outside [0, C) counts as never seen) w_c = allowed_c; with t = double(u) * double(sum) the result is the
 * smallest c whose inclusive prefix sum, converted to double, is > t.  Exact and independent of evaluation order.  u [O, 2] fp32 in
 * [0, 1) (clamped to [0, 1 - 2^-24]): column 0 is object o's size draw, column 1 its location draw, each used at most once, so an
 * image's result does not depend on its place in the batch.  Image n owns the objects with obj_to_img == n and the triples with
 * triple_to_img == n (both vectors sorted ascending; the ranges are found by binary search).  Per image, in this order:
 *  1. a real object whose size block of ``given`` [O, A] (may be null) holds a bit keeps its first one, else
 *     size = draw(size_hist[class], all, u[o, 0]); a given location bit counts as set from the start.  Given bits never change.
 *  2. the __image__ object gets size S - 1 and the cell c + g * c, c = rint(0.5 * (g - 1)) (ties to even), unless given.
 *  3. the image's triples (s, p, o) in stored order; skipped when p is outside 1..6, s == o, either end is an __image__ object or
 *     lies outside the image.  For each kept one step(s, p, o), then step(o, opposite(p), s).
 *  4. step(a, q, b): loc[a] set: nothing.  loc[b] unset: loc[a] = draw(loc_hist[class a], all, u[a, 1]).  loc[b] set and q inside /
 *     surrounding: loc[a] = loc[b] and, unless a's size was given, the size rule below.  loc[b] set and q in 1..4:
 *     loc[a] = draw(loc_hist[class a], allowed(q, loc[b]), u[a, 1]) with (col_b, row_b) of loc[b]:
 *       left of: col <= max(col_b - 1, 0)       right of: col >= min(col_b + 1, g - 1)
 *       above:   row <= max(row_b - 1, 0)       below:    row >= min(row_b + 1, g - 1)
 *  5. real objects that still have no location draw one unrestricted.
 * Size rule SG_ATTR_RULE_REFERENCE (coco_panoptic.py:478-489 as written; the surrounding object becomes the smaller one):
 *     surrounding: size_b <= size_a -> size_a = max(0, size_b - 1);   inside: size_b >= size_a -> size_a = min(S - 1, size_b + 1)
 * SG_ATTR_RULE_GEOMETRIC (the evident intent):
 *     surrounding: size_a <= size_b -> size_a = min(S - 1, size_b + 1);   inside: size_a >= size_b -> size_a = max(0, size_b - 1)
 * One wavefront per image, one lane per cell: 1 <= S <= 64 and g * g <= 64 (else an error before any launch).  Every element of
 * size_idx [O] / loc_idx [O] int32 and attrs [O, A] fp32 (the one-hot block) is written: -1 and no bit where nothing was assigned
 * (objects of no image in [0, N), and the objects past the first SG_ATTR_MAX_OBJS of an image, whose triples are skipped).
 * SG_ATTR_MAX_OBJS: 13 bytes of LDS per object, 13 KB per wavefront, which leaves twelve images resident per CU. */
#define SG_ATTR_MAX_OBJS 1024
#define SG_ATTR_RULE_REFERENCE 0
#define SG_ATTR_RULE_GEOMETRIC 1
int sg_sample_attributes(const int64_t* objs, const int64_t* obj_to_img, const int64_t* triples, const int64_t* triple_to_img,
                         const int64_t* counts, const float* u, const float* given, int32_t* size_idx, int32_t* loc_idx, float* attrs,
                         int N, int O, int T, int C, int S, int g, int image_class, int size_rule, sgStream stream);
/* ---- the object-accuracy classifier (classifier.hip; scene_generation_amd/accuracy.py) ------------------------------------------
 * What a torchvision ResNet (scripts/train_accuracy_net.py:62-101) needs beyond the entry points above.  No float atomics: every
 * result is bit-identical from run to run.  Base pointers may be unaligned (16-byte loads are used only where they allow it).
 *
 * nn.MaxPool2d(3, stride=2, padding=1) on [NC, H, W] with OH = (H - 1) / 2 + 1, OW likewise.  Padding counts as -inf; a NaN in
 * a window wins.  A window's winner is the element torch's scan keeps (rows, then columns, taking a value when it is greater than
 * the running maximum or a NaN): the first maximum in scan order.  _bwd is a gather that recomputes the winners from x (no saved
 * indices): gx[pixel] = sum of gy over the at most four windows the pixel won, in (oh, ow) order.  NC * H * W < 2^31. */
int sg_maxpool3s2_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, sgStream stream);
int sg_maxpool3s2_bwd(const float* x, const float* gy, float* gx, int NC, int H, int W, int OH, int OW, sgStream stream);
/* y = max(a + b, 0) (a NaN stays a NaN): the tail relu(bn(...) + identity) of a residual block.  Its backward is sg_act_bwd
 * (SG_ACT_RELU) on y; the result is the gradient of both operands. */
int sg_add_relu_fwd(const float* a, const float* b, float* y, int64_t n, sgStream stream);
/* An eval-mode BatchNorm folded into the convolution before it: s = gamma / sqrt(var + eps), w_out[co, k] = w[co, k] * s[co]
 * (w as [Cout, K], K = Cin * KS * KS), b_out[co] = beta[co] - mean[co] * s[co].  Cout <= 65535. */
int sg_bn_fold(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* w_out,
               float* b_out, int Cout, int K, sgStream stream);
/* torch.optim.SGD(lr, momentum) without dampening, Nesterov or weight decay over one flat buffer; the gradient enters as
 * g * grad_scale.  first != 0: buf = g (buf is not read); else buf = momentum * buf + g; then p = p - lr * buf.  Every product and
 * every sum is rounded on its own (no fused multiply-add), like torch's sequence of separate operations. */
int sg_sgd_momentum_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, int first, float grad_scale,
                         sgStream stream);
/* torch.max(logits, 1) per row of logits [rows, classes] -- the first index of the maximum, a NaN counting as the maximum -- written
 * to preds [rows] int64 when non-null, and the record acc [3] int64 = {correct, counted, rows}, which the call ADDS to (integer
 * atomics; the caller zeroes it once): a row counts when target[row] != ignore_label and is correct when it counts and its argmax
 * equals its target (scripts/sample_images.py:233-239 with ignore_label = 0); ignore_label = -1 counts every row. */
int sg_classify_stats(const float* logits, const int64_t* target, int rows, int classes, int64_t ignore_label, int64_t* preds,
                      int64_t* acc, sgStream stream);
/* ---- the Inception score (inception.hip; scene_generation_amd/inception.py) ----------------------------------------------------------
 * What torchvision's Inception-v3 and scripts/inception_score.py need beyond the entry points above.  Forward only, fp32 (the score
 * in fp64).  No wrapper synchronises; no float atomics: every result is bit-identical from run to run.  Base pointers may be
 * unaligned (the convolution takes 16-byte loads of the weights only when they allow it).
 *
 * sg_conv2d_rect_fwd: y[n, out_c0 + co, oh, ow] = act(sum_{c, kh, kw} x[n, c, oh * stride - padH + kh, ow * stride - padW + kw] *
 * w[co, c, kh, kw] + bias[co]) with x [N, C, H, W], w [Cout, C, KH, KW], bias [Cout] or NULL, y [N, out_ctot, OH, OW]: the channels
 * outside [out_c0, out_c0 + Cout) are not touched (the branches of an Inception block write their slices of one tensor).  Zero
 * padding, 0 <= pad < kernel extent; stride 1 or 2; KH * KW <= 25; OH = (H + 2 padH - KH) / stride + 1, OW likewise; act is
 * SG_ACT_NONE or SG_ACT_RELU.  An implicit GEMM on the fp32 matrix cores over K = C * KH * KW.  ws >= sg_conv2d_rect_ws_bytes(d)
 * (0 unless the plan splits K; the slabs of a split are added in ascending k order).
 * sg_conv2d_rect_plan (host only): the launch plan of a desc -- tile (SG_RECT_TILE_*) of bm output channels x bn pixels, vec (16-byte
 * weight loads: K % 4 == 0 and w_aligned16), splits k-chunks of kchunk elements each (1: no split, kchunk = K). */
typedef struct sgRectDesc {
  int32_t N, C, H, W, Cout, KH, KW, stride, padH, padW, OH, OW;
  int32_t out_c0, out_ctot;
} sgRectDesc;
enum { SG_RECT_TILE_64X64 = 1, SG_RECT_TILE_32X128 = 2, SG_RECT_TILE_64X128 = 3 };
typedef struct sgRectPlan {
  int32_t tile, bm, bn, vec, splits, kchunk;
} sgRectPlan;
int sg_conv2d_rect_plan(const sgRectDesc* d, int w_aligned16, sgRectPlan* plan);
size_t sg_conv2d_rect_ws_bytes(const sgRectDesc* d);
int sg_conv2d_rect_fwd(const sgRectDesc* d, const float* x, const float* w, const float* bias, float* y, int act, void* ws,
                       size_t ws_bytes, sgStream stream);
/* max_pool2d(3, stride=2) WITHOUT padding (sg_maxpool3s2_* pads by 1): x [N, C, H, W] -> y[n, out_c0 + c, oh, ow] of
 * y [N, out_ctot, OH, OW], OH = (H - 3) / 2 + 1, OW likewise; H, W >= 3.  A NaN in a window wins, as in torch. */
int sg_maxpool3s2v_fwd(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, int out_c0, int out_ctot,
                       sgStream stream);
/* avg_pool2d(3, stride=1, padding=1) with count_include_pad=True (sg_avgpool3s2_* excludes the padding) on [NC, H, W]: the taps
 * inside the plane are added in (kh, kw) order -- rows, then columns -- starting from 0, and the sum is divided by 9 everywhere. */
int sg_avgpool3s1_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream);
/* F.interpolate(mode='bilinear', align_corners=False) of [NC, H, W] to [NC, OH, OW]: src = (dst + 0.5) * in / out - 0.5, clamped
 * below at 0; taps floor(src) and floor(src) + 1, the upper one clamped to the last row / column. */
int sg_resize_bilinear_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, sgStream stream);
/* softmax over the classes of logits [rows, classes] (the row maximum subtracted), written to rows [row0, row0 + rows) of
 * out [capacity, classes]; the other rows are not touched. */
int sg_softmax_rows(const float* logits, int rows, int classes, float* out, int row0, int capacity, sgStream stream);
/* scripts/inception_score.py:48-62 on probs [n, classes] fp32: out (fp64 [2 + splits], 8-byte aligned) = {mean, std, score_0, ...}.
 * Part k = rows [k * (n / splits), (k + 1) * (n / splits)) (the tail rows are dropped); py = the part's column mean; per row
 * KL = sum_j ph log(ph / qh) with ph = p / sum(p), qh = py / sum(py) (scipy.stats.entropy normalises both; a term with p = 0 is
 * 0); score_k = exp(mean KL); mean and POPULATION std over the splits.  Every sum in fp64 in a fixed order.  n / splits == 0
 * gives NaN for both.  ws >= sg_inception_score_ws_bytes(n, classes, splits), 8-byte aligned. */
size_t sg_inception_score_ws_bytes(int n, int classes, int splits);
int sg_inception_score(const float* probs, int n, int classes, int splits, void* out, void* ws, size_t ws_bytes, sgStream stream);
/* The FID form of the network (pytorch-fid's FIDInceptionA / C / E_1 and E_2) needs two more pools on [NC, H, W]:
 * sg_avgpool3s1x_fwd: avg_pool2d(3, stride=1, padding=1, count_include_pad=False) -- the taps of sg_avgpool3s1_fwd in the same
 * (kh, kw) order from 0, divided by the number of taps inside the plane.
 * sg_maxpool3s1_fwd: max_pool2d(3, stride=1, padding=1) -- the taps inside the plane scanned in (kh, kw) order from -inf; a NaN in
 * a window wins, as in the other max-pools. */
int sg_avgpool3s1x_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream);
int sg_maxpool3s1_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream);
/* ---- the Frechet Inception Distance (fid.hip; scene_generation_amd/fid.py) ---------------------------------------------------------
 * The float64 raw moments of feature rows, accumulated on the device over a whole evaluation.
 *
 * sg_fid_moments_update: sum[j] += sum_k x[k][j] and outer[i][j] += sum_k x[k][i] * x[k][j] for i <= j, with x fp32 [rows, D] of row
 * stride ldx >= D elements (any 4-byte aligned base), sum fp64 [D], outer fp64 [D, D] (both 8-byte aligned, zeroed by the caller
 * before the first call).  The lower triangle of outer is unspecified until finalize (whole 64 x 64 diagonal tiles are written).
 * Each fp32 value is converted to fp64, so every product is exact; the sums are fp64 on the f64 matrix cores
 * (v_mfma_f64_16x16x4_f64), k ascending, the call's total added to the stored value once.  One workgroup per tile pair of the block
 * upper triangle, no atomics: the same call sequence gives bit-identical moments.  rows == 0 returns 0 and launches nothing.  A null
 * pointer, D < 1, ldx < D or a misaligned fp64 pointer returns a negative code (sg_last_error_string) and launches nothing.  The call
 * never synchronises and never allocates.  Raw moments, no shift: two accumulators merge by adding counts, sums and outers.
 *
 * sg_fid_moments_finalize: mu = sum / n and the full symmetric sigma[i][j] = sigma[j][i] = (outer[i][j] - sum[i] * sum[j] / n) /
 * (n - 1) read from i <= j only -- numpy.cov(rowvar=False), ddof = 1; sigma equals its transpose bit for bit.  mu fp64 [D], sigma
 * fp64 [D, D], distinct from sum and outer.  n < 2 returns a negative code. */
int sg_fid_moments_update(const float* x, int rows, int D, int ldx, double* sum, double* outer, sgStream stream);
int sg_fid_moments_finalize(const double* sum, const double* outer, long long n, int D, double* mu, double* sigma, sgStream stream);
/* ---- the diversity score: LPIPS on AlexNet / VGG-16 (lpips.hip; scene_generation_amd/lpips.py) ------------------------------------------
 * Forward, and the data gradient of the distance for LPIPS as a loss.  No wrapper synchronises or allocates (the wide convolution keeps its k-split table in the plan cache like every
 * gather); no float atomics: the same calls give bit-identical results.  Base pointers of fp32 operands may be unaligned.  A bad
 * argument returns a negative code (sg_last_error_string) and launches nothing.
 *
 * sg_conv2d_wide_fwd / _plan / _ws_bytes: the contract, descriptor, plan struct and output-slice semantics of sg_conv2d_rect_*, for
 * KH, KW <= 11 (up to 121 taps) and stride 1..4 -- AlexNet's 11 x 11 stride-4 stem.  The same implicit GEMM on the fp32 matrix cores
 * over K = C * KH * KW (k ascending), zero padding, bias + SG_ACT_NONE / SG_ACT_RELU in the epilogue.  The plan's tile is always
 * SG_RECT_TILE_64X64: the 121-tap LDS table of a 64-pixel tile leaves room for three workgroups per compute unit, that of a 128-pixel
 * tile for one. */
int sg_conv2d_wide_plan(const sgRectDesc* d, int w_aligned16, sgRectPlan* plan);
size_t sg_conv2d_wide_ws_bytes(const sgRectDesc* d);
int sg_conv2d_wide_fwd(const sgRectDesc* d, const float* x, const float* w, const float* bias, float* y, int act, void* ws,
                       size_t ws_bytes, sgStream stream);
/* The scaling layer of LPIPS: y[n, c, i] = (v - shift[c]) / scale[c] with shift = (-.030, -.088, -.188), scale = (.458, .448, .450),
 * x [N, 3, HW] -- or, x_nhwc != 0, [N, HW, 3], the pictures a sampler hands out -- fp32 in [-1, 1] (v = x) or, x_uint8 != 0, uint8
 * (v = x / 127.5 - 1); y fp32 [N, 3, HW].  Each operation is rounded to fp32 on its own (no fused multiply-add, no reciprocal). */
int sg_lpips_input(const void* x, int x_uint8, int x_nhwc, int N, int HW, float* y, sgStream stream);
/* One tap of the LPIPS distance.  f0, f1 fp32 [P, C, HW] (the two halves of one 2P forward; they may be the same pointer), w fp32 [C]
 * (>= 0; NULL: all ones), out fp64 [P], 8-byte aligned: out[p] (accumulate != 0: +)= mean over the HW pixels of
 *   s = sum_c w[c] * (f0_c / (n0 + eps) - f1_c / (n1 + eps))^2,   n = sqrt(sum_c f_c^2) per side,
 * in the direct form (normalise, then difference) in fp32, both sides by the same code in the same order, so f0 == f1 gives exactly
 * 0.0; a pixel of all zeros contributes 0 / (0 + eps) = 0.  The spatial sum is fp64 in a fixed order.  Every feature element is read
 * from memory once for C <= 512.  ws >= sg_lpips_layer_ws_bytes(P, C, HW), 8-byte aligned (0 when a pair's pixels fit one workgroup:
 * one launch; two otherwise).  P == 0 returns 0 and launches nothing. */
size_t sg_lpips_layer_ws_bytes(int P, int C, int HW);
int sg_lpips_layer(const float* f0, const float* f1, const float* w, int P, int C, int HW, float eps, double* out, int accumulate,
                   void* ws, size_t ws_bytes, sgStream stream);
/* The gradient of one tap with respect to f0 (LPIPS as a training loss; f1 is the detached target).  gout fp64 [P] on the device,
 * 8-byte aligned, = dL / d out[p]; gf0 fp32 [P, C, HW], every element written exactly once (overwritten).  With n0, s0 = n0 + eps, t_c
 * as above:
 *   g_c = 2 w[c] t_c (float)(gout[p] / HW),   dot = sum_c g_c f0_c,   gf0_k = g_k / s0 - (f0_k / s0) * ((dot / s0) / n0)
 * in fp32, ordered so that no intermediate leaves the fp32 range while n0 is a normal float.  t_c is the forward's, by the same code:
 * f0 == f1 bit for bit gives gf0 == +0 everywhere.  A pixel with n0 == 0 gets the finite g_k / s0 (the second term is defined as 0
 * there; eps > 0 assumed), where autograd of the formula gives NaN from the derivative of sqrt at 0: every tap is a ReLU output, a
 * pixel of all zeros has every pre-activation <= 0, and the ReLU backward drops the value (torch's by selection, sg_act_bwd by the
 * factor 0: the value has to be finite).  Two reads and one write of
 * the feature map, no workspace, no atomics, fixed-order sums: bit-identical from run to run.  P == 0 returns 0 and launches
 * nothing. */
int sg_lpips_layer_bwd(const float* f0, const float* f1, const float* w, const double* gout, int P, int C, int HW, float eps,
                       float* gf0, sgStream stream);
/* The backward of sg_lpips_input for fp32 [N, 3, HW] pictures: gx[n, c, i] = gy[n, c, i] / scale[c], one correctly rounded division. */
int sg_lpips_input_bwd(const float* gy, int N, int HW, float* gx, sgStream stream);
/* ---- statistics of all pairs of feature rows (featsets.hip; scene_generation_amd/featsets.py) --------------------------------------------
 * The Kernel Inception Distance's kernel sums and the k-NN manifold estimate (improved precision / recall, density / coverage).  Feature
 * rows are fp32 [rows, D] with a row stride >= D elements (any 4-byte aligned base).  Every dot product is formed in fp64 from the
 * converted fp32 operands on the f64 matrix cores (v_mfma_f64_16x16x4_f64), k ascending: the products are exact and only the sums
 * round.  d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b) with the norms computed in fp64 by the same unit.  No floating-point atomics:
 * partial results go to ws and are combined in a fixed order; counts are integer atomics and minima are integer atomic minima of
 * the bit patterns of non-negative doubles -- the same call gives bit-identical output.  No call synchronises or allocates.  ws is
 * 8-byte aligned and at least the matching _ws_bytes; fp64 operands are 8-byte, int operands 4-byte aligned.  A null or misaligned
 * pointer, a size < 1, a row stride < D or a k / degree out of range returns a negative code (sg_last_error_string) and launches
 * nothing; zero work (S == 0; n == 0; n == 0 or m == 0) returns 0 without looking at the pointers and writes nothing.
 *
 * sg_feat_poly_sums: x [n, D], y [m, D]; ix, iy int32 [S, s] device tables of row numbers (ix into x, iy into y); out fp64 [S, 3]:
 *   out[q] = ( sum_{i != j} k(x_ix[q,i], x_ix[q,j]),  sum_{i != j} k(y_iy[q,i], y_iy[q,j]),  sum_{i, j} k(x_ix[q,i], y_iy[q,j]) )
 * with k(a, b) = (gamma a.b + coef0)^degree by repeated multiplication, degree in 1..4; i != j is by position in the subset.  Rows
 * are gathered through the tables in the operand loader: no gathered copy and no s x s matrix is written.  An index outside its set
 * reads as a zero row (no address is formed from it).  The symmetric sums run over tile pairs ti <= tj with off-diagonal tiles
 * doubled.
 *
 * sg_feat_knn_radius: r2[i] = the k-th smallest of { d2(x_i, x_j) : j != i } (exclusion by index: duplicate rows count), fp64 [n],
 * 1 <= k <= 8, k < n.  The columns are split over workgroups and the partial lists merged by a second kernel.
 *
 * sg_feat_manifold_counts: references a [n, D] with their radii r2 [n], queries b [m, D]:
 *   count[j] = #{ i : d2(b_j, a_i) <= r2[i] }  (int32 [m]),    mind2[i] = min_j d2(a_i, b_j)  (fp64 [n]);
 * both are initialised by the call. */
size_t sg_feat_poly_sums_ws_bytes(int S, int s);
int sg_feat_poly_sums(const float* x, int n, int ldx, const float* y, int m, int ldy, int D, const int* ix, const int* iy, int S, int s,
                      double gamma, double coef0, int degree, double* out, void* ws, size_t ws_bytes, sgStream stream);
size_t sg_feat_knn_radius_ws_bytes(int n);
int sg_feat_knn_radius(const float* x, int n, int D, int ldx, int k, double* r2, void* ws, size_t ws_bytes, sgStream stream);
size_t sg_feat_manifold_counts_ws_bytes(int n, int m);
int sg_feat_manifold_counts(const float* a, int n, int lda, const double* r2, const float* b, int m, int ldb, int D, int* count,
                            double* mind2, void* ws, size_t ws_bytes, sgStream stream);
/* ---- Pillow-exact antialiased resize of a ragged batch of uint8 RGB images (imageprep.hip; scene_generation_amd/imageprep.py) -----------
 * ``Image.resize((OW, OH), BILINEAR | BICUBIC)`` of Pillow on 8-bit RGB, bit for bit (no ``box``, no ``reducing_gap``), with the
 * loader's ToTensor + Normalize(0.5, 0.5) fused in as a table lookup.
 *
 * The arithmetic, per axis, with S = 1 (bilinear) or 2 (bicubic), in float64 with every operation rounded once (no fma contraction):
 *   scale = in / out, fs = max(scale, 1), support = S fs; for output index xx: center = (xx + 0.5) scale,
 *   xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in), tap x in [0, xmax - xmin) has weight
 *   w = f((x + xmin - center + 0.5) (1 / fs)), f(t) = 1 - |t| below 1 (bilinear); with a = -0.5, ((a + 2)|t| - (a + 3)) |t| |t| + 1 below 1
 *   and (((|t| - 5)|t| + 8)|t| - 4) a below 2 (bicubic); 0 beyond.  ww = the sum of w in tap order from 0.0; w / ww when ww != 0; the
 *   coefficient is k = (int)(0.5 + w 2^22) for w >= 0 and (int)(-0.5 + w 2^22) below, (int) truncating toward zero.
 *   An output byte is clip((2^21 + sum_j pixel[xmin + j] k[j]) >> 22, 0, 255), the sum in int32.
 * The horizontal pass [H, W] -> [H, OW] runs first and is rounded to uint8, the vertical pass [H, OW] -> [OH, OW] follows; a pass whose
 * input and output length are equal is skipped (the identity).  The tap count 2 ceil(support) + 1 is whatever the sizes imply (32 769
 * for 16384 -> 1 bicubic): it is never capped.
 *
 * Limits: 1 <= H, W <= SG_PIL_MAX_IN; 1 <= OH, OW <= SG_PIL_MAX_OUT; N <= SG_PIL_MAX_IMAGES; at most 2^31 - 1 groups of 8 source rows.
 *
 * sg_pil_resize_plan (HOST only; nothing is launched): desc_host int64 [N][3] rows (byte offset, H, W) of images stored as tight
 * [H][W][3] bytes in a buffer of packed_bytes bytes -- offsets are arbitrary (no alignment), every image must lie inside the buffer
 * (a negative code otherwise).  Writes table_host int64 [N + 1][SG_PIL_TABLE_COLS] -- per image {offset, H, W, coefficient offset of
 * the horizontal and of the vertical pass (-1: skipped), their tap strides, offset of the [H, OW, 3] intermediate (-1: none), first
 * horizontal workgroup}; row N holds the workgroup total: the prefix the horizontal pass searches -- and totals_host int64 [4] =
 * {coef_ints, inter_bytes, hblocks, workspace bytes}.
 *
 * sg_pil_resize: packed uint8 (device, 4-byte aligned base), table = the plan's table uploaded as it is (8-byte aligned), coef_ints /
 * inter_bytes / hblocks its totals; lut fp32 [256] (device): the value of y for each byte (the caller builds it with the loader's own
 * expression, so y is bitwise the loader's); y8 uint8 [N, OH, OW, 3] and / or y fp32 [N, 3, OH, OW] (either may be null, not both);
 * ws 16-byte aligned and at least totals[3] bytes: the coefficients, then the ragged intermediates.  Three launches on ``stream``
 * (coefficients of every (image, axis, output index) computed on the device from the table; horizontal; vertical), fewer when every
 * image skips a pass.  ``phases`` = SG_PIL_ALL; a subset of its bits issues only those launches, for timing them one by one (the
 * workspace must then hold what the omitted ones would have written).  No call synchronises or allocates; N == 0 returns 0 and
 * launches nothing.  The horizontal pass stages SG_PIL_LDS_CHUNK bytes of a source row in LDS at once and
 * walks longer tap spans chunk by chunk. */
enum { SG_PIL_BILINEAR = 0, SG_PIL_BICUBIC = 1 };
enum { SG_PIL_COEF = 1, SG_PIL_HORIZONTAL = 2, SG_PIL_VERTICAL = 4, SG_PIL_ALL = 7 };
#define SG_PIL_MAX_IN 16384
#define SG_PIL_MAX_OUT 4096
#define SG_PIL_MAX_IMAGES 65536
#define SG_PIL_TABLE_COLS 9
#define SG_PIL_LDS_CHUNK 4096
int sg_pil_resize_plan(const int64_t* desc_host, int N, int64_t packed_bytes, int OH, int OW, int filter, int64_t* table_host,
                       int64_t* totals_host);
int sg_pil_resize(const void* packed, int64_t packed_bytes, const int64_t* table, int N, int OH, int OW, int filter, int64_t coef_ints,
                  int64_t inter_bytes, int64_t hblocks, const float* lut, void* y8, float* y, void* ws, size_t ws_bytes, int phases,
                  sgStream stream);
/* ---- FID-infinity: every subset's FID from two Gram matrices (fidinf.hip; scene_generation_amd/fidinf.py) --------------------------------
 * For n < D fake rows the Frechet distance of a subset S to fixed real statistics (mu, sigma) needs no D x D matrix: with
 * Z = X - 1 mu^T, P = Z Z^T and G = Z sigma Z^T (both n x n), |mean_S - mu|^2 and tr Sigma_S are sums over P_SS, and the non-zero
 * eigenvalues of sigma Sigma_S are those of H G_SS H / (n_S - 1), H = I - 1 1^T / n_S.  Neither call synchronises or allocates; no
 * atomics: every sum has one owner and a fixed order, so the same call gives bit-identical output.  A null pointer, a size outside the
 * ranges below, ldx < D, a misaligned pointer (fp64 operands and ws 8-byte, x and the int tables 4-byte) or a workspace below the
 * matching _ws_bytes returns a negative code (sg_last_error_string) and launches nothing.
 *
 * sg_fidinf_grams: x fp32 [n, D] of row stride ldx >= D elements (any 4-byte aligned base), n >= 2, D >= 1; mu fp64 [D]; sigma fp64
 * [D, D], read as given (no symmetry is assumed); P, G fp64 [n, n], written completely.
 *   Z[i][k] = fl64((double)x[i][k] - mu[k])            (one rounding; kept in ws)
 *   Y[i][c] = sum_l Z[i][l] sigma[l][c]                (kept in ws)
 *   P[i][j] = sum_k Z[i][k] Z[j][k],   G[i][j] = sum_k Y[i][k] Z[j][k]
 * Every sum is fp64 on the f64 matrix cores (v_mfma_f64_16x16x4_f64) in ascending k from 0.0.  P and G are computed for the 64 x 64
 * tile pairs ti <= tj only -- inside a diagonal tile for i <= j only -- and each value is stored at (i, j) and (j, i): both equal
 * their transposes bit for bit.  ws >= sg_fidinf_grams_ws_bytes(n, D) = 16 n D bytes.
 *
 * sg_fidinf_subset_terms: P, G fp64 [n, n] as above (G symmetric bit for bit), n >= 2; idx int32 [S, smax] (device): row q holds
 * sizes[q] row numbers in [0, n), the rest of the row is not read; sizes int32 [S] (device), each in 2 .. smax; smax >= 2; S >= 0
 * (S == 0 returns 0 without looking at the pointers).  With t_i = idx[q][i], n_q = sizes[q] and all sums over i, j < n_q:
 *   sums[q] = ( sum_i P[t_i][t_i],  sum_ij P[t_i][t_j] )                                        fp64 [S, 2]
 *   r_i = sum_j G[t_i][t_j],   t = sum_i r_i
 *   M[q][i][j] = ((G[t_i][t_j] - (r_i + r_j) / n_q) + t / (n_q n_q)) / (n_q - 1)                fp64 [S, smax, smax], row stride smax
 * A row sum is taken by one wave (lane l adds j = l, l + 64, ... in ascending order, then a butterfly over the lanes), a total by one
 * workgroup in the same manner: fixed orders.  M[q]'s leading n_q x n_q block equals its transpose bit for bit; no entry outside that
 * block is written (subsets are ragged: a tile that straddles n_q writes its inside part only).  The wrapper validates the tables on the
 * host; the kernels form no address from an entry outside [0, n) (it reads as a zero row and column) and clamp a size to [0, smax]
 * (below 2: sums[q] is NaN and M[q] is not written).  ws >= sg_fidinf_subset_terms_ws_bytes(S, smax) = 8 (3 S smax + S) bytes. */
size_t sg_fidinf_grams_ws_bytes(int n, int D);
int sg_fidinf_grams(const float* x, int n, int D, int ldx, const double* mu, const double* sigma, double* P, double* G, void* ws,
                    size_t ws_bytes, sgStream stream);
size_t sg_fidinf_subset_terms_ws_bytes(int S, int smax);
int sg_fidinf_subset_terms(const double* P, const double* G, int n, const int* idx, const int* sizes, int S, int smax, double* M,
                           double* sums, void* ws, size_t ws_bytes, sgStream stream);
/* ---- IS-infinity: the Inception score of every subset of the stored softmax rows (isinf.hip; scene_generation_amd/isinf.py) ------------
 * The definition is that of sg_inception_score with one split, so a subset of all rows in identity order reproduces that score up to
 * the order of the sums.  With p the stored fp32 row, s_i = sum_j (double)p_ij and ph_ij = (double)p_ij / s_i:
 *   h_i = sum_j ph_ij log ph_ij                         a term whose ph is not > 0 is 0: a row of sum 0 contributes nothing
 * and for a subset of n_q rows t_i = idx[q][i], all sums over i < n_q:
 *   q_j = sum_i (double)p[t_i][j],   qh_j = q_j / sum_j q_j,   mh_j = (sum_i ph[t_i][j]) / n_q      (a ph that is not > 0 adds 0)
 *   log score_q = (sum_i h[t_i]) / n_q - sum_j mh_j log qh_j                                        a term whose mh_j is not > 0 is 0
 * Every sum is fp64 in a fixed order and there are no floating-point atomics, so the same call gives bit-identical output.  Neither
 * call synchronises or allocates.  A null pointer, a misaligned one (fp64 operands and ws 8-byte, probs and the int tables 4-byte),
 * n < 1, classes < 1, ldp < classes, S < 0, smax < 2 or a workspace below sg_isinf_subset_scores_ws_bytes returns a negative code
 * (sg_last_error_string) and launches nothing.
 *
 * sg_isinf_row_terms: probs fp32 [n, classes] of row stride ldp >= classes elements (any 4-byte aligned base); writes rs[i] = s_i and
 * h[i], fp64 [n], in one pass over the rows: a wave per row, lane l adds the classes l, l + 64, ... in ascending order, then a
 * butterfly over the lanes.
 *
 * sg_isinf_subset_scores: probs, rs, h as above; idx int32 [S, smax] (device): row q holds sizes[q] row numbers, the rest of the row is
 * not read; sizes int32 [S] (device) -- the layout of fidinf.draw_subsets; smax >= 2; S >= 0 (S == 0 returns 0 without looking at the
 * pointers).  out fp64 [S, 2] = {log score_q, score_q = exp of it}.  The rows are gathered through the table in the loader (there is
 * no gathered copy).  A subset's positions are cut into chunks of SG_ISINF_ROWS_PER_WG; one workgroup per (subset, chunk, tile of 1024
 * classes) adds the chunk's rows in ascending position, a thread per 4 adjacent classes (one 16-byte load per row when probs is
 * 16-byte aligned and ldp a multiple of 4, 4-byte loads otherwise -- the same sums in the same order either way), and writes the
 * partial q_j, the partial sum of ph and the chunk's sum of h (lane l adds the positions l, l + 64, ..., then a butterfly) to ws; one
 * finishing workgroup per subset adds the partials in ascending chunk order and forms the two numbers.  The wrapper validates the
 * tables on the host; the kernels form no address from an entry outside [0, n) (it reads as a row that contributes nothing) and
 * clamp a size to [0, smax]; below 2 both outputs are NaN.
 * ws >= sg_isinf_subset_scores_ws_bytes(S, smax, classes) = 8 S (ceil(smax / SG_ISINF_ROWS_PER_WG) + 1) (2 classes + 1) bytes. */
#define SG_ISINF_ROWS_PER_WG 64
int sg_isinf_row_terms(const float* probs, int n, int classes, int ldp, double* rs, double* h, sgStream stream);
size_t sg_isinf_subset_scores_ws_bytes(int S, int smax, int classes);
int sg_isinf_subset_scores(const float* probs, int n, int classes, int ldp, const double* rs, const double* h, const int* idx,
                           const int* sizes, int S, int smax, double* out, void* ws, size_t ws_bytes, sgStream stream);
/* ---- quasi-random inputs of the generator: scrambled Sobol points on the device (qmc.hip; scene_generation_amd/qmc.py) -----------------
 * One image's randomness -- its mask-noise row, one appearance-bank pick per object, two attribute uniforms per object -- read off ONE
 * point of a digitally shifted Sobol sequence of D = noise_dim + 3 * max_objects dimensions.  Everything below is integer arithmetic
 * but the inverse normal CDF, every output element has one owner, there are no atomics: a call repeats bit for bit.  No call
 * synchronises or allocates.  A bad argument returns one of the negative codes below (sg_last_error_string) and launches nothing:
 *   SG_QMC_ERR_NULL  a null pointer        SG_QMC_ERR_DIMS  D (noise_dim, max_objects, rep, C) outside its range
 *   SG_QMC_ERR_LD    a row stride below D  SG_QMC_ERR_RANGE first < 0 or first + n > 2^SG_QMC_MAXBIT
 *   SG_QMC_ERR_COUNT a negative count, or one beyond the launch grid
 * (counts are checked first, then the dimensions, the stride, the range and last the pointers).
 *
 * sg_sobol_points: out[i][d] int32, i < n, d < D, row stride ld >= D elements (columns D .. ld - 1 are not written) = the
 * SG_QMC_MAXBIT-bit integer state of point number k = first + i in dimension d,
 *   x(i, d) = shift[d] ^ XOR over the set bits b of g of dirs[d][b],   g = k ^ (k >> 1)
 * -- the closed form of the Gray-code recurrence of torch.quasirandom.SobolEngine, whose ``sobolstate`` [D][30] and ``shift`` [D] are
 * dirs and shift (int32, values below 2^30); x * 2^-30 is the point in [0, 1).  Point 0 is ``shift`` itself.  1 <= D <=
 * SG_QMC_MAX_DIMS, first >= 0, n >= 0, first + n <= 2^30; n == 0 returns 0 without looking at the pointers.  A workgroup owns one
 * point and 128 dimensions, so the walk over the bits of g is uniform across it.
 *
 * sg_qmc_unpack: the N points [N][ld] of a batch -> the three tables a forward consumes, one launch.  obj_to_img [O] int64 sorted
 * ascending, seg_off [N + 1] int32 (sg_segment_offsets); object o of image n = obj_to_img[o] sits in slot j = o - seg_off[n] and owns
 * the columns c = noise_dim + 3 j + {0, 1, 2}; ld >= noise_dim + 3 * max_objects, noise_dim >= 0, max_objects >= 0, not both 0.
 *   noise [N][noise_dim] fp32 = (float)normcdfinv(((double)x + 0.5) * 2^-30): the centre of the cell, so every value is finite
 *                               (x = 0 and x = 2^30 - 1 give -+6.1208...)
 *   pick  [O] int32           = x(n, c + 0), the raw 30-bit integer (sg_bank_draw scales it)
 *   u     [O][2] fp32         = (x >> 6) * 2^-24 of the columns c + 1, c + 2: exact in fp32 and below 1 (the contract of
 *                               sg_sample_attributes' u)
 * An object whose image is outside [0, N) or whose slot is outside [0, max_objects) gets pick = -1 and u = 0.
 *
 * sg_bank_draw: bank [R][rep] fp32, the rows of all classes back to back; class_off [C + 1] int64; objs [O] int64; pick [O] int32.
 * With c = objs[o] and rows_c = class_off[c + 1] - class_off[c]:
 *   idx = ((int64)pick[o] * rows_c) >> 30     (exact; idx < rows_c because pick < 2^30)
 *   row_idx[o] = idx,  rows[o][:] = bank[class_off[c] + idx][:]
 * An object with c outside [0, C), rows_c <= 0, pick outside [0, 2^30) or a source row outside [0, R) gets row_idx = -1 and a row
 * of zeros; no address is formed from such an entry.  rep >= 1, C >= 1, R >= 0.  Rows are contiguous, so a load wider than 4 bytes
 * is aligned in every row only if its width divides rep: the copy runs on the widest of 16 / 8 / 4 bytes that divides 4 * rep and
 * both base addresses, which leaves no tail. */
#define SG_QMC_MAXBIT 30
#define SG_QMC_MAX_DIMS 21201
#define SG_QMC_ERR_NULL (-3)
#define SG_QMC_ERR_DIMS (-4)
#define SG_QMC_ERR_LD (-5)
#define SG_QMC_ERR_RANGE (-6)
#define SG_QMC_ERR_COUNT (-7)
int sg_sobol_points(const int32_t* dirs, const int32_t* shift, int32_t* out, int64_t first, int64_t n, int D, int ld, sgStream stream);
int sg_qmc_unpack(const int32_t* points, int ld, const int64_t* obj_to_img, const int32_t* seg_off, float* noise, int32_t* pick,
                  float* u, int N, int O, int noise_dim, int max_objects, sgStream stream);
int sg_bank_draw(const float* bank, const int64_t* class_off, const int64_t* objs, const int32_t* pick, int32_t* row_idx,
                 float* rows, int O, int C, int rep, int64_t R, sgStream stream);
/* g_vecs[o, d] for d in [d_begin, D) (columns below d_begin are zero-filled) */
int sg_masks_to_layout_bwd_vecs(const float* gout, const float* boxes, const void* masks, int masks_i64,
                                const int64_t* obj_to_img, const int32_t* seg_off, float* g_vecs, int N, int O, int D,
                                int M, int H, int W, int avg, int d_begin, sgStream stream);
/* gradients of masks_to_layout w.r.t. the masks (float masks only) and / or the boxes (layout.py:85-86 is differentiable in
 * both): g_masks [O, M, M], g_boxes [O, 4] (either may be null); ws >= sg_masks_to_layout_bwd_geom_ws_bytes (O x H x W
 * floats: the per-object gradient map sum_d gout[n,d] * vecs[o,d]); gather formulation, deterministic */
size_t sg_masks_to_layout_bwd_geom_ws_bytes(int O, int H, int W);
int sg_masks_to_layout_bwd_geom(const float* gout, const float* vecs, const float* boxes, const void* masks, int masks_i64,
                                const int64_t* obj_to_img, const int32_t* seg_off, float* g_masks, float* g_boxes, void* ws,
                                size_t ws_bytes, int N, int O, int D, int M, int H, int W, int avg, sgStream stream);
int sg_crop_bbox_fwd(const float* feats, const float* boxes, const int64_t* box_to_feat, float* out, int N, int C, int H,
                     int W, int B, int HH, int WW, sgStream stream);
/* g_feats [N, C, H, W] is written completely (no zero fill needed; all zero for B = 0): a gather over the crop pixels whose
 * bilinear footprint covers each image pixel, summed in (box, crop row, crop column) order => bit-reproducible */
int sg_crop_bbox_bwd(const float* gout, const float* boxes, const int64_t* box_to_feat, float* g_feats, int N, int C,
                     int H, int W, int B, int HH, int WW, sgStream stream);
/* crop_bbox(feats, bbox, HH, WW, backend='jj') (bilinear.py:101-130 with bilinear_sample, bilinear.py:188-243): one box per
 * image, pixel coordinate X * W without the half-pixel shift, floor / floor + 1 taps clamped to the plane.  No caller of the
 * reference reaches this sampler (crop_bbox_batch never forwards its backend); _bwd = the gradient w.r.t. feats, deterministic. */
int sg_crop_bbox_jj_fwd(const float* feats, const float* boxes, float* out, int N, int C, int H, int W, int HH, int WW,
                        sgStream stream);
int sg_crop_bbox_jj_bwd(const float* gout, const float* boxes, float* g_feats, int N, int C, int H, int W, int HH, int WW,
                        sgStream stream);
/* Per-image filters of the factored layout convs: layout = sum_o [one_hot(class_o) | repr_o] (x) S_o (model.py:165-168,
 * layout.py:85-86) => conv(layout | x2, w)[n] = sum_j wimg[n][:, j] (*) plane_j with
 *   wimg[n][m][j][t] = w[m][class_o][t] + sum_d repr[o][d] w[m][C + d][t]   for the j-th object o of image n (j < cnt_n)
 *                    = w[m][C + R + (j - cnt_n)][t]                         for the C2 channels of the second source
 * w [M][C + R + C2][KS2], repr [O][R], objs [O] class ids, seg_off [N + 1] object offsets per image, wimg [N][M][L][KS2].
 * _bwd: gw [M][C + R + C2][KS2] (written completely) and / or grepr [O][R] from gwimg; sums in index order. */
int sg_factored_weights_fwd(const float* w, const float* repr, const int64_t* objs, const int32_t* seg_off, float* wimg,
                            int N, int O, int M, int L, int KS2, int C, int R, int C2, sgStream stream);
int sg_factored_weights_bwd(const float* gwimg, const float* w, const float* repr, const int64_t* objs,
                            const int32_t* seg_off, const int64_t* img_idx, float* gw, float* grepr, int N, int O, int M,
                            int L, int KS2, int C, int R, int C2, sgStream stream);
/* VectorPool.query on device (utils.py:62-90): plan = int32[4][O] rows {class, src_kind, src_idx, slot}
 * out[i] = src_kind ? pool[class][src_idx] : vectors[src_idx]; then pool[class][slot] = vectors[i] (slot>=0) */
int sg_vector_pool_exchange(float* pool, const float* vectors, const int32_t* plan, float* out, int O, int R,
                            int pool_size, sgStream stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (losses.py:26-90,135-175; trainer.py:215,331-340; discriminators.py:35) and Adam (trainer.py:60,80,106,133)
 * ------------------------------------------------------------------------------------------- */
size_t sg_loss_ws_bytes(int64_t n);
/* out[0] (+)= scale * sum_i l(a_i, b_i or target); deterministic two-stage reduction */
int sg_loss_fwd(int kind, const float* a, const float* b, float target, int64_t n, float scale, float* out,
                int accumulate, void* ws, size_t ws_bytes, sgStream stream);
/* ga_i = gout[0] * scale * dl/da_i */
int sg_loss_bwd(int kind, const float* a, const float* b, float target, int64_t n, float scale, const float* gout,
                float* ga, sgStream stream);
/* Several scalar losses of ONE kind and their weighted sum, one launch forward and one backward:
 *   out[0] = sum_t weight[t] * (scale[t] * sum_i l(a_t[i], b_t[i] | target[t])),   t < nterms <= SG_WSUM_MAX
 * -- the feature-matching L1 terms of calculate_features_loss (trainer.py:331-340), the per-scale terms of GANLoss
 * (losses.py:166-172), the five VGG terms (losses.py:220-224).  Same arithmetic in the same order as sg_loss_fwd per term
 * followed by sg_weighted_sum_fwd (bit-identical).  *_host = HOST arrays of nterms entries (a / b / ga: device pointers;
 * b_host, target_host may be NULL; a NULL ga entry skips that term's gradient); terms_out (optional): the nterms scaled
 * terms.  _bwd: ga_t[i] = weight[t] * gout[0] * scale[t] * dl/da. */
size_t sg_multi_loss_ws_bytes(int nterms);
int sg_multi_loss_fwd(int kind, int nterms, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                      const float* scale_host, const float* weight_host, const float* target_host, float* out,
                      float* terms_out, void* ws, size_t ws_bytes, sgStream stream);
int sg_multi_loss_bwd(int kind, int nterms, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                      const float* scale_host, const float* weight_host, const float* target_host, const float* gout,
                      void* const* ga_host, sgStream stream);
/* mean over rows of -log softmax(logits)[target]; per-row loss kept in row_loss[rows] */
int sg_cross_entropy_fwd(const float* logits, const int64_t* target, int rows, int classes, float* row_loss,
                         float* out, sgStream stream);
int sg_cross_entropy_bwd(const float* logits, const int64_t* target, int rows, int classes, const float* gout,
                         float* glogits, sgStream stream);
/* torch.optim.Adam step (no weight decay / amsgrad) over one flat fp32 buffer.  The gradient enters as g * grad_scale:
 * 1 on one GPU; 1 / world under data parallelism, where g holds the all-reduced SUM (the mean's scaling pass over the flat
 * gradient buffer -- 8 B per parameter -- is folded into this kernel's read) */
int sg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                 float eps, float bias_corr1, float bias_corr2_sqrt, float grad_scale, sgStream stream);
/* sg_adam_step, then the parameter EMA on the updated value: e = e + ema_w * (p_new - e), as fmaf(ema_w, p_new - e, e); ema_w == 1
 * writes e = p_new exactly.  p / m / v are bitwise those of sg_adam_step.  36 B per parameter (profile kind SG_K_ADAM).
 * 0 <= ema_w <= 1; e has the layout of p. */
int sg_adam_step_ema(float* p, const float* g, float* m, float* v, float* e, int64_t n, float lr, float beta1, float beta2,
                     float eps, float bias_corr1, float bias_corr2_sqrt, float grad_scale, float ema_w, sgStream stream);
/* the same EMA expression alone, for parameter runs the Adam step skips: e = ema_w == 1 ? p : fmaf(ema_w, p - e, e) */
int sg_ema_update(float* e, const float* p, int64_t n, float ema_w, sgStream stream);
/* Gradient control of the fused Adam step: global-norm clipping and a skip-on-non-finite guard that never leave the device.
 * The record lives in caller-owned DEVICE memory, 8-byte aligned, 32 bytes, zeroed once by the caller; only the kernels below
 * write it afterwards.  Byte offsets:
 *    0 sumsq   (double)  sum of squares of the raw buffer g
 *    8 norm    (float)   |grad_scale| * sqrt(sumsq), computed in double, rounded once
 *   12 coef    (float)   the factor the _ctl Adam launches multiply grad_scale by
 *   16 skip    (int32)   1 when norm is not finite (NaN / inf in g, or a norm beyond fp32), else 0
 *   20 skipped (int32)   calls that set skip  (only ever incremented)
 *   24 steps   (int32)   calls                (only ever incremented)
 *   28 reserved */
typedef struct sgGradCtl {
  double sumsq;
  float norm, coef;
  int32_t skip, skipped, steps, reserved;
} sgGradCtl;
/* One streaming read of g (4 B per element, profile kind SG_K_GRAD_NORM) fills the record: squares and sums in float64 (an fp32
 * square is exact there) in a FIXED order -- per-workgroup partials in ws, one finishing launch, no floating-point atomics: the
 * same bits on every call and every stream.  coef = (float)min(1, max_norm / (norm_double + 1e-6)), the expression of
 * torch.nn.utils.clip_grad_norm_; max_norm <= 0 or +inf: no clipping, coef = 1.  A non-finite norm sets skip = 1, coef = 1 and
 * increments skipped.  g may start at any 4-byte aligned element.  ws: sg_grad_norm_ws_bytes(n) bytes, 8-byte aligned. */
size_t sg_grad_norm_ws_bytes(int64_t n);
int sg_grad_norm(const float* g, int64_t n, float grad_scale, float max_norm, void* ctl, void* ws, size_t ws_bytes,
                 sgStream stream);
/* sg_adam_step / sg_adam_step_ema under a record sg_grad_norm filled earlier on the same stream (or one ordered before it): the
 * gradient enters as g * (grad_scale * ctl->coef), the product rounded to fp32 once, so coef == 1 gives the bits of sg_adam_step.
 * With ctl->skip set the Adam part writes nothing (p, m, v keep their bits); the EMA part still moves e toward the unchanged p,
 * as sg_ema_update does for parameters the Adam step skips.  Same traffic as the plain launches (28 / 36 B per parameter). */
int sg_adam_step_ctl(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float bias_corr1, float bias_corr2_sqrt, float grad_scale, const void* ctl, sgStream stream);
int sg_adam_step_ema_ctl(float* p, const float* g, float* m, float* v, float* e, int64_t n, float lr, float beta1, float beta2,
                         float eps, float bias_corr1, float bias_corr2_sqrt, float grad_scale, float ema_w, const void* ctl,
                         sgStream stream);
int sg_fill(float* p, float value, int64_t n, sgStream stream);
int sg_scale(float* p, float alpha, int64_t n, sgStream stream);
/* dst (device) <- src (PAGE-LOCKED host memory, read through its device mapping) by a kernel on ``stream``: how a collated host
 * batch reaches the device (replaces the eight ``tensor.cuda()`` of train.py:192 for batches packed into one page-locked buffer;
 * scene_generation_amd/pipeline.py).  Both pointers 16-byte aligned, nbytes a multiple of 16. */
int sg_stage_copy(void* dst, const void* src_host_mapped, int64_t nbytes, sgStream stream);

/* y += alpha * x : a second gradient contribution to a parameter slice of the flat gradient buffer (the first one is
 * written in place by the weight-gradient kernels; replaces autograd's AccumulateGrad add, trainer.py:262,278,299,324) */
int sg_axpy(float* y, const float* x, float alpha, int64_t n, sgStream stream);
/* y += x ; x = 0 : folds a SPILL gradient buffer into the flat gradient buffer and clears it for the next step.  The k-th
 * (k >= 2) contribution a parameter receives between zero_grad() and step() -- the real / wrong-texture passes of a
 * discriminator, trainer.py:281-325 -- is written by its weight-gradient kernel straight into spill buffer k-2 (same layout as
 * the gradient buffer); one launch per spill buffer and optimiser step replaces one temporary + sg_axpy per parameter and pass */
int sg_add_clear(float* y, float* x, int64_t n, sgStream stream);
/* out = a + b : the shortcut add of build_cnn's 'R' residual blocks (reference layers.py:84-118);
 * out = alpha * a * b : nn.Dropout's mask multiply (layers.py:230, build_mlp(dropout=...)); the mask itself is drawn by the host
 * framework's device RNG.  Neither is on the benchmark path. */
int sg_add(const float* a, const float* b, float* out, int64_t n, sgStream stream);
int sg_mul(const float* a, const float* b, float alpha, float* out, int64_t n, sgStream stream);
/* total_loss = sum_i weight_i * loss_i over <= SG_WSUM_MAX device scalars (LossManager.add_loss, utils.py:50-57, and the
 * scale sums of GANLoss / calculate_features_loss, losses.py:166-172, trainer.py:331-340); terms_host = HOST array of
 * DEVICE pointers, weights_host = HOST array.  _bwd: gterms[i] = weights[i] * gout[0] */
int sg_weighted_sum_fwd(const void* const* terms_host, const float* weights_host, int n, float* out, sgStream stream);
int sg_weighted_sum_bwd(const float* weights_host, int n, const float* gout, float* gterms, sgStream stream);

/* ---------------------------------------------------------------------------------------------
 * Opt-in per-kernel timing with HIP events on the launch stream (bench.py roofline leg).
 * ------------------------------------------------------------------------------------------- */
int sg_prof_enable(int on);
int sg_prof_reset(void);
int sg_prof_num_kinds(void);
const char* sg_prof_kind_name(int kind);
/* synchronises the recorded events; totals since the last reset */
int sg_prof_read(int kind, double* total_ms, int64_t* launches, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SG2IM_HIP_H */
