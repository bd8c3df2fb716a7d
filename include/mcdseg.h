/*
 * mcdseg.h -- C ABI of libmcdseg.so, the MI355X (gfx950) kernels behind the MCD hot path.
 *
 * The reference (LittleWat/multichannel-semseg-with-uda) has no FFI layer: its hot path is a chain
 * of stock ATen operators launched from Python.  Each entry point below replaces one such operator
 * call site (cited as file:line of the reference); the Python host side in
 * multichannel-semseg-with-uda_amd/mcdseg/ binds them with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller;
 *   - tensors are fp32, NCHW, contiguous; labels are int64;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates,
 *     never synchronises; scratch space is passed in by the caller (sizes from the *_bytes /
 *     *_count helpers);
 *   - return value 0 = launched; <0 = rejected (bad argument, unsupported shape, launch error) and
 *     mcdseg_last_error() holds the reason (thread-local string).
 */
#ifndef MCDSEG_H
#define MCDSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations below are exported */
#pragma GCC visibility push(default)

#define MCDSEG_VERSION 101

int mcdseg_version(void);
const char* mcdseg_last_error(void);

/* Data parallelism (mcdseg_allreduce(buf, count, comm, stream) over RCCL): what the reference gets from
 * torch.nn.DataParallel's gradient reduction (/root/reference/models/model_util.py:283-284).  A communicator of the library's own:
 * rank 0 draws an id (mcdseg_comm_unique_id: MCDSEG_COMM_ID_BYTES bytes) and hands it to the other ranks by any means (the host side:
 * a broadcast over the process group it already has), every rank calls mcdseg_comm_init (collective); mcdseg_allreduce sums `count`
 * fp32 values in place over the ranks, enqueued on `stream` -- asynchronous, no host synchronisation, like every other entry point.
 * RCCL is bound at run time (the librccl the process has loaded already -- PyTorch's -- else librccl.so.1 on the loader's path):
 * the library does not link it, and returns -38 (ENOSYS) where there is none.  csrc/comm.hip. */
#define MCDSEG_COMM_ID_BYTES 128
int mcdseg_comm_unique_id(void* id128);
int mcdseg_comm_init(void** comm, int32_t nranks, const void* id128, int32_t rank);
int mcdseg_comm_destroy(void* comm);
int mcdseg_allreduce(float* buf, int64_t count, void* comm, void* stream);

/* Plan / development options (tile choices, launch plans, kernel forms: csrc/options.h lists them with their defaults).  The library
 * never reads the process environment: whoever wants another plan says so through this call.  The table is process-wide (a backward
 * pass runs on other threads than the forward pass that built its graph) and read at every launch; a name may carry the "MCDSEG_"
 * prefix of the environment variable the Python host side translates (mcdseg/_lib.py).  Unknown names are rejected. */
int32_t mcdseg_option_count(void);
const char* mcdseg_option_name(int32_t index);
int mcdseg_set_option(const char* name, int64_t value);
int mcdseg_get_option(const char* name, int64_t* value, int64_t* default_value);

/* ------------------------------------------------------------------------------------------------
 * Convolution  (nn.Conv2d call sites: models/drn.py:21-23,127,177,199; models/dilated_fcn.py:227)
 * groups = 1, square kernel, symmetric stride / padding / dilation.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mcdseg_conv_desc {
  int32_t N, Cin, H, W;      /* input  [N,Cin,H,W]                      */
  int32_t Cout, KH, KW;      /* weight [Cout,Cin,KH,KW]                 */
  int32_t stride, pad, dil;
  int32_t Ho, Wo;            /* output [N,Cout,Ho,Wo]                   */
  int32_t Ncb;               /* split operators: batch size of the tensor the pre-split companions (x_cb / dy_cb) were WRITTEN for,
                              * when this call covers only N of its images (a launch addresses < 2 GiB per operand piece, so larger
                              * tensors are processed in slices along N): the companion layout is [piece][Ncb][C/8][H*W][8], the
                              * pointer passed is that of the slice's first image in piece 0, and piece p of the slice lies
                              * p * Ncb * (C/8) * H*W * 16 bytes behind it.  0 = N (the companion belongs to exactly this batch). */
} mcdseg_conv_desc;

/* Padded GEMM dims of the packed weight images: fprop image is [KH*KW][Kp_f][Mp_f] with M = Cout,
 * K = Cin; dgrad image is [KH*KW][Kp_d][Mp_d] with M = Cin, K = Cout. */
int mcdseg_conv_packed_dims(const mcdseg_conv_desc* d, int32_t* Mp_f, int32_t* Kp_f, int32_t* Mp_d, int32_t* Kp_d);
/* w [Cout,Cin,KH,KW] -> fprop image and/or dgrad image (either destination may be NULL). */
int mcdseg_conv_pack_weights(const mcdseg_conv_desc* d, const float* w, float* wp_fprop, float* wp_dgrad, void* stream);

/* Number of per-channel partial-statistics rows conv_fprop writes (each row is 3*Mp_f floats:
 * count, mean, M2 of one wave's slice of pixels). */
int64_t mcdseg_conv_stat_rows(const mcdseg_conv_desc* d);
/* y = conv(x, w) (+ bias).  If stat_partials != NULL also emits the train-mode BatchNorm partials of y
 * (fused epilogue; nn.BatchNorm2d call sites models/drn.py:34,38,129,179,202). */
int mcdseg_conv_fprop(const mcdseg_conv_desc* d, const float* x, const float* wp_fprop, const float* bias,
                      float* y, float* stat_partials, void* stream);
/* Inference form (eval-mode BatchNorm folded into the epilogue, adapt_tester.py:87-104):
 * y = act(scale[c] * conv(x, w) + shift[c] (+ residual)), act = ReLU if relu != 0.  No bn_apply pass. */
int mcdseg_conv_fprop_affine(const mcdseg_conv_desc* d, const float* x, const float* wp_fprop, const float* scale,
                             const float* shift, const float* residual, int32_t relu, float* y, void* stream);
/* dx = conv_transpose(dy, w)   (autograd of the same call sites) */
int mcdseg_conv_dgrad(const mcdseg_conv_desc* d, const float* dy, const float* wp_dgrad, float* dx, void* stream);
/* ---- split-precision variants: the same operators with the fp32 operands carried through the 16-bit matrix pipe as a
 * sum of exact piece products (csrc/split.h).  `math` selects the arithmetic:
 *   MCDSEG_MATH_F16X3   x = s (h1 + h2): two fp16 pieces and a power-of-two scale s per tensor, three cross terms on
 *                       v_mfma_f32_32x32x16_f16 -- 5.3x the f32 MFMA rate, fp32-grade against the reference's fp64 gradients;
 *   MCDSEG_MATH_BF16X6  x = a1 + a2 + a3: three bf16 pieces, the six largest cross terms on v_mfma_f32_32x32x16_bf16
 *                       (2.67x the f32 MFMA rate; no scale needed).
 * *_bound arguments (F16X3 only, NULL otherwise): one device float holding an UPPER BOUND of |tensor| -- written by the
 * producer of the tensor (mcdseg_bn_stats_finalize, mcdseg_bn_bwd_reduce, mcdseg_conv_split_pack_weights) or measured
 * with mcdseg_absmax; every kernel derives the scale 2^(ceil(log2 bound) - 15) from it, so no finite value overflows fp16.
 * Weight images are 16-bit, layout [k-step][piece][k-half 2][Mp][8]; sizes from *_packed_bytes.
 *   MCDSEG_MATH_F16X1   reduced precision: F16X3's operands (same images, companions, bounds -- every producer treats it as
 *                       F16X3) multiplied with the leading term only, h1 h1': one MFMA instead of three, operands rounded to
 *                       fp16's 11 significant bits.  The thin full-resolution layers' window kernels keep three terms. */
#define MCDSEG_MATH_F16X3 3
#define MCDSEG_MATH_BF16X6 6
#define MCDSEG_MATH_F16X1 1
int mcdseg_conv_split_packed_bytes(const mcdseg_conv_desc* d, int32_t math, int64_t* fprop_bytes, int64_t* dgrad_bytes);
/* 1 when the forward of this geometry runs as the direct (LDS-tiled) convolution of the network stem (7x7, stride 1,
 * pad 3, Cin <= 8, Cout <= 16; models/drn.py:126-131) -- the one case where the split path takes fewer than 16
 * contraction channels (always in the bf16x6 arithmetic).  mcdseg_conv_split_stat_rows = rows of the BN partial-statistics
 * buffer mcdseg_conv_split_fprop writes (differs from mcdseg_conv_stat_rows for the direct kernel). */
int32_t mcdseg_conv_split_direct_ok(const mcdseg_conv_desc* d);
int64_t mcdseg_conv_split_stat_rows(const mcdseg_conv_desc* d);
/* The thin full-resolution 3x3 layers (16 contraction channels, 16 / 32 outputs; models/drn.py:195-205 "_make_conv_layers") run,
 * with MCDSEG_MATH_F16X3 and a pre-split operand, on an LDS-window kernel whose partial-statistics rows differ (one per tile of
 * 8 (4) x 32 pixels and wave): mcdseg_conv_split_stat_rows_for gives the row count mcdseg_conv_split_fprop will write for this
 * (math, x_cb != NULL) combination in a call WITHOUT bias / affine epilogue; mcdseg_conv_split_window_ok tells whether that kernel
 * takes the forward (dgrad = 0) or the data gradient (dgrad = 1, stride 1 only).  It has no bias / affine epilogue: calling
 * mcdseg_conv_split_fprop with a companion AND a bias for such a geometry is rejected -- and so is, with stat_partials, the stem with
 * a companion and a bias, which the direct kernel would run with ITS row count (mcdseg_conv_split_stat_rows).  The entry points and
 * these queries read one route (csrc/conv_gemm_split.hip, conv_route): a query's answer is a field of what the launch switches on. */
int64_t mcdseg_conv_split_stat_rows_for(const mcdseg_conv_desc* d, int32_t math, int32_t presplit);
int32_t mcdseg_conv_split_window_ok(const mcdseg_conv_desc* d, int32_t math, int32_t presplit, int32_t dgrad);
/* Workgroup tile mcdseg_conv_split_fprop / _dgrad take for M output rows (Cout forward, Cin for the data gradient) and P output
 * pixels, as the decimal digits WM WN WAVES_M WAVES_N of conv_gemm_split_kernel<P, WM, WN, WAVES_M, WAVES_N, ...>: 4222 = 256 x 128,
 * 4214 = 128 x 256, 2222 = 128 x 128, 2214 = 64 x 256, 1214 = 32 x 256 (rows x pixels).  For profilers and the benchmark's
 * per-kernel accounting; never needed to call the operators. */
int32_t mcdseg_conv_split_tile_config(int32_t M, int64_t P, int32_t presplit);
/* bound[0] = max |x[i]| (exact, order-independent; non-finite data gives a non-finite bound) */
int mcdseg_absmax(const float* x, int64_t n, float* bound, void* stream);
/* w [Cout,Cin,KH,KW] -> fprop and/or dgrad image; F16X3 first measures w_bound = max |w| (device float, written here) */
int mcdseg_conv_split_pack_weights(const mcdseg_conv_desc* d, int32_t math, const float* w, void* wp_fprop, void* wp_dgrad,
                                   float* w_bound, void* stream);
/* The same for n convolutions in two launches (every image of a model after an optimizer step).  Device tables: ptrs[4*e ..] =
 * {w, wp_fprop or 0, wp_dgrad or 0, &bounds[e]} as 64-bit addresses, dims[4*e ..] = {Cout, Cin, KH*KW, 0}; bounds: n device
 * floats, written here (F16X3; may be NULL for BF16X6, the table's bound addresses are then ignored).  The stem's direct-kernel
 * forward image is not produced by this call (pass 0 for it and use mcdseg_conv_split_pack_weights). */
int mcdseg_conv_split_pack_weights_multi(const int64_t* ptrs, const int32_t* dims, int32_t n, int32_t math, float* bounds,
                                         void* stream);
/* x_cb / dy_cb (may be NULL): the gathered operand already split by its producer into the channel-blocked layout
 * [piece][N][C/8][H*W][8 x 16 bit] (mcdseg_bn_apply_cb / mcdseg_bn_bwd_apply_cb / mcdseg_split_cb, same `math` and the same
 * bound scalar); C must be divisible by 8.  With it the K loop does no conversion and moves 16 B per piece, pixel and
 * 8-channel group straight into LDS instead of gathering 8 dwords and splitting them. */
int mcdseg_conv_split_fprop(const mcdseg_conv_desc* d, int32_t math, const float* x, const void* x_cb, const float* x_bound,
                            const void* wp_fprop, const float* w_bound, const float* bias, float* y, float* stat_partials,
                            void* stream);
int mcdseg_conv_split_fprop_affine(const mcdseg_conv_desc* d, int32_t math, const float* x, const void* x_cb, const float* x_bound,
                                   const void* wp_fprop, const float* w_bound, const float* scale, const float* shift,
                                   const float* residual, int32_t relu, float* y, void* stream);
int mcdseg_conv_split_dgrad(const mcdseg_conv_desc* d, int32_t math, const float* dy, const void* dy_cb, const float* dy_bound,
                            const void* wp_dgrad, const float* w_bound, float* dx, void* stream);
/* dx = data gradient + addend: the element-wise add autograd performs when the convolution's input has a second consumer (the
 * shortcut of a residual block: models/drn.py:43-59 BasicBlock, :79-100 Bottleneck), folded into the epilogue -- same sum, same
 * order, same bits; 80 such adds per MCD step at BASELINE config 2.  `addend`: fp32, dx's shape, not dx itself.  `part` as in
 * mcdseg_conv_split_dgrad_part.  Not for geometries of the thin-layer window kernel (mcdseg_conv_split_window_ok(d, math, 1, 1)). */
int mcdseg_conv_split_dgrad_add(const mcdseg_conv_desc* d, int32_t math, const float* dy, const void* dy_cb, const float* dy_bound,
                                const void* wp_dgrad, const float* w_bound, const float* addend, float* dx, int32_t part, void* stream);
/* One convolution may run as TWO launches: whole rounds of 256 x 256 tiles (one per CU) on the 8-wave ping-pong kernel
 * (csrc/conv_gemm_split_pp.hip), the remaining pixels on the 4-wave tiles.  mcdseg_conv_split_parts returns the number of output
 * pixels (a multiple of 256, counted from pixel 0 of the flattened (n, y, x) order) the first launch takes -- 0 when the geometry
 * runs as one launch.  The _part entry points are mcdseg_conv_split_fprop / _dgrad with `part` = 0 (the whole convolution, what
 * those do), 1 (only the ping-pong launch) or 2 (only the rest); parts 1 + 2 write exactly what part 0 writes.  They exist so that
 * a profiler or bench.py can bracket each kernel with its own HIP events.  Reference: nn.Conv2d, models/drn.py:21-23. */
int64_t mcdseg_conv_split_parts(const mcdseg_conv_desc* d, int32_t math, int32_t presplit, int32_t dgrad);
/* 1 when "the rest" (part 2; the whole convolution when mcdseg_conv_split_parts returns 0) runs on the ping-pong kernel's 256 x 128
 * tile, 0 when it runs on the 4-wave tiles -- the kernel name a profiler will see. */
int32_t mcdseg_conv_split_rest_pingpong(const mcdseg_conv_desc* d, int32_t math, int32_t presplit, int32_t dgrad);
/* 1 (2: its 128 x 320 form, for output rows that are a multiple of 128 only; 3: its 256 x 160 form, where only 160-pixel tiles fill
 * their rounds -- partial rows of 160 pixels as well, one per tile) when the WHOLE convolution runs as one launch of the
 * ping-pong kernel's 256 x 320 tile (chosen when fewer than two rounds of
 * 256 x 256 tiles exist but tiles 320 pixels wide fill their rounds to 80 %: 76800 pixels x 256 channels = 240 tiles on 256 CUs);
 * mcdseg_conv_split_parts then returns every pixel, and the BatchNorm partial rows are one per 160 pixels
 * (mcdseg_conv_split_stat_rows_for counts them). */
int32_t mcdseg_conv_split_wide_pingpong(const mcdseg_conv_desc* d, int32_t math, int32_t presplit, int32_t dgrad);
int mcdseg_conv_split_fprop_part(const mcdseg_conv_desc* d, int32_t math, const float* x, const void* x_cb, const float* x_bound,
                                 const void* wp_fprop, const float* w_bound, const float* bias, float* y, float* stat_partials,
                                 int32_t part, void* stream);
int mcdseg_conv_split_dgrad_part(const mcdseg_conv_desc* d, int32_t math, const float* dy, const void* dy_cb, const float* dy_bound,
                                 const void* wp_dgrad, const float* w_bound, float* dx, int32_t part, void* stream);
/* same workspace as mcdseg_conv_wgrad; 128x128-tile layers run on the split path, thin layers on the f32 kernels.
 * x_cb / dy_cb (may be NULL; used only when BOTH are given): the pre-split companions of x and dy in the layout above --
 * the kernel then transposes 8x8 blocks of 16-bit pieces in registers instead of splitting fp32 values.  x / dy may be NULL
 * only when that path applies (both companions, channel counts divisible by 8, min(Cin,Cout) > 64, not the thin-input plan). */
int mcdseg_conv_split_wgrad(const mcdseg_conv_desc* d, int32_t math, const float* x, const void* x_cb, const float* x_bound,
                            const float* dy, const void* dy_cb, const float* dy_bound, float* dw, void* workspace,
                            size_t workspace_bytes, void* stream);
/* which kernel the two weight-gradient entry points launch for a geometry (math = 0: mcdseg_conv_wgrad): 0..3 the f32 plans
 * (128x128, 64x64, 32x32 tiles, tap-packed thin inputs), 10 split arithmetic from fp32 operands, 11 / 12 / 13 from both
 * pre-split companions (register-transposing for bf16x6, transposed-read 128x128, transposed-read 256x128), 14 the 64-channel tap pairs,
 * 15 the thin-layer window kernel, 16 retired (two taps per workgroup), 17 the eight-wave ping-pong kernel over a stream-K decomposition
 * (256-channel blocks on both sides; csrc/conv_wgrad_split_pp.hip), 18 its row-of-taps form for 3 x KH kernels with at most 128
 * channels on one side (tiles of 128 co x three taps x 128 ci).  `presplit`: both companions (and the bound scalars the arithmetic
 * needs) are passed.  This is what callers plan with -- which operands to keep, where to cut a batch, the kernel name a profiler will
 * see -- and what the entry points themselves switch on (csrc/conv_wgrad.hip, wgrad_route). */
int32_t mcdseg_conv_wgrad_variant(const mcdseg_conv_desc* d, int32_t math, int32_t presplit);
/* 1 when ONE launch of mcdseg_conv_wgrad (math = 0) / mcdseg_conv_split_wgrad (presplit: both companions are passed) can address
 * this descriptor's operands with its 32-bit buffer offsets: (N*C + 128 channels of slack) planes below 2 GiB for the kernels that
 * read the fp32 tensors, N*C planes for the plans that read the companions (variants 11..18).  The host cuts larger batches along
 * N -- the reference has no such limit (nn.Conv2d, models/drn.py:21-23).  Host-side arithmetic, no launch. */
int32_t mcdseg_conv_wgrad_fits(const mcdseg_conv_desc* d, int32_t math, int32_t presplit);
/* dw = x (*) dy ; split over pixels into slabs in `workspace`, then reduced in a fixed order.  mcdseg_conv_wgrad_workspace_bytes
 * covers every call a caller may make for this descriptor under the current options: the largest need over mcdseg_conv_wgrad and
 * mcdseg_conv_split_wgrad in each arithmetic, with and without the companions (and variant 15's whether or not its option is on). */
size_t mcdseg_conv_wgrad_workspace_bytes(const mcdseg_conv_desc* d);
int mcdseg_conv_wgrad(const mcdseg_conv_desc* d, const float* x, const float* dy, float* dw,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (train: batch statistics, eps 1e-5, momentum 0.1; eval: running statistics)
 * fused with ReLU and the residual add of BasicBlock/Bottleneck (models/drn.py:43-59, 80-100)
 * ---------------------------------------------------------------------------------------------- */
/* Merge the conv epilogue partials -> mean[C], rstd[C]; update running_mean/var (unbiased var) and
 * num_batches_tracked when those pointers are non-NULL -- running_updates times (>= 1): one launch may stand for several identical
 * forward passes of the reference's schedule (solvers/solver.py; each update is rounded to fp32 as a separate pass would).
 * workspace: 8-byte aligned scratch.
 * y_bound (may be NULL): receives an upper bound of |y| for the tensor mcdseg_bn_apply(_cb) is about to write from these
 * statistics, y = act(gamma*xhat + beta (+ residual)): max_c(|gamma_c| sqrt(n-1) + |beta_c|) + res_bound[0], using
 * Samuelson's inequality |xhat| <= sqrt(n-1) for a batch of n values normalised by their own mean and biased variance
 * (gamma, beta required then; res_bound = bound scalar of the residual tensor or NULL).  The inequality needs z to be the very
 * tensor the statistics came from, so the bound is valid in train mode only: eval mode (running statistics) has no such bound. */
size_t mcdseg_bn_stats_workspace_bytes(int64_t rows, int32_t C);
int mcdseg_bn_stats_finalize(const float* stat_partials, int64_t rows, int32_t C, int32_t Mp,
                             float* mean, float* rstd, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float momentum, float eps,
                             const float* gamma, const float* beta, const float* res_bound, float* y_bound,
                             int32_t running_updates, void* workspace, size_t workspace_bytes, void* stream);
/* eval mode: mean = running_mean, rstd = 1/sqrt(running_var+eps) */
int mcdseg_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps,
                         float* mean, float* rstd, void* stream);
/* eval-mode BN as an affine map: scale = gamma/sqrt(running_var+eps), shift = beta + (conv_bias - running_mean)*scale
 * (conv_bias may be NULL) -- feeds mcdseg_conv_fprop_affine */
int mcdseg_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          const float* conv_bias, int32_t C, float eps, float* scale, float* shift, void* stream);
/* y = act(gamma*(z-mean)*rstd + beta (+ residual)), act = ReLU if relu != 0 */
int mcdseg_bn_apply(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                    const float* residual, float* y, int32_t N, int32_t C, int32_t HW, int32_t relu, void* stream);
/* Same as mcdseg_bn_apply / mcdseg_bn_bwd_apply, additionally emitting the split of the produced tensor (pieces of `math`,
 * scale from the bound scalar for MCDSEG_MATH_F16X3; NULL for BF16X6) in the channel-blocked layout
 * [piece][N][C/8][HW][8 x 16 bit] consumed by the split convolutions; C must be divisible by 8.  mcdseg_bn_bwd_apply_cb
 * accepts dz == NULL (only the split companion is written) for layers whose input and weight gradients both read the
 * companion.  mcdseg_split_cb is the split alone (fp32 NCHW -> companion) for operands no fused BN group produced,
 * mcdseg_unsplit_cb its inverse (value = scale * sum of the pieces: exact for BF16X6, the 22 leading bits for F16X3).
 * Compact activation storage (the fp32 activation is never written; what travels is the companion): mcdseg_bn_apply_cb accepts
 * y == NULL and the residual as a companion (res_cb, res_bound) instead of fp32; the backward kernels accept y == NULL with y_cb,
 * reading the ReLU mask from the companion's leading piece. */
int mcdseg_split_cb(const float* x, void* x_cb, const float* x_bound, int32_t math, int32_t N, int32_t C, int32_t HW, void* stream);
/* The same for a channel count that is not a multiple of 8 (the 6-channel RGB+HHA network input, adapt_trainer.py:157-160): the
 * companion has ceil(C/8) channel groups -- [piece][N][ceil(C/8)][H*W][8 x 16 bit] -- with zeros in the missing channels.  Read
 * by the weight-gradient kernel of the 7x7 stem (models/drn.py:126-131) only. */
int mcdseg_split_cb_padded(const float* x, void* x_cb, const float* x_bound, int32_t math, int32_t N, int32_t C, int32_t HW,
                           void* stream);
int mcdseg_unsplit_cb(const void* x_cb, const float* x_bound, int32_t math, int32_t N, int32_t C, int32_t HW, float* x, void* stream);
/* The stage join of the FuseNet-style generator: x = torch.add(x, x_dk) behind every stage of the RGB pass
 * (FuseDRNSegBase.forward, models/dilated_fcn.py:308-328).  y = a + b (fp32 NCHW, the fp32 add and nothing else) and, y_cb != NULL,
 * the companion of y for the next stage's convolutions in the same pass: [piece][N][C/8][HW][8 x 16 bit], bitwise what
 * mcdseg_split_cb(y, y_bound) writes.  Nothing is reduced: |a + b| <= a_bound[0] + b_bound[0], and y_bound[0] is that one fp32 sum
 * (the scale is at most one power of two coarser than a measured bound would give).  MCDSEG_MATH_F16X3 / _F16X1 need the three bound
 * pointers; MCDSEG_MATH_BF16X6 takes them as NULL (all three or none: given, y_bound is written all the same).  y_cb == NULL: any C,
 * only y (and y_bound, when the bounds are given) is written, `math` is not read.  With a companion the refusals of mcdseg_split_cb
 * apply (C % 8, N * C/8 > 65535); every refusal is answered before anything is launched. */
int mcdseg_stage_join(const float* a, const float* a_bound, const float* b, const float* b_bound, float* y, void* y_cb, float* y_bound,
                      int32_t math, int32_t N, int32_t C, int32_t HW, void* stream);
/* The operators of the U-Net generator and classifiers (models/unet.py of the reference: UNetBase :122-171, UNetUp :29-43,
 * UNetClassifier :174-199), fp32 NCHW.  No float atomics: every result is the same bits run to run.  Every refusal is -EINVAL with a
 * mcdseg_last_error message, answered before anything is launched.
 *
 * mcdseg_maxpool2_fwd / _bwd: nn.MaxPool2d(kernel_size=2) (:135-159).  H and W must be even.  y[n,c,i,j] is the maximum of the 2x2
 * window by torch's CPU rule: the window is walked (0,0), (0,1), (1,0), (1,1) from -inf and a value takes over when it is greater than
 * the best so far or is a NaN -- the first of equal values wins (-0 against +0 included), a NaN wins over what came before it.  The
 * backward takes x and dy and writes EVERY element of dx: dy at the window's arg-max (recomputed from x: no index tensor exists), 0 at
 * the other three.  y_cb != NULL: the companion of y in the same pass, [piece][N][C/8][Ho*Wo][8 x 16 bit], bitwise what
 * mcdseg_split_cb(y, y_bound) writes, with y_bound[0] = x_bound[0] (|max| cannot exceed the bound of x: nothing is reduced); then the
 * refusals of mcdseg_split_cb apply (C % 8, N * C/8 > 65535, MCDSEG_MATH_F16X3 / _F16X1 without the bounds).  The bounds come as both
 * pointers or none.
 *
 * mcdseg_relu_fwd / _bwd: the nn.ReLU behind the BatchNorm-less convolutions of UNetUp (:18-21).  y = x < 0 ? +0 : x (torch's
 * clamp: -0 and NaN pass); y may be x.  The companion and the bound as for the pool.  Backward: dx = y > 0 ? dy : 0, from y; dx may be dy.
 *
 * mcdseg_deconv2x2_fwd / _bwd_data / _bwd_weight: nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) (:34),
 *   y[n,co,2i+a,2j+b] = bias[co] + sum_ci x[n,ci,i,j] * w[ci,co,a,b]
 * with w in torch's [Cin][Cout][2][2] layout as the parameter holds it (bias may be NULL) and x [N][Cin][H][W].  y and dy are channel
 * slices of a larger buffer (the concatenation torch.cat([shortcut, up(h)], 1) of :43): element (n, co, r, s) lies at
 * base[n * batch_stride + (channel_offset + co) * 4*H*W + r * 2*W + s], `channels` being the buffer's channel count; a slice outside
 * the buffer (channel_offset + Cout > channels, batch_stride < channels * 4*H*W) is refused.  Plain fp32 FMA chains in a fixed order.
 * _bwd_weight writes dw [Cin][Cout][2][2] and db [Cout] (db may be NULL) in two stages: fp64 block partials in the workspace
 * (mcdseg_deconv2x2_bwd_weight_workspace_bytes, 8-byte aligned), then one finalize kernel. */
int mcdseg_maxpool2_fwd(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int32_t math, int32_t N, int32_t C,
                        int32_t H, int32_t W, void* stream);
int mcdseg_maxpool2_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int mcdseg_relu_fwd(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int32_t math, int32_t N, int32_t C,
                    int32_t HW, void* stream);
int mcdseg_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
int mcdseg_deconv2x2_fwd(const float* x, const float* w, const float* bias, float* y, int64_t y_batch_stride, int32_t y_channels,
                         int32_t y_channel_offset, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, void* stream);
int mcdseg_deconv2x2_bwd_data(const float* dy, int64_t dy_batch_stride, int32_t dy_channels, int32_t dy_channel_offset, const float* w,
                              float* dx, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, void* stream);
size_t mcdseg_deconv2x2_bwd_weight_workspace_bytes(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W);
int mcdseg_deconv2x2_bwd_weight(const float* x, const float* dy, int64_t dy_batch_stride, int32_t dy_channels, int32_t dy_channel_offset,
                                float* dw, float* db, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, void* workspace,
                                size_t workspace_bytes, void* stream);
int mcdseg_bn_apply_cb(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       const float* residual, const void* res_cb, const float* res_bound, float* y, void* y_cb,
                       const float* y_bound, int32_t math, int32_t N, int32_t C, int32_t HW, int32_t relu, void* stream);
int mcdseg_bn_bwd_apply_cb(const float* dy, const float* y, const void* y_cb, const float* z, const float* mean, const float* rstd,
                           const float* gamma, const float* dgamma, const float* dbeta, float* dz, float* dres,
                           void* dz_cb, const float* dz_bound, int32_t math, int32_t N, int32_t C, int32_t HW, int32_t relu,
                           int32_t train, void* stream);
/* The backward pair for a ReLU group WITHOUT a residual branch (models/drn.py:43-47 bn1; the conv-BN-ReLU chains of
 * _make_conv_layers): the mask y > 0 is recomputed from z -- y > 0 <=> fma(z, gamma rstd, beta - mean gamma rstd) > 0 (with the mean
 * subtracted from z first in a channel whose |mean| rstd exceeds 8: csrc/bn.hip, bn_forward_map), which is the forward kernels' own
 * expression, bit for bit -- so y is not read at all: 8 instead of 12 bytes per element in the reduce, 12
 * instead of 16 in the apply.  Same results as mcdseg_bn_bwd_reduce / mcdseg_bn_bwd_apply_cb with relu = 1 and the group's fp32 y. */
int mcdseg_bn_bwd_reduce_zmask(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, float* dgamma, float* dbeta, float* dz_bound, int32_t train, int32_t N, int32_t C,
                               int32_t HW, void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_bn_bwd_apply_cb_zmask(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, const float* dgamma, const float* dbeta, float* dz, void* dz_cb,
                                 const float* dz_bound, int32_t math, int32_t N, int32_t C, int32_t HW, int32_t train, void* stream);
/* The same economy for a ReLU group WITH a residual branch (models/drn.py:48-57: out = relu(bn2(conv2(out)) + residual)), whose mask
 * cannot be recomputed from z: the forward apply kernel also writes the mask as a bit-plane -- per (image, channel) and block of 256
 * pixels four 64-bit words, bit l of word j = (y > 0) of pixel 256 blk + 4 l + j; mcdseg_bn_relu_mask_bytes gives its size, 0 when the
 * geometry has none (HW not a multiple of 4) -- and the backward pair reads 1 bit per element where mcdseg_bn_bwd_reduce /
 * mcdseg_bn_bwd_apply_cb read the 32 of the fp32 y: 8 instead of 12 and 16 instead of 20 bytes per element.  y > 0 is evaluated once, on
 * the value that was stored: the same mask, the same results bit for bit.  Tensors 16-byte aligned, the mask 8-byte aligned. */
size_t mcdseg_bn_relu_mask_bytes(int32_t N, int32_t C, int32_t HW);
int mcdseg_bn_apply_cb_mask(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                            const float* residual, float* y, void* y_cb, const float* y_bound, void* relu_mask, int32_t math, int32_t N,
                            int32_t C, int32_t HW, void* stream);
int mcdseg_bn_bwd_reduce_mask(const float* dy, const void* relu_mask, const float* z, const float* mean, const float* rstd,
                              const float* gamma, float* dgamma, float* dbeta, float* dz_bound, int32_t train, int32_t N, int32_t C,
                              int32_t HW, void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_bn_bwd_apply_cb_mask(const float* dy, const void* relu_mask, const float* z, const float* mean, const float* rstd,
                                const float* gamma, const float* dgamma, const float* dbeta, float* dz, float* dres, void* dz_cb,
                                const float* dz_bound, int32_t math, int32_t N, int32_t C, int32_t HW, int32_t train, void* stream);
/* Backward.  dy is the gradient w.r.t. y; y (the saved forward output) -- or, when y == NULL, its companion y_cb of
 * arithmetic `math` -- supplies the ReLU mask when relu != 0.  reduce: dgamma[c] = sum dy_m*xhat, dbeta[c] = sum dy_m.
 * With z == NULL only dbeta is produced (used for the conv bias gradient, models/dilated_fcn.py:227).
 * dz_bound (may be NULL; needs z and gamma): receives an upper bound of |dz| for the tensor mcdseg_bn_bwd_apply(_cb) will
 * write: max_c |gamma_c rstd_c| (max|dy_m| + |dbeta_c|/n + sqrt(n-1) |dgamma_c|/n) in train mode, max_c |gamma_c rstd_c|
 * max|dy_m| in eval mode (train selects). */
size_t mcdseg_bn_bwd_workspace_bytes(int32_t N, int32_t C, int32_t HW);
int mcdseg_bn_bwd_reduce(const float* dy, const float* y, const void* y_cb, int32_t math, const float* z, const float* mean,
                         const float* rstd, float* dgamma, float* dbeta, const float* gamma, float* dz_bound, int32_t train,
                         int32_t N, int32_t C, int32_t HW, int32_t relu,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dz = gamma*rstd*(dy_m - dbeta/n - xhat*dgamma/n) (train) or gamma*rstd*dy_m (eval);
 * dres (optional) = dy_m, the gradient of the residual branch. */
int mcdseg_bn_bwd_apply(const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                        const float* gamma, const float* dgamma, const float* dbeta, float* dz, float* dres,
                        int32_t N, int32_t C, int32_t HW, int32_t relu, int32_t train, void* stream);

/* ------------------------------------------------------------------------------------------------
 * x8 learned up-sampler: depthwise ConvTranspose2d(C,C,16,stride 8,pad 4,groups=C,bias=False)
 * (models/dilated_fcn.py:357-366, 479-491).  x [N,C,Hi,Wi] -> y [N,C,8Hi,8Wi], w [C,1,16,16].
 * With x2/w2 != NULL computes y = up(x,w) + up(x2,w2) (ScoreFusion + AddFusion, models/fusion.py:24-29).
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_up8_fwd(const float* x, const float* w, const float* x2, const float* w2, float* y,
                   int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* stream);
int mcdseg_up8_bwd_input(const float* dy, const float* w, float* dx, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                         void* stream);
size_t mcdseg_up8_bwd_weight_workspace_bytes(int32_t N, int32_t C, int32_t Hi, int32_t Wi);
int mcdseg_up8_bwd_weight(const float* dy, const float* x, float* dw, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Both backward passes of the up-sampler (either may be skipped: dx == NULL or dw == NULL) from ONE staged read of dy -- the
 * backward of DRNSegPixelClassifier.up (models/dilated_fcn.py:357-366) as autograd runs it in adapt_trainer.py:172-212.  Same
 * results as mcdseg_up8_bwd_input / mcdseg_up8_bwd_weight up to the order of the fp32 sums; falls back to those two kernels
 * when a dy row band does not fit the LDS ring (Wi > 192). */
size_t mcdseg_up8_bwd_workspace_bytes(int32_t N, int32_t C, int32_t Hi, int32_t Wi);
int mcdseg_up8_bwd(const float* dy, const float* w, const float* x, float* dx, float* dw, int32_t N, int32_t C, int32_t Hi,
                   int32_t Wi, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused per-pixel softmax -> weighted CE (both heads) -> L1 discrepancy, forward + gradient
 * (loss.py:7-13 CrossEntropyLoss2d, loss.py:93-100 Diff2d; three-step use adapt_trainer.py:163-212)
 *
 *   losses[0] = CE(z1,labels)  losses[1] = CE(z2,labels)  losses[2] = mean|softmax(z1)-softmax(z2)|
 *   losses[3] = sum_i w[y_i]
 *   g1 = ce_coef * dCE1/dz1 + diff_coef * dDiff/dz1,   g2 likewise for z2.
 * Any of z2 / labels / g1 / g2 may be NULL (single-head CE, discrepancy only, loss values only).
 * wsum_in (device scalar, may be NULL) overrides the CE normaliser sum_i w[y_i]: under data parallelism the
 * caller passes the all-reduced sum over all shards so that averaged per-rank gradients equal the gradient
 * of the reference's single global weighted mean (nn.DataParallel gathers logits before the loss).
 * ---------------------------------------------------------------------------------------------- */
size_t mcdseg_loss_workspace_bytes(int32_t N, int32_t HW);
int mcdseg_softmax_ce_l1(const float* z1, const float* z2, const int64_t* labels, const float* class_weight,
                         int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in,
                         float* g1, float* g2, float* losses,
                         int32_t N, int32_t C, int32_t HW, void* workspace, size_t workspace_bytes, void* stream);
/* The same losses and gradients for z_k = up8(s_k, w_k) (the x8 up-sampler above) WITHOUT the full-resolution logits ever being
 * stored: the MCD classifiers are exactly that up-sampler (models/dilated_fcn.py:357-366; F1(G(x)), F2(G(x)) of
 * adapt_trainer.py:163-212), so the kernel forms each pixel's logits from the [N,C,Hi,Wi] score maps on the fly.  s1 and s2 may
 * be the same tensor (both heads read the generator's scores); s2 / w2 NULL = single head.  g1 / g2 are [N,C,8Hi,8Wi], to be
 * fed to mcdseg_up8_bwd_input / mcdseg_up8_bwd_weight; they equal the two-pass result bit for bit. */
size_t mcdseg_up8_loss_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi);
int mcdseg_up8_softmax_ce_l1(const float* s1, const float* w1, const float* s2, const float* w2, const int64_t* labels,
                             const float* class_weight, int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in,
                             float* g1, float* g2, float* losses, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same two passes with the classifier discrepancy of the reference's --d_loss (argmyparse.py, loss.py:192-210) in place of the L1
 * distance: losses[2] = the distance, g_k = ce_coef * dCE_k/dz_k + diff_coef * dDist/dz_k.  With p = softmax(z1), q = softmax(z2) and the
 * element mean over N*C*H*W that every one of these criteria uses:
 *   MCDSEG_DIST_L1         mean |p - q|                                  Diff2d                            loss.py:93-100
 *   MCDSEG_DIST_SYMKL      mean 0.5 (p - q)(log p - log q)               Symkl2d, MySymkl2d                loss.py:103-118, 144-154
 *   MCDSEG_DIST_MIS_SYMKL  mean 0.5 (p log p + q log q - 2 p q)          MisSymKLD, SpatialJSD2d           loss.py:66-75, 157-173
 *   MCDSEG_DIST_JSD        mean 0.5 (p log(p/m) + q log(q/m)), m = softmax((z1 + z2) / 2)        JSD       loss.py:78-89
 * Arguments as mcdseg_softmax_ce_l1 / mcdseg_up8_softmax_ce_l1 (workspaces included) plus dist_kind.  MCDSEG_DIST_L1 launches the kernels
 * of those entry points (bitwise the same results); the other kinds are distances between two heads: z2 (s2, w2) must not be NULL.
 * An unknown dist_kind is an argument error.  The fused form launches `up8_softmax_ce_dist_dma_kernel<classes, exact, kind>` where
 * mcdseg_up8_loss_variant is positive and `up8_softmax_ce_dist_kernel<classes, kind>` where it is negative. */
#define MCDSEG_DIST_L1 0
#define MCDSEG_DIST_SYMKL 1
#define MCDSEG_DIST_MIS_SYMKL 2
#define MCDSEG_DIST_JSD 3
int mcdseg_softmax_ce_dist(const float* z1, const float* z2, const int64_t* labels, const float* class_weight,
                           int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in,
                           float* g1, float* g2, float* losses,
                           int32_t N, int32_t C, int32_t HW, int32_t dist_kind, void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_up8_softmax_ce_dist(const float* s1, const float* w1, const float* s2, const float* w2, const int64_t* labels,
                               const float* class_weight, int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in,
                               float* g1, float* g2, float* losses, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t dist_kind,
                               void* workspace, size_t workspace_bytes, void* stream);
/* out[0] = sum_i w[labels_i] over P pixels (ignore_index and out-of-range labels contribute 0) */
size_t mcdseg_label_weight_sum_workspace_bytes(int64_t P);
int mcdseg_label_weight_sum(const int64_t* labels, const float* class_weight, int64_t ignore_index, int32_t C, int64_t P,
                            float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Inference tail (adapt_tester.py:101-124; util.py:44-48): o = z1, or (z1+z2)/2 when z2 != NULL;
 * labels[n,hw] = argmax_{c < C_used} o (uint8; the background channel is excluded by C_used = C-1 unless it was trained);
 * entropy[0] = -mean_{n,c,hw} p log(p + 1e-6), p = softmax over all C classes. */
size_t mcdseg_predict_workspace_bytes(int32_t N, int32_t HW);
int mcdseg_predict_labels(const float* z1, const float* z2, uint8_t* labels, float* entropy, int32_t N, int32_t C,
                          int32_t C_used, int32_t HW, void* workspace, size_t workspace_bytes, void* stream);
/* The same tail fused with the x8 up-sampler that precedes it, so the [N,C,8Hi,8Wi] logits are never stored
 * (the reference's source_tester.py:119-143: DRNSeg's learned up-sampler; adapt_multitask_tester.py:118-141: the multitask decoder's
 * bilinear one on pred_semseg1).  z = up8(s, w) as mcdseg_up8_fwd computes it (single input) when w != NULL (w: [C,1,16,16]), else
 * z = bilinear x8 (align_corners = False) as mcdseg_bilinear8_fwd computes it; then labels [N,8Hi,8Wi] and entropy[0] exactly as
 * mcdseg_predict_labels(z, NULL, ...) defines them -- the labels equal that composition bit for bit.  C <= 48; one workgroup per image and
 * band of 8 output rows holds two input rows of the C channels (+ the C kernels) in LDS: 8 C Wi (+ 1024 C) bytes, at most 160 KB. */
size_t mcdseg_predict_up8_workspace_bytes(int32_t N, int32_t Hi);
int mcdseg_predict_labels_up8(const float* s, const float* w, uint8_t* labels, float* entropy, int32_t N, int32_t C, int32_t C_used,
                              int32_t Hi, int32_t Wi, void* workspace, size_t workspace_bytes, void* stream);
/* The Monte-Carlo dropout loss of the uncertain source-only model, all T draws in one pass over the pixels
 * (UncertainDRNSeg.get_loss, models/dilated_fcn.py:169-214; forward :153-161; source_uncertain_trainer.py:136-140).
 * The reference runs the network T = n_dropout_exp times; its only randomness is Dropout2d(0.2) on the scores s [N,C,Hi,Wi] -- a
 * factor m_t[n,c] in {0, keep_scale} -- and one scalar r_t = np.random.rand() per draw, and both up-samplers are depthwise and linear:
 * with U = up8(s, w_up), V = up8(s, w_std) (mcdseg_up8_fwd's values), pred_mean_t = m_t U, pred_std_t = m_t relu(V),
 * y_hat_t = m_t U + (m_t relu(V)) r_t.  Per pixel i of sample n with label g, W = sum_i class_weight[g_i] (or *wsum_in), HW = 64 Hi Wi,
 * p_t = softmax(y_hat_t)[g], S = sum_t p_t:
 *   losses[0]        = B   = (1/T) sum_t CrossEntropyLoss2d(m_t U, g)     (loss.py:7-13; dilated_fcn.py:178, 202)
 *   losses[1]        = W
 *   losses[2 .. 2+N) = U_n = (lambda/HW) sum_i log(S_i / T)               (dilated_fcn.py:183-204, 212; the reference's sign: + log)
 * keep: uint8 [T,N,C], 1 = the channel is kept in that draw (m = keep_scale = 1/(1-p), 1.25 for the reference's p = 0.2), 0 = dropped;
 * r: fp32 [T] on the device.  Pixels whose label is ignore_index or outside [0,C) contribute 0 to B, W, U_n and to every gradient; HW
 * stays the full pixel count.  class_weight may be NULL (weights 1).  C <= 48, 1 <= T <= 32 and N <= 65535 (argument errors otherwise).
 * Softmax and log-sum-exp subtract the maximum (the reference's bare log(sum(exp)) is the same value wherever it is finite).
 * mcdseg_up8_uncertain_loss_bwd: the gradients w.r.t. U and V (never stored themselves) for the upstream gradients gb (of B, device
 * scalar) and gu [N] (of U_n), read from device memory -- nothing synchronises with the host:
 *   GU[c] = sum_t m_t[c] (a_t[c] + b_t[c]),   GV[c] = sum_t m_t[c] [V[c] > 0] r_t b_t[c]          (both [N,C,8Hi,8Wi])
 *   a_t[c] = gb cw[g] / (T W) (softmax(m_t U)[c] - [c = g]),   b_t[c] = gu[n] (lambda/HW) (p_t / S) ([c = g] - softmax(y_hat_t)[c])
 * wsum: the forward's losses + 1.  mcdseg_up8_bwd(GU, w_up, s, ...) and mcdseg_up8_bwd(GV, w_std, s, ...) finish the backward pass.
 * No tensor with a T dimension is formed; loss values are summed per workgroup and then in fp64 (no atomics: bit-reproducible). */
size_t mcdseg_up8_uncertain_loss_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi);
int mcdseg_up8_uncertain_loss_fwd(const float* s, const float* w_up, const float* w_std, const int64_t* labels,
                                  const float* class_weight, int64_t ignore_index, const uint8_t* keep, const float* r,
                                  float keep_scale, const float* wsum_in, float lambda, float* losses, int32_t N, int32_t C,
                                  int32_t Hi, int32_t Wi, int32_t T, void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_up8_uncertain_loss_bwd(const float* s, const float* w_up, const float* w_std, const int64_t* labels,
                                  const float* class_weight, int64_t ignore_index, const uint8_t* keep, const float* r,
                                  float keep_scale, const float* wsum, float lambda, const float* gb, const float* gu, float* GU,
                                  float* GV, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t T, void* stream);
/* The uncertain tester's map (source_uncertain_tester.py:158-166 with the channel sum that its line 163 and dilated_fcn.py:160 leave
 * commented out; plt.imshow takes the literal [C,H,W] array only for C = 3 or 4):
 * out[n,y,x] = sum_{c < C_used} relu(up8(s, w_std))[n,c,y,x], fp32 [N,8Hi,8Wi], without the C-channel full-resolution tensor. */
int mcdseg_up8_std_sum(const float* s, const float* w_std, float* out, int32_t N, int32_t C, int32_t C_used, int32_t Hi, int32_t Wi,
                       void* stream);
/* The domain classifier of the DANN baseline (DRNSegDomainClassifier, models/dilated_fcn.py:494-551; dann_trainer.py:258-322), fused.
 * csrc/dann.hip.  Everything fp32; no floating-point atomics, every sum in a fixed order: results are bit-identical from run to run.
 *
 * mcdseg_dann_down_fwd: one whole DownConv (models/dilated_fcn.py:506-531): y = maxpool2x2(relu(conv3x3(relu(conv3x3(x, w1) + b1), w2)
 * + b2)), both convolutions with padding 1, x [N,Cin,H,W], w1 [Cmid,Cin,3,3], w2 [Cmid,Cmid,3,3], y [N,Cmid,H/2,W/2] (floor: the last
 * row / column of an odd map takes no part in the pooling, as in torch).  The two full-resolution intermediates exist in LDS only.
 * Nothing couples the samples, so N may be the batch of both domains.  Cmid = Cout is 1 or 10; Cin <= 50 at Cmid = 10 and <= 69 at
 * Cmid = 1 (the backward's tile -- 24 x 24 pixels of every input channel plus three Cmid-channel regions -- must fit the 160 KB of
 * LDS; both entry points refuse a larger shape and launch nothing).
 * mcdseg_dann_down_bwd: dx (may be NULL: not wanted), dw1, db1, dw2, db2 for the upstream gradient dy [N,Cmid,H/2,W/2], recomputed
 * from x and the weights.  A pooling window passes its gradient to its FIRST maximum in row-major order (torch's max_pool2d) and
 * nothing where that maximum is a ReLU zero.  Parameter gradients: one partial per workgroup in `workspace`
 * (mcdseg_dann_down_workspace_bytes), then an ordered second stage (a second launch) that sums each of the `groups` equal groups of
 * samples (domains) by itself and then the groups in order: the gradients of a batch of both domains are, bit for bit, the sum of the
 * gradients of one call per domain, which is what autograd accumulates.  The tail's parameter gradients are formed the same way.
 *
 * mcdseg_dann_tail_fwd: the rest of the classifier (models/dilated_fcn.py:547-551) and nn.CrossEntropyLoss (dann_trainer.py:244,
 * 292-293, 318-319) for G groups (domains) of n rows each in one launch: h [G n, F] (the flattened second DownConv output),
 * z = h w1^T + b1 (w1 [10,F]), BatchNorm1d(10), ReLU, logits [G n, 2] = a w2^T + b2 (w2 [2,10]), loss[g] = the mean over the rows of
 * group g of the cross-entropy against labels[g] (int32 on the device, 0 or 1; any other value counts as 1).  training != 0: the
 * statistics are PER GROUP -- biased variance normalises, running_mean / running_var take (1 - momentum) old + momentum new with the
 * unbiased variance, group after group, as one module call per domain would; n >= 2 (torch refuses one row).  training == 0: the
 * running statistics normalise and are left alone (--fix_bn).  save (mcdseg_dann_tail_save_bytes) keeps z and the statistics used.
 * mcdseg_dann_tail_bwd: for one upstream scalar per group (upstream [G] on the device: -1 in the trainer's first update, +1 in its
 * second) dh [G n, F] (may be NULL) and dw1, db1, dgamma, dbeta, dw2, db2; workspace: mcdseg_dann_tail_workspace_bytes.
 * One workgroup each (the batch couples the rows; the problem is a few kilobytes); G <= 64. */
size_t mcdseg_dann_down_workspace_bytes(int32_t N, int32_t Cin, int32_t Cmid, int32_t H, int32_t W);
int mcdseg_dann_down_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, int32_t N,
                         int32_t Cin, int32_t Cmid, int32_t H, int32_t W, void* stream);
int mcdseg_dann_down_bwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* dy, float* dx,
                         float* dw1, float* db1, float* dw2, float* db2, int32_t N, int32_t Cin, int32_t Cmid, int32_t H, int32_t W,
                         int32_t groups, void* workspace, size_t workspace_bytes, void* stream);
size_t mcdseg_dann_tail_save_bytes(int32_t G, int32_t n);
size_t mcdseg_dann_tail_workspace_bytes(int32_t G, int32_t n);
int mcdseg_dann_tail_fwd(const float* h, const int32_t* labels, const float* w1, const float* b1, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, const float* w2, const float* b2, float momentum, float eps,
                         int32_t training, float* loss, float* logits, float* save, int32_t G, int32_t n, int32_t F, void* stream);
int mcdseg_dann_tail_bwd(const float* h, const int32_t* labels, const float* w1, const float* gamma, const float* beta, const float* w2,
                         const float* logits, const float* save, const float* upstream, float* dh, float* dw1, float* db1, float* dgamma,
                         float* dbeta, float* dw2, float* db2, int32_t training, int32_t G, int32_t n, int32_t F, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Depth image of the multitask tester (adapt_multitask_tester.py:148-155 with transform.py:285-294, unnormalize): d [N,Cd,Hi,Wi] fp32
 * (Cd = 1 or 3, the depth head) -> img [N,8Hi,8Wi,3] uint8 HWC.  v = bilinear x8 of d (mcdseg_bilinear8_fwd's fp32 values) in channel
 * Cd == 1 ? 0 : k; t = ((double)v * STD[k] + MEAN[k]) * 255 with every operation rounded in double (numpy's promotion against the
 * float64 constants MEAN = (.485,.456,.406), STD = (.229,.224,.225)); Cd = 1 broadcasts into three channels as numpy does; the byte
 * is numpy's np.uint8(t) on x86-64: t truncated to int32, low 8 bits kept, 0 for NaN, +-inf and t outside the int32 range (so
 * -1.0 -> 255, 300.7 -> 44: an undertrained regressor's values wrap, as in the reference's PNGs).  No workspace. */
int mcdseg_depth_image_u8(const float* d, uint8_t* img, int32_t N, int32_t Cd, int32_t Hi, int32_t Wi, void* stream);
/* buf[i] *= *scale (device scalar) -- applies autograd's upstream scalar without a host sync */
int mcdseg_scale_by_device_scalar(float* buf, const float* scale, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multitask decoder (BASELINE config 4; models/dilated_fcn.py:661-739)
 *   bilinear x8 up-sampling with align_corners = False (nn.Upsample(scale_factor=8, mode='bilinear'), :676)
 *   loss[0] = mean((pred-target)^2), grad = 2 (pred-target) / n            (F.mse_loss, :712-714)
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_bilinear8_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* stream);
int mcdseg_bilinear8_bwd(const float* dy, float* dx, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* stream);
size_t mcdseg_mse_workspace_bytes(int64_t n);
int mcdseg_mse(const float* pred, const float* target, float* grad, float* loss, int64_t n,
               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MFNet late fusion beyond the plain sum (models/fusion.py:6-50) and its loss (loss.py:16-30)
 *   gate_mix:    out = x1*s + x2*(1-s), s = sigmoid(g)   (GateFusion.forward :19-22; g = 1x1 conv of cat(x1,x2))
 *                backward: dx1 = dy*s, dx2 = dy*(1-s), dg = dy*(x1-x2)*s*(1-s).  n = element count, any n > 0; pointers
 *                need only float alignment (16-byte vector accesses are used when every pointer of the call allows them,
 *                a scalar pass otherwise, with the same bits).
 *   softmax_ch:  softmax over C of NCHW (F.softmax of ScoreGateFusion :13-15); backward dx = y*(dy - sum_c dy*y). C <= 64.
 *   prob_nll:    ProbCrossEntropyLoss2d: NLLLoss2d(weight)(log(p), labels).  loss[0] = weighted mean, loss[1] = weighted
 *                sum, loss[2] = sum of weights; grad (may be NULL) = d loss[size_average ? 0 : 1] / dp, dense NCHW.
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_gate_mix_fwd(const float* x1, const float* x2, const float* g, float* out, int64_t n, void* stream);
int mcdseg_gate_mix_bwd(const float* dy, const float* x1, const float* x2, const float* g, float* dx1, float* dx2, float* dg,
                        int64_t n, void* stream);
int mcdseg_softmax_ch_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t HW, void* stream);
int mcdseg_softmax_ch_bwd(const float* dy, const float* y, float* dx, int32_t N, int32_t C, int32_t HW, void* stream);
size_t mcdseg_prob_nll_workspace_bytes(int32_t N, int32_t HW);
int mcdseg_prob_nll(const float* p, const int64_t* labels, const float* weight, int64_t ignore_index, int32_t size_average,
                    float* grad, float* loss, int32_t N, int32_t C, int32_t HW, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Boundary branch of the segmentation + boundary multitask decoder (MCDSegBDMultiTaskDecoder, models/dilated_fcn.py:1027-1222).
 * H, W are the FULL resolution; every sum below leaves its block as an fp64 partial and is finished by one small kernel in fp64
 * (no float atomics: results are bitwise reproducible); nothing synchronises with the host.
 *   label_boundary (get_boundary, models/dilated_fcn.py:770-774): boundary[n,y,x] = 1 iff the max and the min of labels over the
 *     3x3 neighbourhood differ, neighbours outside the image ignored (max_pool2d(x, 3, 1, 1) != -max_pool2d(-x, 3, 1, 1)).  labels:
 *     int64 [N,H,W], or uint8 when labels_u8 != 0 (what mcdseg_predict_labels writes); every integer is just a value (no ignore
 *     index).  Any H, W; eight pixels per thread in 16-byte label loads when W % 8 == 0 and labels is 16-byte aligned.
 *   boundary_head (boundary_forward, :1118-1128, with upsample1-3 of :1050-1052): s1 [N,1,H/2,W/2], s2 [N,1,H/4,W/4],
 *     s3 [N,1,H/8,W/8] -> p [N,1,H,W] = (sigmoid(up2 s1) + sigmoid(up4 s2) + sigmoid(up8 s3)) / 3, bilinear, align_corners = False.
 *     H % 8 == 0, W % 8 == 0.  _bwd: dp -> ds1, ds2, ds3 in gather form (one thread per low-resolution pixel; sigmoid' is
 *     recomputed from the s maps, nothing is kept from the forward pass).
 *   bce2d (loss.py:131-138): beta = 1 - mean(t), w = 1 - beta + (2 beta - 1) t, loss = mean(w * bce(p, t)) in ONE pass over p and t:
 *     sum(w bce) = (1 - beta) sum(bce) + (2 beta - 1) sum(t bce), so beta needs no pass of its own.  out[0] = loss, out[1] = beta.
 *     target: uint8 {0,1} when target_u8 != 0, else fp32 (soft targets).  _bwd: dp = upstream/n * (p - t) / max(p (1 - p), 1e-12) * w in
 *     one pass; beta is out[1] of the forward call and upstream a device scalar (NULL: 1), both read on the device.  The target gets
 *     no gradient.  Edge arithmetic is that of today's F.binary_cross_entropy: bce = (t - 1) max(log1p(-p), -100) - t max(log p, -100)
 *     (so p exactly 0 or 1 is a legal input and costs 100 per wrong pixel), NOT the reference era's log(p + 1e-12) / log(1 - p + 1e-12):
 *     the two differ only for p within 1e-12 of 0 or 1, where the old form is bounded by 27.6 instead of 100.
 *   boundary_head_bce (get_boundary_loss(pred_type="boundary"), :743-787 via :1202-1204): the train path fused -- out as for bce2d with
 *     p = boundary_head(s1, s2, s3) and t = label_boundary(labels) (int64 labels, 16-byte aligned), neither stored; _bwd: one gather pass
 *     per scale straight to ds1, ds2, ds3, p and t recomputed at the contributing pixels.  Equal to the composition of the three entry
 *     points above: the gradients bit for bit, the loss up to the order of its partial sums.
 * workspace: mcdseg_bce2d_workspace_bytes(N*H*W) bytes, 8-byte aligned, for bce2d and boundary_head_bce_fwd alike.
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_label_boundary(const void* labels, int32_t labels_u8, uint8_t* boundary, int32_t N, int32_t H, int32_t W, void* stream);
int mcdseg_boundary_head_fwd(const float* s1, const float* s2, const float* s3, float* p, int32_t N, int32_t H, int32_t W, void* stream);
int mcdseg_boundary_head_bwd(const float* s1, const float* s2, const float* s3, const float* dp, float* ds1, float* ds2, float* ds3,
                             int32_t N, int32_t H, int32_t W, void* stream);
size_t mcdseg_bce2d_workspace_bytes(int64_t n);
int mcdseg_bce2d(const float* p, const void* target, int32_t target_u8, float* out, int64_t n, void* workspace, size_t workspace_bytes,
                 void* stream);
int mcdseg_bce2d_bwd(const float* p, const void* target, int32_t target_u8, const float* beta, const float* upstream, float* dp, int64_t n,
                     void* stream);
int mcdseg_boundary_head_bce_fwd(const float* s1, const float* s2, const float* s3, const int64_t* labels, float* out, int32_t N, int32_t H,
                                 int32_t W, void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_boundary_head_bce_bwd(const float* s1, const float* s2, const float* s3, const int64_t* labels, const float* beta,
                                 const float* upstream, float* ds1, float* ds2, float* ds3, int32_t N, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Boundary losses of the triple multitask decoder (MCDTripleMultiTaskDecoder, models/dilated_fcn.py:790-1024).  A target here is one
 * plane [H,W] per image, fp32 (soft targets in [0,1] allowed) or uint8 {0,1} when target_u8 != 0; image n's plane starts
 * n * target_batch_stride elements behind `target` (>= H*W: a channel of a wider batch is read in place).  Sums as above: fp64 block
 * partials, one small kernel, no float atomics, bitwise reproducible; nothing synchronises with the host.
 *   boundary_head_bce_target (get_boundary_loss, :1002-1004: bce2d(boundary_forward(x), gt_boundary)): mcdseg_boundary_head_bce with the
 *     target given instead of derived from labels, built from the same device functions -- the gradients equal the composition
 *     boundary_head -> bce2d bit for bit, the loss up to the order of its partial sums.  workspace: mcdseg_bce2d_workspace_bytes(N*H*W).
 *   seg2bd_bce (get_boundary_loss_by_extra_conv, :960-981, with seg2bd_conv = nn.Conv2d(C, 1, 5, padding=2) of :863-864): per head,
 *     u = bilinear8(z) (mcdseg_bilinear8_fwd's map, align_corners = False; 0 outside [0,H) x [0,W): the padding pads u, not z),
 *     v[n,y,x] = b + sum_{c,i,j} w[c,i,j] u[n,c,y+i-2,x+j-2], q = 1 / (1 + expf(-v)), loss = bce2d(q, t) as mcdseg_bce2d defines it.
 *     z1, z2 [N,C,Hi,Wi] are the two heads' low-resolution logits (z2 NULL: one head), H = 8 Hi, W = 8 Wi, w [1,C,5,5], b [1].
 *     out[0], out[1] = the heads' losses (out[1] = 0 with one head), out[2] = beta.  Both maps being linear, the channel sum is taken
 *     at LOW resolution (25 planes sum_c w[c,k] z[c] forward, 25 planes B^T(shifted dL/dv) backward): no C-channel full-resolution
 *     tensor exists in either pass; the workspace holds v and dL/dv (one plane per head each), the 25 planes and the partials.
 *     _bwd: bce2d_bwd -> sigmoid -> 5x5 transpose -> bilinear transpose with torch's clamp (-100) and eps (1e-12) as mcdseg_bce2d_bwd has
 *     them; beta = out + 2 of the forward call, upstream [2] = the two losses' incoming gradients (NULL: 1, 1), both read on the
 *     device; dz1, dz2 (NULL iff z2 is) in gather form, dw [1,C,5,5] and db [1] summed over both heads and all pixels in fp64.  _bwd
 *     needs the workspace its _fwd call left (v); it changes nothing _fwd wrote, so it may be repeated.
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_boundary_head_bce_target_fwd(const float* s1, const float* s2, const float* s3, const void* target, int32_t target_u8,
                                        int64_t target_batch_stride, float* out, int32_t N, int32_t H, int32_t W, void* workspace,
                                        size_t workspace_bytes, void* stream);
int mcdseg_boundary_head_bce_target_bwd(const float* s1, const float* s2, const float* s3, const void* target, int32_t target_u8,
                                        int64_t target_batch_stride, const float* beta, const float* upstream, float* ds1, float* ds2,
                                        float* ds3, int32_t N, int32_t H, int32_t W, void* stream);
size_t mcdseg_seg2bd_bce_workspace_bytes(int32_t N, int32_t C, int32_t Hi, int32_t Wi);
int mcdseg_seg2bd_bce_fwd(const float* z1, const float* z2, const float* w, const float* b, const void* target, int32_t target_u8,
                          int64_t target_batch_stride, float* out, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* workspace,
                          size_t workspace_bytes, void* stream);
int mcdseg_seg2bd_bce_bwd(const float* z1, const float* z2, const float* w, const float* b, const void* target, int32_t target_u8,
                          int64_t target_batch_stride, const float* beta, const float* upstream, float* dz1, float* dz2, float* dw,
                          float* db, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* workspace, size_t workspace_bytes, void* stream);

/* Scale(img_shape, Image.BILINEAR) / Scale(img_shape, Image.NEAREST) in front of the two transforms below (transform.py:303,
 * 320; torchvision's Scale = PIL.Image.resize) on uint8 batches: src [N,H,W,C] -> dst [N,OH,OW,C] (bilinear; Pillow's 8-bit
 * ImagingResample, bit for bit) and src [N,H,W] -> dst [N,OH,OW] (nearest; ImagingScaleAffine, for label maps).  workspace: 4-byte
 * aligned scratch of mcdseg_resize_workspace_bytes (coefficient / index tables built on the device + the image between the passes). */
size_t mcdseg_resize_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW);
int mcdseg_resize_bilinear_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW,
                              void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_resize_nearest_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW,
                             void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Either side of the step: input transform and evaluation histogram
 *   normalize_u8:   ToTensor() + Normalize(mean,std) (transform.py:302-315): src uint8 [N,H,W,Cs] (HWC) ->
 *                   dst fp32 [N,C,H,W], channels [c_off, c_off+Cs): ((u/255) - mean[c]) / std[c], IEEE division.
 *                   mean / std: device arrays of Cs floats.  RGB and HHA = two calls with c_off 0 and 3.
 *   relabel_u8:     ToLabel() + ReLabel(olabel -> nlabel) (transform.py:21-48, 319-325): uint8 -> int64
 *   confusion_hist: fast_hist (eval.py:21-23): hist[n*gt + pred] += 1 for 0 <= gt < n (pred outside [0,n) is
 *                   skipped, where numpy would fail on the reshape); hist is int64 [n*n], ACCUMULATED into.
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_normalize_u8(const uint8_t* src, float* dst, const float* mean, const float* std, int32_t N, int32_t H, int32_t W,
                        int32_t Cs, int32_t C, int32_t c_off, void* stream);
int mcdseg_relabel_u8(const uint8_t* src, int64_t* dst, int64_t count, int32_t olabel, int32_t nlabel, void* stream);
int mcdseg_confusion_hist(const int64_t* gt, const int64_t* pred, int64_t count, int32_t n, int64_t* hist, void* stream);

/* The joint transform of the trainers (joint_transforms.py:248-255, wired in at adapt_trainer.py:101-102 / source_trainer.py:82-83):
 * RandomHorizontallyFlip, RandomRotate(angle), RandomCrop(size) on an image and its label map together, as ONE gather from the
 * output pixel back to the loader's bytes, equal to Pillow's result byte for byte.  Per-sample parameters (drawn on the host) are two
 * device tables: affine [N][6] doubles = the matrix PIL.Image.rotate computes, and geom [N][10] int32 = {mode, flip, x1, y1,
 * fa0..fa5}: mode 0 copy, 1 affine, 2 / 3 / 4 Pillow's ROTATE_180 / ROTATE_90 / ROTATE_270 fast paths; (x1, y1) the crop corner;
 * fa* the 16.16 fixed-point matrix of Pillow's nearest path (affine_fixed).  A source position outside the image is 0.
 *   joint_augment_u8:           img.transpose(FLIP_LEFT_RIGHT).rotate(a, BILINEAR).crop(...) (joint_transforms.py:65, 137, 43):
 *                               src uint8 [N,H,W,Cs] -> dst uint8 [N,OH,OW,Cs]
 *   joint_augment_normalize_u8: the same followed by ToTensor() + Normalize (transform.py:302-315, use_crop: no Scale), i.e. by
 *                               normalize_u8: -> fp32 channels [c_off, c_off+Cs) of dst [N,C,OH,OW]; a fill pixel is byte 0 normalised
 *   joint_augment_label_u8:     mask.transpose(FLIP_LEFT_RIGHT).rotate(a, NEAREST).crop(...): src uint8 [N,H,W] -> dst uint8 [N,OH,OW];
 *                               the fill is label 0 (a real class), as in the reference.  H, W < 32768 (Pillow's fixed-point range).
 *   joint_augment_relabel_u8:   the same followed by ToLabel() + ReLabel (transform.py:319-325), i.e. by relabel_u8: -> int64 */
int mcdseg_joint_augment_u8(const uint8_t* src, uint8_t* dst, const double* affine, const int32_t* geom, int32_t N, int32_t H, int32_t W,
                            int32_t Cs, int32_t OH, int32_t OW, void* stream);
int mcdseg_joint_augment_normalize_u8(const uint8_t* src, float* dst, const float* mean, const float* std, const double* affine,
                                      const int32_t* geom, int32_t N, int32_t H, int32_t W, int32_t Cs, int32_t OH, int32_t OW, int32_t C,
                                      int32_t c_off, void* stream);
int mcdseg_joint_augment_label_u8(const uint8_t* src, uint8_t* dst, const int32_t* geom, int32_t N, int32_t H, int32_t W, int32_t OH,
                                  int32_t OW, void* stream);
int mcdseg_joint_augment_relabel_u8(const uint8_t* src, int64_t* dst, const int32_t* geom, int32_t N, int32_t H, int32_t W, int32_t OH,
                                    int32_t OW, int32_t olabel, int32_t nlabel, void* stream);

/* "Postprocess using Boundary Detection output" (sample_scripts/refine_seg_by_boundary.sh:15-17) on the device; all integer, exact.
 *   boundary_regions:         tools/binalize_boundary.py:9-20 (m = boundary > thre, strictly, inside a frame of ones) and
 *                             tools/apply_bwboundary.m:10-12 (bwboundaries: 8-connected objects, holes labelled, frame cropped):
 *                             boundary uint8 [N,H,W] -> regions int32 [N,H,W].  Pixels are joined iff their mask bits are equal and they
 *                             are 4-adjacent, or diagonal neighbours inside the mask.  regions = -1 for the frame object (every mask
 *                             component with a pixel on the image border: MATLAB's label 1), else the smallest row-major index y*W+x of
 *                             the pixel's component, per image.  Ids stay int32: the saturation at 255 of apply_bwboundary.m:15
 *                             (imwrite(L/255)) is not reproduced.  Lock-free union-find inside `regions`; ws is not used and may be null.
 *   refine_labels_by_regions: tools/refine_seg_by_bwboundary.py:34-42: out = the most common value of seg inside the pixel's region where
 *                             min_thre < pixels of the region < max_thre (strict) and the id is >= 0, else seg; ties go to the value whose
 *                             first pixel in row-major order comes earliest.  seg, out uint8 [N,H,W]; regions int32 [N,H,W], ANY map
 *                             with ids in [-1, H*W) (an id outside is read as -1).  Votes are taken from seg; out must not alias it.
 *   refine_workspace_bytes:   for refine_labels_by_regions, per image: 4*H*W (pixels per id, then its slot) + the vote table, one slot per
 *                             id that can be eligible -- H*W / (max(min_thre, 0) + 1) of them -- x 256 label values x {pixels, first
 *                             index} (8 bytes) + a winner byte per slot; each part padded to 16 bytes.  4-byte aligned. */
size_t mcdseg_refine_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t min_thre);
int mcdseg_boundary_regions(const uint8_t* boundary, int32_t thre, int32_t* regions, int32_t N, int32_t H, int32_t W, void* workspace,
                            size_t workspace_bytes, void* stream);
int mcdseg_refine_labels_by_regions(const uint8_t* seg, const int32_t* regions, uint8_t* out, int32_t N, int32_t H, int32_t W,
                                    int32_t min_thre, int32_t max_thre, void* workspace, size_t workspace_bytes, void* stream);

/* The fully connected CRF over saved logits (tools/crf.py:14-60 dense_crf, :63-66 softmax, :95-112 the driver) with the pairwise sums
 * taken exactly, not on pydensecrf's lattice (csrc/crf.hip).  Per image, N = H*W:
 *   U = -log_softmax(z) over C (finite where tools/crf.py:48 -log(softmax) gives inf); Q^0 = softmax(-U);
 *   Q^{t+1} = softmax(-U + w_g M_g(Q^t) + w_b M_b(Q^t)), M_i = n_i sum_j k(i,j) n_j Q_j, n_i = 1 / sqrt(sum_j k(i,j) + 1e-20),
 *   k(i,j) = exp(-0.5 |f_i - f_j|^2) with j = i included; f = (x/sx, y/sy) for the Gaussian term (crf.py:51-52) and
 *   (x/sx, y/sy, r/sr, g/sg, b/sb) for the bilateral one (crf.py:55-57), which exists only with an image.
 *   logits  fp32 [B,C,H,W] (what prob/<name>.npy holds, crf.py:95);  rgb uint8 [B,H,W,3] or NULL: no bilateral term (crf.py:53, :110);
 *   params  10 floats ON THE HOST in the order of crf.py:14-21: sxy_gaussian x, y; compat_gaussian; sxy_bilateral x, y;
 *           compat_bilateral; srgb_bilateral r, g, b; the tenth is reserved and not read.  n_iters (crf.py:14, :58) is an argument;
 *   q       fp32 [B,C,H,W] = Q^{n_iters}, may be NULL;  labels uint8 [B,H,W] = the arg-max over the first C_used classes (crf.py:112 takes
 *           19), the first maximum on a tie, may be NULL (not both).  n_iters = 0 returns softmax(z).
 * The Gaussian term is summed over |dx| <= ceil(7.5 sx), |dy| <= ceil(7.5 sy): a pair outside has k < exp(-28.125) < 2^-40, and what one
 * pixel loses altogether is below 1e-12 sx sy against a sum >= 1.  The bilateral term is summed over ALL pairs of an image.  Images of a
 * batch never pair.  fp32 throughout, no float atomics: the same bits run to run and for an image alone or in a batch.
 * -EINVAL before anything is launched: C outside [1, 64]; C_used outside [1, C]; n_iters < 0; a standard deviation that is not positive
 * and finite (the bilateral ones only with an image); H*W > 2^24, B*H*W*64 >= 2^31 or B > 65535 (what the index arithmetic covers);
 * a workspace smaller than mcdseg_dense_crf_workspace_bytes (4 x [B N][C up to 32 or 64] floats + n_g; with an image n_b and 8 feature
 * floats per pixel; each part padded to 256 bytes; 0 for dims that are refused) or not 16-byte aligned. */
size_t mcdseg_dense_crf_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_image);
int mcdseg_dense_crf(const float* logits, const uint8_t* rgb, const float* params, float* q, uint8_t* labels, int32_t C_used, int32_t B,
                     int32_t C, int32_t H, int32_t W, int32_t n_iters, void* workspace, size_t workspace_bytes, void* stream);

/* Depth -> HHA, the input encoding of every 6-channel path (horizontal disparity, height above ground, angle with gravity: Gupta,
 * Girshick, Arbelaez, Malik, ECCV 2014: saveHHA, processDepthImage, computeNormalsSquareSupport, getYDir) on the device
 * (csrc/hha.hip).  The procedure of DESIGN.md section 4.13 is the definition and tests/hha_ref.py its fp64 statement; nothing is
 * claimed about byte equality with the MATLAB release.  Per image, pixel (v, u) = (row, column), 0-based:
 *   Z = depth_cm (missing where <= 0 or not finite); a = (u - cx)/fx, b = (v - cy)/fy, P = (aZ, bZ, Z), q = 100/Z;
 *   normals for R = 3 and R = 10: a^2 ab a b^2 b 1 | aq bq q (0 at a missing pixel) summed over [v-R, v+R] x [u-R, u+R] clipped to the
 *   image -> M, t; n = adj(M) t; N = n/|n| with N_z >= 0; (0,0,0) where the window holds fewer than 3 valid pixels or |n| is 0 or not
 *   finite -- 0 meaning |n| <= 1e-14 max(sum a^2, sum b^2, count)^2 max|t|: valid pixels on one line leave only fp64 rounding noise
 *   (below 1e-15 of that scale).  The constant is meant for fx, fy up to about 1000 pixels: three adjacent pixels not on one line lie at
 *   6e-13 of the scale at fx = 520, 3e-14 at 1050 and reach 1e-14 at 1400, beyond which such a window counts as degenerate as well;
 *   g from the R = 10 normals: (0,1,0), then 5 iterations at 45 degrees and 5 at 15: F = {|g.N| > cos}, W = {|g.N| < sin},
 *   A = sum_W N N^T - sum_F N N^T, g' = the unit eigenvector of A's smallest eigenvalue with g.g' >= 0 (g stays when both sets are empty);
 *   h = -g.P - y_min, y_min = the smallest -g.P of a valid pixel, or -130 where that is > -90;
 *   bytes 31000/max(Z,100) | h | acosd(clamp(N3.g, -1, 1)) + 38 (0 where N3 is invalid), rounded half away from zero, saturated to [0,255].
 *   depth_cm  fp32 [N,H,W] centimetres, 4-byte aligned;
 *   camera    fp32 [N][4] = fx fy cx cy per image, ON THE HOST (read before the call returns; fx and fy are checked there);
 *   hha       uint8 [N,H,W,3] in the order disparity, height, angle; a missing pixel is (0,0,0);
 *   normals3  fp32 [N,H,W,3], the R = 3 normals (at missing pixels too), may be NULL;  gravity fp32 [N][3], may be NULL;
 *   height    fp32 [N,H,W], h before rounding, 0 at a missing pixel, may be NULL.
 * fp64 arithmetic throughout (the optional outputs are rounded once), no atomics, every sum in an order that depends on H and W alone:
 * the same bits run to run, beside another process, and for an image alone or in a batch.  g stays on the device: the ten iterations
 * run without a host synchronisation.
 * -EINVAL before anything is launched: a null depth, camera, hha or workspace; a dimension < 1; N > 65535 (one image per grid row);
 * H*W > 2^24 or N*H*W*3 >= 2^31 (what the index arithmetic covers); fx or fy not positive and finite, cx or cy not finite; a workspace
 * smaller than mcdseg_depth_to_hha_workspace_bytes (the cameras, g and y_min in fp64, the block partials, and both normal maps in
 * fp64: 48 bytes per pixel; each part padded to 256 bytes; 0 for dims that are refused) or not 16-byte aligned; an output or the
 * depth not 4-byte aligned. */
size_t mcdseg_depth_to_hha_workspace_bytes(int32_t N, int32_t H, int32_t W);
int mcdseg_depth_to_hha(const float* depth_cm, const float* camera, uint8_t* hha, float* normals3, float* gravity, float* height, int32_t N,
                        int32_t H, int32_t W, void* workspace, size_t workspace_bytes, void* stream);

/* Depth inpainting by colorization (Levin, Lischinski, Weiss, SIGGRAPH 2004, as the NYU Depth toolbox's fill_depth_colorization applies
 * it: the step between a sensor's raw depth and the maps the published HHA images were made from) on the device (csrc/fill.hip).  The
 * procedure of DESIGN.md section 4.16 is the definition and tests/fill_ref.py its fp64 statement; nothing is claimed about byte
 * equality with the MATLAB toolbox.  Per image of H*W >= 2 pixels:
 *   known where depth_cm is finite, > 0 and, with max_valid_cm > 0, < max_valid_cm; g = ((0.299 R + 0.587 G) + 0.114 B) / 255;
 *   zmax = the largest known depth, z = depth / zmax; an image without a known pixel is MCDSEG_FILL_EMPTY: not solved, all zeros;
 *   weights over the 3 x 3 neighbours q of p inside the image, in row-major order: mu and the population variance var of g over them
 *   and p; sigma = max(0.6 var, min_q (g_q - g_p)^2 / ln 100, 2e-6); w_pq = exp(-(g_q - g_p)^2 / sigma) / their sum;
 *   the system (1 + alpha k_p) x_p - sum_q w_pq x_q = alpha k_p z_p (k = 1 at known pixels, else 0): M x = b, D = diag(M);
 *   BiCGSTAB right-preconditioned by D from x0 = b/D, r = rhat = b - M x0, rho = a = omega = 1, v = p = 0; per iteration
 *   rho' = rhat.r, beta = (rho'/rho)(a/omega), p = r + beta (p - omega v), v = M(p/D), a = rho'/(rhat.v), s = r - a v, t = M(s/D),
 *   omega = (t.s)/(t.t), x += a (p/D) + omega (s/D), r = s - omega t;  filled = (float)(x zmax).
 * Three calls share one workspace of mcdseg_fill_depth_workspace_bytes (one record per image, the block partials, the known depth in
 * fp32, the eight weight planes and x r rhat p v s t b in fp64: 132 bytes per pixel; each part padded to 256 bytes; 0 for dims that are
 * refused); the solver's scalars stay in it, on the device, and no call synchronises:
 *   mcdseg_fill_depth_setup    rgb uint8 [N,H,W,3]; depth_cm fp32 [N,H,W], 4-byte aligned; alpha > 0 (the toolbox's is 1);
 *                              max_valid_cm 0 for none.  Writes every part of the workspace the later calls read.
 *   mcdseg_fill_depth_iterate  enqueues n_iter iterations, then one check of the TRUE residual b - M x: an image whose residual 2-norm is
 *                              <= rtol |b| becomes MCDSEG_FILL_CONVERGED.  Only MCDSEG_FILL_RUNNING images are touched: every workgroup of
 *                              another image returns at once, so an image's result and its iteration count are the same bits alone or
 *                              beside slower images.  A zero or non-finite rho', rhat.v or t.t makes the image MCDSEG_FILL_BREAKDOWN
 *                              with x the iterate of the last completed iteration.  n_iter = 0 is the check alone (the one before the
 *                              first iteration).  status_out: N records { int32 status; int32 iterations; double |b - M x| / |b| } in
 *                              device memory, 8-byte aligned, written for every image by every call (the residual is that of the
 *                              image's last check; 0 for an empty image).  Stopping at an iteration limit is the caller's business.
 *   mcdseg_fill_depth_finish   filled fp32 [N,H,W] centimetres at every pixel; with keep_known a known pixel gets its depth_cm back bit
 *                              for bit; x_f64 [N,H,W], weights_f64 [N,8,H,W] (0 for a neighbour outside the image) and zmax_f64 [N] may
 *                              be NULL.
 * fp64 arithmetic, no atomics, plain launches in stream order (no grid barrier, no cooperative launch), every sum in an order that
 * depends on H and W alone: the same bits run to run.
 * -EINVAL before anything is launched: a null rgb, depth, status_out, filled or workspace; a dimension < 1; N > 65535; H*W < 2 or
 * > 2^24; alpha or rtol not positive and finite; max_valid_cm negative or NaN; n_iter outside [0, 65536]; a workspace smaller than
 * mcdseg_fill_depth_workspace_bytes or not 16-byte aligned; depth or filled not 4-byte aligned, status_out or an fp64 output not 8-byte
 * aligned. */
#define MCDSEG_FILL_RUNNING 0
#define MCDSEG_FILL_CONVERGED 1
#define MCDSEG_FILL_EMPTY 2
#define MCDSEG_FILL_NOT_CONVERGED 3 /* never written by the library: what a caller reports for an image still running at its limit */
#define MCDSEG_FILL_BREAKDOWN 4
size_t mcdseg_fill_depth_workspace_bytes(int32_t N, int32_t H, int32_t W);
int mcdseg_fill_depth_setup(const uint8_t* rgb, const float* depth_cm, double alpha, double max_valid_cm, int32_t N, int32_t H, int32_t W,
                            void* workspace, size_t workspace_bytes, void* stream);
int mcdseg_fill_depth_iterate(int32_t n_iter, double rtol, int32_t N, int32_t H, int32_t W, void* workspace, size_t workspace_bytes,
                              void* status_out, void* stream);
int mcdseg_fill_depth_finish(int32_t N, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, float* filled, double* x_f64,
                             double* weights_f64, double* zmax_f64, int32_t keep_known, void* stream);

/* Ensembling of saved predictions (tools/ensemble_predict_from_npy.py:17-56 ensemble_predict) on the device (csrc/ensemble.hip;
 * DESIGN.md section 4.14).  All of it is exact: fp32 additions in a stated order, one division, comparisons, integer gathers.
 *
 * mcdseg_ensemble_probs: K maps of the same N images, combined per element and arg-maxed per pixel in one pass.
 *   maps     K device pointers ON THE HOST (read before the call returns), each fp32 [N][C][H][W], 4-byte aligned: the K uploads as they
 *            stand, no [K,C,H,W] copy is made.  2 <= K <= MCDSEG_ENSEMBLE_MAX_K (16: the pointers travel as a kernel argument);
 *   method   MCDSEG_ENSEMBLE_AVERAGING: sum(probs) / len(probs) as numpy evaluates it (:24): ((0 + p0) + p1) + ... left to right in fp32
 *            -- the leading integer 0 is Python's, so a -0.0 leaves as +0.0 -- then ONE correctly rounded fp32 division by K: no
 *            reciprocal, no contraction;
 *            MCDSEG_ENSEMBLE_NMS: np.max(probs, 0) (:26): m = m > p ? m : p left to right (of +0 and -0 the later one stays, as in
 *            numpy's maximum); a NaN in any map wins;
 *            a NaN result of either leaves as 0x7FC00000 whatever its inputs' payloads were (IEEE leaves the payload of a NaN that an
 *            addition makes to the implementation: numpy's is the host's, 0xFFC00000 on x86).  This holds for NMS too, where numpy
 *            only hands an input NaN through: the payload and sign of an INPUT NaN are NOT preserved under either method;
 *   out      fp32 [N][C][H][W], the combined map, or NULL: nothing is stored and only the first n_used classes are formed, in registers;
 *   labels   uint8 [N][H][W] = argmax over c < n_used of out[c] by numpy's rule (:32): the first maximum wins, a NaN counts as the
 *            maximum and the first NaN wins, +0 and -0 are equal.
 * Four pixels per thread in 16-byte accesses when W % 4 == 0 and every pointer (maps, out, labels) is 16-byte aligned, one pixel per thread
 * otherwise: the same bits.  Plain stores, no atomics: the same bits run to run, for an image alone or in a batch.
 * -EINVAL before anything is launched: a null maps, map or labels; K outside [2, 16]; an unknown method; a dimension < 1; N > 65535;
 * n_used outside [1, min(C, 256)]; H*W >= 2^31 or N*C*H*W >= 2^40; a map or out not 4-byte aligned.
 *
 * mcdseg_label_resize_colorize: Image.resize((OW, OH), NEAREST) of the label map (:33-35) and of its palette image (:43-56) as one gather.
 *   labels     uint8 [N][H][W];  palette uint8 [n_pal][3] in device memory, 1 <= n_pal <= 256 (needed only with vis_out);
 *   label_out  uint8 [N][OH][OW] = labels[iy[y]][ix[x]], ix / iy being Pillow's NEAREST source indices -- the rule of
 *              mcdseg_resize_nearest_u8, computed by the same kernel -- may be NULL;
 *   vis_out    uint8 [N][OH][OW][3] = palette[label_out], (0,0,0) for a label >= n_pal (Colorize.__call__, transform.py:155-165), may be
 *              NULL (not both).
 * -EINVAL before anything is launched: a null labels or workspace; no output; vis_out without a palette of 1..256 colours; a dimension
 * < 1; N*H*W or N*OH*OW >= 2^40; a workspace smaller than mcdseg_label_resize_colorize_workspace_bytes ((OH + OW) ints; 0 for dims that are
 * refused) or not 4-byte aligned. */
#define MCDSEG_ENSEMBLE_MAX_K 16
#define MCDSEG_ENSEMBLE_AVERAGING 0
#define MCDSEG_ENSEMBLE_NMS 1
int mcdseg_ensemble_probs(const float* const* maps, int32_t K, int32_t method, float* out, uint8_t* labels, int32_t n_used, int32_t N,
                          int32_t C, int32_t H, int32_t W, void* stream);
size_t mcdseg_label_resize_colorize_workspace_bytes(int32_t OH, int32_t OW);
int mcdseg_label_resize_colorize(const uint8_t* labels, const uint8_t* palette, int32_t n_pal, uint8_t* label_out, uint8_t* vis_out,
                                 int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* Edge maps of RGB images (tools/edge_detect.py:33-53 of the reference: the luma plane, cv2.Laplacian + 128, the Sobel magnitude and
 * cv2.Canny; sample_scripts/refine_seg_by_boundary.sh:6 takes BOUNDARY_DIR = .../edges/canny from it) on the device (csrc/edge.hip;
 * DESIGN.md section 4.15).  The definition is OpenCV's published 8-bit algorithm, all integer: no OpenCV build was at hand, so byte
 * equality with a particular OpenCV build is neither claimed nor tested -- tests/edge_ref.py is the yardstick, bit for bit.
 *
 * mcdseg_edge_maps: ONE launch for whatever is asked.
 *   rgb        uint8 [N][H][W][3], R, G, B;
 *   luma       uint8 [N][H][W] = Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 (cvtColor(BGR2YUV)[:,:,0]); written only when given;
 *   laplacian  clip(Y[y-1][x] + Y[y+1][x] + Y[y][x-1] + Y[y][x+1] - 4 Y[y][x] + 128, 0, 255), BORDER_REFLECT_101 (-1 -> 1, L -> L - 2, a
 *              dimension of length 1 -> 0);
 *   sobel      min(floor(sqrt(dx^2 + dy^2)), 255), dx = the correlation with [[-1,0,1],[-2,0,2],[-1,0,1]], dy with its transpose,
 *              BORDER_REFLECT_101;
 *   canny_cls  0 / 1 (weak) / 2 (strong): dx, dy as above but BORDER_REPLICATE, mag = |dx| + |dy|, 0 outside the image; low > high are
 *              swapped; mag <= low is 0; else with x = |dx|, y = |dy| << 15, t22 = 13573 x, t67 = t22 + (x << 16): y < t22 keeps
 *              mag > left && mag >= right; y > t67 keeps mag > upper && mag >= lower; else, s = (dx ^ dy) < 0 ? -1 : 1, keeps
 *              mag > mag[y-1][x-s] && mag > mag[y+1][x+s]; a kept pixel is 2 if mag > high, else 1;
 *   each output may be NULL (not wanted), not all four; low and high are read only with canny_cls.
 * -EINVAL before anything is launched: a null rgb; no output; a dimension < 1; N*H*W >= 2^31; N > 65535; more than 65535 tile rows.
 *
 * mcdseg_canny_hysteresis: edges uint8 [N][H][W] = 255 where cls is 1 or 2 and the pixel's 8-connected component of such pixels holds a
 * 2, else 0 (any other value of cls reads as 0).  Connected components by the union-find of mcdseg_boundary_regions; the same bits run
 * to run.  workspace: mcdseg_canny_hysteresis_workspace_bytes = 4*N*H*W (0 for dims that are refused); what it held does not matter.
 * -EINVAL before anything is launched: a null cls or edges; edges == cls; the dims above; a workspace that is null, not 4-byte
 * aligned or too small. */
int mcdseg_edge_maps(const uint8_t* rgb, uint8_t* luma, uint8_t* laplacian, uint8_t* sobel, uint8_t* canny_cls, int32_t low,
                     int32_t high, int32_t N, int32_t H, int32_t W, void* stream);
size_t mcdseg_canny_hysteresis_workspace_bytes(int32_t N, int32_t H, int32_t W);
int mcdseg_canny_hysteresis(const uint8_t* cls, uint8_t* edges, int32_t N, int32_t H, int32_t W, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2-byte activation storage (round 6): BASELINE config 5 ("drn_d_105 ... bf16 ... HBM-bound stress"; the network is the reference's
 * Bottleneck trunk, models/drn.py:62-100, 344-348, trained by adapt_trainer.py:155-220).  In the one-term arithmetic MCDSEG_MATH_F16X1
 * a fused conv + BatchNorm (+ residual) + ReLU group inside a trunk keeps ONE 16-bit value per element of every tensor it moves, all in
 * the companions' unit layout [N][C/8][H*W][8 x 16 bit] (one 16-byte unit = 8 channels of one pixel):
 *   z16    the convolution's output: fp16 of z / scale(z_bound), z_bound = KH KW Cin x_bound w_bound written by the convolution (|z| cannot
 *          exceed it; scale(b) = 2^(e-15), 2^e >= b, as for every F16X3 / F16X1 tensor).  fp16 rather than bf16: 11 significant bits
 *          against 8 where the per-tensor scale keeps the values in range, which a bound known before the tensor is written does;
 *   y_cb   the activation: the leading piece of the F16X3 companion, alone -- it IS the next convolution's operand;
 *   dy16   the gradient arriving from the consumers: bf16 -- gradients span more binades than one scale covers and have no a-priori
 *          bound; written by mcdseg_conv_split_dgrad_half (+ addend16: the other gradient of a residual block's input, same layout);
 *   dz_cb  the leading piece of dz's companion (scale from dz_bound, as in mcdseg_bn_bwd_reduce); dres16: dy16 under the ReLU mask.
 * mean / rstd / running statistics come from the convolution's fp32 accumulators through mcdseg_bn_stats_finalize as always; all
 * BatchNorm arithmetic is fp32.  mask_kind: 0 no ReLU; 2 y > 0 recomputed from z16 (a group without residual: the forward kernel's own
 * expression on the same stored z, so the same mask); 4 from y_cb (a group with residual).
 * F16X1 reads the LEADING piece of every companion only (piece stride 0), so one- and two-piece companions mix freely.
 * ---------------------------------------------------------------------------------------------- */
int32_t mcdseg_conv_split_half_ok(const mcdseg_conv_desc* d, int32_t math, int32_t dgrad);
/* Which kernels a call will launch, for profilers and bench.py's per-kernel tables (the host side derives rocprofv3's kernel names from
 * these instead of restating the dispatch): mcdseg_up8_loss_variant = the class count of mcdseg_up8_softmax_ce_l1's LDS-DMA instantiation
 * (16, 24, 41, 48) or minus that of the register-staged kernel (labelled: 0 no labels, 1 labels at a 16-byte aligned address, 2 labels at
 * an address that is only 8-byte aligned -- the LDS-DMA kernel fetches labels in 16-byte units, so those run the register-staged kernel);
 * mcdseg_conv_wgrad_thin_tr_config = the template arguments
 * <cin8, mt, ntl, tr> of the thin layers' window weight gradient as cin8 * 1000000 + mt * 10000 + ntl * 100 + tr (0: not that kernel). */
int32_t mcdseg_up8_loss_variant(int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t labelled);
int32_t mcdseg_conv_wgrad_thin_tr_config(const mcdseg_conv_desc* d);
/* 1 when the 8-wave ping-pong launches of this convolution run with two K-steps of 16 channels per barrier interval (MCDSEG_MATH_F16X1 with
 * an even number of K-steps; kernel policy SplitF16x1D in profiles): the same products in the same order as the one-step kernel. */
int32_t mcdseg_conv_split_pp_deep(const mcdseg_conv_desc* d, int32_t math, int32_t dgrad);
int mcdseg_conv_split_fprop_half(const mcdseg_conv_desc* d, int32_t math, const void* x_cb, const float* x_bound, const void* wp_fprop,
                                 const float* w_bound, void* z16, float* z_bound, float* stat_partials, int32_t part, void* stream);
int mcdseg_conv_split_dgrad_half(const mcdseg_conv_desc* d, int32_t math, const void* dy_cb, const float* dy_bound, const void* wp_dgrad,
                                 const float* w_bound, const void* addend16, void* dx16, int32_t part, void* stream);
int mcdseg_bn_apply_half(const void* z16, const float* z_bound, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const void* res_cb, const float* res_bound, void* y_cb, const float* y_bound, int32_t N, int32_t C, int32_t HW,
                         int32_t relu, void* stream);
size_t mcdseg_bn_bwd_half_workspace_bytes(int32_t N, int32_t C, int32_t HW);
int mcdseg_bn_bwd_reduce_half(const void* dy16, const void* y_cb, const void* z16, const float* z_bound, const float* mean,
                              const float* rstd, const float* gamma, const float* beta, float* dgamma, float* dbeta, float* dz_bound,
                              int32_t mask_kind, int32_t train, int32_t N, int32_t C, int32_t HW, void* workspace, size_t workspace_bytes,
                              void* stream);
int mcdseg_bn_bwd_apply_half(const void* dy16, const void* y_cb, const void* z16, const float* z_bound, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, const float* dgamma, const float* dbeta, void* dz_cb,
                             const float* dz_bound, void* dres16, int32_t mask_kind, int32_t train, int32_t N, int32_t C, int32_t HW,
                             void* stream);
/* fp32 NCHW <-> bf16 units: a gradient crossing the border of the 2-byte chain through a kernel without the 16-bit epilogue */
int mcdseg_pack_bf16_units(const float* x, void* out16, int32_t N, int32_t C, int32_t HW, void* stream);
int mcdseg_unpack_bf16_units(const void* in16, float* x, int32_t N, int32_t C, int32_t HW, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SGD with momentum + weight decay on flat buffers (torch.optim.SGD via models/model_util.py:289-292)
 *   d = g*grad_scale + wd*p ; v = mu*v + d ; p -= lr*v        (v starts at 0, so the first v = d)
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_sgd_momentum_flat(float* p, const float* g, float* v, int64_t n, float lr, float momentum,
                             float weight_decay, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam with L2 weight decay on flat buffers (torch.optim.Adam via models/model_util.py:293-294: no amsgrad, no maximize,
 * no decoupled decay).  The caller forms the bias corrections of step t in double precision and passes
 * lr_over_bc1 = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t); the kernel reads no step counter.
 *   d = g*grad_scale + wd*p ; m += (1-beta1)*(d - m) ; v = beta2*v + (1-beta2)*d*d     (m in the form of torch's lerp)
 *   p -= lr_over_bc1 * m / (sqrt(v)*inv_sqrt_bc2 + eps)                                  (m and v start at 0)
 * 1 - beta is formed in double precision from the decimal the float stands for when beta has at most six decimals
 * (0.5, 0.9, 0.999, ...), from the float itself otherwise.  28 B per parameter.
 * ---------------------------------------------------------------------------------------------- */
int mcdseg_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr_over_bc1, float beta1, float beta2,
                     float inv_sqrt_bc2, float eps, float weight_decay, float grad_scale, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* MCDSEG_H */
