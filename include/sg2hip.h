/*
 * sg2hip -- C-ABI of the MI355X (gfx950) kernels of the StyleGAN2-ADA training hot path.
 *
 * The library (libsg2hip.so, built from gan-track_amd/csrc) replaces the reference's two
 * pybind11 CUDA plugins and the cuDNN convolutions reached through conv2d_gradfix:
 *
 *   reference (ltronchin/Gan-track, src/models/stylegan3 = SG3/)          replaced by
 *   SG3/torch_utils/ops/bias_act.cpp:32   bias_act(x,b,xref,yref,dy,grad,dim,act,alpha,gain,clamp)
 *                                                                          -> sg2_bias_act
 *   SG3/torch_utils/ops/upfirdn2d.cpp:16  upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)
 *                                                                          -> sg2_upfirdn2d
 *   SG3/torch_utils/ops/conv2d_gradfix.py:37-45 (F.conv2d / F.conv_transpose2d, cuDNN)
 *                                                                          -> sg2_conv2d (fwd + dgrad)
 *   autograd weight gradient of those convolutions (cuDNN wgrad)          -> sg2_conv2d_wgrad
 *   SG3/torch_utils/ops/grid_sample_gradfix.py:28-65 (aten grid_sampler_2d fwd/bwd)
 *                                                                          -> sg2_grid_sample_fwd / _bwd
 *   SG3/training/networks_stylegan2.py:59-63 demodulation coefficients    -> sg2_demod_fwd / _bwd
 *   SG3/training/training_loop_mi_multimodal.py:341-351 (flat grad, /N, nan_to_num, torch.optim.Adam)
 *                                                                          -> sg2_adam_multi
 *   SG3/training/training_loop_mi_multimodal.py:358-366 (G_ema lerp)      -> sg2_lerp_multi
 *
 * Conventions
 *  - Every pointer is a device pointer; the library never allocates or frees device memory.
 *  - Mutable state: three mode switches, set between launches and read by every later launch --
 *      sg2_set_deterministic (PROCESS-WIDE: the caller's scratch arena for fixed-order slot reductions; process-
 *        wide because autograd runs a deterministic scope's backward on its own device thread),
 *      sg2_set_zeroed_accumulators, sg2_set_clean_workspace (PER HOST THREAD),
 *    plus the per-thread sg2_last_error() message.  Otherwise the kernels are re-entrant and capturable into a
 *    hipGraph; do not change the process-wide deterministic arena while another thread is launching.
 *  - `stream` is a hipStream_t (pass the caller's current stream; NULL = default stream).
 *  - dtype codes: SG2_F32 = 0, SG2_F16 = 1, SG2_BF16 = 2 (arithmetic is always f32 internally).
 *  - 4-D activations are NHWC in memory (torch channels_last); sizes are given as [N, C, H, W]
 *    like the reference, strides (in elements) as [sN, sC, sH, sW] where a function accepts strides.
 *  - Return value: 0 = success, < 0 = invalid argument (see sg2_last_error()), > 0 = hipError_t of
 *    the launch.  The Python wrapper raises RuntimeError with sg2_last_error() -- the same behaviour
 *    as the reference's TORCH_CHECK / AT_CUDA_CHECK.
 */
#ifndef SG2HIP_H
#define SG2HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG2_ABI_VERSION 11

enum sg2_dtype { SG2_F32 = 0, SG2_F16 = 1, SG2_BF16 = 2, SG2_F32S3 = 3 };

/* SG2_F32S3 (ABI 5): float32 operands handed over PRE-SPLIT as three bf16 planes h, m, l (x = h + m + l, exact
 * for normal floats; sg2_split3), each plane the tensor's element order, the planes back to back.  Accepted as
 * the operand dtype of sg2_conv2d / sg2_conv2d_fused (x and w; the output, epilogue and workspace are float32;
 * Cin % 8 == 0; in_scale must be folded into x's planes) and of sg2_conv2d_wgrad (g and x; A, B % 8 == 0;
 * scales folded in).  The f32 convolutions then run the split form's six bf16 MFMA products on operands split
 * once per call instead of once per workgroup that stages them.
 *
 * planes[p * n + i] = piece p of x[i] * scale[(i / C) / pix_per_n, i % C]   (scale NULL = 1; x f32, n elements,
 * C % 8 == 0, 16-byte aligned) */
int sg2_split3(void* planes, const float* x, int64_t n, int C, int64_t pix_per_n, const float* scale, void* stream);

/* ABI version of the loaded library (SG2_ABI_VERSION). */
int sg2_abi_version(void);

/* Message of the last failing call on this host thread ("" if none). */
const char* sg2_last_error(void);

/* Fused bias + activation + gain + clamp, and its 1st/2nd order gradients.
 * Replaces SG3/torch_utils/ops/bias_act.cpp:32 (kernel semantics bias_act.cu:23-147).
 *   y[i] = f(x[i], b[(i / step_b) % size_b], ...) for i < numel.
 *   grad = 0: y = clamp(act(x + b) * gain)
 *   grad = 1: y = x * act'(...) * gain masked by |yref| < clamp     (x holds dL/dy)
 *   grad = 2: second-order term (needs dy, the first-order incoming gradient)
 * b / xref / yref / dy may be NULL (absent, like the reference's empty tensor).
 * numel == 0 is a no-op whatever the pointers are (an empty tensor has no storage).
 * act: 1 linear, 2 relu, 3 lrelu, 4 tanh, 5 sigmoid, 6 elu, 7 selu, 8 softplus, 9 swish
 * (the reference's cuda_idx, bias_act.py:21-31).  clamp < 0 disables clamping. */
int sg2_bias_act(void* y, const void* x, const void* b, const void* xref, const void* yref, const void* dy,
                 int dtype, int64_t numel, int64_t size_b, int64_t step_b, int grad, int act, float alpha,
                 float gain, float clamp, void* stream);

/* Upsample (zero insertion), pad/crop, 2-D FIR, downsample.
 * Replaces SG3/torch_utils/ops/upfirdn2d.cpp:16 (semantics upfirdn2d.py:118-211).
 *   in/out sizes [N, C, H, W], strides in elements (any layout); f is a float32 [fh, fw] filter
 *   (row-major, device).  flip = 0: true convolution (filter flipped), 1: correlation.
 *   Output size must equal ((in*up + pad0 + pad1 - f) / down) + 1 per axis. */
int sg2_upfirdn2d(void* y, const void* x, const float* f, int dtype, const int64_t* in_size,
                  const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride, int fw, int fh,
                  int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip,
                  float gain, void* stream);

/* sg2_upfirdn2d of a dynamically sized image held at the origin of a static buffer (the ADA pipe's padded
 * image, augment_mi.py:288-321, whose size is data dependent): lim = device int[2] output extent (rows,
 * cols).  Outputs inside it are computed, outputs within 32 rows / cols beyond it are written as zeros
 * (exact when the image's support ends inside the extent), the rest of y is left unwritten.  Generic
 * (any-stride) kernel. */
int sg2_upfirdn2d_lim(void* y, const void* x, const float* f, int dtype, const int64_t* in_size,
                      const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride, int fw, int fh,
                      int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip,
                      float gain, const int* lim, void* stream);

/* sg2_upfirdn2d followed by the fused layer epilogue (sg2_epilogue, defined below) -- the FIR of
 * an up-2 synthesis layer with its demodulation, noise, bias, lrelu and clamp
 * (networks_stylegan2.py:68-76 + :325-327).  epi may be NULL; with an epilogue the activations
 * must be NHWC with C % 8 == 0 (C % 4 for f32). */
typedef struct sg2_epilogue sg2_epilogue;
int sg2_upfirdn2d_fused(void* y, const void* x, const float* f, int dtype, const int64_t* in_size,
                        const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride, int fw, int fh,
                        int upx, int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip,
                        float gain, const sg2_epilogue* epi, void* stream);

/* Dense 2-D convolution on NHWC activations (implicit GEMM on MFMA).
 *   transpose = 0: y = conv2d(x, w, stride, padding)            (torch.nn.functional.conv2d)
 *                  w packed [Cout][KH][KW][Cin]  (= OIHW weight in channels_last memory)
 *   transpose = 1: y = conv_transpose2d(x, w, stride, padding)  (torch.nn.functional.conv_transpose2d)
 *                  w packed [Cout][KH][KW][Cin]  (= the [Cin, Cout, KH, KW] torch weight permuted (1,2,3,0))
 *   x [N, H, W, Cin], y [N, OH, OW, Cout] (OH/OW explicit: output_padding is implied).
 *   workspace: float32 scratch of >= N*OH*OW*Cout elements, or NULL (then no split-K is used). */
int sg2_conv2d(void* y, const void* x, const void* w, int dtype, int N, int Cin, int H, int W, int Cout,
               int OH, int OW, int KH, int KW, int stride, int pad_y, int pad_x, int transpose,
               float* workspace, int64_t workspace_elems, void* stream);

/* Fused epilogue of sg2_conv2d_fused (all pointers optional):
 *   z   = clamp(act(c * out_scale[n,o] + noise[n,oy,ox] * noise_gain + bias[o]) * gain, +-clamp)
 *   y   = round(z) + residual[n,oy,ox,o]          (residual: the resnet skip of the D block)
 *   aux = c (aux_mode 1) or z (aux_mode 2)        (saved for the fused backward)
 *   dot_out[n,o] = sum_{oy,ox} c * dot_src        (the modulation gradient when the call is a dgrad)
 * Replaces the fma / bias_act / add passes the reference runs after each conv
 * (networks_stylegan2.py:68-76, :172-181, :621-627). */
struct sg2_epilogue {
    const float* out_scale;  /* [N, Cout] float32 */
    const void* noise;       /* [N, OH, OW], activation dtype */
    const float* bias;       /* [Cout] float32, added rounded to the activation dtype (the reference's b.to(x.dtype)) */
    const void* residual;    /* [N, OH, OW, Cout] NHWC, activation dtype */
    void* aux;               /* [N, OH, OW, Cout] NHWC, activation dtype */
    float noise_gain, alpha, gain, clamp;   /* clamp < 0: off */
    int act;                 /* 0 linear, 1 lrelu(alpha) */
    int aux_mode;            /* 0 none, 1 conv result c, 2 activation z */
    const void* dot_src;     /* [N, OH, OW, Cout] or NULL (sg2_conv2d_fused only; needs aux_mode 0 or 1) */
    float* dot_out;          /* [N, Cout] float32: sum over pixels of c * dot_src, zeroed by the call */
};

/* sg2_conv2d with the A operand modulated by in_scale[n, ci] (float32 [N, Cin], or NULL) and the
 * fused epilogue above (epi may be NULL = plain convolution).  Transposed convolutions run all their
 * stride x stride output phases in one launch (up to 4 phases per launch). */
int sg2_conv2d_fused(void* y, const void* x, const void* w, int dtype, int N, int Cin, int H, int W, int Cout,
                     int OH, int OW, int KH, int KW, int stride, int pad_y, int pad_x, int transpose,
                     const float* in_scale, const sg2_epilogue* epi, float* workspace, int64_t workspace_elems,
                     void* stream);

/* 3x3 / stride 1 / pad 1 convolution of 16-bit NHWC activations with an LDS halo tile, optional
 * modulation of the input and the fused StyleGAN2 layer epilogue (networks_stylegan2.py:309-328):
 *   c      = conv(x[n,:,:,ci] * in_scale[n,ci], w)          w packed [Cout][3][3][Cin], Cin % 8 == 0
 *   y_raw  = c                                              (optional second output, may be NULL)
 *   y      = clamp(act(c * out_scale[n,o] + noise[n,y,x] * noise_gain + bias[o]) * gain, +-clamp)
 * in_scale / out_scale / bias are float32 (NULL = off); noise has the activation dtype, [N,H,W]
 * (NULL = off); act 0 = linear, 1 = lrelu(alpha); clamp < 0 = off.  dtype: SG2_F16 or SG2_BF16.
 * dot_src / dot_out (both or neither): dot_out[n,o] = sum_{y,x} c[n,y,x,o] * dot_src[n,y,x,o] (float,
 * zeroed by the call) -- the modulation gradient of the layer when this kernel runs its dgrad. */
int sg2_conv3x3(void* y, void* y_raw, const void* x, const void* w, int dtype, int N, int Cin, int H, int W,
                int Cout, const float* in_scale, const float* out_scale, const void* noise, float noise_gain,
                const float* bias, int act, float alpha, float gain, float clamp, const void* dot_src,
                float* dot_out, void* stream);

/* While on (per host thread), the entry points below skip zeroing their float accumulator outputs --
 * sg2_conv2d_fused / sg2_conv3x3 / sg2_conv3x3_s2 dot_out, sg2_conv2d_wgrad dw, sg2_layer_bwd db / dd --
 * because the caller zeroed them (one fill for all of a layer's accumulators instead of one memset per
 * call).  Default off. */
void sg2_set_zeroed_accumulators(int on);

/* While on (per host thread), the split-K f32 workspace passed to sg2_conv2d / sg2_conv2d_fused is zero on
 * entry and is left zero on return (the finalize pass clears what it read), so a split-K call issues no
 * memset.  The caller keeps one persistent zeroed workspace per stream.  Default off. */
void sg2_set_clean_workspace(int on);

/* Deterministic mode (process-wide, so that autograd's backward threads see it; scratch NULL = off, the
 * default).  While a device scratch buffer is
 * registered, every float accumulation the entry points otherwise make with atomics -- split-K partial sums,
 * weight-gradient pixel splits, dot_out / db / dd reductions, the grid-sample input-gradient scatter -- is made
 * by writing each contribution to a slot of the scratch and summing the slots in a fixed order, so results
 * are bitwise reproducible.  Calls made while it is on must be stream-ordered (they share the scratch); a call
 * whose partial sums do not fit returns -1 ("deterministic scratch too small").  The explicit-grid
 * sg2_grid_sample_bwd keeps its atomics (only the affine form has the gather used here).  Since round 6 this is
 * the training iteration's default arithmetic (Trainer(deterministic=True) registers a 2 GiB scratch around every
 * phase's forward and backward): the slot reductions (per-tile dot slots, split sums folded into the split-K
 * finalize, one-launch det_sum) measured faster than the float atomics on the bench step. */
void sg2_set_deterministic(void* scratch, int64_t bytes);

/* Stride-2 / pad-0 form of sg2_conv3x3 (conv2d_resample.py:139-142 with down = 2: the discriminator's
 * down-2 3x3 layers after their FIR pre-filter, and the input gradient of the up-2 synthesis layers):
 * x [N, H, W, Cin] -> y [N, (H-3)/2+1, (W-3)/2+1, Cout]; same epilogue and dot as sg2_conv3x3, plus
 *   residual  [N, OH, OW, Cout] (dtype, NULL = off): y = round(epilogue) + residual, rounded
 *             (the resnet add of DiscriminatorBlock, networks_stylegan2.py:621-627)
 *   raw_act   1: y_raw receives the epilogue value before the residual add (the activation gradient's
 *             input) instead of the raw conv. */
int sg2_conv3x3_s2(void* y, void* y_raw, const void* x, const void* w, int dtype, int N, int Cin, int H, int W,
                   int Cout, const float* in_scale, const float* out_scale, const void* noise, float noise_gain,
                   const float* bias, int act, float alpha, float gain, float clamp, const void* residual,
                   int raw_act, const void* dot_src, float* dot_out, void* stream);

/* Stride-2 transposed 3x3 convolution, padding 0, 16-bit (conv2d_resample.py:112-129, the up-2 plan's
 * conv_transpose2d; also the input gradient of a stride-2 3x3 convolution):
 *   y[n, 2i+ky, 2j+kx, o] = sum_{c, (i,j) -> (2i+ky, 2j+kx)} x[n, i, j, c] (* s[n, c]) w[o][ky][kx][c]
 * x [N, H, W, Cin] NHWC, y [N, 2H+1, 2W+1, Cout] NHWC (overwritten), w packed [Cout][3][3][Cin] (the
 * conv_transpose2d weight [Cin, Cout, 3, 3] read as [Cout][Cin] without a tap flip), in_scale [N, Cin] f32
 * or NULL (the modulation x * s rounded as the reference's x * s.to(x.dtype)).  Cin % 32 == 0, Cout % 8 == 0. */
int sg2_conv3x3_up2(void* y, const void* x, const void* w, int dtype, int N, int Cin, int H, int W, int Cout,
                    const float* in_scale, void* stream);

/* Weight gradient of sg2_conv2d (transpose = 0 form):
 *   dw[a][ky][kx][b] = sum_{n,oy,ox} g[n,oy,ox,a] * u[n,a] * x[n, oy*stride+ky-pad_y, ox*stride+kx-pad_x, b] * s[n,b]
 *   u = g_scale [N, A], s = x_scale [N, B] float32 (a layer's modulation), or NULL for 1.
 *   g [N, OH, OW, A] NHWC, x [N, H, W, B] NHWC; dw is float32 [A][KH][KW][B], overwritten.
 *   The conv_transpose2d weight gradient is the same call with (g, x) = (x_of_convT, dy).
 *   alpha scales the result (dw = alpha * sum ...): a layer's weight gain, the backward of the reference's
 *   `self.weight * self.weight_gain` (networks_stylegan2.py:173) folded in (ABI 3). */
int sg2_conv2d_wgrad(float* dw, const void* g, const void* x, int dtype, int N, int A, int OH, int OW, int B,
                     int H, int W, int KH, int KW, int stride, int pad_y, int pad_x, const float* g_scale,
                     const float* x_scale, float alpha, void* stream);

/* sg2_conv2d_wgrad with dw written as float32 [A][B][KH][KW] -- torch's [O, I, kh, kw] parameter layout, so the
 * gradient reaches the parameter without a layout copy -- or, swap_ab != 0, as [B][A][KH][KW] (a transposed
 * convolution's weight, whose gradient is the call with g and x exchanged) (ABI 9).  SG2_F32S3 operands (the f32
 * layers) in deterministic mode only, B % 4 == 0, KH * KW <= 9: its fixed-order slot sum writes the transposed
 * layout. */
int sg2_conv2d_wgrad_oikk(float* dw, const void* g, const void* x, int dtype, int N, int A, int OH, int OW, int B,
                          int H, int W, int KH, int KW, int stride, int pad_y, int pad_x, float alpha, int swap_ab,
                          void* stream);

/* Fused first-order backward of the layer epilogue z = c*d + noise + b, y = clamp(act(z)*gain):
 *   dc = dz * d;  db[o] = sum dz;  dd[n,o] = sum_p dz*c;  dnoise[n,p] = sum_o dz
 * where dz = dy * act'(y) * gain masked by |y| < clamp.  dy, y, c, dc: [N, HW, C] NHWC (any dtype),
 * C % 8 == 0.  c / d / db / dd / dnoise may be NULL; db and dd are zeroed by the call. */
int sg2_layer_bwd(void* dc, float* db, float* dd, float* dnoise, const void* dy, const void* y, const void* c,
                  const float* d, int dtype, int N, int HW, int C, int act, float alpha, float gain, float clamp,
                  void* stream);

/* The elementwise steps of the layers' create_graph VJP (path-length / R1 passes; the reference runs them as
 * autograd's mul / add / bias_act-grad nodes, SG3/training/networks_stylegan2.py:59-89 and bias_act.py:154-207):
 *   out[n,p,c] = act'(a * sa[n,c] + b * sb[n,c]; y)      (sa / sb NULL = 1, b NULL = off, y NULL = no act')
 *   dot[n,c]   = sum_p a[n,p,c] * e[n,p,c]                (e and dot both or neither; dot zeroed by the call)
 * act' = the bias_act gradient given the output y: * gain, * alpha where y <= 0 (lrelu), 0 where |y| >= clamp
 * (clamp < 0 = off).  a, b, y, e, out: [N, HW, C] NHWC of dtype (f16 / bf16 / f32), C % 8 == 0; f32
 * arithmetic, one rounding. */
int sg2_vjp_axpy(void* out, const void* a, const float* sa, const void* b, const float* sb, const void* y, int act,
                 float alpha, float gain, float clamp, const void* e, float* dot, int dtype, int N, int HW, int C,
                 void* stream);

/* out[n, c] = sum_p a[n, p, c] * b[n, p, c] (f32 accumulation; a, b: [N, HW, C] NHWC f16/bf16, C % 8 == 0;
 * out zeroed by the call).  The reductions (dz * c).sum([2, 3]) and (dxs * x).sum([2, 3]) of the
 * modulated-conv backward (SG3/training/networks_stylegan2.py:59-70 under autograd) without the
 * full-size product in HBM. */
int sg2_dot_hw(float* out, const void* a, const void* b, int dtype, int N, int HW, int C, void* stream);

/* Bilinear grid sample, zeros padding, align_corners = False (the only mode the reference uses,
 * grid_sample_gradfix.py:9-12).  in [N,C,Hi,Wi] any strides; grid float32 [N,Ho,Wo,2] contiguous;
 * out [N,C,Ho,Wo] any strides. */
int sg2_grid_sample_fwd(void* out, const void* in, const float* grid, int dtype, const int64_t* in_size,
                        const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride,
                        const int* dyn_hw, void* stream);

/* Gradient of sg2_grid_sample_fwd w.r.t. its input: gin (float32, [N,C,Hi,Wi] with in_stride) is
 * zero-filled then accumulated. */
int sg2_grid_sample_bwd(float* gin, const void* gout, const float* grid, int dtype, const int64_t* in_size,
                        const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride,
                        const int* dyn_hw, void* stream);

/* The same two ops with the sampling grid built inline from theta (float32 [N,2,3] contiguous) as
 * torch.nn.functional.affine_grid(theta, [N,C,Ho,Wo], align_corners=False) would build it: the fusion of
 * SG3/training/augment_mi.py:317-318 (affine_grid + grid_sample_gradfix.grid_sample), which never
 * materialises the [N,Ho,Wo,2] grid in HBM. */
int sg2_affine_grid_sample_fwd(void* out, const void* in, const float* theta, int dtype, const int64_t* in_size,
                               const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride,
                               const int* dyn_hw, void* stream);
int sg2_affine_grid_sample_bwd(float* gin, const void* gout, const float* theta, int dtype, const int64_t* in_size,
                               const int64_t* in_stride, const int64_t* out_size, const int64_t* out_stride,
                               const int* dyn_hw, void* stream);

/* dyn_hw (all grid-sample calls; may be NULL): device int[2], the logical input height / width when
 * `in` is a larger static buffer whose valid region starts at the origin -- the ADA pipe's padded image
 * whose size depends on device-side margins (augment_mi.py:288-318), sampled without a host sync. */

/* Reflect padding with device-side margins (augment_mi.py:301): margins = device int[4] {mx0, my0,
 * mx1, my1} (each <= size - 1).  adjoint = 0: y [N,C,Hs,Ws] (NCHW, f32) = reflect-padded x [N,C,H,W]
 * at the origin, zeros elsewhere; Hs >= 3H-2, Ws >= 3W-2.  adjoint = 1: y [N,C,H,W] = the adjoint
 * (gather of the reflected positions) of x [N,C,Hs,Ws]. */
int sg2_reflect_pad_dyn(float* y, const float* x, const int* margins, int N, int C, int H, int W, int Hs, int Ws,
                        int adjoint, void* stream);

/* ADA geometric transforms of a batch in one launch (ABI 6; replaces the per-op matrix algebra of
 * SG3/training/augment_mi.py:214-318 -- stack / sin / cos / where / matmul per enabled op, the corner margins
 * and the pad / up-sampling conjugations).  draw[2k], draw[2k+1]: the value draw and the choice draw of op k
 * in the reference's order -- 0 xflip (rand[N], rand[N]), 1 rotate90 (rand[N], rand[N]), 2 xint (rand[N,2],
 * rand[N,1]), 3 scale (randn[N], rand[N]), 4 rotate (rand[N], rand[N]), 5 aniso (randn[N], rand[N]), 6 the
 * second rotate, 7 xfrac (randn[N,2], rand[N,1]); NULL for an op whose probability is 0.  p: device f32
 * scalar, the augmentation probability.  pad_x / pad_y: f32(2 hz_pad - (W-1)/2) / (.. (H-1)/2); inv_sx /
 * inv_sy: f32(1 / (2 / Wup)) / f32(1 / (2 / Hup)) of the up-sampled static buffer (the reference's Python
 * floats).  Writes theta [N,2,3] (the grid-sample transform), margins int[4] (mx0, my0, mx1, my1: the
 * reflect pad), lims int[8] (the up-sampling extents) and dyn_hw int[2] (the logical up-sampled size). */
typedef struct sg2_aug_geom_args {
    const float* draw[16];
    const float* p;
    float xflip, rotate90, xint, xint_max, scale, rotate, aniso, xfrac;
    float scale_std, rotate_max, aniso_std, xfrac_std;
    float pad_x, pad_y, inv_sx, inv_sy;
    int n, h, w;
} sg2_aug_geom_args;
int sg2_aug_geom(float* theta, int* margins, int* lims, int* dyn_hw, const sg2_aug_geom_args* args, void* stream);

/* training_stats.report in one launch (ABI 6; SG3/torch_utils/training_stats.py:55-99): row[0] += n,
 * row[1] += sum v, row[2] += sum v^2 over the n f32 values v (mode 1: of sign(v)), accumulated in float64 in a
 * fixed order.  row: device double[3], the statistic's row of the caller's moment table. */
int sg2_moments(double* row, const float* v, int64_t n, int mode, void* stream);

/* Demodulation coefficients d[n,o] = rsqrt(sum_i s[n,i]^2 * wsq[o,i] + eps), wsq[o,i] = sum_k w[o,i,k]^2
 * (SG3/training/networks_stylegan2.py:59-63, summation regrouped); s [N,I] f32, w [O,I*KK] f32.  Also
 * writes wsq [O, I] (may be NULL) for the backward. */
int sg2_demod_fwd(float* d, float* wsq, const float* s, const float* w, int N, int O, int I, int KK, float eps,
                  void* stream);

/* Gradient of sg2_demod_fwd (first order): with gu = -dd * d^3 / 2,
 *   gw[o,i,k] = 2 w[o,i,k] sum_n gu[n,o] s[n,i]^2,   gs[n,i] = 2 s[n,i] sum_o gu[n,o] wsq[o,i].
 * gs / gw may be NULL (gs needs wsq).  The reference gets these from autograd of
 * networks_stylegan2.py:59-63. */
int sg2_demod_bwd(float* gs, float* gw, const float* dd, const float* d, const float* s, const float* w,
                  const float* wsq, int N, int O, int I, int KK, void* stream);

/* Backward of sg2_demod_bwd's styles gradient gs = 2 s (u @ wsq), u = -dd d^3 / 2 (ABI 7; the path-length pass
 * differentiates it once more -- the reference by autograd of networks_stylegan2.py:59-63 under create_graph):
 * given g = dL/dgs [N,I],
 *   g_dd = -d^3 v,  g_d = -3 dd d^2 v  (v = (s g) @ wsq^T),   g_w[o,i,k] = 2 w (u^T @ 2 s g)[o,i],
 *   g_s = 2 g (u @ wsq).
 * Any output may be NULL; w [O,I*KK], wsq [O,I] as written by sg2_demod_fwd. */
int sg2_demod_vjp_bwd(float* g_dd, float* g_d, float* g_w, float* g_s, const float* g, const float* dd,
                      const float* d, const float* s, const float* w, const float* wsq, int N, int O, int I, int KK,
                      void* stream);

/* Convolution weight pack (replaces the strided-permute copies that feed every conv launch,
 * conv2d_gradfix.py _pack_conv / _pack_convT; the reference feeds cuDNN the [O,I,kh,kw] weight
 * directly, networks_stylegan2.py:70/176):  out[a][k][b] = in[a*sa + b*sb + k'*sk], k' = K-1-k when
 * flip != 0, else k.  Strides in elements; in/out dtypes SG2_F32/F16/BF16 (cast in the same pass); K <= 9.
 * [O,I,kh,kw] -> [O][kh][kw][I]: A=O, B=I, K=kh*kw, sa=I*K, sb=K, sk=1.
 * Each element is multiplied by `scale` in f32 before the cast (ABI 3): a layer's weight gain, the
 * reference's `self.weight * self.weight_gain` (networks_stylegan2.py:173) in the same pass. */
int sg2_pack_weight(void* out, int out_dtype, const void* in, int in_dtype, int A, int B, int K, int64_t sa,
                    int64_t sb, int64_t sk, int flip, float scale, void* stream);

/* Many packs in one launch per 64 (ABI 8): `descs` is a HOST array of n sg2_pack_desc (copied into the launch's
 * kernel arguments, so the call can be captured into a hipGraph; block0 is ignored).  Each pack is bitwise what
 * sg2_pack_weight computes for the same arguments; strides must fit 32 bits.  Used by conv2d_gradfix.pack_cache to
 * pack all of a training phase's conv weights at the phase start. */
typedef struct sg2_pack_desc {
    void* out;
    const void* in;
    int64_t sa, sb, sk;
    int out_dtype, in_dtype, A, B, K, flip;
    float scale;
    int block0;
} sg2_pack_desc;
int sg2_pack_weight_multi(const sg2_pack_desc* descs, int n, void* stream);

/* fp16 range pre-normalisation, row-wise (SG3/training/networks_stylegan2.py:52-54): t [rows, L] f32,
 * n[r] = max_i |t[r,i]| (written to nrm [rows]); mode 0: y = t * ((1/n) * c)  (the weight, c = 1/sqrt(fan_in)),
 * mode 1: y = t / n  (the styles). */
int sg2_infnorm_fwd(float* y, float* nrm, const float* t, int rows, int L, float c, int mode, void* stream);

/* First-order gradient of sg2_infnorm_fwd w.r.t. t (torch's infinity-norm backward: the norm's gradient split
 * evenly between tied maxima). */
int sg2_infnorm_bwd(float* dt, const float* dy, const float* t, const float* nrm, int rows, int L, float c, int mode,
                    void* stream);

/* The style path of a whole synthesis pass in table launches (csrc/misc.hip).  ADDITIVE entry point:
 * SG2_ABI_VERSION stays 11.  `jobs` is a HOST array of n sg2_style_job (copied into the launches' kernel arguments,
 * 40 jobs per launch, so the call can be captured into a hipGraph).  A job is one launch of a single-layer entry
 * point and gives bitwise its result; the jobs of one call must not depend on each other.
 *   kind                    is              p[0..5]                       n[0..3]         c     mode   workgroups
 *   SG2_STYLE_INFNORM_FWD   sg2_infnorm_fwd y, nrm, t                     rows, L         c     mode   rows
 *   SG2_STYLE_DEMOD_FWD     sg2_demod_fwd   d, wsq (or NULL), s, w        N, O, I, KK     eps   -      O
 *   SG2_STYLE_DEMOD_BWD_W   sg2_demod_bwd   gw, dd, d, s, w, add          N, O, I, KK     -     -      O
 *   SG2_STYLE_DEMOD_BWD_S   sg2_demod_bwd   gs, dd, d, s, wsq, add        N, O, I         -     -      N ceil(I/64)
 *   SG2_STYLE_INFNORM_BWD   sg2_infnorm_bwd dt, dy, t, nrm                rows, L         c     mode   rows
 * add (NULL: none): a second gradient of the same tensor, added to the job's result as a separate f32 add would (the
 * sum autograd makes of a tensor's two gradients); for gw its element (o, i, k) is at add[o st[0] + i st[1] + k st[2]],
 * for gs it is contiguous [N, I]. */
enum { SG2_STYLE_INFNORM_FWD = 0, SG2_STYLE_DEMOD_FWD = 1, SG2_STYLE_DEMOD_BWD_W = 2, SG2_STYLE_DEMOD_BWD_S = 3,
       SG2_STYLE_INFNORM_BWD = 4 };
typedef struct sg2_style_job {
    void* p[6];
    int n[4];
    int st[3];
    float c;
    int mode, kind;
} sg2_style_job;
int sg2_style_table(const sg2_style_job* jobs, int n, void* stream);

/* Backward of sg2_infnorm_bwd (ABI 7; the path-length pass's second order through the fp16 pre-normalisation,
 * reference: autograd of networks_stylegan2.py:52-54 under create_graph).  With the first-order gradient
 * dt = c dy / n - c P e / n^2, P = sum dy t, e = sgn(t) [|t| = n] / cnt, and g = dL/ddt [rows, L]:
 *   g_dy = c (g - t (g.e) / n) / n,   g_t = c (2 P (g.e) e / n^3 - ((g.dy) e + (g.e) dy) / n^2).
 * c = the mode-0 scale (1 for mode 1); either output may be NULL. */
int sg2_infnorm_vjp_bwd(float* g_dy, float* g_t, const float* g, const float* dy, const float* t, const float* nrm,
                        int rows, int L, float c, void* stream);

/* Multi-tensor launches of the optimiser step.  A segment is one parameter tensor; `blocks` [nblocks] lists
 * the work items as (segment << 40) | start, one per 4096 elements of a segment (start = 0, 4096, ...),
 * so one launch covers a whole module.  Tables are device int64 / float arrays built by the caller. */

/* torch.optim.Adam (no weight decay, amsgrad off; foreach arithmetic) of every parameter in one exchanged
 * flat gradient, with the reference's sanitation in front (training_loop_mi_multimodal.py:341-351):
 *   g = nan_to_num(grad * grad_scale, nan=0, posinf=1e5, neginf=-1e5)      (grad_scale = 1/num_gpus)
 *   m = m.lerp(g, 1-beta1);  v = v*beta2 + (1-beta2)*g*g;  p += -step_size * m / (sqrt(v)/bc2_sqrt + eps)
 * seg [nseg][3] = {float* param, offset of the segment in grad / exp_avg / exp_avg_sq, numel};
 * coef [nseg][2] f32 = {step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)} (the caller's
 * per-parameter step counts, as torch keeps them).  write_grad != 0 stores the sanitised g back. */
int sg2_adam_multi(const int64_t* seg, const float* coef, const int64_t* blocks, int nblocks, float* grad,
                   float* exp_avg, float* exp_avg_sq, float beta1, float beta2, float eps, float grad_scale,
                   int write_grad, void* stream);

/* dst = src.lerp(dst, beta) per segment (the G_ema update, training_loop_mi_multimodal.py:363-364);
 * seg [nseg][3] = {float* dst, const float* src, numel}. */
int sg2_lerp_multi(const int64_t* seg, const int64_t* blocks, int nblocks, float beta, void* stream);

/* k-nearest-neighbour manifolds of the improved precision / recall metric (ABI 10; SG3/metrics/precision_recall.py:
 * 51-61: cdist in blocks, kthvalue(nhood_size + 1), `dist <= kth`, any).  One fp16 "NT" GEMM whose [rows, cols]
 * distance matrix is never stored: the epilogue keeps the k + 1 smallest entries (radii) or one flag (membership)
 * per row.  Arithmetic of both calls:
 *   d2 = max(|a|^2 + |b|^2 - 2 a.b, 0) in f32 (a.b: fp16 MFMA, f32 accumulation; the squared norms: f32 sums of the
 *   fp16 values in a fixed order), dist = sqrtf(d2); round16 != 0: dist is rounded to fp16 (nearest even) before it
 *   is ranked or compared -- the reference's fp16 distance matrix, fp16 radii and fp16 `<=`.
 * Results are bitwise reproducible (no atomics: per-split partials merged by a second kernel).
 * dtype: SG2_F16 only; d % 8 == 0; 1 <= k <= 7; each operand below 2 GiB and 16-byte aligned.
 *
 * sg2_knn_scratch_bytes: the scratch both calls below need for `rows` rows against `cols` columns (radii:
 * rows = cols = n; membership: rows = p, cols = n).  A shorter scratch is an argument error.
 * sg2_knn_radii: radii[i] = the (k + 1)-th smallest of dist(x_i, x_j) over all j < n, the diagonal taken as exactly
 *   0 and counted (x [n, d] row-major, n >= k + 1).
 * sg2_manifold_member: hit[i] = 1 if dist(probes_i, manifold_j) <= radii[j] for any j < n, else 0
 *   (probes [p, d], manifold [n, d], radii [n]; a NaN or negative radius never matches). */
int sg2_knn_scratch_bytes(int64_t* bytes, int64_t rows, int64_t cols, int k);
int sg2_knn_radii(float* radii, const void* x, int dtype, int64_t n, int d, int k, int round16, void* scratch,
                  int64_t scratch_bytes, void* stream);
int sg2_manifold_member(uint8_t* hit, const void* probes, int64_t p, const void* manifold, int64_t n,
                        const float* radii, int dtype, int d, int round16, void* scratch, int64_t scratch_bytes,
                        void* stream);

/* Density and coverage (Naeem et al., ICML 2020) on the membership pass (additive to ABI 11): the same GEMM, tiles,
 * distances, round16 and per-column `<=` thresholds as sg2_manifold_member, with an epilogue that counts instead of
 * OR-ing and also reduces along the manifold axis.  One pass over the p x n distance tiles gives
 *   count[i]   = #{ j < n : dist(probes_i, manifold_j) <= radii[j] }      (int32 [p]; density = sum / (k p))
 *   covered[j] = 1 if dist(probes_i, manifold_j) <= radii[j] for any i < p, else 0      (uint8 [n]; coverage = mean)
 * and count[i] > 0 is sg2_manifold_member's hit[i], bit for bit.  Integer sums and ORs of per-(split, row) and
 * per-(row tile, column) partials, every partial written by the call that reads it: no atomics, no memset, bitwise
 * reproducible.  The same argument rules as sg2_manifold_member; the scratch size is a query of its own. */
int sg2_manifold_count_scratch_bytes(int64_t* bytes, int64_t p, int64_t n);
int sg2_manifold_count(int32_t* count, uint8_t* covered, const void* probes, int64_t p, const void* manifold,
                       int64_t n, const float* radii, int dtype, int d, int round16, void* scratch,
                       int64_t scratch_bytes, void* stream);

/* The small-tensor part of a latent projection step (ABI 11; SG3/genlib/projector/projector.py:259-268 the noise
 * regulariser, :294-298 the per-buffer renormalisation).  All noise buffers of a generator live in ONE flat f32 device
 * buffer; `table` is a HOST array int64 [nbuf][2] of (offset of the buffer in flat, in floats; R) rows, 1 <= nbuf <= 32.
 * R is a power of two in 4..1024 (square buffers), every offset a multiple of 4 floats, flat 16-byte aligned; anything
 * else is an argument error and no device work is issued.  A buffer's levels: evaluate at the current size, stop if the
 * size is <= 8, else 2x2 average-pool and repeat (R <= 8: one level, 16: two, 256: six).
 * No atomics: every sum is a fixed tree (serial runs of <= 16 terms), so results are bitwise reproducible.
 *
 * sg2_noise_reg_scratch_bytes: the scratch (pooled levels + per-chunk partial sums) the two calls below need.
 * sg2_noise_reg_fwd (3 launches): reg[0] = sum_buf sum_level mean(n roll_x n)^2 + mean(n roll_y n)^2 (circular shifts by
 *   one); means [sum of levels][2] = the (x, y) means, buffers in table order, levels from the finest.
 * sg2_noise_reg_bwd (1 launch): gflat[off + i] (+)= greg[0] * sum_level 4^-l (2 mx_l / cnt_l (W + E) + 2 my_l / cnt_l
 *   (N + S)) of element i's level-l ancestor's circular neighbours; `flat`, `means` and `scratch` as the forward call
 *   left them; greg: device scalar; accumulate != 0 adds into gflat, 0 assigns every element of every buffer.
 * sg2_noise_normalize_multi (1 launch): per buffer, in place, x -= mean(x); x *= 1 / sqrt(mean(x^2)). */
int sg2_noise_reg_scratch_bytes(int64_t* bytes, const int64_t* table, int nbuf);
int sg2_noise_reg_fwd(float* reg, float* means, const float* flat, const int64_t* table, int nbuf, void* scratch,
                      void* stream);
int sg2_noise_reg_bwd(float* gflat, const float* greg, const float* means, const float* flat, const int64_t* table,
                      int nbuf, const void* scratch, int accumulate, void* stream);
int sg2_noise_normalize_multi(float* flat, const int64_t* table, int nbuf, void* stream);

/* The same step for B independent projections at once (a batch of latents, each with its own noise buffers).
 * ADDITIVE entry points: SG2_ABI_VERSION stays 11 -- the four calls above keep their kernels and results.
 * Layout: buffer-major.  Row k of `table` is (off_k, R_k) as above, and the buffer holds B samples one after another:
 * sample s of buffer k is the R_k x R_k block at flat + off_k + s R_k^2 (so [B, 1, R, R] views of flat are contiguous).
 * 1 <= B <= 64, and off_k + B R_k^2 must stay below 2 GiB; nbuf, R, offsets and alignment as above; anything else is an
 * argument error and no device work is issued.  The sample is a grid dimension, so the launch counts do not depend on B.
 * Per sample the summation trees are those of the calls above: sample s's reg, means, gradient and normalised buffers
 * are BITWISE what the batch-1 calls give on that sample's buffers alone.  No atomics; two calls give the same bits.
 *
 * sg2_noise_reg_batched_scratch_bytes: the scratch of the two calls below (B shares, each the batch-1 scratch rounded
 *   up to 16 bytes).
 * sg2_noise_reg_fwd_batched (3 launches): reg [B]; means [B][sum of levels][2], per sample as sg2_noise_reg_fwd's.
 * sg2_noise_reg_bwd_batched (1 launch): gflat[off_k + s R_k^2 + i] (+)= greg[s] * d reg[s] / d flat[the same]; greg
 *   device f32 [B]; `flat`, `means` and `scratch` as the forward call left them; accumulate != 0 adds, 0 assigns every
 *   element of every sample of every buffer.  Nothing outside the buffers (the latents, padding) is read or written.
 * sg2_noise_normalize_batched (1 launch): per sample and buffer, in place, x -= mean(x); x *= 1 / sqrt(mean(x^2)). */
int sg2_noise_reg_batched_scratch_bytes(int64_t* bytes, const int64_t* table, int nbuf, int B);
int sg2_noise_reg_fwd_batched(float* reg, float* means, const float* flat, const int64_t* table, int nbuf, int B,
                              void* scratch, void* stream);
int sg2_noise_reg_bwd_batched(float* gflat, const float* greg, const float* means, const float* flat,
                              const int64_t* table, int nbuf, int B, const void* scratch, int accumulate, void* stream);
int sg2_noise_normalize_batched(float* flat, const int64_t* table, int nbuf, int B, void* stream);

/* The per-sample loss of a batched projection step (csrc/proj_loss.hip).  ADDITIVE entry points: SG2_ABI_VERSION stays
 * 11.  All tensors f32, contiguous; no atomics, every sum a fixed tree: results are bitwise reproducible, and a sample
 * (a row) gives the same bits alone or in a batch.
 *
 * sg2_proj_prep_fwd (2 launches): synth [B, C, H, H] (the generator's output) and target [B, C, H, H] in [0, 255], H a
 *   power of two in 4..1024, 1 <= C <= 16, 16-byte aligned.  Channel rule (projector.split_modalities): C = 1: one
 *   modality (M = 1), the channel repeated to three; C = 3: one RGB modality as it is; any other C: M = C modalities,
 *   each channel repeated.  With s = (x + 1) * 127.5 (an add and a multiply, two roundings, never an FMA) it writes
 *   det_in [M B, 3, Hd, Hd], row m B + b: s itself up to 256^2 (f = 1: bitwise the f32 torch composition
 *   (synth + 1) * (255 / 2) and the split), above it the mean of s over f x f, f = H / 256, Hd = H / f;
 *   pix [B][M] = mean (t - s)^2 over the modality's channels at full resolution (a repeated modality's three channels
 *   are equal: the mean over its H H source elements).  The tree depends on C and H only (csrc/proj_loss.hip).
 *   sg2_proj_prep_scratch_bytes: the scratch (one partial per 256 groups of 4 f^2 elements) the call needs.
 * sg2_proj_prep_bwd (1 launch): assigns every element of gsynth [B, C, H, H] once:
 *   127.5 (sum over the det_in channels that read (b, c) of gdet_in / f^2 + gpix[b][m] 2 (s - t) / n_m), n_m the
 *   modality's source elements (H H, RGB: 3 H H).  gdet_in [M B, 3, Hd, Hd], gpix [B][M].
 * sg2_sqdist_rows_fwd (2 launches): dist[r] = sum_j (f[r][j] - tf[r][j])^2 for R rows of any length F, f and tf
 *   [R, F] row-contiguous behind two pointers (no concatenated copy), on sg2_lpips_pair_dist's tree, whose shape
 *   depends on F only; rows that are not 16-byte aligned are read element by element on the same tree.
 *   1 <= R <= 65535.  sg2_sqdist_rows_scratch_bytes: one partial per row and 8192-element chunk.
 * sg2_sqdist_rows_bwd (1 launch): gf[r][j] = 2 g[r] (f[r][j] - tf[r][j]), every element assigned. */
int sg2_proj_prep_scratch_bytes(int64_t* bytes, int B, int C, int H);
int sg2_proj_prep_fwd(float* det_in, float* pix, const float* synth, const float* target, int B, int C, int H,
                      void* scratch, int64_t scratch_bytes, void* stream);
int sg2_proj_prep_bwd(float* gsynth, const float* gdet_in, const float* gpix, const float* synth, const float* target,
                      int B, int C, int H, void* stream);
int sg2_sqdist_rows_scratch_bytes(int64_t* bytes, int64_t R, int64_t F);
int sg2_sqdist_rows_fwd(float* dist, const float* f, const float* tf, int64_t R, int64_t F, void* scratch,
                        int64_t scratch_bytes, void* stream);
int sg2_sqdist_rows_bwd(float* gf, const float* g, const float* f, const float* tf, int64_t R, int64_t F, void* stream);

/* The two streaming passes of a perceptual-path-length sampler call (SG3/metrics/perceptual_path_length.py:71-89).
 * ADDITIVE entry points: SG2_ABI_VERSION stays 11 -- nothing that existed changes, and a caller built against the
 * ABI-11 header keeps working; callers that need them look the symbols up.
 *
 * sg2_ppl_prep (1 launch): the detector's input from the generator's output.  img f32 NCHW contiguous [N, C, H, W];
 *   crop != 0: with c = H / 8 the window rows 3c..7c, columns 2c..6c (needs H == W, H % 8 == 0); factor >= 1 divides the
 *   (cropped) height and width; channel = one source channel, written to all three output channels, or -1 = all
 *   channels (C = 3: as they are; C = 1: repeated; any other C is an argument error).
 *   out f32 NCHW [N, 3, H' / factor, W' / factor] = (mean over factor x factor of x + 1) * 127.5 -- an add and a multiply,
 *   two roundings, never an FMA: at factor 1 bitwise the f32 torch composition (x + 1) * (255 / 2).
 * sg2_lpips_pair_dist (2 launches): feats f32 [2B, F] row-contiguous (rows 0..B-1 against rows B..2B-1),
 *   dist[b] = (sum_j (feats[b][j] - feats[B + b][j])^2) / (float)(eps * eps), f32 arithmetic, no atomics: a fixed tree
 *   whose shape depends on F only (serial runs of 8 and of ceil(ceil(F / 8192) / 256) terms, tree depth 18; csrc/ppl.hip),
 *   so results are bitwise reproducible and a pair gives the same bits alone or in a batch.  Any F; rows that are not
 *   16-byte aligned are read element by element on the same tree.  1 <= B <= 65535, eps > 0.
 * sg2_lpips_pair_dist_scratch_bytes: the scratch (one partial sum per 8192-element chunk and pair) the call needs; a
 *   shorter scratch is an argument error. */
int sg2_ppl_prep(float* out, const float* img, int N, int C, int H, int W, int channel, int crop, int factor,
                 void* stream);
int sg2_lpips_pair_dist_scratch_bytes(int64_t* bytes, int64_t B, int64_t F);
int sg2_lpips_pair_dist(float* dist, const float* feats, int64_t B, int64_t F, double eps, void* scratch,
                        int64_t scratch_bytes, void* stream);

/* The polynomial-kernel MMD sums of the kernel inception distance (SG3/metrics/kernel_inception_distance.py:33-44).
 * ADDITIVE entry points: SG2_ABI_VERSION stays 11.
 *
 * gen f32 [n_gen, d] and real f32 [n_real, d] row-major, 16-byte aligned, any size (row addresses are 64-bit);
 * idx_gen, idx_real: DEVICE int32 [S, m] tables of row numbers, TRUSTED (0 <= idx < n is the caller's to check).
 * With x_i = gen[idx_gen[s][i]], y_j = real[idx_real[s][j]] and k(a, b) = (a.b / d + 1)^3,
 *   sums[s] = ( sum_{i != j} k(x_i, x_j),  sum_{i != j} k(y_i, y_j),  sum_{i, j} k(x_i, y_j) )     (f64 [S, 3], device)
 * where i != j compares subset POSITIONS, not row numbers: a row drawn twice counts as two points.
 * The dot product is an exact-f32 fma chain (the f32-input MFMA); / d, + 1 and the cube are f32 operations, as in
 * float32 numpy; every addition of kernel values is f64 in an order fixed by (S, m) alone, without atomics: two calls
 * give the same bits.  Neither a gathered [S, m, d] copy nor an m x m matrix is written to memory.
 * d >= 4 and d % 4 == 0, m >= 2, S >= 1, n_gen and n_real >= 1; anything else is an argument error and nothing is
 * launched.  2 launches.
 * sg2_poly_mmd_scratch_bytes: the scratch (one f64 per 128 x 128 tile) the call needs; a shorter one is an argument
 *   error.  Every scratch element the call reads it has written itself. */
int sg2_poly_mmd_scratch_bytes(int64_t* bytes, int S, int m);
int sg2_poly_mmd_sums(double* sums, const float* gen, int64_t n_gen, const float* real, int64_t n_real,
                      const int32_t* idx_gen, const int32_t* idx_real, int S, int m, int d, void* scratch,
                      int64_t scratch_bytes, void* stream);

/* The generator's output stage: images -> uint8 tiles of an HWC canvas in one launch (SG3/gen_video.py layout_grid,
 * gen_images*.py, save_image / save_image_grid; csrc/imgout.hip).  ADDITIVE entry point: SG2_ABI_VERSION stays 11.
 *
 * img [N, C, H, W] contiguous, dtype SG2_F32 / SG2_F16 / SG2_BF16 (16-bit values are widened to f32 first, exactly);
 * canvas uint8 [gh * H, gw * W, Cout] contiguous (HWC: what an image or video writer takes), any byte alignment.
 * tiles:  a channel k >= 0     tile n = channel k of image n,           Cout = 1, T = N tiles
 *         SG2_TILES_GREY       tile n * C + c = channel c of image n,   Cout = 1, T = N * C
 *         SG2_TILES_HWC        tile n = image n, channels interleaved,  Cout = C in {1, 3}, T = N
 * Tile t goes to grid cell first_tile + t: row (first_tile + t) / gw, column (first_tile + t) % gw;
 * first_tile + T > gw * gh is an argument error.  Canvas bytes outside the addressed tiles are not written.
 * mode SG2_U8_TRUNC (lo, hi ignored): v = x * 127.5f rounded to f32, then + 128.0f rounded to f32 (two roundings,
 *   never an FMA), clamped to [0, 255], truncated toward zero: bitwise the torch composition
 *   (x.float() * 127.5 + 128).clamp(0, 255).to(uint8).
 * mode SG2_U8_RINT: v = (x - (float)lo) * (float)(255.0 / (hi - lo)) (the quotient in double, cast once; a subtract
 *   and a multiply, two roundings), rounded half to even, clipped to [0, 255]: bitwise numpy's
 *   rint((x - lo) * (255 / (hi - lo))).clip(0, 255) on a float32 array.  lo, hi finite, hi != lo.
 * Both modes, by this build's definition (the torch and numpy casts of NaN are undefined): NaN -> 0, +inf -> 255,
 *   -inf -> 0.
 * One read of img, one write of the canvas, no scratch, no atomics, 64-bit offsets; 16-byte loads and stores per lane
 * when Cout = 1, W % 16 == 0 and both bases are 16-byte aligned, aligned 4-byte stores otherwise. */
#define SG2_TILES_HWC (-1)
#define SG2_TILES_GREY (-2)
#define SG2_U8_TRUNC 0
#define SG2_U8_RINT 1
int sg2_image_tiles_u8(uint8_t* canvas, const void* img, int dtype, int N, int C, int H, int W, int tiles, int mode,
                       double lo, double hi, int gw, int gh, int64_t first_tile, void* stream);

/* The summed 2-D power spectrum of a batch of windowed, zero-padded images (SG3/avg_spectra.py:164-166 summed over the
 * batch and kept per channel; csrc/spectrum.hip).  ADDITIVE entry points: SG2_ABI_VERSION stays 11.
 *
 *   out[c, u, v] = sum_b | sum_{y, x} ((img[b, c, y, x] - mean[c]) / std[c]) w[y] w[x]
 *                                     exp(-2 pi i (u y + v x) / S) |^2,     S = N * interp,  u, v in [0, S)
 * out f64 [C, S, S] contiguous, WRITTEN (not accumulated), every element exactly once per call.
 * img [B, C, N, N] of dtype SG2_U8 or SG2_F32 with element strides[4] = [sB, sC, sY, sX] (any view); window f64 [N],
 * mean and std f64 [C] (std > 0 is the caller's to check), twiddle: S complex f64 values (re, im interleaved),
 * twiddle[k] = exp(-2 pi i k / S), computed by the caller in f64 or better and conjugate-symmetric bit for bit
 * (twiddle[S - k] = conj(twiddle[k]), twiddle[0] = 1, twiddle[S / 2] = -1): the bitwise Hermitian symmetry of out
 * on the lines v = 0 and v = S / 2 rests on it.  All DEVICE pointers.
 * A pruned DFT as two f64 MFMA GEMMs with K = N: the padding's zeros are never multiplied, no S x S complex spectrum
 * is stored (scratch holds the half-transformed [B, C, 2, N, ~S / 2 + 1] f64 rows and one f64 [C, S, S / 2 + 1] sum
 * per batch group).  Every sum's order depends on (B, C, N, interp) alone, there are no atomics: two calls give the
 * same bits.  Every scratch element the call reads it has written itself.
 * N a multiple of 4 in 8..1024, interp >= 1, S <= 4096, B >= 1, C >= 1, B * C <= 65535; anything else, a null
 * pointer or a short scratch is an argument error and nothing is launched.  3 launches.
 * sg2_power_spectrum_scratch_bytes: the scratch the call needs. */
#define SG2_U8 4
int sg2_power_spectrum_scratch_bytes(int64_t* bytes, int B, int C, int N, int interp);
int sg2_power_spectrum_sum(double* out, const void* img, int dtype, const int64_t* strides, int B, int C, int N,
                           int interp, const double* window, const double* mean, const double* std,
                           const double* twiddle, void* scratch, int64_t scratch_bytes, void* stream);

/* Structural similarity (Wang et al. 2004, the original formulation) and mean squared error of N C image pairs in one
 * pass over the two images (csrc/ssim.hip).  ADDITIVE entry points: SG2_ABI_VERSION stays 11.
 *
 * x, y f32 [N, C, H, W] contiguous, DEVICE pointers; window11: HOST pointer to the 11 f64 weights g of the separable
 * window w = g g^T (the Gaussian of sigma 1.5 normalised to sum 1 is the caller's to pass); data_range L > 0.
 * Valid positions only, OH x OW = (H - 10) x (W - 10):
 *   mx = sum w x, my = sum w y, sxx = sum w x^2 - mx^2, syy = sum w y^2 - my^2, sxy = sum w x y - mx my
 *   ssim = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = (0.01 L)^2, C2 = (0.03 L)^2
 * out f64 [N C][2], WRITTEN: out[i][0] = mean of ssim over the valid positions, out[i][1] = mean of (x - y)^2 over all
 * H W pixels.  map, when non-null: f32 [N C][OH][OW], every element written once, ssim rounded to f32.
 * The five moments are f64 fma chains (horizontal, then vertical, taps in increasing order) and the expression is
 * evaluated in f64 without contraction: x against itself gives exactly 1.0 everywhere.  No atomics: every 16 x 32 output
 * tile writes its two partial sums to scratch [N C][tiles][2] and a finalize launch adds them in an order fixed by
 * (H, W): two calls give the same bits, a pair gives the same bits alone or in a batch, and map == NULL does not change
 * out.  Every scratch element the call reads it has written itself.  2 launches.
 * N, C >= 1, H and W in 11..1024, data_range > 0; anything else, a null out, x, y, window11 or scratch, or a short
 * scratch is an argument error and nothing is launched.
 * sg2_ssim_scratch_bytes: 16 bytes per tile and pair, N C ceil(OH / 16) ceil(OW / 32) 16. */
int sg2_ssim_scratch_bytes(int64_t* bytes, int N, int C, int H, int W);
int sg2_ssim_mse(double* out, float* map, const float* x, const float* y, int N, int C, int H, int W,
                 const double* window11, double data_range, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SG2HIP_H */
