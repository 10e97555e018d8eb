/*
 * fmgan_hip.h — C-ABI of libfmgan_hip.so: the MI355X (gfx950) kernels behind the
 * 3D-FM GAN forward hot path `(photo, render) -> image`.
 *
 * This is the drop-in boundary.  Every entry point takes plain device pointers,
 * sizes and a `hipStream_t` (passed as void*), launches asynchronously on that
 * stream, never allocates, never synchronises, keeps no global state and is
 * re-entrant (one call per Python thread / per rank is fine).  The caller owns
 * all buffers; outputs must be pre-allocated (the reference allocates inside the
 * op with at::empty — here the host-side shim does that).
 *
 * Return value: FMGAN_OK (0) or a negative FMGAN_E* code.  The reference checks
 * only "is a CUDA tensor" (op/upfirdn2d.cpp:8,15-16, op/fused_bias_act.cpp:7,13-14)
 * and never calls cudaGetLastError; this library additionally validates shapes
 * and reports launch failures, and the Python shim turns any non-zero status into
 * RuntimeError (same exception type as TORCH_CHECK).
 *
 * Reference interfaces replaced (paths relative to the reference repo root):
 *   fmgan_upfirdn2d        <- upfirdn2d_op()        op/upfirdn2d_kernel.cu:209-369
 *                             (pybind `upfirdn2d`    op/upfirdn2d.cpp:12-23)
 *   fmgan_fused_bias_act   <- fused_bias_act_op()   op/fused_bias_act_kernel.cu:52-99
 *                             (pybind `fused_bias_act` op/fused_bias_act.cpp:11-21)
 *   fmgan_modconv_demod,
 *   fmgan_modconv2d        <- ModulatedConv2d.forward  stylegan2.py:250-298
 *                             (F.conv2d / F.conv_transpose2d with groups=batch)
 *   fmgan_torgb            <- ToRGB.forward            stylegan2.py:389-404
 *   fmgan_images_to_tensor <- transforms.ToTensor()+Normalize   train_3_encoder.py:233-239
 *   fmgan_resize_*         <- transforms.Resize(size) (PIL BILINEAR) train_3_encoder.py:235
 *   fmgan_tensor_to_images <- tensor2im                 Evaluation/visual_eval.py:24-38
 *   fmgan_ema_f32          <- accumulate                train_3_encoder.py:195-200
 *   fmgan_loss_row_f32     <- the nine .item() of Print_Train_Status   train_3_encoder.py:641-651
 */
#ifndef FMGAN_HIP_H
#define FMGAN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FMGAN_ABI_VERSION 1

/* status codes */
#define FMGAN_OK            0
#define FMGAN_EINVAL       -1   /* null pointer / non-positive or inconsistent dims */
#define FMGAN_EUNSUPPORTED -2   /* dtype / act / mode outside what the reference dispatches */
#define FMGAN_ELAUNCH      -3   /* hipGetLastError() != hipSuccess after the launch */
#define FMGAN_EOVERFLOW    -4   /* an element count does not fit the kernel's index type */

/* element types (the reference dispatches float/double/half:
 * op/upfirdn2d_kernel.cu:311, op/fused_bias_act_kernel.cu:79) */
#define FMGAN_F32 0
#define FMGAN_F64 1
#define FMGAN_F16 2
#define FMGAN_BF16 3  /* fmgan_act16_* and fmgan_ufd16 only: the entry points above take FMGAN_F32/F64/F16 */

int         fmgan_abi_version(void);
const char *fmgan_status_string(int status);

/* Which upfirdn2d kernel `fmgan_upfirdn2d` runs for these arguments:
 * 0 generic, 1 row-march (up=down=1, wide rows), 2 LDS plane-tile (up=down=1,
 * small planes), 3 up=2 polyphase.  Pure host logic, no GPU needed: the launch's
 * own plan with the launch left out.  A kernel id is returned exactly when the
 * launch with these arguments (and valid pointers) runs that kernel; arguments
 * the launch refuses return the launch's status (< 0).  The query has no
 * addresses, so 1 stands for both row-march variants (path 1 and 1b).
 * `force_path` in fmgan_upfirdn2d uses the same numbering (-1 = automatic). */
int fmgan_upfirdn2d_select(int dtype, int major, int in_h, int in_w, int minor,
                           int kernel_h, int kernel_w, int up_x, int up_y,
                           int down_x, int down_y, int pad_x0, int pad_x1,
                           int pad_y0, int pad_y1);

/* out_h/out_w exactly as upfirdn2d_op computes them (op/upfirdn2d_kernel.cu:237-240). */
int fmgan_upfirdn2d_out_size(int in_h, int in_w, int kernel_h, int kernel_w,
                             int up_x, int up_y, int down_x, int down_y,
                             int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                             int *out_h, int *out_w);

/*
 * upfirdn2d: zero-stuff by (up_y,up_x), pad/crop by (pad_*; negative = crop),
 * correlate with the FLIPPED `kernel` (i.e. true convolution), keep every
 * (down_y,down_x)-th sample.
 *   input  [major, in_h, in_w, minor]   contiguous, `dtype`
 *   kernel [kernel_h, kernel_w]         contiguous, `dtype` (un-flipped, as the caller holds it)
 *   out    [major, out_h, out_w, minor] contiguous, `dtype`, pre-allocated
 * Semantics: op/upfirdn2d_kernel.cu:107-207 (== upfirdn2d_native, op/upfirdn2d.py:168-209).
 * force_path: -1 automatic; otherwise a path number from fmgan_upfirdn2d_select
 * (FMGAN_EUNSUPPORTED if that path cannot serve the arguments) — used by tests/bench.
 */
int fmgan_upfirdn2d(int dtype, const void *input, const void *kernel, void *out,
                    int major, int in_h, int in_w, int minor,
                    int kernel_h, int kernel_w,
                    int up_x, int up_y, int down_x, int down_y,
                    int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                    int force_path, void *stream);

/*
 * Same op on a row/plane-strided input (minor must be 1 when strides are not the contiguous ones):
 * element (n, y, x) of the input lives at input[n*in_plane_stride + y*in_row_stride + x] (strides in elements).
 * Used for the private conv_transpose -> blur intermediate of ModulatedConv2d(upsample) (stylegan2.py:276-279):
 * its rows are 2W+1 floats, never 16-byte aligned when contiguous; with row stride round_up(2W+2, 4) and a
 * one-float left offset every dwordx4 load of the blur is aligned (4.08 -> 4.8 TB/s on the 1024^2 layer).
 */
int fmgan_upfirdn2d_strided(int dtype, const void *input, const void *kernel, void *out,
                            int major, int in_h, int in_w, int minor,
                            long long in_plane_stride, int in_row_stride,
                            int kernel_h, int kernel_w,
                            int up_x, int up_y, int down_x, int down_y,
                            int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                            int force_path, void *stream);

/*
 * The tail of an upsampling StyledConv in one pass (stylegan2.py:279 + 371-373): 4x4 (or smaller) FIR blur of the
 * transposed-conv result, then noise + bias + leaky ReLU * scale applied to the filtered value before it is stored:
 *   out[b,c,y,x] = lrelu( (blur(in)[b,c,y,x] + noise_weight[0]*noise[b or 0,y,x]) + bias[c] ) * act_scale
 * in [batch*channels planes, in_h, in_w] with element strides as in fmgan_upfirdn2d_strided; out contiguous
 * [batch,channels,out_h,out_w]; noise [noise_batch (1|batch), out_h*out_w] or NULL; bias [channels] or NULL.
 * Served by the row-march kernels (out_w >= 64) and, for small planes (in_h*in_w <= 12288: the 4^2..32^2 upsampling
 * layers), by the plane-tile kernel; FMGAN_EUNSUPPORTED otherwise — the caller then runs fmgan_upfirdn2d(_strided)
 * followed by fmgan_noise_bias_act_f32, which gives bit-identical results (same kernel family, same roundings).
 */
int fmgan_blur_noise_bias_act_f32(const float *input, const float *kernel, float *out,
                                  int batch, int channels, int in_h, int in_w,
                                  long long in_plane_stride, int in_row_stride,
                                  int kernel_h, int kernel_w,
                                  int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                                  const float *noise, const float *noise_weight, const float *bias,
                                  int noise_batch, float alpha, float act_scale, void *stream);
/* Which kernel serves a fused-blur call with these arguments (host logic, nothing is launched): 5 = LDS-DMA ring
 * (path 1b), 1 = register row-march (path 1), 2 = plane-tile.  It is the launch's own plan with the launch left out: a
 * positive id is returned exactly when fmgan_blur_noise_bias_act_f32 with these arguments runs that kernel; otherwise the
 * launch's status (FMGAN_EUNSUPPORTED: no kernel serves the shape; FMGAN_EINVAL / FMGAN_EOVERFLOW as the launch, and
 * FMGAN_EINVAL for batch <= 0, where the launch of an empty batch is a no-op).  Path 1b is chosen by address: called
 * without addresses the answer is 1 or 2, never 5.  bench.py names the kernel of its roofline object from this. */
int fmgan_blur_noise_bias_act_select(const float *input, const float *out, const float *noise,
                                     int batch, int channels, int in_h, int in_w,
                                     long long in_plane_stride, int in_row_stride,
                                     int kernel_h, int kernel_w,
                                     int pad_x0, int pad_x1, int pad_y0, int pad_y1);
/* The same with the row-march variant chosen by the caller (tests, measurements): force_path -1 / 1 automatic,
 * 4 = register row-march (path 1), 5 = LDS-DMA ring (path 1b; FMGAN_EUNSUPPORTED when its alignment rules do not hold).
 * Both variants produce the same bits.  fmgan_upfirdn2d(_strided) accept the same two values. */
int fmgan_blur_noise_bias_act_path_f32(const float *input, const float *kernel, float *out,
                                       int batch, int channels, int in_h, int in_w,
                                       long long in_plane_stride, int in_row_stride,
                                       int kernel_h, int kernel_w,
                                       int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                                       const float *noise, const float *noise_weight, const float *bias,
                                       int noise_batch, float alpha, float act_scale, int force_path, void *stream);

/*
 * fused_bias_act: out[i] = act'(x[i] + bias[(i / step_b) % size_b]; refer[i]) * scale
 *   act*10+grad: 10,11 linear; 12 zero; 30 lrelu(x); 31 (refer>0 ? x : alpha*x); 32 zero
 *   (op/fused_bias_act_kernel.cu:36-45).  bias == NULL or size_b == 0: no bias;
 *   refer == NULL: refer treated as 0 (the reference passes an empty tensor).
 *   x, refer, out: `size_x` contiguous elements of `dtype`; bias: `size_b` elements.
 *   step_b = product of x.shape[2:] (op/fused_bias_act_kernel.cu:67-71).
 */
int fmgan_fused_bias_act(int dtype, const void *x, const void *bias, const void *refer,
                         void *out, long long size_x, int size_b, int step_b,
                         int act, int grad, float alpha, float scale, void *stream);

/*
 * StyledConv epilogue in one pass (stylegan2.py:360-376: NoiseInjection then FusedLeakyReLU):
 *   out[b,c,p] = lrelu(x[b,c,p] + noise_weight[0] * noise[b or 0, p] + bias[c]) * scale
 *   x/out [batch, channel, hw] f32; noise [noise_batch (1 or batch), hw] f32 or NULL;
 *   noise_weight device scalar f32 (NoiseInjection.weight, stylegan2.py:305) or NULL; bias [channel] or NULL.
 */
int fmgan_noise_bias_act_f32(const float *x, const float *noise, const float *noise_weight,
                             const float *bias, float *out,
                             int batch, int channel, int hw, int noise_batch,
                             float alpha, float scale, void *stream);

/*
 * FusedLeakyReLUFunctionBackward in one pass (op/fused_act.py:29-50: fused_bias_act(grad_output, empty, out, 3, 1, ...)
 * followed by grad_input.sum over batch and space for the bias):
 *   grad_in[p,i] = (ref_out[p,i] > 0 ? grad_out[p,i] : alpha * grad_out[p,i]) * scale     (bits of fmgan_fused_bias_act 3/1)
 *   partial[p, blk] = sum of the block's share of grad_in[p, :]
 * over `planes` = batch*channels contiguous planes of `hw` f32 elements; partial [planes, fmgan_fused_bias_act_bwd_blocks]
 * — the caller sums it to [channels] (deterministic).  hw % 4 == 0, hw >= 64 and 16-byte aligned pointers, else
 * FMGAN_EUNSUPPORTED (fmgan_fused_bias_act_bwd_blocks returns 0): the caller then uses fmgan_fused_bias_act + a sum.
 */
int fmgan_fused_bias_act_bwd_blocks(long long planes, int hw);
int fmgan_fused_bias_act_bwd_f32(const float *grad_out, const float *ref_out, float *grad_in, float *partial,
                                 long long planes, int hw, float alpha, float scale, void *stream);

/*
 * Backward of PReLU(channels) on channels-innermost activations (the pSp encoder's units,
 * psp_encoder_model/encoders/helpers.py:107,130, run in NHWC): x/grad/grad_x [rows, channels] f32, slope [channels],
 *   grad_x = grad * (x > 0 ? 1 : slope[c]);   partial[blk, c] = sum over the block's rows of grad * x * (x <= 0)
 * partial [fmgan_prelu_backward_blocks(rows, channels), channels]: the caller sums it over dim 0 (deterministic).
 * channels % 4 == 0 and 16-byte aligned pointers, else FMGAN_EUNSUPPORTED.
 */
int fmgan_prelu_backward_blocks(long long rows, int channels);
int fmgan_prelu_backward_f32(const float *x, const float *grad, const float *slope, float *grad_x,
                             float *partial, long long rows, int channels, void *stream);

/*
 * Face-regional loss of the dual-supervision G step (Util/training_util.py:228-256, Get_Render_Mask +
 * Face_Regional_Loss) on a render r and a generated image g, both [batch, channels, hw] contiguous f32 (hw = H*W):
 *   m[b,p] = (sum_c r[b,c,p]) * (1/C) > -1, with the serial fp32 channel sum and the float factor of ATen's
 *            r.mean(1) (bit-identical to it for channels <= 4)
 *   fmgan_face_region_loss_f32     : partial[b, blk] = sum over block blk's pixels of sample b of m * (r - g)^2;
 *                                    partial [batch, fmgan_face_region_blocks(batch, hw)], fixed association (no atomics):
 *                                    the caller sums each row (S[b]); loss = sum_b S[b] / (batch*channels*hw)
 *   fmgan_face_region_backward_f32 : grad_g = grad_loss[0] * 2/(batch*channels*hw) * m * (g - r), 0 where m = 0;
 *                                    grad_loss is a DEVICE scalar (no host synchronisation)
 *   fmgan_render_mask_f32          : mask [batch, hw] = m as 0.f / 1.f
 * 16-byte loads when hw % 4 == 0 and the pointers are 16-byte aligned, otherwise a scalar form with the same arithmetic
 * in the same order (same bits).  FMGAN_EOVERFLOW when batch*channels*hw does not fit a long long.
 */
int fmgan_face_region_blocks(int batch, long long hw);
int fmgan_face_region_loss_f32(const float *r, const float *g, float *partial, int batch, int channels, long long hw,
                               void *stream);
int fmgan_face_region_backward_f32(const float *r, const float *g, const float *grad_loss, float *grad_g, int batch,
                                   int channels, long long hw, void *stream);
int fmgan_render_mask_f32(const float *r, float *mask, int batch, int channels, long long hw, void *stream);

/*
 * Metric stage of the quantitative evaluation (Evaluation/quant_eval.py:25-49, 100): the face-recognition network's input
 * of one or two [batch, 3, h, w] contiguous f32 image batches and the per-sample L1 between them, every element read once.
 *   gray_x[b,0,oy,ox] = (1/k^2) * sum over the k x k window of (c0*x0 + c1*x1) + c2*x2   ([batch, 1, h/k, w/k];
 *                       RGB_to_GrayScale + avg_pool2d(k, k), Util/training_util.py:130-161).  The three products are
 *                       rounded separately (coefficients float(0.2989), float(0.587), float(0.114)), no fused
 *                       multiply-add; the window sum is serial from 0, rows top to bottom, columns left to right.
 *   l1_partial[b, blk] = sum over block blk's share of sample b of |a - b|; [batch, fmgan_face_input_blocks(...)], fixed
 *                       association (no atomics, longest serial chain 40 additions): the caller sums each row and
 *                       divides by 3*h*w.
 * NULL b, gray_a, gray_b or l1_partial: not wanted.  gray_b or l1_partial without b, or no output at all: FMGAN_EINVAL.
 * Served: k in {1, 2, 4, 8}, h % k == 0, w % k == 0; FMGAN_EUNSUPPORTED otherwise (fmgan_face_input_blocks returns 0, as
 * it does whenever the launch would refuse the shape): the caller then evaluates the composite.  FMGAN_EOVERFLOW when
 * batch*3*h*w does not fit a long long, h*w does not fit 31 bits, or batch * blocks exceeds the grid's 2^31 - 1.
 * 16-byte loads when w % 4 == 0 and a, b are 16-byte aligned, otherwise a bounded scalar form with the same arithmetic
 * in the same order (same bits).
 */
int fmgan_face_input_blocks(int batch, int h, int w, int k);
int fmgan_face_input_f32(const float *a, const float *b, float *gray_a, float *gray_b, float *l1_partial, int batch,
                         int h, int w, int k, void *stream);

/*
 * Input stage of the perceptual path length (Evaluation/ppl.py; lpips ScalingLayer): from the Generator's interleaved
 * image batch to the two inputs of the channels_last VGG trunk, every needed source pixel read once.
 *   img [2*pairs, 3, h, w] contiguous f32 NCHW; sample 2p is the first image of pair p, sample 2p+1 the second.
 *   Window: rows y0 .. y0+hc, columns x0 .. x0+wc (the whole image: 0, 0, h, w);  oh = hc/f, ow = wc/f.
 *   v = img[n, c, y0+y, x0+x] at f = 1; at f = 2 or 4, with o = f/2 - 1, a, b the pixels at row y0+f*y+o, columns
 *       x0+f*x+o and +1, and c, d the same columns one row below:  v = 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d), in
 *       exactly this association (columns inside a row first), no fused multiply-add.  This is bilinear interpolation
 *       with align_corners = false at the integer ratios 2 and 4 (source index f*d + f/2 - 0.5: both weights 1/2).
 *   out0[p, y, x, c] (n = 2p) / out1[p, y, x, c] (n = 2p+1) = (v - shift[c]) / scale[c], IEEE subtraction and correctly
 *       rounded division; [pairs, oh, ow, 3] dense: the NHWC storage of a [pairs, 3, oh, ow] channels_last tensor.
 *   shift, scale: DEVICE pointers to three floats each, read by the kernel (no host copy, no synchronisation).
 * No allocation, no synchronisation, no global state; the kernel runs on `stream`.  Dword-aligned pointers suffice.
 * fmgan_lpips_pair_input_select is the launch's plan with the launch left out: a positive kernel id exactly when the
 * launch with these arguments runs that kernel (f: the vector form, ow % 4 == 0, a lane writes four pixels as three
 * 16-byte stores; 8 + f: the bounded form for any other width, same arithmetic, same bits), otherwise the status the
 * launch returns: FMGAN_EINVAL for pairs <= 0, non-positive sizes or a window outside the image (the launch also for a
 * NULL pointer), FMGAN_EUNSUPPORTED for f outside {1, 2, 4} or hc % f != 0 or wc % f != 0 (the caller then evaluates the
 * composite), FMGAN_EOVERFLOW when h*w does not fit 31 bits, 2*pairs*3*h*w does not fit a long long, or samples * blocks
 * exceeds the grid's 2^31 - 1.
 */
int fmgan_lpips_pair_input_select(int pairs, int h, int w, int y0, int x0, int hc, int wc, int f);
int fmgan_lpips_pair_input_f32(const float *img, const float *shift, const float *scale, float *out0, float *out1,
                               int pairs, int h, int w, int y0, int x0, int hc, int wc, int f, void *stream);

/*
 * Image stage of the projection criterion (Evaluation/image_projection/project: mse (+ mask) and the LPIPS trunk input
 * of the optimised image), forward and backward, one launch each.
 *   x, target [batch, 3, h, w] contiguous f32 NCHW, h = w = 256 * f, f in {1, 2, 4};  mask [h, w] f32 or NULL.
 *   forward : partial[i], i < fmgan_projection_loss_blocks(...): the sum over block i's elements of q = (x - t)^2, or of
 *             q * mask[row, col]; per-lane serial fma, wave butterfly, waves in order: no atomics, bit-reproducible.  The
 *             caller adds the partials (in float64).
 *             y [batch, 256, 256, 3] dense (NHWC storage of a channels_last [batch, 3, 256, 256]) or NULL (not wanted):
 *             with a = clamp(x, -1, 1) (NaN stays NaN), v = a at f = 1; at f = 2 or 4, with o = f/2 - 1, a, b the clamped
 *             pixels at row f*i + o, columns f*j + o and + 1, and c, d the same columns one row below,
 *                 v = 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d)
 *             in exactly this association (columns inside a row first), no fused multiply-add: bilinear interpolation
 *             to 256 with align_corners = false;  y[n, i, j, c] = (v - shift[c]) / scale[c], IEEE subtraction and
 *             correctly rounded division.  shift, scale: DEVICE pointers to three floats (needed only with y).
 *   backward: grad_x[n, c, row, col] = (k[0] * (x - t)) * mask[row, col] + p,  (without a mask: k[0] * (x - t) + p)
 *             p = wf * (g_y[n, row/f, col/f, c] / scale[c]) where -1 <= x <= 1 (the bounds included) and (row, col) is
 *             one of the four taps of its reduced pixel, 0 otherwise, wf = 1 at f = 1 and 0.25 at f = 2, 4; in exactly
 *             this association, no fused multiply-add.  g_y NULL: p = 0 everywhere.  k: DEVICE pointer to one float,
 *             grad_loss * 2 * mse_weight / denominator (no host copy, no synchronisation).
 *   The mask multiplies: a NaN of x or target reaches the sum and its own grad_x element also where the mask is 0.
 * No allocation, no synchronisation, no global state; the kernels run on `stream`.  Dword-aligned pointers suffice.
 * fmgan_projection_loss_select is the launch's plan with the launch left out: the positive kernel id f exactly when the
 * launches with these arguments run, otherwise the status they return: FMGAN_EINVAL for a non-positive argument (the
 * launches also for a NULL x, target, partial, grad_x or k, a y without shift and scale, a g_y without scale),
 * FMGAN_EUNSUPPORTED for h != w, h outside {256, 512, 1024} or f != h / 256 (the caller then evaluates the composite),
 * FMGAN_EOVERFLOW when batch * blocks per sample exceeds the grid's 2^31 - 1 (element offsets are 64-bit).
 * fmgan_projection_loss_blocks: the number of partials, 0 where select is not positive.
 */
int fmgan_projection_loss_select(int batch, int h, int w, int f);
int fmgan_projection_loss_blocks(int batch, int h, int w, int f);
int fmgan_projection_loss_fwd_f32(const float *x, const float *target, const float *mask, const float *shift,
                                  const float *scale, float *partial, float *y, int batch, int h, int w, int f,
                                  void *stream);
int fmgan_projection_loss_bwd_f32(const float *x, const float *target, const float *mask, const float *g_y,
                                  const float *k, const float *scale, float *grad_x, int batch, int h, int w, int f,
                                  void *stream);

/*
 * Running feature statistics of the FID (Evaluation/fid.py; op/fid_stats.py): first and second moments of the Inception
 * features, accumulated on the device in float64, batch by batch; doubles travel by pointer.
 *   State over d features: shift [d] f64 (fixed before the first update), sum [d] f64, outer [d, d] f64 row-major of which
 *   only the elements with i <= j are meaningful (the others are never read or written); the sample count is the caller's.
 *   update: feat [b, d] contiguous f32 row-major;  y[r, c] = (double)feat[r, c] - shift[c]  (one rounding),
 *             sum[c]      = sum[c]      + ((g0 + g1) + g2) + g3,  g_k = y[k, c] + y[k+4, c] + y[k+8, c] + ... in row order,
 *             outer[i][j] = outer[i][j] + P_ij  for i <= j,       P_ij = sum_r y[r, i] * y[r, j] on the fp64 matrix
 *           instruction (v_mfma_f64_16x16x4_f64): rows in order, four per instruction, starting from 0; rows beyond b are
 *           exact zeros.  Accumulation is in place; every element is read, added to and written by one lane: no atomics,
 *           and the bits do not depend on the grid.  Only 16 x 16 tiles on or above the diagonal are computed.
 *   finish: n the number of samples accumulated;  mean[i] = shift[i] + sum[i] / n;
 *           cov[i][j] = cov[j][i] = (outer[i][j] - (sum[i] * sum[j]) / n) / (n - 1)  for i <= j, in this order, no fused
 *           multiply-add, n converted to double: cov [d, d] f64 is exactly symmetric.  Any d.
 * No allocation, no synchronisation, no global state; the kernels run on `stream`.  Naturally aligned pointers suffice.
 * fmgan_fid_stats_select is update's plan with the launch left out: the positive kernel id 1 exactly when the launch with
 * these arguments runs, otherwise the status it returns: FMGAN_EINVAL for b <= 0 or d <= 0 (the launch also for a NULL
 * pointer), FMGAN_EUNSUPPORTED for d % 16 != 0 (the caller then evaluates the composite), FMGAN_EOVERFLOW for d > 2^21
 * (block indices are ints, element offsets 64-bit).  finish: FMGAN_EINVAL for n < 2, d <= 0 or a NULL pointer,
 * FMGAN_EOVERFLOW for d > 16 * 65535.
 */
int fmgan_fid_stats_select(int b, int d);
int fmgan_fid_stats_update_f32(const float *feat, const double *shift, double *sum, double *outer, int b, int d,
                               void *stream);
int fmgan_fid_stats_finish_f64(const double *sum, const double *outer, const double *shift, long long n, double *mean,
                               double *cov, int d, void *stream);

/*
 * Input stage of the FID's Inception network (Evaluation/inception.py): from the Generator's image batch to the
 * channels_last input of the first convolution, one launch, only tap pixels read.
 *   img [batch, 3, s, s] contiguous f32 NCHW, s in {256, 512, 1024, 299};  out [batch, 299, 299, 3] dense: the NHWC storage
 *   of a [batch, 3, 299, 299] channels_last tensor.
 *   v = bilinear interpolation to 299 x 299 with align_corners = false by aten's fp32 rule, per axis and output index d:
 *         scale = (float)s / 299.f;  src = max(fmaf(scale, d + 0.5f, -0.5f), 0.f)  (ONE rounding: aten's kernels are
 *         compiled with the multiply and subtract contracted);  i0 = (int)src;  i1 = i0 + (i0 < s - 1);
 *         l1 = src - i0;  l0 = 1.f - l1;
 *       with (y0, y1, h0, h1) those of the output row and (x0, x1, w0, w1) those of the output column,
 *         v = h0 * (w0 * img[y0, x0] + w1 * img[y0, x1]) + h1 * (w0 * img[y1, x0] + w1 * img[y1, x1]),
 *       every product and sum rounded, in exactly this association, no fused multiply-add.  A tap of weight 0 is read and
 *       multiplied (its NaN reaches the output), as in aten.  s = 299: v = img, nothing is multiplied.
 *   out[n, y, x, c] = normalize ? 2 * v - 1 : v  (2 * v is exact: one rounding).
 * No allocation, no synchronisation, no global state; the kernel runs on `stream`.  Dword-aligned pointers suffice.
 * fmgan_inception_input_select is the launch's plan with the launch left out: a positive kernel id exactly when the launch
 * with these arguments runs that kernel (1: resampling, 2: s = 299, layout change only), otherwise the status the launch
 * returns: FMGAN_EINVAL for a non-positive argument (the launch also for a NULL pointer), FMGAN_EUNSUPPORTED for h != w
 * or h outside {256, 512, 1024, 299} (the caller then evaluates the composite), FMGAN_EOVERFLOW when batch * blocks per
 * sample exceeds the grid's 2^31 - 1 (element offsets are 64-bit).
 */
int fmgan_inception_input_select(int batch, int h, int w);
int fmgan_inception_input_f32(const float *img, float *out, int batch, int h, int w, int normalize, void *stream);

/*
 * Tensor work around the landmark networks (Util/landmark_util.py; Util/training_util.py Heat_Map_Loss): face crop forward
 * and backward, the detector's input, the heat-map distance forward and backward, the landmark decode.  One launch each,
 * f32, no atomics: the same input gives the same bits.  All tensors contiguous.
 *   face crop: img [batch, 3, h, w] NCHW in [-1, 1];  box: DEVICE pointer to [batch, 4] 32-bit ints (ux, uy, bx, by), read
 *     by the kernel;  out [batch, 3, r, r].  Per sample the canvas has hc = by - uy rows and wc = bx - ux columns,
 *       canvas[c, y, x] = ((img[c, y + uy, x + ux] + 1) * 255) * 0.5  where 0 <= y + uy < h and 0 <= x + ux < w, else 0,
 *       out = bilinear(canvas -> r x r, align_corners = false) / 255  (correctly rounded division),
 *     taps and weights per axis by the fp32 rule stated for fmgan_inception_input_f32 with scale = (float)hc / (float)r
 *     (wc for columns), v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d), every product and sum rounded.  The canvas is
 *     never stored; any ratio, up or down (two taps per axis, no antialiasing).  A box with a side outside [1, 2^24]
 *     gives a zero crop and a zero gradient.  Every read of img is bounds-tested whatever the box holds.
 *     backward: grad_img[n, c, y, x] = ((sum of (hk * wk) * (grad_out[n, c, oy, ox] / 255)) * 0.5) * 255 over the output
 *     pixels and taps that name canvas pixel (y - uy, x - ux), output rows, then columns, then the row tap, then the
 *     column tap ascending; the taps are found with the forward's own function.  Exactly 0 outside the crop.
 *   fmgan_face_crop_select: the launches' plan with the launch left out: 1 when they run, FMGAN_EINVAL for a non-positive
 *     argument (the launches also for a NULL pointer), FMGAN_EOVERFLOW for h, w or r above 2^15 or a grid above 2^31 - 1.
 *   detector input: out[n, c] = ((img[n, 2 - c] + 1) * 255) * 0.5 - mean[c], mean = (104, 117, 123), planes of hw elements.
 *   heat-map distance: a, b [batch, m], m % 4 == 0 (else FMGAN_EUNSUPPORTED: the caller evaluates the composite).
 *     forward : partial[n * blocks + i], blocks = fmgan_heatmap_distance_blocks(batch, m) (0 where the launch does not
 *               run): the sum of (a - b)^2 over elements [4096 i, 4096 (i + 1)) of sample n; per-lane serial fma, wave
 *               butterfly, waves in order.  The caller adds a sample's partials (in float64).
 *     backward: grad_a = (2 * g[n]) * (a - b), grad_b = -grad_a; either may be NULL (not wanted), not both.  g: DEVICE
 *               pointer to [batch] floats, the upstream gradient (no host copy, no synchronisation).
 *   landmark decode (_get_preds_fromhm_torch): hm [batch, channels, 64, 64] (another size: FMGAN_EUNSUPPORTED), one wave
 *     per map.  idx = argmax over the 4096 values, the smallest index on a tie, NaN above every number;
 *     px = idx % 64, py = idx / 64;  (x, y) = (px + 1, py + 1), plus 0.25 * sign(hm[py][px + 1] - hm[py][px - 1]) and
 *     0.25 * sign(hm[py + 1][px] - hm[py - 1][px]) where 0 < px, py < 63 (sign(0) = 0), minus 0.5:
 *     preds[b, c] = (x, y).  center [batch, 2], scale [batch]: DEVICE pointers, both or neither; with them
 *     preds_orig[b, c] = trunc((p - 64 * (-center / hs + 0.5)) * hs / 64), hs = 200 * scale[b], per coordinate, in this
 *     association, no fused multiply-add; without them zeros.  preds, preds_orig [batch, channels, 2].
 * No allocation, no synchronisation, no global state; the kernels run on `stream`.  Dword-aligned pointers suffice.
 */
int fmgan_face_crop_select(int batch, int h, int w, int r);
int fmgan_face_crop_fwd_f32(const float *img, const void *box, float *out, int batch, int h, int w, int r, void *stream);
int fmgan_face_crop_bwd_f32(const float *grad_out, const void *box, float *grad_img, int batch, int h, int w, int r,
                            void *stream);
int fmgan_detector_input_f32(const float *img, float *out, int batch, long long hw, void *stream);
int fmgan_heatmap_distance_blocks(int batch, long long m);
int fmgan_heatmap_distance_fwd_f32(const float *a, const float *b, float *partial, int batch, long long m, void *stream);
int fmgan_heatmap_distance_bwd_f32(const float *a, const float *b, const float *g, float *grad_a, float *grad_b, int batch,
                                   long long m, void *stream);
int fmgan_landmark_decode_f32(const float *hm, const float *center, const float *scale, float *preds, float *preds_orig,
                              int batch, int channels, int h, int w, void *stream);

/*
 * Inference glue of the pSp encoder's IR / IR-SE units (psp_encoder_model/encoders/helpers.py): what runs between the
 * MIOpen convolutions of a unit.  All tensors f32 in NHWC storage ([batch, h, w, channels]); a BatchNorm2d in eval mode is
 * given as its four [channels] vectors and eps and is evaluated in-kernel on every launch as
 *   bn(v) = (v - mean[c]) * (gamma[c] * (1 / sqrt(var[c] + eps))) + beta[c]
 *   fmgan_bn_prelu_f32 : t = prelu(bn(x), slope[c]);  y = t (y may be NULL);  y_next = bn_next(t) (NULL: not wanted, the
 *                        next_* vectors are then ignored);  y_sub [batch, (h-1)/s+1, (w-1)/s+1, channels] = t[:, ::s, ::s]
 *                        with s = sub_stride >= 1 (NULL: not wanted).  At least one output.
 *   fmgan_se_pool_f32  : partial[b, k, c] = sum over the rows of chunk k, in pixel order, of r[b, :, :, c];
 *                        partial [batch, fmgan_se_pool_chunks(batch, channels, h, w), channels]
 *   fmgan_se_gate_f32  : pooled = bn(sum_k partial[b, k, :] / hw) (chunks in order; the mean of the affine map is the affine
 *                        map of the mean);  gate[b, :] = sigmoid(fc2 . relu(fc1 . pooled)),  fc1 [mid, channels],
 *                        fc2 [channels, mid];  gate [batch, channels]
 *   fmgan_ir_tail_f32  : out = bn(r) * gate[b, c] + shortcut (gate NULL: no SE gate);  out_next = bn_next(out) (NULL: not
 *                        wanted).  With the sc_* vectors given, shortcut [batch, h, w, channels] is the 1x1 shortcut
 *                        convolution's output and bn_sc is applied to it (sc_h = h, sc_w = w, sc_stride = 1); with all
 *                        four NULL it is the unit's input [batch, sc_h, sc_w, channels] read in place at (s*y, s*x),
 *                        s = sc_stride, (sc_h-1)/s+1 = h and (sc_w-1)/s+1 = w  (MaxPool2d(1, s)).
 * No atomics, fixed summation order: bit-reproducible.  Served: channels % 4 == 0, channels <= 1024 (se_gate: mid <= 256)
 * and 16-byte aligned pointers; FMGAN_EUNSUPPORTED otherwise (fmgan_se_pool_chunks returns 0): the caller then runs the
 * modules.  batch == 0 returns FMGAN_OK before anything else; FMGAN_EOVERFLOW when batch > 65535 or a row index / an
 * offset inside a row does not fit 32 bits (tensor offsets are 64-bit).
 */
int fmgan_bn_prelu_f32(const float *x, const float *mean, const float *var, const float *gamma, const float *beta,
                       float eps, const float *slope, float *y, const float *next_mean, const float *next_var,
                       const float *next_gamma, const float *next_beta, float next_eps, float *y_next, float *y_sub,
                       int batch, int channels, int h, int w, int sub_stride, void *stream);
int fmgan_se_pool_chunks(int batch, int channels, int h, int w);
int fmgan_se_pool_f32(const float *r, float *partial, int batch, int channels, int h, int w, void *stream);
int fmgan_se_gate_f32(const float *partial, int chunks, long long hw, const float *mean, const float *var,
                      const float *gamma, const float *beta, float eps, const float *fc1, const float *fc2, float *gate,
                      int batch, int channels, int mid, void *stream);
int fmgan_ir_tail_f32(const float *r, const float *mean, const float *var, const float *gamma, const float *beta,
                      float eps, const float *gate, const float *shortcut, int sc_h, int sc_w, int sc_stride,
                      const float *sc_mean, const float *sc_var, const float *sc_gamma, const float *sc_beta, float sc_eps,
                      float *out, const float *next_mean, const float *next_var, const float *next_gamma,
                      const float *next_beta, float next_eps, float *out_next, int batch, int channels, int h, int w,
                      void *stream);

/*
 * LPIPS distance of one VGG tap (lpips/__init__.py, PNetLin.forward: unit-normalise over channels, squared difference,
 * 1x1 conv to one channel, spatial mean) and its data gradients.  f0, f1 [batch, hw, channels] f32 (NHWC storage of
 * [batch, channels, H, W] features, hw = H*W), w [channels] the 1x1 weight:
 *   r_k = sqrt(sum_c f_k^2),  n_k = r_k + eps,  u_k = f_k / n_k                      (per pixel)
 *   fmgan_lpips_distance_f32          : partial[b, blk] = sum over block blk's pixels of sample b of
 *                                       sum_c w_c (u0_c - u1_c)^2; partial [batch, fmgan_lpips_distance_blocks(...)],
 *                                       fixed association (no atomics): the caller sums each row and divides by hw
 *   fmgan_lpips_distance_backward_f32 : with q1_c = -2 w_c (u0_c - u1_c) grad[b]/hw and q0 = -q1,
 *                                       grad_fk_c = (qk_c - fk_c * (sum_c' qk_c' fk_c') / (r_k n_k)) / n_k;
 *                                       grad [batch] is read on the DEVICE (no host synchronisation); grad_f0 / grad_f1
 *                                       like f0 / f1, either may be NULL (not wanted), not both.  A pixel whose f_k is
 *                                       exactly zero gets NaN in grad_fk (0/0, as autograd's sqrt backward) and
 *                                       touches no other pixel.
 * Served: channels in {64, 128, 256, 512} and 16-byte aligned pointers; FMGAN_EUNSUPPORTED otherwise
 * (fmgan_lpips_distance_blocks returns 0 for such a channel count): the caller then evaluates the composite.
 * batch == 0 returns FMGAN_OK before anything else; batch > 65535 or hw * channels >= 2^30 (a sample's element offsets
 * are 32-bit) returns FMGAN_EOVERFLOW, and fmgan_lpips_distance_blocks 0.
 */
int fmgan_lpips_distance_blocks(int batch, int channels, int hw);
int fmgan_lpips_distance_f32(const float *f0, const float *f1, const float *w, float *partial, int batch, int channels,
                             int hw, float eps, void *stream);
int fmgan_lpips_distance_backward_f32(const float *f0, const float *f1, const float *w, const float *grad,
                                      float *grad_f0, float *grad_f1, int batch, int channels, int hw, float eps,
                                      void *stream);

/*
 * Demodulation coefficients of ModulatedConv2d (stylegan2.py:258-262):
 *   demod[b,o] = rsqrt( sum_{i,k} (scale * weight[o,i,k] * style[b,i])^2 + eps )
 *   weight [cout, cin, ktaps] f32 (the [1,cout,cin,k,k] parameter), style [batch, cin] f32,
 *   demod [batch, cout] f32.  One wave per output channel; the sum over cin is a wave-shuffle reduction.
 */
int fmgan_modconv_demod_f32(const float *weight, const float *style, float *demod,
                            int batch, int cout, int cin, int ktaps,
                            float scale, float eps, void *stream);

/*
 * Winograd F(2x2,3x3) form of the plain 3x3 modulated conv (mode 0 of fmgan_modconv2d_f32; /root/reference/stylegan2.py:250-298):
 * 16 products per 2x2 output tile instead of 36.  Three steps; the middle one is a plain batched GEMM done by the caller
 * (M[xi] = U[xi] @ V[xi], xi = 0..15).  H and W even; T = (H/2)*(W/2) tiles per sample; fp32; results differ from the direct
 * kernel by fp32 rounding of re-associated sums.
 *   fmgan_wino_weight_f32:  wt [cin,9,cout] (fmgan_modconv_weight_prep_f32, kind 0) -> U [16, cout, cin]
 *   fmgan_wino_input_f32:   x [B,C,H,W], style [B,C] -> V [16, C, B*T]   (column b*T + ty*(W/2) + tx; modulated, zero padded)
 *   fmgan_wino_output_f32:  M [16, cout, B*T] -> out [B,cout,H,W] contiguous = epilogue(demod * At M A); demod / noise /
 *                           bias may be NULL; epilogue as fmgan_modconv2d_f32 with fuse_act
 * The two activation transforms each have two kernels that give the same bits: one thread per strip of four horizontally
 * adjacent tiles with 16-byte accesses throughout, taken where (W/2) % 4 == 0 and x and V (M, out and the noise plane) start
 * on 16-byte boundaries — by the output transform only on rows of at least 32 floats —, and one thread per tile for
 * everything else.
 *   fmgan_wino_select:      which of them a launch with these sizes takes (pure host logic, no launch): 1 = strips, 0 = one
 *                           tile per thread; output: 0 = fmgan_wino_input_f32, 1 = fmgan_wino_output_f32 (c = cout);
 *                           all_aligned16: every such pointer of the launch is 16-byte aligned.  Sizes the launch refuses
 *                           return its FMGAN_EINVAL.
 */
int fmgan_wino_select(int output, int batch, int c, int h, int w, int all_aligned16);
int fmgan_wino_weight_f32(const float *wt, float *u, int cin, int cout, void *stream);
int fmgan_wino_input_f32(const float *x, const float *style, float *v, int batch, int c, int h, int w, void *stream);
int fmgan_wino_output_f32(const float *m, const float *demod, const float *noise, const float *noise_weight,
                          const float *bias, float *out, int batch, int cout, int h, int w, int noise_batch,
                          int fuse_act, float alpha, float act_scale, void *stream);

/*
 * EqualLinear at inference batch sizes (replaces F.linear(input, weight*scale, bias=bias*lr_mul) of
 * /root/reference/stylegan2.py:146-180 where it is a ModulatedConv2d's modulation, stylegan2.py:226):
 *   out[b,n] = sum_k x[b,k] * weight[n,k] (+ bias[n])      x [batch,k_in], weight [n_out,k_in] (already scaled), bias [n_out] or NULL
 * One wave per (n, b), fixed summation order: bit-reproducible and independent of the batch size.
 */
int fmgan_equal_linear_f32(const float *x, const float *weight, const float *bias, float *out,
                           int batch, int n_out, int k_in, void *stream);

/*
 * The same coefficients in two steps, for weights that change rarely (inference, or once per optimiser step):
 *   fmgan_modconv_wsq_f32:        wsq[o,i] = sum_k weight[o,i,k]^2          [cout, cin] f32, cached by the caller
 *   fmgan_modconv_demod_wsq_f32:  demod[b,o] = rsqrt(scale^2 * sum_i wsq[o,i] * style[b,i]^2 + eps)
 * Same fma chains in the same order as fmgan_modconv_demod_f32: bit-identical results; the per-forward kernel reads
 * cout*cin floats instead of cout*cin*ktaps.
 */
int fmgan_modconv_wsq_f32(const float *weight, float *wsq, int cout, int cin, int ktaps, void *stream);
int fmgan_modconv_demod_wsq_f32(const float *wsq, const float *style, float *demod,
                                int batch, int cout, int cin, float scale, float eps, void *stream);

/*
 * Weight layouts for the MFMA contraction (last index contiguous, so a 32-lane MFMA A-operand read is one LDS bank
 * row and staging is coalesced).  weight [cout, cin, ktaps] f32; wt pre-allocated, cout*cin*ktaps floats:
 *   kind 0  wt[i][tap][o] = scale * weight[o][i][tap]            forward (modes 0, 1, and the downsample branch, mode 2)
 *   kind 1  wt[o][tap][i] = scale * weight[o][i][ktaps-1-tap]    data-gradient of the plain conv    (run as mode 0)
 *   kind 2  wt[o][tap][i] = scale * weight[o][i][tap]            data-gradient of the transposed conv (run as mode 2)
 * Depends on the parameter only.  The host shim never caches it across forwards (in-place parameter updates
 * through `.data` give no invalidation signal): inference re-derives every layer's table with fmgan_weight_refresh_f32.
 */
int fmgan_modconv_weight_prep_f32(const float *weight, float *wt, int cout, int cin, int ktaps,
                                  float scale, int kind, void *stream);

/*
 * All derived weights of a network, re-derived from the live parameters in ONE launch per inference forward
 * (replaces the per-call `weight * scale` / `bias * lr_mul` of every EqualLinear, stylegan2.py:165-175, and the
 * per-call weight preparation of every ModulatedConv2d, stylegan2.py:257-262; nothing is cached across forwards, so
 * the reference's in-place EMA update `accumulate`, train_3_encoder.py:195-200, needs no invalidation hook).
 *   table_dev: DEVICE array of n_entries entries, sorted by block_begin (entry k owns logical blocks
 *              [block_begin_k, block_begin_k + fmgan_weight_refresh_blocks(entry k)) ); total_blocks = their sum.
 *   kind 0: dst[k] = src[k] * scale, k < n
 *   kind 1: dst = wt[i][tap][o] = scale * src[o][i][tap] (layout kind 0 of fmgan_modconv_weight_prep_f32), and, if
 *           dst2 != NULL, dst2 = wsq[o][i] = sum_tap src[o][i][tap]^2 (fmgan_modconv_wsq_f32); ktaps <= 9.  If
 *           dst3 != NULL (ktaps == 9 only), dst3 = U [16, cout, cin], the Winograd weight fmgan_wino_weight_f32 makes of wt.
 * Bit-identical to the separate kernels (same operations in the same order).
 */
typedef struct fmgan_refresh_entry {
  const void *src;
  void *dst;
  void *dst2;
  void *dst3;
  long long n;            /* kind 0: element count */
  int kind, cout, cin, ktaps;
  float scale;
  unsigned block_begin;
} fmgan_refresh_entry;
int fmgan_refresh_entry_bytes(void);      /* sizeof(fmgan_refresh_entry), for bindings that build the table by hand */
long long fmgan_weight_refresh_blocks(int kind, int cout, int cin, int ktaps, long long n);
int fmgan_weight_refresh_f32(const fmgan_refresh_entry *table_dev, int n_entries, long long total_blocks,
                             void *stream);

/*
 * Style bank: the style vector of EVERY modulated layer of a synthesis network in one launch, and the demodulation
 * coefficients of every demodulated 3x3 layer in a second one (replaces, when all latent columns are known before the
 * network starts, one fmgan_equal_linear_f32 + one fmgan_modconv_demod_wsq_f32 + one elementwise W * W+[:, col] per
 * layer).  table_dev: DEVICE array of n_entries (<= 65535) entries, one per layer:
 *   ws [cin, style_dim] = modulation weight * scale, bs [cin] = bias * lr_mul (or NULL), wsq [cout, cin] = sum_tap W^2
 *   (or NULL: no demodulation) — the fmgan_weight_refresh_f32 buffers of the layer;
 *   col: latent column; sliced != 0: the column is co-modulated; n_styles: columns per sample of `wplus`;
 *   style_off / demod_off: PER-SAMPLE float offsets of the layer's block in the flat outputs (prefix sums of cin / cout).
 * fmgan_style_bank_f32:  styles_out[batch*style_off + t*cin + n] = sum_k ws[n,k] * x[t,k] + bs[n],
 *   x[t,k] = w[t,k], or fl(w[t,k] * wplus[p,col,k]) where sliced; w [batch, style_dim], wplus [wplus_batch, n_styles,
 *   style_dim], wplus_batch = 1 (one photo shared by the batch: p = 0) or batch (p = t).
 * fmgan_demod_bank_f32:  demod_out[batch*demod_off + t*cout + o] = 1/sqrt(scale^2 * sum_i wsq[o,i] * s[t,i]^2 + eps) for
 *   every entry with demodulate != 0 and wsq != NULL, s = that entry's block of `styles`.
 * fmgan_style_bank_concat_f32 (the concatenating co-modulation of the 2-encoder scheme): every entry's ws is
 *   [cin, dv + dw] and x[t,k] = v[t,k] for k < dv, wplus[p,col,k-dv] for k >= dv; v [batch, dv], wplus [wplus_batch,
 *   n_styles, dw]; `sliced` is not read (every column is concatenated), dv and dw are any positive ints.  ONE fma chain
 *   over the concatenated index: the bits of fmgan_equal_linear_f32 on the materialised concatenation.  An entry whose
 *   col is outside [0, n_styles) is skipped.  Its demodulation coefficients come from fmgan_demod_bank_f32.
 * Same fma chains, butterfly and rounding as the per-layer entry points (one shared definition): bit-identical.
 * No atomics, one writer per element.  EINVAL for NULL pointers, n_entries outside [1, 65535], non-positive dims or
 * wplus_batch not in {1, batch}; batch == 0 is a no-op (both checked before any HIP call).
 */
typedef struct fmgan_style_bank_entry {
  const void *ws;
  const void *bs;
  const void *wsq;
  long long style_off, demod_off;
  int col, sliced, n_styles, cin, cout, demodulate;
  float scale, eps;
} fmgan_style_bank_entry;
int fmgan_style_bank_entry_bytes(void);   /* sizeof(fmgan_style_bank_entry), for bindings that build the table by hand */
int fmgan_style_bank_f32(const fmgan_style_bank_entry *table_dev, int n_entries, const float *w, const float *wplus,
                         int wplus_batch, int batch, int style_dim, float *styles_out, void *stream);
int fmgan_style_bank_concat_f32(const fmgan_style_bank_entry *table_dev, int n_entries, const float *v,
                                const float *wplus, int wplus_batch, int batch, int dv, int dw, float *styles_out,
                                void *stream);
int fmgan_demod_bank_f32(const fmgan_style_bank_entry *table_dev, int n_entries, const float *styles, int batch,
                         float *demod_out, void *stream);

/*
 * Modulated 3x3 convolution, input-modulated form with batch-shared weights
 * (algebraically equal to the reference's per-sample weight-modulated grouped conv,
 * stylegan2.py:258-293):
 *   mode 0 (plain, stylegan2.py:289-293): out[b,o,y,x] = demod[b,o] * sum_{i,ky,kx}
 *             wt[i,ky*3+kx,o] * style[b,i] * in[b,i,y+ky-1,x+kx-1]                 out [b,o,h,w]
 *   mode 1 (transposed, stride 2, pad 0; stylegan2.py:268-277):                    out [b,o,2h+1,2w+1]
 *             out[b,o,Y,X] = demod[b,o] * sum_{i, 2y+ky=Y, 2x+kx=X} wt[i,ky*3+kx,o]*style[b,i]*in[b,i,y,x]
 *   mode 2 (stride 2, pad 0; the downsample branch stylegan2.py:281-286 after its blur, and the data-gradient of
 *             mode 1):  out[b,o,y,x] = demod[b,o] * sum_{i,ky,kx} wt[i,ky*3+kx,o]*style[b,i]*in[b,i,2y+ky,2x+kx]
 *                                                                                    out [b,o,(h-3)/2+1,(w-3)/2+1]
 *   in [batch,cin,h,w], wt from fmgan_modconv_weight_prep_f32 (ktaps = 9), style [batch,cin],
 *   demod [batch,cout] or NULL (no demodulation); out pre-allocated; all f32 contiguous.
 * Optional fused StyledConv epilogue (mode 0 only; stylegan2.py:371-373), enabled by fuse_act != 0:
 *   out = lrelu( (conv + noise_weight[0]*noise[b or 0,y,x]) + bias[o] ) * act_scale
 *   noise [noise_batch (1 or batch), h*w] or NULL, noise_weight device scalar or NULL, bias [cout] or NULL.
 * The contraction runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).
 * out_plane_stride / out_row_stride (elements; 0 = contiguous): element (b,o,y,x) is written to
 *   out[(b*cout+o)*out_plane_stride + y*out_row_stride + x] — see fmgan_upfirdn2d_strided.
 * workspace: tiny layers (4x4..32x32 at small batch) have too few output tiles to fill 256 CUs, so the
 *   input-channel loop is split over blocks (split-K) and the partial sums are combined by a finish kernel.
 *   Pass a device buffer of at least fmgan_modconv2d_workspace_bytes() bytes (0 = no split for this shape);
 *   with workspace == NULL the call still works, unsplit.  Results do not depend on timing or placement
 *   (no atomics: each partial slab is written once and summed in a fixed order).
 */
long long fmgan_modconv2d_workspace_bytes(int batch, int cin, int cout, int h, int w, int mode);
int fmgan_modconv2d_f32(const float *in, const float *wt, const float *style,
                        const float *demod, float *out,
                        int batch, int cin, int cout, int h, int w, int mode,
                        const float *noise, const float *noise_weight, const float *bias,
                        int noise_batch, int fuse_act, float alpha, float act_scale,
                        long long out_plane_stride, int out_row_stride,
                        void *workspace, long long workspace_bytes, void *stream);

/*
 * Reduced-precision form of fmgan_modconv2d_f32 for BASELINE config 5's bf16 leg (NOT the parity path; the reference has
 * no such path: its ModulatedConv2d is F.conv2d in the tensors' dtype, stylegan2.py:250-298, and its op kernels
 * dispatch float / double / half only, op/upfirdn2d_kernel.cu:311): the same operator with both MFMA operands rounded to
 * bf16 (RNE) — the scaled weight, and the modulated activation style[b,i]*in[b,i,..] on its way into LDS — and fp32
 * accumulation on v_mfma_f32_32x32x16_bf16; fp32 tensors in HBM on both sides, same arguments and epilogue.
 *   fmgan_modconv_weight_bf16_bytes / fmgan_modconv_weight_to_bf16: convert the fp32 MFMA layout wt[cin][taps][cout]
 *       (fmgan_modconv_weight_prep_f32, any kind; cin / cout = the CONV's input / output channels) into the bf16 operand
 *       image [cin/16][tap][2][cout padded to 32][8].
 *   fmgan_modconv2d_bf16_supported: 1 when the shape is served (cin % 16 == 0, cout % 32 == 0, position grid >= 32 wide
 *       and >= 4 high, 32-bit buffer ranges); otherwise fmgan_modconv2d_bf16 returns FMGAN_EUNSUPPORTED and the caller
 *       keeps the fp32 kernel.  mode 1 runs over the (h+1) x (w+1) quad grid; the quads m = h / n = w own only the last
 *       output row / column.
 */
long long fmgan_modconv_weight_bf16_bytes(int cin, int cout, int ktaps);
int fmgan_modconv_weight_to_bf16(const float *wt, void *wt_bf16, int cin, int cout, int ktaps, void *stream);
int fmgan_modconv2d_bf16_supported(int batch, int cin, int cout, int h, int w, int mode);
int fmgan_modconv2d_bf16(const float *in, const void *wt_bf16, const float *style, const float *demod, float *out,
                         int batch, int cin, int cout, int h, int w, int mode,
                         const float *noise, const float *noise_weight, const float *bias,
                         int noise_batch, int fuse_act, float alpha, float act_scale,
                         long long out_plane_stride, int out_row_stride, void *stream);

/*
 * fp32 contraction on the bf16 matrix pipe by operand splitting ("bf16x3"; forward modes 0 and 1; a LABELLED path, not
 * the parity path): each fp32 operand is split exactly into three bf16 pieces (hi + mid + lo) and the product is
 * accumulated in fp32 from the six largest piece products (ah*bh + ah*bm + am*bh + am*bm + ah*bl + al*bh; the dropped
 * terms are O(2^-24) of the product, one fp32 rounding), on v_mfma_f32_32x32x16_bf16 — 16/6 = 2.7x the matrix-pipe rate of
 * v_mfma_f32_32x32x2_f32 at fp32 accuracy.  Same arguments and epilogue as fmgan_modconv2d_f32; wt_split from
 * fmgan_modconv_weight_to_bf16x3 (the fp32 MFMA layout split into three bf16 operand images).
 */
long long fmgan_modconv_weight_bf16x3_bytes(int cin, int cout, int ktaps);
int fmgan_modconv_weight_to_bf16x3(const float *wt, void *wt_split, int cin, int cout, int ktaps, void *stream);
int fmgan_modconv2d_bf16x3_supported(int batch, int cin, int cout, int h, int w, int mode);
int fmgan_modconv2d_bf16x3(const float *in, const void *wt_split, const float *style, const float *demod, float *out,
                           int batch, int cin, int cout, int h, int w, int mode,
                           const float *noise, const float *noise_weight, const float *bias,
                           int noise_batch, int fuse_act, float alpha, float act_scale,
                           long long out_plane_stride, int out_row_stride, void *stream);

/*
 * The first convolution of a pSp style head (psp_encoders.py GradualStyleBlock) on the same split-operand contraction
 * (csrc/conv3x3_x3.hip; the modulated entries above are csrc/modconv_bf16.hip):
 *     out[b,o,y,x] = lrelu(bias[o] + sum_{i,ky,kx} W[o,i,ky,kx] * in[b,i,2y+ky-1,2x+kx-1]),  lrelu(v) = v > 0 ? v : alpha*v
 * a plain 3x3 convolution with stride 2 and zero padding 1, NCHW fp32 in and out ([batch,cout,(h-1)/2+1,(w-1)/2+1]), no
 * style and no demodulation; bias may be NULL.  out_nhwc = 1 writes the same values as out[b][y][x][o] (channels_last
 * storage, what MIOpen's NHWC kernels read; out 16-byte aligned when cout % 4 == 0), 0 as out[b][o][y][x].  wt_split = fmgan_modconv_weight_to_bf16x3 of W in [cin][9][cout] order.
 * Fixed summation order (no split-K, no atomics): two calls give the same bits.  A finite operand never yields an
 * infinite piece; a block that finds Inf or NaN among its operands recomputes its tile as fp32 products, so non-finite
 * values propagate as they do in an fp32 convolution.  Any cin, cout, h, w >= 1 within 32-bit buffer ranges:
 * fmgan_conv3x3s2_bf16x3_supported answers from the launch's plan, and the launch returns FMGAN_EUNSUPPORTED (and
 * launches nothing) where it says 0.
 */
int fmgan_conv3x3s2_bf16x3_supported(int batch, int cin, int cout, int h, int w);
int fmgan_conv3x3s2_bf16x3_f32(const float *in, const void *wt_split, const float *bias, float *out,
                               int batch, int cin, int cout, int h, int w, float alpha, int out_nhwc, void *stream);

/*
 * The same kernel as a family (csrc/conv3x3_x3.hip; the pSp encoder body's 3x3 convolutions, helpers.py _fused_unit): a plain 3x3 convolution
 * with zero padding 1 and
 *   stride   1 or 2 (out [batch,cout,(h-1)/stride+1,(w-1)/stride+1]); anything else is FMGAN_EINVAL;
 *   in_nhwc  0: in[b][i][y][x]; 1: in[b][y][x][i] (channels_last storage, 16-byte aligned; needs cin % 4 == 0 — other
 *            widths are declined: the query says 0 and the launch returns FMGAN_EUNSUPPORTED);
 *   out_nhwc as above;
 *   epilogue 0: out = conv;  1: out = lrelu(conv + aux[o]) with lrelu(v) = v > 0 ? v : alpha*v (aux = bias, may be NULL);
 *            2: out = conv > 0 ? conv : aux[o]*conv (aux = the per-channel PReLU slope, required; aten's prelu
 *            arithmetic, no bias).  alpha is read by epilogue 1 only.
 * fmgan_conv3x3s2_bf16x3_f32 is (stride 2, in_nhwc 0, epilogue 1) of it; same summation order in every member, so the
 * channels_last-input result has the bits of the NCHW-input one.  wt_split, special values and refusals as above.
 */
int fmgan_conv3x3_bf16x3_supported(int batch, int cin, int cout, int h, int w, int stride, int in_nhwc);
int fmgan_conv3x3_bf16x3_f32(const float *in, const void *wt_split, const float *aux, float *out,
                             int batch, int cin, int cout, int h, int w, int stride, int in_nhwc, int out_nhwc,
                             int epilogue, float alpha, void *stream);

/*
 * The narrow-tile members of the family (csrc/conv3x3_x3.hip conv3x3_tail_x3; the pSp style heads' convolutions whose
 * output is 5 .. 16 wide): stride 2, in[b][y][x][i] (channels_last storage, 16-byte aligned, cin % 4 == 0), epilogue
 * lrelu(conv + bias[o]) (bias may be NULL), out_nhwc as above.  An MFMA's 32 position lanes are 2 output rows of 16
 * columns (outputs 9 .. 16 wide) or 4 rows of 8 (5 .. 8 wide) instead of one row of 32; contraction, summation order,
 * wt_split and special values are those of fmgan_conv3x3_bf16x3_f32, whose bits the result has on finite operands.
 * fmgan_conv3x3_tail_bf16x3_select is the launch's plan without the launch: 16 or 8, the tile width that serves the
 * shape, or the status the launch would return — FMGAN_EINVAL for a non-positive size, FMGAN_EUNSUPPORTED for an
 * output wider than 16 (fmgan_conv3x3_bf16x3_f32 serves those) or at most 4 wide, cin % 4 != 0 and sizes past the
 * 32-bit buffer ranges.  A declined launch launches nothing.
 */
int fmgan_conv3x3_tail_bf16x3_select(int batch, int cin, int cout, int h, int w);
int fmgan_conv3x3_tail_bf16x3_f32(const float *in, const void *wt_split, const float *bias, float *out,
                                  int batch, int cin, int cout, int h, int w, float alpha, int out_nhwc, void *stream);

/*
 * Plain (mode 0) modulated conv with the FOLLOWING ToRGB layer folded into its epilogue.  In the reference these are
 * two modules and three HBM passes over the activation (StyledConv conv2 -> ToRGB, stylegan2.py:646-651 calling
 * :360-376 and :393-404).  When one block holds every output channel of its pixels (cout <= the tile's channel
 * extent and every tile lies in one sample: fmgan_modconv2d_rgb_fusable() == 1; the launch runs without split-K), the 1x1 modulated conv to <= 3 channels is a reduction
 * over the accumulator rows:
 *   act[b,o,p]  = lrelu(demod*conv + noise_weight*noise + bias) * act_scale          (as fmgan_modconv2d_f32)
 *   rgb[b,c,p]  = sum_o act[b,o,p] * wmod[b,c,o] + rgb_bias[c] + rgb_skip[b,c,p]
 *   wmod[b,c,o] = rgb_scale * rgb_weight[c,o] * rgb_style[b,o]   ([batch, 3, cout], rows >= rgb_channels zero) is
 *   built once per forward by fmgan_torgb_weight_mod_f32 from the [1,3,cout,1,1] ToRGB parameter and its style;
 *   rgb_bias [rgb_channels] or NULL, rgb_skip [batch, rgb_channels, h, w] (the already upsampled skip) or NULL,
 *   rgb_out like rgb_skip.
 * out may be NULL: the activation is then never written (last layer of the synthesis network — ToRGB is its only
 * consumer).  Summation order over o is fixed (rows of a lane, lane halves, then waves): run-to-run bit-identical.
 * Returns FMGAN_EUNSUPPORTED when the shape is not fusable; the caller then runs fmgan_modconv2d_f32 + fmgan_torgb_f32.
 */
int fmgan_torgb_weight_mod_f32(const float *rgb_weight, const float *rgb_style, float *wmod,
                               int batch, int cout, int rgb_channels, float rgb_scale, void *stream);
int fmgan_modconv2d_rgb_fusable(int batch, int cin, int cout, int h, int w);
int fmgan_modconv2d_rgb_f32(const float *in, const float *wt, const float *style,
                            const float *demod, float *out,
                            int batch, int cin, int cout, int h, int w,
                            const float *noise, const float *noise_weight, const float *bias,
                            int noise_batch, int fuse_act, float alpha, float act_scale,
                            const float *rgb_wmod, const float *rgb_bias,
                            const float *rgb_skip, float *rgb_out, int rgb_channels, void *stream);

/*
 * Which tile, which split (pure host logic, no HIP call — as fmgan_upfirdn2d_select): the plan of fmgan_modconv2d_f32
 * (rgb == 0) or fmgan_modconv2d_rgb_f32 (rgb != 0; mode must be 0) for these arguments, made by the launch's own planning
 * code with the launch left out.  has_workspace: the caller passes the fmgan_modconv2d_workspace_bytes() buffer (without
 * it the launch runs unsplit).  The plan is that of a 16-byte-aligned input, whose halo patch is the wider one: a misaligned
 * input takes the same tile, or the LDS-DMA tile where the aligned one's LDS image was too large and 'A' is reported.
 *   *cfg     output-channel class of the shape: 0 = 128, 1 = 64, 2 = 32 channels per block
 *   *variant the tile's letter in its (mode, cfg) row of the tile table: 'A' = register prefetch, 'B'..'E' = LDS-DMA
 *            (after the fall-back to 'A' when the LDS-DMA tile declines the shape)
 *   *bm, *bn output channels x positions of the launched block;  *ksplit blocks along the input channels (1 = no split)
 * Any of the five may be NULL.  Returns the status the launch returns before it launches (FMGAN_OK: it would launch);
 * on an error, and for batch == 0, *cfg is -1 and the others 0.
 * fmgan_modconv2d_tiles: the tiles of this build, six ints each (mode, cfg, variant, BM, BN, fuses_rgb: takes launches
 * of fmgan_modconv2d_rgb_f32); writes the first `cap` tiles to out (may be NULL) and returns the number of tiles.
 */
int fmgan_modconv2d_select(int batch, int cin, int cout, int h, int w, int mode, int rgb, int has_workspace,
                           int *cfg, int *variant, int *bm, int *bn, int *ksplit);
int fmgan_modconv2d_tiles(int *out, int cap);

/*
 * Weight gradient of the plain (mode 0) modulated conv on the MFMA units:
 *   gw[o,i,ky,kx] = scale * sum_{b,y,x} (demod[b,o] * go[b,o,y,x]) * (style[b,i] * x[b,i,y+ky-1,x+kx-1])
 * (the conv part of d loss / d weight; the demodulation chain-rule term is [B,Cout]x[Cout,Cin] algebra on the host).
 *   go [batch,cout,h,w], demod [batch,cout] or NULL, x [batch,cin,h,w], style [batch,cin], gw [cout,cin,3,3].
 *   workspace: fmgan_modconv_wgrad_workspace_bytes() bytes (partial slabs of the split over pixels; fixed-order
 *   finish, bit-reproducible).  w < 16 returns FMGAN_EUNSUPPORTED (0 workspace bytes): tiny layers stay on MIOpen.
 */
long long fmgan_modconv_wgrad_workspace_bytes(int batch, int cin, int cout, int h, int w);
/*
 * The same for every mode of fmgan_modconv2d_f32 (h, w = the conv INPUT's size; go has that mode's output size):
 *   mode 1 (transposed, go [batch,cout,2h+1,2w+1]):  gw[o,i,ky,kx] = scale * sum (demod*go)[b,o,2y+ky,2x+kx] * (style*x)[b,i,y,x]
 *   mode 2 (stride 2,   go [batch,cout,(h-3)/2+1,(w-3)/2+1]):  ... sum (demod*go)[b,o,y,x] * (style*x)[b,i,2y+ky,2x+kx]
 * 64 x 64 output tiles whose four waves walk the same 2 x TW pixels per step; an MFMA's pixel pair comes from the two
 * rows, so consecutive K-steps move one pixel along x and the 3 x 3 window of the shifted operand slides (SP new
 * LDS reads per tap row and step).  Served: >= 48 channels on both sides and >= 16 pixels per row of the unshifted
 * operand (mode 0 also the 32 x 32-tile kernel for narrower layers); otherwise FMGAN_EUNSUPPORTED / 0 bytes.
 */
long long fmgan_modconv_wgrad_mode_workspace_bytes(int batch, int cin, int cout, int h, int w, int mode);
int fmgan_modconv_wgrad_mode_f32(const float *go, const float *demod, const float *x, const float *style,
                                 float *gw, int batch, int cin, int cout, int h, int w, int mode, float scale,
                                 void *workspace, long long workspace_bytes, void *stream);
int fmgan_modconv_wgrad_f32(const float *go, const float *demod, const float *x, const float *style,
                            float *gw, int batch, int cin, int cout, int h, int w, float scale,
                            void *workspace, long long workspace_bytes, void *stream);
/*
 * Which kernel, which tile, which split (pure host logic, no launch — as fmgan_modconv2d_select): the plan of
 * fmgan_modconv_wgrad_mode_f32 for these arguments, made by the one plan function that the launch and
 * fmgan_modconv_wgrad_mode_workspace_bytes call too.  aligned16: the unshifted operand (go; x in mode 1) starts on a
 * 16-byte boundary.
 *   *family  0 = declined (FMGAN_EUNSUPPORTED is returned), 32 = the 32 x 32-tile kernel, 64 = a 64 x 64-tile kernel
 *   *tw, *sp pixels per tile row (16 / 32) and the stride of the shifted operand (1; 2 in modes 1 and 2): the 64 x 64
 *            kernel launched is modconv_wgrad64_f32<log2 tw, sp>
 *   *ntiles  pixel tiles over the batch;  *tiles_per_split of them per block, in *ksplit splits (the last one may be
 *            shorter); the workspace is ksplit * 9 * cout * cin floats
 *   *vec     1 when the 64 x 64 kernel stages its operands with 16-byte loads (row length of the unshifted operand a
 *            multiple of 4 and aligned16), 0 for its guarded scalar fill and for the 32 x 32 kernel, which has one path
 * Any of the seven may be NULL.  Returns the status the launch returns before it launches (its pointer and workspace
 * checks left out); on any status but FMGAN_OK all seven are 0.
 */
int fmgan_modconv_wgrad_select(int batch, int cin, int cout, int h, int w, int mode, int aligned16, int *family,
                               int *tw, int *sp, int *ksplit, int *tiles_per_split, int *ntiles, int *vec);

/*
 * ToRGB (stylegan2.py:389-404): 1x1 modulated conv without demodulation + bias + optional skip:
 *   out[b,c,p] = sum_i scale*weight[c,i]*style[b,i]*in[b,i,p] + bias[c] (+ skip[b,c,p])
 *   in [batch,cin,hw], weight [cout,cin], style [batch,cin], bias [cout] or NULL,
 *   skip [batch,cout,hw] or NULL (already upsampled), out [batch,cout,hw]; cout <= 4.
 */
int fmgan_torgb_f32(const float *in, const float *weight, const float *style,
                    const float *bias, const float *skip, float *out,
                    int batch, int cin, int cout, int hw, float scale, void *stream);

/*
 * Backward of ToRGB's modulated 1x1 conv in one pass over its input (the reference: autograd of a grouped F.conv2d,
 * stylegan2.py:268-286 called from :389-404):
 *   grad_x[b,i,p] = sum_c scale*weight[c,i]*style[b,i] * grad_out[b,c,p]
 *   m_partial[s,b,c,i] = sum over the pixels of split s of grad_out[b,c,p] * x[b,i,p]
 * x / grad_x [batch,cin,hw], grad_out [batch,cout,hw], weight [cout,cin], style [batch,cin], cout <= 4;
 * m_partial [fmgan_torgb_backward_splits(batch,cin,hw), batch, cout, cin].  The caller sums m_partial over s (fixed order:
 * bit-reproducible) to M[b,c,i] and forms grad_weight[c,i] = scale * sum_b style[b,i]*M[b,c,i],
 * grad_style[b,i] = scale * sum_c weight[c,i]*M[b,c,i]; grad_bias and grad_skip are sums / copies of grad_out.
 * hw % 4 == 0 and 16-byte aligned pointers, else FMGAN_EUNSUPPORTED (splits() returns 0): the caller differentiates the
 * composite instead.
 */
int fmgan_torgb_backward_splits(int batch, int cin, int hw);
int fmgan_torgb_backward_f32(const float *x, const float *grad_out, const float *weight, const float *style,
                             float *grad_x, float *m_partial, int batch, int cin, int cout, int hw, float scale,
                             void *stream);

/*
 * The steps either side of the path, 3-channel images:
 *   fmgan_images_to_tensor: in uint8 [batch,h,w,3] -> out f32 [batch,3,h,w] = ((in/255) - mean) / std
 *       == transforms.ToTensor() + Normalize(mean, std) (train_3_encoder.py:233-239; Resize: fmgan_resize_* below)
 *   fmgan_tensor_to_images: in f32 [batch,3,h,w] -> out uint8 [batch,h,w,3] = (uint8)((clip(in,-1,1) + cent) * factor)
 *       == tensor2im (Evaluation/visual_eval.py:24-38), for every image of the batch.
 *   fmgan_tiles_to_canvas: the same conversion into square slots of uint8 canvases, one launch for n tiles:
 *       in f32 [n,3,src,src], canvas uint8 [n_canvas,canvas_h,canvas_w,3], slots int32 [n,3] ON THE DEVICE, one
 *       (canvas, y0, x0) per tile;  canvas[slots[i].canvas, y0+y, x0+x, c] = (uint8)(int)((clip(v,-1,1) + cent) * factor)
 *       with v = pixel (y,x) of tile i reduced from src to tile by f = src/tile in {1,2,4}: the pixel itself (f = 1: the
 *       bits of fmgan_tensor_to_images), else aten's bilinear rule at align_corners=False, the four centre taps of the
 *       f x f cell: 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d), columns first, no fused multiply-add.  Only the tiles'
 *       pixels are written; every other byte of the canvas keeps its value.  A tile whose slot does not lie wholly
 *       inside its canvas (or names no canvas) is skipped.  FMGAN_EINVAL: non-positive sizes, null pointers, src not
 *       tile, 2*tile or 4*tile; n == 0: FMGAN_OK; FMGAN_EOVERFLOW beyond the 32-bit pixel / grid indices.
 */
/*
 * transforms.Resize(size) of the same pipeline (train_3_encoder.py:233-239) = PIL.Image.resize(BILINEAR), whose
 * arithmetic is Pillow's ImagingResample (third-party, pinned pillow=8.2.0: src/libImaging/Resample.c): per-axis tap
 * windows of the triangle filter stretched by max(scale,1), weights in 22-bit fixed point, a horizontal then a
 * vertical integer pass with a uint8 rounding in between.  Bit-exact with Pillow.
 *   fmgan_resize_output_size : torchvision's Resize(int) rule (shorter edge -> size, longer int(size*long/short),
 *                              unchanged if the shorter edge already equals size).
 *   fmgan_resize_plan_ints / fmgan_resize_plan : HOST functions; fill a caller-owned host buffer with the coefficient
 *       tables for (in_h,in_w)->(out_h,out_w): header[8] = {ksize_x, ksize_y, in_h, in_w, out_h, out_w, max input
 *       rows per 8-row output tile, 8}, then bounds_x[2*out_w], coeff_x[out_w*ksize_x], bounds_y[2*out_h],
 *       coeff_y[out_h*ksize_y].  The caller copies it to the device once per size pair.
 *   fmgan_resize_bilinear_u8 : in uint8 [batch,in_h,in_w,3] -> out_u8 uint8 [batch,out_h,out_w,3] (what PIL returns)
 *       and/or out_f32 f32 [batch,3,out_h,out_w] = ((v/255) - mean) / std (Resize + ToTensor + Normalize in one pass);
 *       either output may be NULL.  `plan` is the DEVICE copy of the table for exactly these sizes.
 */
int fmgan_resize_output_size(int h, int w, int size, int *out_h, int *out_w);
long long fmgan_resize_plan_ints(int in_h, int in_w, int out_h, int out_w);
int fmgan_resize_plan(int in_h, int in_w, int out_h, int out_w, int *plan, long long plan_ints);
int fmgan_resize_bilinear_u8(const unsigned char *in, const int *plan, unsigned char *out_u8, float *out_f32,
                             int batch, int in_h, int in_w, int out_h, int out_w,
                             float mean, float stdv, void *stream);

int fmgan_images_to_tensor(const unsigned char *in, float *out, int batch, int h, int w,
                           float mean, float stdv, void *stream);
int fmgan_tensor_to_images(const float *in, unsigned char *out, int batch, int h, int w,
                           float cent, float factor, void *stream);
int fmgan_tiles_to_canvas(const float *in, unsigned char *canvas, const int *slots, int n, int src, int tile,
                          int n_canvas, int canvas_h, int canvas_w, float cent, float factor, void *stream);

/*
 * Batches out of device-resident image banks (csrc/image_bank.hip), one launch:
 *   out[s] = ((bank[k_s][i_s] / 255) - mean) / stdv      uint8 [h,w,3] -> f32 [3,h,w], the bits of fmgan_images_to_tensor
 * Up to 4 banks uint8 [count_k,h,w,3] of one h x w (a bank with count 0 is absent).  out is f32
 * [n_groups*members,3,h,w]: n_groups (1..8) groups of `members` images.  `groups` is a HOST array of 5 ints per group,
 * {bank, source, swap, mul, add}, passed to the kernel by value; member j of the group reads
 *   b = j*stride;  pos = offset + (b ^ swap);  i = index[source][pos]*mul + add;  image i of bank `bank`
 * index_a / index_b: DEVICE int32 arrays of len_a / len_b entries (source 0 / 1; index_b may be NULL), the epoch's
 * index list and, where an item needs one, its drawn partners; offset: the batch's first position.  swap 0/1 pairs
 * position b with b ^ 1 (Swap_List_Pair), stride 1/2 keeps every member or the even ones.  A slot whose bank id,
 * position or image index is out of range is skipped, its source never read and its output left as it was.
 * Vector path (a lane owns pixels_per_lane = 4 or 16 consecutive pixels; 0 = the measured default): bank bases aligned
 * to 4 / 16 bytes, h*w % 4 / 16 == 0 and out 16-byte aligned; otherwise one pixel per lane.  All offsets are 64-bit.
 * members == 0: FMGAN_OK without a launch.  FMGAN_EINVAL: non-positive sizes, n_groups outside 1..8, stride not 1 or
 * 2, swap not 0 or 1, negative counts / lengths / offset, stdv == 0, pixels_per_lane not 0, 4 or 16, null groups / out
 * / index_a; FMGAN_EOVERFLOW beyond the 32-bit pixel / slot / grid indices.
 */
int fmgan_bank_gather(const void *bank0, const void *bank1, const void *bank2, const void *bank3,
                      int count0, int count1, int count2, int count3, int h, int w,
                      const void *index_a, long long len_a, const void *index_b, long long len_b,
                      long long offset, int members, int stride, const int *groups, int n_groups,
                      float *out, float mean, float stdv, int pixels_per_lane, void *stream);

/*
 * L-BFGS on flat float32 state, the direction computed in Gram space (csrc/lbfgs.hip; the fused path of
 * Evaluation/image_projection/LBFGS.py's FullBatchLBFGS.step).  The caller owns, on one device:
 *   g, g_prev, d, g_new   f32 [n]           gradient, previous gradient, direction, trial gradient
 *   S, Y                  f32 [m + 1, n]    ring of the steps s and the gradient differences y; the slot after the
 *                                           head is spare and receives the candidate pair
 *   G                     f64 [D, D]        D = 2 (m + 1) + 1: products of s slots, y slots and g, kept between steps
 *   state                 int32 [m + 2]     head slot, live pairs, then the live slots, oldest first
 *   record                f64 [8]           accepted, H_diag, ys, sBs, g.d, g_new.d, g.g, yy
 *   coef                  f64 [D]           the direction's coefficients in slot order
 *   partial               f64 [max(fmgan_lbfgs_pair_blocks(n) * (6 m + 7), 2048)]
 * `segs` is a HOST table of 3 long long per parameter tensor, {address of the f32 parameter, address of its f32 gradient
 * or 0 (read as zeros), numel}, nseg in 1..64, the numels adding up to n; it travels to the kernels by value.
 * Every sum is float64, added in a fixed order without atomics: bit-reproducible.
 *   fmgan_lbfgs_pair_f32      g = gradients; with has_pair also the candidate s = t d, y = g - g_prev into the spare slot;
 *                             partials of every product the Gram rows of s, y and g need, of ys, yy and s.g_prev
 *   fmgan_lbfgs_coeffs_f64    one block: finalises the partials, accepts the pair iff ys > eps * sBs with
 *                             sBs = -t (s.g_prev) (then: head advances, G gains the pair's rows, H_diag = ys / yy),
 *                             runs the two-loop recursion on coefficient vectors and writes coef and record[0..3, 6, 7]
 *   fmgan_lbfgs_direction_f32 d = sum coef * basis, g_prev = g, record[4] = g.d (measured from the vectors)
 *   fmgan_lbfgs_update_f32    param += a d through the table (one fused multiply-add per element)
 *   fmgan_lbfgs_gather_f32    g_new = gradients, record[5] = g_new.d
 * FMGAN_EINVAL: null pointers, n <= 0, nseg outside 1..64, numels that do not add up to n; FMGAN_EUNSUPPORTED: m
 * outside 1..32; FMGAN_EOVERFLOW: more tiles than a grid holds.
 */
long long fmgan_lbfgs_pair_blocks(long long n);
int fmgan_lbfgs_pair_f32(const long long *segs, int nseg, float *g, const float *g_prev, const float *d, float *S,
                         float *Y, const void *state, double *partial, long long n, int m, float t, int has_pair,
                         void *stream);
int fmgan_lbfgs_coeffs_f64(const double *partial, double *G, void *state, double *record, double *coef, long long n,
                           int m, float t, float eps, int has_pair, void *stream);
int fmgan_lbfgs_direction_f32(const double *coef, const void *state, const float *S, const float *Y, const float *g,
                              float *g_prev, float *d, double *partial, double *record, long long n, int m,
                              void *stream);
int fmgan_lbfgs_update_f32(const long long *segs, int nseg, const float *d, float a, long long n, void *stream);
int fmgan_lbfgs_gather_f32(const long long *segs, int nseg, float *g_new, const float *d, double *partial,
                           double *record, long long n, void *stream);

/*
 * The two launches train() adds per iteration (csrc/train_loop.hip).
 *
 * fmgan_ema_f32: dst <- decay * dst + alpha * src over a whole parameter set in ONE launch (replaces the two aten
 * launches per parameter of `accumulate`, train_3_encoder.py:195-200).  table_dev: DEVICE array of n_entries entries
 * sorted by block_begin; entry k owns the logical blocks [block_begin_k, block_begin_k + fmgan_ema_blocks(numel_k)),
 * total_blocks = their sum; an entry of 0 elements owns none.  A block handles 4096 consecutive elements of one tensor
 * with 16-byte accesses from the first 16-byte boundary of dst when src is aligned there too, scalar accesses before
 * it, after the last whole vector, and everywhere when the two alignments differ.  Every offset is 64-bit.  Per element
 * fmaf(alpha, src, dst * decay): two roundings, written explicitly; elementwise, hence bit-reproducible.  dst and src
 * ranges of different entries must not overlap.  n_entries == 0 or total_blocks == 0: FMGAN_OK without a launch.
 * FMGAN_EINVAL: negative counts, NULL table; FMGAN_EOVERFLOW: more blocks than a grid holds (2^31 - 1).
 *
 * fmgan_loss_row_f32: one row of the loss log.  `ptrs` is a HOST struct of 16 device addresses (each of one float, or
 * NULL); it is read during the call and travels to the kernel by value.  One wave: lane i < n writes *p[i] (0.0f for
 * NULL) to row_dev[i], lanes n..15 write 0.0f.  FMGAN_EINVAL: n outside 0..16, NULL ptrs or row_dev.
 */
typedef struct fmgan_ema_entry {
  void *dst;
  const void *src;
  long long numel;
  long long block_begin;
} fmgan_ema_entry;
typedef struct fmgan_loss_ptrs {
  const float *p[16];
} fmgan_loss_ptrs;
long long fmgan_ema_blocks(long long numel);
int fmgan_ema_f32(const fmgan_ema_entry *table_dev, int n_entries, long long total_blocks, float decay, float alpha,
                  void *stream);
int fmgan_loss_row_f32(const fmgan_loss_ptrs *ptrs, int n, float *row_dev, void *stream);

/*
 * 16-bit activations in HBM (csrc/act16.hip): bf16 (FMGAN_BF16) and f16 (FMGAN_F16) tensors read and written as they
 * are; every value is widened to fp32, the arithmetic is that of the fp32 entry point in the same order, and the result
 * is narrowed once (round to nearest even) at the store.  Any other dtype: FMGAN_EUNSUPPORTED.  Data pointers need
 * 2-byte alignment only: 16-byte accesses are used from the first 16-byte boundary of the output where the inputs are
 * aligned there too, 2-byte accesses elsewhere.
 *
 * fmgan_act16_fba: fmgan_fused_bias_act on 16-bit x / refer / out, for the codes 10, 11, 12, 30, 31, 32 (another
 * act*10+grad: FMGAN_EUNSUPPORTED).  bias is ALWAYS an fp32 array of size_b elements (NULL or size_b == 0: none).
 * Layouts: step_b > 1 — planes of step_b elements, one bias scalar per plane (size_x % step_b != 0: FMGAN_EINVAL);
 * step_b == 1 — the bias runs along the innermost dimension.  fmgan_act16_fba_select answers without a GPU: 1 planes
 * kernel, 2 bias-innermost kernel, 3 planes kernel over the whole tensor (no bias), else the status the launch returns
 * (the launch also returns FMGAN_EINVAL for a NULL or odd data pointer).
 *
 * fmgan_act16_fba_bwd: fmgan_fused_bias_act_bwd_f32 on 16-bit grad_out / ref_out / grad_in, any hw >= 1:
 *   grad_in[p,i] = narrow((ref_out[p,i] > 0 ? grad_out[p,i] : alpha * grad_out[p,i]) * scale)
 *   partial[p, blk] = fp32 sum of the block's share of the STORED grad_in[p, :] (widened back), fixed association
 * partial [planes, fmgan_act16_fba_bwd_blocks(planes, hw)] f32; the blocks query returns 0 for planes <= 0, hw <= 0 or
 * planes or hw > 0x7f000000 (the launch: FMGAN_EINVAL / FMGAN_EOVERFLOW; planes == 0 is FMGAN_OK without a launch).
 *
 * fmgan_ufd16: fmgan_upfirdn2d on 16-bit input / out with fp32 taps `kernel` [kernel_h, kernel_w] (un-flipped).
 * fmgan_ufd16_select answers without a GPU: 1 = the FIR kernel (up = down = 1, minor = 1, at most 4x4 taps, any pads:
 * 8 outputs per lane, taps accumulated with fmaf in tap order), 0 = one output per thread (everything else), else the
 * launch's status: FMGAN_EINVAL for non-positive sizes or an empty output, FMGAN_EOVERFLOW when a plane or major does
 * not fit 31 bits.
 */
int fmgan_act16_fba_select(int dtype, long long size_x, int size_b, int step_b, int act, int grad);
int fmgan_act16_fba(int dtype, const void *x, const float *bias, const void *refer, void *out,
                    long long size_x, int size_b, int step_b, int act, int grad, float alpha, float scale,
                    void *stream);
int fmgan_act16_fba_bwd_blocks(long long planes, int hw);
int fmgan_act16_fba_bwd(int dtype, const void *grad_out, const void *ref_out, void *grad_in, float *partial,
                        long long planes, int hw, float alpha, float scale, void *stream);
int fmgan_ufd16_select(int dtype, int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                       int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1);
int fmgan_ufd16(int dtype, const void *input, const float *kernel, void *out, int major, int in_h, int in_w,
                int minor, int kernel_h, int kernel_w, int up_x, int up_y, int down_x, int down_y,
                int pad_x0, int pad_x1, int pad_y0, int pad_y1, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FMGAN_HIP_H */
