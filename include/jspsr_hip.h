/* jspsr_hip.h -- C ABI of the MI355X (gfx950) JSPSR hot-path library, libjspsr_hip.so.
 *
 * Plain pointers and sizes only; every pointer is DEVICE memory unless stated otherwise.
 * Every launcher is asynchronous on `stream` (a hipStream_t passed as void*), allocates
 * nothing, keeps no pointer after return and is safe to call from any host thread
 * (the reference's backward runs on PyTorch's autograd thread -- SURVEY.md section 8b).
 * Return value: 0 on success, otherwise a negative JSPSR_E* code or a positive hipError_t;
 * jspsr_last_error() gives the text for the calling thread.
 *
 * The reference (xandercai/JSPSR) is pure Python and has no FFI of its own; the seam these
 * entry points replace is the operator call inside its nn.Modules (cited per function,
 * paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding.
 */
#ifndef JSPSR_HIP_H
#define JSPSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JSPSR_OK 0
#define JSPSR_EINVAL (-1)   /* bad shape / null pointer / unsupported combination */
#define JSPSR_EALIGN (-2)   /* pointer not aligned as documented */

typedef void* jspsr_stream_t; /* hipStream_t */

/* ABI version of this header (bumped on any signature change). */
int jspsr_abi_version(void);
/* Diagnostics: launches so far (this process) of the kernel family named `what` -- the names the error texts use:
 * "conv64_resident" (K2r), "conv128_resident" (K2q), "conv_patch", "conv_patch_16x16", "conv_igemm", "conv2d_wgrad_patch", "prop_forward (dma)",
 * "prop_backward (dma)", "prop_forward", "prop_head_forward", ...  Lets a parity test assert that a shape really took
 * the kernel it is meant to exercise.  -1 for a NULL name, 0 for a name never launched. */
long long jspsr_launch_count(const char* what);
/* The persistent register-resident conv kernels (K2r: "conv64_resident", K2q: "conv128_resident") hand their tiles out either
 * by a static stride walk (default alone on the GPU: neighbouring tiles share an XCD's L2) or from a global ticket in runs of
 * four (on = 1).  One workgroup of these kernels needs a WHOLE compute unit; where another kernel holds some CUs for long --
 * RCCL's all-reduce beside the backward pass of a data-parallel step -- the workgroups that start late would, with the static
 * walk, still do their full share after everybody else has finished; drawing from the ticket they find it empty and leave.
 * on = -1: back to the environment's default (JSPSR_CONV_DYNQ / JSPSR_CONV_DYNQ128).  Returns the previous setting.
 * jspsr_amd.ddp.GradReducer switches it on for world sizes > 1 -- a precaution (no multi-GPU box to measure it on; on one GPU
 * the two walks time the same inside the step).  (ABI v15) */
int jspsr_conv_dynamic_queue(int on);
/* Text of the last error raised on the calling thread ("" if none). */
const char* jspsr_last_error(void);

/* ---- K1: fused spatial propagation ------------------------------------------------------
 * Replaces PostProcessor.forward, models/components/spn.py:99-118, i.e. the sequence
 *   weight - mean_k(weight)                                   (spn.py:100-101)
 *   torchvision.ops.deform_conv2d(dem, offset, w, b, pad 1, mask=weight)   (spn.py:105-114)
 *   + scale * dem                                             (spn.py:116-117)
 * and the identical Post_process_deconv.forward, models/LRRU.py:267-298.
 *
 * dem    [B][H][W]      fp32   (B,1,H,W contiguous)
 * weight [B][9][H][W]   fp32   affinities after the sigmoid, tap k row-major over the 3x3 window
 * offset [B][OC][H][W]  fp32   OC = 18: channel 2k = dy_k, 2k+1 = dx_k (torchvision layout);
 *                              OC = 16: the 8 learned taps only (k = 0..3, 5..8), centre tap
 *                              implicitly (0,0) -- what Generator emits before spn.py:70-73
 * wk     [9], b0 [1]    fp32   PostProcessor.w / .b (device pointers: no host sync)
 * out    [B][H][W]      fp32
 * All pointers 4-byte aligned; 16-byte aligned pointers with W % 4 == 0 take the fast path.
 */
int jspsr_prop_forward_f32(const float* dem, const float* weight, const float* offset,
                           int offset_channels, const float* wk, const float* b0, float scale,
                           float* out, int B, int H, int W, jspsr_stream_t stream);

/* Bytes of scratch jspsr_prop_backward_f32 needs for a (B,H,W) problem. */
size_t jspsr_prop_backward_workspace_bytes(int B, int H, int W);

/* Backward of the above (the autograd of spn.py:99-118).
 * grad_out [B][H][W]; grad_weight [B][9][H][W]; grad_offset [B][OC][H][W];
 * grad_wk [9], grad_b0 [1] are overwritten (not accumulated).  grad wrt dem is not produced:
 * every caller detaches it (models/JSPSR.py:372, models/LRRU.py:453,467,481,496).
 * workspace: jspsr_prop_backward_workspace_bytes() bytes, 16-byte aligned.
 * Two launches: the streaming kernel (writes grad_weight / grad_offset and one row of 10 partial sums per
 * workgroup into the workspace) and a 10-workgroup fold of those rows into grad_wk / grad_b0.  With
 * grad_wk == grad_b0 == NULL only the first is launched; jspsr_prop_backward_fold_f32 is the second on its own, on the
 * same workspace (16-byte aligned there too: JSPSR_EALIGN before any launch).  Layout: a 16-byte header whose first
 * word is the number of rows the streaming kernel wrote, then the rows of 10 floats; the query covers every kernel form
 * of jspsr_prop_backward_f32 and jspsr_prop_logits_backward_f32 (0 for a non-positive size).
 */
int jspsr_prop_backward_f32(const float* grad_out, const float* dem, const float* weight,
                            const float* offset, int offset_channels, const float* wk,
                            float* grad_weight, float* grad_offset, float* grad_wk,
                            float* grad_b0, void* workspace, int B, int H, int W,
                            jspsr_stream_t stream);

int jspsr_prop_backward_fold_f32(const void* workspace, int B, int H, int W, float* grad_wk, float* grad_b0,
                                 jspsr_stream_t stream);

/* ---- K1s: one propagation step in its general form, for chains of steps ------------------------------------------
 * Replaces NLSPN._propagate_once, models/components/nlspn.py:177-187, called prop_time times on its own output
 * (nlspn.py:226-233) with affinities normalised once outside the loop (nlspn.py:158-173) -- and, with normalize != 0,
 * is the same operator as jspsr_prop_forward_f32 / jspsr_prop_backward_f32 plus the gradient they do not produce.
 *   normalize == 0:  out = b0 + sum_k wk[k] weight_k S_k + scale * dem      (affinities taken as they are)
 *   normalize != 0:  out = b0 + sum_k wk[k] (weight_k - mean_k weight) S_k + scale * dem      (spn.py:99-118)
 * Operand layout as for jspsr_prop_forward_f32.  out must not alias dem.
 * Backward: grad_weight / grad_offset are overwritten, or ADDED to when accumulate != 0 (the affinities and offsets
 * of an N-step chain are shared by all steps: their gradients sum over the steps).  grad_dem (may be NULL): the
 * gradient with respect to dem is ADDED into it (bilinear scatter + scale * grad_out; the caller zero-fills it or
 * lets it carry another contribution); a tap beyond tile + halo (possible from |offset| >= 7 px on) is added with a float
 * atomic, so its last bits depend on the execution order only where such taps exist.
 * grad_wk / grad_b0: both NULL (partial rows stay in the workspace) or both valid (overwritten).
 * workspace: jspsr_prop_step_backward_workspace_bytes() bytes, 16-byte aligned. */
int jspsr_prop_step_forward_f32(const float* dem, const float* weight, const float* offset, int offset_channels,
                                const float* wk, const float* b0, float scale, int normalize, float* out,
                                int B, int H, int W, jspsr_stream_t stream);
size_t jspsr_prop_step_backward_workspace_bytes(int B, int H, int W);
int jspsr_prop_step_backward_f32(const float* grad_out, const float* dem, const float* weight, const float* offset,
                                 int offset_channels, const float* wk, float scale, int normalize, int accumulate,
                                 float* grad_weight, float* grad_offset, float* grad_dem, float* grad_wk,
                                 float* grad_b0, void* workspace, int B, int H, int W, jspsr_stream_t stream);

/* ---- K1h: the same propagation step fed straight from the generator head's NHWC output ----------------------
 * Inside the models the two 1x1 heads of Generator.forward (models/components/spn.py:41-52,66-68; LRRU.py:238-247) run
 * as ONE 32-channel convolution; these entry points read its output where it lies and fold in what the reference does
 * between the heads and deform_conv2d: the Sigmoid of conv_weight (spn.py:43), the zero centre offset (spn.py:69-73),
 * the mean subtraction (spn.py:100-101) and the residual (spn.py:116-117).  The public planar entries above stay the
 * boundary of PostProcessor.forward.
 *
 * head [B][H][W][32], dtype JSPSR_F32 or JSPSR_BF16 (defined below), 16-byte aligned, channel c = 4 t + j:
 *   t = 0..7 the learned taps in window order without the centre (k = t < 4 ? t : t + 1),
 *   j = 0 affinity LOGIT of tap k (pre-sigmoid), j = 1 dy_k, j = 2 dx_k,
 *   j = 3: the centre tap's affinity logit for t == 0; ignored for t > 0.
 * dem, out [B][H][W] fp32; wk [9], b0 [1] as above.
 * Backward: grad_head in the same layout and dtype = d/d(head) (sigmoid derivative included; channels 4t+3, t > 0,
 * are written as zeros); grad_wk / grad_b0 overwritten, or both NULL to leave the per-workgroup partial rows in the
 * workspace (jspsr_prop_head_backward_workspace_bytes; the fold is the 10-workgroup launch jspsr_prop_backward_f32 also uses). */
int jspsr_prop_head_forward(int dtype, const float* dem, const void* head, const float* wk, const float* b0,
                            float scale, float* out, int B, int H, int W, jspsr_stream_t stream);
size_t jspsr_prop_head_backward_workspace_bytes(int B, int H, int W);
int jspsr_prop_head_backward(int dtype, const float* grad_out, const float* dem, const void* head, const float* wk,
                             void* grad_head, float* grad_wk, float* grad_b0, void* workspace, int B, int H, int W,
                             jspsr_stream_t stream);

/* ---- K8: the steps either side of the model call, on device rasters -----------------------------
 * jspsr_tiles_crop_f32: TileCrop's square cover, data/data_utils.py:87-194 -- x [C][H][W] -> out [n_x*n_x][C][k][k], tile
 *   (r, c) = rows stride*r .., columns stride*c .., row-major over the cover.
 * jspsr_tiles_merge_f32: merge_dem(method = copyto_add) with gen_weight_row / gen_weight_col, utils/utils.py:802-967 --
 *   tiles [n_x*n_x][k][k] predictions, each first losing border_px pixels per side, weighted by the linear ramps over the
 *   p = (k - 2 border_px) - stride pixels neighbours share (ramp [p] = linspace(1, 0, p + 2) without its ends, from the
 *   caller) and summed into out [S][S], S = stride (n_x - 1) + k - 2 border_px.  Every mosaic pixel gathers its <= 4 tiles
 *   in tile order: the same additions in the same order as the reference's tile-by-tile accumulation.
 * jspsr_mirror_pad_f32: add_padding, utils/utils.py:1501-1520, index for index -- x [C][H][W] -> out [C][H+2n][W+2n].
 * jspsr_elev_scale_f32: ToTensor.scale_data (descale = 0; data/data_utils.py:289-312: (z - base - min) / (max - min), or
 *   log(z - base - min) / log(max - min) + 1e-8) and ToDEM.descale_data (descale = 1; data_utils.py:441-457). */
int jspsr_tiles_crop_f32(const float* x, float* out, int C, int H, int W, int k, int stride, int n_x, jspsr_stream_t stream);
int jspsr_tiles_merge_f32(const float* tiles, const float* ramp, float* out, int n_x, int k, int border_px, int stride,
                          jspsr_stream_t stream);
int jspsr_mirror_pad_f32(const float* x, float* out, int C, int H, int W, int n, jspsr_stream_t stream);
int jspsr_elev_scale_f32(const float* in, float* out, long long n, int descale, int elev_log, double elev_min, double elev_max,
                         double base_elev, jspsr_stream_t stream);

/* ---- K9: the training batch on device, from a device-resident scene store ------------------------
 * jspsr_batch_make: every raster of a batch in one launch -- RandomCrop / TileCrop's window, RandomFlipRotate90's D4 map
 *   (data/data_utils.py:9-168) and ToTensor's per-kind arithmetic (data_utils.py:217-312) -- written as the fp32 NCHW
 *   tensors collate_fn stacks (data/dfc30.py:346-364), or as channel slices of one concatenated tensor (EDSR's input,
 *   utils/utils.py:248-315).  Kinds, indexed 0..5: lr_dem, hr_dem (fp32, 1 channel), image, mask (uint8, 1..16 channels),
 *   canopy (uint8, 1 channel), coord (2 channels, computed: row / (H - 1), col / (W - 1) over the whole scene).
 *   src[6], src_bytes[6], out[6], channels[6], coff[6], cpitch[6] are HOST arrays: kind i's scene store (HWC, all scenes
 *   back to back, 4-byte aligned; NULL for coord) and its size in bytes, its output (NULL: kind absent; 4-byte aligned) of
 *   (B, cpitch, k, k) whose channels coff .. coff + channels - 1 this kind writes.
 *   scenes  device int64 [n_scenes][3] = {pixel offset into every store, H, W}.
 *   samples device int32 [B][8] = {scene, y0, x0, code, base elevation (fp32 bit pattern), 0, 0, 0}: the crop is rows
 *     y0 .. y0 + k - 1, columns x0 .. x0 + k - 1; code = rot90 angle * 4 + flip_lr * 2 + flip_ud.  A row that leaves its
 *     scene or the store writes NaN.
 *   flags JSPSR_BATCH_*; elev_min / elev_max the DEM range (the Python numbers of tensor_kwargs); mask_div =
 *   len(mask_channel) + 1.  Image, mask, canopy and coord values are the reference's bits; DEM values within 1 ulp of
 *   numpy's fp32 log.  No host synchronisation. */
#define JSPSR_BATCH_LOG 1          /* tensor_kwargs log: log min-max scaling of the DEMs */
#define JSPSR_BATCH_SCALE_MASK 2   /* tensor_kwargs scale_mask: mask channel i times (i + 1) / mask_div */
#define JSPSR_BATCH_IMAGE_11 4     /* image_range "[-1, 1]" (image and lr_dem) */
#define JSPSR_BATCH_LABEL_11 8     /* label_range "[-1, 1]" (hr_dem) */
#define JSPSR_BATCH_IMAGE_255 16   /* image_range "[0, 255]" (image: a second division by 255) */
#define JSPSR_BATCH_FLAGS 31
int jspsr_batch_make(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                     const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples, int B,
                     int k, int flags, double elev_min, double elev_max, int mask_div, jspsr_stream_t stream);
/* K19, jspsr_batch_valid: the validity plane of the same batch.  store: one byte per pixel (nonzero = valid), all scenes
 *   back to back at the pixel offsets of `scenes`, 4-byte aligned, store_bytes of it (a device pointer, like out, scenes and
 *   samples).  out (B, 1, k, k) bytes, 1 = valid, made from the same sample rows through the same D4 map as
 *   jspsr_batch_make, so it lines up with every raster of the batch element for element.  A row that leaves its scene or
 *   the store writes 0 (where the float kinds write NaN).  One launch, no host synchronisation. */
int jspsr_batch_valid(const unsigned char* store, long long store_bytes, unsigned char* out, const long long* scenes,
                      int n_scenes, const int* samples, int B, int k, jspsr_stream_t stream);

/* ---- K1 in the models (round 4): logits + offsets as PLANES of one tensor ---------------------------------------
 * The same operator as jspsr_prop_forward_f32 / jspsr_prop_backward_f32 -- same kernels, same 108 / 208 algorithmic bytes
 * per pixel -- with what the reference does between the generator's heads and deform_conv2d folded in: the Sigmoid of
 * conv_weight (models/components/spn.py:43), the zero centre offset (spn.py:69-73), the mean subtraction
 * (spn.py:100-101), the residual (spn.py:116-117).
 *   head [B][25][H][W] fp32: planes 0..8 affinity LOGITS of tap k (row-major over the 3x3 window), planes 9..24 the sixteen
 *   learned offsets in Generator's order (dy, dx of taps 0..3, 5..8) -- what jspsr_head_forward writes.
 * Backward: grad_head in the same layout = d/d(head) (sigmoid derivative included); grad_wk / grad_b0 overwritten, or both
 * NULL to leave the partial rows in the workspace (jspsr_prop_backward_workspace_bytes; jspsr_prop_backward_fold_f32).
 * Any W and 4-byte aligned pointers; 16-byte aligned pointers with W % 4 == 0 take the persistent LDS-DMA kernel. */
int jspsr_prop_logits_forward_f32(const float* dem, const float* head, const float* wk, const float* b0, float scale,
                                  float* out, int B, int H, int W, jspsr_stream_t stream);
int jspsr_prop_logits_backward_f32(const float* grad_out, const float* dem, const float* head, const float* wk,
                                   float* grad_head, float* grad_wk, float* grad_b0, void* workspace, int B, int H, int W,
                                   jspsr_stream_t stream);

/* ---- K1c: the generator's two 1x1 heads as one convolution that writes planes -------------------------------------
 * Replaces conv_weight (without its Sigmoid) and conv_offset of Generator.forward, models/components/spn.py:41-52,66-68
 * (and BasicDepthEncoder's heads, models/LRRU.py:238-247), and their autograd.
 *   x      NHWC feature (B,H,W,Cin) of `dtype` (0 fp32 / 1 bf16, as JSPSR_F32 / JSPSR_BF16 below), channel pitch x_cstride,
 *          first channel x_coff >= 0 (elements; multiples of 4 fp32 / 8 bf16), 16-byte aligned
 *   w25    [25][Cin] fp32: rows 0..8 = conv_weight.0.weight, rows 9..24 = conv_offset.conv.0.weight;  b25 [25] the biases
 *   planes [B][25][H][W] fp32 = the `head` operand of jspsr_prop_logits_forward_f32
 * jspsr_head_ok(dtype, B, H, W, Cin) != 0: H * W a multiple of 32, Cin in {32, 64, 128}.
 * Backward, one pass over grad_planes [B][25][H][W]: grad_x (NHWC, `dtype`, pitch / offset as x; NULL = not wanted),
 * grad_nhwc32 [B][H][W][32] in `dtype` (channels 25..31 zero) = the G operand jspsr_conv2d_wgrad takes for the weight
 * gradient, grad_b25 [25] (overwritten).  workspace: jspsr_head_backward_workspace_bytes(), 16-byte aligned. */
int jspsr_head_ok(int dtype, int B, int H, int W, int Cin);
int jspsr_head_forward(int dtype, const void* x, int x_cstride, int x_coff, int Cin, const float* w25, const float* b25,
                       float* planes, int B, int H, int W, jspsr_stream_t stream);
size_t jspsr_head_backward_workspace_bytes(int B, int H, int W);
int jspsr_head_backward(int dtype, const float* grad_planes, const float* w25, int Cin, void* grad_x, int gx_cstride,
                        int gx_coff, void* grad_nhwc32, float* grad_b25, void* workspace, int B, int H, int W,
                        jspsr_stream_t stream);

/* ---- K1p: the plain output head (spn=False): nn.Conv2d(C, 1, 3, padding=1) writing the fp32 prediction -----------------
 * Replaces JSPSR's postprocessor = Basic2d(c0_channels, 1, 3, bn=False, relu=False) (models/JSPSR.py:195-204,378) and EDSR's
 * self.head (models/EDSR.py:108-111,132-136), and their autograd.  fp32 arithmetic (bf16 inputs widened exactly), fixed
 * summation order.
 *   x      NHWC (B,H,W,·) of `dtype` (JSPSR_F32 / JSPSR_BF16), channel pitch x_cstride, first channel x_coff (both multiples of
 *          4 fp32 / 8 bf16), 16-byte aligned; C a multiple of 8, at most 256 (JSPSR_EINVAL otherwise, before any launch)
 *   w      [C][3][3] fp32 (the nn.Conv2d weight as it is), bias [1] fp32;  y  (B,1,H,W) fp32
 * Zero padding at the image borders only; any H, W.
 * Backward, one pass over dy (B,1,H,W) fp32 and x: dx (NHWC, `dtype`, pitch / offset as x; NULL = not wanted), dw [C][3][3] and
 * db [1] fp32, overwritten.  The weight / bias gradient goes through per-workgroup partial rows in `workspace`
 * (jspsr_conv_head1_workspace_bytes(B, H, W, C) bytes, 16-byte aligned; 0 for an unsupported C) folded in a fixed order by
 * a second launch: the same bits from run to run.  Launch-count names "head1_forward", "head1_backward",
 * "head1_backward_fold". */
int jspsr_conv_head1_forward(int dtype, const void* x, int x_cstride, int x_coff, int C, const float* w, const float* bias,
                             float* y, int B, int H, int W, jspsr_stream_t stream);
size_t jspsr_conv_head1_workspace_bytes(int B, int H, int W, int C);
int jspsr_conv_head1_backward(int dtype, const float* dy, const void* x, int x_cstride, int x_coff, int C, const float* w,
                              void* dx, int dx_cstride, int dx_coff, float* dw, float* db, void* workspace, int B, int H,
                              int W, jspsr_stream_t stream);

/* ---- K2: convolutions on the matrix cores (implicit GEMM, NHWC) ---------------------------
 * Replace the reference's nn.Conv2d / nn.ConvTranspose2d calls and their autograd
 * (models/components/basics.py:6-20,39-47,69-77; every conv of models/JSPSR.py:66-180 and
 * models/components/spn.py:16-52).  Activations are NHWC; a tensor argument is described by
 * (pointer, C, channel pitch, channel offset) so a conv can read or write a channel slice of a
 * wider buffer (the reference's torch.cat fusion, basics.py:134, needs no copy).
 * dtype: JSPSR_F32 -> v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, fp32 storage);
 *        JSPSR_BF16 -> v_mfma_f32_32x32x16_bf16 (bf16 storage, fp32 accumulate).
 * Gathered channel counts / pitches / offsets must be multiples of 4 (fp32) or 8 (bf16).
 */
#define JSPSR_F32 0
#define JSPSR_BF16 1

/* Re-lay a master weight (O, I, KH, KW) fp32 (PyTorch Conv2d layout) for the kernels:
 *   mode 0: packed[o][ky][kx][i]  (i zero-padded to c_pad) -- forward of Conv2d(I->O)
 *   mode 1: packed[i][ky][kx][o]  (o zero-padded to c_pad) -- data gradient of Conv2d(I->O);
 *           also the forward of ConvTranspose2d whose weight is stored (I_T=O, O_T=I, KH, KW).
 */
int jspsr_pack_weight(int dtype, const float* w, void* packed, int O, int I, int KH, int KW,
                      int mode, int c_pad, jspsr_stream_t stream);

/* The same re-lay for MANY weights in one launch (after an optimizer step: 76 conv weights x 2 layouts for the
 * image+mask JSPSR instead of 152 launches).  `descs` is DEVICE memory, n descriptors sorted by `start`; descriptor i
 * is served by workgroups [start, start + ceil(total / jspsr_pack_chunk())) of the launch, total = rows * KH * KW *
 * c_pad elements; total_blocks = the sum of those block counts.  Each descriptor names its own output dtype. */
typedef struct jspsr_pack_desc {
  const float* w;     /* (O, I, KH, KW) fp32 master */
  void* out;          /* packed output */
  long long start;    /* first workgroup of this descriptor = sum of ceil(total / jspsr_pack_chunk()) over the preceding ones */
  long long total;    /* elements of this packed output */
  int O, I, KH, KW;
  int mode;           /* 0 / 1 as for jspsr_pack_weight */
  int c_pad;
  int dtype;          /* JSPSR_F32 / JSPSR_BF16 */
  int reserved;
} jspsr_pack_desc;
int jspsr_pack_chunk(void);
int jspsr_pack_weights_multi(const jspsr_pack_desc* descs, int n, long long total_blocks, jspsr_stream_t stream);

/* out[b,oy,ox,n] = bias[n] + sum_{ky,kx,c} in[b, oy*stride-pad+ky, ox*stride-pad+kx, c] * W[n,ky,kx,c]
 * (+ ReLU if relu != 0).  wpack: mode-0 packing with c_pad = Cin.  bias may be NULL.
 * stats (may be NULL; requires bias == NULL and relu == 0): the epilogue also writes the BatchNorm batch
 * statistics of the result taken from the fp32 accumulators -- jspsr_conv2d_stats_rows(B,OH,OW) partial
 * rows of [sum over the row's pixels | sum of squares] x Cout floats, to be handed to jspsr_bn_forward
 * (ext_partial / ext_rows), which then skips its own pass over the tensor. */
/* Inference epilogue (all optional, NULL = absent): out = [relu](acc * scale[c] + bias[c] + addend), the ReLU always
 * last.  With scale/bias from jspsr_bn_fold and addend = the shortcut tensor this is conv -> BatchNorm(eval)
 * (-> + residual) (-> ReLU) of basics.py:49-53,111-123 in one launch.  Not combinable with `stats`. */
/* Input transform (in_affine, may be NULL): [2][Cin] fp32 (scale | shift), 16-byte aligned.  The gathered tensor is
 * then read as [relu](in * scale[c] + shift[c]) -- applied between the patch registers and LDS, zero padding stays
 * zero -- so a conv can consume the RAW output of the preceding conv plus that layer's BatchNorm affine
 * (jspsr_bn_forward: affine_out) instead of a normalised copy: conv -> BN -> ReLU -> conv of BasicBlock,
 * basics.py:111-117, without the normalised activation ever existing in memory.  Available where
 * jspsr_conv2d_in_affine_ok(dtype, Cin, KH, KW, stride) != 0 (the patch kernel: stride 1, 2..9 taps, Cin a multiple
 * of 32 fp32 / 64 bf16); JSPSR_EINVAL otherwise. */
int jspsr_conv2d_stats_rows(int B, int OH, int OW);
int jspsr_conv2d_in_affine_ok(int dtype, int Cin, int KH, int KW, int stride);
int jspsr_conv2d_forward(int dtype, const void* in, const void* wpack, const float* bias, void* out,
                         int B, int IH, int IW, int Cin, int in_cstride, int in_coff, int Cout,
                         int out_cstride, int out_coff, int KH, int KW, int stride, int pad, int relu,
                         float* stats, const float* scale, const void* addend, int add_cstride,
                         const float* in_affine, int in_relu, jspsr_stream_t stream);
/* The same conv reading its input through a PER-IMAGE per-channel scale (ChannelAttention in front of a conv,
 * basics.py:57-58): in_scale [B][in_scale_bstride] fp32 (16-byte aligned, the stride a multiple of 4 and >= Cin) -- the s
 * of jspsr_gate_mlp_forward as it stands.  A tile lies inside one image b and reads in[b,..,c] * in_scale[b][c] while it
 * stages its patch: a plain fp32 multiply rounded once to `dtype`, the bits jspsr_gate_scale would have stored; zero
 * padding stays zero.  Available where jspsr_conv2d_in_affine_ok(...) != 0; JSPSR_EINVAL otherwise. */
int jspsr_conv2d_forward_scaled(int dtype, const void* in, const void* wpack, const float* bias, void* out,
                                int B, int IH, int IW, int Cin, int in_cstride, int in_coff, int Cout,
                                int out_cstride, int out_coff, int KH, int KW, int stride, int pad, int relu,
                                float* stats, const float* scale, const void* addend, int add_cstride,
                                const float* in_scale, int in_scale_bstride, jspsr_stream_t stream);

/* gin[b,y,x,c] = bias[c] + sum_{ky,kx,n} gout[b,(y+pad-ky)/stride,(x+pad-kx)/stride,n] * W[n,c,ky,kx]
 * over the taps where the division is exact: the data gradient of the conv above, and equally
 * ConvTranspose2d(stride, pad) forward with gout := its input (IH, IW = its output size).
 * wpack_t: mode-1 packing with c_pad = Cg.  One launch per stride phase (no wasted taps).
 * addend (may be NULL): a tensor on gin's grid, Cin channels at pitch add_cstride, added in the epilogue --
 * gin = [relu](...) + addend.  It carries the gradient that reaches the same tensor along another path (the
 * residual branch of a BasicBlock, basics.py:113-122), which autograd would otherwise add in a separate pass.
 * scale (may be NULL): per-channel factor as in jspsr_conv2d_forward -- ConvTranspose2d -> BatchNorm(eval) -> ReLU
 * of the decoder (basics.py:69-85) in one launch at inference.  gin = [relu](acc * scale + bias + addend).
 * red_x / red_cstride / red_par / red_out (round 4; all NULL / 0: off): the REDUCE pass of the BatchNorm whose output
 * gradient this launch produces (conv -> BN -> ReLU -> conv of BasicBlock, basics.py:111-117: gin is the gradient of the
 * ReLU's output), taken in the epilogue instead of by a pass of its own.  red_x: that BatchNorm's saved input on gin's grid
 * (Cin channels at pitch red_cstride); red_par [4][Cin] from jspsr_bn_reduce_params; red_out: partial rows
 * [jspsr_conv2d_stats_rows(B, IH, IW)][2][Cin] = per 8x16-pixel tile the sums of dz and dz * xhat, dz = the stored gin where
 * the ReLU was open -- handed to jspsr_bn_backward as ext_partial.  Available where
 * jspsr_conv2d_dgrad_reduce_ok(...) != 0 (3x3, stride 1, pad 1 on the patch kernel). */
int jspsr_conv2d_dgrad_reduce_ok(int dtype, int B, int IH, int IW, int Cg, int Cin, int KH, int KW, int stride, int pad);
int jspsr_conv2d_dgrad(int dtype, const void* gout, const void* wpack_t, const float* bias, void* gin,
                       int B, int OH, int OW, int Cg, int g_cstride, int g_coff, int IH, int IW,
                       int Cin, int in_cstride, int in_coff, int KH, int KW, int stride, int pad,
                       int relu, const void* addend, int add_cstride, const float* scale,
                       const void* red_x, int red_cstride, const float* red_par, float* red_out, jspsr_stream_t stream);

/* Weight gradient (autograd of nn.Conv2d / nn.ConvTranspose2d w.r.t. .weight):
 *   dW[r][c][ky][kx] = sum_{b,oy,ox} G[b,oy,ox,r] * X[b, oy*stride-pad+ky, ox*stride-pad+kx, c]
 * G lives on the conv's output grid (B,OH,OW,Cg), X on its input grid (B,IH,IW,Cx); Cg, Cx are the
 * chunk-padded channel counts, R <= Cg and C <= Cx the real ones; dW is fp32 in PyTorch's
 * (R, C, KH, KW) layout and is overwritten (accumulate == 0) or added to (accumulate != 0).
 * Conv2d(I->O): G = grad_out, X = input, R = O, C = I.  ConvTranspose2d(I->O, weight (I,O,KH,KW)):
 * G = its input, X = grad of its output, R = I, C = O.
 * workspace: jspsr_conv2d_wgrad_workspace_bytes() bytes (split-K slabs, summed in a fixed order).
 * x_affine (may be NULL): [2][Cx] (scale | shift) -- X is read as [relu](X * scale + shift), the counterpart of
 * jspsr_conv2d_forward's in_affine for the weight gradient of a conv whose normalised input was never materialised.
 * Available where jspsr_conv2d_wgrad_x_affine_ok(...) != 0 (the nine-tap kernel: 3x3, stride 1, pad 1).
 */
size_t jspsr_conv2d_wgrad_workspace_bytes(int dtype, int B, int OH, int OW, int Cg, int Cx, int KH, int KW);
int jspsr_conv2d_wgrad_x_affine_ok(int dtype, int B, int OH, int OW, int Cg, int Cx, int KH, int KW, int stride, int pad);
int jspsr_conv2d_wgrad(int dtype, const void* G, int Cg, int g_cstride, int g_coff, const void* X, int Cx,
                       int x_cstride, int x_coff, float* dW, int R, int C, int B, int OH, int OW,
                       int IH, int IW, int KH, int KW, int stride, int pad, int accumulate,
                       const float* x_affine, int x_relu, void* workspace, jspsr_stream_t stream);
/* The weight gradient of jspsr_conv2d_forward_scaled: X is read as X[b,..,c] * x_scale[b][c] (x_scale [B][x_scale_bstride]
 * fp32, as in_scale there) while it is staged.  Available where jspsr_conv2d_wgrad_x_affine_ok(...) != 0. */
int jspsr_conv2d_wgrad_scaled(int dtype, const void* G, int Cg, int g_cstride, int g_coff, const void* X, int Cx,
                              int x_cstride, int x_coff, float* dW, int R, int C, int B, int OH, int OW,
                              int IH, int IW, int KH, int KW, int stride, int pad, int accumulate,
                              const float* x_scale, int x_scale_bstride, void* workspace, jspsr_stream_t stream);

/* ---- K4/K5: per-channel operators around the convolutions (HBM-bound, NHWC) -----------------
 * Tensors are (pointer, channel pitch, channel offset) slices of NHWC buffers, `npix` pixels,
 * `C` channels (multiple of 4 for fp32 / 8 for bf16); statistics and parameters are fp32.
 * workspace: jspsr_reduce_workspace_bytes(dtype, C, nseg) bytes, 16-byte aligned
 * (nseg = 1, or the batch size for the per-image gate kernels).  It is the maximum over what the entry points write,
 * in floats, with chunks = the pixel chunks of a segment (at most max(1, JSPSR_RED_BLOCKS / (ceil(C / vec / 64) * nseg)),
 * JSPSR_RED_BLOCKS = 1024 by default) and rows = nseg * chunks:
 *   jspsr_bn_forward            scale | shift [2][C], then partial rows [r][2][C]: r = chunks with its own statistics
 *                               pass, r = min(ext_rows, 256) with ext_partial (copied, or folded when ext_rows > 256)
 *                               -> up to (2 + 2 * 256) C whatever the chunk count
 *   jspsr_bn_backward           coef [3][C], then partial rows [r][2][C], r = chunks (own reduce pass, or the fold of
 *                               more than 1024 ext_partial rows; up to 1024 such rows are read in place)
 *   jspsr_act_backward          partial rows [chunks][C]
 *   jspsr_gate_pool             sum | max | index, [rows][C] each
 *   jspsr_gate_backward_reduce  partial rows [rows][C]
 * -> max(3 rows + 4, 2 + 2 * 256) * C floats (+ 64 bytes).
 *   jspsr_bn_backward_pair      coef [6][C], then partial rows [chunks][3][C] = (3 rows + 6) C: two C MORE than the above
 *                               at the full chunk count -> its own query, jspsr_bn_backward_pair_workspace_bytes
 */
size_t jspsr_reduce_workspace_bytes(int dtype, int C, int nseg);

/* nn.BatchNorm2d forward fused with the residual add and ReLU of BasicBlock
 * (models/components/basics.py:49-53,81-85,111-123):
 *   y = [relu]( bn(x) * res_scale + res )      (res may be NULL)
 * training != 0: batch statistics (biased var), running stats updated in place with `momentum`
 * (unbiased var), save_mean / save_invstd [C] written for the backward.  training == 0: running
 * stats are used (and copied to save_*).  ext_partial / ext_rows: statistics already accumulated by
 * jspsr_conv2d_forward (NULL / 0: this call makes its own pass over x).
 * The shortcut of a projecting BasicBlock is itself conv1x1 -> BatchNorm (basics.py:118-119): instead of normalising
 * it in a pass of its own, that BatchNorm is called with y == NULL and affine_out [2][C] (statistics, running stats
 * and its per-channel scale | shift only), and the block's second BatchNorm takes the RAW conv1x1 output as `res`
 * together with res_affine = that [2][C]:  y = [relu]( bn(x) * res_scale + (res * res_affine[0] + res_affine[1]) ).
 * mask_out (may be NULL; needs res, relu and y): the ReLU's bit mask for the backward, jspsr_bn_mask_bytes(dtype, npix, C)
 * bytes -- one bit per element, set where y AS STORED (after rounding to the storage type) is > 0.  jspsr_bn_backward
 * (relu = 1) takes it in place of y: one byte per 16 bytes of y to read.  The layout is private to the two entries. */
size_t jspsr_bn_mask_bytes(int dtype, long long npix, int C);
int jspsr_bn_forward(int dtype, const void* x, int x_cs, int x_coff, const void* res, int r_cs, int r_coff,
                     void* y, int y_cs, int y_coff, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, int training,
                     int relu, float res_scale, float* save_mean, float* save_invstd, long long npix, int C,
                     const float* ext_partial, int ext_rows, const float* res_affine, float* affine_out,
                     void* mask_out, void* workspace, jspsr_stream_t stream);

/* BatchNorm in eval mode as a per-channel affine: scale = gamma / sqrt(var + eps) * res_scale,
 * shift = (beta - mean * gamma / sqrt(var + eps)) * res_scale. */
int jspsr_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                  float eps, float res_scale, int C, float* scale, float* shift, jspsr_stream_t stream);

/* Backward of the above.  dy is the gradient w.r.t. y.  relu: 0 = none; 1 = mask from the saved output
 * (y > 0); 2 = mask recomputed from x as gamma*xhat + beta > 0 (valid without a residual; y is not read).
 * dx (dense, pitch C) = grad w.r.t. x; dres (dense, may be NULL) = grad w.r.t. res;
 * dgamma, dbeta [C]: overwritten, or added to when accumulate != 0 (gradients landing directly in a
 * caller-owned accumulation buffer).
 * ext_partial / ext_rows (NULL / 0: this call makes its own reduce pass): the per-tile sums of dz and dz * xhat, rows of
 * [2][C], that the producing data gradient's epilogue wrote (jspsr_conv2d_dgrad: red_out) -- relu mode 2 only.
 * mask (may be NULL; relu = 1 only): the bit mask jspsr_bn_forward wrote (mask_out); it replaces the reads of y, which
 * may then be NULL.  Same bits as with y.
 * relu = 1 with dres != NULL makes 7 tensor passes (6 with mask) instead of 8: the reduce pass writes dres = the masked dy
 * while it sums, and the apply pass reads dres back as its dy.  Sums, order and results are those of the 8-pass form. */
int jspsr_bn_reduce_params(const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, int C,
                           float* par, jspsr_stream_t stream);
int jspsr_bn_backward(int dtype, const void* dy, int dy_cs, int dy_coff, const void* y, int y_cs, int y_coff,
                      const void* x, int x_cs, int x_coff, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_invstd, int training, int relu, float res_scale, void* dx, void* dres,
                      float* dgamma, float* dbeta, int accumulate, long long npix, int C, void* workspace,
                      const float* ext_partial, int ext_rows, const void* mask, jspsr_stream_t stream);

/* (ABI v25, additive) The backward of a projecting BasicBlock's two BatchNorms in one reduce and one apply pass: the block's
 * second BatchNorm (input x2; residual + ReLU, `mask` = the bit mask jspsr_bn_forward wrote; sees dz * res_scale) and the
 * shortcut's BatchNorm (input xd = the raw 1x1 output; no ReLU, no scale) receive the same gradient dz = dy where the ReLU
 * was open.  Equivalent, bit for bit, to
 *   jspsr_bn_backward(dy, x2, relu = 1, mask, res_scale, dx = dx2, dres)  then  jspsr_bn_backward(dres, xd, relu = 0, 1.0, dx = dxd)
 * without dres: 8.12 tensor passes instead of 11.06, 3 launches instead of 6 (census labels bn_bwd_reduce_pair,
 * bn_bwd_finalize_pair, bn_bwd_apply_pair).  dy, x2, xd: channel slices (pitch, offset); dx2, dxd: dense, pitch C, distinct.
 * training / accumulate / the parameter-gradient buffers are per layer, with jspsr_bn_backward's meaning.
 * JSPSR_EINVAL: a null pointer (mask included: the mask-from-y and ReLU-free forms stay with the two calls), npix <= 0, C,
 * a pitch or an offset that is no multiple of the vector width, a slice that does not fit its pitch, shared outputs;
 * JSPSR_EALIGN: a tensor or the workspace not 16-byte aligned; all decided before any launch.
 * workspace: jspsr_bn_backward_pair_workspace_bytes(dtype, C) bytes (0 = bad arguments). */
size_t jspsr_bn_backward_pair_workspace_bytes(int dtype, int C);
int jspsr_bn_backward_pair(int dtype, const void* dy, int dy_cs, int dy_coff, const void* mask, const void* x2, int x2_cs,
                           int x2_coff, const float* gamma2, const float* save_mean2, const float* save_invstd2,
                           int training2, float res_scale, const void* xd, int xd_cs, int xd_coff, const float* gammad,
                           const float* save_meand, const float* save_invstdd, int trainingd, void* dx2, void* dxd,
                           float* dgamma2, float* dbeta2, int accumulate2, float* dgammad, float* dbetad, int accumulated,
                           long long npix, int C, void* workspace, jspsr_stream_t stream);

/* Backward of the conv epilogue `y = [relu](conv + bias)` of the BN-free Basic2d (basics.py:36-53):
 * dz = dy * [y > 0] (y read with channel pitch y_cs; dz written with pitch dz_cs if dz != NULL),
 * dbias[c] = sum dz (if dbias != NULL). */
int jspsr_act_backward(int dtype, const void* dy, int dy_cs, int dy_coff, const void* y, int y_cs, int relu, void* dz,
                       int dz_cs, float* dbias, long long npix, int C, void* workspace, jspsr_stream_t stream);

/* ChannelAttention (models/components/resnet_cbam.py:36-53; applied in basics.py:57-58).
 * gate_pool: avg[b,c], mx[b,c] over the npix pixels of image b, amax = smallest pixel index of the
 * max.  gate_scale: y = x * s[b,c].  Backward: ds[b,c] = sum_p dy*x (reduce), then
 * dx = dy*s + davg/npix + [p == amax] dmax (apply).  The C -> C/16 -> C MLP between pool and
 * scale works on B x C vectors: jspsr_gate_mlp_* below. */
int jspsr_gate_pool(int dtype, const void* x, int B, long long npix, int C, float* avg, float* mx, int* amax,
                    void* workspace, jspsr_stream_t stream);
int jspsr_gate_scale(int dtype, const void* x, const float* s, void* y, int B, long long npix, int C,
                     jspsr_stream_t stream);
int jspsr_gate_backward_reduce(int dtype, const void* dy, const void* x, float* ds, int B, long long npix, int C,
                               void* workspace, jspsr_stream_t stream);
int jspsr_gate_backward_apply(int dtype, const void* dy, const float* s, const float* davg, const float* dmax,
                              const int* amax, void* dx, int B, long long npix, int C, jspsr_stream_t stream);

/* ---- the two ends of the training step ----------------------------------------------------
 * Fused loss of the reference configs (MultiLoss, losses/loss_schemes.py:55-72; weights from
 * configs/<name>.yml:67-70): losses[4] = {L1, L2, Grad, Total = w1*L1 + w2*L2 + wg*Grad} on fp32
 * (B,1,H,W) tensors; Grad = L1 between normalised Sobel gradients with replicate padding
 * (losses/loss_functions.py:171-185).  The backward writes d(Total)/d(pred) * grad_total[0]
 * (grad_total may be NULL = 1).  workspace: jspsr_loss_workspace_bytes() bytes (0 = a non-positive size), 16-byte aligned
 * (JSPSR_EALIGN, decided before any launch), shared by both calls; the same holds for jspsr_loss_valid_*, whose
 * workspace carries two 64-bit counts from the forward to the backward.
 */
size_t jspsr_loss_workspace_bytes(int B, int H, int W);
int jspsr_loss_forward(const float* pred, const float* gt, float w1, float w2, float wg, float* losses,
                       void* workspace, int B, int H, int W, jspsr_stream_t stream);
int jspsr_loss_backward(const float* pred, const float* gt, const float* grad_total, float w1, float w2,
                        float wg, float* grad_pred, const void* workspace, int B, int H, int W,
                        jspsr_stream_t stream);

/* The rest of the reference's loss menu (get_loss, losses/loss_schemes.py:6-33; get_criterion,
 * utils/common_config.py:209-233) on fp32 (planes, H, W) tensors (ABI v17).  `terms` is a bit set: 1 BerHu
 * (BerhuLoss, losses/loss_functions.py:191-208), 2 BCE-with-logits (nn.BCEWithLogitsLoss), 4 surface normal of a
 * one-channel map (SurfaceNormalLoss :211-229), 8 SSIM (SSIMLoss :232-239 = 1 - piq.ssim(clamp(pred,0,1), gt,
 * data_range=1, downsample=False): 11-tap Gaussian (sigma 1.5) window, valid map (H-10) x (W-10)).  Term slots:
 * 0 L1, 1 L2, 2 Grad (taken from losses[0..2] of jspsr_loss_forward, passed as base_losses), 3 BerHu, 4 BCE, 5 Norm,
 * 6 SSIM.  BerHu's threshold 0.6 max|pred - gt| stays in device memory.  No host synchronisation.
 * Forward: out[k] = the term of key k (key_slot[k], host array of n_keys <= 16), out[n_keys] = Total = sum_k
 * key_weight[k] * out[k] (host doubles; in double, rounded once).  workspace: jspsr_loss_menu_workspace_bytes(), shared
 * with the backward, which ADDS d(sum_s slot_weight[s] term_s)/d(pred) * grad_total[0] over the slots 3..6 of `terms`
 * (slot_weight: host doubles [7]; grad_total may be NULL = 1) to grad_pred.  JSPSR_EINVAL on bad arguments, SSIM with
 * H < 11 or W < 11 among them; the workspace query returns 0 there.  The workspace of every entry of this family
 * (jspsr_loss_menu_*, jspsr_loss_menu_valid_*, jspsr_loss_menu_valid_ssim_*, jspsr_ssim_forward,
 * jspsr_ssim_tiles_forward) is 16-byte aligned: JSPSR_EALIGN, decided before any launch. */
size_t jspsr_loss_menu_workspace_bytes(int terms, int planes, int H, int W);
int jspsr_loss_menu_forward(const float* pred, const float* gt, int terms, int planes, int H, int W, int n_keys,
                            const int* key_slot, const double* key_weight, const float* base_losses, float* out,
                            void* workspace, jspsr_stream_t stream);
int jspsr_loss_menu_backward(const float* pred, const float* gt, int terms, int planes, int H, int W,
                             const double* slot_weight, const float* grad_total, float* grad_pred,
                             const void* workspace, jspsr_stream_t stream);
/* K19: both loss families over the elements a validity plane keeps (training on a ground truth with voids).  valid:
 * [planes][H][W] bytes beside pred and gt, nonzero = valid; every other argument as in the unmasked call of the same name.
 * A masked element has no influence whatever pred and gt hold there (NaN, inf, a no-data code): they are read only behind
 * a select on the plane.  With d = pred - gt and N the valid elements of the whole call: L1 = sum_valid |d| / N, L2 =
 * sum_valid d^2 / N; a Sobel output counts iff its nine replicate-clamped taps are valid, Grad = sum_counted (|gx| + |gy|)
 * / (2 N_g); BerHu's threshold is 0.6 max_valid |d|; BerHu, BCE and Norm are their pointwise expressions over the valid
 * elements, divided by N.  N = 0 (N_g = 0) gives value 0 and gradient 0.  N and N_g are counted exactly, as integers, by
 * the forward and stay in the workspace, where the backward reads them: no host synchronisation, capturable in a graph.
 * The gradient is +0.0 at every invalid element: jspsr_loss_valid_backward writes it, jspsr_loss_menu_valid_backward leaves
 * the caller's value (which it ADDS to elsewhere) untouched there.  An all-ones plane gives the bits of the unmasked calls:
 * every pass is one kernel body, instantiated with and without the plane.
 * jspsr_loss_menu_valid_* refuse SSIM (term bit 8, slot 6): JSPSR_EINVAL, workspace query 0.  They are
 * jspsr_loss_menu_valid_ssim_* (below) with that bit refused: the same host path, launches and workspace. */
size_t jspsr_loss_valid_workspace_bytes(int B, int H, int W);
int jspsr_loss_valid_forward(const float* pred, const float* gt, const unsigned char* valid, float w1, float w2, float wg,
                             float* losses, void* workspace, int B, int H, int W, jspsr_stream_t stream);
int jspsr_loss_valid_backward(const float* pred, const float* gt, const unsigned char* valid, const float* grad_total,
                              float w1, float w2, float wg, float* grad_pred, const void* workspace, int B, int H, int W,
                              jspsr_stream_t stream);
size_t jspsr_loss_menu_valid_workspace_bytes(int terms, int planes, int H, int W);
int jspsr_loss_menu_valid_forward(const float* pred, const float* gt, const unsigned char* valid, int terms, int planes,
                                  int H, int W, int n_keys, const int* key_slot, const double* key_weight,
                                  const float* base_losses, float* out, void* workspace, jspsr_stream_t stream);
int jspsr_loss_menu_valid_backward(const float* pred, const float* gt, const unsigned char* valid, int terms, int planes,
                                   int H, int W, const double* slot_weight, const float* grad_total, float* grad_pred,
                                   const void* workspace, jspsr_stream_t stream);
/* K23: the K19 menu entries with SSIM over the plane under the "window" rule (ssim_rule = 1; anything else is
 * JSPSR_EINVAL): an element of the valid (H-10) x (W-10) SSIM map counts iff all 121 pixels under its window are valid;
 * with N_s the counted elements of the whole call, SSIM = 1 - sum_counted S / N_s.  N_s = 0 gives value 0 and gradient 0.
 * pred and gt are staged as 0 at invalid pixels behind a select, so a masked pixel has no influence whatever they hold
 * there, and its gradient stays the caller's +0.0; a NaN at a valid pixel poisons the result as in the unmasked call.  N_s
 * is counted as an integer by the forward (one launch, census label ssim_valid_forward), folded by the combine kernel and
 * kept in the workspace, where the backward (one launch, ssim_valid_backward) forms (float)(w / (double)N_s): no host
 * synchronisation.  An all-ones plane gives the bits of jspsr_loss_menu_forward / _backward.  Every other argument and
 * every other term as in jspsr_loss_menu_valid_*.  The three menu families are one host path and one kernel family
 * (csrc/loss_terms.hip): without a plane, with a plane and SSIM refused, with a plane and SSIM under ssim_rule; without
 * the SSIM bit ssim_rule is only range-checked.  SSIM needs H, W >= 11 (JSPSR_EINVAL, workspace query 0). */
size_t jspsr_loss_menu_valid_ssim_workspace_bytes(int terms, int planes, int H, int W, int ssim_rule);
int jspsr_loss_menu_valid_ssim_forward(const float* pred, const float* gt, const unsigned char* valid, int terms, int planes,
                                       int H, int W, int ssim_rule, int n_keys, const int* key_slot,
                                       const double* key_weight, const float* base_losses, float* out, void* workspace,
                                       jspsr_stream_t stream);
int jspsr_loss_menu_valid_ssim_backward(const float* pred, const float* gt, const unsigned char* valid, int terms,
                                        int planes, int H, int W, int ssim_rule, const double* slot_weight,
                                        const float* grad_total, float* grad_pred, const void* workspace,
                                        jspsr_stream_t stream);
/* K23: SSIM of every tile of a batch for the meters.  pred, gt: UNCROPPED fp32 [B][H][W]; the crop of `border` (a
 * fraction in [0, 0.5): int(H * border) rows and int(W * border) columns on every side, in double) is index arithmetic.
 * valid: [B][H][W] bytes, nonzero = valid, or NULL = every pixel.  same / window11 as jspsr_ssim_forward (same = 0: the
 * valid map, all of whose windows lie inside the crop; same = 1: the map of the crop with zero padding 5, where a tap
 * outside the crop is padding, not a void).  out[b] (device) = the mean of S over tile b's counted map elements, NaN
 * where there is none; counts[b] (device int32) = their number.  Two launches whatever B is (ssim_tiles_forward,
 * ssim_tiles_finalize); tile b's partials are folded in the order jspsr_ssim_forward folds a one-plane call, so with
 * valid = NULL or all ones out[b] has the bits of jspsr_ssim_forward on the prepared tile b alone.  JSPSR_EINVAL: a null
 * pointer (valid excepted), B <= 0, a border outside [0, 0.5), nothing left after the crop, same = 0 with fewer than 11
 * rows or columns left.  workspace: jspsr_ssim_tiles_workspace_bytes() (0 = bad arguments). */
size_t jspsr_ssim_tiles_workspace_bytes(int B, int H, int W, double border, int same);
int jspsr_ssim_tiles_forward(const float* pred, const float* gt, const unsigned char* valid, int B, int H, int W,
                             double border, int same, const float* window11, float* out, int* counts, void* workspace,
                             jspsr_stream_t stream);
/* Mean SSIM of prepared [0,1] tiles (MeterSSIM.update, evaluation/metrics.py:275-335), pred clamped to [0,1]:
 * same = 0 is piq.ssim(downsample=False) on the valid map with the Gaussian window (window11 ignored, may be NULL);
 * same = 1 is the local ssim (metrics.py:20-63): H x W map over the zero-padded planes with the 11-tap window11 (host
 * floats; NULL = the Gaussian).  out[0] (device) = the mean over every map element of every plane.  workspace:
 * jspsr_ssim_workspace_bytes() (0 = bad arguments). */
size_t jspsr_ssim_workspace_bytes(int planes, int H, int W, int same);
int jspsr_ssim_forward(const float* pred, const float* gt, int planes, int H, int W, int same, const float* window11,
                       float* out, void* workspace, jspsr_stream_t stream);

/* Evaluation scores of one tile on the device (evaluation/metrics.py: MeterBase._prepare :147-199, MeterPSNR :229-235,
 * MeterRMSE :372-384, MeterMedian :453, MeterNMAD :508-510, MeterLE95 :565-568; ToDEM.descale_data,
 * data/data_utils.py:441-457).  pred, gt: fp32 [H][W] in the network's [0,1] range (the reference evaluates one tile
 * at a time).  border: fraction cropped on every side (int(H * border) rows, int(W * border) columns); the prediction is
 * clamped to [0,1]; both are de-scaled to metres with (value_min, value_max, elev_log).
 * scores[5] (device) = {PSNR on the [0,1] tensors, RMSE, median, NMAD, LE95 of the elevation differences}.  The order
 * statistics are exact (radix select; torch.median's lower-middle convention, kthvalue with k = 1 + round(0.95 (n-1))).
 * No host synchronisation.  workspace: jspsr_metrics_workspace_bytes(H, W) bytes, 16-byte aligned. */
size_t jspsr_metrics_workspace_bytes(int H, int W);
int jspsr_metrics_forward(const float* pred, const float* gt, int H, int W, float border, float value_min,
                          float value_max, int elev_log, float* scores, void* workspace, jspsr_stream_t stream);

/* K10 (ABI v19): the evaluation scores of a whole batch of tiles in one call -- what PerformanceMeter.update does one
 * tile at a time with one meter object and one host round trip per score (evaluation/evaluate_utils.py:26-47, get_meter
 * :50-118; evaluation/metrics.py: MeterBase._prepare :147-199, psnr :97-113, Sobel :116-139, MeterPSNR :229-250,
 * MeterRMSE :372-384, MeterMedian :453, MeterNMAD :508-510, MeterLE95 :565-568, MeterSlope :648-673).
 * pred, gt: fp32 [B][H][W] in the network's range.  Crop, clamp and de-scaling as jspsr_metrics_forward (the same
 * expressions: the elevation differences dh have the same bits).  scores (device, [B][8]), per tile:
 *   0 PSNR "piq"   -10 log10(mse + 1e-8) on the [0,1] tensors      1 PSNR "local"  20 log10(1 / sqrt(mse)), 100 at mse == 0
 *   2 RMSE   3 median   4 NMAD   5 LE95 of dh (the three order statistics exact, as jspsr_metrics_forward)
 *   6 slope "local":  sqrt(mean((|S P| - |S G|)^2)) over the (h-2)(w-2) valid outputs of the unnormalised 3x3 Sobel pair
 *   7 slope "kornia": sqrt(mean((grad P - grad G)^2)) over 2 h w values of spatial_gradient (replicate pad, Sobel / 8);
 *                     restated from kornia's public source, not pinned against kornia itself
 * A cropped tile of at most 20 272 pixels (142 x 142; 128 x 128 at border 0) is scored by ONE launch, one workgroup per
 * tile with both de-scaled rasters in LDS; larger tiles stream through 27 launches whatever B is.  Sums fold in double in
 * an order fixed by (h, w): row b does not depend on B or on the other tiles.  No host synchronisation.
 * JSPSR_EINVAL: B <= 0, border outside [0, 0.5), value_max - value_min <= 1, nothing or fewer than 3 rows / columns
 * left after the crop.  workspace: jspsr_scores_batch_workspace_bytes(B, H, W) bytes, 16-byte aligned (JSPSR_EALIGN).
 * The query returns 0 for what the entry refuses whatever the border is: B <= 0, H < 3, W < 3, H * W above 2^30 - 1.
 * A raster of at most 20 272 pixels before the crop gets 16 bytes, of which the one-launch path touches none. */
size_t jspsr_scores_batch_workspace_bytes(int B, int H, int W);
int jspsr_scores_batch_forward(const float* pred, const float* gt, int B, int H, int W, float border, float value_min,
                               float value_max, int elev_log, float* scores, void* workspace, jspsr_stream_t stream);

/* K12 (ABI v22): the whole-set validation summary -- what the reference's --val path does on the host after the model has
 * run (csrc/summary.hip).
 *
 * jspsr_scenes_assemble_f32: save_prediction_to_disk (evaluation/evaluate_utils.py:242-271: clip to [0,1], descale_data,
 *   + base) and merge_dem(..., p.val_border, method = copyto_add) (utils/utils.py:914-967, called at :1272) for all S
 *   scenes of a batch in ONE launch.  tiles [S * n_x * n_x][k][k] fp32 in the network's range, row-major over each scene's
 *   cover; base [S] (device) the scenes' base elevations; ramp [p] as for the K8 merge (NULL when p = 0 or n_x = 1);
 *   out_off [S] (device, int64) the element offset of mosaic s in the pooled buffer `out` of out_numel elements (a mosaic
 *   that would leave it is not written).  Mosaic side: stride (n_x - 1) + k - 2 border_px; n_x = 1 is the 8 m case: the
 *   de-scaled tile, k x k, uncropped (border_px and stride ignored; the crop happens at summary time, utils.py:1300-1306).
 *   Bit-equal to clamp -> jspsr_elev_scale_f32 (descale) -> + base -> the K8 merge run scene by scene.
 *
 * jspsr_summary_forward: summarise_evaluation (utils/utils.py:1238-1356) -- RMSE, median, NMAD, LE95 and PSNR of the errors
 *   of n_cand candidates (1..8: the prediction and the baseline DEMs, fp32 metres) against one ground truth, pooled over
 *   SEGMENTS of pitched windows (one segment of all scenes: the reference's "offline" numbers; one per scene: its
 *   "online" ones).  cands / cand_numel: HOST arrays of n_cand device pointers and their element counts; gt likewise.
 *   windows (device, int64 [n_windows][22]) = { segment, h, w, offset of the window's first error in the pooled error
 *     array, gt offset, gt row pitch, then { offset, row pitch } of candidate 0..7 } in elements; rows ascending in the
 *     error offset, the windows of a segment back to back, the error array without gaps.  A read outside its buffer, and
 *     an element no window of its segment covers, give NaN.  Crops are read in place.
 *   segments (device, int64 [n_segments][8]) = { start in the error array, n, first chunk, median ranks (n - 1) / 2 and
 *     n / 2, LE95 ranks l = floor(0.95 (n - 1)) and min(l + 1, n - 1), the bits of the double g = 0.95 (n - 1) - l };
 *     chunks are runs of 8192 elements of ONE segment, numbered through the segments in order.  total = sum of n;
 *     total_chunks = sum of ceil(n / 8192).  The table is made by one host function (jspsr_amd/summary.py: segment_ranks).
 *   out (device, [n_cand * n_segments][11], row = candidate * n_segments + segment) =
 *     { RMSE, Median, NMAD, LE95, PSNR, median lo, hi, MAD lo, hi, LE95 lo, hi }, the last six the bracketing order
 *     statistics (exact elements of e, |e - median|, |e|).
 *   e = cand - gt in fp32.  RMSE = sqrt(sum e^2 / n), squares and sum in fp64 folded in an order the segment's size alone
 *     fixes, rounded once (the reference's fp32 pairwise np.mean of fp32 squares is NOT reproduced).  Median = (lo + hi) *
 *     0.5f, bit for bit np.median of a float32 array.  NMAD = fp32(1.4826 * double((lo + hi) * 0.5f)) over |e - Median| in
 *     fp32.  LE95 = fp32(lo + (hi - lo) g) in double: np.percentile(|e| as float64, 95); on float32 input numpy 2 forms the
 *     virtual index in float32 and numpy 1 in float64, so the reference's own value depends on the numpy version (up to
 *     2.4e-4 relative apart in random trials) -- not chased.  PSNR = 20 log10(value_max / rmse) in double, +inf at rmse = 0
 *     (the 1e-8 that the reference's online form adds for the baselines is NOT reproduced).  A NaN among a segment's
 *     errors makes the row's five scores NaN.
 *   16 launches whatever n_windows, n_segments and n_cand are; a row has the same bits for every n_cand, whatever other
 *   segments the call holds, on every run.  No host synchronisation.
 *   JSPSR_EINVAL: a null pointer, n_cand outside 1..8, an empty table or total <= 0, total >= 2^32 (32-bit rank counters),
 *   sizes that do not fit together.  workspace: jspsr_summary_workspace_bytes(...) bytes (0 = bad arguments), 16-byte
 *   aligned (JSPSR_EALIGN). */
int jspsr_scenes_assemble_f32(const float* tiles, const float* base, const float* ramp, float* out, const long long* out_off,
                              long long out_numel, int S, int n_x, int k, int border_px, int stride, int elev_log,
                              double elev_min, double elev_max, jspsr_stream_t stream);
size_t jspsr_summary_workspace_bytes(int n_cand, int n_segments, long long total, long long total_chunks);
int jspsr_summary_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                          long long gt_numel, const long long* windows, int n_windows, const long long* segments,
                          int n_segments, long long total, long long total_chunks, double value_max, float* out,
                          void* workspace, jspsr_stream_t stream);

/* ---- K13 (ABI v23): whole-scene inference, the steps either side of the forward (csrc/scene_prepare.hip, scene.hip)
 * What upscale_dem does around the model call (utils/utils.py:1556-1654): add_padding (:1501-1520) and ToTensor
 * (data/data_utils.py:217-312) before it, remove_padding (:1523-1531) after it -- and, for metres, the clip, descale_data
 * and + base of save_prediction_to_disk (evaluation/evaluate_utils.py:242-271) -- each side ONE launch for a batch of B
 * equally sized scenes.
 *
 * jspsr_scene_prepare: the raw HWC scene store -> the model's fp32 NCHW inputs.  src, src_bytes, out, channels, coff, cpitch
 *   (HOST arrays of 6), scenes, n_scenes, flags, elev_min / elev_max and mask_div exactly as for jspsr_batch_make (K9); kind 1
 *   (hr_dem) is no input of a model and must be absent (out[1] NULL).  out[kind] is (B, cpitch, Hp, Wp).
 *   samples device int32 [B][2] = {scene, base elevation (fp32 bit pattern)}.
 *   rows    device int32 [Hp], cols device int32 [Wp]: out[b][c][Y][X] = ToTensor_kind(scene[rows[Y]][cols[X]][c]).  The
 *     mirror border of add_padding is separable (left / right depend on X only, top / bottom -- the bottom with its
 *     off-by-one -- on Y only), so the two maps carry it index for index, and the extension of the frame to a multiple of
 *     the model's stride and plain crops as well; the policy lives with the caller (jspsr_amd/infer.py: frame_maps).
 *     coord writes rows[Y] / (H - 1) and cols[X] / (W - 1): the local coordinates of the SOURCE pixel.  A sample whose
 *     scene index or store extent is bad, and a map entry outside [0, H) / [0, W), write NaN; nothing is read there.
 *   The per-kind arithmetic is K9's (csrc/totensor.h, shared by both translation units): image, mask, canopy and coord are
 *   the reference's bits, DEM values within 1 ulp of numpy's fp32 log.  16-byte stores when Wp % 4 == 0 and out[kind] is
 *   16-byte aligned; otherwise any 4-byte aligned output.
 *
 * jspsr_scene_finish: pred [B][1][Hp][Wp] in the network's range (dtype JSPSR_F32 or JSPSR_BF16) -> out [B][H][W] fp32,
 *   the window whose corner is (top, left).  metres != 0: clamp to [0, 1] (a NaN stays a NaN, as under torch.clamp), then
 *   v * (max - min) + min, or exp(v * log(max - min)) + min with elev_log, then + base (samples[b][1]), every operation
 *   rounded on its own in fp32 with the constants formed as jspsr_elev_scale_f32 forms them: bit-equal to clamp ->
 *   jspsr_elev_scale_f32 (descale) -> + base.  metres == 0: the window is copied (converted to fp32), nothing else.
 *   samples as above (only the base is read).
 *
 * JSPSR_EINVAL: a null pointer, B <= 0, sizes that do not fit together, a window that leaves the frame.  No host
 * synchronisation. */
int jspsr_scene_prepare(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                        const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples, int B,
                        const int* rows, const int* cols, int Hp, int Wp, int flags, double elev_min, double elev_max,
                        int mask_div, jspsr_stream_t stream);
int jspsr_scene_finish(int dtype, const void* pred, float* out, const int* samples, int B, int Hp, int Wp, int top, int left,
                       int H, int W, int metres, int elev_log, double elev_min, double elev_max, jspsr_stream_t stream);

/* ---- K14 (ABI v24): whole-scene self-ensemble over the flips and quarter turns (csrc/scene_prepare.hip, scene_tta.hip)
 * The reference has no self-ensemble.  What these two replace is the host work a user of K13 needs for one: np.rot90 /
 * fliplr / flipud of every decoded raster (the order of RandomFlipRotate90, data/data_utils.py:26-28), a store and a
 * jspsr_scene_prepare + jspsr_scene_finish pair per orientation, and the inverse transforms and the mean in numpy.
 * A D4 element is K9's code = rot90 * 4 + flip_lr * 2 + flip_ud, the transformed raster flipud?(fliplr?(rot90(a, rot90))),
 * W x H for an odd rot90.  Codes c and c' with flip_ud set / clear, the other flip inverted and rot90 two apart denote the
 * same element (16 codes, 8 elements).
 *
 * jspsr_scene_prepare_d4: replaces the host transform + jspsr_scene_prepare.  As jspsr_scene_prepare, except
 *   samples device int32 [B][3] = {scene, base elevation (fp32 bit pattern), code};
 *   codes   HOST int32 [B], the same codes: every rot90 of a launch has one parity (JSPSR_EINVAL otherwise), so that one
 *     frame serves it;
 *   rows [Hp] / cols [Wp] index the TRANSFORMED scene (padding comes after the transform: the reference's mirror border is
 *     not symmetric): out[b][c][Y][X] = ToTensor_kind(T_b[rows[Y]][cols[X]][c]), T_b the transformed raster of sample b.
 *     coord is transformed with the rest: it holds the local coordinates of the SOURCE pixel.  NaN where
 *     jspsr_scene_prepare writes it (the entries are checked against the transformed shape) and for a sample whose device
 *     code is outside 0..15 or of the other parity.
 *   Even rot90: jspsr_scene_prepare's gather with reversed indices.  Odd rot90: 32 x 32 frame tiles, the source window
 *   staged in LDS (a frame row walks a source column); B <= 65535.  The bits of jspsr_scene_prepare on a store of the
 *   transformed rasters.
 *
 * jspsr_scene_finish_mean: replaces K jspsr_scene_finish launches, the inverse transforms and the mean.  variants HOST
 *   array of K = 1..JSPSR_TTA_MAX_VARIANTS entries, copied into the kernel's arguments (no upload): prediction
 *   [B][1][Hp][Wp] of dtype JSPSR_F32 / JSPSR_BF16 for element `code`, whose h x w window -- the transformed shape of the
 *   H x W scene, JSPSR_EINVAL otherwise -- has its corner at (top, left).  out [B][H][W] fp32 =
 *     post((((y'_0 + y'_1) + y'_2) + ...) / (float)K),  y'_k = the window of variant k carried back by the inverse of its
 *   element, widened to fp32; fp32 additions in the order given, one fp32 division (K = 1: the bits of
 *   jspsr_scene_finish); a NaN in any variant makes the pixel NaN.  post: with metres != 0 the expressions of
 *   jspsr_scene_finish, bit for bit; nothing otherwise.  samples device int32 [B][2] as for jspsr_scene_finish.
 *   JSPSR_EINVAL: K outside 1..8, two variants of the same element, a window that leaves its frame or does not have the
 *   transformed shape, B outside 1..65535.  JSPSR_EALIGN: a pointer not aligned to its element size.  16-byte stores when
 *   W % 4 == 0 and out is 16-byte aligned.  No host synchronisation. */
#define JSPSR_TTA_MAX_VARIANTS 8
typedef struct jspsr_tta_variant {
  const void* pred;
  int dtype, code, Hp, Wp, top, left, h, w;
} jspsr_tta_variant;
int jspsr_scene_prepare_d4(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                           const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                           const int* codes, int B, const int* rows, const int* cols, int Hp, int Wp, int flags,
                           double elev_min, double elev_max, int mask_div, jspsr_stream_t stream);
int jspsr_scene_finish_mean(const jspsr_tta_variant* variants, int K, float* out, const int* samples, int B, int H, int W,
                            int metres, int elev_log, double elev_min, double elev_max, jspsr_stream_t stream);

/* ---- K15 (ABI v25): tiled whole-scene inference, scenes of any size (csrc/scene_prepare.hip, scene_tiles.hip)
 * The reference's evaluation protocol -- tiles of the training size, linear ramps in the overlaps (TileCrop,
 * data/data_utils.py:87-194; gen_weight_row / col + merge_dem, utils/utils.py:802-967) -- for a cover of any H x W scene by
 * n_y x n_x tiles of kh x kw (jspsr_amd/infer.py: plan_cover makes the origins and the weights).  What these two replace
 * is host slicing of the decoded rasters per tile, a store of tiles, a jspsr_scene_prepare + jspsr_scene_finish pair, and
 * the feather merge in numpy.
 *
 * jspsr_scene_prepare_windows: as jspsr_scene_prepare without the rows / cols maps; the windows of a batch may come from
 *   any scenes of the store, of any shapes.
 *   samples device int32 [B][4] = {scene, base elevation (fp32 bit pattern), y0, x0}.
 *   out[kind] is (B, cpitch, kh, kw): out[b][c][y][x] = ToTensor_kind(scene[y0 + y][x0 + x][c]), the arithmetic of
 *   csrc/totensor.h unchanged: the bits of jspsr_scene_prepare's unpadded frame at (y0 + y, x0 + x).  The base is the
 *   scene's, and coord holds the local coordinates of the source pixel over the WHOLE scene, (y0 + y) / (H - 1) and
 *   (x0 + x) / (W - 1).  A window pixel outside its scene, and every pixel of a sample whose scene index or store extent
 *   is bad, is NaN; nothing is read there.  Element offsets are 64-bit (a 37 000 x 37 000 scene's image passes 2^31 bytes).
 *   16-byte stores when kw % 4 == 0 and out[kind] is 16-byte aligned; otherwise any 4-byte aligned output.
 *
 * jspsr_scene_merge_windows: S scenes of one shape H x W and one cover.
 *   tiles   [S][n_y * n_x][kh][kw], dtype JSPSR_F32 or JSPSR_BF16, the tiles of a scene row-major over the cover;
 *   oy [n_y], ox [n_x]   device int32, the tile origins;
 *   wy [n_y][kh], wx [n_x][kw]   device fp32, the weight of tile row ty at its row j (scene row oy[ty] + j), likewise wx;
 *   lo_y [H], lo_x [W]   device int32, the lowest tile index whose weight at that coordinate is not zero;
 *   samples device int32 [S][2] as for jspsr_scene_finish (only the base is read).
 *   out [S][H][W] fp32.  Per pixel (y, x): acc = 0; for ty in {lo_y[y], lo_y[y] + 1}, for tx in {lo_x[x], lo_x[x] + 1}, in
 *   that (row-major) order, where the tile exists, holds the pixel and wy[ty][y - oy[ty]] != 0 and wx[tx][x - ox[tx]] != 0:
 *     acc = acc + (m * wx) * wy,   every operation rounded on its own in fp32,
 *   m = the tile's value after jspsr_scene_finish's expressions (clamp, de-scale, + base) with metres != 0 -- K12's order,
 *   conversion first and feathering in metres -- and the value widened to fp32 otherwise.  A tile whose weight at a pixel
 *   is zero is NOT read: a NaN in a trimmed margin does not reach the output.  A gather without atomics: every run gives
 *   the same bits.  On the reference's own covers (2 x 2, 3 x 3 of a square scene) with border 0: the bits of
 *   jspsr_scenes_assemble_f32.  16-byte stores when W % 4 == 0 and out is 16-byte aligned.
 *
 * Both: JSPSR_EINVAL on a null pointer, a non-positive size (B, S, kh, kw, ...), tiles that cannot cover the scene;
 * JSPSR_EALIGN on a pointer not aligned to its element size; both decided before any launch.  No host synchronisation. */
int jspsr_scene_prepare_windows(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                                int B, int kh, int kw, int flags, double elev_min, double elev_max, int mask_div,
                                jspsr_stream_t stream);
int jspsr_scene_merge_windows(int dtype, const void* tiles, const float* wy, const float* wx, const int* lo_y, const int* lo_x,
                              const int* oy, const int* ox, const int* samples, float* out, int S, int n_y, int n_x, int kh,
                              int kw, int H, int W, int metres, int elev_log, double elev_min, double elev_max,
                              jspsr_stream_t stream);

/* ---- K16 (ABI v25, additive): the self-ensemble per window of a tiled scene (csrc/scene_prepare.hip) ----------
 * jspsr_scene_prepare_windows_d4: jspsr_scene_prepare_windows composed with K14's D4 map, a window and a code per sample.
 *   What it replaces is jspsr_scene_prepare_windows followed by a flip / rot90 of every input tensor of every sample.
 *   samples device int32 [B][5] = {scene, base elevation (fp32 bit pattern), y0, x0, code}, code = rot90 * 4 + flip_lr * 2 +
 *     flip_ud as for jspsr_scene_prepare_d4;
 *   codes   HOST int32 [B], the same codes: every rot90 of a launch has one parity (JSPSR_EINVAL otherwise), so that one
 *     output shape serves it -- (B, cpitch, kh, kw) for an even rot90, (B, cpitch, kw, kh) for an odd one.
 *   out[b][c][i][j] = ToTensor_kind(scene[y0 + sy][x0 + sx][c]) with (sy, sx) the pixel of the kh x kw window that the
 *   element flipud?(fliplr?(rot90(window, rot90))) puts at (i, j): the bits of jspsr_scene_prepare_windows' output moved
 *   by the transform.  The base, H and W are the scene's own, so coord holds the local coordinates of the SOURCE pixel over
 *   the whole scene; a source pixel outside its scene is NaN, and so is every pixel of a sample whose scene index or store
 *   extent is bad or whose device code is outside 0..15 or of the other parity.  The windows of a launch may come from any
 *   scenes and shapes of the store.  Element offsets are 64-bit.
 *   Even rot90: jspsr_scene_prepare_windows' streaming kernel with rows and columns walked forwards or backwards.  Odd
 *   rot90: 32 x 32 output tiles, the pre-image staged in LDS (an output row walks a source column); B <= 65535.
 *   16-byte stores when the output row length (kw even, kh odd) is a multiple of 4 and out[kind] is 16-byte aligned;
 *   otherwise any 4-byte aligned output.
 *   JSPSR_EINVAL: a null pointer, B <= 0 or > 65535, kh <= 0, kw <= 0, a code outside 0..15, two parities, an hr_dem
 *   output, bad channel counts, both image ranges; JSPSR_EALIGN: a pointer not aligned to its element size; all decided
 *   before any launch.  No host synchronisation.
 * The mean of a window's predictions is jspsr_scene_finish_mean with the tile as its scene (H = kh, W = kw, metres = 0), and
 * the merge jspsr_scene_merge_windows on those fp32 tiles: no further entry point. */
int jspsr_scene_prepare_windows_d4(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                   const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                                   const int* codes, int B, int kh, int kw, int flags, double elev_min, double elev_max,
                                   int mask_div, jspsr_stream_t stream);

/* ---- K17 (ABI v25, additive): voids in whole-scene inference (csrc/scene_voids.hip) --------------------------
 * Real DEM tiles have voids (sea, data gaps, no-data values).  What these entries replace is a Euclidean feature transform
 * and a gather on the host, a second upload of the store, and a numpy np.where over the results.
 *
 * jspsr_scene_nearest_seed: for every pixel of every scene of a store, the nearest seed pixel of the SAME scene.
 *   seed    device uint8 [pixels], flat, the scenes back to back in the store's pixel layout; non-zero = seed;
 *   scenes  device int64 [n_scenes][3] = {pixel offset, H, W} (the store's scene table); scenes_host the same on the HOST
 *     (the sizes are checked and the grids sized from it before any launch);
 *   limit   0 = none, else a pixel whose nearest seed is farther than `limit` pixels (d2 > limit^2) finds none;
 *   src, d2 device int32 [pixels]: src = y_s * W + x_s of the seed inside its scene, d2 = dy^2 + dx^2; a seed pixel has
 *     src = itself and d2 = 0; both are -1 where the scene has no seed or none within the limit.
 *   The rule: among the seeds of the scene the one that minimises (dy^2 + dx^2, |dx|, dx, dy) lexicographically, d = seed -
 *   query.  Exact, integer, the same bits on every run.  Sides are at most 32767 (d2 < 2^31): a larger one is JSPSR_EINVAL,
 *   not a launch.  A search never crosses a scene boundary.  On the device every scene is checked against `pixels` again; one
 *   that does not fit is skipped.
 *   Phase 1, per column: the vertical distance to the column's nearest seed, ties to the upper one, int16, in `workspace`
 *   (jspsr_scene_nearest_seed_workspace_bytes, 2 B per pixel, 2-byte aligned); the columns are cut into bands of 64 rows,
 *   a thread per (band, column), so that a tall narrow scene fills the chip.  Phase 2, per row: the row's column distances
 *   staged in LDS; every pixel walks outwards x, x-1, x+1, x-2, ... over k^2 + g^2, strict improvements only, until
 *   k^2 >= best or k > limit.  Cost O(distance to the nearest seed) per query.  Three kernels, one call; src and d2 double
 *   as scratch between them.
 * jspsr_scene_fill_voids: in place on the fp32 lr_dem store, dem[p] = void[p] ? (src[p] >= 0 ? dem[scene offset + src[p]] :
 *   base[scene]) : dem[p].  src as jspsr_scene_nearest_seed gives it for seed = not void (NULL: every void gets the base);
 *   base device fp32 [n_scenes].  A source that is itself a void, or outside its scene, counts as none: no value is both
 *   read and written.
 * jspsr_scene_mask_out: rows device int64 [n_rows][3] = {offset into out, offset into void_out, pixels};
 *   out[row offset + i] = nodata where void_out[plane offset + i] is set, i < pixels; out has out_len elements and void_out
 *   `pixels` bytes, a row that leaves either is skipped.  One launch for all scenes of a predict_scenes call.
 * All: JSPSR_EINVAL on a null pointer, a non-positive size, a negative limit, a scene outside the plane; JSPSR_EALIGN on a
 * pointer not aligned to its element size; decided before any launch.  No host synchronisation. */
size_t jspsr_scene_nearest_seed_workspace_bytes(long long pixels);
int jspsr_scene_nearest_seed(const unsigned char* seed, long long pixels, const long long* scenes, const long long* scenes_host,
                             int n_scenes, int limit, int* src, int* d2, void* workspace, jspsr_stream_t stream);
int jspsr_scene_fill_voids(float* dem, const unsigned char* void_plane, const int* src, long long pixels,
                           const long long* scenes, int n_scenes, const float* base, jspsr_stream_t stream);
int jspsr_scene_mask_out(float* out, long long out_len, const unsigned char* void_out, long long pixels,
                         const long long* rows, int n_rows, float nodata, jspsr_stream_t stream);

/* ---- K18 (ABI v25, additive): pooled scores over valid pixels -- the masked form of K12(b) (csrc/summary.hip)
 * A K17 result carries the no-data value where the input had voids, and a real ground truth has holes of its own: one
 * such pixel wrecks RMSE, LE95 and PSNR of a whole table.  What this entry replaces is a device-to-host copy of every raster,
 * boolean indexing and np.median / np.percentile on the host.
 *
 * jspsr_summary_valid_forward: jspsr_summary_forward over the elements a validity plane keeps.  Arguments as K12's, plus
 *   valid   device uint8 [valid_numel] in the GROUND TRUTH's layout: read at the gt offset and pitch of every window;
 *     valid_numel must equal gt_numel.  A pixel counts iff its byte is non-zero.  One plane serves all candidates: every
 *     row of a table is scored over the same pixels.
 *   counts  device int64 [n_segments]: the number n_v of valid elements of every segment.
 *   segments: K12's table; words 3..7 (ranks and weight) are IGNORED.  n stays the segment's element count before masking
 *     and still fixes the chunking, total and total_chunks.
 *   With a mask n_v is data on the device, so the ranks, the weight and the divisor are formed there, by the first scan:
 *     n_v = the sum of the chunks' counts (exact, integer); median ranks (n_v - 1) / 2 and n_v / 2; v = 0.95 (n_v - 1) in
 *     double, l = floor(v), LE95 ranks l and min(l + 1, n_v - 1), g = v - l (no contraction: -ffp-contract=off); RMSE =
 *     sqrt(sum / n_v).  One __host__ __device__ inline forms them; jspsr_summary_ranks is its host twin, and the bits are
 *     those of jspsr_amd/summary.py: segment_ranks(n_v).
 *   A masked element's candidate and ground-truth values have no influence whatever they are (NaN, inf, -32767, 1e30): it
 *     is left out of the fp64 sum and of every histogram.  An element that is valid and NaN makes the row's five scores
 *     NaN, as in K12.  An element no window covers, or read outside a buffer, counts as valid and is NaN, as in K12.
 *   A segment with n_v = 0: all 11 columns NaN, counts = 0; not an error (the host cannot know).
 *   Departure from K12: none in the arithmetic.  A workgroup still owns one chunk of one segment and masked elements add
 *     nothing, so a call with an all-ones plane has exactly the bits of jspsr_summary_forward, all 11 columns.
 *   16 launches whatever the windows, segments, candidates and mask are (census labels summary_valid_prepare /
 *   summary_valid_select; K12's labels do not move); a row has the same bits for every n_cand, whatever other segments the
 *   call holds, on every run.  No host synchronisation.
 *   JSPSR_EINVAL: K12's cases, a null valid or counts, valid_numel != gt_numel.  workspace:
 *   jspsr_summary_valid_workspace_bytes(...) bytes (K12's plus one byte per pooled element and four per chunk; 0 = bad
 *   arguments), 16-byte aligned (JSPSR_EALIGN); counts 8-byte aligned.
 * jspsr_summary_ranks: out5 (HOST) = { (n - 1) / 2, n / 2, l, min(l + 1, n - 1), the bits of the double g }; JSPSR_EINVAL
 *   for n < 1 or a null out5.  No device is touched. */
size_t jspsr_summary_valid_workspace_bytes(int n_cand, int n_segments, long long total, long long total_chunks);
int jspsr_summary_valid_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                                long long gt_numel, const unsigned char* valid, long long valid_numel,
                                const long long* windows, int n_windows, const long long* segments, int n_segments,
                                long long total, long long total_chunks, double value_max, float* out, long long* counts,
                                void* workspace, jspsr_stream_t stream);
int jspsr_summary_ranks(long long n, long long* out5);

/* ---- K20 (ABI v25, additive): per-tile scores over valid pixels -- the masked form of K10 (csrc/scores.hip)
 * A ground truth with voids (K19's stores) makes K10's per-tile scores useless: one -32767 in a 64 x 64 tile is an RMSE of
 * about 500 m, the ranks are taken over the wrong n, and a void beside terrain is the largest Sobel edge of the tile.
 *
 * jspsr_scores_batch_valid_forward: jspsr_scores_batch_forward over the pixels a validity plane keeps.  Arguments as K10's, plus
 *   valid   device uint8 [B][H][W], cropped by the same int(H * border) / int(W * border) as the rasters.  A pixel counts
 *     iff its byte is non-zero.  pred and gt at a masked pixel have no influence whatever they hold (NaN, inf, -32767,
 *     1e30): they are read behind a select only and never multiplied by the mask.
 *   counts  device int32 [B][3] = {N, N_sl, N_sk}, exact: the valid pixels of the crop; the interior positions (1 <= y <
 *     h - 1, 1 <= x < w - 1) whose nine taps are all valid; the positions whose nine replicate-clamped taps (clamped to the
 *     crop) are all valid -- K19's rule for the Grad loss, so a void never makes an edge.
 *   Columns 0, 1, 2: sums over the valid pixels, divisor N; PSNR "local" is 100 where the masked mse is 0 and N > 0.
 *   Columns 3, 4, 5: exact selections over the valid differences, K10's ranks of N ((N - 1) / 2; llrint(0.95 (N - 1))) formed
 *     on the device; the NMAD centre is the masked median.  Column 6: the N_sl counted positions, divisor N_sl.  Column 7:
 *     the N_sk counted positions, divisor 2 N_sk.
 *   A column whose count is 0 is NaN (all eight when N = 0; the slope columns when their own count is 0); not an error,
 *     and no rank is formed from a zero count.
 *   Departure from K10: none in the arithmetic.  The sums fold in K10's order with masked elements adding nothing in place,
 *     and the path is chosen from the cropped size alone, so a call with an all-ones plane has exactly the bits of
 *     jspsr_scores_batch_forward, all eight columns.  The mask travels inside the de-scaled prediction (a NaN there; a counted
 *     pixel's is finite after the clamp), so the LDS path still holds 142 x 142.
 *   One launch (LDS path) or 27 (streaming path) whatever B and the mask are (census labels scores_batch_valid (lds) /
 *   scores_batch_valid (stream); K10's labels do not move).  Row b does not depend on B, on the other tiles or on their masks;
 *   the same bits on every run.  No host synchronisation.
 *   JSPSR_EINVAL: K10's cases, a null valid or counts.  workspace: jspsr_scores_batch_valid_workspace_bytes(B, H, W) bytes
 *   (K10's plus 16 per streaming block; 0 = bad arguments), 16-byte aligned (JSPSR_EALIGN); counts 4-byte aligned. */
size_t jspsr_scores_batch_valid_workspace_bytes(int B, int H, int W);
int jspsr_scores_batch_valid_forward(const float* pred, const float* gt, const unsigned char* valid, int B, int H, int W,
                                     float border, float value_min, float value_max, int elev_log, float* scores,
                                     int* counts, void* workspace, jspsr_stream_t stream);

/* ---- K21 (ABI v25, additive): the whole-set error distribution -- float16 histogram and Gaussian KDE (csrc/errdist.hip;
 * DESIGN.md).  The numbers behind the reference's figure "Elevation Error Distribution in [-5, 5] m" (summarise_evaluation,
 * utils/utils.py:1394-1456): per candidate the pooled errors with lo <= e <= hi, stored as float16, drawn by
 * sns.kdeplot(bw_adjust=1, cut=0.5, common_norm=False).  What these entries replace is a device-to-host copy of every
 * raster, boolean indexing and a KDE over 10^8 points on the host.  seaborn was not available to pin against: the curve is
 * pinned to scipy.stats.gaussian_kde (scotts_factor, set_bandwidth(factor * bw_adjust)) and to the rules written here, which
 * are seaborn 0.12's _define_support_grid with clip=None and numpy's linspace.
 *
 * jspsr_errdist_bins (HOST, no device is touched): *key0 = key(f16(float32(lo))), *K = key(f16(float32(hi))) - key0 + 1, with
 *   f16 = round to nearest, ties to even, subnormals produced (np.float32(x).astype(np.float16), formed in integer arithmetic by
 *   one __host__ __device__ function: the wave's FP16 denormal mode cannot matter) and key(bits) = bits ^ (bits & 0x8000 ?
 *   0xffff : 0x8000), the order-preserving key.  Bin b holds the float16 of key key0 + b; -0 and +0 are two neighbouring
 *   bins of value 0.  (-5, 5): K = 35 330.  JSPSR_EINVAL unless lo <= hi, both finite, both magnitudes <= 65504.
 * jspsr_errdist_key (HOST twin of the kernel's classification): the bin of an error e, or -1 below the range, -2 above it,
 *   -3 for a NaN; -4 for a bad range.  In range iff e >= float32(lo) && e <= float32(hi): NaN fails, -inf is below, +inf above.
 *   With lo = +0 the element -0 is in range although its key is key0 - 1: it is counted in bin 0 (the same value, 0).
 * jspsr_errdist_hist_forward: cands / cand_numel / gt / gt_numel / windows / n_windows / total as K12's; the windows'
 *   segment word is NOT read, everything the call is given is one pool.  valid: K18's plane (device uint8 [valid_numel] in the
 *   ground truth's layout, valid_numel == gt_numel) or NULL for "no mask".
 *   Per pooled element and candidate: e = cand - gt in fp32, one rounded subtraction, as K12.  With a plane an element whose
 *     byte is 0 is not scored and influences nothing whatever the rasters hold there (read behind a select).  A scored
 *     element in range increments bin key(f16(e)) - key0.  Departure from K12's rows: a NaN or an infinity poisons nothing
 *     here, it is counted and left out, as the reference's comparison leaves it out.  An element no window covers, or read
 *     outside a buffer, is scored and is a NaN.
 *   hist    device int64 [n_cand][K], exact.
 *   counts  device int64 [n_cand][4] = { n_scored, n_in, n_below, n_above }; n_scored is equal for all candidates and
 *     n_scored - n_in - n_below - n_above is the number of NaNs.
 *   Two clears and ONE launch whatever the sizes, the candidates and the range are (census labels errdist_hist /
 *   errdist_hist (valid)); a range of more bins than one LDS image of 36 864 holds is walked twice inside that launch.
 *   Integer adds only: a candidate's histogram does not depend on the other candidates of the call, nor on the run.  No host
 *   synchronisation, no workspace.  Departures from the arithmetic above: none intended.
 *   JSPSR_EINVAL: a null pointer, n_cand outside 1..8, an empty table, a bad range, total >= 2^32, valid_numel != gt_numel;
 *   JSPSR_EALIGN: rasters not 4-byte, hist / counts not 8-byte aligned.
 * jspsr_errdist_kde_forward: the curves of n_cand histograms hist [n_cand][K] of bins key0 .. key0 + K - 1, all in fp64:
 *   n = sum c_b, v_b the value of bin b; mean = sum c_b v_b / n; var = sum c_b (v_b - mean)^2 / (n - 1); bw = sqrt(var) *
 *   n^(-1/5) * bw_adjust; with vmin, vmax the values of the lowest and highest occupied bins, support = linspace(vmin - cut bw,
 *   vmax + cut bw, gridsize) by numpy's rule (start + i * step, two roundings; the last point is stop exactly); density_j = sum
 *   c_b exp(-(g_j - v_b)^2 / (2 bw^2)) / (n bw sqrt(2 pi)).  Every sum is folded per thread over bins t, t + 256, ... and then by
 *   a fixed tree: the bits depend on K and the counts alone.  n < 2 or var == 0: support and density are NaN (seaborn draws
 *   nothing there); std and bw are NaN for n < 2, mean for n = 0.
 *   support, density  device fp64 [n_cand][gridsize];  stats  device fp64 [n_cand][3] = { mean, std, bw }.
 *   Two launches (census label errdist_kde), no host synchronisation.  JSPSR_EINVAL: a null pointer, n_cand outside 1..8, bins
 *   that are not finite float16 values, gridsize outside 2..65535, cut < 0, bw_adjust <= 0.  workspace:
 *   jspsr_errdist_workspace_bytes(n_cand, gridsize) bytes (0 = n_cand or gridsize outside the bounds above), 16-byte aligned
 *   (JSPSR_EALIGN). */
int jspsr_errdist_bins(double lo, double hi, int* key0, int* K);
int jspsr_errdist_key(float e, double lo, double hi);
size_t jspsr_errdist_workspace_bytes(int n_cand, int gridsize);
int jspsr_errdist_hist_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                               long long gt_numel, const unsigned char* valid, long long valid_numel,
                               const long long* windows, int n_windows, long long total, double lo, double hi,
                               long long* hist, long long* counts, jspsr_stream_t stream);
int jspsr_errdist_kde_forward(const long long* hist, int n_cand, int key0, int K, int gridsize, double cut, double bw_adjust,
                              double* support, double* density, double* stats, void* workspace, jspsr_stream_t stream);

/* ---- K22 (ABI v25, additive): whole-set scores by terrain class -- the stratified pooled table (csrc/strata.hip)
 * Every DEM accuracy assessment reports its scores per land-cover class and per slope class.  What these entries replace is
 * one jspsr_summary_valid_forward call per class (16 launches and a full read of every candidate each), or a device-to-host
 * copy of every raster, boolean indexing and numpy.  The version stays 25: the entries are additive, as K16..K21 were.
 *
 * jspsr_strata_forward: K12's eleven-column row for every candidate and every class of a label plane, from ONE pool.
 *   cands / cand_numel / n_cand / gt / gt_numel / windows / n_windows / total as K21's jspsr_errdist_hist_forward: the
 *     windows' segment word is NOT read, everything the call is given is one pool; total = the sum of h * w < 2^32.
 *   labels  device uint8 [labels_numel] in the GROUND TRUTH's layout, read at the gt offset and pitch of every window, as
 *     K18 reads valid; labels_numel must equal gt_numel.
 *   n_classes  1..32.
 *   valid   K18's plane (device uint8 [valid_numel], valid_numel == gt_numel) or NULL.
 *   A pooled element i belongs to class c = labels[i] iff c < n_classes and (valid is NULL or valid[i] != 0).  Every other
 *     element influences nothing whatever the rasters hold there (NaN, inf, -32767, 1e30): it is read behind a select only
 *     and never multiplied by a mask.  One label plane serves all candidates: every row is scored over the same elements.
 *   out     device fp32 [n_cand][n_classes][11], K12's columns.  counts  device int64 [n_classes].
 *   Per class the definitions are K12's and K18's: e = cand - gt, one rounded subtraction; the six bracketing order
 *     statistics are exact elements of e, |e - Median| and |e|; the ranks and the LE95 weight come from the class count n_c
 *     through the __host__ __device__ inline K18 uses (host twin: jspsr_summary_ranks), formed on the device; Median = (lo +
 *     hi) * 0.5f; NMAD and LE95 by K12's expressions; RMSE = sqrt(sum / n_c) with the squares summed in fp64 per fixed run of
 *     8192 pooled elements (per thread in element order, then K18's fold of a chunk), the runs folded in K12's order and
 *     the result rounded once; PSNR formed in double.  n_c is the sum of the class's top-digit histogram, exact.
 *   A class without an element: all 11 columns NaN, count 0; not an error.  A counted NaN makes that class's five scores
 *     NaN for that candidate and touches no other class or candidate.  An element no window covers, or read outside a
 *     buffer, is a NaN of class 0 (K12 counts it too).
 *   Every pass over the pool serves all classes: per-class digit histograms in LDS (n_classes x 256 counters per key kind
 *     and state), integer adds only, hot counters by ballot-aggregated increments.  16 launches whatever n_classes, n_cand,
 *     the windows and the data are (census labels strata_prepare / strata_select); a row has the same bits for every n_cand,
 *     whatever the other classes hold, on every run.  No host synchronisation.  A workgroup's LDS grows with n_classes, up to
 *     128 KiB at 32.
 *   JSPSR_EINVAL: a null pointer, n_cand outside 1..8, n_classes outside 1..32, an empty table, total >= 2^32, labels_numel or
 *     valid_numel != gt_numel.  workspace: jspsr_strata_workspace_bytes(n_cand, n_classes, total) bytes (0 = bad arguments),
 *     16-byte aligned (JSPSR_EALIGN); rasters and out 4-byte, counts 8-byte aligned.
 * jspsr_slope_classes: a slope-class label plane from metre rasters in store layout, ONE launch (census label slope_classes).
 *   z       device fp32 [pixels], the scenes back to back;  scenes  device int64 [n_scenes][3] = {offset, h, w}, offsets
 *     ascending; a pixel no scene holds, or of a scene that leaves the plane, gets 255.
 *   thresholds  HOST fp32 [n_thr], n_thr <= 31, >= 0 and ascending: t_k = float32((8 cell tan(edge_k pi / 180))^2), formed by
 *     the caller in double and rounded once, so the device never evaluates atan.
 *   valid   device uint8 [valid_numel] (valid_numel == pixels) or NULL;  out  device uint8 [pixels].
 *   The 3 x 3 taps a b c / d e f / g h i (a b c the row above) are replicate-clamped inside their own scene.  In fp32, every
 *     operation rounded once, in exactly this order: gx = ((c + 2f) + i) - ((a + 2d) + g); gy = ((g + 2h) + i) - ((a + 2b) +
 *     c); p = gx*gx + gy*gy.  label = the number of thresholds t_k <= p; 255 where any of the nine clamped taps is invalid
 *     (valid given and 0 there: K19's rule) or p is NaN.  A numpy float32 restatement reproduces every label bit for bit.
 *   JSPSR_EINVAL: a null pointer, an empty plane, n_thr outside 0..31, thresholds negative, NaN or descending, valid_numel
 *     != pixels; JSPSR_EALIGN: z not 4-byte aligned.  No host synchronisation, no workspace. */
size_t jspsr_strata_workspace_bytes(int n_cand, int n_classes, long long total);
int jspsr_strata_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                         long long gt_numel, const unsigned char* labels, long long labels_numel, int n_classes,
                         const unsigned char* valid, long long valid_numel, const long long* windows, int n_windows,
                         long long total, double value_max, float* out, long long* counts, void* workspace,
                         jspsr_stream_t stream);
int jspsr_slope_classes(const float* z, long long pixels, const long long* scenes, int n_scenes, const float* thresholds,
                        int n_thr, const unsigned char* valid, long long valid_numel, unsigned char* out,
                        jspsr_stream_t stream);

/* ---- K25 (ABI v25, additive): single-channel fp32 rasters resampled to a finer grid -- F.interpolate with size=, mode
 * "bicubic" or "bilinear" and align_corners=False, for a list of rasters of different shapes in one launch
 * (csrc/resample.hip).  Upsampling only.  No workspace.
 * jspsr_resample_axis: plain host code, no GPU.  The taps of one axis, output length H over a source of h: first HOST int32
 *   [H], weights HOST fp32 [H][4].  In integers n = (2Y + 1) h - H, d = 2H, i = floor(n / d), r = n - i d; t = r / d in double.
 *   JSPSR_RESAMPLE_BICUBIC (A = -0.75): first = i - 1, weights = { c2 at t + 1, c1 at t, c1 at 1 - t, c2 at 2 - t } with
 *     c1 x = ((A + 2) x - (A + 3)) x^2 + 1 and c2 x = ((A x - 5A) x + 8A) x - 4A, evaluated in double, each rounded to fp32 once.
 *   JSPSR_RESAMPLE_BILINEAR: n < 0 counts as 0 (i = 0, t = 0); first = i, weights = { 1 - t, t, 0, 0 } from double.
 *   Tap k of output Y is the source index first[Y] + k clamped to [0, h - 1]; H == h gives weights { 0, 1, 0, 0 } and
 *     { 1, 0, 0, 0 }.
 *   JSPSR_EINVAL: a null pointer, another mode, h < 1, H < h (downsampling needs a prefilter and is not built).
 * jspsr_resample_forward: ONE launch, no host synchronisation.
 *   src     device fp32 [src_numel];  dst  device fp32 [dst_numel];  n rasters, 1..65535
 *   table   device int64 [n][8] = { src_off, h, w, dst_off, H, W, ytaps_off, xtaps_off } and host_table, the same rows on
 *     the HOST: every row is checked there against src_numel, dst_numel and n_taps before the launch (H >= h, W >= w).
 *   first / weights  device int32 [n_taps] / fp32 [n_taps][4]: the axis tables of the call back to back, a raster's rows at
 *     ytaps_off, its columns at xtaps_off, made by jspsr_resample_axis for `mode`.  Source indices are clamped in the
 *     kernel, so a table that does not belong to the shapes gives wrong values and no access outside the buffers.
 *   clamp   device fp32 [n][2] = { lo, hi } per raster, or NULL
 *   src_void / dst_void  device uint8 [src_numel] / [dst_numel], both or neither: dst_void of an output pixel = src_void of
 *     the source pixel (iy, ix) clamped to the raster, i the index above.
 *   In fp32, every operation rounded once, no fused multiply-add, in exactly this order (bicubic; bilinear: two taps per
 *     axis, the first one the centre): c = v[iy][ix], indices clamped; r_k = ((wx0 (v_k0 - c) + wx1 (v_k1 - c)) + wx2 (v_k2 -
 *     c)) + wx3 (v_k3 - c); s = ((wy0 r_0 + wy1 r_1) + wy2 r_2) + wy3 r_3; out = s + c; with a clamp out < lo ? lo : (out > hi
 *     ? hi : out), which keeps a NaN.  A numpy float32 restatement reproduces every bit, whatever rasters share the call.
 *   JSPSR_EINVAL: a null pointer, another mode, n outside 1..65535, one void plane without the other, a row that
 *     downsamples or leaves a buffer; JSPSR_EALIGN: a tensor not 4-byte, the table not 8-byte, weights not 16-byte aligned. */
#define JSPSR_RESAMPLE_BICUBIC 0
#define JSPSR_RESAMPLE_BILINEAR 1
int jspsr_resample_axis(int h, int H, int mode, int* first, float* weights);
int jspsr_resample_forward(const float* src, long long src_numel, float* dst, long long dst_numel, const long long* table,
                           const long long* host_table, int n, const int* first, const float* weights, long long n_taps,
                           int mode, const float* clamp, const unsigned char* src_void, unsigned char* dst_void,
                           jspsr_stream_t stream);

/* ---- K26 (ABI v25, additive): HWC uint8 rasters brought to a coarser grid by their exact area mean -- image, mask and
 * canopy held finer than their scene -- for a list of rasters of different shapes and one channel count in one launch
 * (csrc/area.hip).  Downsampling (and the identity) only, any ratio >= 1 per axis.  No workspace.
 * The rule of one axis, output length H over a source of h, 1 <= H <= h <= 65535: the weight of source pixel i under output Y
 *   is the overlap a(Y, i) = min((Y + 1) h, (i + 1) H) - max(Y h, i H) where positive; taps i0 = floor(Y h / H) ..
 *   floor(((Y + 1) h - 1) / H), at most ceil(h / H) + 1; sum_i a = h, sum_Y a = H.
 * jspsr_area_axis: plain host code, no GPU.  first / count HOST int32 [H]: the first source index and the number of taps
 *   of every output; weights HOST uint32 [H][ceil(h / H) + 1] or NULL: a(Y, first[Y] + k), zero past count[Y] -- from the
 *   inline the kernel evaluates.  JSPSR_EINVAL: a null first or count, h or H < 1, H > h (upsampling), h > 65535.
 * jspsr_area_forward: ONE launch, no host synchronisation, integer accumulators.
 *   src     device uint8 [src_numel][channels];  dst  device uint8 [dst_numel][channels] (numel in PIXELS);  channels 1..16
 *   table   device int64 [n][6] = { src_off, h, w, dst_off, H, W }, offsets in pixels, and host_table, the same rows on the
 *     HOST: every row is checked there before the launch.  n rasters, 1..65535.
 *   With S = sum_y sum_x a_y a_x v per channel and D = h w:
 *   JSPSR_AREA_MEAN      out = floor((S + floor(D / 2)) / D), exactly (round half up); H == h and W == w copies the raster.
 *   JSPSR_AREA_MAJORITY  a non-zero byte counts as 1; none = D - sum_c S_c (signed); c* = the lowest index among the
 *     channels of largest S_c; the output pixel is one-hot (a byte 1) at c* iff S_c* > 0 and S_c* >= none, else all zeros.
 *   Every raster's bytes are those of the raster alone, on every run.
 *   JSPSR_EINVAL: a null pointer, another mode, channels outside 1..16, n outside 1..65535, a row with an empty side, one
 *     that upsamples (H > h or W > w), a source side above 65535 (the weight products are 32-bit, S + D / 2 < 2^40) or one
 *     that leaves src or dst; JSPSR_EALIGN: the table not 8-byte aligned.  src and dst need no alignment. */
#define JSPSR_AREA_MEAN 0
#define JSPSR_AREA_MAJORITY 1
int jspsr_area_axis(int h, int H, int* first, int* count, unsigned* weights);
int jspsr_area_forward(const unsigned char* src, long long src_numel, unsigned char* dst, long long dst_numel,
                       const long long* table, const long long* host_table, int n, int channels, int mode,
                       jspsr_stream_t stream);

/* One AdamW step (torch.optim.AdamW semantics: decoupled weight decay, bias correction) over a flat
 * fp32 parameter / gradient / moment buffer of n elements (utils/common_config.py:241-291).  The four pointers are
 * 4-byte aligned and share one offset from a 16-byte boundary (sub-ranges of four identically laid out buffers). */
int jspsr_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, jspsr_stream_t stream);
/* The same step with its scalars in DEVICE memory, for launches captured in a hipGraph (jspsr_amd/graph.py): hyper[7] =
 * { lr, beta1, beta2, eps, weight_decay, 1 - beta1^step, sqrt(1 - beta2^step) } (the bias corrections computed by the caller
 * in double, as torch.optim.AdamW does), refreshed by the caller before every replay. */
int jspsr_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                         const float* hyper, jspsr_stream_t stream);

/* K11 (ABI v20): the rest of the reference's optimizer menu over the same flat buffers (utils/common_config.py:241-291 builds
 * torch.optim.SGD / Adam / AdamW / RMSprop; their per-tensor step loops are what this replaces), torch's semantics at its
 * defaults, with the gradient range of the training monitor (train/train_utils.py:127-143, get_gradient_range) fused in.
 *   kind            state1              state2                   a         b
 *   JSPSR_OPT_SGD      momentum_buffer | NULL  NULL                     momentum  -       dampening 0, no Nesterov, coupled decay;
 *                                                                                      step == 1: the buffer becomes the gradient
 *   JSPSR_OPT_ADAM     exp_avg             exp_avg_sq               beta1     beta2   coupled L2 (g += wd * p before the moments)
 *   JSPSR_OPT_ADAMW    exp_avg             exp_avg_sq               beta1     beta2   jspsr_adamw_step's arithmetic, bit for bit
 *   JSPSR_OPT_RMSPROP  square_avg          momentum_buffer | NULL   momentum  alpha   eps outside the root, not centered, coupled
 * A NULL momentum buffer selects the update without momentum.  Pointers as for jspsr_adamw_step.  `step` >= 1 feeds Adam's
 * bias corrections (computed here in double) and SGD's first step.
 * hyper != NULL: the scalars come from DEVICE memory instead (launches captured in a hipGraph), hyper[7] = { lr, a, b, eps,
 * weight_decay, c1, c2 } with c1 = 1 - beta1^step, c2 = sqrt(1 - beta2^step) for Adam / AdamW (jspsr_adamw_step_dev's row)
 * and c1 = 1 on SGD's first step, else 0; lr .. step are then ignored.  Same arithmetic, same bits as the argument form.
 * grad_range != NULL (4 floats: min, max, count of non-finite elements, spare): the kernel also reduces the gradient it
 * has just read -- a wave reduction, per-workgroup partials in `workspace` (jspsr_optim_workspace_bytes(), 4-byte aligned),
 * one small last reduction -- and FOLDS the result into grad_range: min / max over the finite values, the count added.
 * Several ranges of one step combine in the same 4 floats; the caller resets them once per step (the reference starts
 * from 999 / -999).  The parameters do not depend on whether grad_range is given. */
#define JSPSR_OPT_SGD 0
#define JSPSR_OPT_ADAM 1
#define JSPSR_OPT_ADAMW 2
#define JSPSR_OPT_RMSPROP 3
size_t jspsr_optim_workspace_bytes(void);
int jspsr_optim_step(int kind, float* param, const float* grad, float* state1, float* state2, long long n, float lr, float a,
                     float b, float eps, float weight_decay, int step, const float* hyper, float* grad_range, void* workspace,
                     jspsr_stream_t stream);
/* min / max of up to 8 device tensors (JSPSR_F32 or JSPSR_BF16, contiguous, numel[k] elements) in one call: what
 * get_tensor_range (train/train_utils.py:84-96: torch.min + torch.max per tensor, read back with .item()) gives for
 * `monitor_value: input / pred`.  tensors / numel / dtypes are HOST arrays of `count` entries; table[k][4] on the device
 * receives { min, max, count of non-finite elements, 0 } of tensor k, min / max over its finite values.  workspace:
 * jspsr_tensor_ranges_workspace_bytes(), 4-byte aligned. */
size_t jspsr_tensor_ranges_workspace_bytes(void);
int jspsr_tensor_ranges(int count, const void* const* tensors, const long long* numel, const int* dtypes, float* table,
                        void* workspace, jspsr_stream_t stream);

/* The MLP between gate_pool and gate_scale (resnet_cbam.py:41-53: two bias-free 1x1 convs C -> Ch -> C shared by the
 * average- and the max-pooled vector, ReLU between, Sigmoid of the sum): s[b,c] = sigmoid(W2 relu(W1 avg[b]) + W2 relu(W1
 * mx[b])).  w1 (Ch, C), w2 (C, Ch) fp32 row-major; hid (B, 2, Ch) receives the two hidden vectors for the backward pass.
 * Backward: from ds (B, C) the gradients of avg, mx (B, C) and of the two weights (summed over the batch in image order);
 * workspace of jspsr_gate_mlp_backward_workspace_bytes: dz (B, C) then dh (B, 2, Ch), fp32, 4-byte aligned (every access
 * is one float).  Needs (C + 2 Ch) * 4 bytes <= 64 KiB: above it the entry is JSPSR_EINVAL and the query returns 0, as it
 * does for a non-positive size. */
int jspsr_gate_mlp_forward(const float* avg, const float* mx, const float* w1, const float* w2, int B, int C, int Ch,
                           float* s, float* hid, jspsr_stream_t stream);
size_t jspsr_gate_mlp_backward_workspace_bytes(int B, int C, int Ch);
int jspsr_gate_mlp_backward(const float* ds, const float* s, const float* hid, const float* avg, const float* mx,
                            const float* w1, const float* w2, int B, int C, int Ch, float* davg, float* dmax, float* dw1,
                            float* dw2, void* workspace, jspsr_stream_t stream);
/* The two calls above run chip-wide kernels (a wave per hidden unit, a thread per channel).  The earlier kernels -- one
 * workgroup per image, the same sums in the same order, the same bits -- stay behind this switch for comparison:
 * on = 1 / 0 selects them / the wide ones, on < 0 only asks; returns the previous setting.  Initial value: the
 * environment's JSPSR_GATE_MLP_LEGACY (default 0). */
int jspsr_gate_mlp_legacy(int on);

/* The models' first step with every input (the reference hands them contiguous planar fp32 tensors, utils/utils.py:156-179;
 * models/JSPSR.py:208-222 then feeds the stems): src (B,C,H,W) fp32 -> dst (B,H,W,c_pad) in `dtype`, channels last and
 * zero-padded to c_pad (a multiple of 4 fp32 / 8 bf16 channels, >= C).  One pass; dst 16-byte aligned. */
int jspsr_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, int c_pad, jspsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JSPSR_HIP_H */
