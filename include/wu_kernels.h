/*
 * wu_kernels.h -- C ABI of libwu_kernels.so, the MI355X (gfx950) kernels behind the
 * conditional-U-Net hot path of Sota0726/weather-Unet.
 *
 * The reference has no native code: every entry point below replaces a torch.nn op that the
 * reference's Python modules call (file:line cited per function).  The reference-side binding
 * is the ctypes stub shown in INTEGRATION.md (weather-unet_amd/wu/_lib.py is that stub).
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless said otherwise.  The library never allocates,
 *     frees or synchronises: buffers and workspaces are owned by the caller and only borrowed
 *     for the duration of the launch; every call only enqueues work on `stream`
 *     (a hipStream_t passed as void*), so calls are graph-capturable and re-entrant.
 *   - Activations are NHWC ("channels-last"): element (n,h,w,c) of a tensor with pixel stride
 *     `ld` (in elements, >= C, multiple of 8) lives at ((n*H + h)*W + w)*ld + c.  A channel
 *     slice of a wider buffer is passed as (ptr + c0, ld = total channels); that is how the
 *     skip-concat (cunet.py:62,69,76) is done without a copy.
 *   - `dtype`: WU_F32 (0) = fp32 storage, exact-fp32 MFMA;  WU_BF16 (1) = bf16 storage,
 *     bf16 MFMA with fp32 accumulation.  Parameters, their gradients, statistics are fp32.
 *   - Network input / output images are NCHW fp32 (the reference's layout).
 *   - Return value: 0 on success, a hipError_t (>0) from the launch, or < 0 for a rejected
 *     argument (shape / alignment); wu_last_error() gives a host string for the last failure
 *     on the calling thread.
 */
#ifndef WU_KERNELS_H
#define WU_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WU_F32 0
#define WU_BF16 1

#define WU_ACT_NONE 0
#define WU_ACT_RELU 1   /* nets.py:21,23 nn.ReLU */
#define WU_ACT_LEAKY 2  /* nets.py:32 nn.LeakyReLU(0.2) */

const char* wu_last_error(void);
int wu_version(void);
/* Compute units of the current HIP device (256 on MI355X): the persistent conv / weight-gradient grids are sized from it. */
int wu_cu_count(void);
/* Kernel-variant switches for in-process A/B benchmarking -- DIAGNOSTIC / TEST-ONLY: process-global mutable state, not part of
 * the re-entrant launcher contract.  A production caller never touches it: the defaults ARE the production
 * choices and every variant computes identical results; set it only from a single-threaded benchmark harness, between launches.
 *   0: conv LDS-DMA path (0 off = generic template, 1 auto wave shape (default), 2 always 4 waves, 3 always 8 waves)
 *   1: persistent tile loop on/off      2: LDS-DMA wgrad (0 off, 1 = 8 waves (default), 2 = 4 waves)
 *   3: stride-1 bf16 convs on images at most 16 pixels wide on the small-image kernel (128-pixel tiles, in-workgroup K split, stacked images; default 1 = where the generic template's 256-pixel tiles
 *      would under-fill the chip or lie mostly outside the image, 2 = always, 0 = never)
 *   4: wgrad DMA issue spread over K-steps (default 1)   5: first conv (0 matrix cores in bf16 (default), 1 rows kernel, 2 VALU kernel)
 *   6: static priority for the younger wave half (default 1)   7: grid-strided tile assignment (default 1)
 *   8: AdaIN-upsample backward (0 = 16-tap gather, 1 = default: bf16 with keep bits streams through an LDS ring, everything else marches
 *      with the columns per thread chosen by size; 2 / 3 = marching with one / two columns, 5 = marching also where the ring kernel would run)
 *   9: marching AdaIN-upsample forward (default 1)
 *   10: persistent-grid size override in compute units (0 = the device's count; experiments on CU-masked streams)
 *   11: Cin = 64 / one-cout-tile convs keep both weight chunks resident in LDS across a workgroup's tiles (default 1)
 *   12: pointwise-GEMM pixel tile (0 = 64 rows (default), 1 = 256 rows, 2 = 128 rows)
 *   13: image-layout 3 -> 3 conv (SNDisc's first layer): 1 = LDS-tiled kernels (default), 0 = one thread per pixel
 *   14: stride-2 data gradient: 1 = four parity-class sparse-tap convs in one launch (default), 0 = zero-stuffed dY + stride-1 conv
 *   15: persistent LDS-DMA GEMM pipeline (round 4: pointwise convs with 128 x 128 / 128 x 64 tiles; stride-2 3x3 convs and the parity classes of
 *       their data gradient with gathered rows).  Bits 0-2 = ring depth D (0 = off: the register-staged kernels everywhere), bit 3 = eight waves
 *       per workgroup (else four), bit 4 = 64-cout tiles also for the 3x3 forms, bits 5.. = the least number of tiles that takes this path.
 *       Default 2 + 8 + (128 << 5): D = 2, eight waves, two workgroups per CU, from 128 tiles. */
int wu_set_option(int key, int value);
/* Diagnostic: device buffer of 256*8*8 uint64 receiving per-wave phase cycle sums of the persistent conv / wgrad kernels
 * (DMA wait, compute, whole-kernel s_memtime and s_memrealtime deltas -> in-kernel clock, barrier, epilogue, tiles, chunks);
 * NULL (default) disables stamping. */
int wu_set_debug_buffer(void* p);
/* Stream ordering inside one device without a system-scope fence (host plumbing of the fused backward, wu/unet_graph.py: the
 * weight-gradient hand-offs between its two streams).  wu_stream_order_after(waiter, producer, event): work enqueued on `waiter` after
 * the call runs after everything enqueued on `producer` before it; `event` (wu_event_create: no timing, hipEventDisableSystemFence) may
 * be reused for every call.  Nothing in the reference corresponds to this (autograd there runs on one stream). */
int wu_event_create(void** event_out);
int wu_event_destroy(void* event);
int wu_stream_order_after(void* waiter_stream, void* producer_stream, void* event);

/* Experiment support (DIAGNOSTIC): a HIP stream confined to the compute units whose bits are set in mask[0..words) (hipExtStreamCreateWithCUMask),
 * for measuring CU-partitioned overlap of the data-gradient and weight-gradient kernels (scratch/ab_cumask.py); unused by the product path. */
int wu_stream_create_cu_mask(const unsigned* mask, int words, void** stream_out);
int wu_stream_destroy(void* stream);

/* ---- weights -------------------------------------------------------------------------------
 * Repack one 3x3 conv weight (nets.py:20,22,28-31; OIHW fp32, the state-dict layout) into the two
 * MFMA operand layouts: w_fwd[tap][Cout][Cin] and w_dgrad[tap'][Cin][Cout] with tap' the
 * 180-degree-rotated tap (the data-gradient is a correlation with the flipped, transposed
 * filter).  `inv_sigma` (device scalar, may be NULL) multiplies every weight: the spectral-norm
 * division W/sigma of torch.nn.utils.spectral_norm (nets.py:27-31).  Either output may be NULL. */
int wu_pack_conv3x3(const float* w_oihw, void* w_fwd, void* w_dgrad, int Cout, int Cin,
                    const float* inv_sigma, int dtype, void* stream);
/* wu_pack_conv3x3 (no spectral-norm factor) for n <= 16 weights in one launch: entry i packs w_oihw[i] (Cout[i] x Cin[i] x 3 x 3)
 * into w_fwd[i] and w_dgrad[i].  The pointer / size arrays live in HOST memory and are consumed before the call returns. */
int wu_pack_conv3x3_multi(int n, const float* const* w_oihw, void* const* w_fwd, void* const* w_dgrad,
                          const int* Cout, const int* Cin, int dtype, void* stream);

/* Spectral normalisation of a conv weight (torch.nn.utils.spectral_norm around the convs of nets.py:28-31):
 * one power iteration (power_iter != 0: v <- normalize(W^T u), u <- normalize(W v), buffers updated in place),
 * sigma = u . (W v); sigma_out[0] = sigma, sigma_out[1] = 1/sigma; w_eff (may be NULL) = W / sigma.  W is the OIHW
 * fp32 weight viewed as rows = Cout, cols = Cin*9.  Backward: dw = g/sigma - (<g,w>/sigma^2) u v^T with u, v the
 * buffers the forward used (constants of the graph, as in torch).  scratch: wu_spectral_norm_scratch_floats(). */
size_t wu_spectral_norm_scratch_floats(int rows, int cols);
int wu_spectral_norm_fwd(const float* w, int rows, int cols, float* u, float* v, int power_iter, float eps,
                         float* sigma_out, float* w_eff, float* scratch, void* stream);
int wu_spectral_norm_bwd(const float* g, const float* w, const float* u, const float* v, const float* sigma,
                         float* dw, int rows, int cols, float* scratch, void* stream);
/* The same for n <= 16 weights per call -- all ten SN layers of SNDisc (disc.py:11-24: eight convs, `l`, `embed`) in 5 launches forward
 * and 2 backward instead of 5 n / 2 n.  Arrays of n entries in HOST memory (read during the call), entry i as in the single-weight
 * call; results are bit-identical to n single calls.  u_save / v_save (the arrays and their entries may be NULL): copies of the u, v
 * that define sigma_out[i], for the backward pass (the buffers advance on the next forward). */
int wu_spectral_norm_fwd_multi(int n, const float* const* w, const int* rows, const int* cols, float* const* u, float* const* v,
                               int power_iter, float eps, float* const* sigma_out, float* const* w_eff, float* const* scratch,
                               float* const* u_save, float* const* v_save, void* stream);
int wu_spectral_norm_bwd_multi(int n, const float* const* g, const float* const* w, const float* const* u, const float* const* v,
                               const float* const* sigma, float* const* dw, const int* rows, const int* cols, float* const* scratch,
                               void* stream);

/* ---- conv3x3, pad 1, MFMA implicit GEMM -----------------------------------------------------
 * y = act(conv3x3(x, w) + bias)   replaces nn.Conv2d(cin,cout,3,padding=1[,stride=2]) + ReLU /
 * LeakyReLU of nets.py:18-33.  x: (N,H,W,Cin) ld=ldx; y: (N,Ho,Wo,Cout) ld=ldy with
 * Ho = (H-1)/stride + 1.  Cin % (64/sizeof(T)) == 0, Cout % 64 == 0.  bias may be NULL.
 * If `mask` != NULL the staged input is gated by the activation derivative of `mask`
 * (same geometry as x, ld=ldmask):  x * (mask > 0 ? 1 : slope(mask_act)) -- this is how the
 * data-gradient pass (called with w_dgrad, Cin<->Cout swapped, stride 1) fuses the ReLU backward
 * of autograd (t_cls_train.py:272,307) into its input gather.
 * If `egate` != NULL the OUTPUT is multiplied by act'(egate) in the epilogue (egate: output geometry,
 * ld=ldegate): used by the data-gradient pass to hand the upstream layer a gradient that is already gated
 * by that layer's own activation (egate = this conv's forward input, which is that layer's output). */
int wu_conv3x3_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                   int N, int H, int W, int Cin, int Cout, int stride, int act,
                   const void* mask, int ldmask, int mask_act,
                   const void* egate, int ldegate, int egate_act, int dtype, void* stream);

/* "Gate bits": the ReLU gate of an activation tensor y (N,H,W,C; C % 64 == 0) as one bit per element instead of the tensor,
 *     uint32 bits[N*H*W][C/64][2];   bit (8k + i) of bits[p][ct][hf]  =  y[p][64 ct + 16 k + 8 hf + i] > 0   (k < 4, i < 8)
 * -- the 32 channels one lane of the conv epilogue holds, so a gated epilogue reads one dword per lane and row where the gate
 * tensor costs four 16-byte loads (the gated data-gradient convs of the 64-channel 256x256 layers are HBM-bound: 805 -> 554 MB).
 * wu_conv3x3_fwd_bits is wu_conv3x3_fwd (stride 1, bf16) with either
 *   gate_bits_out != NULL: act must be WU_ACT_RELU; the bits of the output are written next to y (forward of a block's first conv), or
 *   egate_bits   != NULL: act = NONE, bias = NULL; the output is multiplied by the gate the bits encode (data-gradient pass of the
 *                          block's second conv; egate_bits has the OUTPUT geometry, Cout channels).
 * Only the LDS-DMA kernel has this epilogue: wu_conv3x3_gate_bits_supported(...) != 0 must hold for the shape (else use the
 * gate-tensor form of wu_conv3x3_fwd).  wu_gate_bits_bytes: size of a bits buffer. */
int wu_conv3x3_gate_bits_supported(int H, int W, int ldx, int ldy, int Cin, int Cout, int dtype);
size_t wu_gate_bits_bytes(int N, int H, int W, int C);
int wu_conv3x3_fwd_bits(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                        void* gate_bits_out, const void* egate_bits, int N, int H, int W, int Cin, int Cout,
                        int act, int dtype, void* stream);

/* y = ReLU(conv3x3(x) + bias) AND pool = max_pool2d(y, 2) (floor: [N][H/2][W/2][Cout], pixel stride ldpool) in one call
 * (cunet.py:45-46, 49-50, 53-54).  On the bf16 LDS-DMA path the conv epilogue writes the pooled tensor itself; otherwise the
 * conv is followed by wu_maxpool2_fwd.  Same argument rules as wu_conv3x3_fwd (stride 1); H and W even. */
int wu_conv3x3_relu_pool_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                             void* pool, int ldpool, int N, int H, int W, int Cin, int Cout, int dtype, void* stream);
/* The same with TWO bits per element of y from the epilogue (round 4; LDS-DMA path: ask wu_conv3x3_gate_bits_supported): the ReLU gate
 * (gate-bit layout, above) and, in the same layout, "this element is the FIRST maximum of its 2x2 window" (scan order (0,0), (0,1), (1,0),
 * (1,1): torch.nn.MaxPool2d's rule).  wu_maxpool2_bwd_bits computes MaxPool2d's backward fused with the skip-gradient sum and the ReLU
 * gate (cunet.py:46,49,52 in backward) from those bits instead of the activation tensor. */
int wu_conv3x3_relu_pool_bits_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                                  void* pool, int ldpool, void* gate_bits_out, void* sel_bits_out,
                                  int N, int H, int W, int Cin, int Cout, int dtype, void* stream);
/* 3x3 conv, stride 1, bf16, on images at most 16 pixels wide with CHUNK-MAJOR weights (round 4; the frozen estimator's layer3 / layer4 convs and their
 * data gradient, classifier.py:106): w_chunked[Cin / 32][9][Cout][32] = the pack of wu_pack_conv3x3 ([9][Cout][Cin]) viewed as [9][Cout][Cin / 32][32] and
 * permuted (2, 0, 1, 3), so that a chunk's tap slab is 4 KiB contiguous (the small-image kernel is bound by the bytes it pulls out of L2).  y = act(conv(x) +
 * bias) [* act'(egate)] exactly as wu_conv3x3_fwd computes it on the small-image kernel (option 3).  wu_conv3x3_small_supported: 1 = the shape runs there
 * and the dispatch rule prefers it to the generic template; otherwise call wu_conv3x3_fwd with the ordinary pack. */
int wu_conv3x3_small_supported(int N, int H, int W, int ldx, int ldy, int ldegate, int Cin, int Cout);
int wu_conv3x3_small_fwd(const void* x, int ldx, const void* w_chunked, const float* bias, void* y, int ldy,
                         const void* egate, int ldegate, int egate_act, int N, int H, int W, int Cin, int Cout, int act, void* stream);

/* The last decoder conv AND the network's head in one launch (round 4; cunet.py:78-82: dconv_up1[2] + ReLU, then tanh(conv_last(y))):
 * y = ReLU(conv3x3(x) + bias) as above and out_nchw[N][3][H][W] (fp32) = tanh(head_w[3][64] . y + head_bias), the head computed on the matrix
 * cores from the conv epilogue's packed registers (head weights split into three bf16 terms: fp32-exact products of the STORED
 * bf16 y).  y == NULL: the 64-channel tensor is not written at all (inference; ldy ignored).  bf16 LDS-DMA path only, Cout == 64,
 * 64 <= Cin < 256, Cin % 32 == 0: ask wu_conv3x3_relu_head_supported (1 = yes); otherwise call wu_conv3x3_fwd + wu_conv1x1_tanh_fwd. */
int wu_conv3x3_relu_head_supported(int H, int W, int ldx, int ldy, int Cin, int Cout, int dtype);
int wu_conv3x3_relu_head_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                             const float* head_w, const float* head_bias, float* out_nchw,
                             int N, int H, int W, int Cin, int Cout, int dtype, void* stream);
int wu_maxpool2_bwd_bits(const unsigned* gate_bits, const unsigned* sel_bits, const void* dy, int lddy, const void* dskip, int lddskip,
                         void* dx, int lddx, int N, int H, int W, int C, int dtype, void* stream);

/* Weight + bias gradient of the conv above: dw_oihw[Cout][Cin][3][3] (+)= sum_pixels dy (x) x,
 * dbias[Cout] (+)= sum dy, with dy gated by act'(y) when `y` != NULL.  `workspace` must hold
 * wu_conv3x3_wgrad_workspace() bytes (deterministic split-K slabs).  accumulate != 0 adds into
 * dw/dbias (autograd's .grad accumulation), else overwrites. */
size_t wu_conv3x3_wgrad_workspace(int N, int H, int W, int Cin, int Cout, int stride, int dtype);
int wu_conv3x3_wgrad(const void* x, int ldx, const void* dy, int lddy, const void* y, int ldy_, int act,
                     float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes,
                     int N, int H, int W, int Cin, int Cout, int stride, int accumulate,
                     int dtype, void* stream);

/* Data gradient of the stride-2 conv (nets.py:30-31): dx (N,H,W,Cin) from dy (N,Ho,Wo,Cout),
 * w_dgrad as packed above; dy gated by act'(y) when y != NULL.  `workspace` holds
 * wu_conv3x3_s2_dgrad_workspace() bytes (the zero-upsampled gradient); egate as in wu_conv3x3_fwd,
 * except that a bf16 LeakyReLU gate multiplies the fp32 sum, in front of the ONE rounding, on every
 * path (wu_conv3x3_fwd gates the stored bf16 value: the two roundings of a stand-alone gate pass). */
size_t wu_conv3x3_s2_dgrad_workspace(int N, int H, int W, int Cout, int dtype);
int wu_conv3x3_s2_dgrad(const void* dy, int lddy, const void* y, int ldy_, int act, const void* w_dgrad,
                        void* dx, int lddx, void* workspace, size_t workspace_bytes,
                        const void* egate, int ldegate, int egate_act,
                        int N, int H, int W, int Cin, int Cout, int dtype, void* stream);

/* Activation backward as one streaming pass: out = g * act'(y) (ReLU: y > 0; LeakyReLU: y > 0 ? 1 : 0.2),
 * all three NHWC with their own pixel strides; `out` may alias `g`.  Lets both gradient GEMMs of a conv
 * consume a pre-gated gradient (y == NULL / mask == NULL paths), which is what the LDS-DMA wgrad needs. */
int wu_act_gate(const void* g, int ldg, const void* y, int ldy, void* out, int ldo,
                int N, int H, int W, int C, int act, int dtype, void* stream);

/* ---- thin layers (HBM-bound, no MFMA) -------------------------------------------------------
 * First conv of dconv_down1 / of the discriminator: Cin = 3 read straight from the NCHW fp32
 * image (cunet.py:45 via nets.py:20; disc.py:28 via nets.py:28-31).
 * out_nchw == 0: y is NHWC `dtype` with ld=ldy (Cout % 8 == 0);  out_nchw != 0: y is NCHW fp32
 * (the 3->3 SN conv of disc.conv1[0]).  w is OIHW fp32 (Cout,3,3,3) scaled by *inv_sigma if given. */
int wu_conv3x3_c3_fwd(const float* x_nchw, const float* w_oihw, const float* bias, const float* inv_sigma,
                      void* y, int ldy, int out_nchw, int N, int H, int W, int Cout, int stride, int act,
                      int dtype, void* stream);
/* wu_conv3x3_c3_fwd with NHWC output, Cout = 64, ReLU, that also writes the gate bits of its output (see "gate bits" above;
 * the matrix-core form only: wu_conv3x3_c3_gate_bits_supported(...) != 0). */
int wu_conv3x3_c3_gate_bits_supported(int N, int H, int W, int Cout, int stride, const float* bias, int dtype);
int wu_conv3x3_c3_fwd_bits(const float* x_nchw, const float* w_oihw, const float* bias, const float* inv_sigma,
                           void* y, int ldy, void* gate_bits_out, int N, int H, int W, int Cout, int stride, int dtype, void* stream);
/* its weight/bias gradient (the image needs no data gradient in the generator); dy NHWC or NCHW fp32 */
int wu_conv3x3_c3_wgrad(const float* x_nchw, const void* dy, int lddy, int dy_nchw, const void* y, int ldy_,
                        int act, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int Cout, int stride, int accumulate, int dtype, void* stream);
/* Bytes of caller-owned scratch that make the two thin-layer weight gradients (wu_conv3x3_c3_wgrad on its bf16 64-channel
 * path, wu_conv1x1_tanh_bwd) bitwise reproducible: per-workgroup partial sums land there and are folded in a fixed order.
 * Passing workspace = NULL (or a smaller size) selects fp32 atomics across workgroups instead (last-bit run-to-run noise). */
size_t wu_thin_workspace_bytes(void);
/* data gradient wrt the NCHW fp32 image (needed when D is differentiated wrt G's output,
 * t_cls_train.py:243,272): dx_nchw (N,3,H,W) fp32. */
int wu_conv3x3_c3_dgrad(const void* dy, int lddy, int dy_nchw, const void* y, int ldy_, int act,
                        const float* w_oihw, const float* inv_sigma, float* dx_nchw, int N, int H, int W,
                        int Cout, int stride, int accumulate, int dtype, void* stream);

/* conv_last + Tanh (cunet.py:39-40,80-82): out_nchw (N,3,H,W) fp32 = tanh(W x + b),
 * x NHWC (N,H,W,Cin) ld=ldx, w (3,Cin) fp32. */
int wu_conv1x1_tanh_fwd(const void* x, int ldx, const float* w, const float* bias, float* out_nchw,
                        int N, int H, int W, int Cin, int dtype, void* stream);
/* backward: g = dout*(1-out^2); dx = W^T g (NHWC ld=lddx) [* act'(x) if x_gate_act]; dw (+)= g x^T; dbias (+)= sum g. */
int wu_conv1x1_tanh_bwd(const float* dout_nchw, const float* out_nchw, const void* x, int ldx, const float* w,
                        void* dx, int lddx, float* dw, float* dbias, void* workspace, size_t workspace_bytes,
                        int N, int H, int W, int Cin, int accumulate, int x_gate_act, int dtype, void* stream);

/* ---- glue ------------------------------------------------------------------------------------
 * nn.MaxPool2d(2) (cunet.py:27; calls :46,49,52).  x (N,H,W,C) -> y (N,H/2,W/2,C). */
int wu_maxpool2_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int dtype, void* stream);
/* dx = route(dy to the first arg-max of each window, PyTorch's tie rule) [+ dskip]:
 * `dskip` (may be NULL, ld=lddskip) is the gradient arriving over the skip connection of the same
 * tensor (cunet.py:62,69,76), summed here instead of by a separate autograd add.  gate_act != 0: the
 * result is additionally multiplied by act'(x) (x is the pooled conv's activation output). */
int wu_maxpool2_bwd(const void* x, int ldx, const void* dy, int lddy, const void* dskip, int lddskip,
                    void* dx, int lddx, int N, int H, int W, int C, int gate_act, int dtype, void* stream);

/* AdaIN style statistics (utils.py:41-48): y_ = l1(y).view(N, C, 4) with l1 = Linear(nc, 4C) (w: [4C][nc] fp32, b: [4C] or NULL);
 * y_mean[n][c] = mean_k y_[n][c][k], y_std[n][c] = sqrt(unbiased var_k + eps).  `y4` (may be NULL; N*C*4 floats, 16-B aligned)
 * receives y_ for the backward pass.  One launch instead of ~8 stock kernels; nc <= 32. */
int wu_adain_style_fwd(const float* y, const float* w, const float* b, float eps, float* y_std, float* y_mean, float* y4,
                       int N, int C, int nc, void* stream);
/* Gradients of the above wrt l1.weight (dw [4C][nc]) and l1.bias (db [4C], may be NULL) from d_std, d_mean [N][C]
 * (autograd of utils.py:41-48); fixed summation order over n.  accumulate != 0 adds into dw / db. */
int wu_adain_style_bwd(const float* d_std, const float* d_mean, const float* y, const float* y4, const float* y_std,
                       const float* y_mean, float* dw, float* db, int N, int C, int nc, int accumulate, void* stream);

/* The same two calls for up to 4 AdaIN layers that share the conditioning input y -- the three decoder levels of a U-Net pass (cunet.py:59,66,73) --
 * in ONE launch each (round 4).  Host arrays of `levels` entries: w / b / y_std / y_mean / y4 / dw / db pointers (b[i], y4[i], db[i] may be NULL), eps, C.
 * Per level the arithmetic is the single call's: results are bit-identical. */
int wu_adain_style_fwd_multi(int levels, const float* y, const float* const* w, const float* const* b, const float* eps,
                             float* const* y_std, float* const* y_mean, float* const* y4, int N, const int* C, int nc, void* stream);
int wu_adain_style_bwd_multi(int levels, const float* const* d_std, const float* const* d_mean, const float* y, const float* const* y4,
                             const float* const* y_std, const float* const* y_mean, float* const* dw, float* const* db,
                             int N, const int* C, int nc, int accumulate, void* stream);

/* AdaIN instance statistics (utils.py:34-39,47): per (n,c) over H*W: stats[n][c] = {mean, rstd}
 * with rstd = 1/sqrt(unbiased_var + eps).  `scratch` holds N*C*2*WU_MAX_SPLITS floats (per-split partial
 * sums, folded in fixed order: results are bitwise reproducible). */
#define WU_MAX_SPLITS 16
int wu_adain_stats(const void* x, int ldx, float* stats, float* scratch, int N, int H, int W, int C,
                   float eps, int dtype, void* stream);
/* The same statistics of N images, computed with the split count wu_adain_stats picks for a batch of `split_batch` images (a positive
 * multiple of N): bit for bit what wu_adain_stats returns for these images inside a batch of that size.  The condition sweep
 * (wu_adain_upcat_sweep_fwd) computes the bottleneck statistics once for B images and must match the repeated batch of R * B. */
int wu_adain_stats_as_batch(const void* x, int ldx, float* stats, float* scratch, int N, int H, int W, int C,
                            float eps, int split_batch, int dtype, void* stream);

/* Fused AdaIN-apply (utils.py:49-50) -> bilinear x2 align_corners=True (cunet.py:26,60,67,74) ->
 * Dropout(p) (cunet.py:28,61,68,75) written into channels [0,C) of the concat buffer `y`
 * (N,2H,2W,*) ld=ldy; the skip tensor already lives in channels [C, ...) (torch.cat, cunet.py:62).
 * y_std / y_mean: (N,C) fp32 style statistics of utils.py:46,48.  p_drop == 0 -> eval mode.
 * Dropout keep-mask = counter RNG(seed, element index); keep scale 1/(1-p).  `mask_bits` (may be NULL):
 * N*2H*2W*(C / elements-per-16-B) bytes receiving one keep-bit per element, so the backward pass reads the
 * mask instead of re-hashing (pass the same pointer, or NULL to regenerate from the seed).
 * `seed_dev` (may be NULL): device-resident uint64 added to `seed` inside the kernel -- a captured hipGraph freezes the
 * `seed` argument, the counter it points to can be bumped between replays (the reference's inference loops run with
 * Dropout ACTIVE: inference/inf_transfer_c.py:88-96 never calls .eval()).
 * mask_is_input != 0: `mask_bits` is READ instead of drawn (an externally supplied keep-mask, e.g. one captured from the
 * reference's own nn.Dropout, for parity tests and replays of a recorded step). */
int wu_adain_upcat_fwd(const void* x, int ldx, const float* stats, const float* y_std, const float* y_mean,
                       void* y, int ldy, int N, int H, int W, int C, float p_drop, uint64_t seed,
                       const uint64_t* seed_dev, uint8_t* mask_bits, int mask_is_input, int dtype, void* stream);
/* Condition sweep (forward only): wu_adain_upcat_fwd over a VIRTUAL batch of N images whose sources are not repeated in memory.
 * Output image n reads the activation x and `stats` of source image n % Bx (x: (Bx,H,W,C) ld=ldx, stats: (Bx,C,2); Bx divides N:
 * Bx = B where one encoder output serves every conditioning row, Bx = N where the input is already per (row, image)), the style rows
 * y_std / y_mean (N,C) of image n, and draws its dropout decisions from the element index of the virtual batch -- bit for bit what
 * wu_adain_upcat_fwd writes for the materialised repeat, with the formulation chosen as that function chooses it.  The same launch
 * also fills channels [C, C + Cs) of concat image n from `skip` (Bs,2H,2W,>=Cs) ld=ldskip, image n % Bs (Bs divides N; Cs == 0: no
 * skip copy), so one launch writes the whole [upsampled | skip] row the consumer conv reads.  No keep bytes: nothing differentiates. */
int wu_adain_upcat_sweep_fwd(const void* x, int ldx, int Bx, const float* stats, const float* y_std, const float* y_mean,
                             const void* skip, int ldskip, int Bs, int Cs, void* y, int ldy, int N, int H, int W, int C,
                             float p_drop, uint64_t seed, const uint64_t* seed_dev, int dtype, void* stream);
/* Backward of the above.  dy: gradient of the concat buffer channels [0,C) (N,2H,2W) ld=lddy.
 * Produces dx (N,H,W,C) ld=lddx and d_y_std, d_y_mean (N,C) fp32.  `gtmp` (N*H*W*C elements of `dtype`) and
 * `sums` (N*C*2*(1+WU_MAX_SPLITS) floats) are caller-provided scratch.  x_gate_act != 0: dx is additionally multiplied by
 * act'(x) (x is a conv activation output; the producer conv then receives a pre-gated gradient). */
int wu_adain_upcat_bwd(const void* dy, int lddy, const void* x, int ldx, const float* stats, const float* y_std,
                       void* dx, int lddx, float* d_y_std, float* d_y_mean, void* gtmp, float* sums,
                       int N, int H, int W, int C, float p_drop, uint64_t seed, const uint8_t* mask_bits,
                       int x_gate_act, int dtype, void* stream);
/* The keep-mask wu_adain_upcat_fwd draws for (seed, p): mask[n][c][h2][w2] (NCHW uint8), for tests. */
int wu_dropout_mask(uint8_t* mask_nchw, int N, int H2, int W2, int C, float p_drop, uint64_t seed, void* stream);

/* Mean absolute error between two fp32 tensors of n elements (reference ops.py:22-24 l1_loss = F.l1_loss): *loss = mean|a - b|
 * and, when grad != NULL, grad[i] = sign(a[i] - b[i]) / n (the gradient wrt a for an upstream gradient of 1), in one pass.
 * scratch: wu_l1_mean_scratch_floats() floats of per-workgroup partial sums, folded in index order (deterministic). */
size_t wu_l1_mean_scratch_floats(void);
int wu_l1_mean(const float* a, const float* b, float* grad, float* scratch, float* loss, long long n, void* stream);

/* Discriminator head (disc.py:32): feat[n][c] = sum_{h,w} x[n,h,w,c]  (fp32), and its backward
 * dx[n,h,w,c] = dfeat[n][c]. */
int wu_sumpool_fwd(const void* x, int ldx, float* feat, int N, int H, int W, int C, int dtype, void* stream);
int wu_sumpool_bwd(const float* dfeat, void* dx, int lddx, int N, int H, int W, int C, int dtype, void* stream);

/* ---- frozen ResNet-101 estimator in the GAN loop -------------------------------------------------------------------------
 * The reference runs torchvision.models.resnet101 (classifier.py:106-112, estimator.py:143-151) four times per iteration and
 * differentiates it once wrt its input (t_cls_train.py:237,247-250,297,424); it is frozen and in eval mode, so every BatchNorm
 * is a per-channel affine that the caller folds into the conv weight / bias.  The 3x3 convs of the Bottleneck blocks use
 * wu_conv3x3_fwd / wu_conv3x3_s2_dgrad above; these are the remaining ops.
 *
 * 1x1 conv as a GEMM on the matrix cores.  One GEMM row per point (n, hc, wc) of a COARSE grid N x Hc x Wc:
 *     in  = x[n, hc*in_stride, wc*in_stride, :]      (x: N x Hin x Win x Cin,  pixel stride ldx)
 *     out = y[n, hc*out_stride, wc*out_stride, :]    (y: N x Hout x Wout x Cout, pixel stride ldy)
 *     out = act(w . in + bias + residual) * act'(egate)          w: [Cout][Cin] in `dtype`, bias fp32 (may be NULL)
 * in_stride = 2 is the downsample conv (nn.Conv2d(cin, cout, 1, stride=2)); out_stride = 2 is its data gradient (called with
 * the transposed weight): the other pixels of each 2x2 output block receive act(residual) * act'(egate), or zero.
 * `residual` / `egate` (may be NULL) have y's geometry (pixel strides ldres / ldegate).  Cin % (128 / sizeof(T)) == 0,
 * Cout % 64 == 0. */
int wu_conv1x1_fwd(const void* x, int ldx, const void* w, const float* bias, const void* residual, int ldres,
                   void* y, int ldy, int N, int Hc, int Wc, int in_stride, int Hin, int Win,
                   int out_stride, int Hout, int Wout, int Cin, int Cout, int act,
                   const void* egate, int ldegate, int egate_act, int dtype, void* stream);
/* Two chained 1x1 convs in ONE launch (bf16): y1 = act1(wa . x + bias_a + res) * act'(gate1), y2 = act2(wb . y1 + bias_b) * act'(gate2),
 * both stored.  x: [M][K1] (pixel stride ldx); wa = the [C1][K1] weight and wb = the [C2][C1] weight in MFMA-FRAGMENT ORDER
 * [cout / 32][k / 16][k half (2)][cout row (32)][8 elements] (a wave's 16-byte A fragments of one (cout block, K step) are 1 KiB
 * contiguous: weights are streamed straight into registers); res / gate1 with y1's geometry, gate2 with y2's; any of bias_a, bias_b,
 * res, gate1, gate2 may be NULL.  Forward: torchvision Bottleneck conv3 + bn3 + residual + ReLU of one block followed
 * by conv1 + bn1 + ReLU of the next (classifier.py:106-112 / estimator.py:143-151 build resnet101); backward: conv1^T of a block (+ the
 * identity-path gradient, gated by the block boundary's ReLU) followed by conv3^T of the previous block (gated by its 3x3 conv's ReLU).
 * Bit-identical to two wu_conv1x1_fwd calls.  Shapes: wu_conv1x1_chain_supported(K1, C1, C2, dtype) != 0. */
int wu_conv1x1_chain_supported(int K1, int C1, int C2, int dtype);
int wu_conv1x1_chain(const void* x, int ldx, const void* wa, const float* bias_a, const void* res, int ldres, int act1,
                     const void* gate1, int ldg1, int gate1_act, void* y1, int ldy1,
                     const void* wb, const float* bias_b, int act2, const void* gate2, int ldg2, int gate2_act, void* y2, int ldy2,
                     long long M, int K1, int C1, int C2, int dtype, void* stream);
/* Stem: nn.Conv2d(3, 64, 7, stride=2, padding=3) + folded BN + ReLU from the NCHW fp32 image to NHWC `dtype`
 * (N, Ho, Wo, 64), Ho = (H-1)/2 + 1; w: OIHW fp32 [64][3][7][7], bias [64] (may be NULL). */
int wu_stem7x7_fwd(const float* x_nchw, const float* w_oihw, const float* bias, void* y, int ldy,
                   int N, int H, int W, int act, int dtype, void* stream);
/* its data gradient wrt the image (g_loss flows through estimator(fake_out) into the generator, t_cls_train.py:247-250,272):
 * dx_nchw (N,3,H,W) fp32 (+)= conv_transpose(dy); dy (N,Ho,Wo,64) already gated by the stem's ReLU. */
int wu_stem7x7_dgrad(const void* dy, int lddy, const float* w_oihw, float* dx_nchw, int N, int H, int W,
                     int accumulate, int dtype, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1): x (N,H,W,C) -> y (N,Ho,Wo,C); `argmax` (may be NULL; N*Ho*Wo*C bytes)
 * receives the window-local index 0..8 of the FIRST maximum (PyTorch's tie rule) for the backward pass. */
int wu_maxpool3s2_fwd(const void* x, int ldx, void* y, int ldy, uint8_t* argmax, int N, int H, int W, int C,
                      int dtype, void* stream);
/* dx (N,H,W,C) = sum over the (overlapping) windows whose arg-max is this pixel of dy; gate_act != 0: * act'(x). */
int wu_maxpool3s2_bwd(const void* dy, int lddy, const uint8_t* argmax, const void* x, int ldx, void* dx, int lddx,
                      int N, int H, int W, int C, int gate_act, int dtype, void* stream);

/* ---- trainable ResNet-101 (classifier.py:106 / estimator.py:143 trained from scratch, sh/train_classifier.sh, sh/train_estimator.sh) --------
 * Train-mode BatchNorm and the weight gradients the frozen estimator does not need.  Rows = the M = N*H*W pixels of an NHWC tensor (pixel
 * stride ld, 16-byte aligned); C % 64 == 0.  Per-channel vectors are fp32; `stats` is float[2][C] = {mean[C], rstd[C]},
 * rstd = 1 / sqrt(var_biased + eps).  Every reduction writes per-split partial sums into the caller-owned `workspace` (size from the
 * matching *_workspace query) and folds them in split order: deterministic, no atomics.
 *
 * Batch statistics of x (shifted one-pass sums, robust on offset data); running_mean / running_var (may be NULL) are updated as
 * nn.BatchNorm2d does in training: r = momentum * batch + (1 - momentum) * r, running_var from the UNBIASED variance (n / (n - 1));
 * num_batches_tracked (int64, may be NULL) += 1. */
size_t wu_bn_stats_workspace(long long M, int C, int dtype);
int wu_bn_stats(const void* x, int ldx, long long M, int C, float eps, float momentum, float* stats,
                float* running_mean, float* running_var, long long* num_batches_tracked,
                void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* y = act(x * scale + shift [+ x2 * scale2 + shift2 | + residual]),  scale = gamma * rstd, shift = beta - mean * scale (per branch):
 * a BatchNorm + ReLU, a Bottleneck's relu(bn3(conv3) + bn_ds(downsample)) (x2 != NULL) or relu(bn3(conv3) + identity) (residual != NULL). */
int wu_bn_apply(const void* x, int ldx, const float* stats, const float* gamma, const float* beta,
                const void* x2, int ldx2, const float* stats2, const float* gamma2, const float* beta2,
                const void* residual, int ldres, void* y, int ldy, long long M, int C, int act, int dtype, void* stream);
/* BatchNorm backward.  gg = g * act'(y) (y = the stored activation output, NULL: gg = g).  dbeta = sum gg, dgamma = sum gg * xhat (overwritten),
 * dx = gamma * rstd * (gg - mean(gg) - xhat * mean(gg * xhat)).  Optional second branch sharing gg (x2 != NULL: dgamma2, dbeta2, dx2) and
 * optional copy of gg itself (gres != NULL: the identity path of a Bottleneck). */
size_t wu_bn_bwd_workspace(long long M, int C, int dtype);
int wu_bn_bwd(const void* g, int ldg, const void* y, int ldy, int act,
              const void* x, int ldx, const float* stats, const float* gamma, float* dgamma, float* dbeta, void* dx, int lddx,
              const void* x2, int ldx2, const float* stats2, const float* gamma2, float* dgamma2, float* dbeta2, void* dx2, int lddx2,
              void* gres, int ldgres, long long M, int C, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* Pointwise conv weight gradient: dw[Cout][Cin] (fp32) (+)= sum over the N x Hc x Wc rows r of dy[r][co] * x[pix(r)][ci], pix as in
 * wu_conv1x1_fwd (in_stride 2: the downsample conv's gather, Hc = (Hin-1)/2+1).  Matrix cores (bf16, or exact fp32); split-K over rows.
 * Cin % 64 == 0, Cout % 64 == 0; accumulate != 0 adds into dw. */
size_t wu_conv1x1_wgrad_workspace(long long M, int Cin, int Cout);
int wu_conv1x1_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, void* workspace, size_t workspace_bytes,
                     int N, int Hc, int Wc, int in_stride, int Hin, int Win, int Cin, int Cout, int accumulate, int dtype, void* stream);
/* Stem weight gradient: dw_oihw[64][3][7][7] (fp32) (+)= the gradient of nn.Conv2d(3, 64, 7, stride=2, padding=3) from the fp32 NCHW
 * image x (N,3,H,W; any H, W) and dy (N,Ho,Wo,64) in `dtype`, Ho = (H-1)/2 + 1. */
size_t wu_stem7x7_wgrad_workspace(int N, int H, int W);
int wu_stem7x7_wgrad(const float* x_nchw, const void* dy, int lddy, float* dw_oihw, void* workspace, size_t workspace_bytes,
                     int N, int H, int W, int accumulate, int dtype, void* stream);

/* ---- input pipeline (t_cls_train.py:81-108: the torchvision / PIL transforms every training image goes through) ----------
 * A batch of decoded RGB images lives in one uint8 buffer `src`; image n starts at byte geo[n].src_off, is src_h x src_w pixels
 * with a row stride of src_ld pixels.  `geo` is an array of N records of wu_image_geo_bytes() (= 72) bytes:
 *     int64 src_off; int32 src_h, src_w, src_ld, crop_top, crop_left, crop_h, crop_w, flip, rot[6], do_rot, pad;
 * The crop window is resized to S x S with Pillow's two-pass fixed-point bilinear resample (transforms.Resize: the window is the
 * whole image; RandomResizedCrop: the drawn box); rot[] are the 16.16 fixed-point coefficients of Image.rotate(angle, NEAREST)
 * (libImaging/Geometry.c affine_fixed) -- for the S x S image when rot_first == 0 (Resize -> RandomRotation, :96-97), for the
 * source image when rot_first != 0 (RandomRotation -> RandomResizedCrop, :83-84); flip = RandomHorizontalFlip.  Results are
 * bit-identical to Pillow's.  dst_u8 (N,S,S,3) and / or dst_nchw (N,3,S,S fp32, ToTensor + Normalize(0.5, 0.5)) may be NULL.
 * ksize >= 2 * ceil(max(1, crop / S)) + 1 over the batch; `workspace` holds wu_image_workspace_bytes(N, S, ksize) bytes. */
size_t wu_image_geo_bytes(void);
size_t wu_image_workspace_bytes(int N, int S, int ksize);
int wu_image_geometry(const uint8_t* src, const void* geo, void* workspace, size_t workspace_bytes,
                      uint8_t* dst_u8, float* dst_nchw, int N, int S, int ksize, int rot_first, void* stream);
/* transforms.ColorJitter(brightness, contrast, saturation, hue=0) in place on the (N,S,S,3) uint8 batch: for image n the ops
 * order[n][0..2] (0 brightness, 1 contrast, 2 saturation, -1 none) with factors[n][op], each Image.blend(degenerate, image, f)
 * with Pillow's arithmetic; then (dst_nchw != NULL) ToTensor + Normalize(0.5, 0.5) into (N,3,S,S) fp32. */
int wu_image_color_jitter(uint8_t* img_u8, const float* factors, const int* order, float* dst_nchw, int N, int S, void* stream);

/* ---- JPEG decoding (dataset.py:64-67, 92-96, 128-129, 148-149: Image.open(path).convert('RGB') in every loader) -------------
 * Baseline JPEG in two halves.  The HOST half (marker parsing, Huffman decoding) is plain re-entrant C++: no global state, no
 * allocation, callable from many threads at once and without a GPU.  The DEVICE half (dequantisation, 8x8 inverse DCT, chroma
 * upsampling, YCbCr -> RGB, zero padding into the batch) is two kernel launches for a whole batch.  The arithmetic is libjpeg's
 * default path (islow IDCT, fancy upsampling, jdcolor tables), so the bytes equal Pillow's.
 *
 * Decoded natively: 8-bit sequential Huffman (SOF0, SOF1), one interleaved scan, greyscale or YCbCr (JFIF marker, or Adobe marker
 * with transform 1, or neither and component ids 1, 2, 3) with luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1, restart intervals.
 * Everything else is REPORTED (supported = 0 and a reason), never guessed at.  Opt-in through wu_jpeg_parse_ex's flags: progressive
 * Huffman frames (SOF2; the host half runs every scan into the same coefficient buffer) and luma sampling 1x2 (4:4:0). */
#define WU_JPEG_OK 0
#define WU_JPEG_NOT_JPEG 1       /* no SOI: another format */
#define WU_JPEG_CORRUPT 2        /* truncated or inconsistent header */
#define WU_JPEG_PROGRESSIVE 3    /* SOF2 */
#define WU_JPEG_ARITHMETIC 4     /* SOF9..15, DAC */
#define WU_JPEG_PRECISION 5      /* 12-bit samples */
#define WU_JPEG_LOSSLESS 6       /* lossless / hierarchical frames */
#define WU_JPEG_COLORSPACE 7     /* CMYK, YCCK, RGB-tagged, two components */
#define WU_JPEG_QTABLE16 8       /* 16-bit quantisation table */
#define WU_JPEG_SAMPLING 9       /* 4:4:0, 4:1:1, sub-sampled luma ... */
#define WU_JPEG_MULTISCAN 10     /* components spread over several scans */
#define WU_JPEG_MAGNITUDE 11     /* set by the entropy stage: a block exceeds the IDCT's overflow bound */
#define WU_JPEG_PROGRESSIVE_INCOMPLETE 12   /* set by the entropy stage: the scans do not deliver every coefficient at full precision, or
                                               follow a script libjpeg only warns about */
#define WU_JPEG_MODE_GREY 0
#define WU_JPEG_MODE_444 1
#define WU_JPEG_MODE_H2V1 2      /* 4:2:2 */
#define WU_JPEG_MODE_H2V2 3      /* 4:2:0 */
#define WU_JPEG_MODE_H1V2 4      /* 4:4:0: only with WU_JPEG_ALLOW_H1V2 */
/* wu_jpeg_parse_ex flags: what is decoded natively BEYOND the list above.  Opt-in; wu_jpeg_parse is flags = 0. */
#define WU_JPEG_ALLOW_PROGRESSIVE 1   /* SOF2, 8-bit, grey or YCbCr: any legal scan script that ends with every coefficient at Al = 0 */
#define WU_JPEG_ALLOW_H1V2 2          /* luma sampling 1x2 (a 4:2:2 file after a lossless 90 degree rotation) */
/* wu_jpeg_info.reserved: the frame kind */
#define WU_JPEG_FRAME_SEQUENTIAL 0    /* SOF0 / SOF1, one interleaved scan */
#define WU_JPEG_FRAME_PROGRESSIVE 1   /* SOF2: scan_offset is the first scan's data; td / ta are unused (every scan names its own) */
typedef struct wu_jpeg_info {
    long long coef_bytes;            /* coefficient storage the image needs: total_blocks * 64 int16 */
    int height, width, ncomp, mode;
    int hs[3], vs[3], tq[3], td[3], ta[3];   /* sampling factors, quantisation / DC / AC table ids per component */
    int restart_interval;            /* in MCUs, 0 = none */
    int mcus_x, mcus_y;
    int blocks_w[3], blocks_h[3];    /* blocks per row / rows of each component plane (MCU-padded) */
    int total_blocks;
    int supported, reason;
    int scan_offset;                 /* first byte of the entropy-coded data */
    int dht_off[8], dqt_off[4];      /* byte offsets of the table bodies inside the file (DC 0-3, AC 0-3; 0 = absent) */
    int max_block_l1;                /* written by the entropy stage: max over blocks of sum |c * q| */
    int reserved;                    /* WU_JPEG_FRAME_* */
} wu_jpeg_info;
size_t wu_jpeg_info_bytes(void);
/* Walks the markers up to SOS.  Returns 0 whenever `info` was filled; a file that cannot be decoded natively has
 * info->supported == 0 and info->reason set. */
int wu_jpeg_parse(const uint8_t* data, size_t nbytes, wu_jpeg_info* info);
/* The same with an OR of WU_JPEG_ALLOW_* in `flags`: a progressive frame (8-bit, 1 or 3 components under the colour-space rule above,
 * sampling as supported after the flags) and / or luma sampling 1x2 are reported supported instead of refused. */
int wu_jpeg_parse_ex(const uint8_t* data, size_t nbytes, wu_jpeg_info* info, int flags);
/* Huffman-decodes the scan of a file wu_jpeg_parse reported supported into caller-owned memory: `coef` receives
 * info->total_blocks blocks of 64 int16 QUANTISED coefficients in natural (row-major) order, plane of component 0 first, blocks
 * of a plane in raster order; `qtab_out` receives 3 tables of 64 uint16 in natural order (unused ones filled with 1).
 * A progressive frame: walks the markers from the start of the file to EOI and runs EVERY scan into the (zeroed) buffer; the
 * quantisation table of a component is the one in force when its first scan starts.
 * Returns 0, or 1 with info->reason set when the file is to be decoded elsewhere -- WU_JPEG_MAGNITUDE: a block's sum |c * q| exceeds
 * the bound under which the 16- / 32-bit IDCT arithmetic cannot overflow; WU_JPEG_PROGRESSIVE_INCOMPLETE: the scans of a progressive
 * file leave a coefficient of a component short of full precision (libjpeg then smooths between blocks) or follow a script libjpeg
 * warns about; WU_JPEG_QTABLE16: a 16-bit table defined between scans -- or a negative code with a message for corrupt data (bad
 * Huffman code or table, coefficient index past 63 or past the scan's band, bad restart sequence, premature marker or end of data,
 * inconsistent scan header, buffer too small). */
int wu_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, wu_jpeg_info* info, int16_t* coef, size_t coef_capacity_bytes,
                           uint16_t* qtab_out);
int wu_jpeg_max_block_l1(void);
/* Device reconstruction of a batch.  coef_dev: the images' coefficient blocks; image n starts at block desc[n].first_block, a
 * multiple of 32.  desc_dev: N records of wu_jpeg_desc_bytes() (= 64) bytes:
 *     int32 first_block, h, w, mode, bw_y, bh_y, bw_c, bh_c, first_tile, nblocks, pad[6];
 * tile_image_dev[t] = image of IDCT tile t (32 blocks; image n owns tiles first_tile .. first_tile + ceil(nblocks / 32) - 1);
 * qtab_dev: N x 3 x 64 uint16.  workspace: wu_jpeg_workspace_bytes(32 * n_tiles) bytes (the uint8 component planes).
 * out_u8 (N, Hmax, Wmax, 3): RGB inside each image's h x w, zero outside.  Stream-ordered, no allocation, no synchronisation.
 * The caller builds the descriptors from wu_jpeg_parse results only; nothing here reads them on the host. */
size_t wu_jpeg_desc_bytes(void);
size_t wu_jpeg_workspace_bytes(long long total_blocks);
int wu_jpeg_reconstruct(const int16_t* coef_dev, const void* desc_dev, const int* tile_image_dev, const uint16_t* qtab_dev,
                        void* workspace, size_t workspace_bytes, uint8_t* out_u8, int N, int Hmax, int Wmax, int n_tiles,
                        void* stream);

/* ---- Huffman decoding of the scan on the device (csrc/jpeg_huff.hip): fills the coefficient buffer wu_jpeg_reconstruct consumes ----
 * What goes over the link is the compressed scan, not the zero-filled coefficients.  HOST half: wu_jpeg_scan_stage copies the
 * entropy-coded bytes of a file wu_jpeg_parse reported supported -- byte stuffing removed, split at the RSTn markers -- and the raw
 * tables into caller-owned memory (re-entrant, no allocation, no GPU).  DEVICE half: wu_jpeg_huff_decode, one 256-thread workgroup per
 * image, a self-synchronising walk over subsequences of `subseq_bits` bits (a multiple of 32 in [64, 4096]).
 *
 * A "segment" is one restart interval (the whole scan without DRI); it starts on a subseq_bits boundary of the image's scan region
 * and is padded with zero bytes; every segment owns at least one subsequence.  Segment record: int32 first_subseq, bit_length,
 * first_mcu, mcu_count.  Tables: 6 records of 272 bytes per image (16 counts + 256 values; DC of component 0, 1, 2, then AC of
 * component 0, 1, 2; zero where unused); 3 x 64 uint16 quantisation tables in natural order as wu_jpeg_entropy_decode writes them.
 * Status word of an image: 0 = its blocks and tables equal wu_jpeg_entropy_decode's; WU_JPEG_MAGNITUDE = decoded, over the bound;
 * otherwise an OR of the WU_JPEG_HUFF_* bits (corrupt entropy-coded data: decode the file elsewhere). */
#define WU_JPEG_HUFF_BAD_CODE 0x100      /* no table entry matches */
#define WU_JPEG_HUFF_DC_CATEGORY 0x200   /* DC category > 15 */
#define WU_JPEG_HUFF_INDEX 0x400         /* coefficient index past 63 */
#define WU_JPEG_HUFF_SHORT 0x800         /* a segment ended before its MCU count was reached (or does not end where its last MCU ends) */
#define WU_JPEG_HUFF_DC_RANGE 0x1000     /* a DC value outside int16 */
#define WU_JPEG_HUFF_DEFAULT_SUBSEQ_BITS 1024
typedef struct wu_jpeg_scan {
    int scan_bytes;                  /* bytes written to scan_out: a multiple of 16, the last 8 are zero padding */
    int n_segments, n_subseq;
    int reserved;
} wu_jpeg_scan;
/* Upper bound of wu_jpeg_scan.scan_bytes for a file of nbytes bytes (0: not staged -- unsupported info, a bad subseq_bits, or more
 * than 2^28 bytes, beyond which bit positions would leave 32 bits); wu_jpeg_scan_segments: the exact number of segment records. */
size_t wu_jpeg_scan_stage_bytes(const wu_jpeg_info* info, size_t nbytes, int subseq_bits);
int wu_jpeg_scan_segments(const wu_jpeg_info* info);
/* Returns 0, or a negative code with a message: -1 arguments / capacity, -2 corrupt Huffman table, -3 bad restart marker sequence. */
int wu_jpeg_scan_stage(const uint8_t* data, size_t nbytes, const wu_jpeg_info* info, int subseq_bits, uint8_t* scan_out,
                       size_t scan_capacity, int* seg_out, size_t seg_capacity_bytes, uint8_t* dht_out1632, uint16_t* qtab_out192,
                       wu_jpeg_scan* result);
/* hdesc_dev: N records of wu_jpeg_huff_desc_bytes() (= 64) bytes, built by the caller from wu_jpeg_parse / wu_jpeg_scan_stage results:
 *     int32 scan_off (bytes into scan_dev, a multiple of 16), scan_bytes, first_seg, n_segments, n_subseq, first_block, nblocks, ncomp,
 *           hs0, vs0, mcus_x, total_mcus, pad[4];       n_subseq = 0: nothing to decode (an image decoded elsewhere)
 * dht_dev: N x 1632 bytes, qtab_dev: N x 3 x 64 uint16, coef_dev: image n's nblocks blocks at first_block, status_dev: N int32.
 * Zeroes exactly the images' blocks, decodes, turns DC differences into values and takes the magnitude bound: three launches whatever
 * N is.  Nothing outside [first_block, first_block + nblocks) of an image is written.  Stream-ordered, no allocation, no
 * synchronisation. */
size_t wu_jpeg_huff_desc_bytes(void);
int wu_jpeg_huff_decode(const uint8_t* scan_dev, const int* seg_dev, const uint8_t* dht_dev, const void* hdesc_dev,
                        const uint16_t* qtab_dev, int16_t* coef_dev, int* status_dev, int N, int subseq_bits, void* stream);

/* ---- JPEG encoding (inference/inf_transfer_c.py:119-120, inf_transfer_e.py:141-142, inf_1year_signals.py:105: save_image(x, '....jpg',
 * normalize=True), i.e. one Pillow Image.save(path) per output image with Pillow's defaults) -------------------------------------
 * Baseline JPEG (SOF0, one interleaved scan, the Annex K Huffman tables, no restart markers), YCbCr 4:2:0 or 4:4:4, quality 1..100,
 * encoded for a whole batch in five kernel launches whatever N and the image sizes: colour conversion + chroma downsampling + forward
 * DCT + quantisation, per-block Huffman bit counts with a prefix sum, bit packing, 0xFF counting, byte stuffing + framing.  The
 * arithmetic is libjpeg's default compress path (jccolor / jcsample / jfdctint "islow" / jcdctmgr / jccoefct / jchuff) in integers, so
 * every file equals the one Pillow writes, byte for byte.  The header functions are host-only and work without a GPU. */
#define WU_JPEG_ENC_U8 2         /* sample type of the source besides WU_F32 / WU_BF16 */
#define WU_JPEG_ENC_420 0        /* chroma subsampling */
#define WU_JPEG_ENC_444 1
size_t wu_jpeg_enc_header_bytes(void);      /* 623: SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS */
/* Writes that header for an h x w image; returns the byte count (> 0) or a negative code with a message. */
int wu_jpeg_enc_header(int h, int w, int quality, int subsampling, uint8_t* out, size_t capacity);
/* The two quantisation tables of `quality` (luma, chroma; 64 uint16 each, natural order): Annex K scaled as libjpeg does. */
int wu_jpeg_enc_qtables(int quality, uint16_t* out128);
/* Per-image descriptor (16 bytes): int32 h, w, capacity, pad.  `capacity`: bytes the image's entropy-coded data may take, at most
 * cap_max.  An image that needs more is NOT truncated: its result is (0, 1). */
size_t wu_jpeg_enc_desc_bytes(void);
/* Caller-owned workspace for a batch of N images of at most Hmax x Wmax (0 for a shape that cannot be encoded); the byte distance
 * between two images' files in `out`; and (tests, tools) the workspace's sections: out8 = byte offsets of the coefficient blocks
 * (int16, 64 per block in zig-zag order, scan order, image n at block n * blocks_max), the per-block bit offsets inside their 256-block
 * tile, the tile totals, (bits, overflow) per image, the raw bit streams (image n at n * raw_stride), the 0xFF counts per 4 KiB
 * chunk; then blocks_max and raw_stride. */
size_t wu_jpeg_enc_workspace_bytes(int N, int Hmax, int Wmax, int subsampling, long long cap_max);
size_t wu_jpeg_enc_out_stride(long long cap_max);
int wu_jpeg_enc_workspace_layout(int N, int Hmax, int Wmax, int subsampling, long long cap_max, long long* out8);
/* Encodes the batch.  Sample (n, c, y, x) of the source is element src[n * sn + c * sc + y * sy + x * sx] of type `dtype`; float
 * samples become bytes as x * 255 (in the tensor's precision), clamped to [0, 255], truncated.  Image n covers y < desc[n].h,
 * x < desc[n].w; nothing outside is read.  qtab_dev: what wu_jpeg_enc_qtables wrote; hdr_dev: image n's header at n * hdr_stride.
 * Image n's file starts at out + n * wu_jpeg_enc_out_stride(cap_max); result_dev[2n] = its byte count, result_dev[2n + 1] = 1 when
 * it did not fit its capacity (count 0, encode it elsewhere).  Stream-ordered: no allocation, no synchronisation. */
int wu_jpeg_enc_encode(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                       const uint16_t* qtab_dev, const uint8_t* hdr_dev, int hdr_stride, void* workspace, size_t workspace_bytes,
                       uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax, int Wmax, int subsampling, long long cap_max,
                       void* stream);

/* ---- PNG encoding (the '.png' variants of the same writers; lossless files for python -m wu.fid) -----------------------------------
 * 8-bit RGB, colour type 2, no interlace, no ancillary chunks, for a whole batch in three kernel launches whatever N and the image
 * sizes: row filters (per row the type with the smallest sum of min(r, 256 - r), ties to the smallest type number), then per
 * wu_png_enc_segment_bytes() of an image's filtered stream one literal-only dynamic-Huffman deflate block (code lengths <= 15), or one
 * stored block where that is not larger, every segment but the last closed by an empty stored block so that the next starts on a byte
 * boundary; then signature, IHDR, one IDAT chunk per segment (zlib header 78 01 in the first, Adler-32 in the last), IEND, with every
 * CRC-32 and the Adler-32 computed on the device.  No LZ77 matching: the files are larger than zlib's, and decode to the same pixels. */
#define WU_PNG_ENC_U8 2          /* sample type of the source besides WU_F32 / WU_BF16 */
/* Per-image descriptor (16 bytes): int32 h, w, pad, pad. */
size_t wu_png_enc_desc_bytes(void);
size_t wu_png_enc_segment_bytes(void);      /* 32768 */
/* Caller-owned workspace for a batch of N images of at most Hmax x Wmax (0 for a shape that cannot be encoded), and the byte distance
 * between two images' files in `out`: the exact worst case of an Hmax x Wmax file, every segment stored --
 * Hmax (1 + 3 Wmax) + (5 + 12) per segment + 51 -- so a file always fits. */
size_t wu_png_enc_workspace_bytes(int N, int Hmax, int Wmax);
size_t wu_png_enc_out_stride(int Hmax, int Wmax);
/* Encodes the batch.  Samples are addressed and converted as by wu_jpeg_enc_encode; image n covers y < desc[n].h, x < desc[n].w and
 * nothing outside is read.  Image n's file starts at out + n * wu_png_enc_out_stride(Hmax, Wmax); result_dev[n] = its byte count.
 * Stream-ordered: no allocation, no synchronisation. */
int wu_png_enc_encode(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                      void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax, int Wmax,
                      void* stream);
/* The same encoder with its options; flags == 0 is wu_png_enc_encode: same bytes, same workspace, same three launches.
 *   WU_PNG_ENC_LZ77  two more launches per batch (match-and-parse, coding) between deflate and frame.  Per segment, nothing crossing a
 *                    segment: the hash of the three bytes at p is ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1) >> 19; the segment is walked in
 *                    blocks of 64 positions, every position of a block reading the head table before the block is inserted (the largest
 *                    position of a hash stays), so the head candidate of p is the nearest position with its hash in front of its block.
 *                    Candidates in this order: distances 1, 3, rowstride - 3, rowstride, rowstride + 3 (rowstride = 1 + 3 w), the head
 *                    candidate; those outside [1, p] are skipped; each is extended to at most min(258, n - p) bytes; the longest wins, a
 *                    tie goes to the earlier candidate, under 3 bytes is no match; a match is dropped where the one found at the next
 *                    position is longer.  Greedy parse from position 0.  One dynamic block:
 *                    both codes limited to 15 bits, HLIT / HDIST trimmed to the last used code, one distance code of length 1 where
 *                    fewer than two are in use.  The block replaces the stored / literal-only one only where it is strictly smaller, so
 *                    no file is larger than wu_png_enc_encode's and wu_png_enc_out_stride stays the worst case.  Integer atomics only:
 *                    the bytes do not depend on scheduling.  Restated in tests/_png_lz_ref.py.
 * The workspace of the options is larger (one 32-bit word per filtered byte): wu_png_enc_workspace_bytes_ex, 0 for a bad shape or
 * unknown flags; with flags == 0 it is wu_png_enc_workspace_bytes.  Word 3 of a segment's info in the workspace tells its block:
 * 0 literal-only, 1 stored, 2 LZ77 (wu_png_enc_seginfo_offset gives where the N * segments * 4 words start). */
#define WU_PNG_ENC_LZ77 1
size_t wu_png_enc_workspace_bytes_ex(int N, int Hmax, int Wmax, int flags);
size_t wu_png_enc_seginfo_offset(int N, int Hmax, int Wmax);
int wu_png_enc_encode_ex(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                         void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax, int Wmax,
                         int flags, void* stream);

/* ---- image grids and tables (torchvision.utils.make_grid in front of the writers above) ------------------------------------------------
 * Every multi-image output of the reference is make_grid(..., normalize=True, scale_each=True) of the pinned torchvision (< 0.4):
 * demo.py:74-82 (per angle, 1 + num_classes one-column grids side by side, the frames of the GIF), t_cls_train.py:361-378 and
 * t_est_train.py:342 (the evaluation summary: a blank and the reference images, then one strip per image), and the tables of
 * inf_transfer_c.py:122-123 / inf_transfer_e.py:151-156.  A table is a list of CELLS, described once on the host and uploaded; one call
 * composes any number of cells in any number of frames of one geometry in THREE launches (csrc/grid.hip): pad fill + range reset, ranges,
 * compose.  Per pixel, in fp32, IEEE round-to-nearest, in this order:
 *     x = source value (bf16 widened), 0 for a blank cell;   WU_GRID_PRE: x = (x + 1) * 127.5            (demo.py:80)
 *     WU_GRID_NORMALIZE: v = clamp(x, lo, hi);  x = (v - lo) / (hi - lo + 1e-5f)                          (make_grid's norm_ip; true division)
 * with (lo, hi) the minimum and maximum of x over ALL cells of the cell's group (blank cells count with their zeros), or the cell's own
 * lo / hi with WU_GRID_FIXED_RANGE (make_grid's range=; every cell of a group carries the same pair).  The ranges do not depend on the
 * launch geometry.  NaN in a source: the range of its group and every pixel normalised by it are unspecified.
 * Output, every byte written (pad_value where no cell lies):
 *     WU_GRID_OUT_F32  fp32 planar (frames, 3, Hg, Wg): what make_grid returns
 *     WU_GRID_OUT_U8   uint8 interleaved (frames, Hg, Wg, 3): x * 255, clamped to [0, 255], truncated (save_image's bytes; pad_value goes
 *                      through the same conversion) -- the batch wu_jpeg_enc_encode / wu_png_enc_encode take as it is
 * The descriptors live in device memory, so the kernels check them: a cell that is empty, lies outside its frame in any direction, has
 * no source and is not blank, or normalises by a group outside [0, n_groups) is ignored -- nothing is written outside the output. */
#define WU_GRID_BF16 1          /* flags: the source holds bf16 (else fp32) */
#define WU_GRID_PRE 2           /*        pre-transform (x + 1) * 127.5 */
#define WU_GRID_BLANK 4         /*        zeros, no source is read (t_cls_train.py:324,361) */
#define WU_GRID_NORMALIZE 8     /*        normalise by the group's range (else the value is written as it is) */
#define WU_GRID_FIXED_RANGE 16  /*        ... by this cell's lo / hi instead: no reduction */
#define WU_GRID_OUT_F32 0
#define WU_GRID_OUT_U8 1
typedef struct wu_grid_cell {
    uint64_t src;                    /* device pointer of sample (c = 0, y = 0, x = 0) */
    long long sc, sy, sx;            /* element strides: sample (c, y, x) at src[c * sc + y * sy + x * sx] -- NCHW, channels-last and slices alike */
    int h, w;
    int frame, y0, x0;               /* the cell covers rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of its frame */
    int group;
    int flags;
    float lo, hi;                    /* WU_GRID_FIXED_RANGE */
    int reserved;
} wu_grid_cell;
size_t wu_grid_cell_bytes(void);     /* 72 */
/* Caller-owned workspace (0 for counts outside 1 .. 2^20), and for tests and tools its sections as byte offsets: out2[0] = the per-group
 * (lo, hi) fp32 pairs, group g at out2[0] + 8 g, written by the compose launch for every group a WU_GRID_NORMALIZE cell uses (zero
 * otherwise); out2[1] = the order-preserving uint32 images the range launch reduces into. */
size_t wu_grid_workspace_bytes(int n_cells, int n_groups);
int wu_grid_workspace_layout(int n_cells, int n_groups, long long* out2);
/* Composes the table.  Everything the host can know is checked before the first launch (rc < 0, wu_last_error): the counts, the geometry
 * (frames, Hg, Wg in 1 .. 2^20), out_kind, out_bytes >= frames * Hg * Wg * 3 * element size, the workspace size, null pointers, alignment
 * (descriptors 8, workspace and output 16 bytes).  Stream-ordered: no allocation, no synchronisation, capturable. */
int wu_grid_compose(const void* cells_dev, int n_cells, int n_groups, void* workspace, size_t workspace_bytes, void* out, size_t out_bytes,
                    int out_kind, int frames, int Hg, int Wg, float pad_value, void* stream);

/* ---- PNG decoding (the reader of wu_png_enc_encode's files: the header parse on the host, inflate and unfilter on the device) ---------
 * 8-bit RGB, colour type 2, no interlace, and the framing the encoder writes: IDAT chunk k holds the deflate data of bytes
 * [32768 k, 32768 (k + 1)) of the filtered stream as a self-contained, byte-aligned run of deflate blocks that references nothing before
 * its start (zlib's Z_FULL_FLUSH every wu_png_enc_segment_bytes(), pigz -i), the zlib header in front of the first, the Adler-32 behind
 * the last.  The segments of such a file are found from the chunk headers alone and can be inflated independently of each other.
 *
 * wu_png_dec_parse: host only, no GPU.  Reads untrusted bytes: every length is checked against `nbytes` in 64-bit arithmetic before
 * use.  Returns 0 whenever `info` was filled; a file that is not taken natively has info->supported == 0 and info->reason:
 *   NOT_PNG        no signature
 *   HEADER         no IHDR of 13 bytes with a right CRC as the first chunk, a zero size, compression / filter method not 0, interlace > 1
 *   COLOUR_TYPE / BIT_DEPTH / INTERLACED   not colour type 2 / not 8 bits / Adam7 (tested in this order)
 *   TOO_LARGE      height * width over `max_pixels`, or a side over 65535
 *   CORRUPT_CHUNK  a chunk that runs past the end of the file (a truncated file, no IEND), IDAT chunks that are not consecutive, none at
 *                  all, a critical chunk other than IHDR / IDAT / IEND (PLTE included), or a bad zlib header (CM = 8, window <= 32 KiB,
 *                  FCHECK, no FDICT) at the start of the first IDAT
 *   NOT_SEGMENTED  not exactly ceil(height (1 + 3 width) / 32768) IDAT chunks, a first one without room for the zlib header, a last one
 *                  without room for the Adler-32, or one of more than wu_png_dec_max_chunk_bytes() bytes
 * Ancillary chunks before and after the IDAT run are skipped unread; the IDAT CRCs are left to whoever inflates.  idat[2 i], idat[2 i + 1]
 * receive offset (inside the file) and length of the i-th IDAT body for i < idat_capacity; info->n_idat counts all of them, so a caller
 * whose list was too short calls again.  A supported file may still be a foreign one with the right chunk count by coincidence: that
 * shows when the segments are inflated. */
#define WU_PNG_DEC_OK 0
#define WU_PNG_DEC_NOT_PNG 1
#define WU_PNG_DEC_HEADER 2
#define WU_PNG_DEC_COLOUR_TYPE 3
#define WU_PNG_DEC_BIT_DEPTH 4
#define WU_PNG_DEC_INTERLACED 5
#define WU_PNG_DEC_NOT_SEGMENTED 6
#define WU_PNG_DEC_TOO_LARGE 7
#define WU_PNG_DEC_CORRUPT_CHUNK 8
typedef struct wu_png_dec_info {
    long long filtered_bytes;        /* height (1 + 3 width) */
    int height, width;
    int bit_depth, colour_type, interlace;
    int n_idat;                      /* IDAT chunks in the file */
    int n_segments;                  /* ceil(filtered_bytes / 32768) */
    int supported, reason;
    int reserved;
} wu_png_dec_info;
size_t wu_png_dec_info_bytes(void);
size_t wu_png_dec_max_chunk_bytes(void);    /* 40960: a 32 KiB segment of 9-bit fixed-Huffman literals and some */
int wu_png_dec_parse(const uint8_t* data, size_t nbytes, long long max_pixels, wu_png_dec_info* info, long long* idat, int idat_capacity);

/* The device stage: two launches for a batch of N parsed files, each a grid of one-wave workgroups (csrc/png_dec.hip).
 * src_dev: the files' bytes, uploaded by the caller.  desc_dev: N descriptors of wu_png_dec_desc_bytes() (32) bytes
 *     { long long src_off; int file_bytes, h, w, first_seg, nseg, pad; }     h = w = 0: not decoded here, the slot is zeroed, status 0
 * seg_dev: n_segments rows of wu_png_dec_seg_bytes() (16) bytes { int image, k; uint32_t off, len; } -- the k-th IDAT body of `image` at
 * `off` inside its file -- the rows of one image consecutive from its first_seg.  out_u8: (N, Hmax, Wmax, 3), every byte written: the
 * image, zeros as padding, all zeros for an image with a status other than 0.  status_dev[n]: 0, or 1 chunk-crc, 2 bad-stream,
 * 3 distance (a match reaching in front of its segment), 4 segment-size, 5 filter-type, 6 adler -- the first failing check of the first
 * failing segment, then filter-type, then adler; at least as strict as zlib.
 * Every buffer comes with its length in bytes and the call is refused (-1, wu_last_error) if one is smaller than N, Hmax, Wmax and
 * n_segments require; the kernels check every descriptor and segment row against the same lengths before they follow it, so a bad row
 * gives status 2, never an access outside a buffer.  workspace: wu_png_dec_workspace_bytes() bytes, 256-byte aligned (0: unsupported
 * shape -- a side over 65535, more than 2^30 filtered bytes per image, more segments than N images of that size have).
 * Stream-ordered: no allocation, no synchronisation. */
size_t wu_png_dec_desc_bytes(void);
size_t wu_png_dec_seg_bytes(void);
size_t wu_png_dec_workspace_bytes(int N, int Hmax, int Wmax, long long n_segments);
int wu_png_dec_decode(const uint8_t* src_dev, size_t src_bytes, const void* desc_dev, size_t desc_bytes, const void* seg_dev, size_t seg_bytes,
                      int n_segments, void* workspace, size_t workspace_bytes, uint8_t* out_u8, size_t out_bytes, int* status_dev,
                      size_t status_bytes, int N, int Hmax, int Wmax, void* stream);

/* ---- InceptionV3 forward for FID / Inception Score (eval/fid_score.py, eval/inception.py, eval/inception_score.py) ---------------------
 * pytorch-fid's FID InceptionV3 and torchvision's Inception3 in eval mode: every BasicConv2d is conv (no bias) + BatchNorm(eps 1e-3) + ReLU,
 * folded by the caller into one conv with an fp32 bias.  Forward only; no atomics, every result is deterministic.
 *
 * Generic KH x KW conv (every conv of the network, and the fc head as a 1x1 over N x 1 x 1 pixels) as an implicit GEMM on the matrix cores:
 *     y = act(conv(x, w) + bias),  x (N,H,W,Cin) ld=ldx,  y (N,Ho,Wo,Cout) ld=ldy,  Ho = (H + 2 pad_h - KH) / stride_h + 1 (likewise Wo)
 * Zero padding; act WU_ACT_NONE or WU_ACT_RELU; only channels [0, Cout) of y are written (a Mixed block's branches write their channel
 * slices of the concat buffer).  Cin % 16 == 0, Cout % 16 == 0, KH, KW <= 15, pad < kernel, ldx / ldy multiples of 8, x / y / w_packed /
 * bias (may be NULL) 16-byte aligned.  w_packed: wu_conv_kxk_packed_bytes() bytes written once per weight by wu_pack_conv_kxk from the
 * OIHW fp32 weight [Cout][Cin_w][KH][KW]; input channels Cin_w..Cin-1 are zero (the first layer's 3 image channels padded to 16). */
size_t wu_conv_kxk_packed_bytes(int Cout, int Cin, int KH, int KW, int dtype);
int wu_pack_conv_kxk(const float* w_oihw, void* w_packed, int Cout, int Cin_w, int Cin, int KH, int KW, int dtype, void* stream);
int wu_conv_kxk_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                    int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                    int act, int dtype, void* stream);
/* 3x3 pools, x (N,H,W,C) -> y (N,Ho,Wo,C), Ho = (H + 2 pad - 3) / stride + 1; C % 4 == 0, 16-byte aligned x / y.
 *   WU_POOL_MAX:          F.max_pool2d(x, 3, stride, pad) (stride 1 or 2, pad 0 or 1; padding never wins)
 *   WU_POOL_AVG:          F.avg_pool2d(x, 3, 1, 1) (count_include_pad=True: torchvision's InceptionA / C / E)
 *   WU_POOL_AVG_EXCL_PAD: F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) (the FID InceptionV3) */
#define WU_POOL_MAX 0
#define WU_POOL_AVG 1
#define WU_POOL_AVG_EXCL_PAD 2
int wu_pool3x3_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int stride, int pad, int mode, int dtype, void* stream);
/* Global average pool: out[n * ldo + c] = mean over H x W of x[n,:,:,c] (fp32 out; fp64 sums in a fixed order).  C % 4 == 0. */
int wu_global_avgpool_fwd(const void* x, int ldx, float* out, int ldo, int N, int H, int W, int C, int dtype, void* stream);
/* Network input: src_u8 == 0: NCHW fp32 images (N,3,Hin,Win); src_u8 != 0: dense NHWC uint8 (N,Hin,Win,3), read as x / 255 (correctly
 * rounded, as numpy's float32 division).  v = v * in_scale + in_shift (1, 0 = none; 0.5, 0.5 maps [-1, 1] generator output to [0, 1]),
 * bilinear resize to Ho x Wo (F.interpolate, align_corners=False, no antialias; Ho x Wo = Hin x Win copies), normalize != 0: 2 v - 1.
 * y (N,Ho,Wo,cpad) ld=ldy in `dtype`, channels 3..cpad-1 zero; cpad % 4 == 0, 4 <= cpad <= ldy. */
int wu_inception_input(const void* src, int src_u8, int N, int Hin, int Win, float in_scale, float in_shift, int normalize,
                       void* y, int ldy, int Ho, int Wo, int cpad, int dtype, void* stream);
/* Feature statistics for the FID: for a batch x (B x D fp32, row stride ldx) and the shift K = shift[D] (fp32),
 *     sum[d] += sum_b (x[b][d] - K[d]),   cross[i * D + j] += sum_b (x[b][i] - K[i]) (x[b][j] - K[j])     (both fp64, caller-zeroed)
 * init_shift != 0: K is first SET to this batch's column mean (the first batch of a data set).  The per-batch products are exact fp32
 * MFMA chains over b, the cross-batch sums fp64: mu = K + sum / n, sigma = (cross - sum sum^T / n) / (n - 1). */
int wu_feature_stats_update(const float* x, int ldx, int B, int D, float* shift, int init_shift, double* sum, double* cross, void* stream);

/* ---- Kernel Inception Distance (wu/kid.py): the unbiased polynomial-kernel MMD^2 of S subsets of m rows of two feature banks -----------
 * x (n1 x D fp32, row stride ldx) and y (n2 x D, ldy) are the banks; idx (S, 2, m) int32 on the device holds, per subset, the m row
 * positions into x and then the m into y (values are clamped into the bank by the kernel; validate them before upload).  With
 *     k(a, b) = (gamma <a, b> + coef0)^degree      in fp64 on the rows widened to fp64, the power by repeated multiplication,
 *     sums[3 s + 0] = sxx = sum_{i != j} k(x_i, x_j),   sums[3 s + 1] = syy likewise,   sums[3 s + 2] = sxy = sum_{i, j} k(x_i, y_j),
 *     mmd2[s] = (sxx + syy) / (m (m - 1)) - 2 sxy / (m m).
 * Two launches for all S subsets: 64 x 64 tiles on the fp64 matrix cores (upper-triangular tiles of xx / yy, every tile of xy), each
 * reduced to one double in `workspace` in a fixed order, then one wave per subset.  No atomics: the same inputs give the same bits.
 * Stream-ordered, caller-owned buffers, no allocation, no synchronisation.  m >= 2, m <= min(n1, n2), degree >= 1, S <= 65535, ld >= D. */
size_t wu_kid_workspace_bytes(int S, int m);      /* 0 for S or m out of range */
int wu_kid_mmd(const float* x, int ldx, int n1, const float* y, int ldy, int n2, const int* idx, int S, int m, int D, int degree,
               double gamma, double coef0, void* workspace, double* sums, double* mmd2, void* stream);

/* ---- Improved precision / recall and density / coverage (wu/prdc.py): k-NN radii and manifold-membership counts of two feature banks ----
 * For fp32 rows a, b of width D widened to fp64:  d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0), every operation rounded on its own.
 *   wu_knn_radii:   radii[i] = the (k + 1)-th smallest of { d2(x_i, x_j) : j < n } with d2(x_i, x_i) forced to 0 (the row itself counts).
 *   wu_prdc_counts: A[i] = #{ j : d2(x_i, y_j) <= radii_x[i] },  B[i] = #{ j : d2(x_i, y_j) <= radii_y[j] }   (n1 values each),
 *                   C[j] = #{ i : d2(x_i, y_j) <= radii_x[i] }                                                  (n2 values).
 * 64 x 64 tiles of <a, b> on the fp64 matrix cores; no distance matrix and no tile of one reaches global memory.  wu_knn_radii runs a grid
 * of (row tiles, col_splits): each workgroup keeps the k + 1 smallest d2 per row over the column tiles of its split, a finish launch merges
 * the splits.  col_splits = 0 lets the library choose from n; 1..1024 forces that many (a split without columns contributes +inf).  The
 * counts cross workgroups as integer atomic adds, the radii are order-independent: the same inputs give the same bits.
 * workspace: wu_prdc_workspace_bytes(n1, n2, k, col_splits) bytes serve wu_knn_radii on either bank (with that k and col_splits) and
 * wu_prdc_counts; 0 for arguments out of range.  Stream-ordered, caller-owned buffers, no allocation, no synchronisation.
 * 1 <= k <= 16, k + 1 <= n <= 2^21, ld >= D >= 1. */
size_t wu_prdc_workspace_bytes(int n1, int n2, int k, int col_splits);
int wu_knn_radii(const float* x, int ldx, int n, int D, int k, int col_splits, void* workspace, double* radii, void* stream);
int wu_prdc_counts(const float* x, int ldx, int n1, const double* radii_x, const float* y, int ldy, int n2, const double* radii_y, int D,
                   void* workspace, unsigned* A, unsigned* B, unsigned* C, void* stream);

/* ---- Top-k nearest bank rows of every query row (wu/retrieval.py): which rows of a bank a row is closest to, and how close ------------------
 * d2 as above, formed as wu_knn_radii forms it.  For query row i, dist2[i*k + j] / index[i*k + j], j < k, are the k smallest pairs
 * (d2(q_i, b_c), c) over the bank columns c < nb in the lexicographic order: the smaller d2 first, on equal d2 the smaller c.  A total
 * order, so the result does not depend on col_splits or on the order workgroups finish in; no floating-point atomics: the same inputs give
 * the same bits.  self_offset >= 0 says that query row i IS bank row self_offset + i (the queries are a chunk of the bank, or the whole of
 * it at 0): that one column is skipped.  self_offset = -1: no column is skipped.
 * 64 x 64 tiles of <q, b> on the fp64 matrix cores, grid (query row tiles, col_splits); each (row, split) keeps its k best pairs, a finish
 * launch merges the splits.  col_splits = 0 lets the library choose as wu_knn_radii does; 1..1024 forces that many.  No distance matrix and
 * no tile of one reaches global memory.  workspace: wu_nn_workspace_bytes(nq, nb, k, col_splits) bytes, aligned to 8 (0 for arguments out of
 * range; pure host); ws_bytes is what the caller holds, a short one is refused.  Stream-ordered, caller-owned buffers, no allocation, no
 * synchronisation.  1 <= k <= 16, 1 <= nq <= 2^21, k <= nb <= 2^21 (k + 1 <= nb and self_offset + nq <= nb with self_offset >= 0),
 * ld >= D >= 1.  Non-finite features give meaningless neighbours, never an access outside a buffer. */
size_t wu_nn_workspace_bytes(int nq, int nb, int k, int col_splits);
int wu_nn_topk(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, int k, int self_offset, int col_splits, void* ws,
               size_t ws_bytes, double* dist2, int* index, void* stream);

/* ---- Every pair under a radius (wu/retrieval.py: radius_join, leak_mask, duplicate_groups): the clean split a top-k search cannot give -------
 * d2 as above, the same bits as wu_nn_topk and wu_knn_radii form.  The pair (i, c), i < nq, c < nb, is a MEMBER when
 *     d2(q_i, b_c) <= radius2                                  (`<=`, as wu_prdc_counts decides it),
 *     c != self_offset + i        when self_offset >= 0        (query row i IS bank row self_offset + i, as in wu_nn_topk),
 *     c >  self_offset + i        when upper_only != 0         (needs self_offset >= 0: each unordered pair of a self-join once).
 * The result is CSR: row_ptr (nq + 1 int64, row_ptr[0] = 0), and for row i at positions row_ptr[i] .. row_ptr[i + 1] - 1 the member columns
 * col, ascending, with dist2 beside them.  Two passes over the same 64 x 64 fp64 matrix-core tiles, grid (query row tiles, col_splits):
 *   wu_nn_radius_count   norms, then per (row, split) the number of members and per tile one byte that says whether it holds any, then ONE
 *                        workgroup turns the counts into exclusive int64 offsets (kept in the workspace, as the bytes are) and row_ptr.  The caller reads row_ptr[nq] (8 bytes: the one synchronisation) and sizes
 *                        col / dist2 with it.
 *   wu_nn_radius_fill    the SAME arguments and the workspace as wu_nn_radius_count left it, plus row_ptr and the capacity of col / dist2
 *                        in entries: recomputes the tiles that hold a member and writes each row's members from its (row, split) offset.  A
 *                        workgroup whose rows have no member in its split returns before its first tile.  capacity must be >= row_ptr[nq] (the caller, who
 *                        has read it, checks; the kernel stores only inside min(row_ptr[i + 1], capacity), so a short buffer loses entries
 *                        and is never overrun).  capacity == 0 launches nothing and accepts NULL col / dist2.
 * One (row, split) slot is written by one thread, columns ascending, so the bytes do not depend on col_splits or on the order workgroups
 * finish in; nothing crosses workgroups through an atomic and no workgroup waits on another.  col_splits = 0 lets the library choose: among
 * 1 .. max(768 / row tiles, 8) splits (at most one per column tile) the one whose row tiles x splits best fill whole rounds of the 768
 * workgroups resident at once on a 256-CU part, the fewer on a tie; 1..1024 forces that many.  No distance matrix and no tile of one
 * reaches global memory.  workspace: wu_nn_radius_workspace_bytes(nq, nb, col_splits) bytes, aligned to 8
 * (0 for arguments out of range; pure host); ws_bytes is what the caller holds, a short one is refused.  Stream-ordered, caller-owned
 * buffers, no allocation, no synchronisation.  radius2 finite and >= 0 (NaN, inf and negative values are refused), 1 <= nq, nb <= 2^21,
 * self_offset = -1 or 0 <= self_offset <= nb - nq, ld >= D >= 1.  Non-finite features give a meaningless result, never an access outside a
 * buffer. */
size_t wu_nn_radius_workspace_bytes(int nq, int nb, int col_splits);
int wu_nn_radius_count(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, double radius2, int self_offset,
                       int upper_only, int col_splits, void* ws, size_t ws_bytes, long long* row_ptr, void* stream);
int wu_nn_radius_fill(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, double radius2, int self_offset,
                      int upper_only, int col_splits, void* ws, size_t ws_bytes, const long long* row_ptr, long long capacity, int* col,
                      double* dist2, void* stream);

/* ---- Per-row realism and rarity against a bank's k-NN balls (wu/retrieval.py: ball_scores) ----------------------------------------------------
 * r2 (nb doubles) are the bank's squared k-NN radii, what wu_knn_radii writes.  Per query row i, over the columns j < nb that self_offset
 * leaves in (as above), with d2_ij = d2(q_i, b_j):
 *     count[i]         = #{ j : d2_ij <= r2[j] }                      without a self_offset wu_prdc_counts' B[i], bit for bit;
 *     rarity_r2[i]     = min{ r2[j] : d2_ij <= r2[j] }, +inf when the row lies in no ball (Han et al. 2022: the smallest ball that holds it);
 *     rarity_index[i]  = its column, the smaller j on equal radii, -1 when there is none;
 *     realism_*[i]     : the maximiser over j of rho_ij = r2[j] / d2_ij, ONE IEEE fp64 division per pair, +inf when d2_ij == 0 whatever
 *                        r2[j] is, on equal rho the smaller j: realism_r2[i] = r2[j], realism_d2[i] = d2_ij, realism_index[i] = j.  The
 *                        realism score of Kynkaanniemi et al. 2019 is sqrt(rho), formed by the caller from the pair.
 * One walk of the same tiles, grid (query row tiles, col_splits), then a finish launch that merges the splits by the same total-order rules:
 * the result does not depend on col_splits or on the order workgroups finish in.  col_splits as above.  workspace:
 * wu_nn_ball_workspace_bytes(nq, nb, col_splits) bytes, aligned to 8 (0 for arguments out of range; pure host).  The limits are the join's,
 * and nb >= 2 with self_offset >= 0 (a maximiser must exist).  r2 is expected finite and >= 0; other values give meaningless scores. */
size_t wu_nn_ball_workspace_bytes(int nq, int nb, int col_splits);
int wu_nn_ball_scores(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, const double* r2, int self_offset,
                      int col_splits, void* ws, size_t ws_bytes, unsigned* count, double* rarity_r2, int* rarity_index, double* realism_r2,
                      double* realism_d2, int* realism_index, void* stream);

/* ---- Rank-aware Frechet distance on feature rows (wu/frechet.py): Tr sqrt(Sigma1 Sigma2) = ||A B^T||_* / sqrt((n1 - 1)(n2 - 1)) ------------
 * A, B are the centred rows of x1 (n1 x D fp32, row stride ld1) and x2 (n2 x D, ld2); A B^T is the double-centred cross-Gram matrix of the
 * raw rows, and its singular values come from a one-sided (Hestenes) Jacobi iteration: no covariance, no matrix square root, any rank.
 * The "vectors" are the rows of the set with FEWER rows (a tie goes to set 1): ns = min(n1, n2) <= 4096, nl = max(n1, n2) <= 2^21.
 *   wu_fd_cross_gram     V[i][j] = <p_i, q_j> (64 x 64 tiles on the fp64 matrix cores), then centred in place:
 *                        V[i][j] = ((V[i][j] - r_i / nl) - c_j / ns) + t / (ns nl), r row sums, c column sums, t their total.  V is the first
 *                        ns x ld doubles of `workspace`, row-major, ld = wu_fd_ld(n1, n2) >= nl.
 *   wu_fd_moments        mu (D doubles), dev2[i] = |x_i - mu|^2 (n doubles) and s[0] = sum_i dev2[i]: tr Sigma = s / (n - 1).
 *   wu_fd_jacobi_sweep   one sweep over the rows of ANY fp64 matrix V (ns x nl, row stride ld): zeroes rotations[0], then N = 2 ceil(ns / 2) - 1
 *                        launches, one per round-robin step, a workgroup per row pair: step s pairs (N, s) and ((s + k) mod N, (s - k + N)
 *                        mod N), k = 1 .. (N - 1) / 2; an index >= ns is the phantom of an odd ns.  With alpha = |p|^2, beta = |q|^2,
 *                        gamma = <p, q> (p the smaller index) and tol = sqrt(nl) 2^-53 a pair is left alone when
 *                        |gamma| <= tol sqrt(alpha) sqrt(beta); a vector whose squared norm is below 2^-969 (underflow has taken its
 *                        precision) is stored as zero and left alone; otherwise zeta = (beta - alpha) / (2 gamma),
 *                        t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (1 at zeta = 0), c = 1 / sqrt(1 + t^2), s = c t,
 *                        p <- c p - s q, q <- s p + c q, and rotations[0] grows by one (an integer atomic).  The caller reads rotations[0]
 *                        after the sweep and stops at 0.  Vectors up to 2048 long stay in registers; longer ones are read twice.
 *   wu_fd_finish         sigma[i] = sqrt(|v_i|^2) (ns doubles, index order, not sorted) and total[0] = their sum in index order.
 * Every floating-point sum runs in one fixed order (a thread's elements t, t + 256, .. in order, lanes l += l + off for off = 32 .. 1, the
 * four waves in wave order; column sums and means row by row): the same inputs give the same bits.  Every launch ends on its own: no grid
 * barrier, no cooperative launch.  workspace: wu_fd_workspace_bytes(n1, n2, D) bytes (V, then r, c, t); 0, and wu_fd_ld 0, for arguments
 * out of range.  Stream-ordered, caller-owned buffers, no allocation, no synchronisation.  n1, n2 >= 2, ld >= D >= 1. */
int wu_fd_ld(int n1, int n2);
size_t wu_fd_workspace_bytes(int n1, int n2, int D);
int wu_fd_cross_gram(const float* x1, int ld1, int n1, const float* x2, int ld2, int n2, int D, void* workspace, void* stream);
int wu_fd_moments(const float* x, int ldx, int n, int D, double* mu, double* dev2, double* s, void* stream);
int wu_fd_jacobi_sweep(double* V, int ld, int ns, int nl, unsigned* rotations, void* stream);
int wu_fd_finish(const double* V, int ld, int ns, int nl, double* sigma, double* total, void* stream);

/* ---- Paired content preservation (wu/paired.py): SSIM / MS-SSIM means and error sums of x against R conditioned outputs y --------------
 * x (B, C, H, W) with ELEMENT strides (xs_n, xs_c, xs_h, xs_w), y (R, B, C, H, W) with (ys_r, ys_n, ys_c, ys_h, ys_w); dtype WU_F32, WU_BF16
 * or WU_SSIM_U8.  A value is widened to fp64 and mapped v * scale + shift; L is the data range, C1 = (K1 L)^2, C2 = (K2 L)^2.  `window` is a
 * HOST array of k doubles (k odd, 3..11): it is copied into the kernels' argument struct, no device buffer.  All arithmetic in fp64, every
 * operation rounded on its own (no FMA), the valid filter along H first and then along W, taps in ascending order:
 *     mu_x = F(x), mxx = mu_x mu_x, myy, mxy likewise;  sx = F(x x) - mxx,  sy = F(y y) - myy,  sxy = F(x y) - mxy
 *     cs = (2 sxy + C2) / ((sx + sy) + C2),   ssim = ((2 mxy + C1) / ((mxx + myy) + C1)) cs        over (H - k + 1) x (W - k + 1) positions
 * levels = 1 or 5; between levels both images go through ((p00 + p01) + (p10 + p11)) * 0.25 with a zero row / column in FRONT of an odd
 * dimension (size s -> s / 2 + s % 2); levels = 5 needs min(H, W) > 16 (k - 1).
 *     ssim_mean, cs_mean (R, B, C, levels): the means of the two maps;   err (R, B, 2): sum (x - y)^2 and sum |x - y| over C H W values;
 *     ssim_map: NULL, or (R, B, C, H - k + 1, W - k + 1) for the level-0 ssim entries.
 * A workgroup owns a wu_ssim_tile_h() x wu_ssim_tile_w() output tile of one (n, c), filters x once and walks the R rows (where B C tiles
 * is too small to fill the device, the rows are split over several workgroups instead); no filtered map reaches global memory.  At most 2 * levels launches whatever B, R, C; per-tile sums go to `workspace` (wu_ssim_workspace_bytes, with the
 * pooled fp64 levels) and are folded in a fixed order: no atomics, the same inputs give the same bits, and a row's numbers do not depend
 * on R.  Stream-ordered, caller-owned buffers, no allocation, no synchronisation. */
#define WU_SSIM_U8 2
size_t wu_ssim_workspace_bytes(int B, int R, int C, int H, int W, int k, int levels);      /* 0 for anything out of range */
int wu_ssim_tile_h(void);
int wu_ssim_tile_w(void);
int wu_ssim_pairs(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, const void* y, long long ys_r,
                  long long ys_n, long long ys_c, long long ys_h, long long ys_w, int dtype, int B, int R, int C, int H, int W,
                  double scale, double shift, double L, double K1, double K2, const double* window, int k, int levels,
                  void* workspace, double* ssim_mean, double* cs_mean, double* err, double* ssim_map, void* stream);

/* ---- Sliced Wasserstein distance on Laplacian-pyramid patches (wu/swd.py; Karras et al. 2018) ------------------------------------------
 * Four stages, each stream-ordered on caller-owned buffers, no allocation, no synchronisation, no floating-point atomics: the same inputs
 * give the same bits.  tests/_swd_ref.py restates the arithmetic.  All pyramid arithmetic in fp64, every operation rounded on its own.
 *   wu_swd_descriptors   x (N, 3, H, W) with ELEMENT strides, dtype WU_F32, WU_BF16 or WU_SSIM_U8; a value is widened and mapped
 *                        v * scale + shift.  f = (1, 4, 6, 4, 1) / 16; the blur B is separable, along H first and then along W, taps in
 *                        ascending order, the border mirrored without repeating the edge sample (i < 0 -> -i, i >= n -> 2 (n - 1) - i).
 *                        G_0 = x, G_{l+1}[y, x] = B(G_l)[2y, 2x]; U_l = the same pass with taps 2 f over G_{l+1} with zeros stuffed between
 *                        its samples; L_l = G_l - U_l, L_{levels-1} = G_{levels-1}.  `positions` is a DEVICE array (levels, N, P, 2) of
 *                        centres (cy, cx), 3 <= cy <= H_l - 4, 3 <= cx <= W_l - 4 (the caller checks them; the kernel clamps).  desc is
 *                        (levels, N P, 147) float32: descriptor (n, p) of level l holds L_l[n][c][cy - 3 + dy][cx - 3 + dx] at
 *                        c * 49 + dy * 7 + dx.  Only G_1.. are stored (fp64, in the workspace); L_l is formed at the gathered pixels only.
 *                        H and W divisible by 2^(levels-1), every level at least 7 x 7, 1 <= levels <= 12, N P <= 2^21.
 *   wu_swd_normalize     stats[0..2] = mu_c, stats[3..5] = sigma_c: mean and population standard deviation of the 49 m values of channel c,
 *                        accumulated in fp64 in a fixed order; out = float((double(v) - mu_c) / sigma_c), 0 where sigma_c == 0 (out may be
 *                        desc itself).
 *   wu_swd_project_sort  sorted[j][:] = ascending sort of { <desc_i, dirs_j> : i < m } for the ndirs rows of dirs (ndirs, 147): products and
 *                        sums in fp64 on the fp32 operands (64 x 64 tiles on the fp64 matrix cores), then a segmented sort: blocks of
 *                        wu_swd_sort_block() keys are sorted on-chip, then merged pairwise over global memory.  dir_chunk directions are
 *                        handled per pass (0: the library chooses), which only sets the size of the temporary: the result does not depend
 *                        on it, bit for bit.  workspace: wu_swd_workspace_bytes(m, ndirs, dir_chunk).  1 <= m <= 2^21, 1 <= ndirs <= 4096.
 *   wu_swd_sort_columns  the sort of wu_swd_project_sort on its own: every row of keys (ncols, m), finite doubles, ascending and in place;
 *                        workspace: wu_swd_workspace_bytes(m, ncols, ncols) bytes.  Same ranges.
 *   wu_swd_distance      w[j] = mean_i |a[j][i] - b[j][i]| of two (ndirs, m) arrays, a fixed-order tree sum per direction.
 *   wu_swd_distance_unequal
 *                        a (ndirs, m1), b (ndirs, m2), rows ascending: w[j] = the exact W1 of the two empirical distributions, the integral
 *                        of |Fa^-1(t) - Fb^-1(t)| over t in [0, 1].  With x the longer row (ml keys), y the shorter (ms <= ml; x = a when
 *                        m1 == m2) and t in units of 1 / (ml ms), x_i owns [i ms, (i + 1) ms) and y_j owns [j ml, (j + 1) ml); in int64,
 *                        lo = i ms, hi = lo + ms, j0 = lo / ml, j1 = (hi - 1) / ml <= j0 + 1, cut = (j0 + 1) ml, w0 = min(hi, cut) - lo,
 *                        w1 = hi - min(hi, cut); w[j] = (sum_i w0 |x_i - y_j0| + w1 |x_i - y_j1|) / (double)(m1 m2): thread t of 256 adds
 *                        the two terms of i = t, t + 256, .. in that order (the second also when w1 == 0), then the fixed-order tree sum of
 *                        wu_swd_distance.  No search, no atomics; W(a, b) and W(b, a) are the same bits.  1 <= m1, m2 <= 2^21.
 * The *_workspace_bytes functions return 0 for anything out of range. */
int wu_swd_sort_block(void);
size_t wu_swd_pyramid_workspace_bytes(int N, int H, int W, int levels, int P);
int wu_swd_descriptors(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int H, int W,
                       double scale, double shift, int levels, const int* positions, int P, void* workspace, float* desc, void* stream);
size_t wu_swd_stats_workspace_bytes(int m);
int wu_swd_normalize(const float* desc, int m, void* workspace, float* out, double* stats, void* stream);
size_t wu_swd_workspace_bytes(int m, int ndirs, int dir_chunk);
int wu_swd_project_sort(const float* desc, int m, const float* dirs, int ndirs, int dir_chunk, void* workspace, double* sorted,
                        void* stream);
int wu_swd_sort_columns(double* keys, int m, int ncols, void* workspace, void* stream);
int wu_swd_distance(const double* a, const double* b, int m, int ndirs, double* w, void* stream);
int wu_swd_distance_unequal(const double* a, int m1, const double* b, int m2, int ndirs, double* w, void* stream);

/* ---- Radial power spectrum of image luma (wu/spectrum.py; Durall et al. 2020, Dzanic et al. 2020) ---------------------------------------
 * A 2-D DFT of any side up to 1024 as two matrix products against twiddle tables on the fp64 matrix cores, then the azimuthal average over
 * integer radial bins.  Stream-ordered on caller-owned buffers, no allocation, no synchronisation, no floating-point atomics: the same
 * inputs give the same bits, and an image's profile does not depend on which images share its call.  tests/_spectrum_ref.py restates the
 * arithmetic.  Every product and sum outside the matrix cores is rounded on its own.
 *   wu_spectrum_luma      x (N, C, H, W) with ELEMENT strides, C 1 or 3, dtype WU_F32, WU_BF16 or WU_SSIM_U8 -> planes (N, H, W) fp64:
 *                         s = (double(v) * scale + shift) / L; y = (0.299 s_R + 0.587 s_G) + 0.114 s_B (C = 1: y = s); with the window
 *                         tables wh (H doubles) and ww (W doubles), both DEVICE arrays or both NULL, y = (y * wh[i]) * ww[j].
 *   wu_spectrum_profiles_planes
 *                         planes (N, H, W) fp64; cw / sw (W doubles) and ch / sh (H doubles) are DEVICE tables of cos / sin(2 pi k / n).
 *                         Wh = W / 2 + 1.  Row stage: Tr[i][v] = sum_j y[i][j] cw[(v j) mod W], Ti[i][v] = -sum_j y[i][j] sw[(v j) mod W];
 *                         column stage: Xr[u][v] = sum_i (ch[(u i) mod H] Tr[i][v] + sh[(u i) mod H] Ti[i][v]),
 *                         Xi[u][v] = sum_i (ch[(u i) mod H] Ti[i][v] - sh[(u i) mod H] Tr[i][v]); P = Xr Xr + Xi Xi.  Entry (u, v) has
 *                         mirror weight 2 for 0 < 2 v < W and 1 otherwise, and radial bin k = isqrt(q M^2) / (H W) in int64 with
 *                         fu = u <= H / 2 ? u : u - H, q = fu^2 W^2 + v^2 H^2, M = min(H, W).  prof (N, K):
 *                         prof[n][k] = (sum of weight P over the bin) / (sum of weights) / (H W)^2, the sum taken per 64 x 64 tile (entries
 *                         in row-major order) and then over tiles ascending.  K must be wu_spectrum_bins(H, W).  spectrum_sum, when not
 *                         NULL, is (H, Wh) fp64 and receives spectrum_sum[u][v] += P[n][u][v] for n ascending (the caller zeroes it):
 *                         the column stage is then launched once per image and adds P in its epilogue, so no 2-D spectrum other than
 *                         that sum reaches memory.  workspace: wu_spectrum_workspace_bytes(N, H, W), the (N, H, 2 Wh) fp64
 *                         intermediate, the per-tile partial sums and the per-tile bin order.
 *   wu_spectrum_profiles  the same from the strided source: luma and window are applied while the row stage stages its tile, no fp64
 *                         plane exists in memory; bit for bit wu_spectrum_luma followed by wu_spectrum_profiles_planes.
 * 1 <= N <= 65535 (the column stage puts the image in grid.y), 1 <= H, W <= 1024.  wu_spectrum_workspace_bytes and wu_spectrum_bins return 0 for anything out of range. */
int wu_spectrum_bins(int H, int W);
size_t wu_spectrum_workspace_bytes(int N, int H, int W);
int wu_spectrum_luma(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int C, int H, int W,
                     double scale, double shift, double L, const double* wh, const double* ww, double* planes, void* stream);
int wu_spectrum_profiles_planes(const double* planes, int N, int H, int W, const double* cw, const double* sw, const double* ch,
                                const double* sh, int K, void* workspace, double* prof, double* spectrum_sum, void* stream);
int wu_spectrum_profiles(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int C, int H,
                         int W, double scale, double shift, double L, const double* wh, const double* ww, const double* cw,
                         const double* sw, const double* ch, const double* sh, int K, void* workspace, double* prof,
                         double* spectrum_sum, void* stream);

/* ---- Colour-transfer baselines (wu/colour.py): histogram matching and sliced optimal transport of pixel colours --------------------------
 * A "virtual image" g = r B + b is input image b on its way to target r; its state is (3, n) fp64 in [0, 1] units, n = H W.  `first` is the
 * g of the first state of a call, so that any run of virtual images can be in flight.  All arithmetic in fp64, every operation rounded on
 * its own (no FMA); no atomics and no sums across threads: the same inputs give the same bits.  tests/_colour_ref.py restates it.
 * `rotation` is a HOST array of 9 doubles, row a = axis a; it is copied into the kernels' arguments.
 *   wu_colour_ot_load          x (B, 3, H, W) with ELEMENT strides, dtype WU_F32, WU_BF16 or WU_SSIM_U8 -> state (nimg, 3, n):
 *                              s = (double(v) * scale + shift) / L; state v reads image (first + v) % B.
 *   wu_colour_ot_palette_keys  palette (npal, P, 3) fp64 -> keys (npal * 3, P): key_a = (R[a][0] s_0 + R[a][1] s_1) + R[a][2] s_2, then
 *                              every row sorted ascending by wu_swd_sort_columns.  workspace: wu_colour_ot_workspace_bytes(1, 1, npal, P).
 *   wu_colour_ot_step          one iteration on nimg states in place: the keys of every state are projected and sorted (the same sort), and
 *                              per pixel and axis a, among the n keys of its image, lo = #{key' < key}, hi = #{key' <= key},
 *                              t = ((lo + hi) P) / (2 n) in int64, delta_a = q[t] - key_a with q the sorted keys of axis a of palette
 *                              classes[v] (a DEVICE array of nimg ints in 0..npal-1; the caller checks them, an image with a class outside
 *                              is left unchanged); then d_c = (delta_0 R[0][c] + delta_1 R[1][c]) + delta_2 R[2][c] and
 *                              s_c = s_c + step * d_c.  workspace: wu_colour_ot_workspace_bytes(nimg, n, npal, P).
 *   wu_colour_ot_store         u = min(max(s, 0), 1), v = lo + u * span, rint(v) (half to even) when round_int or for WU_SSIM_U8, then
 *                              fp64 -> fp32 (-> bf16), nearest-even, into y (R, B, 3, H, W) with ELEMENT strides: state v goes to
 *                              r = (first + v) / B, b = (first + v) % B.
 * 1 <= n, P <= 2^21.  wu_colour_ot_workspace_bytes returns 0 for anything out of range.  Stream-ordered, caller-owned buffers, no
 * allocation, no synchronisation. */
size_t wu_colour_ot_workspace_bytes(int nimg, int n, int npal, int P);
int wu_colour_ot_load(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int B, int H, int W,
                      double scale, double shift, double L, long long first, int nimg, double* state, void* stream);
int wu_colour_ot_palette_keys(const double* palette, int npal, int P, const double* rotation, double* keys, void* workspace, void* stream);
int wu_colour_ot_step(double* state, int nimg, int n, const double* palette_keys, int npal, int P, const int* classes,
                      const double* rotation, double step, void* workspace, void* stream);
int wu_colour_ot_store(const double* state, long long first, int nimg, void* y, long long ys_r, long long ys_n, long long ys_c,
                       long long ys_h, long long ys_w, int dtype, int B, int H, int W, double lo, double span, int round_int, void* stream);

/* ---- Regraining (wu/colour.py; Pitie, Kokaram, Dahyot, CVIU 2007, section 5): keep the transferred colours, take the original's gradients -----
 * On states as wu_colour_ot_load writes them: `state` (nimg, 3, n) holds the transfer IT (unclipped) on entry and the result IR on return,
 * `original` (nimg, 3, n) the original I0, n = H W <= 2^21.  fp64, every operation rounded on its own, no FMA; tests/_regrain_ref.py restates
 * it and the result is bit-identical.  sh(a, dy, dx)(y, x) = a(clamp(y + dy), clamp(x + dx)): every neighbour read clamps at the image edge.
 *   levels   level 0 is H x W; level l + 1 exists iff l + 1 < n_iters and ceil(h_l / 2) > min_side and ceil(w_l / 2) > min_side, and has
 *            those ceilings as its size.  wu_colour_regrain_levels applies the rule on the host (0 for arguments out of range: H, W >= 1,
 *            1 <= n_iters <= 6, min_side >= 0); wu_colour_regrain takes the COUNT, 1..6, and halves (rounding up) that many times.
 *   down     per axis (a[2d] + a[min(2d + 1, last)]) * 0.5, rows first, then columns.
 *   up       per axis a[d / 2] * 0.75 + a[o] * 0.25, o = d / 2 - 1 for even d and d / 2 + 1 for odd d, clamped; rows first, then columns.
 *   rec(IR, I0, IT, l): if level l + 1 exists, c0 = down(IR), c1 = rec(c0, down(I0), down(IT), l + 1), IR = IR + up(c1 - c0); then
 *            IR = solve(IR, I0, IT, iters[l], l).  The top call starts from IR = IT.  A coarse-grid CORRECTION: IR is not replaced.
 *   solve    gx = sh(I0, 0, +1) - sh(I0, 0, -1), gy = sh(I0, +1, 0) - sh(I0, -1, 0); q_c = gx_c gx_c + gy_c gy_c; dI = sqrt((q_0 + q_1) + q_2);
 *            psi = min((256 dI) / 5, 1); phi = (30 * 2^-l) / (1 + (10 dI) / smoothness); for the neighbours j = up (-1, 0), down (+1, 0),
 *            left (0, -1), right (0, +1): phi_j = (sh(phi, j) + phi) * 0.5; den = ((((psi + phi_1) + phi_2) + phi_3) + phi_4) + 2^-52;
 *            b = (((psi IT + phi_1 (I0 - sh(I0, 1))) + phi_2 (I0 - sh(I0, 2))) + phi_3 (..)) + phi_4 (..) per channel; one iteration
 *            (Jacobi: every read is of the previous iterate): a = (((b + phi_1 sh(IR, 1)) + phi_2 sh(IR, 2)) + phi_3 sh(IR, 3)) + phi_4 sh(IR, 4),
 *            IR = (a / den) * 0.8 + 0.2 * IR.  The weights are shared by the three channels.
 * `iters_host` is a HOST array of `levels` counts, finest level first, each in 1..2^20.  smoothness > 0.  The result is not clipped.
 * workspace: wu_colour_regrain_workspace_bytes(nimg, H, W, levels), 0 for anything out of range (133 bytes per pixel and image at four
 * levels).  No atomics, no sum across threads: two runs, any split of the images into calls and any tile size give the same bytes.
 * Stream-ordered, caller-owned buffers, no allocation, no synchronisation; arguments are refused before any launch. */
size_t wu_colour_regrain_workspace_bytes(int nimg, int H, int W, int levels);
int wu_colour_regrain_levels(int H, int W, int n_iters, int min_side);
int wu_colour_regrain(double* state, const double* original, int nimg, int H, int W, int levels, const int* iters_host, double smoothness,
                      void* workspace, void* stream);

/* ---- Linear colour maps (wu/colour.py): mean / sigma transfer (Reinhard et al. 2001) and the Monge-Kantorovich map (Pitie & Kokaram 2007) ---
 *   wu_colour_moments       nsets point sets of n points: channel c of point i of set s is points[s 3 n + i stride_point + c stride_channel];
 *                           (stride_point, stride_channel) is (1, n) for the planar state (nimg, 3, n) or (3, 1) for palettes (C, P, 3).
 *                           moments_out (nsets, 12): mu (3), then the 3 x 3 covariance, row-major and symmetric.  Two passes: mu = S / n, then
 *                           Sigma_ab = (sum_i (s_ia - mu_a) (s_ib - mu_b)) / n for a <= b (the population form: n = 1 gives 0).
 *                           THE ORDER OF EVERY SUM depends on n alone: with the addends padded by +0.0 to a multiple of 4096, chunk k holds
 *                           addends 4096 k .. 4096 k + 4095; in a chunk, lane t (0..255) adds addends t, t + 256, .., t + 3840 in that order
 *                           to +0.0, and the 256 lanes are folded by v[t] = v[t] + v[t + s] for s = 128, 64, .., 1; the chunk sums, padded
 *                           by +0.0 to a multiple of 256, go the same way: lane t adds chunk sums t, t + 256, .. in order, then the fold.
 *                           workspace: wu_colour_moments_workspace_bytes(nsets, n) (0 out of range: 1 <= nsets <= 65535, 1 <= n <= 2^21).
 *   wu_colour_linear_apply  s <- mu_t + A (s - mu_s) on every state v, with (mu_s, Sigma_s) = state_moments[v] and (mu_t, Sigma_t) =
 *                           palette_moments[classes[v]] (a DEVICE array; an image with a class outside 0..npal-1 is left unchanged):
 *                           d = s - mu_s, s_c = ((A_c0 d_0 + A_c1 d_1) + A_c2 d_2) + mu_t_c.
 *                           WU_COLOUR_MEANSTD: A = diag(sqrt(Sigma_t_cc / max(Sigma_s_cc, eps_var))).
 *                           WU_COLOUR_MKL: A = Si ((S Sigma_t) S)^(1/2) Si, S = f(Sigma_s) with sqrt(max(lambda, eps_var)), Si with its
 *                           reciprocal 1 / sqrt(max(lambda, eps_var)), the inner root with sqrt(max(lambda, 0)).
 *                           f(M) = V diag(f) V^T from a cyclic Jacobi on M's upper triangle: exactly 8 sweeps over (p, q) = (0,1), (0,2), (1,2),
 *                           a rotation skipped when a_pq == 0, else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
 *                           sqrt(theta theta + 1)) with sign(0) = +1, c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0,
 *                           (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), and for every row i of V (v_ip, v_iq) = (c v_ip - s v_iq,
 *                           s v_ip + c v_iq).  Entry (i, j), i <= j, of f(M) is ((V_i0 f_0) V_j0 + (V_i1 f_1) V_j1) + (V_i2 f_2) V_j2, mirrored;
 *                           a matrix product entry is (x_i0 y_0j + x_i1 y_1j) + x_i2 y_2j.  No trigonometry: tests/_regrain_ref.py gives
 *                           the same bits.  The map is formed on the device: nothing is read back.
 * fp64, no FMA, no atomics.  Stream-ordered, caller-owned buffers, no allocation, no synchronisation. */
#define WU_COLOUR_MEANSTD 0
#define WU_COLOUR_MKL 1
size_t wu_colour_moments_workspace_bytes(int nsets, int n);
int wu_colour_moments(const double* points, long long stride_point, long long stride_channel, int nsets, int n, double* moments_out,
                      void* workspace, void* stream);
int wu_colour_linear_apply(double* state, int nimg, int n, const double* state_moments, const double* palette_moments, int npal,
                           const int* classes, int mode, double eps_var, void* stream);

/* layout helpers for the module boundary: NHWC `dtype` <-> NCHW fp32 (feature maps returned by
 * SNDisc.forward, disc.py:38; gradients flowing back into them). */
int wu_nhwc_to_nchw_f32(const void* x, int ldx, float* y_nchw, int N, int H, int W, int C, int dtype, void* stream);
int wu_nchw_f32_to_nhwc(const float* x_nchw, void* y, int ldy, int N, int H, int W, int C, int dtype, void* stream);

/* ---- GIF encoding (the animation of the demo tables: wu.infer_driver.save_demo(..., gif_encoder=)) ------------------------------------
 * T frames (uint8, interleaved RGB, any non-negative element strides) become T GIF89a image blocks -- graphic control extension, image
 * descriptor, a 256-entry local colour table, LZW data in 255-byte sub-blocks -- in five launches and one stream-ordered memset, whatever
 * T and the frame size.  Per frame, independently: a 32768-bin histogram over the top 5 bits of each channel (count and 64-bit channel
 * sums), median cut over the occupied bins down to at most 256 boxes (the box with the largest count x extent is cut at the median of
 * its longest axis), palette entry = rounded mean of the box, index = the box of the pixel's bin (no dithering, no nearest-colour
 * search); then GIF LZW with an 8-bit minimum code size over segments of wu_gif_enc_segment_pixels() indices, every segment starting
 * from the fresh dictionary and ending in a Clear code (the last in the end-of-information code), the segments' bit strings joined at
 * bit granularity.  All integer, deterministic: the blocks equal tests/_gif_enc_ref.py byte for byte.  The host puts `GIF89a`, the
 * logical screen descriptor, the loop extension and the trailer around the blocks (wu/gif_enc.py). */
size_t wu_gif_enc_segment_pixels(void);     /* 8192 */
/* Caller-owned workspace for T frames of H x W (0 for a shape that cannot be encoded: over 65535 on a side or over 2^26 pixels), and the
 * byte distance between two frames' blocks in `out`: the exact worst case of a block, every pixel a 12-bit code and four more codes per
 * segment -- with nseg = ceil(H W / 8192) and P = ceil(12 (H W + 4 nseg) / 8):  8 + 10 + 768 + 1 + P + ceil(P / 255) + 1. */
size_t wu_gif_enc_workspace_bytes(int T, int H, int W);
size_t wu_gif_enc_block_stride(int H, int W);
/* Encodes the frames: pixel (t, y, x), channel c at frames[t * stride_t + y * stride_y + x * stride_x + c * stride_c].  Frame t's block
 * starts at out + t * wu_gif_enc_block_stride(H, W); result_dev[t] = its byte count.  delay_cs: the frame delay in 1/100 s (0..65535).
 * Stream-ordered: no allocation, no synchronisation. */
int wu_gif_enc_encode(const uint8_t* frames, long long stride_t, long long stride_y, long long stride_x, long long stride_c, void* workspace,
                      size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int T, int H, int W, int delay_cs,
                      void* stream);
/* The same encoder with its quality options; flags == 0 writes the blocks of wu_gif_enc_encode (same stride; the workspace is a little
 * larger, by the info) through the kernels of the options.  All rules
 * are integer and restated in tests/_gif_quality_ref.py; still one memset and five launches, stream-ordered, nothing allocated.
 *   WU_GIF_NEAREST  the index of a pixel is the palette entry, among those in use, at the smallest squared Euclidean distance in 8-bit RGB
 *                   (lowest index among equals; a brute-force search over the palette in LDS in the LZW kernel's map phase) instead of the
 *                   median-cut box of its histogram bin.
 *   WU_GIF_ORDERED  with WU_GIF_NEAREST only: the colour searched is clamp(pixel_c + floor((2 M + 1 - 64) A_c / 128), 0, 255).  M, 0..63, is
 *                   the 8 x 8 threshold of the pixel's position in the FRAME: with x_b, y_b bit b of x & 7, y & 7,
 *                   M = sum over b = 0..2 of ((x_b ^ y_b) << 1 | y_b) << 2 (2 - b).  A_c = min(16, 8 (hi_c - lo_c + 1)), lo / hi the final
 *                   tight 5-bit bounds of the box of the pixel's bin.
 *   WU_GIF_EXACT    a frame (under WU_GIF_GLOBAL: the animation) with at most 256 distinct colours gets exactly those as its palette, in
 *                   ascending order of r << 16 | g << 8 | b, zeros behind, index = rank: reproduced bit for bit, no median cut, no dither.
 *                   The colours are counted in a 1024-slot open-addressed set beside the histogram; 257 colours end the counting.
 *   WU_GIF_GLOBAL   one histogram, one median cut or exact set and one palette for all T frames (T H W < 2^32): palette_dev receives its 768
 *                   bytes for a global colour table, and the blocks carry no local table (image descriptor flags 0x00; the fixed part of a
 *                   block is 8 + 10 + 1 bytes, and wu_gif_enc_block_stride_ex is 768 bytes less).
 * palette_dev: 768 bytes, needed under WU_GIF_GLOBAL only (else may be null).  info_dev: 2 T ints; info_dev[2 t] = palette entries in use
 * for frame t, info_dev[2 t + 1] = 1 if the frame took the exact path, else 0. */
#define WU_GIF_NEAREST 1
#define WU_GIF_ORDERED 2
#define WU_GIF_EXACT 4
#define WU_GIF_GLOBAL 8
size_t wu_gif_enc_workspace_bytes_ex(int T, int H, int W, int flags);      /* 0: bad shape or flags */
size_t wu_gif_enc_block_stride_ex(int H, int W, int flags);
int wu_gif_enc_encode_ex(const uint8_t* frames, long long stride_t, long long stride_y, long long stride_x, long long stride_c, void* workspace,
                         size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int T, int H, int W, int delay_cs, int flags,
                         uint8_t* palette_dev, int* info_dev, void* stream);

/* ---- LPIPS perceptual distance (wu/lpips.py; Zhang et al. 2018, net = alex, version 0.1) -------------------------------------------------
 * tests/_lpips_ref.py restates the arithmetic.  The AlexNet trunk itself runs on wu_conv_kxk_fwd / wu_pool3x3_fwd; these are the two ends.
 *   wu_lpips_input   src (N, 3, H, W) with ELEMENT strides, src_dtype WU_F32, WU_BF16 or WU_LPIPS_U8 -> dst, the dense (N, H, W, 16) network
 *                    input in `dtype` storage.  In float32, every operation rounded on its own (no FMA): t = v * scale + offset, then
 *                    u_c = (t - shift_c) / scale_c with shift = (-.030, -.088, -.188), scale = (.458, .448, .450); channels 3..15 are zero.
 *   wu_lpips_head    one layer's distance of fx (B, h, w, C) ld = ldx against the R rows of fy (R, B, h, w, C) ld = ldy, row r at
 *                    fy + r * fy_row_stride elements; `weight` (C,) fp32.  Features are widened to fp64; per pixel, a = fx, b = fy:
 *                        n_a = sqrt(sum_c a_c^2),  ah_c = a_c / (n_a + 1e-10)  (likewise bh),   d = sum_c w_c (ah_c - bh_c)^2
 *                    out[r * ldo + b] = (sum over the h w pixels of d) / (h w).  C % 16 == 0, 16 <= C <= 512; ldx, ldy multiples of 8, fx / fy
 *                    16-byte aligned (a channel slice of a wider buffer is ptr + c0, ld = total channels).
 *   wu_lpips_pairs   the same distance between all rows of f (R, B, h, w, C): out[(i * R + j) * ldo + b] for i < j, entry (j, i) a copy of it,
 *                    exact zeros on the diagonal.  A block of 4 / 2 / 1 rows i (for C <= 128 / <= 256 / above) is held in registers while
 *                    the rows j behind it walk past, each normalised once per block: pair (i, j) is formed exactly as wu_lpips_head forms
 *                    (x = row i, y = row j), from the direct differences (no Gram identity), so the result of a pair does not depend on
 *                    R or on how the rows are blocked.  2 <= R <= 64.
 * A workgroup owns wu_lpips_tile_pixels() pixels of one image: 16 lanes share a pixel, each lane keeps its channels of the normalised x
 * vector in registers while the rows walk past.  Per-wave partial sums go to `workspace` (wu_lpips_workspace_bytes(B, R, h, w, pairs), 0
 * for anything out of range) and one wave per output folds them in a fixed order: no atomics, the same inputs give the same bits, and an
 * entry does not depend on B or R.  Stream-ordered, caller-owned buffers, no allocation, no synchronisation. */
#define WU_LPIPS_U8 2
int wu_lpips_tile_pixels(void);
size_t wu_lpips_workspace_bytes(int B, int R, int h, int w, int pairs);
int wu_lpips_input(const void* src, long long s_n, long long s_c, long long s_h, long long s_w, int src_dtype, int N, int H, int W,
                   float scale, float offset, void* dst, int dtype, void* stream);
int wu_lpips_head(const void* fx, int ldx, const void* fy, int ldy, long long fy_row_stride, const float* weight, int dtype, int B, int R,
                  int h, int w, int C, void* workspace, double* out, int ldo, void* stream);
int wu_lpips_pairs(const void* f, int ld, long long row_stride, const float* weight, int dtype, int B, int R, int h, int w, int C,
                   void* workspace, double* out, int ldo, void* stream);

/* ---- Full-resolution output through the fast colour guided filter (wu/guided.py; He, Sun, Tang 2013; He, Sun 2015) ----------------------
 * tests/_guided_ref.py restates the arithmetic.  All of it in fp64, every operation rounded on its own (no FMA), no atomics: the same
 * inputs give the same bits and a row's numbers do not depend on R.  Stream-ordered, caller-owned buffers, no allocation, no
 * synchronisation.
 *   wu_guided_coeffs   guide I (N, 3, hl, wl) fp32 with ELEMENT strides, mapped v * g_scale + g_shift; targets p (R, N, 3, hl, wl) of
 *                      t_dtype WU_F32 or WU_BF16 with ELEMENT strides, mapped v * t_scale + t_shift.  box(v) = the mean over the
 *                      (2r+1)^2 window clipped to the image: the in-range taps of a row summed left to right, those row sums summed top to
 *                      bottom, ONE division by count_y * count_x.  Per pixel: mI_k = box(I_k); S_jk = box(I_j I_k) - mI_j mI_k, eps added
 *                      to the diagonal; with S = [[a b c] [b d e] [c e f]] the cofactors c00 = d f - e e, c01 = c e - b f, c02 = b e - c d,
 *                      c11 = a f - c c, c12 = b c - a e, c22 = a d - b b, det = (a c00 + b c01) + c c02, inv_jk = c_jk / det.  Per row and
 *                      output channel c: cov_k = box(I_k p_c) - mI_k box(p_c); a_ck = (inv_k0 cov_0 + inv_k1 cov_1) + inv_k2 cov_2;
 *                      b_c = box(p_c) - ((a_c0 mI_0 + a_c1 mI_1) + a_c2 mI_2).  coeffs (R, N, 12, hl, wl) fp64: box(a_ck) at map 3 c + k,
 *                      box(b_c) at map 9 + c.  r >= max(hl, wl) is one global regression.  SIX launches whatever N and R, FIVE for r <= 8 (the
 *                      last two passes are then one tiled launch; the same bits); the guide's moments and inverse are formed once per image.  `workspace`: wu_guided_workspace_bytes(N, R, hl, wl) bytes.
 *   wu_guided_apply    photos (N, Hmax, Wmax, 3) uint8, image n of size sizes[2 n] x sizes[2 n + 1] (h, w): `sizes_host` is checked on the
 *                      host, `sizes_dev` is the same array in device memory, read by the kernel.  Output pixel (Y, X) of image n:
 *                      vy = (Y + 0.5) (hl / h) - 0.5 clamped to [0, hl - 1], y0 = floor(vy), y1 = min(y0 + 1, hl - 1), fy = vy - y0, the
 *                      same in x; each coefficient top = v00 + (v01 - v00) fx, bot = v10 + (v11 - v10) fx, top + (bot - top) fy;
 *                      I_k = byte_k / 255.0; q_c = ((A_c0 I_0 + A_c1 I_1) + A_c2 I_2) + b_c.  Exactly one of out_u8 (R, N, Hmax, Wmax, 3),
 *                      bytes (int)min(max(q 255, 0), 255) (truncation), and out_f32 (R, N, 3, Hmax, Wmax), (float)q; nothing outside an
 *                      image's (h, w) is written.  ONE launch: a workgroup owns a wu_guided_tile_h() x wu_guided_tile_w() tile of a
 *                      photograph, reads its pixels once, keeps the low-resolution coefficients it needs in LDS and walks the R rows.
 * Argument errors (r < 0, eps <= 0, a zero size, (h, w) beyond (Hmax, Wmax), a NULL pointer, an unknown dtype) return a negative code
 * before anything touches the device. */
size_t wu_guided_workspace_bytes(int N, int R, int hl, int wl);      /* 0 for anything out of range */
int wu_guided_tile_h(void);
int wu_guided_tile_w(void);
int wu_guided_coeffs(const float* guide, long long gs_n, long long gs_c, long long gs_h, long long gs_w, double g_scale, double g_shift,
                     const void* targets, long long ts_r, long long ts_n, long long ts_c, long long ts_h, long long ts_w, int t_dtype,
                     double t_scale, double t_shift, int N, int R, int hl, int wl, int r, double eps, void* workspace, double* coeffs,
                     void* stream);
int wu_guided_apply(const double* coeffs, int N, int R, int hl, int wl, const unsigned char* photos, int Hmax, int Wmax,
                    const int* sizes_host, const int* sizes_dev, unsigned char* out_u8, float* out_f32, void* stream);

/* ---- Antialiased resampling in front of the metrics (wu/resample.py; csrc/resample.hip) ------------------------------------------------
 * Pillow's ImagingResample (libImaging/Resample.c: horizontal pass, rounded intermediate, vertical pass; a pass between equal sizes is
 * skipped) on a ragged batch, ONE launch, no intermediate image in global memory; tests/_resample_ref.py restates the arithmetic.
 * Bit-identical to Image.resize on RGB uint8 (8-bit mode: 22-bit fixed-point coefficients, uint8 intermediate) and to Image.resize
 * on each channel as a mode 'F' image (float mode: float64 sums in ascending source order, float32 intermediate, no clipping).
 *   src        src_kind 0: uint8, 1: float32, 2: bf16; image n's sample (y, x, c) is element src_off + y s_row + x s_col + c s_ch.  A float
 *              source is mapped to 0..255 in float32 as x * 255.0f, or with WU_RESAMPLE_RANGE_PM1 as x * 127.5f + 127.5f (two roundings);
 *              in 8-bit mode it is then clamped to [0, 255] and truncated (wu.infer_driver.to_uint8).
 *   workspace  N descriptors of wu_resample_desc_bytes() (= 64) bytes, then the tables; `descs_host` is the same N descriptors in host
 *              memory, checked before anything touches the device:
 *                  int64 src_off, s_row, s_col, s_ch; int32 src_h, src_w, hb, hk, vb, vk, kx, ky;
 *              hb / vb: byte offsets in the workspace of int32 bounds[out][2] = {first source index, count}; hk: coefficients [kx][Wout]
 *              (tap-major), vk: [Hout][ky]; float64 in float mode, int32 (normalize_coeffs_8bpc) in 8-bit mode.  kx == 0 / ky == 0: that
 *              pass is skipped (src_w == Wout / src_h == Hout).  The caller builds the tables (precompute_coeffs) on the host.
 *   flags      WU_RESAMPLE_MODE_U8 | epilogue << 4 | band << 8 | WU_RESAMPLE_NORMALIZE | WU_RESAMPLE_RANGE_PM1.  band: output rows per
 *              workgroup, 1..wu_resample_max_band(), 0 = the default; every band height gives the same bits.
 *   epilogues  WU_RESAMPLE_OUT_NHWC_U8 (N, Hout, Wout, 3) uint8, 8-bit mode only; WU_RESAMPLE_OUT_RAW (N, 3, Hout, Wout) fp32, Pillow's
 *              value itself; _UNIT: clip(v, 0, 255) / 255.0f; _NORM: (unit - 0.5f) / 0.5f; _INCEPTION: unit, then with
 *              WU_RESAMPLE_NORMALIZE (float)(2.0 * unit - 1.0), into (N, Hout, Wout, cpad) of dst_dtype with pixel stride ldy, channels
 *              3..cpad-1 zero -- what wu_inception_input writes for the same (0, 1) image of the network's size.
 * Hout, Wout <= 1024; N * Hout * Wout < 2^31; a source row that takes a horizontal pass must fit 64 KiB of LDS (21845 pixels as bytes,
 * 5461 as float32: a float source in float mode). */
#define WU_RESAMPLE_MODE_U8 1
#define WU_RESAMPLE_OUT_NHWC_U8 0
#define WU_RESAMPLE_OUT_RAW 1
#define WU_RESAMPLE_OUT_UNIT 2
#define WU_RESAMPLE_OUT_NORM 3
#define WU_RESAMPLE_OUT_INCEPTION 4
#define WU_RESAMPLE_NORMALIZE (1 << 16)
#define WU_RESAMPLE_RANGE_PM1 (1 << 17)
size_t wu_resample_desc_bytes(void);
int wu_resample_max_band(void);
size_t wu_resample_workspace_bytes(int N, size_t table_bytes);       /* 0 for N <= 0 */
int wu_resample(const void* src, int src_kind, const void* descs_host, const void* workspace, size_t workspace_bytes, int N, int Hout,
                int Wout, void* dst, int ldy, int cpad, int dst_dtype, int flags, void* stream);

/* ---- instrumentation (bench.py roofline leg) -------------------------------------------------
 * While enabled, the launchers of the kernel families in `family_mask` (bit f = family f) bracket each
 * launch with hipEvents on the launch stream (events come from a pool created by wu_prof_begin; nothing
 * is allocated per launch).  wu_prof_query synchronises on a family's events and returns its number of
 * launches, summed duration, and summed ALGORITHMIC flops / bytes (DESIGN.md gives the per-launch
 * formulas).  One kernel (template instantiation) per family, so the totals match one rocprofv3 row. */
#define WU_FAM_CONV_FWD 1    /* conv3x3_mfma_kernel<T,1,false>: forward convs */
#define WU_FAM_WGRAD 2       /* conv3x3_wgrad_kernel<T,1,P> */
#define WU_FAM_CONV_DGRAD 3  /* conv3x3_mfma_kernel<T,1,true>: gated data-gradient pass */
#define WU_FAM_CONV_S2 4     /* conv3x3_mfma_kernel<T,2,false>: discriminator stride-2 forward */
#define WU_FAM_WGRAD_S2 5    /* conv3x3_wgrad_kernel<T,2,P> */
#define WU_FAM_CONV1X1 6     /* conv1x1_mfma_kernel<T>: pointwise convs of the estimator */
#define WU_FAM_GRID 7        /* the three launches of wu_grid_compose (bytes: the fill only; the cells' sizes are device data) */
int wu_prof_begin(unsigned family_mask, int max_launches);
int wu_prof_query(int family, int* launches, double* total_ms, double* total_flops, double* total_bytes);
int wu_prof_end(void);

#ifdef __cplusplus
}
#endif
#endif
