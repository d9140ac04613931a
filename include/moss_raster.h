/*
 * moss_raster.h -- C ABI of the MI355X (gfx950) differentiable Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary.  Each entry point replaces one function of the reference's native API
 * (3DHumanRehab/MOSS, submodules/diff-gaussian-rasterization = "DGR/", submodules/simple-knn = "SKNN/"),
 * with the same arguments in the same order and the same meaning; only C++-isms are flattened:
 *   - std::function<char*(size_t)> buffer growers  ->  a C callback + user pointer (moss_alloc_fn),
 *   - exceptions                                    ->  negative return code + moss_last_error(),
 *   - the implicit CUDA legacy default stream       ->  an explicit hipStream_t passed as void*.
 * All pointers are DEVICE pointers to contiguous fp32 (int32 for radii) unless stated otherwise; an absent
 * optional input is NULL (DGR/rasterize_points.cu passes the null data_ptr() of an empty tensor).
 * No torch types appear here.  The rasterizer entry points are bound by the compiled PyTorch-ROCm extension
 * moss_amd/csrc/torch_binding.cpp (the counterpart of DGR/rasterize_points.cu); the side kernels (k-NN, loss, AdamW,
 * densification statistics) by ctypes in moss_amd/_lib.py.
 *
 * The three scratch buffers are opaque to the caller exactly as in the reference (their internal layout is
 * this library's own); the caller must keep them alive and unmodified between forward and
 * backward, as the reference's autograd ctx does (DGR/diff_gaussian_rasterization/__init__.py:97).
 */
#ifndef MOSS_RASTER_H
#define MOSS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version 2 (round 3): the frame state is an ARGUMENT of the asynchronous forwards (version 1 armed it per host thread through
 * moss_raster_frame_state(), removed); the `debug` argument is a bit set (MOSS_DEBUG_*); moss_adamw_state_bytes() replaces the
 * caller's knowledge of the device-step block's size (288 bytes in early version-1 builds, 9216 later); diagnostics
 * (environment knobs, stamp buffers) exist only in -DMOSS_DIAG builds.  A binding compiled against another version must refuse to
 * load: compare ITS compile-time MOSS_ABI_VERSION with moss_abi_version(). */
/* ABI 5 (round 5): two more bits of `debug` -- MOSS_DEBUG_EXACT_MATH, MOSS_DEBUG_TRACE (below) -- and moss_raster_binning_bytes
 * follows the slimmer gradient-record layout.  No signature changed. */
/* ABI 6 (round 6): MOSS_FORWARD_ONLY (a bit of the forward entry points' `debug` argument) + moss_raster_binning_bytes_forward_only;
 * moss_fused_adamw gained sh_active_degree / sh_inactive_zero and moss_adamw_flat_ex takes the same two per segment (degree-aware SH
 * traffic: coefficients above the highest degree ever active are never read or written when they are known to be zero);
 * moss_photometric_loss_roi (MOSS's own loss expression: bound_mask selection, bounding-rectangle crop) and moss_adamw_multi (up to eight
 * tensors with buffers of their own in one launch) are new entry points. */
/* ABI 7: the rasterizer's positional variants collapse into moss_raster_forward_ex / moss_raster_backward_ex (one argument block per
 * direction; capacity 0 is refused), and the positional flat AdamW forms into moss_adamw_flat_ex (the map of the
 * removed names).  moss_raster_forward / moss_raster_backward keep the reference's signatures. */
#define MOSS_ABI_VERSION 7
/* Version 3 (round 4): EVERY forward / backward entry point takes the `debug` bit set (version 2: only moss_raster_forward /
 * moss_raster_backward did, so MOSS_DEBUG_NO_BLOCK_CULL was silently dropped on the _async / _tf / _raw paths: last argument before
 * `stream`); moss_adamw_flat_guarded (an optimizer step that a dropped frame turns into a no-op); MOSS_RAW_POSE and the
 * `translation` / `dL_dtranslation` arguments of the _raw entry points (the canonical positions are posed inside the op). */

/* error codes (negative returns) */
#define MOSS_ERR_INVALID_ARG   (-1)   /* bad shape / null where required (AT_ERROR in DGR/rasterize_points.cu:57-59) */
#define MOSS_ERR_HIP           (-2)   /* a HIP runtime call or kernel failed (CHECK_CUDA, DGR/cuda_rasterizer/auxiliary.h:166-173) */
#define MOSS_ERR_ALLOC         (-3)   /* an allocation callback returned NULL */
#define MOSS_ERR_PREFILTERED   (-4)   /* a point was culled although `prefiltered` was set (__trap in auxiliary.h:156-160) */
#define MOSS_ERR_UNSUPPORTED   (-5)   /* e.g. no colours for NUM_CHANNELS != 3 (DGR/cuda_rasterizer/rasterizer_impl.cu:244-247) */

/* Replaces std::function<char*(size_t)> (DGR/cuda_rasterizer/rasterizer.h:32-34; grown by resizeFunctional,
 * DGR/rasterize_points.cu:27-33).  Must return a device pointer to at least nbytes, 256-byte aligned, or NULL. */
typedef char* (*moss_alloc_fn)(void* user, size_t nbytes);

int moss_abi_version(void);

/* Text of the last error on the calling thread ("" if none). */
const char* moss_last_error(void);

/*
 * Replaces CudaRasterizer::Rasterizer::forward (DGR/cuda_rasterizer/rasterizer.h:31-55,
 * DGR/cuda_rasterizer/rasterizer_impl.cu:198-341).
 *   P  number of Gaussians, D active SH degree (0..3), M stored SH coefficients per Gaussian (0 if shs==NULL).
 *   background (3), means3D (P,3), shs (P,M,3) | colors_precomp (P,3), opacities (P),
 *   scales (P,3) + rotations (P,4) | cov3D_precomp (P,6), viewmatrix/projmatrix (16, transposed = column-major),
 *   cam_pos (3).   Outputs: out_color (3,H,W), out_depth (H,W), out_alpha (H,W), radii (P) int32 (may be NULL).
 *   Outputs need NOT be pre-zeroed (the reference requires zero-filled tensors; every element is written here).
 * Returns num_rendered >= 0 (the number of (Gaussian, tile) instances), or a negative error code.
 * Performs ONE stream synchronisation (to size the binning buffer), like the reference's blocking read
 * at rasterizer_impl.cu:283.
 * `debug` is a bit set.  MOSS_DEBUG_SYNC (1, the reference's `debug = true`): the stream is synchronised and checked after every
 * launch (CHECK_CUDA, auxiliary.h:166-173).  MOSS_DEBUG_NO_BLOCK_CULL (2; forward AND the matching backward call): the blend kernels
 * ignore the per-instance 4x4-block masks and test every list entry against every block.  The masks only SKIP (entry, block)
 * pairs that cannot reach alpha >= 1/255: final_T and n_contrib are bit-identical either way, images and gradients equal up to
 * float32 summation order (tests/test_gpu_ops.py::test_block_mask_culling_never_changes_a_result).  Per call, no global state.
 * In the BACKWARD the masks' box is also an addressing contract (a pair's gradient record has a cell only inside the box): a pair
 * outside it leaves no record in this mode either (light tiles: visited, record dropped; heavy tiles: the masks are followed) --
 * whether such a pair could have reached 1/255 is what the no-cull FORWARD image shows.
 * MOSS_DEBUG_EXACT_MATH (4; ABI 5; forward AND the matching backward call): the blend kernels evaluate what decides a pixel's list
 * -- the exponent, exp(), alpha, the transmittance chain -- exactly as the reference's SOURCE reads (forward.cu:336-356,
 * backward.cu:504-516): `power = -0.5f * (A dx dx + C dy dy) - B dx dy` with one rounding per operation (the fast path spells two
 * of them as FMAs), exp() as a correctly defined function (the restatement of glibc's expf that oracle/moss_oracle.c carries as
 * moss_expf_det: the same bits on CPU and GPU; the fast path uses v_exp_f32, ~1 ulp), and T = T / (1 - alpha) as a chain of IEEE
 * divisions (the fast path: v_rcp_f32 and a prefix product).  Under it n_contrib and final_T equal the CPU oracle's (with the same
 * exp) BIT FOR BIT on every pixel -- which turns "n_contrib may differ on <= 1e-4 of the pixels" of the fast path into a checked
 * statement: fast and exact differ only where a decision sits within rounding of its threshold.  2-3x slower blend kernels; a
 * checking mode, not a product path.
 * MOSS_DEBUG_TRACE (8; ABI 5): every stage launcher is wrapped in a roctx range ("moss:preprocess_fwd", "moss:scatter", ...), so
 * that a `rocprofv3 --kernel-trace --marker-trace` timeline of the CALLER's program shows the op's stages.  The
 * roctx library (librocprofiler-sdk-roctx.so) is resolved with dlopen at the first traced call: no link-time dependency, nothing
 * happens without the bit.  Ranges bracket the LAUNCH calls on the host (inside a captured hipGraph they are recorded once, at capture).
 */
#define MOSS_DEBUG_SYNC          1
#define MOSS_DEBUG_NO_BLOCK_CULL 2
#define MOSS_DEBUG_EXACT_MATH    4
#define MOSS_DEBUG_TRACE         8
/* MOSS_FORWARD_ONLY (16; ABI 6; a bit of the same argument of every FORWARD entry point -- not a diagnostic: the one call option the
 * reference's signature has no room for): the caller promises that NO backward call follows this forward -- an evaluation render
 * (render_ZJU.py:56-72: `render(view, gaussians, pipeline, background)` under torch.no_grad()).  The outputs are the
 * training forward's BIT FOR BIT (the blend folds its sums at the same list positions); what is not produced is the state only the
 * backward reads: depth-segment cuts, per-block tails, gradient-record cells and their validity bits.  The binning buffer then holds
 * ids, block masks, the 48-byte records and the 8-byte sort keys only: moss_raster_binning_bytes_forward_only(R), 62 B per instance
 * (training: ~370 B).  With a capacity (asynchronous forward) the keys go through the scan -> scatter chain into exact ranges -- six
 * launches -- because the per-tile key buckets of the four-launch training forward live in the record pool's address space.
 * A backward call over such buffers is a no-op that returns ZERO gradients and takes no optimizer step (status flag
 * MOSS_STATUS_FORWARD_ONLY; the kernels check it on the device, like a capacity overflow): never out-of-bounds. */
#define MOSS_FORWARD_ONLY        16
int moss_raster_forward(
    moss_alloc_fn geometry_alloc, void* geometry_user,
    moss_alloc_fn binning_alloc, void* binning_user,
    moss_alloc_fn image_alloc, void* image_user,
    int P, int D, int M,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* opacities,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    float tan_fovx, float tan_fovy,
    int prefiltered,
    float* out_color,
    float* out_depth,
    float* out_alpha,
    int* radii,
    int debug,
    void* stream);

/*
 * The asynchronous forward (moss_raster_forward_ex with capacity > 0, below) for launch-bound training loops and hipGraph capture: NO
 * host read-back.  The caller states an upper bound `capacity` on the number of (Gaussian, tile) instances (e.g. 2x the value a previous,
 * synchronous call returned); scratch buffers and launch grids are sized for it and every kernel bounds itself with the device-side
 * count.  Returns `capacity` -- pass that as R to the backward -- or a negative error code.
 * If a frame needs more instances than `capacity`, nothing is rendered (outputs = background, gradients = 0) and the
 * overflow bit is set in the status words; poll them with moss_raster_read_status once the stream has advanced.
 * `debug`: MOSS_DEBUG_NO_BLOCK_CULL is honoured; MOSS_DEBUG_SYNC is refused (MOSS_ERR_INVALID_ARG: it synchronises by definition).
 *
 * `frame_state` (optional, may be NULL; no counterpart in the reference, which memsets its buffers in every forward): a caller-owned
 * device block of moss_raster_frame_state_bytes(width, height) bytes, zero-initialised ONCE.  With it the call keeps the per-frame
 * counters its kernels add to (tile histogram, tile cursors, error flags) in that block instead of in the image buffer and returns
 * the block all-zero again (its sort kernel re-zeroes it; error paths clean it too), so no clear kernel runs in front of the
 * preprocess kernel -- one launch less per frame (4 us inside a captured graph).  One block per concurrent user (stream); the same
 * block serves every call of that user, also across image sizes up to the one it was sized for.  The library keeps NO state between
 * calls: the block is an argument (ABI version 1 armed it per host thread).  Its address is a kernel argument, so a block handed
 * to a call that was captured into a hipGraph must stay alive for as long as that graph is replayed.
 * The 32-bit word MOSS_FRAME_STATE_DROPPED_WORD of the block is a STICKY counter: the library adds 1 for every frame that
 * overflowed its capacity (and therefore rendered nothing) and never clears it; the caller reads it whenever it likes (e.g. once per
 * few hundred replays of a captured step -- the status words only describe the LAST frame) and writes 0 back.
 */
#define MOSS_FRAME_STATE_DROPPED_WORD 4
size_t moss_raster_frame_state_bytes(int width, int height);

/* Enqueue (on `stream`) a copy of the forward's 8 status words from the image buffer to pinned host memory:
 * [0] instances rendered  [1] longest tile list  [2] flags: bit0 prefiltered-point culled, bit1 capacity overflow
 * [3] the capacity that holds this frame: >= [6] -- the buffer's gradient-record pool (6 cells of 48 B per instance of capacity; a
 *     frame of wide Gaussians uses up to 16 per instance) and the per-tile key buckets are sized from the capacity too; a caller's
 *     policy grows the capacity from THIS word (moss_amd/diff_gaussian_rasterization/_C.py: margin x [3])
 * [4] sort chunks  [5] non-empty tiles  [6] instances the frame needed. */
#define MOSS_STATUS_PREFILTERED 1u
#define MOSS_STATUS_OVERFLOW    2u
#define MOSS_STATUS_FORWARD_ONLY 4u  /* the forward ran with MOSS_FORWARD_ONLY: its buffers carry no backward state */
int moss_raster_read_status(const char* image_buffer, uint32_t* host_pinned_out, void* stream);

/*
 * Replaces CudaRasterizer::Rasterizer::backward (DGR/cuda_rasterizer/rasterizer.h:57-89,
 * DGR/cuda_rasterizer/rasterizer_impl.cu:345-447).  R is the value forward returned.
 *   dL_dpix (3,H,W), dL_ddepths (H,W), dL_dalphas (H,W): incoming gradients; any (not all) of them may be NULL, meaning
 *   zeros (an output that did not take part in the loss), which saves the caller a zero-filled image.
 *   Gradient outputs: dL_dmean2D (P,3), dL_dconic (P,4 = 2x2), dL_dopacity (P), dL_dcolor (P,3),
 *   dL_dmean3D (P,3), dL_dcov3D (P,6), dL_dsh (P,M,3) (may be NULL if M==0), dL_dscale (P,3), dL_drot (P,4).
 *   Every element of every output is written (zeros for culled Gaussians, for dL_dscale/dL_drot when
 *   scales==NULL and for SH coefficients above the active degree), so outputs need NOT be pre-zeroed.
 *   dL_dconic (an intermediate), dL_dcolor and dL_dcov3D (gradients of the optional inputs colors_precomp / cov3D_precomp) may be
 *   NULL = not wanted (ABI 4): 52 bytes per Gaussian a caller working from SH and scales / rotations never reads.
 *   `alphas` and `radii` are accepted for signature parity and ignored (the reference ignores alphas too,
 *   DGR/cuda_rasterizer/backward.cu:410).
 * Gradients are bitwise reproducible run to run (no float atomics), unlike the reference.
 * Returns 0 or a negative error code.
 */
int moss_raster_backward(
    int P, int D, int M, int R,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* alphas,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* campos,
    float tan_fovx, float tan_fovy,
    const int* radii,
    char* geom_buffer,
    char* binning_buffer,
    char* image_buffer,
    const float* dL_dpix,
    const float* dL_ddepths,
    const float* dL_dalphas,
    float* dL_dmean2D,
    float* dL_dconic,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_dmean3D,
    float* dL_dcov3D,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    int debug,
    void* stream);

/* Replaces CudaRasterizer::Rasterizer::markVisible (DGR/cuda_rasterizer/rasterizer.h:24-29,
 * rasterizer_impl.cu:141-153).  present: (P) bytes, 1 if z_view > 0.2. */
int moss_raster_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                             uint8_t* present, void* stream);

/*
 * Replaces SimpleKNN::knn (SKNN/simple_knn.h:16-19, SKNN/simple_knn.cu:185-221) behind distCUDA2
 * (SKNN/spatial.cu:16-25): mean_dists[i] = mean of the squared distances from point i to its 3 nearest
 * other points.  points (P,3), mean_dists (P).  workspace: device scratch of moss_knn_workspace_bytes(P).
 * Fully asynchronous on `stream` (the reference blocks twice to fetch the scene bounding box, simple_knn.cu:197,200;
 * here the box is reduced and consumed on the device).
 */
size_t moss_knn_workspace_bytes(int P);
int moss_knn_dist2(int P, const float* points, float* mean_dists, char* workspace, size_t workspace_bytes, void* stream);

/*
 * Fused photometric loss of the training step and its gradient (the consumer side of the rasterizer's outputs):
 *   loss = mean|image - gt| + lambda_mask * mean((alpha - mask)^2) + lambda_dssim * (1 - mean SSIM(image, gt))
 * Replaces the torch graph built from l1_loss / l2_loss / ssim (utils/loss_utils.py:41-87) as combined in
 * train_ZJU.py:111-112,119,131 (lambda_dssim 0.2, lambda_mask 0.5) and its autograd backward.
 *   image, gt (C,H,W); alpha, mask (H,W) or both NULL; loss_out: 4 device floats {total, l1, ssim, mask_l2};
 *   dL_dimage (C,H,W), dL_dalpha (H,W; NULL iff alpha NULL): gradients of `total`, every element written.
 *   workspace: device scratch of moss_loss_workspace_bytes(C,H,W).  Asynchronous on `stream`, deterministic.
 */
size_t moss_loss_workspace_bytes(int C, int H, int W);
int moss_photometric_loss(int C, int H, int W, const float* image, const float* gt, const float* alpha, const float* mask,
                          float lambda_dssim, float lambda_mask, float* loss_out, float* dL_dimage, float* dL_dalpha,
                          char* workspace, size_t workspace_bytes, void* stream);
/* The same with a weight on the L1 term too (ABI 4): total = lambda_l1 L1 + lambda_mask maskL2 + lambda_dssim (1 - SSIM); lambda_l1 = 1
 * gives moss_photometric_loss bit for bit.  With lambda_l1 = 0, lambda_dssim = 1 and no alpha, loss_out[2] is the reference's
 * ssim(img1, img2) (utils/loss_utils.py:47-87: 11x11 window, zero padding, mean over all elements) and -dL_dimage its gradient:
 * a drop-in for MOSS's own ssim() call (train_ZJU.py:119) without changing its loss expression. */
int moss_photometric_loss_weighted(int C, int H, int W, const float* image, const float* gt, const float* alpha, const float* mask,
                                   float lambda_l1, float lambda_dssim, float lambda_mask, float* loss_out, float* dL_dimage,
                                   float* dL_dalpha, char* workspace, size_t workspace_bytes, void* stream);
/* MOSS's OWN loss expression for these three terms (ABI 6; train_ZJU.py:108-119,131): the L1 and the mask term are means over the
 * pixels of the view's `bound_mask` -- Ll1 = l1_loss(image[bound], gt[bound]) (:111), mask_loss = l2_loss(alpha[bound], mask[bound])
 * (:112) -- and SSIM is taken on the crop x, y, w, h = cv2.boundingRect(bound_mask) of both images (:115-119: zero padding at the
 * CROP's edges, mean over C*w*h).  total = lambda_l1 Ll1 + lambda_mask mask_loss + lambda_dssim (1 - ssim).
 *   bound: (H,W) bytes, non-zero = counted; NULL = every pixel of the rectangle.
 *   rect:  FIVE int32 in DEVICE memory: x, y, w, h, and the number of non-zero bytes of `bound` (ignored when bound is NULL).  Device
 *          memory so that a step captured in a hipGraph changes view by rewriting them (and `bound`, `gt`, `mask`) in place.  The
 *          rectangle is clipped to the image.  Pixels of `bound` outside it count for nothing (MOSS's rectangle is the bounding box of
 *          the mask: there are none).  An empty mask gives NaN means, like torch's mean of an empty selection (MOSS's own expression
 *          raises there: its ssim() is handed a 0 x 0 crop).
 *   dL_dimage, dL_dalpha: written for the WHOLE image (zero off the crop / off the mask), so they are the gradients of `total`
 *          w.r.t. the full-size tensors the rasterizer produced.  Same workspace, same two launches, deterministic. */
int moss_photometric_loss_roi(int C, int H, int W, const float* image, const float* gt, const float* alpha, const float* mask,
                              const unsigned char* bound, const int* rect, float lambda_l1, float lambda_dssim, float lambda_mask,
                              float* loss_out, float* dL_dimage, float* dL_dalpha, char* workspace, size_t workspace_bytes, void* stream);

/*
 * Flat fused AdamW (torch.optim.AdamW semantics, amsgrad off) over contiguous fp32 parameters with their gradients and moments, every
 * form of the update behind one argument block (ABI 6; the positional forms of ABI 2-5 were removed in ABI 7).  Replaces the per-group
 * optimizer step of scene/gaussian_model.py:215-226 for the Gaussian parameters.
 *   params, grads, exp_avg, exp_avg_sq: the elements [first, first + count) (first a multiple of 4) of flat buffers that the segment
 *     table -- global indices -- describes.  Every array (grads_extra too) starts on 16 bytes: the update moves float4; a misaligned
 *     pointer is refused (MOSS_ERR_INVALID_ARG).  Any count: arrays of 4 GB and more take a form of the kernel that loads through
 *     64-bit pointers (and has no degree-aware shortcut: see segment_active).  first = 0, count = n: the whole buffer.  A SHARD is for N ranks that reduce-scatter the
 *     gradient bucket, update their 1/N of the parameters (moments memory and update time / N) and all-gather the result (SURVEY
 *     section 8e; moss_amd/dist.py ShardedStep).
 *   Up to 8 learning-rate segments: parameter i belongs to the first segment s with i < segment_end[s] (host arrays).
 *   Optional periodic pattern per segment (all three arrays NULL = none): where segment_period[s] > 0, element j of segment s uses
 *     segment_lr[s] if j % segment_period[s] < segment_split[s], else segment_lr2[s] -- e.g. the SH coefficients stored as ONE
 *     (P,16,3) tensor with the DC term's learning rate on the first 3 of every 48 floats and lr/20 on the rest (the reference's
 *     separate f_dc / f_rest groups, without the per-step torch.cat of get_features).
 *   step_state NULL: `step` counts from 1.  Else the step counter is kept on the device: `step_state` is moss_adamw_state_bytes()
 *     (= MOSS_ADAMW_STATE_BYTES of the header the library was built from; ask the library, a binding's copy of the constant can be
 *     stale) zero-initialised device bytes (32-bit words: [0] = int step, advanced by one per call by the update kernel itself;
 *     [8..11] = the bias corrections of the current / next step, double-buffered by step parity; [64] and [128 + 64 g], g < 32 = its
 *     two-level block-completion counters, each on a 256-byte line of its own), count must be > 0, and nothing in the call depends
 *     on a host-side counter, so a captured hipGraph of a training step replays correctly.
 *   LEARNING RATES ON THE DEVICE (ABI 4): when word MOSS_ADAMW_LR_VALID_WORD of the step-state block is non-zero, every kernel that is
 *     given the block (this update and the fused backward, moss_raster_backward_ex with `opt`) takes segment s's learning rate from
 *     float word MOSS_ADAMW_LR_WORD0 + s and its second rate (periodic pattern) from MOSS_ADAMW_LR2_WORD0 + s instead of from
 *     segment_lr / segment_lr2: a schedule -- MOSS decays the position rate every iteration, scene/gaussian_model.py:263-268 -- is
 *     then a 64-byte host-to-device copy between two replays of a captured step, not a re-capture.
 *   skip_word (needs step_state: a host-side count cannot know about the skipped step): a GUARD.  If (*skip_word & skip_mask) != 0
 *     when the kernel runs, the call is a no-op -- parameters, moments and the device-side step counter stay bit for bit what they
 *     were.  E.g. the frame's status word (image buffer, 32-bit word 2; skip_mask = 2: the capacity-overflow bit of the asynchronous
 *     forward) -- a frame that overflowed its capacity rendered nothing and left zero gradients, and inside a captured step nobody is
 *     there to skip the optimizer: without the guard such a frame is a weight-decay-only step that also decays the moments.  Or a
 *     float that is non-zero when ANY rank dropped its frame (the flag averaged with the gradient bucket, skip_mask = 0x7fffffff) so
 *     that replicas skip together.
 * Plus the DEGREE-AWARE update of an SH tensor: MOSS trains at SH degree 0 / 1 / 2 for iterations 1-2999 and at degree 3 for the last
 * one (train_ZJU.py:85-86, scene/gaussian_model.py:171-173); the coefficients above the highest degree that has ever been active have
 * received no gradient, so their moments are exactly zero and their AdamW step is the decoupled weight decay alone.
 *   segment_active (NULL = none; else one int per segment, meaningful where segment_period[s] > 0 and a multiple of 4): of every
 *     `period` elements of segment s only the first segment_active[s] are ACTIVE (0 = all).  Inactive elements: gradient and moments are
 *     neither read nor written; the parameter takes p <- p (1 - lr wd), which is bit for bit what the full update gives for g = m = v = 0.
 *     The float4 that holds a period's last active element is read whole: its inactive gradients must be zero (the backward writes
 *     them so).  Where the shortcut does not apply -- a segment that does not start on a multiple of 4, a period that is not a
 *     multiple of 4, eps = 0, arrays of 4 GB and more -- every element takes the full update: inactive gradients must then be zero.
 *   inactive_zero != 0: the caller also knows the inactive PARAMETERS to be exactly zero (MOSS initialises features_rest with zeros,
 *     scene/gaussian_model.py:179-181, and 0 x decay = 0): they are not read or written at all.
 */
#define MOSS_ADAMW_STATE_BYTES 9216
#define MOSS_ADAMW_LR_VALID_WORD 12
#define MOSS_ADAMW_LR_WORD0 16
#define MOSS_ADAMW_LR2_WORD0 24
size_t moss_adamw_state_bytes(void);
typedef struct moss_adamw_flat_args {
    long long first, count;
    float* params; const float* grads; float* exp_avg; float* exp_avg_sq;
    int num_segments; const long long* segment_end; const float* segment_lr;
    const int* segment_period; const int* segment_split; const float* segment_lr2;
    const int* segment_active; int inactive_zero;
    double beta1, beta2; float eps, weight_decay;
    int step; void* step_state; const uint32_t* skip_word; uint32_t skip_mask;
    /* B views rendered for ONE optimizer step on one device (moss_amd/multiview.py: the data-parallel step of SURVEY 8e with the "ranks"
     * on one GPU): up to three more gradient buffers of the same layout as `grads` (for a range: its elements [first, first + count)).
     * The step's gradient is ((grads + grads_extra[0]) + grads_extra[1] ...) x grad_scale, added in that order, one float32 rounding
     * per operation -- bit for bit what accumulating the views one after the other into one buffer and scaling it gives.
     * num_grads_extra = 0: `grads` as it is (grad_scale is then ignored). */
    int num_grads_extra; const float* grads_extra[3]; float grad_scale;
} moss_adamw_flat_args;
int moss_adamw_flat_ex(const moss_adamw_flat_args* args, void* stream);

/* Up to eight parameter tensors with buffers OF THEIR OWN in one launch (ABI 6): what a torch.optim-style optimizer holds -- MOSS's six
 * single-tensor Gaussian groups (scene/gaussian_model.py:215-226), each with its `exp_avg` / `exp_avg_sq` state tensors and its own
 * step count (densification surgery keeps them per tensor).  Per element the arithmetic of moss_adamw_flat_ex with one segment, a
 * host-side step and the tensor's `lr` and `step`: bit-identical to num_tensors calls of it.  Pointers 16-byte aligned; an entry with numel 0 is skipped.
 * moss_amd.optim.AdamW -- the drop-in for `torch.optim.AdamW` of patches/gaussian_model.diff -- steps its single-tensor groups with it. */
typedef struct moss_adamw_multi_args {
    int32_t num_tensors;                     /* 1..8 */
    long long numel[8];
    float* params[8]; const float* grads[8]; float* exp_avg[8]; float* exp_avg_sq[8];
    float lr[8]; int32_t step[8];            /* step counts from 1, like moss_adamw_flat_args.step */
    double beta1, beta2; float eps, weight_decay;
} moss_adamw_multi_args;
int moss_adamw_multi(const moss_adamw_multi_args* args, void* stream);

/*
 * Evaluation metrics of a split (additive in ABI 6; no existing entry point changes): the per-view lines of MOSS's training_report,
 * train_ZJU.py:244-253 --
 *     image = clamp(render, 0, 1); gt = clamp(gt, 0, 1); image.permute(1,2,0)[bound_mask[0]==0] = 0 if bg.sum() == 0 else 1
 *     l1_test += l1_loss(image, gt).mean().double()         (utils/loss_utils.py:41-42: mean over all C*H*W elements)
 *     psnr_test += psnr(image, gt).mean().double()          (utils/image_utils.py:19-21: the MEAN of the C per-channel PSNRs;
 *                                                            an exact match gives +inf)
 *     ssim_test += ssim(image, gt).mean().double()          (utils/loss_utils.py:47-87: 11x11 window, sigma 1.5, fp32-normalised,
 *                                                            C1 = 0.01^2, C2 = 0.03^2, zero padding at the FULL frame's edge)
 * -- and render_ZJU.py:73-94 (render_set: the same metrics without a mask).  Up to eight views of one size per call.
 *   image[v], gt[v]: (C,H,W) fp32 device arrays, C = 1..4; bound[v]: (H,W) bytes, 0 = fill the render there (the view's bound_mask
 *     selection, moss_amd.loss.ViewRegion.bound), or NULL = no fill; out_image[v]: (C,H,W) fp32 receiving the clamped and filled
 *     render (what the caller's LPIPS is given), or NULL.  fill: 0 or 1, decided ONCE by the caller from its background colour.
 *   state: MOSS_METRICS_STATE_BYTES zero-initialised device bytes, 8-byte aligned: double [0] sum of l1, [1] sum of psnr, [2] sum of
 *     ssim, int64 [3] the number of views added; doubles [4..7] are never touched (the caller's, e.g. an LPIPS sum).  The views'
 *     float32 values are added in view order, one float64 rounding each: the reference's accumulation bit for bit.  Zero it to reset.
 *   per_view (optional): (per_view_capacity, 3) float32 {l1, psnr, ssim}; the view added as the n-th since the reset is written to
 *     row n while n < per_view_capacity.
 *   workspace: moss_metrics_workspace_bytes(num_views, C, H, W) device bytes (host-side function).
 * Two launches on `stream`, no host synchronisation, no allocation, deterministic (no float atomics): capturable in a hipGraph. */
#define MOSS_METRICS_STATE_BYTES 64
typedef struct moss_eval_metrics_args {
    int32_t num_views;                       /* 1..8 */
    int32_t C, H, W;
    const float* image[8];
    const float* gt[8];
    const unsigned char* bound[8];
    float* out_image[8];
    float fill;
    void* state;
    float* per_view; int32_t per_view_capacity;
    char* workspace; size_t workspace_bytes;
} moss_eval_metrics_args;
size_t moss_metrics_workspace_bytes(int num_views, int C, int H, int W);
size_t moss_metrics_state_bytes(void);
int moss_eval_metrics(const moss_eval_metrics_args* args, void* stream);

/*
 * Float32 frames to 8-bit pixels (additive in ABI 7; no existing entry point changes): what render_ZJU.py:83-84 does through
 * torchvision.utils.save_image and train_ZJU.py:75 for the viewer.  Up to eight views of one size per call, planar float32 in,
 * interleaved bytes out.  Per element, in float32 with each operation rounded on its own:
 *     rounding 0 (nearest):   trunc(min(max(x * 255 + 0.5, 0), 255))      save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
 *     rounding 1 (truncate):  trunc(min(max(x, 0), 1) * 255)              (clamp(img, 0, 1) * 255).byte()
 * NaN gives 0 in both.
 *   image[v]: (3,H,W) fp32; alpha[v]: (H,W) fp32, required iff channels_out == 4 (the fourth byte of every pixel; quantised by the same
 *     rule, never filled); bound[v]: (H,W) bytes or NULL -- where != 1 the colour is `fill`, applied before the quantisation (the
 *     selection of moss_eval_metrics); out[v]: (H,W,channels_out) bytes at ANY byte address, every byte written and none beside them.
 *   image and alpha must be 4-byte aligned (float arrays); wide loads and packed stores are used per view where its pointers allow.
 * One launch on `stream`, no workspace, no host synchronisation: capturable in a hipGraph. */
typedef struct moss_frames_to_u8_args {
    int32_t num_views;                       /* 1..8 */
    int32_t H, W;
    int32_t channels_out;                    /* 3 = RGB, 4 = RGBA (alpha from alpha[b]) */
    int32_t rounding;                        /* 0 = nearest, 1 = truncate */
    const float* image[8];
    const float* alpha[8];
    const unsigned char* bound[8];
    float fill;
    unsigned char* out[8];
} moss_frames_to_u8_args;
int moss_frames_to_u8(const moss_frames_to_u8_args* args, void* stream);

/*
 * A view's ground truth from its raw image and mask (additive in ABI 7; no existing entry point changes): the image path of MOSS's
 * dataset readers -- scene/dataset_readers.py:613-654 (ZJU), :361-407 (MonoCap), :830-868 (DNA-Rendering) and, later,
 * PILtoTorch(...)/255 (utils/general_utils.py:22-28): imread/255, cv2.undistort of image and mask, image[msk == 0] = background,
 * cv2.resize by an integer factor (INTER_AREA; INTER_NEAREST for the mask), np.array(image*255.0, dtype=np.byte).  Up to eight views of
 * one size per call: raw bytes in, packed 8-bit ground truth out.  THE CONTRACT is the text below -- the maintainers' reading of
 * OpenCV 4 (undistort = initUndistortRectifyMap(R = I, newK = K) + remap(INTER_LINEAR, BORDER_CONSTANT 0), source coordinates
 * quantised to 1/32 pixel, INTER_AREA at an integer factor = a box mean) -- and not OpenCV: the agreement with cv2 is unmeasured
 * (DESIGN.md lists where the two may differ).  Every operation is rounded on its own (no FMA contraction).
 *   rgb[b] (H0,W0,3) bytes, interleaved; mask[b] (H0,W0) bytes; K[b] 9 doubles, row-major (K[b][1] must be 0, fx = K[b][0] and
 *   fy = K[b][4] positive; cx = K[b][2], cy = K[b][5]; row 2 is not read); D[b] = k1, k2, p1, p2, k3 (all zero: no distortion, sampled
 *   by the same code).  K and D are HOST values of the block.  scale = 1, 2 or 4 must divide H0 and W0: H = H0/scale, W = W0/scale.
 * Per full-resolution sample (u, v), u the column:
 *   1. the map, in float64, in this order:  x = (u - cx)/fx, y = (v - cy)/fy;  x2 = x*x, y2 = y*y, r2 = x2 + y2, xy2 = 2*x*y;
 *      kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2;  xd = x*kr + p1*xy2 + p2*(r2 + 2*x2),  yd = y*kr + p1*(r2 + 2*y2) + p2*xy2  (sums left to
 *      right);  su = fx*xd + cx, sv = fy*yd + cy;  iu = rint(su*32), iv = rint(sv*32), ties to even.  If either is not finite or has
 *      magnitude >= 2^30 every tap of the sample is outside; else ix = iu >> 5 (floor), ax = iu & 31, likewise iy, ay.
 *   2. taps (ix,iy), (ix+1,iy), (ix,iy+1), (ix+1,iy+1); a tap outside the image reads 0.
 *   3. colour, in float32: per channel p = byte/255.f, weights w00 = (1-ay/32.f)*(1-ax/32.f), w01 = (1-ay/32.f)*(ax/32.f),
 *      w10 = (ay/32.f)*(1-ax/32.f), w11 = (ay/32.f)*(ax/32.f);  c = ((p00*w00 + p01*w01) + p10*w10) + p11*w11.
 *   4. mask_mode 0 ("round": ZJU's uint8 msk != 0, whose byte remap rounds), in integers: weights in 1/1024 (32-ax)(32-ay),
 *      ax(32-ay), (32-ax)ay, ax*ay; a tap is foreground iff its byte != 0; the sample is foreground iff the foreground weights sum to
 *      >= 512 (half rounds up); m = 0 or 1.
 *   5. mask_mode 1 ("any": MonoCap / DNA-Rendering's float mask/255), in float32: m = the bilinear value of byte/255.f with the
 *      weights and the order of 3; foreground iff m != 0.
 *   6. a background sample's colour is `background` (float32 0 or 1).
 * Output pixel (i, j) takes the samples (scale*j + dx, scale*i + dy):
 *   colour: scale 1 the sample; scale 2 ((c00 + c01) + (c10 + c11)) * 0.25f; scale 4 the balanced pairwise tree over the 16 samples in
 *     row-major order -- neighbours, then pairs (a row's four), then rows 0+1 and 2+3, then the two halves -- times 0.0625f;
 *   gt_u8[b] planar (3,H,W): trunc(colour * 255.f), in [0, 255];  bkgd_u8[b] (H,W): trunc(m * 255.f) of the sample dx = dy = 0
 *     (INTER_NEAREST at an integer factor): 0 or 255 in mode 0.
 * Every output byte is written and none beside them, at any address; wide loads and packed stores are used per view where its
 * pointers allow.  H0 * W0 * 3 must be < 2^31.  One launch on `stream`, no workspace, no host synchronisation: capturable.
 */
typedef struct moss_view_images_prepare_args {
    int32_t num_views;                       /* 1..8 */
    int32_t H0, W0;                          /* the raw size; every view of a call has it */
    int32_t scale;                           /* 1, 2 or 4; divides H0 and W0 */
    int32_t background;                      /* 0 or 1 */
    int32_t mask_mode;                       /* 0 = round, 1 = any */
    const unsigned char* rgb[8];
    const unsigned char* mask[8];
    double K[8][9];
    double D[8][5];
    unsigned char* gt_u8[8];                 /* (3,H,W) */
    unsigned char* bkgd_u8[8];               /* (H,W) */
} moss_view_images_prepare_args;
int moss_view_images_prepare(const moss_view_images_prepare_args* args, void* stream);

/*
 * One view's packed ground truth to the float32 static inputs of a step (additive in ABI 7): what PILtoTorch(...)/255
 * (utils/general_utils.py:22-28) makes of the reader's bytes.  gt_image (3,H,W) = gt_u8/255.f and bkgd_mask (1,H,W) = bkgd_u8/255.f,
 * a correctly rounded float32 division (not a multiplication by a reciprocal): bit for bit torch.from_numpy(u8)/255.0.  The float
 * outputs must be 4-byte aligned; the bytes may start anywhere.  One launch on `stream`, no host read: capturable -- what a caller's
 * load_frame calls per frame change.
 */
typedef struct moss_view_images_load_args {
    int32_t H, W;
    const unsigned char* gt_u8;              /* (3,H,W) */
    const unsigned char* bkgd_u8;            /* (H,W) */
    float* gt_image;                         /* (3,H,W) */
    float* bkgd_mask;                        /* (1,H,W) */
} moss_view_images_load_args;
int moss_view_images_load(const moss_view_images_load_args* args, void* stream);

/*
 * Per-Gaussian linear blend skinning of MOSS's coarse_deform_c2source (scene/gaussian_model.py:820-923, called from
 * gaussian_renderer/__init__.py:60,72), from the blend weights to the world-space transform, fused into one launch each way.
 * Per Gaussian i with v = vert_ids[i] (its nearest big-pose SMPL vertex):
 *     w = softmax(log(W[v] + 1e-9) + L[i])             (w = W[v] without L: :828-834)
 *     [B3 | b] = sum_j w_j A_big[j][:3,:]               (:837-839)       [O3 | o] = sum_j w_j A_obs[j][:3,:]   (:904-907)
 *     Q = B3^-1 (adjugate / determinant; torch.inverse at :841), M = R O3
 *     T = M Q                                           (`transforms`, :844,913,917)
 *     t = M (d[i] - Q b) + R o + Th                     (`translation`, :848-850,871,879,898,916,921)
 *     p = T x[i] + t                                    (`world_src_pts`, :839-842,869,877,896,908-914)
 * d[i] = (shape_off - pose_off_big + pose_off_obs)[v] is gathered by the caller (:855-898).  Shapes (fp32, contiguous): vert_ids
 * (P) int64; W (V,J); L (P,J) or NULL; A_big, A_obs (J,4,4) (row 3 is not read); d, x (P,3); R (3,3); Th (3) -- R and Th are DEVICE
 * pointers, so that a captured graph reads the frame's values at replay.  Outputs: T (P,3,3), t (P,3), p (P,3) (needs x) and w (P,J)
 * (MOSS's `bweights`), each optional but T and t.  An id outside [0, V) is never dereferenced: that Gaussian's output rows are NaN.
 * J = 1..64 (SMPL: 24), P >= 0 (0 launches nothing), V >= 1.  A singular B3 gives inf / NaN (the reference raises).
 */
typedef struct moss_lbs_forward_args {
    int32_t P, J, V;
    const int64_t* vert_ids;
    const float* weights;                    /* W (V,J) */
    const float* lbs_offsets;                /* L (P,J) or NULL */
    const float* A_big;                      /* (J,4,4) */
    const float* A_obs;                      /* (J,4,4) */
    const float* d;                          /* (P,3) */
    const float* R;                          /* (3,3) */
    const float* Th;                         /* (3) */
    const float* x;                          /* (P,3) or NULL */
    float* T;                                /* (P,3,3) */
    float* t;                                /* (P,3) */
    float* p;                                /* (P,3) or NULL; needs x */
    float* w;                                /* (P,J) or NULL */
} moss_lbs_forward_args;
/* One launch on `stream`; no host synchronisation, no allocation: capturable.  Returns 0 or a negative error code. */
int moss_lbs_deform_forward(const moss_lbs_forward_args* args, void* stream);

/*
 * Backward of moss_lbs_deform_forward (the autograd of the same reference lines), given the incoming gradients g_T (P,3,3), g_t (P,3)
 * and g_p (P,3; needs x), each NULL when zero.  The forward is recomputed per Gaussian.  Outputs, each optional:
 *   g_L (P,J; needs L): the gradient of the LBS offsets (the softmax's backward); g_d (P,3); g_x (P,3; needs x);
 *   g_A_obs (J,4,4): sum over the Gaussians of w_ij [gO3 | go] (row 3 written as zero) -- a two-level reduction in a fixed order
 *     (per-workgroup sums in `workspace`, then one fold launch in workgroup order, in float64): no float atomics, bitwise reproducible.
 *   workspace: moss_lbs_workspace_bytes(P, J) device bytes (needed with g_A_obs).
 * A_big, R, Th and W get no gradient (constants in MOSS).  Rows of Gaussians with an out-of-range id are NaN in g_L / g_d / g_x and
 * add nothing to g_A_obs.  Two launches on `stream` (one without g_A_obs); no host synchronisation, no allocation, no memset:
 * capturable.  P = 0 launches nothing (g_A_obs is then not written).
 */
typedef struct moss_lbs_backward_args {
    int32_t P, J, V;
    const int64_t* vert_ids;
    const float* weights;
    const float* lbs_offsets;
    const float* A_big;
    const float* A_obs;
    const float* d;
    const float* R;
    const float* Th;
    const float* x;
    const float* g_T;                        /* (P,3,3) or NULL */
    const float* g_t;                        /* (P,3) or NULL */
    const float* g_p;                        /* (P,3) or NULL; needs x */
    float* g_L;                              /* (P,J) or NULL; needs lbs_offsets */
    float* g_A_obs;                          /* (J,4,4) or NULL */
    float* g_d;                              /* (P,3) or NULL */
    float* g_x;                              /* (P,3) or NULL; needs x */
    char* workspace; size_t workspace_bytes;
} moss_lbs_backward_args;
int moss_lbs_deform_backward(const moss_lbs_backward_args* args, void* stream);
/* device bytes of the backward's workspace (host-side arithmetic); 0 for P <= 0 or J outside 1..64 */
size_t moss_lbs_workspace_bytes(int P, int J);

/*
 * moss_lbs_deform_backward with the frame's R and Th as variables too (additive in ABI 7): what fitting a frame's SMPL parameters to
 * images needs.  Every field of moss_lbs_backward_args with its meaning there, plus g_R (3,3) and g_Th (3), each optional.  With
 *     gT'_i = g_T_i + g_p_i x_i^T,   gt'_i = g_t_i + g_p_i,   N_i = O3 Q,   n_i = O3 (d_i - Q b) + o      (T = R N, t = R n + Th)
 *     g_Th = sum_i gt'_i,            g_R = sum_i (gT'_i N_i^T + gt'_i n_i^T)
 * -- the gradient of the op as defined above (M = R O3), not of the reference's torch.inverse(R) expression (scene/gaussian_model.py:
 * 915-918); the two agree where R is a rotation.  The twelve values ride the reduction of g_A_obs: per-workgroup sums (float64, in lane
 * order) in `workspace`, folded in workgroup order in float64 by the same fold launch; no float atomics: bitwise reproducible.  A
 * Gaussian with an id outside [0, V) adds nothing.  g_L, g_A_obs, g_d and g_x equal moss_lbs_deform_backward's bit for bit.
 *   workspace: moss_lbs_frame_workspace_bytes(P, J) device bytes (needed with g_A_obs, g_R or g_Th; >= moss_lbs_workspace_bytes).
 * Three launches on `stream` (moss_lbs_deform_backward's kernel as it is, a kernel of the same shape for the twelve values, the fold);
 * no host synchronisation, no allocation, no memset: capturable.  Every device loop has a trip count fixed by the arguments.  P = 0
 * launches nothing that reads a Gaussian: g_R and g_Th are written as zero (g_A_obs is not written).  Bad
 * arguments return MOSS_ERR_INVALID_ARG with "moss_lbs_deform_backward_frame" in moss_last_error().
 */
typedef struct moss_lbs_backward_frame_args {
    int32_t P, J, V;
    const int64_t* vert_ids;
    const float* weights;
    const float* lbs_offsets;
    const float* A_big;
    const float* A_obs;
    const float* d;
    const float* R;
    const float* Th;
    const float* x;
    const float* g_T;                        /* (P,3,3) or NULL */
    const float* g_t;                        /* (P,3) or NULL */
    const float* g_p;                        /* (P,3) or NULL; needs x */
    float* g_L;                              /* (P,J) or NULL; needs lbs_offsets */
    float* g_A_obs;                          /* (J,4,4) or NULL */
    float* g_d;                              /* (P,3) or NULL */
    float* g_x;                              /* (P,3) or NULL; needs x */
    char* workspace; size_t workspace_bytes;
    float* g_R;                              /* (3,3) or NULL */
    float* g_Th;                             /* (3) or NULL */
} moss_lbs_backward_frame_args;
int moss_lbs_deform_backward_frame(const moss_lbs_backward_frame_args* args, void* stream);
/* device bytes of moss_lbs_deform_backward_frame's workspace (host-side arithmetic, monotonic); 0 for P <= 0 or J outside 1..64 */
size_t moss_lbs_frame_workspace_bytes(int P, int J);

/*
 * The per-frame, per-subject part of MOSS's coarse_deform_c2source (additive in ABI 7): what scene/gaussian_model.py:835-901 computes
 * before and between the per-Gaussian steps, with get_transform_params_torch / get_rigid_transformation_torch (:965-1031) and
 * batch_rodrigues_torch (:945-963).  It feeds moss_lbs_deform_forward (A_big, A_obs, d) and takes its gradients back.
 *     rot_big = Rodrigues(poses_big), rot = Rodrigues(poses)      angle = |r + 1e-8|, R = I + sin K + (1 - cos) K K    (:859,883,945-963)
 *     rot[1:] = rot[1:] correct_Rs                                 with correct_Rs                                       (:885-888)
 *     joints_s = J_regressor (v_template + shapedirs[..., :nb_s] beta_s)   for s = big (shapes_big), obs (shapes)         (:1004-1007,1021)
 *     G_0 = [rot_0 | joints_0], G_j = G_parent[j] [rot_j | joints_j - joints_parent[j]], A_j = [G_j.R | G_j.t - G_j.R joints_j]   (:965-995)
 *     D = shapedirs[..., :nb] beta_obs + posedirs ((rot[1:] - I) - (rot_big[1:] - I))   (V,3): ONE pass over posedirs       (:855-899)
 *     d = D[vert_ids]                                               (P,3)                                                  (:863,872,894)
 * Shapes (fp32, contiguous): v_template (V,3); shapedirs (V,3,shapedirs_stride), of which the first num_betas_big / num_betas enter;
 * posedirs (V,3,9(J-1)); J_regressor (J,V); poses_big, poses (3J); shapes_big (num_betas_big), shapes (num_betas); correct_Rs
 * (J-1,3,3) or NULL; vert_ids (P) int64 -- all DEVICE pointers, so that a captured graph reads the frame's values at replay.
 * parents: by value, parents[j] in [0, j) for j >= 1 (parents[0] is not read); J = 1..MOSS_SMPL_FRAME_MAX_JOINTS.
 * Outputs: A_big, A_obs (J,4,4) (row 3 = 0 0 0 1); d (P,3), a NaN row for an id outside [0, V) (never dereferenced); rot_mats (J,3,3),
 * the frame's rotations after correct_Rs; saved: MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT * J floats for the backward, or NULL.
 * workspace: moss_smpl_frame_workspace_bytes(max(P, 1), V, J) device bytes (D and the regressor shares; garbage afterwards).
 * Two launches on `stream`.  Every sum is formed in float64 in a fixed order, no atomics: bitwise reproducible.  No host
 * synchronisation, no allocation, no memset: capturable.  Bad arguments return MOSS_ERR_INVALID_ARG with moss_last_error() set.
 */
#define MOSS_SMPL_FRAME_MAX_JOINTS 64
#define MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT 33
typedef struct moss_smpl_frame_args {
    int32_t P, V, J;
    int32_t num_betas_big, num_betas, shapedirs_stride;
    int32_t parents[MOSS_SMPL_FRAME_MAX_JOINTS];
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;                   /* may be NULL for J = 1 */
    const float* J_regressor;
    const float* poses_big;
    const float* shapes_big;
    const float* poses;
    const float* shapes;
    const float* correct_Rs;                 /* (J-1,3,3) or NULL */
    const int64_t* vert_ids;
    float* A_big;
    float* A_obs;
    float* d;
    float* rot_mats;
    float* saved;                            /* or NULL: no backward will follow */
    char* workspace; size_t workspace_bytes;
} moss_smpl_frame_args;
int moss_smpl_frame_forward(const moss_smpl_frame_args* args, void* stream);   /* scene/gaussian_model.py:835-901, :945-1031 */

/*
 * Backward of moss_smpl_frame_forward to correct_Rs (the autograd of scene/gaussian_model.py:885-901 and :965-995; poses, shapes, the
 * body model and the big pose are data in MOSS and get no gradient).  g_A_obs (J,4,4) and g_d (P,3) are what moss_lbs_deform_backward
 * hands back, each NULL when zero; g_correct_Rs (J-1,3,3) is written, never accumulated into.
 *     g_feat[k] = sum_i sum_c posedirs[vert_ids[i], c, k] g_d[i, c]: every workgroup owns a fixed run of Gaussians and walks it in index
 *       order, the workgroups' vectors are folded in workgroup order (g_D (V,3) is never formed; coinciding ids cost nothing extra;
 *       a Gaussian with an id outside [0, V) adds nothing);
 *     the chain's adjoint as a reverse walk of the tree: gGR_j = g_A_j[:3,:3] - g_A_j[:3,3] joints_j^T, gGt_j = g_A_j[:3,3];
 *       for j = J-1 .. 1, p = parents[j]: g_rot_j = G_p.R^T gGR_j, gGR_p += gGR_j rot_j^T + gGt_j rel_j^T, gGt_p += gGt_j;
 *     g_correct_Rs[q] = rot_raw[q+1]^T (g_rot[q+1] + g_feat[9q .. 9q+8]).
 * saved: as the forward wrote it.  workspace: moss_smpl_frame_workspace_bytes(P, V, J) device bytes (needed with g_d).  Three launches
 * on `stream` (one without g_d or with P = 0), float64 sums in a fixed order, no atomics: bitwise reproducible; capturable.
 */
typedef struct moss_smpl_frame_backward_args {
    int32_t P, V, J;
    int32_t parents[MOSS_SMPL_FRAME_MAX_JOINTS];
    const float* posedirs;
    const int64_t* vert_ids;
    const float* saved;
    const float* g_A_obs;                    /* (J,4,4) or NULL; row 3 is not read */
    const float* g_d;                        /* (P,3) or NULL */
    float* g_correct_Rs;                     /* (J-1,3,3) */
    char* workspace; size_t workspace_bytes;
} moss_smpl_frame_backward_args;
int moss_smpl_frame_backward(const moss_smpl_frame_backward_args* args, void* stream);   /* the adjoint of scene/gaussian_model.py:885-901, :965-995 */
/* device bytes of either call's workspace (host-side arithmetic, monotonic); 0 for a size <= 0 or J outside 1..64 (gaussian_model.py:835-901) */
size_t moss_smpl_frame_workspace_bytes(int P, int V, int J);

/*
 * Backward of moss_smpl_frame_forward to the frame's pose as well (additive in ABI 7): what fitting a frame's SMPL parameters to
 * images needs.  Every field of moss_smpl_frame_backward_args with its meaning there (g_correct_Rs becomes optional), plus poses (3J)
 * and correct_Rs ((J-1,3,3) or NULL: the identity) as the forward read them, and the output g_poses (3J), written, never accumulated
 * into.  g_feat and the reverse walk of the tree are moss_smpl_frame_backward's; then
 *     g_rot_0 = gGR_0 after the walk has accumulated into it (G_0.R = rot_0),    g_raw_0 = g_rot_0,
 *     g_raw_j = (g_rot_j + g_feat[9(j-1) .. 9(j-1)+8]) correct_Rs[j-1]^T         for j >= 1,
 *     and the adjoint of batch_rodrigues_torch as the reference writes it (scene/gaussian_model.py:945-963), one joint per thread:
 *     e = r + 1e-8, a = |e|, k = r / a (the shift is in the norm only), raw = I + sin a K + (1 - cos a) K K, G = g_raw_j:
 *       g_s = <G, K>,  g_c = <G, K K>,  gK = sin a G + (1 - cos a)(G K^T + K^T G),  g_k = (gK_21 - gK_12, gK_02 - gK_20, gK_10 - gK_01),
 *       g_a = g_s cos a + g_c sin a - <g_k, r> / a^2,   g_poses[3j .. 3j+2] = g_k / a + g_a e / a.
 * shapes, the body model and the big pose stay data.  saved: as the forward wrote it (MOSS_SMPL_FRAME_SAVED_FLOATS_PER_JOINT per joint).
 * workspace: moss_smpl_frame_workspace_bytes(P, V, J) device bytes (needed with g_d).  Three launches on `stream` (one without g_d or
 * with P = 0: g_poses then comes from g_A_obs alone), float64 sums in a fixed order, no atomics: bitwise reproducible.  No host
 * synchronisation, no allocation, no memset: capturable.  Every device loop has a trip count fixed by the arguments (J, a workgroup's
 * run of Gaussians, the number of workgroups).  Bad arguments return MOSS_ERR_INVALID_ARG with "moss_smpl_frame_backward_pose" in
 * moss_last_error().
 */
typedef struct moss_smpl_frame_backward_pose_args {
    int32_t P, V, J;
    int32_t parents[MOSS_SMPL_FRAME_MAX_JOINTS];
    const float* posedirs;
    const int64_t* vert_ids;
    const float* saved;
    const float* g_A_obs;                    /* (J,4,4) or NULL; row 3 is not read */
    const float* g_d;                        /* (P,3) or NULL */
    float* g_correct_Rs;                     /* (J-1,3,3) or NULL */
    char* workspace; size_t workspace_bytes;
    const float* poses;                      /* (3J) */
    const float* correct_Rs;                 /* (J-1,3,3) or NULL */
    float* g_poses;                          /* (3J) */
} moss_smpl_frame_backward_pose_args;
int moss_smpl_frame_backward_pose(const moss_smpl_frame_backward_pose_args* args, void* stream);   /* the adjoint of scene/gaussian_model.py:885-901, :945-995 */

/*
 * The posed SMPL vertices of a frame in the world and their padded box (additive in ABI 7): the reference's numpy SMPL.__call__
 * (smpl/smpl_numpy.py:46-98) followed by `xyz @ R^T + Th` and the min / max of scene/dataset_readers.py:428-436 (the frame, pad 0.1)
 * and :331-339 (the big pose, pad 0.05), on the device.
 *     v_shaped = v_template + shapedirs[..., :num_betas] beta                                                (smpl_numpy.py:52)
 *     joints   = J_regressor v_shaped                                                                        (:53)
 *     rot      = Rodrigues(poses)      the project's form: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K K (:61; gaussian_model.py:945-963)
 *     v_posed  = v_shaped + posedirs (rot[1:] - I)                        ONE pass over posedirs             (:68-71)
 *     G_0 = [rot_0 | joints_0], G_j = G_parent[j] [rot_j | joints_j - joints_parent[j]], A_j = [G_j.R | G_j.t - G_j.R joints_j]   (:73-92)
 *     T_v = sum_j weights[v, j] A_j,  world_v = R (T_v [v_posed, 1]) + Th                                    (:94-96; dataset_readers.py:429)
 *     world_bound = fl32(min_v world_v - fl32(pad)), fl32(max_v world_v + fl32(pad))     over the float32 world_v written (:432-436)
 *     joints_out[j] = G_j.t                  the posed joints SMPL.__call__ returns second (SMPL space: R and Th do not enter)   (:85)
 * Shapes (fp32, contiguous): the body-model arrays as moss_smpl_frame_args names them, plus weights (V,J); poses (3J), shapes
 * (num_betas <= shapedirs_stride), R (3,3), Th (3), pad (1) -- all DEVICE pointers, so that a captured graph serves a new pose after
 * five small copies.  parents: by value, parents[j] in [0, j) for j >= 1; J = 1..MOSS_SMPL_FRAME_MAX_JOINTS, V >= 1.
 * Outputs: world_vertex (V,3), world_bound (2,3), joints (J,3) or NULL.  workspace: moss_smpl_vertices_workspace_bytes(V, J) device
 * bytes (v_posed in float64, the regressor shares, one min / max record per workgroup; garbage afterwards).
 * Three launches on `stream`.  Every sum is formed in float64 in a fixed order and rounded to float32 once; the min / max are folded
 * from per-workgroup records in workgroup order; no atomics: bitwise reproducible.  No host synchronisation, no allocation, no memset,
 * every output element written: capturable.  Bad arguments return MOSS_ERR_INVALID_ARG with the field named in moss_last_error().
 */
typedef struct moss_smpl_vertices_args {
    int32_t V, J;
    int32_t num_betas, shapedirs_stride;
    int32_t parents[MOSS_SMPL_FRAME_MAX_JOINTS];
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;                   /* may be NULL for J = 1 */
    const float* J_regressor;
    const float* weights;
    const float* poses;
    const float* shapes;                     /* may be NULL for num_betas = 0 */
    const float* R;
    const float* Th;
    const float* pad;
    float* world_vertex;
    float* world_bound;
    float* joints;                           /* (J,3) or NULL */
    char* workspace; size_t workspace_bytes;
} moss_smpl_vertices_args;
int moss_smpl_vertices(const moss_smpl_vertices_args* args, void* stream);   /* smpl/smpl_numpy.py:46-98, scene/dataset_readers.py:331-339, :428-436 */
/* device bytes of the call's workspace (host-side arithmetic, monotonic); 0 for V <= 0 or J outside 1..64 */
size_t moss_smpl_vertices_workspace_bytes(int V, int J);

/*
 * The 2D bound masks of one world_bound seen by C >= 1 cameras, with their bounding rectangles (additive in ABI 7):
 * get_bound_2d_mask of scene/dataset_readers.py:1034-1045 with get_bound_corners (:1008-1021) and project (:1023-1032), and
 * cv2.boundingRect of the mask (train_ZJU.py:115), in one call for all cameras.
 *   Corners: the eight corners in get_bound_corners' order (corner i takes max x for i & 4, max y for i & 2, max z for i & 1);
 *     cam = c RT[:, :3]^T + RT[:, 3], uvw = K cam, xy = uvw[:2] / uvw[2], computed in FLOAT64 from the float32 inputs, every operation
 *     rounded on its own ((c0 RT[r][0] + c1 RT[r][1]) + c2 RT[r][2]) + RT[r][3]; (K[r][0] cam0 + K[r][1] cam1) + K[r][2] cam2), then
 *     rounded half-to-even as np.round does.
 *   Flag: flags[c] bit 0 is set when any corner has uvw[2] <= 0 or a rounded coordinate exceeds 2^20 in magnitude (a NaN counts): the
 *     reference divides through and fills garbage there.  For a flagged camera the mask is the WHOLE frame, rect = (0, 0, W, H, W H).
 *     corners holds what was computed, clamped to +-2^20 (a NaN: -2^20).
 *   Mask: pixel (x, y) is 1 when it belongs to at least one of the six faces [0,1,3,2], [4,5,7,6], [0,1,5,4], [2,3,7,6], [0,2,6,4],
 *     [1,3,7,5] (:1039-1044).  A face has integer vertices q0..q3 in that cyclic order; all arithmetic is int64.  A pixel p belongs to
 *     a face when
 *       (a) closed quad: p is inside the face's bounding box and the four cross products (q_{k+1} - q_k) x (p - q_k) are all >= 0 or
 *           all <= 0; or
 *       (b) drawn edge: for some k, with (dx, dy) = q_{k+1} - q_k and m = max(|dx|, |dy|), p is inside the edge's bounding box and
 *           |2 (dx (y - q_k.y) - dy (x - q_k.x))| <= m: the nearest pixel along the major axis, both at an exact tie (fillPoly draws
 *           every polygon edge as an 8-connected line beside filling the interior).
 *   Rect: (x, y, w, h) of the mask's non-zero pixels (moss_amd.loss.bounding_rect; 0 0 0 0 when empty) and the number of ones, laid
 *     out as ViewRegion.rect is.
 * Not verified against cv2.fillPoly: tie pixels of rule (b) and lines cv2 clips at the image border may differ
 * by single pixels on the outline.
 * Inputs (DEVICE pointers): world_bound (2,3), K (C,3,3), RT (C,3,4) float32.  Outputs: bound (C,H,W) uint8 of 0 / 1, rect (C,5) int32,
 * corners (C,8,2) int32 (x, y), flags (C) int32.  C = 1..65535, H, W >= 1 with H W < 2^31.  workspace:
 * moss_bound_mask_workspace_bytes(C, H, W) device bytes (one record per 64 x 8 pixel tile and camera; garbage afterwards).
 * Two launches on `stream` whatever C is.  Integer arithmetic, no atomics, every output element written, no clearing launch:
 * bitwise reproducible; capturable.  Bad arguments return MOSS_ERR_INVALID_ARG with the field named in moss_last_error().
 */
typedef struct moss_bound_mask_args {
    int32_t C, H, W;
    const float* world_bound;
    const float* K;
    const float* RT;
    uint8_t* bound;
    int32_t* rect;
    int32_t* corners;
    int32_t* flags;
    char* workspace; size_t workspace_bytes;
} moss_bound_mask_args;
int moss_bound_mask(const moss_bound_mask_args* args, void* stream);   /* scene/dataset_readers.py:1008-1045, train_ZJU.py:115 */
/* device bytes of the call's workspace (host-side arithmetic, monotonic); 0 for a size <= 0, C > 65535 or H W >= 2^31 */
size_t moss_bound_mask_workspace_bytes(int C, int H, int W);

/*
 * Backward of moss_smpl_vertices to the frame's poses, R and Th (additive in ABI 7): what fitting a frame's SMPL parameters to
 * keypoints needs.  The body arrays, parents, poses (3J), shapes, R, Th with their meaning in moss_smpl_vertices_args, plus
 * g_world_vertex (V,3).  Outputs, written and never accumulated into: g_poses (3J), g_R (3,3), g_Th (3).  shapes and the body model
 * are data.  Nothing is saved by the forward: v_posed, the joints, the chain and A_j are recomputed here from the inputs (the forward
 * entry keeps its outputs and its launches).  With the forward's names, g_v = g_world_vertex[v] and h_v = R^T g_v:
 *     g_Th = sum_v g_v                      g_R = sum_v g_v y_v^T                       y_v = T_v [v_posed_v, 1],  T_v = sum_j w[v,j] A_j
 *     g_A_j[:3,:3] = sum_v w[v,j] h_v v_posed_v^T          g_A_j[:3,3] = sum_v w[v,j] h_v
 *     g_vposed_v = T_v[:3,:3]^T h_v        g_feat[k] = sum_v sum_c posedirs[v,c,k] g_vposed[v,c]        ONE pass over posedirs
 * and from there the reverse walk of the tree and the adjoint of Rodrigues exactly as moss_smpl_frame_backward_pose states them, with
 * correct_Rs = the identity: g_raw_0 = g_rot_0, g_raw_j = g_rot_j + g_feat[9(j-1) .. 9(j-1)+8]; e = r + 1e-8, 1 - cos a = 2 sin^2(a/2).
 * Four launches on `stream`:
 *   posed     moss_smpl_vertices' first kernel as it is: v_posed (float64) and the regressor shares, into `workspace`;
 *   skin      a grid over ranges of 256 vertices: every workgroup folds the shares, walks the chain, then forms y_v, h_v and g_vposed_v of
 *             its vertices and, walking them in index order, its partial sums of g_Th, g_R and g_A (12 + 12 J values per workgroup);
 *   features  a grid over ranges of 32 vertices, threads over the 9 (J - 1) features: one partial vector per workgroup (not for J = 1);
 *   chain     one workgroup folds both sets of partials in a fixed order (the skin partials in workgroup order; the feature partials in
 *             1024 / (9 (J - 1)) runs of workgroups, each in order, then the runs in order), walks the tree in reverse, and one joint
 *             per thread forms g_poses.
 * Every sum is formed in float64 in a fixed order and rounded to float32 once; no atomics: bitwise reproducible.  Every device loop has
 * a trip count fixed by the arguments (V, J, a workgroup's run of vertices, the number of workgroups): no convergence loop, no
 * spin-wait, no hand-over between workgroups inside a launch.  No host synchronisation, no allocation, no memset, every output element
 * written: capturable.  J = 1 works without posedirs.  workspace: moss_smpl_vertices_backward_workspace_bytes(V, J) device bytes
 * (garbage afterwards).  Bad arguments return MOSS_ERR_INVALID_ARG with "moss_smpl_vertices_backward" and the field in moss_last_error().
 */
typedef struct moss_smpl_vertices_backward_args {
    int32_t V, J;
    int32_t num_betas, shapedirs_stride;
    int32_t parents[MOSS_SMPL_FRAME_MAX_JOINTS];
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;                   /* may be NULL for J = 1 */
    const float* J_regressor;
    const float* weights;
    const float* poses;
    const float* shapes;                     /* may be NULL for num_betas = 0 */
    const float* R;
    const float* Th;
    const float* g_world_vertex;             /* (V,3) */
    float* g_poses;                          /* (3J) */
    float* g_R;                              /* (3,3) */
    float* g_Th;                             /* (3) */
    char* workspace; size_t workspace_bytes;
} moss_smpl_vertices_backward_args;
int moss_smpl_vertices_backward(const moss_smpl_vertices_backward_args* args, void* stream);   /* the adjoint of smpl/smpl_numpy.py:46-98 and `xyz @ R^T + Th` */
/* device bytes of the call's workspace (host-side arithmetic, monotonic); 0 for V <= 0 or J outside 1..64 */
size_t moss_smpl_vertices_backward_workspace_bytes(int V, int J);

/*
 * A keypoint loss on posed vertices, value and vertex gradient in one call (additive in ABI 7).  Keypoints of any convention
 * (OpenPose, COCO, H36M, markers glued to vertices) are a dense linear regressor over the vertices; they are compared with 2D
 * detections in C cameras and / or with 3D points under a Geman-McClure robustifier:
 *     X_k = sum_v regressor[k,v] world_vertex[v]
 *     cam = RT_c [X_k, 1],  uvw = K_c cam,  u = (uvw_x / uvw_z, uvw_y / uvw_z),  r2 = |u - uv[c,k]|^2      (moss_bound_mask's cameras)
 *     rho_s(r2) = s^2 r2 / (s^2 + r2)        (r2 itself for s <= 0: no robustifier)
 *     loss = weight2d / (C Kp) sum_c sum_k conf[c,k] rho_sigma(r2)  +  weight3d / Kp sum_k conf3[k] rho_sigma3(|X_k - xyz_k|^2)
 * An entry with uvw_z <= 0 contributes nothing to the value or the gradient and sets flags[c] |= 1 (moss_bound_mask's rule and bit).
 * Inputs (DEVICE pointers, float32, contiguous): world_vertex (V,3); regressor (Kp,V); the 2D part, absent when C = 0: K (C,3,3),
 * RT (C,3,4), uv (C,Kp,2) in pixels, conf (C,Kp) >= 0; the 3D part, absent when xyz is NULL: xyz (Kp,3), conf3 (Kp).  At least one
 * part is present.  By value: sigma (pixels), sigma3 (metres), weight2d, weight3d; Kp = 1..MOSS_KEYPOINTS_MAX, V >= 1, C = 0..65535.
 * Outputs: loss (1); g_world_vertex (V,3) = regressor^T g_X for a unit upstream gradient; keypoints (Kp,3) = X, or NULL; flags (C)
 * int32, written whole (not read for C = 0).  The loss is a scalar: nothing is saved for a backward.
 * Three launches on `stream`:
 *   keypoints  one workgroup per keypoint sums its row of the regressor over the vertices (threads stride the vertices, then a fixed
 *              butterfly and the waves in order); X goes to `workspace` in float64;
 *   residuals  one workgroup per camera (one more for the 3D part), one thread per keypoint: the entry's value and its gradient to
 *              X_k go to `workspace`, the camera's values are summed in keypoint order, flags[c] is written;
 *   scatter    a grid over ranges of 256 vertices: every workgroup folds g_X over the cameras in camera order, workgroup 0 also the
 *              loss; then g_world_vertex[v] = sum_k regressor[k,v] g_X[k] in keypoint order.
 * Every sum is formed in float64 in a fixed order and rounded to float32 once; no atomics: bitwise reproducible.  Every device loop has
 * a trip count fixed by the arguments (V, Kp, C).  No host synchronisation, no allocation, no memset, every output element written:
 * capturable.  workspace: moss_keypoint_loss_workspace_bytes(C, Kp) device bytes (garbage afterwards).  Bad arguments return
 * MOSS_ERR_INVALID_ARG with "moss_keypoint_loss" and the field in moss_last_error().
 */
#define MOSS_KEYPOINTS_MAX 128
typedef struct moss_keypoint_loss_args {
    int32_t V, Kp, C;
    const float* world_vertex;
    const float* regressor;
    const float* K;                          /* (C,3,3); not read for C = 0 */
    const float* RT;                         /* (C,3,4) */
    const float* uv;                         /* (C,Kp,2) */
    const float* conf;                       /* (C,Kp) */
    const float* xyz;                        /* (Kp,3) or NULL: no 3D part */
    const float* conf3;                      /* (Kp); needed with xyz */
    float sigma, sigma3;
    float weight2d, weight3d;
    float* loss;
    float* g_world_vertex;
    float* keypoints;                        /* (Kp,3) or NULL */
    int32_t* flags;                          /* (C) */
    char* workspace; size_t workspace_bytes;
} moss_keypoint_loss_args;
int moss_keypoint_loss(const moss_keypoint_loss_args* args, void* stream);
/* device bytes of the call's workspace (host-side arithmetic, monotonic); 0 for C outside 0..65535 or Kp outside 1..MOSS_KEYPOINTS_MAX */
size_t moss_keypoint_loss_workspace_bytes(int C, int Kp);

/*
 * MOSS's S3IM term and its gradient (additive in ABI 7): s3im_loss = s3im_fun(img_pred, img_gt) (train_ZJU.py:123, weighted 0.3 at
 * :131; utils/loss_utils.py:17-38).  MOSS hands it two (1,C,h,w) crops, so every randperm(1) is [0] and the term is deterministic:
 *     s3im = 1 - ssim(x~, y~),   x~ = the crop with every pixel repeated `repeat` times along a row (width repeat * w)
 * with the reference's ssim (utils/loss_utils.py:57-87: 11x11 window, sigma 1.5, fp32-normalised, zero padding at the crop's edges,
 * per channel, C1 = 0.01^2, C2 = 0.03^2, mean over C * h * repeat * w).  The widened images are never formed: HBM traffic per source
 * pixel-channel does not depend on `repeat`.
 *   image, gt (C,H,W) fp32; rect: 5 DEVICE ints as moss_photometric_loss_roi's (x, y, w, h of the crop; the fifth is not read), clipped
 *     to the frame the same way, or NULL = the whole image; repeat: 1..16 (MOSS: 10);
 *   loss_out: 2 device floats {1 - ssim, ssim}; dL_dimage (C,H,W): d(1 - ssim)/d image, written everywhere, zero off the crop;
 *   workspace: moss_s3im_workspace_bytes(C, H, W) device bytes (any repeat).
 * An empty crop gives NaN values (0 / 0) and a zero gradient.  Two launches on `stream`, no host synchronisation, no allocation: a
 * captured step changes view by rewriting `rect`.  Sums in a fixed order, no atomics: bitwise reproducible.  Bad arguments (sizes
 * <= 0, repeat outside 1..16, a short workspace, a NULL output) return MOSS_ERR_INVALID_ARG with moss_last_error() set.
 */
size_t moss_s3im_workspace_bytes(int C, int H, int W);  /* 0 for a size <= 0 */
int moss_s3im_loss(int C, int H, int W, const float* image, const float* gt, const int* rect, int repeat, float* loss_out,
                   float* dL_dimage, char* workspace, size_t workspace_bytes, void* stream);

/*
 * MOSS's pose-refinement head and its matrix-Fisher loss term (additive in ABI 7), one launch each way:
 *   pc.auto_regression(smpl_param['poses'])   gaussian_renderer/__init__.py:66-71 -> nets/mlp_delta_body_pose.py:56-82 (Autoregression.forward)
 *   matrix_fisher_nll(F, U, S, V, target_R)   train_ZJU.py:125-129 -> utils/loss_utils.py:283-317, LogMFNormConstant :222-280
 * Forward, for the 23 non-root joints (joint j here is joint j + 1 of `parents`):
 *     h = W4 relu(W2 relu(W0 poses[3:72] + b0) + b2) + b4               the MLP 69 -> 128 -> 128 -> 69 (:57), h viewed as (23,3)
 *     r_j = fc_j [h_j, h_a1, h_a2, ...] + c_j                            a1, a2, ... the non-root ancestors of j, parent first (:62-71, :41-54)
 *     Rs_j = n n^T (1 - cos th) + cos th I + sin th [n]x,  th = sqrt(1e-5 + |r_j|^2), n = r_j / th     RodriguesModule (:258-284)
 *     Rs_j = U diag(s) V^T (one-sided Jacobi, s descending);  S_j = (s1, s2, s3 det(U V^T))            torch.svd (:75), loss_utils.py:310-313
 *     log c(S) = log(1/2 int_-1^1 I0~((S2 - S3)(1 - u)/2) I0~((S2 + S3)(1 + u)/2) exp((S3 + S1)(u - 1)) du) + S1 + S2 + S3
 *                512-point trapezoid, I0~(x) = exp(-|x|) I0(x) by two polynomials split at |x| <= 3.75 (:98-184, :245-258)
 *     nll_j = -<Rs_j, target_R_j> + overreg log c(S_j)                  (:315-317)
 * Backward, from g_Rs (23,3,3) and g_nll (23), each NULL when zero: dlog c / dS_k = (the same integral with a factor u, over the
 * cyclic shift that puts S_k first) / c~ (:187-219, :261-280); dL/dRs = g_Rs - g_nll target_R + overreg g_nll U diag(dlog c/dS . (1, 1, det)) V^T;
 * then back through Rodrigues, the joint layers (each scatters into h of its joint and of its ancestors: gathered per element in joint
 * order) and the MLP.  The gradient of EVERY parameter tensor is written (never accumulated into).  poses and target_R get none.
 *   params / grads: the 52 tensors in state_dict order -- block_mlps.{0,2,4}.{weight,bias}, then fc_pose.{0..22}.0.{weight,bias} --
 *     fp32, contiguous, (out,in) row-major as torch.nn.Linear stores them; fc_in[j] = the input width of fc_pose.j, which must be
 *     3 (1 + number of non-root ancestors of j) by `parents`;
 *   parents: 24 ints by value, parents[0] = -1 and 0 <= parents[i] < i (SMPL's kintree); poses (72), target_R (23,3,3): DEVICE
 *     pointers, so that a captured graph reads the frame's values at replay;
 *   Rs (23,3,3), S (23,3), nll (23): outputs; saved: MOSS_POSE_HEAD_SAVED_FLOATS device floats the backward reads (activations, r,
 *     U, V, det, c~) -- with S it must reach the backward unchanged.
 * U and V are not outputs: Rs is within 1e-5 of a rotation, its singular vectors are not unique; only S, det(U V^T) and the product
 * U diag(.) V^T enter any result.  One workgroup, sums in a fixed order, no atomics: bitwise reproducible.  No host synchronisation,
 * no allocation: capturable.  Bad arguments return MOSS_ERR_INVALID_ARG with moss_last_error() set.
 */
#define MOSS_POSE_JOINTS 23
#define MOSS_POSE_PARAMS 52
#define MOSS_POSE_HEAD_SAVED_FLOATS 896
typedef struct moss_pose_head_args {
    const float* poses;                      /* (72); the first 3 are not read */
    const float* target_R;                   /* (23,3,3) */
    const float* params[MOSS_POSE_PARAMS];
    int32_t parents[MOSS_POSE_JOINTS + 1];
    int32_t fc_in[MOSS_POSE_JOINTS];
    float overreg;                           /* MOSS: 1.005 */
    float* Rs;                               /* (23,3,3) */
    float* S;                                /* (23,3) proper singular values */
    float* nll;                              /* (23) */
    float* saved;                            /* MOSS_POSE_HEAD_SAVED_FLOATS */
} moss_pose_head_args;
int moss_pose_head_forward(const moss_pose_head_args* args, void* stream);

typedef struct moss_pose_head_backward_args {
    const float* poses;
    const float* target_R;
    const float* params[MOSS_POSE_PARAMS];
    int32_t parents[MOSS_POSE_JOINTS + 1];
    int32_t fc_in[MOSS_POSE_JOINTS];
    float overreg;
    const float* S;                          /* as the forward wrote it */
    const float* saved;                      /* as the forward wrote it */
    const float* g_Rs;                       /* (23,3,3) or NULL */
    const float* g_nll;                      /* (23) or NULL */
    float* grads[MOSS_POSE_PARAMS];          /* every one written, shaped as params */
} moss_pose_head_backward_args;
int moss_pose_head_backward(const moss_pose_head_backward_args* args, void* stream);

/*
 * The loss term alone for n general 3x3 matrices (utils/loss_utils.py:283-317 with the torch.svd of its caller): the same SVD and
 * quadrature code, one wave per matrix.  F, target_R (n,3,3); nll_out (n); dF_out (n,3,3) or NULL: d nll_i / d F_i =
 * -target_R_i + overreg U diag(dlog c/dS . (1, 1, det)) V^T.  Right for any F: either determinant sign, distinct or coinciding
 * singular values (tested to S = 80).  n = 0 launches nothing.  One launch, no host synchronisation, no allocation.
 */
int moss_matrix_fisher_nll(int n, const float* F, const float* target_R, float overreg, float* nll_out, float* dF_out, void* stream);

/*
 * MOSS's LBS-weight network (additive in ABI 7): pc.cross_attention_lbs(means3D[None], correct_Rs), gaussian_renderer/__init__.py:72 ->
 * CrossAttention_lbs.forward, nets/mlp_delta_weight_lbs.py:31-54 (the embedding: get_embedder(10), :87-133).  Per point x (3), with
 * the refined rotations Rs (23,3,3):
 *     e (63)  = [x, sin(x 2^0), cos(x 2^0), ..., sin(x 2^9), cos(x 2^9)]      the input first, per frequency three sines then three cosines
 *     h0 = relu(W0 e + b0), h1 = relu(W1 h0 + b1), h2 = relu(W2 h1 + b2), h3 = relu(W3 [e ; h2] + b3)     (:35-38; the skip puts e FIRST)
 *     q0 (24) = Wfc h3 + bfc (:39);  Q (24) = Wq q0 + bq (:46)
 *     M (24,9) = a row of nine ONES, then Rs[j] flattened (:43);  K = M Wk^T + bk,  V = M Wv^T + bv   (24,9) (:47-48)
 *     s (9) = sum_i Q[i] K[i,:] / sqrt(24);  a = softmax(s);  out[j] = sum_c a[c] V[j,c]   (24) (:49-52)
 * out_layer, gate_proj and num_heads are not read by that forward and cross no boundary.
 *   params / grads: the 16 tensors bw_linears.{0,1,2,3}.{weight,bias}, bw_fc.{weight,bias}, query.{weight,bias}, key.{weight,bias},
 *     value.{weight,bias} -- fp32, contiguous, (out,in) row-major (a Conv1d(k=1) weight (out,in,1) is exactly that);
 *   x (P,3), Rs (23,3,3), out (P,24), g_out (P,24), g_x (P,3), g_Rs (23,3,3): fp32 device arrays;
 *   saved: moss_lbs_weight_net_saved_bytes(P) bytes the forward writes (e, the four hidden activations, q0, Q, a per point:
 *     MOSS_LBS_WEIGHT_NET_SAVED_FLOATS each) and the backward reads; NULL in the forward = nothing is kept (no backward follows);
 *   workspace: moss_lbs_weight_net_workspace_bytes(P) bytes of scratch for the backward (contents irrelevant before, garbage after).
 * Forward: ONE launch, 32 points per workgroup, every layer on the f32-input matrix cores (exact float32).  Backward: THREE launches
 * -- the data gradients per tile of points (writes g_x and every layer's pre-activation gradient to the workspace), the weight
 * gradients as matrix products over the points with a FIXED split into MOSS_LBS_WEIGHT_NET_SPLITS ranges, and a fold of the partial
 * sums in split order that also forms the gradients of key / value and Rs.  Every output and gradient element is WRITTEN (no buffer
 * needs a zero fill), every sum has a fixed order and there is no atomic: bitwise reproducible.  No host synchronisation, no
 * allocation: capturable.  P = 0 is a no-op.  Bad arguments (a NULL required pointer, P < 0, a short workspace) return
 * MOSS_ERR_INVALID_ARG with moss_last_error() set.
 */
#define MOSS_LBS_WEIGHT_NET_PARAMS 16
#define MOSS_LBS_WEIGHT_NET_SAVED_FLOATS 640
#define MOSS_LBS_WEIGHT_NET_SPLITS 64
typedef struct moss_lbs_weight_net_args {
    int32_t P;
    const float* x;                          /* (P,3) */
    const float* Rs;                         /* (23,3,3) */
    const float* params[MOSS_LBS_WEIGHT_NET_PARAMS];
    float* out;                              /* (P,24) */
    float* saved;                            /* moss_lbs_weight_net_saved_bytes(P), or NULL */
} moss_lbs_weight_net_args;
int moss_lbs_weight_net_forward(const moss_lbs_weight_net_args* args, void* stream);   /* nets/mlp_delta_weight_lbs.py:31-54 */

typedef struct moss_lbs_weight_net_backward_args {
    int32_t P;
    const float* Rs;
    const float* params[MOSS_LBS_WEIGHT_NET_PARAMS];
    const float* saved;                      /* as the forward wrote it */
    const float* g_out;                      /* (P,24) */
    float* g_x;                              /* (P,3) */
    float* g_Rs;                             /* (23,3,3) */
    float* grads[MOSS_LBS_WEIGHT_NET_PARAMS];/* every one written, shaped as params */
    char* workspace;
    size_t workspace_bytes;
} moss_lbs_weight_net_backward_args;
int moss_lbs_weight_net_backward(const moss_lbs_weight_net_backward_args* args, void* stream);   /* the adjoint of nets/mlp_delta_weight_lbs.py:31-54 */
size_t moss_lbs_weight_net_workspace_bytes(int P);  /* scratch of the backward of nets/mlp_delta_weight_lbs.py:31-54; 0 for P <= 0 */
size_t moss_lbs_weight_net_saved_bytes(int P);      /* what its forward keeps for the backward; 0 for P <= 0 */
/*
 * The same pair in the split-bf16 (three-product) mode (additive in ABI 7).  In the five wide products (layers 0-3 and bw_fc) --
 * forward (activation x weight), data gradient (d pre-activation x weight) and weight gradient (d pre-activation x layer input, summed
 * over the points) -- both operands are split, hi = bf16(a) (round to nearest even), lo = bf16(a - hi), and a b is taken as
 * lo(a) hi(b) + hi(a) lo(b) + hi(a) hi(b) on the bf16-input matrix cores; all sums are float32.  The embedding, the biases and their
 * gradients, the ReLU masks, query / key / value, the scores, the softmax, the output and g_x from d e are float32 as above.  Same
 * argument blocks, same launches, same refusals, same determinism; `saved` and
 * the workspace have the SAME layouts and sizes (moss_lbs_weight_net_saved_bytes / _workspace_bytes).  A forward's `saved` belongs to
 * the backward of the same mode.
 */
int moss_lbs_weight_net_forward_bf16x3(const moss_lbs_weight_net_args* args, void* stream);   /* nets/mlp_delta_weight_lbs.py:31-54, split-bf16 products */
int moss_lbs_weight_net_backward_bf16x3(const moss_lbs_weight_net_backward_args* args, void* stream);   /* the adjoint of nets/mlp_delta_weight_lbs.py:31-54, split-bf16 products */

/*
 * MOSS's LPIPS term (additive in ABI 7): loss_fn_vgg(img_pred, img_gt), train_ZJU.py:121 (weighted 0.5 at :131) and :256 ->
 * LPIPS.forward with net_type='vgg', lpipsPyTorch/modules/lpips.py:31-37 (BaseNet.forward networks.py:49-62, VGG16 :87-95,
 * normalize_activation utils.py:5-7):
 *     z = (img - shift) / scale                                    per channel
 *     VGG16 features[0:30]: 13 x (conv 3x3, padding 1, bias, ReLU), widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512,
 *                           a 2x2 stride-2 max-pool (floor) between the groups
 *     tap l = the activations after ReLU 1_2, 2_2, 3_3, 4_3, 5_3:   n = f / (sqrt(sum_c f^2) + 1e-10) per pixel
 *     term_l = mean over pixels of sum_c lin_l[c] (nx - ny)^2;   out = sum_l term_l
 * Both images run as one batch of two; the weights are frozen and y gets no gradient, so the backward is the data gradient w.r.t. x.
 *   x, y: (3,frame_H,frame_W) fp32 planes; the term is taken on the crop of H x W pixels whose corner is rect[0] (x), rect[1] (y) --
 *     DEVICE ints as moss_photometric_loss_roi's, moved so that the crop fits the frame -- or (0,0) with rect NULL; frame_H = frame_W
 *     = 0 means the frame is the crop.  H, W >= 16, H * W <= 2^22, and H <= 32768, W <= 65536 (the convolution kernels keep a
 *     pixel's y and x in the two halves of one signed 32-bit word); neither needs to be a multiple of anything.
 *   weights / biases: per convolution, packed by moss_lpips_vgg_pack_weights (`fwd`); lin: 5 arrays of 64, 128, 256, 512, 512 floats;
 *     shift, scale: 3 device floats each.  weights_bwd: the `bwd` arrays of the same packing.
 *   out: 1 device float; terms: 5 device floats or NULL; saved: moss_lpips_vgg_saved_bytes(H, W) bytes the forward writes for the
 *     backward -- one sign bit per activation of x, two bits per pooled activation (which of the four won), and per tap d term_l / d fx
 *     -- or NULL: nothing is kept (an evaluation call);
 *   g_out: the upstream gradient of `out`, 1 DEVICE float; dL_dx (3,frame_H,frame_W): written everywhere, zero off the crop;
 *   workspace: moss_lpips_vgg_workspace_bytes(H, W) bytes of scratch for either call (monotonic in H * W: one sized for the frame
 *     serves every crop), contents irrelevant before, garbage after.
 * Every convolution but the first runs on the f32-input matrix cores in exact float32.  No host synchronisation, no allocation:
 * capturable; a captured step changes view by rewriting `rect`.  Every sum has a fixed order and there is no atomic: bitwise
 * reproducible.  Bad arguments (a NULL required pointer, a size outside the range, a short workspace) return MOSS_ERR_INVALID_ARG
 * with moss_last_error() set.
 *
 * A crop whose SIZE changes under a captured step (additive in ABI 7): cap_H, cap_W, the last two fields of both blocks.  0, 0 is the
 * static call above.  With a capacity set -- the largest crop the call will ever see, within the range of H, W above, no larger
 * than the frame -- rect is required and H, W are ignored: every kernel reads w = rect[2], h = rect[3] on the device (clamped into
 * [16, capacity] per axis for memory safety; the caller validates on the host where it can see the rectangle) and derives each level's
 * sizes, the row counts, the pool and tap extents and the 1 / (H_l W_l) of the means from them.  The launches, `workspace` and `saved`
 * are sized for the capacity: workspace_bytes >= moss_lpips_vgg_workspace_bytes(cap_H, cap_W), saved holds
 * moss_lpips_vgg_saved_bytes(cap_H, cap_W), and the backward is given the capacity the forward had.  Zero padding is at the actual
 * crop's edge, the frame outside the crop is never read, dL_dx is zero off the actual crop, and nothing depends on what `workspace`
 * or `saved` held before.  The arithmetic is the static call's.  The wide convolution has two kernel shapes which sum K in different
 * orders, picked on the host from the row count -- with a capacity from the capacity's -- so a call with a capacity is BIT-IDENTICAL
 * to the static call at the same h x w exactly when every layer gets the same shape in both: always when the crop equals the
 * capacity, and for any capacity up to 64 x 64 on a device with more than 64 CUs (both then take the narrow shape everywhere).
 * Otherwise the two agree to float32 summation order, and each is as close to float64 as the other.  Refused with
 * MOSS_ERR_INVALID_ARG: a capacity with rect NULL, one outside the range, one larger than the frame, only one of cap_H / cap_W set,
 * a workspace shorter than the capacity's.
 */
#define MOSS_LPIPS_VGG_CONVS 13
#define MOSS_LPIPS_VGG_TAPS 5
typedef struct moss_lpips_vgg_args {
    const float* x;                          /* (3,frame_H,frame_W) */
    const float* y;
    int32_t H, W;                            /* the crop */
    int32_t frame_H, frame_W;                /* 0, 0 = H, W */
    const int* rect;                         /* device ints {x, y, ...} or NULL */
    const float* weights[MOSS_LPIPS_VGG_CONVS]; /* moss_lpips_vgg_forward_bf16: [1..12] are the uint16_t `fwd` arrays of ..._pack_weights_bf16 */
    const float* biases[MOSS_LPIPS_VGG_CONVS];
    const float* lin[MOSS_LPIPS_VGG_TAPS];
    const float* shift;
    const float* scale;
    float* out;
    float* terms;                            /* 5 floats, or NULL */
    char* saved;                             /* moss_lpips_vgg_saved_bytes(H, W) (of cap_H, cap_W with a capacity), or NULL */
    char* workspace;
    size_t workspace_bytes;
    int32_t cap_H, cap_W;                    /* 0, 0 = the static call; else the crop's size is rect[3] x rect[2], at most this */
} moss_lpips_vgg_args;
int moss_lpips_vgg_forward(const moss_lpips_vgg_args* args, void* stream);   /* lpipsPyTorch/modules/lpips.py:31-37 */

typedef struct moss_lpips_vgg_backward_args {
    int32_t H, W;
    int32_t frame_H, frame_W;
    const int* rect;
    const float* weights_bwd[MOSS_LPIPS_VGG_CONVS]; /* moss_lpips_vgg_backward_bf16: [1..12] are the uint16_t `bwd` arrays of ..._pack_weights_bf16 */
    const float* scale;
    const char* saved;                       /* as the forward wrote it */
    const float* g_out;                      /* 1 device float */
    float* dL_dx;                            /* (3,frame_H,frame_W) */
    char* workspace;
    size_t workspace_bytes;
    int32_t cap_H, cap_W;                    /* the forward's */
} moss_lpips_vgg_backward_args;
int moss_lpips_vgg_backward(const moss_lpips_vgg_backward_args* args, void* stream);   /* the adjoint of lpipsPyTorch/modules/lpips.py:31-37 w.r.t. x */
size_t moss_lpips_vgg_workspace_bytes(int H, int W);  /* scratch of either call; 0 for a size outside the range */
size_t moss_lpips_vgg_saved_bytes(int H, int W);      /* what the forward keeps for the backward; 0 for a size outside the range */
/* w (cout,cin,3,3) fp32 -> fwd [cout][tap][cin] and bwd [cin][8 - tap][cout] (cout * cin * 9 floats each): once, the weights are frozen */
int moss_lpips_vgg_pack_weights(int cin, int cout, const float* w, float* fwd, float* bwd, void* stream);

/*
 * The same term with bf16 OPERANDS in the twelve wide convolutions (additive in ABI 7): a mixed-precision form of the TRAINING term.
 * The float32 calls above stay the default, keep their results bit for bit, and are the only form an evaluation metric may use.
 * The arithmetic, exactly: in convolutions 2..13 (conv 1_2 .. 5_3), forward and data gradient alike, both operands of every product
 * are rounded to bf16 with round-to-nearest-even -- the weights once, by moss_lpips_vgg_pack_weights_bf16; the activations (forward)
 * and the incoming gradients (backward) each time a slice of them is staged for the matrix cores, while in memory they stay float32.
 * A product of two bf16 values is exact in float32, and every sum is accumulated in float32 (v_mfma_f32_32x32x16_bf16), in a fixed
 * order.  Nothing else is rounded: conv 1_1 and its adjoint, the bias, ReLU, the pools, the taps and the means are the float32 call's.
 * It is lpips_vgg_torch(..., operand_dtype=torch.bfloat16) of moss_amd/lpips.py up to float32 summation order.
 *
 * Both calls take the argument blocks of the float32 pair, REINTERPRETED in one place: weights[1..12] / weights_bwd[1..12] point at the
 * uint16_t arrays of moss_lpips_vgg_pack_weights_bf16 (`fwd` / `bwd`: the two layouts of the float32 packer, cout * cin * 9 16-bit
 * values each); weights[0] / weights_bwd[0] (conv 1_1) are the float32 packing.  Everything else -- sizes, rect, the capacity and its
 * bit-identity rule (the shapes are picked the same way), `saved`, `workspace` and their sizes, capturability, bitwise
 * reproducibility, every element of dL_dx written, the refusals and the texts of moss_last_error() -- is the float32 pair's; a `saved`
 * block goes to the backward of the precision that wrote it.
 */
int moss_lpips_vgg_forward_bf16(const moss_lpips_vgg_args* args, void* stream);
int moss_lpips_vgg_backward_bf16(const moss_lpips_vgg_backward_args* args, void* stream);
int moss_lpips_vgg_pack_weights_bf16(int cin, int cout, const float* w, uint16_t* fwd, uint16_t* bwd, void* stream);

/*
 * ONE of the wide convolutions of the term above, on its own (additive in ABI 7): the 3x3, padding-1 convolution of conv 1_2 .. 5_3,
 * forward or data gradient, through the launcher the two full calls use and so on the very kernels they run -- with the kernel SHAPE
 * named by the caller, which the full calls pick from the row count and the device's compute units.  It exists so that a layer can be
 * checked per element, in either shape, at sizes of a few rows; the full calls are the product's path.
 *   in: (nimg * H * W, cin) fp32 channels-last, row m = img * H * W + y * W + x; out: (nimg * H * W, cout).  cin, cout: multiples of 64.
 *   weights: the `fwd` (mode 0) or `bwd` (modes 1, 2) array of moss_lpips_vgg_pack_weights -- of ..._pack_weights_bf16 with bf16 = 1 --
 *     packed with the (cin, cout) of the FORWARD layer; for a data gradient this call's cin is that layer's cout and the other way round.
 *   mode 0, forward: out = relu(conv(in) + bias); mask_out, if given, gets the sign words of the rows of the FIRST image (H * W rows).
 *   mode 1, data gradient below a ReLU: out = conv(in) with the flipped, transposed weights where the bit of mask_in is set, +0 elsewhere.
 *   mode 2, data gradient below a pool: the same, unmasked.
 *   MASK WORDS: row-major, cout / 32 uint32_t per row; bit j of word k of row m is channel 32 k + j of that row (set: the activation
 *     was > 0).  mask_in has a row for every row of `out`.
 *   shape: 0 the launcher's own choice, 1 the 128-row shape, 2 the 32-row split-K shape (bf16: its slice is 128 channels where cin is a
 *     multiple of 128, else 64, as in the full calls).  The two shapes sum K in different orders.
 *   rect, cap_H, cap_W, level: the dynamic form of the full calls.  With a capacity (both > 0; 16 <= cap, within the range below) rect is
 *     required, H and W are ignored, the grid is sized for (cap_H >> level) x (cap_W >> level), level 0..4, and the kernel reads
 *     h = rect[3], w = rect[2] on the device, clamps them into [16, capacity] and halves them `level` times.  The rows are compact at that
 *     size; rows beyond it are not written.
 * Static sizes: H, W >= 1 (the levels a 16-pixel crop reaches are 1 x 1), H <= 32768, W <= 65536, H * W <= 2^22.  No host
 * synchronisation, no allocation.  Refused with MOSS_ERR_INVALID_ARG and a text: a NULL block, in, weights or out, bias (mode 0) or
 * mask_in (mode 1); cin or cout not a positive multiple of 64; a mode, shape, bf16 or level out of range; nimg outside 1..2; a size
 * < 1 or beyond the range; a capacity without rect, outside the range, or with only one of cap_H / cap_W set.
 */
typedef struct moss_lpips_conv3x3_args {
    const float* in;
    const void* weights;                     /* float (bf16 = 0) or uint16_t (bf16 = 1) */
    const float* bias;                       /* mode 0: cout floats */
    float* out;
    const uint32_t* mask_in;                 /* mode 1 */
    uint32_t* mask_out;                      /* mode 0, or NULL */
    int32_t nimg, H, W, cin, cout;
    int32_t mode;                            /* 0 forward, 1 data gradient masked by ReLU bits, 2 data gradient plain */
    int32_t shape;                           /* 0 the launcher's choice, 1 128 rows, 2 32 rows with split K */
    int32_t bf16;                            /* 0 or 1 */
    const int* rect;                         /* device ints {x, y, w, h}; required with a capacity */
    int32_t cap_H, cap_W, level;             /* 0, 0 = the static call */
} moss_lpips_conv3x3_args;
int moss_lpips_vgg_conv3x3(const moss_lpips_conv3x3_args* args, void* stream);

/*
 * The same term with SPLIT-bf16 operands in the twelve wide convolutions (additive in ABI 7): three bf16 products per float32 product,
 * about 16 bits of every operand -- between the float32 calls and the bf16 ones in cost and in accuracy.  A form of the TRAINING term;
 * the float32 calls stay the default, keep their bits, and are the only form an evaluation metric may use.
 * The arithmetic, exactly: for a float32 value a let hi(a) = bf16_rne(a) and lo(a) = bf16_rne(a - hi(a)) (the subtraction is exact in
 * float32).  In convolutions 2..13 (conv 1_2 .. 5_3), forward and data gradient alike, every product a b is replaced by
 *     hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b)
 * -- each bf16 x bf16 product exact in float32, every sum float32 in a fixed order (on v_mfma_f32_32x32x16_bf16; the hi hi products in
 * one accumulator, the two small terms in another -- per sixteen k lo hi, then hi lo -- the two added per element after the last k),
 * the lo lo term dropped.  The weights are split once, by moss_lpips_vgg_pack_weights_bf16x3; the
 * activations (forward) and the incoming gradients (backward) each time a slice of them is staged, while in memory they stay float32.
 * Nothing else changes: conv 1_1 and its adjoint, the bias, ReLU and its sign words, the pools, the taps, unpool and the means are the
 * float32 call's kernels.  Per element the split sum is held to 2^-16 x mass of the unsplit product sum, mass = conv(|in|, |w|) +
 * |bias| (measured: 0.04-0.12 of it).  One product alone: |lo| <= 2^-8 |a|, |a - hi - lo| <= 2^-17 |a| for either operand and the dropped
 * product is at most 2^-16 |a b|, so it is off by at most 2^-15 |a b|; a sum's roundings are not all at their worst at once.
 * A lo below bf16's normal range (|lo| < 2^-126) may be flushed to zero by the matrix core; that is not part of the contract.
 * The split convolution equals one plain convolution over 3 cin channels, inputs [lo, hi, hi] against weights [hi, lo, hi]; it is
 * lpips_vgg_torch(..., operand_dtype=torch.bfloat16, operand_split=True) of moss_amd/lpips.py up to float32 summation order.
 *
 * moss_lpips_vgg_pack_weights_bf16x3: `fwd` and `bwd` hold 2 * cout * cin * 9 16-bit values each, two planes in the layouts of the
 * float32 packer: [0, n) the hi plane -- bit for bit what moss_lpips_vgg_pack_weights_bf16 writes -- and [n, 2n) the lo plane.
 * moss_lpips_vgg_forward_bf16x3 / _backward_bf16x3 take the argument blocks of the float32 pair, REINTERPRETED in one place:
 * weights[1..12] / weights_bwd[1..12] point at those arrays; [0] (conv 1_1) is the float32 packing.  Everything else -- sizes, rect, the
 * capacity and its bit-identity rule, `saved`, `workspace` and their sizes, capturability, bitwise reproducibility, every element of
 * dL_dx written, the refusals and the texts of moss_last_error() -- is the float32 pair's; a `saved` block goes to the backward of the
 * precision that wrote it.
 * moss_lpips_vgg_conv3x3_bf16x3: ONE layer on the split kernels, the block and the rules of moss_lpips_vgg_conv3x3 with `weights` the
 * split packing (uint16_t) and the bf16 field required to be 0; the slices are the bf16 call's (64 channels, 128 in the 32-row shape
 *   where cin is a multiple of 128).
 */
int moss_lpips_vgg_forward_bf16x3(const moss_lpips_vgg_args* args, void* stream);
int moss_lpips_vgg_backward_bf16x3(const moss_lpips_vgg_backward_args* args, void* stream);
int moss_lpips_vgg_pack_weights_bf16x3(int cin, int cout, const float* w, uint16_t* fwd, uint16_t* bwd, void* stream);
int moss_lpips_vgg_conv3x3_bf16x3(const moss_lpips_conv3x3_args* args, void* stream);

/*
 * The ground truth's half of the term, computed ONCE (additive in ABI 7).  y is fixed per camera -- viewpoint_cam.original_image
 * cropped to its bound_mask's rectangle, train_ZJU.py:108-121 -- yet both calls above run VGG16 on it every time.  A REFERENCE is what
 * y contributes, kept by the caller and accepted in y's place:
 *   moss_lpips_vgg_reference{,_bf16,_bf16x3}: the forward on y ALONE (one image, M = H W rows) -- feat_y = self.net(y),
 *     lpipsPyTorch/modules/lpips.py:32, second half -- with no sign masks, pool winners or tap gradients.  It leaves the tapped
 *     activations in `reference`.
 *   moss_lpips_vgg_forward_ref{,_bf16,_bf16x3}: lpipsPyTorch/modules/lpips.py:31-37 on x ALONE with feat_y read from `reference`; out,
 *     terms and `saved` are those of moss_lpips_vgg_forward, in its layout, and moss_lpips_vgg_backward{,_bf16,_bf16x3} of the same
 *     precision takes that `saved` unchanged.
 * THE BLOCK: moss_lpips_vgg_reference_bytes(H, W) bytes (0 for a size the calls refuse), five regions in tap order -- the RAW
 * activations after ReLU 1_2, 2_2, 3_3, 4_3, 5_3 (the normalisation of lpips.py:34 is done by the tap, by the float32 operations
 * the two-image call uses) -- region l at the sum of the sizes before it, each (H >> l) * (W >> l) * C_l * 4 bytes rounded up to 256,
 * C = 64, 128, 256, 512, 512; inside a region row y * W_l + x, C_l floats, channels-last.  That is 122 floats per crop pixel: 22 MB at
 * 256 x 176.  With a capacity the regions are laid out for cap_H x cap_W and the rows are compact at the ACTUAL size, as in `saved`; a
 * block may be copied (all its bytes) into another of the same capacity.  A block is valid for ONE (weights, precision, crop size or
 * capacity): in the bf16 modes y's activations are what that mode's kernels compute for y.
 *   y / x: (3,frame_H,frame_W); H, W, frame_H, frame_W, rect, cap_H, cap_W, weights, biases, lin, shift, scale, out, terms, saved,
 *   workspace: as in moss_lpips_vgg_args (the crop of y starts where the two-image call's does: rect's corner, moved so that the crop
 *   fits).  workspace: moss_lpips_vgg_workspace_bytes, the two-image call's.
 * THE SAME RESULT: per row the convolution does not know how many images the batch holds; what can differ is the kernel shape, picked
 * from the row count, which is H W here and 2 H W in the two-image call.  out, terms, `saved` and so the gradient are BIT-IDENTICAL to
 * the two-image call of the same inputs and capacity whenever every wide layer gets the same shape at M = H W as at M = 2 H W: on a
 * device with more than 122 CUs, for every crop or capacity up to 101 x 77 (all layers take the 32-row shape either way).  Otherwise
 * the two agree to float32 summation order and are as close to float64 as each other.
 * No host synchronisation, no allocation: capturable; bitwise reproducible.  Refused with MOSS_ERR_INVALID_ARG before any launch, the
 * field named in moss_last_error(): a NULL block, y / x, out, shift, scale, weight, bias or lin; a `reference` that is NULL or shorter
 * than moss_lpips_vgg_reference_bytes; a short workspace; a capacity without rect; every size the two-image call refuses.
 */
typedef struct moss_lpips_vgg_reference_args {
    const float* y;                          /* (3,frame_H,frame_W): the ground truth */
    int32_t H, W;
    int32_t frame_H, frame_W;
    const int* rect;
    const float* weights[MOSS_LPIPS_VGG_CONVS]; /* the precision's `fwd` packing, as in moss_lpips_vgg_args */
    const float* biases[MOSS_LPIPS_VGG_CONVS];
    const float* shift;
    const float* scale;
    char* reference;                         /* written: moss_lpips_vgg_reference_bytes(H, W) (of cap_H, cap_W with a capacity) */
    size_t reference_bytes;
    char* workspace;
    size_t workspace_bytes;
    int32_t cap_H, cap_W;
} moss_lpips_vgg_reference_args;
typedef struct moss_lpips_vgg_forward_ref_args {
    const float* x;                          /* (3,frame_H,frame_W) */
    const char* reference;                   /* as moss_lpips_vgg_reference of this precision, weights and size / capacity wrote it */
    size_t reference_bytes;
    int32_t H, W;
    int32_t frame_H, frame_W;
    const int* rect;
    const float* weights[MOSS_LPIPS_VGG_CONVS];
    const float* biases[MOSS_LPIPS_VGG_CONVS];
    const float* lin[MOSS_LPIPS_VGG_TAPS];
    const float* shift;
    const float* scale;
    float* out;
    float* terms;                            /* 5 floats, or NULL */
    char* saved;                             /* moss_lpips_vgg_saved_bytes, or NULL */
    char* workspace;
    size_t workspace_bytes;
    int32_t cap_H, cap_W;
} moss_lpips_vgg_forward_ref_args;
size_t moss_lpips_vgg_reference_bytes(int H, int W);
int moss_lpips_vgg_reference(const moss_lpips_vgg_reference_args* args, void* stream);          /* lpipsPyTorch/modules/lpips.py:32, y's half */
int moss_lpips_vgg_reference_bf16(const moss_lpips_vgg_reference_args* args, void* stream);
int moss_lpips_vgg_reference_bf16x3(const moss_lpips_vgg_reference_args* args, void* stream);
int moss_lpips_vgg_forward_ref(const moss_lpips_vgg_forward_ref_args* args, void* stream);      /* lpipsPyTorch/modules/lpips.py:31-37 */
int moss_lpips_vgg_forward_ref_bf16(const moss_lpips_vgg_forward_ref_args* args, void* stream);
int moss_lpips_vgg_forward_ref_bf16x3(const moss_lpips_vgg_forward_ref_args* args, void* stream);

/*
 * k nearest reference points of every query point, 3-D, exact, k = 1..4: replaces the third-party
 * `knn_cuda.KNN(k, transpose_mode=True)(ref, query)` MOSS calls at scene/gaussian_model.py:85-86,586,657,759,827 (a CUDA-only
 * binary wheel, not in the repository; parity unpinned by the reference).
 *   ref (Nr,3), query (Nq,3) fp32 device arrays; dist_out (Nq,k) Euclidean distances ascending; idx_out (Nq,k) int64 reference
 *   indices.  Nr >= k.  Ties: the lower reference index first.  Asynchronous on `stream`.
 */
int moss_knn_query(int Nr, int Nq, int k, const float* ref, const float* query, float* dist_out, long long* idx_out, void* stream);

/*
 * The same query through a uniform cell grid over the references (exact; results identical to moss_knn_query bit for bit, ties
 * included).  Built once per reference set (8 small launches), queried any number of times: MOSS queries the SAME template
 * vertices every step (scene/gaussian_model.py:827) and the Gaussians themselves when densifying (:586,759; 100k x 100k is 7.7 ms
 * by brute force).  workspace: moss_knn_grid_workspace_bytes(Nr) device bytes, owned by the caller, read-only for queries.
 * Cost grows with the distance between a query and its k-th neighbour measured in cells (about two cells per reference): meant
 * for queries that lie among the references; far outliers stay exact but approach brute-force cost.  Asynchronous on `stream`.
 */
size_t moss_knn_grid_workspace_bytes(int Nr);
int moss_knn_grid_build(int Nr, const float* ref, char* workspace, size_t workspace_bytes, void* stream);
int moss_knn_grid_query(int Nr, int Nq, int k, const char* workspace, size_t workspace_bytes, const float* query,
                        float* dist_out, long long* idx_out, void* stream);

/*
 * The nearest reference of every query, k = 1, against a vertex set that never changes, through an index built ONCE: replaces MOSS's
 * per-step knn(t_vertices, query_pts) (scene/gaussian_model.py:827; the vertices are view.big_pose_world_vertex, the same every
 * step) and the vertex distance of the final prune (:657).  Exact: ids and distances equal moss_knn_query(k = 1) bit for bit, ties
 * to the lower vertex index; a query with a non-finite coordinate gets id -1 and distance +inf, as there.  (csrc/nearest_vertex.hip)
 *   moss_nearest_vertex_index_bytes(V): device bytes of the index, 1 <= V <= 65536 (0 outside that range).
 *   moss_nearest_vertex_build: vertices (V,3) fp32 -> index (caller-owned; a snapshot of the vertices: Morton-ordered blocks of 64
 *     with their boxes).  Three launches on `stream`, no host read.
 *   moss_nearest_vertex_query: points (P,3) fp32 -> ids_out (P) int64, dist_out (P) fp32 Euclidean distances or NULL.  ONE launch on
 *     `stream`, no host read, no allocation: capturable.  The index is read-only.  P = 0 is a no-op.
 * Bad arguments (V outside 1..65536, P < 0, a NULL pointer, index_bytes below moss_nearest_vertex_index_bytes(V)) return
 * MOSS_ERR_INVALID_ARG with moss_last_error() set and launch nothing.
 */
size_t moss_nearest_vertex_index_bytes(int V);
int moss_nearest_vertex_build(int V, const float* vertices, char* index, size_t index_bytes, void* stream);
int moss_nearest_vertex_query(int V, int P, const char* index, size_t index_bytes, const float* points,
                              long long* ids_out, float* dist_out /* may be NULL */, void* stream);

/*
 * Densification bookkeeping, one launch, no host synchronisation.  Replaces, for vis = radii > 0,
 *   gaussians.max_radii2D[vis] = max(max_radii2D[vis], radii[vis])                          (train_ZJU.py:173)
 *   xyz_gradient_accum[vis] += norm(viewspace_points.grad[vis,:2], dim=-1); denom[vis] += 1  (scene/gaussian_model.py:815-817)
 * radii (P) int32 from the forward; viewspace_grad (P, grad_stride >= 2) = dL_dmeans2D of the backward;
 * xyz_gradient_accum (P), denom (P), max_radii2D (P, may be NULL) fp32, updated in place.
 */
int moss_densify_stats(int P, const int* radii, const float* viewspace_grad, int grad_stride,
                       float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream);
/*
 * KL divergence between pairs of Gaussians, with the gather fused in: replaces GaussianModel.kl_div
 * (scene/gaussian_model.py:773-813) applied to the pairs picked by the k = 2 self-query (:586-597, :759-770).
 *   xyz (Nsrc,3), rotation (Nsrc,4) raw quaternions (normalised inside like build_rotation, utils/general_utils.py:79-100),
 *   scaling (Nsrc,3) ACTIVATED scales; pair_idx (P,2) int64 = the kNN result (column 0: Gaussian "0", column 1: Gaussian "1");
 *   kl_out (P) = 0.5 (tr(S1^-1 S0) + (mu1-mu0)^T S1^-1 (mu1-mu0) + ln prod((s1/s0)^2) - 3).  An out-of-range index gives NaN.
 */
int moss_neighbour_kl(int P, int Nsrc, const float* xyz, const float* rotation, const float* scaling,
                      const long long* pair_idx, float* kl_out, void* stream);

/*
 * The KL densify-and-prune DECISION of MOSS (GaussianModel.densify_and_prune, scene/gaussian_model.py:621-666, and the three phase
 * functions it calls: kl_densify_and_clone :495-526, kl_densify_and_split :528-571, kl_merge :573-619), additive in ABI 7.  The
 * surface-change test of the clone (:503-507) is an INPUT (surface_mask).  All tensors fp32 and contiguous unless said otherwise; every
 * entry point enqueues on `stream`, allocates nothing and reads nothing back on the host.  Bad arguments (a NULL required pointer, a
 * negative size, a short workspace, an unknown mode) return MOSS_ERR_INVALID_ARG with moss_last_error() set and launch nothing.
 *
 * moss_densify_joint_table (:624-640): ONE launch, one lane per joint.  F_j = joint_F_sum[j] / denom[0] (denom[0] is read on the
 *   device), its 3x3 SVD (one-sided Jacobi, csrc/pose_math.h), the sign rule U[:,2] *= det U, V[:,2] *= det V (:628-633), rot = U V^T.
 *   table (24,12): row 0 is twelve ONES (torch.ones(1,3,3) and torch.ones(1,3) at :637,640 -- not the identity); row j+1 holds the
 *   nine floats of rot_j row-major and the three singular values in descending order.  A joint whose F has a non-finite element
 *   (denom[0] == 0) gets twelve NaNs.
 *
 * moss_densify_select: the selection mask of one phase, its ascending index list and its count.
 *   grad_i = xyz_gradient_accum[i] / denom[i] with NaN -> 0 (:622,642) for i < n_grads and 0 beyond (the zero padding of :540-541);
 *   smax_i = max_k exp(scaling[i,k]);  KL_i = kl_div of Gaussian ids[i,0] against ids[i,1] (moss_neighbour_kl's arithmetic on
 *   exp(scaling)); an index of ids outside [0,P) unselects i (its KL is NaN).
 *   MOSS_DENSIFY_CLONE (:499-509): |grad| >= max_grad && smax <= scale_limit && KL > kl_threshold && surface_mask[i] (NULL = all set)
 *   MOSS_DENSIFY_SPLIT (:540-549):  grad  >= max_grad && smax >  scale_limit && KL > kl_threshold
 *   MOSS_DENSIFY_MERGE (:579-602):  grad  >= max_grad && smax <= scale_limit && KL < kl_threshold
 *   MOSS_DENSIFY_PRUNE (:650-662): sigmoid(opacity[i]) < min_opacity || (use_screen_size && (max_radii2D[i] > max_screen_size ||
 *     smax > world_scale_limit)) || vertex_dist[i] > vertex_dist_limit      (vertex_dist: the k = 1 query against the SMPL vertices)
 *   scale_limit = percent_dense * extent, world_scale_limit = 0.1 * extent: formed by the caller.
 *   mask (P) bytes 0/1; index (>= count) int32: the selected i in ASCENDING order (the row order of boolean indexing), entries beyond
 *   the count untouched, may be NULL; count: one device int32; count_host: one int32 of PINNED host memory that receives the count by
 *   an asynchronous copy on `stream` (may be NULL) -- the caller's single host read per phase; kl_out (P), may be NULL: KL_i, bit
 *   for bit what moss_neighbour_kl returns for the scales THIS library activates (the device expf of its kernels: what
 *   moss_gaussian_activate_forward writes as out_scaling); nothing is promised about another library's exp.
 *   The KL is computed by moss_neighbour_kl's OWN kernel on exp(scaling) (one launch to activate the scales, one for the KL):
 *   the same machine code, so the same bits.  Then the ordered compaction in TWO launches: flags + per-workgroup totals (wave
 *   ballots, an LDS sum), then the offsets (each workgroup sums the totals before it -- integers, no atomic) and the ranks (ballot +
 *   popcount in the wave, wave totals through LDS).  Bitwise reproducible.  PRUNE: the two compaction launches only.
 *   workspace: moss_densify_select_workspace_bytes(P) bytes (per-workgroup totals, activated scales, the KL); PRUNE needs only the
 *   first 4 * ceil(P / 256) of them, the totals.
 *
 * moss_densify_emit: the new rows of one phase from the index list (n_sel = the count the caller read).  Features: features_dc /
 *   features_rest point at the 3 / rest_floats floats of a row, rows dc_stride / rest_stride floats apart (two tensors: 3 and
 *   rest_floats; views of one (P,16,3) tensor: 48 and 48); copies run with the lanes along a row's 3 + rest_floats floats.
 *   R(q) = build_rotation (utils/general_utils.py:79-100); noise (n_new,3): standard normal draws, row r uses noise[r]
 *   (torch.normal(mean, std) = mean + std * noise).
 *   CLONE (:511-524), n_new = n_sel, i = index[r]:  w = lbs_weights[i,:] / denom[0] (24);  rot_joint = w . table[:, :9],
 *     scl_joint = w . table[:, 9:] (the table is held in LDS; nothing of size (P,3,3) exists);  std = scl_joint * exp(scaling[i]);
 *     new_xyz = (rot_joint R(q_i)) (std * noise[r]) + xyz[i];  new_scaling = log(exp(scaling[i]) * scl_joint);
 *     new_rotation = matrix_to_quaternion(rot_joint) * rotation[i] ELEMENTWISE (what :520 computes); matrix_to_quaternion as in
 *     pytorch3d (real part first, the candidate of the largest component, no sign standardisation); features, opacity copied.
 *   SPLIT (:551-566), n_new = 2 n_sel, i = index[r mod n_sel] (the repeat(2,1) layout):  new_xyz = R(q_i)(exp(scaling[i]) * noise[r])
 *     + xyz[i];  new_scaling = log(exp(scaling[i]) / 1.6);  everything else copied.
 *   MERGE (:606-616), n_new = n_sel, (a,b) = ids[index[r],:]:  means of the pair for xyz, both feature tensors and the raw opacity;
 *     new_scaling = log(exp(scaling[a]) / 0.8);  new_rotation = rotation[a];  prune_mask[b] = 1 (bytes; the select's mask).
 *   An index outside [0,P) (a stale list) writes a row of zeros and reads nothing.
 */
#define MOSS_DENSIFY_CLONE 0
#define MOSS_DENSIFY_SPLIT 1
#define MOSS_DENSIFY_MERGE 2
#define MOSS_DENSIFY_PRUNE 3
#define MOSS_DENSIFY_JOINTS 24
int moss_densify_joint_table(const float* joint_F_sum /* (23,3,3) */, const float* denom, float* table /* (24,12) */, void* stream);

typedef struct moss_densify_select_args {
    int32_t mode;                            /* MOSS_DENSIFY_* */
    int32_t P, n_grads;                      /* n_grads <= P rows carry a gradient */
    const float* xyz_gradient_accum;         /* (n_grads) */
    const float* denom;                      /* (n_grads) */
    const float* xyz;                        /* (P,3) */
    const float* rotation;                   /* (P,4) raw */
    const float* scaling;                    /* (P,3) raw (logarithms) */
    const float* opacity;                    /* (P) raw (logits); PRUNE */
    const long long* ids;                    /* (P,2): the k = 2 self query; CLONE / SPLIT / MERGE */
    const uint8_t* surface_mask;             /* (P) or NULL; CLONE */
    const float* max_radii2D;                /* (P); PRUNE with use_screen_size */
    const float* vertex_dist;                /* (P); PRUNE */
    float max_grad, scale_limit, kl_threshold;
    float min_opacity, max_screen_size, world_scale_limit, vertex_dist_limit;
    int32_t use_screen_size;
    uint8_t* mask;                           /* (P) */
    int32_t* index;                          /* (>= count) or NULL */
    int32_t* count;                          /* device */
    int32_t* count_host;                     /* pinned host, or NULL */
    float* kl_out;                           /* (P) or NULL */
    char* workspace;
    size_t workspace_bytes;
} moss_densify_select_args;
size_t moss_densify_select_workspace_bytes(int P);
int moss_densify_select(const moss_densify_select_args* args, void* stream);   /* scene/gaussian_model.py:499-509, :540-549, :579-602, :650-662 */

typedef struct moss_densify_emit_args {
    int32_t mode;                            /* MOSS_DENSIFY_CLONE / _SPLIT / _MERGE */
    int32_t P, n_sel, n_new;
    int32_t rest_floats;                     /* floats of a features_rest row (45) */
    int32_t dc_stride, rest_stride;          /* floats between rows of features_dc / features_rest */
    const int32_t* index;                    /* (n_sel) */
    const long long* ids;                    /* (P,2); MERGE */
    const float* xyz; const float* features_dc; const float* features_rest; const float* opacity; const float* scaling;
    const float* rotation;
    const float* lbs_weights;                /* (P,24) accumulated sum; CLONE */
    const float* denom;                      /* denom[0] is read; CLONE */
    const float* table;                      /* (24,12); CLONE */
    const float* noise;                      /* (n_new,3); CLONE / SPLIT */
    float* new_xyz; float* new_features_dc; float* new_features_rest; float* new_opacity; float* new_scaling; float* new_rotation;
    uint8_t* prune_mask;                     /* (P); MERGE */
} moss_densify_emit_args;
int moss_densify_emit(const moss_densify_emit_args* args, void* stream);       /* scene/gaussian_model.py:511-524, :551-566, :606-616 */

/*
 * Carrying a densification decision OUT: the row changes of one event as ONE gather pass over the flat optimizer buffers, additive in
 * ABI 7.  MOSS rebuilds every parameter tensor and both AdamW moments of each, one torch indexing / cat call at a time, in
 * _prune_optimizer (scene/gaussian_model.py:377-394), prune_points (:396-411), cat_tensors_to_optimizer (:413-434) and
 * densification_postfix (:436-454).  Here a ROW MAP says where each row of the new set comes from and one launch moves everything.
 * Both entry points enqueue on `stream`, allocate nothing and read nothing back on the host; a refused call launches nothing.
 *
 * moss_rows_keep_map (the `[mask]` of :384-388 and the `torch.cat` of :422-426 as an index list): map_out receives the ASCENDING
 *   indices i < rows_old with remove_mask[i] == 0 (bytes; a NULL mask keeps every row), then rows_old, rows_old + 1, ...,
 *   rows_old + rows_app - 1; *count_out (one DEVICE int32) is the map's length.  map_out holds rows_old + rows_app entries; those
 *   beyond the count stay untouched.  Stable compaction in two launches with no order-dependent atomic, as moss_densify_select's:
 *   per-workgroup totals (wave ballots, an LDS sum), then every workgroup sums the totals before it and ranks its rows with a
 *   ballot.  workspace: moss_rows_map_workspace_bytes(rows_old) bytes.  Bad arguments: MOSS_ERR_INVALID_ARG.
 *
 * moss_rows_relayout: for every tensor descriptor t and destination row r < rows_new, s = map[r]:
 *     s <  rows_old:  dst[r] = src[s], dst_m[r] = src_m[s], dst_v[r] = src_v[s]                       (:384-388: the kept rows)
 *     s >= rows_old:  dst[r] = app[s - rows_old], dst_m[r] = dst_v[r] = 0     (:422-423: torch.zeros_like(extension_tensor))
 *   and the `pad_after` floats behind the tensor's last row are written as ZEROS in dst, dst_m and dst_v (the flat layout promises
 *   zeros in its alignment gaps), so the destinations may be uninitialised memory.  A descriptor with use_map == 0 is not per-row:
 *   its `width` floats (and moments) are copied as they are.  src_m / src_v / dst_m / dst_v may be NULL TOGETHER: a tensor without
 *   optimizer state (:408-411, the statistics).  A map entry outside [0, rows_old + rows_app) writes a row of zeros and reads nothing.
 *   ONE launch for all tensors: the lanes run along the destination's flat elements (a wave stores 256 contiguous bytes), the
 *   source row of element e is map[e / width].
 *   Refused, with the offending field named in moss_last_error(): a NULL block or a NULL required pointer, a negative size, width
 *   < 1, pad_after outside 0..3, a destination range that overlaps a source range, the map or another destination
 *   (MOSS_ERR_INVALID_ARG); num_tensors > MOSS_ROWS_MAX_TENSORS, rows * width >= 2^31 (MOSS_ERR_UNSUPPORTED).
 */
#define MOSS_ROWS_MAX_TENSORS 12
typedef struct moss_rows_tensor {
    const float* src;                        /* (rows_old, width); (width) with use_map == 0 */
    const float* src_m; const float* src_v;  /* its two moments, or both NULL */
    const float* app;                        /* (rows_app, width); NULL when rows_app == 0 or use_map == 0 */
    float* dst;                              /* (rows_new, width) + pad_after floats */
    float* dst_m; float* dst_v;              /* NULL exactly when src_m / src_v are */
    int32_t width;                           /* floats per row */
    int32_t pad_after;                       /* 0..3 floats of alignment gap behind the tensor */
    int32_t use_map;                         /* 0: not per-row */
    int32_t reserved;
} moss_rows_tensor;
typedef struct moss_rows_relayout_args {
    int32_t rows_old, rows_app, rows_new;
    int32_t num_tensors;                     /* <= MOSS_ROWS_MAX_TENSORS */
    const int32_t* map;                      /* (rows_new), entries in [0, rows_old + rows_app) */
    moss_rows_tensor tensors[MOSS_ROWS_MAX_TENSORS];
} moss_rows_relayout_args;
size_t moss_rows_map_workspace_bytes(int rows_old);
int moss_rows_keep_map(int rows_old, const uint8_t* remove_mask, int rows_app, int* map_out, int* count_out, char* workspace,
                       size_t workspace_bytes, void* stream);                  /* scene/gaussian_model.py:384-388, :396-411, :422-426 */
int moss_rows_relayout(const moss_rows_relayout_args* args, void* stream);     /* scene/gaussian_model.py:377-394, :396-411, :413-434, :436-454 */

/*
 * The rasterizer with every extension (ABI 7): one argument block per direction.  The fields are those of moss_raster_forward /
 * moss_raster_backward plus the extensions below; NULL or 0 in an extension field means "not used".  moss_raster_forward /
 * moss_raster_backward fill these blocks with no extension and `capacity` = -1.
 *
 * capacity (forward): < 0 synchronous (one host read-back sizes the binning buffer, like moss_raster_forward); > 0 asynchronous with that
 *   capacity (above; `frame_state` is used with either).  0 is refused (MOSS_ERR_INVALID_ARG).  MOSS_DEBUG_SYNC only with capacity < 0.
 *   The backward's R is what the forward returned.
 *
 * transforms: covariance with a per-Gaussian 3x3 transform INSIDE the op.  MOSS feeds cov3D_precomp =
 *   strip_symmetric(T (R S S^T R^T) T^T) built by torch ops (scene/gaussian_model.py:37-44,168-169; gaussian_renderer/__init__.py:88-91)
 *   because the LBS transform T of each Gaussian changes every frame; on MI355X that Python path costs more than the whole rasterizer.
 *   transforms (P,3,3) row-major, with scales and rotations, no cov3D_precomp; the backward also needs dL_dtransforms.
 *   dL_dcov3D (P,6): gradient w.r.t. the transformed covariance (what the op stores); dL_dscale / dL_drot include the transform;
 *   dL_dtransforms (P,9): written for every Gaussian (zeros for culled ones).
 *
 * raw_flags (caller side of the boundary): the GaussianModel getters applied INSIDE the op.  MOSS hands the rasterizer
 *   get_opacity = sigmoid(_opacity), get_scaling = exp(_scaling), get_rotation = normalize(_rotation) (scene/gaussian_model.py:142-161,
 *   gaussian_renderer/__init__.py:77-93): five torch ops forward and a dozen backward per step.  With raw_flags the op takes the RAW
 *   parameters for the inputs named there and returns the gradients w.r.t. the raw parameters; it needs scales and rotations, no
 *   cov3D_precomp.
 *   MOSS_RAW_OPACITY (opacities are logits) | MOSS_RAW_SCALE (scales are logarithms) | MOSS_RAW_ROTATION (rotations are not normalised;
 *   normalised as x / max(|x|, 1e-12) like torch.nn.functional.normalize).
 *   The backward needs the raw `opacities` again (the reference backward does not take opacities at all).
 *   MOSS_HINT_SPATIAL_ORDER may be OR-ed in: "neighbours in index are neighbours in space" (the caller re-indexed its Gaussians along
 *   a space-filling curve, e.g. moss_amd.densify.spatial_order).  It changes no result beyond the order of some float32 sums, only how
 *   the per-Gaussian backward deals Gaussians to its workgroups (groups of 16 from places spread over the index range, so that no
 *   workgroup is all-heavy).
 *   MOSS_RAW_POSE (needs `transforms`): means3D are the CANONICAL positions x and the op poses them itself, p = T x (+ translation
 *   (P,3), may be NULL), rows of T times x summed left to right -- what MOSS's caller does with torch ops before the call
 *   (gaussian_renderer/__init__.py:74-77: torch.matmul(transforms, means3D[..., None]).squeeze(-1) + translation).  dL_dmean3D is
 *   then the gradient w.r.t. x (= T^T dL/dp: it can be written straight into the position parameter's gradient), dL_dtransforms
 *   gains dL/dp x^T, and dL_dtranslation (P,3; may be NULL) = dL/dp.  translation and dL_dtranslation only with MOSS_RAW_POSE.
 *   MOSS_SH_GRAD_ACTIVE_ONLY (ABI 6; backward only): dL_dsh is written for the coefficients of the ACTIVE degree only, (D+1)^2 of
 *   M per Gaussian; the rest of the destination is left untouched.  For a caller whose destination already holds zeros there and whose
 *   consumers never read them -- a gradient sink into a zero-initialised bucket consumed by the degree-aware flat AdamW
 *   (moss_adamw_flat_ex) and the active-degree exchange.  Without the bit every element is written (zeros above the degree), as ever.
 *
 * opt (backward; SURVEY section 8f row n4, ABI 4): the raw-parameter backward that also TAKES THE OPTIMIZER STEP.  The Gaussian parameters
 *   of MOSS receive their gradients from this op alone (every loss term of train_ZJU.py:111-131 goes through the rendered image; the
 *   exception is the position, which also feeds the LBS-weight network), and torch.optim.AdamW then streams parameter, gradient and
 *   both moments through the device once more (scene/gaussian_model.py:215-226, train_ZJU.py:204-205).  Here the per-Gaussian backward
 *   kernel, which holds a Gaussian's gradients in registers / LDS when it finishes, applies the AdamW update of the tensors named in
 *   opt->tensors itself: the parameters (= the op's inputs: writable memory, although the fields are const for the calls without `opt`)
 *   are updated in place, the moments in opt->exp_avg / exp_avg_sq, and the gradient of an updated tensor need not be written at all
 *   (its dL_d* pointer may be NULL).
 *   Same arithmetic, bit for bit, as moss_adamw_flat_ex with a step_state on the same values (both use csrc/adamw.h); a frame that
 *   overflowed its capacity (asynchronous forward) takes no step, like moss_adamw_flat_ex guarded by the frame's status word.
 *   Requirements: raw_flags contains MOSS_RAW_OPACITY | MOSS_RAW_SCALE | MOSS_RAW_ROTATION (the inputs must be the parameters
 *   themselves, not activated copies); MOSS_OPT_SH needs M == 16 and 16-byte aligned shs / moments; MOSS_OPT_MEANS only if the
 *   means the op sees are the parameter (no transforms, or MOSS_RAW_POSE) and nothing else contributes to its gradient.
 *   opt->step_state: moss_adamw_state_bytes() zeroed device bytes owned by this optimizer (not shared with a moss_adamw_flat_ex call
 *   of the same step: each launch that is given the block advances the count).
 *   opt == NULL or opt->tensors == 0: no update.
 */
#define MOSS_RAW_OPACITY 1
#define MOSS_RAW_SCALE 2
#define MOSS_RAW_ROTATION 4
#define MOSS_HINT_SPATIAL_ORDER 8
#define MOSS_RAW_POSE 16
#define MOSS_SH_GRAD_ACTIVE_ONLY 32
#define MOSS_OPT_MEANS 1
#define MOSS_OPT_SH 2
#define MOSS_OPT_OPACITY 4
#define MOSS_OPT_SCALES 8
#define MOSS_OPT_ROTATIONS 16
typedef struct moss_fused_adamw {
    uint32_t tensors;            /* MOSS_OPT_* bits: which parameters this call updates */
    float* exp_avg[5];           /* first moments, same shapes as the parameters; order: means, sh, opacity, scales, rotations */
    float* exp_avg_sq[5];        /* second moments */
    float lr[5];                 /* learning rates, same order; sh: of a Gaussian's first 3 floats (MOSS's features_dc group) */
    float lr_sh_rest;            /* sh: of the other 45 floats of a record (features_rest) */
    double beta1, beta2;         /* doubles (ABI 4): the kernels use float(beta) and float(1 - beta), rounded independently like torch's */
    float eps, weight_decay;
    void* step_state;
    int32_t lr_segment[5];       /* per tensor: its entry s (0..7) in the step-state block's learning-rate table, or -1; when word
                                  * MOSS_ADAMW_LR_VALID_WORD of step_state is non-zero the kernel reads lr from float word
                                  * MOSS_ADAMW_LR_WORD0 + s (sh: lr_sh_rest from MOSS_ADAMW_LR2_WORD0 + s) instead of from this struct */
    int32_t sh_active_degree;    /* ABI 6.  The HIGHEST SH degree that has ever been active for these parameters (0..3; the call's own
                                  * D is the floor; 3 = everything is active, the behaviour before ABI 6).  Coefficients above it have
                                  * never received a gradient: their moments are exactly zero and are neither read nor written, and
                                  * their parameters take the weight decay alone -- bit for bit the full update's result.  MOSS: degree
                                  * 0 / 1 / 2 for iterations 1-2999 (train_ZJU.py:85-86). */
    int32_t sh_inactive_zero;    /* != 0: the caller also knows those parameters to be exactly ZERO (features_rest starts as zeros,
                                  * scene/gaussian_model.py:179-181; 0 x decay = 0): they are not read or written at all */
} moss_fused_adamw;

typedef struct moss_raster_forward_args {
    moss_alloc_fn geometry_alloc; void* geometry_user;
    moss_alloc_fn binning_alloc; void* binning_user;
    moss_alloc_fn image_alloc; void* image_user;
    int P, D, M;
    const float* background; int width, height;
    const float* means3D; const float* shs; const float* colors_precomp; const float* opacities;
    const float* scales; float scale_modifier; const float* rotations; const float* cov3D_precomp;
    const float* viewmatrix; const float* projmatrix; const float* cam_pos;
    float tan_fovx, tan_fovy; int prefiltered;
    float* out_color; float* out_depth; float* out_alpha; int* radii;
    int debug;
    /* extensions */
    const float* transforms; const float* translation; int raw_flags;
    int capacity; char* frame_state;
} moss_raster_forward_args;
/* Returns num_rendered (capacity < 0) or `capacity` (> 0), or a negative error code. */
int moss_raster_forward_ex(const moss_raster_forward_args* args, void* stream);

typedef struct moss_raster_backward_args {
    int P, D, M, R;
    const float* background; int width, height;
    const float* means3D; const float* shs; const float* colors_precomp;
    const float* scales; float scale_modifier; const float* rotations; const float* cov3D_precomp;
    const float* viewmatrix; const float* projmatrix; const float* campos;
    float tan_fovx, tan_fovy;
    char* geom_buffer; char* binning_buffer; char* image_buffer;
    const float* dL_dpix; const float* dL_ddepths; const float* dL_dalphas;
    float* dL_dmean2D; float* dL_dconic; float* dL_dopacity; float* dL_dcolor; float* dL_dmean3D;
    float* dL_dcov3D; float* dL_dsh; float* dL_dscale; float* dL_drot;
    int debug;
    /* extensions */
    const float* transforms; const float* translation; const float* opacities;
    float* dL_dtransforms; float* dL_dtranslation;
    int raw_flags;
    const moss_fused_adamw* opt;
} moss_raster_backward_args;
/* Returns 0 or a negative error code. */
int moss_raster_backward_ex(const moss_raster_backward_args* args, void* stream);

/*
 * Gaussian parameter activations, forward and backward, one launch each (the rasterizer-facing getters of MOSS's GaussianModel,
 * scene/gaussian_model.py:46-53 and :134-166: get_xyz identity, get_features = cat(_features_dc, _features_rest, dim=1),
 * get_opacity = sigmoid, get_scaling = exp, get_rotation = F.normalize (eps 1e-12)).  K = SH coefficients per channel
 * ((max_sh_degree+1)^2); features_dc is (P,1,3), features_rest (P,K-1,3), out_features (P,K,3); all fp32, contiguous.
 * K = 0: the features are not touched (callers that keep them as one (P,K,3) tensor need no concatenation).
 * Backward: a NULL incoming gradient means that output was unused (its parameter gets zeros); every element of every d_*
 * array is written exactly once, so destinations (e.g. slices of a flat gradient bucket) need no zero fill.
 */
int moss_gaussian_activate_forward(int P, int K, const float* xyz, const float* features_dc, const float* features_rest,
                                   const float* opacity, const float* scaling, const float* rotation,
                                   float* out_xyz, float* out_features, float* out_opacity, float* out_scaling,
                                   float* out_rotation, void* stream);
int moss_gaussian_activate_backward(int P, int K, const float* rotation, const float* out_opacity, const float* out_scaling,
                                    const float* g_xyz, const float* g_features, const float* g_opacity,
                                    const float* g_scaling, const float* g_rotation,
                                    float* d_xyz, float* d_features_dc, float* d_features_rest, float* d_opacity,
                                    float* d_scaling, float* d_rotation, void* stream);

/* ---- inspection entry points (used by the parity tests; not needed by a caller of the op) ---------------- */

/* Scratch sizes this library will request for a given problem (host-only arithmetic, no GPU touched). */
size_t moss_raster_geometry_bytes(int P);
size_t moss_raster_image_bytes(int width, int height);
size_t moss_raster_binning_bytes(int R);
size_t moss_raster_binning_bytes_forward_only(int R);   /* the binning buffer of a MOSS_FORWARD_ONLY forward (ABI 6) */

/*
 * Re-express the opaque geometry buffer in the reference's GeometryState terms
 * (DGR/cuda_rasterizer/rasterizer_impl.cu:155-170); any output pointer may be NULL.
 *   depths (P), means2D (P,2), conic_opacity (P,4), rgb (P,3), tiles_touched (P) u32, clamped (P,3) bytes,
 *   cov3D (P,6; only meaningful when forward computed it from scales/rotations).
 * Entries of culled Gaussians read as zero.
 */
int moss_raster_export_geometry(const char* geom_buffer, int P,
    float* depths, float* means2D, float* conic_opacity, float* rgb, uint32_t* tiles_touched,
    uint8_t* clamped, float* cov3D, void* stream);

/*
 * Re-express the opaque binning + image buffers in the reference's BinningState / ImageState terms
 * (rasterizer_impl.cu:172-194): the SORTED 64-bit keys (tile << 32 | depth bits), the sorted Gaussian ids,
 * the per-tile ranges (tiles,2) u32, and per pixel final_T / n_contrib.  Any output pointer may be NULL.
 */
int moss_raster_export_binning(const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
    int P, int R, int width, int height,
    uint64_t* point_list_keys, uint32_t* point_list, uint32_t* ranges, float* final_T, uint32_t* n_contrib,
    void* stream);

/*
 * Per-stage device timing, measured with HIP events recorded on the stream each stage is launched on (so it sees exactly
 * what a profiler's kernel trace sees, minus nothing).  Enable a set of stages (bit i = stage i), run, then read:
 * ms_sum[i] = summed duration of stage i over count[i] executions since the last read; reading synchronises those events.
 */
#define MOSS_STAGE_PREPROCESS_FWD 0
#define MOSS_STAGE_SCAN           1
#define MOSS_STAGE_SCATTER        2
#define MOSS_STAGE_TILE_SORT      3   /* the chunk sort kernel */
#define MOSS_STAGE_BLEND_FWD      4
#define MOSS_STAGE_BLEND_BWD      5
#define MOSS_STAGE_PREPROCESS_BWD 6
#define MOSS_STAGE_MERGE_GATHER   7   /* the second kernel of the tile sort: rank merge + per-instance emit */
#define MOSS_NUM_STAGES           8
void moss_raster_profile_enable(uint32_t stage_mask);
int moss_raster_profile_read(float* ms_sum /* [MOSS_NUM_STAGES] */, uint32_t* count /* [MOSS_NUM_STAGES] */);

/* 1 if the library was built with -DMOSS_DIAG (python -m moss_amd.build --diag -> moss_amd/lib_diag/): it then reads MOSS_*
 * environment knobs that select kernel variants for A/B timing -- some give WRONG results on purpose -- and exports the stamp
 * entry points below.  The product build returns 0, reads no environment variable and does not export them. */
int moss_build_has_diagnostics(void);
#ifdef MOSS_DIAG
/* register a device buffer of 8 x (4 * padded tile count) uint64; while set, the forward blend kernel stores per item
 * {total, list length, starve, first trip, begin, trip cycles, rounds, trips} of its blender wave.  NULL = off. */
void moss_raster_debug_set_stamps(unsigned long long* device_buffer);
/* the same for the backward blend kernel: 16 words per wave (start, end of the segment phase, end, item counts and cycle sums) */
void moss_raster_debug_set_bwd_stamps(unsigned long long* device_buffer);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MOSS_RASTER_H */
