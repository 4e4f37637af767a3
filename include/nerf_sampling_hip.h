/*
 * nerf_sampling_hip.h -- C ABI of libnerf_sampling_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of MarcinKadziolka/nerf-sampling: the ray-batch render
 * operator (ray generation, ray-sphere intersection, positional encoding, DepthNet and
 * radiance-field MLP forward, alpha compositing).  The reference has no native code, so
 * each entry point below names the reference *Python* function (file:line relative to the
 * reference tree) whose arithmetic it replaces; a ctypes binding for every one of them is in
 * nerf_sampling_amd/_lib.py and the reference-side stub is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer, fp32 unless stated; caller-owned
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     asynchronous on it and re-entrant across streams (weight handles are read-only after packing and
 *     own no per-call scratch; per-call intermediates live in the caller's workspace)
 *   - return value: 0 = ok, negative = NS_E_* below (nothing was launched), never throws
 *   - no torch types, no global state except lazily-queried device properties
 */
#ifndef NERF_SAMPLING_HIP_H
#define NERF_SAMPLING_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS_OK 0
#define NS_E_INVALID (-1)     /* bad argument (null pointer, non-positive size, ...)   */
#define NS_E_UNSUPPORTED (-2) /* network shape outside what the kernels are built for  */
#define NS_E_HIP (-3)         /* a HIP runtime call failed; see ns_last_error()        */
#define NS_E_NOMEM (-4)

/* operand precision of the MFMA kernels (accumulation is always fp32) */
#define NS_DTYPE_F32 0  /* v_mfma_f32_32x32x2_f32, exact-fp32 parity path (k-major engine)             */
#define NS_DTYPE_BF16 1 /* v_mfma_f32_16x16x32_bf16, both networks (output-sub-block-major engine)      */
#define NS_DTYPE_F16 2  /* v_mfma_f32_16x16x32_f16, same engine                                         */
#define NS_DTYPE_F16X3 3 /* split fp16 operands (x = hi + lo), three v_mfma_f32_16x16x32_f16 per product term: fp32-grade
                          * results (the fp32 parity gates hold) at ~1/3 of the fp16 rate; operands must fit fp16's
                          * range (|w| < 65504, checked at pack time)                                    */
#define NS_DTYPE_F16M 4  /* DepthNet only, the production 10 x 256 trunk: MIXED fp16 operands -- the first
                          * NS_F16M_SPLIT_LAYERS trunk layers split as in F16X3 (that is where an fp16 DepthNet loses its depth:
                          * 90 % of the error's variance), the rest plain F16; 1.6 x the fp16 kernel's MFMAs instead of 3 x */
#define NS_F16M_SPLIT_LAYERS 3

/* sample placement modes, utils.py:220-244 */
#define NS_MODE_DEPTH_ONLY 0
#define NS_MODE_UNIFORM 1
#define NS_MODE_GAUSSIAN 2

const char* ns_last_error(void);
int ns_version(void);
/* number of compute units of the current device (0 if no device) */
int ns_device_cu_count(void);
/* Diagnostic switches of the kernel dispatch (tests compare code paths inside one process; no effect on results):
 *   "generic_kernels" 0/1 -- 1: the production network (8 x 256, skips = [4]) runs the generic compiler-scheduled kernels
 *                            instead of the generated instruction streams;
 *   "prod_tiles" 0/4/5    -- tiles per wave of the 16-bit production kernel, 0 = chosen per launch;
 *   "hier_chain" 0/1      -- 1: ns_render_rays_hierarchical keeps raw [R,N,4] in HBM and composites with ns_raw2outputs instead
 *                            of in the MLP kernels' epilogues;
 *   "no_colour_skip" 0/1  -- 1: launches the render kernel would take (a 16-bit production field composited in the kernel,
 *                            N a power of two <= 64, no raw / max-weight / guard outputs; five tiles) run the production kernel;
 *   "count_colour_skips" 0/1 -- 1: every render-kernel launch counts the waves that skipped their colour statements and the
 *                            chunk steps whose MFMAs the K-block-skipping kernel jumped over;
 *   "kblock_skip" 0/1     -- 1: launches the render kernel takes run its K-block-skipping twin instead (same results bit for
 *                            bit; off by default: it measured no faster than the render kernel);
 *   "kblock_suffix" 0/1/2 -- launches the render kernel takes run its dead-suffix twin instead (same results bit for bit): 0
 *                            never, 1 on every handle with finite weights, 2 (the initial value) only on handles marked by
 *                            ns_weights_set_unit_ordered; -1 restores the initial value; "kblock_skip" = 1 wins over it;
 *   "mesh_raster_big_box" n >= 0 -- ns_mesh_raster's faces whose clamped bounding box has more than n pixels take its workgroup
 *                            launch; 0 = NS_MESH_RASTER_BIG_BOX.
 * Initial values come from the environment (NS_OB16_GENERIC, NS_OB16_TILES, NS_KBLOCK_SKIP, NS_KBLOCK_SUFFIX), read once at first use. */
int ns_debug_set(const char* name, int value);
/* Waves that skipped the colour layers in the LAST bf16 / f16 radiance-field launch on the current device that ran with
 * "count_colour_skips" set: 0 when that launch ran another kernel than the render kernel, and before any such launch.
 * Waits for the device.                                                                                            */
int ns_colour_skip_count(int64_t* waves_out);
/* Chunk steps (five MFMAs each) whose input K-block was all zero bits and whose MFMAs were jumped over, summed over the waves of
 * the LAST such launch with "count_colour_skips" set: 0 when it did not run the K-block-skipping render kernel.  Waits for the
 * device.                                                                                                          */
int ns_kblock_skip_count(int64_t* steps_out);
/* The same for the dead-suffix render kernel: chunk steps absent from the bodies its waves ran, i.e. sub-blocks x trailing dead
 * K-blocks per statement; 0 when the launch did not run that kernel.  Waits for the device.                           */
int ns_kblock_suffix_count(int64_t* steps_out);

/* ---- a1  get_rays + prepare_rays  (run_nerf_helpers.py:187-202, nerf_utils.py:156-188) ----
 * Pixel rows [row0,row1) of an HxW pinhole camera, row-major.  c2w is 12 HOST floats (3x4,
 * row-major).  Any output pointer may be NULL.  ray_batch is [R,11] =
 * [o(3) d(3) near far viewdir(3)], viewdir = d/|d|; R = (row1-row0)*W.                      */
int ns_get_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host,
                int row0, int row1, float near_, float far_, float* rays_o_dev, float* rays_d_dev,
                float* viewdirs_dev, float* ray_batch_dev, void* stream);

/* ---- training ray batches from a device-resident dataset  (Trainer.sample_random_ray_batch, Trainer.py:400-475) ----
 * "B training rays and their target colours" with images and poses uploaded once.  images_dev is fp32 [n_images, H, W, C],
 * C = 3 or 4; poses_dev holds pose_stride = 12 or 16 floats per image, the first 12 being c2w[:3,:4] row-major.  The target of
 * a ray is its pixel's rgb; with C == 4 and white_bkgd it is rgb * a + (1 - a) in separate fp32 roundings (Blender.py:26-29).
 * rays_o / rays_d / viewdirs are the bits a1 writes at that pixel.  n_images * H * W must stay below 2^31.                 */
typedef struct ns_ray_dataset {
  const float* images_dev;
  const float* poses_dev;
  int n_images, H, W, C;
  int pose_stride, white_bkgd;
  float fx, fy, cx, cy;
} ns_ray_dataset;
/* Ray i of the batch is pixel pixel_dev[i] (int32, flat row * W + col) of image image_idx_dev[i] (int32), or of image
 * `image_idx` for every ray when image_idx_dev is NULL.  Outputs are [B,3]; any of them may be NULL.  Indices read from
 * device memory are clamped into range by the kernel; the host scalar is checked here.                                     */
int ns_ray_batch_gather(const ns_ray_dataset* ds, const int* image_idx_dev, int image_idx, const int* pixel_dev, int64_t B,
                        float* rays_o_dev, float* rays_d_dev, float* viewdirs_dev, float* target_dev, void* stream);
/* The same with the indices drawn in the launch, without replacement, by a keyed permutation P_{seed,counter} of [0, n): a
 * balanced Feistel network of NS_RAY_DRAW_ROUNDS rounds over the smallest even bit width covering n, cycle-walked into
 * [0, n) -- O(1) per ray, no memory (DESIGN.md section 8 states the constants).  This is NOT numpy's generator.
 *   NS_RAY_SCOPE_PER_IMAGE  (no_batching): every ray from image train_idx[h(seed, step) mod n_train]; ray i is pixel
 *       P_{seed,step}(i) of the window rows [row0,row1) x columns [col0,col1), as a full-frame flat index; B <= window size.
 *   NS_RAY_SCOPE_ALL_IMAGES (use_batching): pos = step * B + i, N = n_train * H * W, g = P_{seed, pos div N}(pos mod N):
 *       image train_idx[g div (H * W)], pixel g mod (H * W); every epoch of N rays visits each ray once.  The window is unused.
 * {step, row0, row1, col0, col1} is read from params_dev (five int32 in device memory: nothing in the launch changes from
 * step to step, so a captured hipGraph replays it, ns_add_i32 advancing the step) or from *params_host -- exactly one of
 * the two is given.  Host params are checked here (NS_E_INVALID: empty window, window outside the frame, B above the
 * window size); device params cannot be, so the kernel clamps the window to a non-empty part of the frame and wraps ray
 * indices beyond it.  train_idx_dev: int32 [n_train], clamped into [0, n_images).  image_idx_out_dev / pixel_out_dev:
 * int32 [B] or NULL, the indices drawn.                                                                                   */
#define NS_RAY_SCOPE_PER_IMAGE 0
#define NS_RAY_SCOPE_ALL_IMAGES 1
#define NS_RAY_DRAW_ROUNDS 6
typedef struct ns_ray_draw_params {
  int step, row0, row1, col0, col1;
} ns_ray_draw_params;
int ns_ray_batch_draw(const ns_ray_dataset* ds, const int* train_idx_dev, int n_train, int scope, const int* params_dev,
                      const ns_ray_draw_params* params_host, uint64_t seed, int64_t B, int* image_idx_out_dev,
                      int* pixel_out_dev, float* rays_o_dev, float* rays_d_dev, float* viewdirs_dev, float* target_dev,
                      void* stream);

/* ---- frame PSNR against a dataset image  (nerf_utils.py:303-336 render_path's per-frame PSNR, Trainer.py:289-316 the test-set
 * log) ----  *sum_dev = sum over the pixels of rows [row0,row1) of image image_idx and the three colour channels of
 * (double)(fl32(rgb - target))^2: ONE fp32 subtraction (numpy's rgbs - gt on fp32 arrays), squared and accumulated in double.
 * target is the ray-batch kernels' target, bit for bit (the white-background blend included).  Ray r = (row - row0) * W + col
 * reads rgb_dev[r * rgb_stride + c]; rgb_stride is in floats, 0 = packed 3, 4 = the interleaved [R,4] shard
 * parallel.FrameRenderer all-gathers.  sum_dev is one double in device memory (a slot of a longer array: a test split is read
 * back once); PSNR = -10 log10(sum / (3 * pixels)) is the host's.  Deterministic: the partition of pixels over threads and
 * the order of every addition depend on (row1 - row0) * W alone -- per-thread doubles, a wave tree, per-workgroup partials
 * in workspace_dev (ns_image_sqerr_workspace_bytes(pixels) bytes) and a second launch that adds them in index order; no
 * atomics.  A NaN pixel makes the sum NaN, as numpy's mean does.  Checked before any launch (NS_E_INVALID): image_idx
 * outside [0, n_images), an empty row band or one outside the frame, images_dev / rgb_dev / sum_dev / workspace_dev NULL,
 * a stride other than 0, 3 or 4.                                                                                          */
int64_t ns_image_sqerr_workspace_bytes(int64_t n_pixels);
int ns_image_sqerr(const ns_ray_dataset* ds, int image_idx, int row0, int row1, const float* rgb_dev, int64_t rgb_stride,
                   double* sum_dev, void* workspace_dev, void* stream);

/* ---- frame SSIM against a dataset image  (not in the reference, which reports a PSNR only) ----  Wang et al. 2004 as
 * tf.image.ssim and skimage's structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
 * data_range=1) compute it: per colour channel, over every 11 x 11 window that lies wholly inside the frame --
 * (H - 10)(W - 10) of them -- with weights w(i,j) = g(i) g(j), g(k) = exp(-(k - 5)^2 / 4.5) / sum; mu_x, mu_y, E[x^2], E[y^2],
 * E[xy] the w-weighted sums, var_x = E[x^2] - mu_x^2, var_y likewise, cov = E[xy] - mu_x mu_y, C1 = 1e-4, C2 = 9e-4,
 *   S = (2 mu_x mu_y + C1)(2 cov + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x + var_y + C2)).
 * *sum_dev = the sum of S over all windows and the three channels; the mean, sum / (3 (H - 10)(W - 10)), is the host's.
 * x is rgb_dev[r * rgb_stride + c] of the WHOLE frame (ray r = row * W + col; rgb_stride as ns_image_sqerr's: 0 = packed 3,
 * 4 = the interleaved [R,4] shard), y the ray-batch kernels' target of image image_idx, bit for bit (the white-background
 * blend included).  Everything after the fp32 loads is double -- the five moments (the taps are 17-digit literals), S and
 * the sum: in fp32 the cancellation E[x^2] - mu^2 on a flat background leaves rounding noise of 1e-7 against C2.
 * Deterministic: workgroups own NS_SSIM_TILE_H x NS_SSIM_TILE_W tiles of window origins in row-major order, one thread per
 * window; the order of every addition depends on (H, W) alone -- row sums with the taps in index order, then the rows in
 * order, the channels in order, a wave tree, per-workgroup partials in workspace_dev (ns_image_ssim_workspace_bytes(H, W)
 * bytes) and ns_image_sqerr's second launch adding them in index order; no atomics.  A window outside the valid range is
 * predicated out.  A NaN pixel makes the sum NaN.  Checked before any launch (NS_E_INVALID): H < 11 or W < 11, image_idx
 * outside [0, n_images), images_dev / rgb_dev / sum_dev / workspace_dev NULL, a stride other than 0, 3 or 4.
 * ns_image_ssim_tile writes the two tile extents (either pointer may be NULL).                                             */
#define NS_SSIM_WINDOW 11
#define NS_SSIM_TILE_H 16
#define NS_SSIM_TILE_W 16
void ns_image_ssim_tile(int* tile_h, int* tile_w);
int64_t ns_image_ssim_workspace_bytes(int H, int W);
int ns_image_ssim(const ns_ray_dataset* ds, int image_idx, const float* rgb_dev, int64_t rgb_stride, double* sum_dev,
                  void* workspace_dev, void* stream);

/* ---- placed samples against the field's depth  (nerf_utils.py:311-317 render_path's "MSE:" under compare_nerf,
 * mse_loss(max_z_vals, depth_net_z_vals); Trainer.py:537 depth_net_loss = mse(depth_net_z_vals, max_z_vals)) ----
 * *sum_dev = sum over rays r in [0, R) and samples k in [0, N) of (double)(fl32(z_dev[r * z_row_stride + k] - ref_dev[r]))^2:
 * ONE fp32 subtraction (torch's mse_loss on fp32 tensors), its square exact in double, the sum kept in double; the mean,
 * sum / (R * N), is the host's.  ref_dev is [R] packed (a contiguous [R,1] has the same layout); z_row_stride is in floats,
 * 0 = packed N, otherwise >= N (a column slice of a wider buffer); N = 1 scores a vector [R].  sum_dev is one double in
 * device memory (a slot of a longer array).  Deterministic as ns_image_sqerr: workgroup g owns the NS_DEPTH_SQERR_SHARE flat
 * elements e = r * N + k from g * NS_DEPTH_SQERR_SHARE on, a thread adds its elements in index order, then a wave tree,
 * per-workgroup partials in workspace_dev (ns_depth_sqerr_workspace_bytes(R, N) bytes) and ns_image_sqerr's second launch
 * adding them in index order -- the order of every addition depends on (R, N) alone; no atomics.  A NaN term (a ray that
 * misses the sphere has a NaN DepthNet depth) makes the sum NaN, as the reference's MSE is then.  Checked before any launch
 * (NS_E_INVALID): z_dev / ref_dev / sum_dev / workspace_dev NULL, R < 1, N < 1, a stride in [1, N), and R * N >= 2^31 -- the
 * flat element index and its division by N are 32-bit (800 x 800 x 64 is 4.1e7).  ns_depth_sqerr_workspace_bytes is 0 for a
 * shape that would be refused.                                                                                            */
#define NS_DEPTH_SQERR_SHARE 2048
int64_t ns_depth_sqerr_workspace_bytes(int64_t R, int N);
int ns_depth_sqerr(const float* z_dev, int64_t z_row_stride, const float* ref_dev, int64_t R, int N, double* sum_dev,
                   void* workspace_dev, void* stream);

/* ---- the scene's point cloud  (experiments/plot.py:13-22: all_pts[all_weights >= t] of the per-sample points and weights
 * render_path(save_scene_data=True) collects; utils.py:36-43 get_min_indices) ----  An ordered stream compaction.  The flat
 * element e = r * N + k, r in [0, R), k in [0, N), is KEPT iff w_dev[r * w_row_stride + k] >= min_weight: a NaN weight is
 * dropped, -0.0 >= 0.0 keeps.  A kept element's record index is i = *count_dev (its value before the call) + the number of
 * kept elements with a smaller e: records are ray-major, sample-minor and call after call, the order of
 * torch.cat(all_pts)[torch.cat(all_weights) >= t].  The record is written iff 0 <= i < capacity -- nothing is ever written at
 * or beyond capacity --
 *   pts_out[i] = o[r] + d[r] * z_dev[r * z_row_stride + k]   (multiply and add rounded separately: ns_points_along_rays' bits),
 *   w_out[i]   = the weight,
 *   rgb_out[i] = rgb_dev[r * rgb_stride + 0..2], the colour of the RAY, when rgb_out is given (rgb_dev is then required; rgb_dev
 *                alone is ignored),
 * and afterwards *count_dev has grown by the number of ALL kept elements, those that did not fit included: one 8-byte readback
 * at the very end tells the caller the capacity it would have needed.  *count_dev must not be negative.  o, d are [R,3] packed;
 * the strides are in floats, 0 = packed (N, N, 3), otherwise >= N, >= N, >= 3 (column slices of wider buffers, the interleaved
 * [R,4] shard).  R == 0 leaves everything untouched; capacity == 0 (the outputs may then be NULL) is a pure count.
 * Three launches on `stream`, no atomics: (1) workgroup g counts the kept elements among its NS_CLOUD_SHARE flat elements from
 * g * NS_CLOUD_SHARE on (thread t takes g * NS_CLOUD_SHARE + j * 256 + t) into workspace_dev (one int64 per share,
 * ns_cloud_workspace_bytes(R, N) bytes); (2) ONE workgroup reads *count_dev, turns the counts into absolute record indices in
 * the order of g and writes *count_dev + total back; (3) every workgroup evaluates the predicate again and places its kept
 * elements: the share's index + the kept elements of its earlier steps j and waves (LDS) + the kept lanes below (a 64-bit
 * ballot and a popcount).  No workgroup waits on another's memory, and the result depends on the inputs alone.  Checked before
 * any launch (NS_E_INVALID): R < 0, N < 1, R * N >= 2^31 (the flat index and its division by N are 32-bit), a negative stride
 * or one below the packed one, a negative capacity, capacity > 0 without pts_out / w_out, rgb_out without rgb_dev, count_dev
 * NULL, count_dev / workspace_dev not 8-byte aligned, and for R > 0 o / d / z / w / workspace_dev NULL.
 * ns_cloud_workspace_bytes is 0 for a shape that would be refused or has no work (R < 1).                                  */
#define NS_CLOUD_SHARE 2048
int64_t ns_cloud_workspace_bytes(int64_t R, int N);
int ns_cloud_append(const float* o_dev, const float* d_dev, const float* z_dev, int64_t z_row_stride, const float* w_dev,
                    int64_t w_row_stride, const float* rgb_dev, int64_t rgb_stride, int64_t R, int N, float min_weight,
                    float* pts_out, float* w_out, float* rgb_out, int64_t capacity, int64_t* count_dev, void* workspace_dev,
                    void* stream);

/* ---- the field's isosurface mesh  (the original NeRF code's extract_mesh notebook: marching cubes of a density lattice on the
 * host; not in the reference) ----  Marching TETRAHEDRA on the Kuhn split of every lattice cell: a 16-entry case table without
 * ambiguous cases, and a split that is translation-invariant and face-compatible, so the surface is a closed oriented manifold
 * wherever it stays off the lattice boundary.  An ordered stream compaction, the sibling of ns_cloud_append.
 * LATTICE: point (i, j, k), i in [0, Gx), j in [0, Gy), k in [0, Gz), has lattice index lin = (k * Gy + j) * Gx + i, value
 * sigma_dev[lin * sigma_stride] (the stride in floats; 0 or 1 = packed, 4 = the sigma column of a raw [., 4] array) and position
 * lo + (float)idx * h per axis, the multiply and the add rounded separately in fp32.
 * CELLS: cell (i, j, k), i < Gx - 1, j < Gy - 1, k < Gz - 1, has the flat index e = (k * (Gy - 1) + j) * (Gx - 1) + i and eight
 * corners, named by their code dx + 2 dy + 4 dz.  Its six tetrahedra t = 0 .. 5 belong to the permutations pi of the axes
 * (x, y, z) in lexicographic order -- xyz, xzy, yxz, yzx, zxy, zyx --: tetrahedron t has the corners w0 = 000, w1 = w0 + e_pi0,
 * w2 = w1 + e_pi1, w3 = 111.  A corner is INSIDE iff its value >= iso.  A cell with a corner that is NaN or +-inf emits nothing
 * and is counted as skipped.
 * TRIANGLES of a tetrahedron, by its inside corners (numbered 0 .. 3 as w0 .. w3): none or all four, no triangle; one (a) and
 * three outside (b0 < b1 < b2), the triangle (a b0, a b1, a b2) of the crossed edges; three (a0 < a1 < a2) and one outside (b),
 * the triangle (a0 b, a1 b, a2 b); two (a0 < a1) and two outside (b0 < b1), the quad (a0 b0, a0 b1, a1 b1, a1 b0) split as
 * (0, 1, 2) and (0, 2, 3).  WINDING: vertices 1 and 2 of a triangle are exchanged iff the normal (m1 - m0) x (m2 - m0) through
 * the MIDPOINTS m of its three lattice edges has a negative dot product with (mean of the tetrahedron's outside corners - mean of
 * its inside corners): a function of (t, inside corners) alone, a table (csrc/ns_mesh_table.h), never of the vertex positions --
 * a corner exactly at iso gives triangles of zero area, whose own normal says nothing.  The surface faces from inside to outside.
 * VERTEX on the lattice edge between points a and b, lin(a) < lin(b), with values s_a and s_b:
 *   tt = (iso - s_a) / (s_b - s_a)       one correctly rounded fp32 division,
 *   p  = p_a + tt * (p_b - p_a)          per axis, every operation rounded separately,
 *   key = lin(a) * 8 + (dx + 2 dy + 4 dz),  d = b - a in {0, 1}^3:
 * a function of the edge alone, so every triangle around an edge carries the same position bits under the same key.
 * ORDER: triangles are numbered by (e, t, triangle within the tetrahedron).  Triangle n is written iff n < capacity -- nothing is
 * ever written at or beyond capacity --: tri_out[n * 9 ..] its three vertices xyz, key_out[n * 3 ..] their keys.  capacity == 0
 * (the outputs may then be NULL) is a pure count.  count_dev[0] = the number of ALL triangles, those that did not fit included,
 * count_dev[1] = the number of skipped cells; both are overwritten, not accumulated.
 * Three launches on `stream`, no atomics: (1) workgroup g counts the triangles and the skipped cells among its NS_MESH_SHARE
 * cells from g * NS_MESH_SHARE on (thread t takes g * NS_MESH_SHARE + s * 256 + t) into workspace_dev (two int64 per share,
 * ns_mesh_workspace_bytes(Gx, Gy, Gz) bytes; what it holds before the call does not matter); (2) ONE workgroup turns the
 * triangle counts into absolute triangle indices in the order of g and writes the two totals; (3) every workgroup evaluates its
 * cells again and emits: the share's index + the triangles of its earlier steps s and waves (LDS) + those of the lanes below (a
 * cell has 0 .. 12 triangles: an integer exclusive scan over the wave).  The result depends on the inputs alone.  Values whose
 * differences overflow fp32 give NaN positions.  Checked before any launch (NS_E_INVALID): a dimension below 2,
 * Gx * Gy * Gz >= 2^31 (lattice and cell indices are 32-bit), a negative stride, a negative capacity, capacity > 0 without
 * tri_out / key_out, count_dev / sigma_dev / workspace_dev NULL, count_dev / key_out / workspace_dev not 8-byte aligned, a
 * non-finite iso, lo or h, and h <= 0.  ns_mesh_workspace_bytes is 0 for a shape that would be refused.                      */
#define NS_MESH_SHARE 1024
int64_t ns_mesh_workspace_bytes(int Gx, int Gy, int Gz);
int ns_mesh_extract(const float* sigma_dev, int64_t sigma_stride, int Gx, int Gy, int Gz, float iso, float lo_x, float lo_y,
                    float lo_z, float h_x, float h_y, float h_z, float* tri_out, int64_t* key_out, int64_t capacity,
                    int64_t* count_dev, void* workspace_dev, void* stream);

/* ---- the connected components of a mesh's faces  (what every NeRF mesh export does on the host to drop floaters, the small
 * closed blobs of stray density around the object; not in the reference) ----  A lock-free union-find over the vertices.
 * CONNECTIVITY: faces_dev[f * 3 .. f * 3 + 2], f in [0, F), are vertex indices, as ops.mesh_weld returns them.  Two vertices are
 * connected iff a chain of faces joins them; a face joins its three vertices, so two faces that share a single vertex lie in one
 * component.  A face with two or three equal indices is legal and joins whatever indices it has.  A face with any index outside
 * [0, V) joins nothing and is counted; none of its indices is ever used as an address.
 * OUTPUTS: label_dev[v], v in [0, V), is the smallest vertex index of v's component; a vertex in no face is a component of its
 * own.  At a root r == label_dev[r], tri_count_dev[r] is the number of valid faces of the component and vert_count_dev[r] the
 * number of its vertices; every other entry of the two is 0.  count_dev[0] = the number of components, count_dev[1] = the number
 * of ignored faces; both are overwritten, not accumulated.  Nothing is written outside [0, V) of the three arrays.
 * Four launches on `stream` (one where V == 0), with label_dev as the parent array: (1) parent[v] = v, the counts and the two
 * 32-bit counters in workspace_dev zeroed (ns_mesh_components_workspace_bytes(V, F) bytes; what it holds before the call does
 * not matter); (2) workgroup g takes the NS_MESH_COMPONENTS_SHARE faces from g * NS_MESH_COMPONENTS_SHARE on (thread t takes
 * g * NS_MESH_COMPONENTS_SHARE + s * 256 + t) and unites (a, b) and (a, c) of each: two walks towards the roots side by side,
 * halving their paths (atomicMin) and over as soon as they meet, else the larger root linked below the smaller by atomicCAS on
 * the root's own word; (3) label_dev[v] = the root of v, the vertices counted
 * per root and the roots counted; (4) the valid faces counted at the label of their first vertex, and the totals written.
 * A parent never exceeds its vertex and only ever decreases, so every walk visits strictly decreasing indices and ends; no
 * workgroup waits for memory another one writes, and a CAS is retried only because another thread's CAS succeeded.  Integer
 * atomics at agent scope (atomicMin, atomicCAS, atomicAdd on 32-bit words), unlike the sibling kernels -- they are what makes
 * the labelling parallel --, and no floating-point ones: the smallest index, the counts and the totals do not depend on the
 * order of the atomics, so the result depends on the inputs alone.  Not part of this: per-component area or volume (floating-
 * point sums whose order is not fixed), and meshes of 2^31 vertices or faces or more.
 * Checked before any launch (NS_E_INVALID): negative F or V, V >= 2^31 or F >= 2^31, count_dev NULL, faces_dev NULL with F > 0,
 * label_dev / tri_count_dev / vert_count_dev / workspace_dev NULL with V > 0, count_dev / workspace_dev / faces_dev not 8-byte
 * aligned, label_dev / tri_count_dev / vert_count_dev not 4-byte aligned.  V == 0 writes only the two counters (0 and F: every
 * face is out of range).  ns_mesh_components_workspace_bytes is 0 for a shape that would be refused.                          */
#define NS_MESH_COMPONENTS_SHARE 1024
int64_t ns_mesh_components_workspace_bytes(int64_t V, int64_t F);
int ns_mesh_components(const int64_t* faces_dev, int64_t F, int64_t V, int32_t* label_dev, int32_t* tri_count_dev,
                       int32_t* vert_count_dev, int64_t* count_dev, void* workspace_dev, void* stream);

/* ---- per-vertex normals of the device mesh  (what every NeRF mesh export ships so that a viewer shades the surface, not the
 * triangulation; not in the reference) ----  The finite-difference gradient of the density lattice, interpolated along the
 * vertex's own lattice edge: a function of the edge alone, as the position is -- no atomics, no adjacency, no dependence on the
 * triangulation.  Lattice, sigma_stride and lin are exactly ns_mesh_extract's.
 * KEY: key_dev[v], v in [0, V), is lin(a) * 8 + code as ns_mesh_extract's key_out holds it: the offset is
 * d = (code & 1, (code >> 1) & 1, code >> 2) and b = a + d.  Keys need not be sorted or distinct.
 * NODAL GRADIENT at lattice point q, per axis with index x in [0, G) and spacing h, s[.] the values along that axis through q:
 *   xm = max(x - 1, 0),  xp = min(x + 1, G - 1),
 *   g  = (s[xp] - s[xm]) / ((float)(xp - xm) * h)     one fp32 subtraction, one fp32 multiplication (exact: the factor is 1 or
 *                                                     2) and one correctly rounded fp32 division:
 * the central difference where both neighbours exist, the one-sided one on the lattice boundary.
 * GRADIENT AT THE VERTEX on the edge between a and b with values s_a and s_b:
 *   tt = (iso - s_a) / (s_b - s_a)       the same expression as the vertex's,
 *   g  = g_a + tt * (g_b - g_a)          per axis, every operation rounded separately.
 * NORMAL: G = (double) g, len = sqrt(Gx * Gx + Gy * Gy + Gz * Gz) added left to right in fp64, n = (float)(-G / len) per axis,
 * normal_out[v * 3 ..] -- fp64 so that no density scale overflows the sum of squares and numpy float64 restates the bits (a
 * correctly rounded fp64 square root and division).  It points outward: inside is sigma >= iso and the density falls towards the
 * outside, the side ns_mesh_extract's winding faces.
 * DEGENERATE vertex: s_a, s_b, tt or any component of g is not finite, or len == 0: the normal is (0, 0, 0) and the vertex is
 * counted in count_dev[0].  A key whose edge does not cross iso is legal: tt lies outside [0, 1] and the formula extrapolates.
 * INVALID key: negative, lin(a) >= Gx * Gy * Gz, code == 0, or b outside the lattice on any axis: the normal is (0, 0, 0) and
 * the key is counted in count_dev[1] only, not also as degenerate; no address is ever formed from an invalid key.
 * Both counters are overwritten, not accumulated.  Nothing is written outside normal_out[0 .. 3 V).
 * Two launches on `stream`, no atomics of any kind: (1) workgroup g takes the NS_MESH_NORMALS_SHARE keys from
 * g * NS_MESH_NORMALS_SHARE on (thread t takes g * NS_MESH_NORMALS_SHARE + s * 256 + t), writes their normals and its two int64
 * partial counts into workspace_dev (ns_mesh_normals_workspace_bytes(V) bytes; what it holds before the call does not matter);
 * (2) ONE workgroup adds the partials in the order of g and writes count_dev.  V == 0 writes the two zeros and launches nothing
 * else.  A gather: per vertex s_a, s_b and up to twelve stencil neighbours as 4-byte loads; ascending keys (ops.mesh_weld's
 * order) make neighbouring threads read neighbouring lattice rows.  Not part of this: normals of meshes that did not come from
 * a lattice (no keys), the field's analytic gradient, normal maps of rendered frames.
 * Checked before any launch (NS_E_INVALID): a dimension below 2, Gx * Gy * Gz >= 2^31, a negative stride, a non-finite iso or
 * h, h <= 0, V < 0 or V >= 2^31, count_dev NULL, with V > 0 any of sigma_dev / key_dev / normal_out / workspace_dev NULL,
 * key_dev / count_dev / workspace_dev not 8-byte aligned, normal_out not 4-byte aligned.  ns_mesh_normals_workspace_bytes is 0
 * for a shape that would be refused (and for V == 0, which needs none).                                                       */
#define NS_MESH_NORMALS_SHARE 1024
int64_t ns_mesh_normals_workspace_bytes(int64_t V);
int ns_mesh_normals(const float* sigma_dev, int64_t sigma_stride, int Gx, int Gy, int Gz, float iso, float h_x, float h_y,
                    float h_z, const int64_t* key_dev, int64_t V, float* normal_out, int64_t* count_dev, void* workspace_dev,
                    void* stream);

/* ---- the device mesh rasterised from a pinhole camera  (the frame a mesh viewer shows; not in the reference) ----  A z-buffer
 * rasteriser whose frame sits on the field's: depth_out is the ray parameter along the unnormalised direction of ns_get_rays'
 * pixel (its camera-space z component is -1), the unit of the one-call renderers' depth extra, so ns_depth_sqerr and
 * ns_image_sqerr score the mesh against the field and the photographs.  A result is a function of the inputs alone.
 * INPUTS: vertices_dev fp32 [V,3]; faces_dev int64 [F,3] (ops.mesh_weld's); attr_dev fp32 [V,3] vertex colours or NULL; the
 * camera as ns_get_rays takes it (c2w_host: 12 host floats, row-major [3,4]; fx, fy, cx, cy; H, W); near_ > 0; cull 0 none,
 * 1 back faces, 2 front faces; background.
 * PROJECTION of vertex p, every fp32 operation rounded on its own (the inverse of ns_get_rays' pixel ray), r = c2w[:3,:3]
 * row-major, t = c2w[:3,3]:  e_c = p_c - t_c;  q_k = (e_0 r[k] + e_1 r[3 + k]) + e_2 r[6 + k], k = 0, 1, 2;  z = -q_2;
 * x = cx + fx (q_0 / z);  y = cy - fy (q_1 / z).  Pixel (column i, row j) is the sample point (x, y) = (i, j), NOT
 * (i + 1/2, j + 1/2): the project's ray through pixel (i, j) uses (i - cx) / fx.
 * SNAPPING: X = (int64) rintf(x * 256.0f), Y likewise: eight sub-pixel bits, round half to even.  A vertex is UNUSABLE if x, y
 * or z is not finite, z < near_, or |x| or |y| exceeds 2^20 pixels -- with that bound |X|, |Y| <= 2^28 and every edge value
 * below is smaller than 2^59 in magnitude.  A face with an unusable vertex is dropped and counted in count_dev[0] (clipped):
 * there is no near-plane clipping, and the count says when a camera sits inside the mesh.
 * COVERAGE, int64 throughout: E_AB(P) = (B_x - A_x)(P_y - A_y) - (B_y - A_y)(P_x - A_x); pixel (i, j) is P = (256 i, 256 j);
 * area2 = E_01(V_2).  area2 == 0: dropped and counted in count_dev[1] (degenerate).  FACING: x grows to the right and y DOWN the
 * frame, so a face of ns_mesh_extract's outward winding seen from outside has area2 < 0: that is the FRONT; cull = 1 drops
 * faces with area2 > 0, cull = 2 those with area2 < 0 (neither is counted).  w_0 = E_12(P), w_1 = E_20(P), w_2 = E_01(P) are
 * the edge values opposite vertices 0, 1, 2 and sum to area2.  With sg = the sign of area2, the pixel is covered iff for each
 * k: sg w_k > 0, or sg w_k == 0 and the TIE RULE gives the edge's points to this side -- top-left, a function of the edge's two
 * snapped end points and the side alone: for d = sg (B - A), the edge walked so that the triangle lies where its edge value is
 * positive, a centre on the edge is covered iff d_y < 0 (the triangle lies at larger x: a left edge) or d_y == 0 and d_x > 0
 * (it lies at larger y: a top edge).  The two sides of an edge get opposite d, so a centre on an edge shared by two triangles
 * that do not overlap is covered by exactly one of them whatever their windings, and a centre on the shared vertex of a closed
 * fan by exactly one triangle of the fan (the rule is that of sampling at P + (eps, eps^2)).  The bounding box is clamped to
 * the frame; faces wholly outside it are no error and are not counted.
 * DEPTH of a covered pixel, fp64: s = ((double) w_0 / (double) z_0 + (double) w_1 / (double) z_1) + (double) w_2 / (double) z_2,
 * zpix = (float)((double) area2 / s): perspective-correct (1 / z is affine on the screen), never below the smallest z_k.
 * Z-BUFFER: one uint64 per pixel, all ones when empty; a fragment is ((uint64) bits(zpix) << 32) | (uint32) face index, merged
 * by a 64-bit unsigned atomic minimum: zpix >= near_ > 0, so the bits order as the values do -- the nearest surface wins, at
 * equal depth bits the smaller face index.  Integer atomics only (that minimum, and atomicAdd on the counters and on the
 * length of a list of faces); no floating-point atomic anywhere, so nothing depends on the order of the atomics.
 * RESOLVE: an empty pixel gets depth_out = 0 (the field's depth of a ray through empty space), tri_out = -1, rgb_out =
 * background.  A covered one: depth_out and tri_out from the word; rgb_out per channel c from the w_k of that face recomputed
 * at that pixel, num = ((w_0 / z_0) a_0c + (w_1 / z_1) a_1c) + (w_2 / z_2) a_2c in fp64 with the quotients of DEPTH,
 * rgb_out = (float)(num / s).  depth_out fp32 [H*W], tri_out int32 [H*W], rgb_out fp32 [H*W,3]: any may be NULL.
 * INVALID face: an index outside [0, V) -- negative ones and those >= 2^32 included -- is counted in count_dev[2] and only
 * there; none of its indices is ever used as an address.  count_dev[3] = the number of covered pixels.  All four int64 are
 * overwritten, not accumulated.  Nothing is written outside the outputs and workspace_dev
 * (ns_mesh_raster_workspace_bytes(V, F, H, W) bytes; what it holds before the call does not matter).
 * LAUNCHES, all on `stream`, nothing read back in between, no workgroup waiting for another: (1) z-buffer and counters cleared;
 * (2) every vertex projected once into the workspace (X, Y, z, usable); (3) workgroup g takes the NS_MESH_RASTER_SHARE faces
 * from g * NS_MESH_RASTER_SHARE on (thread t takes g * NS_MESH_RASTER_SHARE + s * 256 + t): a face whose clamped bounding box
 * has at most NS_MESH_RASTER_BIG_BOX pixels is rasterised by its thread, a larger one is appended to a list in the workspace;
 * (4) a grid of fixed size strides over that list, whose length it reads from device memory, in tiles of 16 x 16 pixels, one
 * pixel per thread; (5) resolve, one thread per pixel.  The path a face takes is not observable (ns_debug_set
 * "mesh_raster_big_box" moves the threshold; the bits stay).  F == 0 is one launch: a frame of background, four zeros.
 * Checked before any launch (NS_E_INVALID): H or W < 1 or > 16384; V or F < 0 or >= 2^31; c2w_host NULL; a non-finite c2w, fx,
 * fy, cx, cy, near_ or background; fx or fy == 0; near_ <= 0; cull outside 0 .. 2; count_dev NULL; with F > 0 vertices_dev,
 * faces_dev or workspace_dev NULL; rgb_out without attr_dev; faces_dev, count_dev or workspace_dev not 8-byte aligned.
 * ns_mesh_raster_workspace_bytes is 0 for a shape that would be refused (and for F == 0, which needs none).  Not part of this:
 * antialiasing, lighting, textures, near-plane clipping, meshes or frames of 2^31 elements.                                  */
#define NS_MESH_RASTER_SHARE 1024
#define NS_MESH_RASTER_BIG_BOX 1024
int64_t ns_mesh_raster_workspace_bytes(int64_t V, int64_t F, int H, int W);
int ns_mesh_raster(const float* vertices_dev, int64_t V, const int64_t* faces_dev, int64_t F, const float* attr_dev,
                   const float* c2w_host, float fx, float fy, float cx, float cy, int H, int W, float near_, int cull,
                   float background, float* depth_out, int32_t* tri_out, float* rgb_out, int64_t* count_dev,
                   void* workspace_dev, void* stream);

/* ---- the device mesh simplified by vertex clustering  (what every NeRF mesh export does on the host before it hands the mesh
 * to a viewer -- the lattice-resolution surface is millions of slivers; not in the reference) ----  Rossignac and Borrel's vertex
 * clustering on a coarse lattice, with one change: a cluster is represented by ONE OF ITS OWN vertices, the member nearest the
 * cluster's centroid, not by a new point.  Every vertex that stays is an input vertex bit for bit: its lattice-edge key, its
 * ns_mesh_normals normal and its colour stay valid, and it still lies on the isosurface.  A result is a function of the inputs
 * alone.  The arithmetic is csrc/ns_mesh_cluster.h, one text for the kernels and the CPU, every fp64 operation rounded on its own.
 * INPUTS: vertices_dev fp32 [V,3]; faces_dev int64 [F,3]; lo_host, cell_host: three host floats each; dims_host: three host ints.
 * CLUSTER LATTICE: lo and cell finite, cell > 0; dims Cx, Cy, Cz each in [1, 2^15], Cx * Cy * Cz <= 2^24 (the table is dense: 40
 * bytes per cell, 640 MiB at the limit; 128^3 is 80 MiB).
 * COORDINATE of a vertex per axis, 16 fractional bits: u = llrint((((double) v - (double) lo) / (double) cell) * 65536.0), round
 * half to even, clamped to [0, C * 65536 - 1] -- a vertex outside the lattice belongs to the nearest boundary cell.  CELL per axis:
 * u >> 16; linear (cz * Cy + cy) * Cx + cx.  A vertex with a NaN or infinite coordinate belongs to no cluster: rep_out[v] = -1,
 * and it is counted in count_dev[3].
 * ACCUMULATE: per cluster S = the three sums of u over its members (int64; u < 2^31 and n < 2^31, so S < 2^62) and n = their
 * number (int32), by integer atomicAdd.
 * REPRESENTATIVE: for a member v, d = sum over x, y, z in that order of ((double) u - (double) S / (double) n)^2 in fp64, every
 * operation rounded on its own, d32 = (float) d.  The representative is the member with the smallest 64-bit word
 * ((uint64) bits(d32) << 32) | v, merged by a 64-bit unsigned atomic minimum (ns_mesh_raster's z-buffer pattern): d32 >= 0, so
 * the bits order as the values do -- the member nearest the centroid wins, at equal d32 the smaller index.  rep_out[v] int32,
 * v in [0, V): the representative of v's cluster, in the input numbering; rep_out[rep_out[v]] == rep_out[v].
 * FACES: face (a, b, c) is judged in this order: an index outside [0, V) -> INVALID, counted in count_dev[2] (none of its indices
 * is used as an address); else a corner with rep == -1 -> counted in count_dev[4]; else two of rep[a], rep[b], rep[c] equal ->
 * COLLAPSED, counted in count_dev[1]; else KEPT: (rep[a], rep[b], rep[c]) is written to faces_out (int64 [capacity,3], input
 * vertex numbering, winding kept) at its rank among the kept faces in input order.  count_dev[0] = the number of kept faces,
 * whatever the capacity: those at rank >= capacity are counted and never written (capacity == 0: a pure count).
 * count_dev[5] = the number of representatives (the occupied clusters).  All six int64 are overwritten, not accumulated.
 * Nothing is written outside rep_out[0 .. V), faces_out[0 .. 3 min(kept, capacity)), count_dev[0 .. 6) and workspace_dev
 * (ns_mesh_simplify_workspace_bytes(V, F, Cx, Cy, Cz) bytes; what it holds before the call does not matter).
 * LAUNCHES, all on `stream`, nothing read back in between, no workgroup waiting for another: (1) the table and two 32-bit
 * counters cleared; (2) accumulate: workgroup g takes the NS_MESH_SIMPLIFY_SHARE vertices from g * NS_MESH_SIMPLIFY_SHARE on
 * (thread t takes g * NS_MESH_SIMPLIFY_SHARE + s * 256 + t); (3) choose: every member reads its cluster's finished sums and
 * offers its word; (4) resolve: rep_out written, the representatives counted; (5) count: workgroup g judges the
 * NS_MESH_SIMPLIFY_SHARE faces from g * NS_MESH_SIMPLIFY_SHARE on, four int64 per share into the workspace; (6) ONE workgroup
 * turns the kept counts into output indices and writes count_dev; (7) emit: every workgroup judges its faces again and places the
 * kept ones by ns_block.h's share_place -- no atomics on the output.  Integer atomics only (atomicAdd on 64- and 32-bit words,
 * the 64-bit atomicMin); no floating-point atomic anywhere, so nothing depends on the order of the atomics.  V == 0 skips (2) to
 * (4) (every face is invalid), F == 0 skips (5) and (7).
 * Checked before any launch (NS_E_INVALID): V or F < 0 or >= 2^31; lo_host, cell_host or dims_host NULL; a non-finite lo or
 * cell, cell <= 0; a dimension below 1 or above 2^15, a product above 2^24; capacity < 0; count_dev or workspace_dev NULL; with
 * V > 0 vertices_dev or rep_out NULL; with F > 0 faces_dev NULL, and faces_out NULL unless capacity == 0; faces_dev, faces_out,
 * count_dev or workspace_dev not 8-byte aligned; vertices_dev or rep_out not 4-byte aligned.
 * ns_mesh_simplify_workspace_bytes is 0 for a shape that would be refused.
 * ns_mesh_cluster_coord and ns_mesh_cluster_distance run csrc/ns_mesh_cluster.h on the host for one vertex (no device, no
 * launch): u_out[3] and *cell_out (the linear cell, -1 for a non-finite vertex) -- returns 1 for a finite vertex, 0 for a
 * non-finite one, NS_E_INVALID for a lattice the entry would refuse --, and *d_out = d32 of a member with coordinate u_host[3] in
 * a cluster with sums sums_host[3] and n >= 1 members.  They exist so that the tests compare the library's own text with numpy.
 * Not part of this: quadric error metrics, new vertex positions at the centroid, manifold or topology guarantees, the removal of
 * duplicate faces (ops.mesh_simplify does that in torch), and meshes of 2^31 vertices or faces or more.                       */
#define NS_MESH_SIMPLIFY_SHARE 1024
int64_t ns_mesh_simplify_workspace_bytes(int64_t V, int64_t F, int Cx, int Cy, int Cz);
int ns_mesh_simplify(const float* vertices_dev, int64_t V, const int64_t* faces_dev, int64_t F, const float* lo_host,
                     const float* cell_host, const int* dims_host, int32_t* rep_out, int64_t* faces_out, int64_t capacity,
                     int64_t* count_dev, void* workspace_dev, void* stream);
int ns_mesh_cluster_coord(const float* vertex_host, const float* lo_host, const float* cell_host, const int* dims_host,
                          int32_t* u_out, int32_t* cell_out);
int ns_mesh_cluster_distance(const int32_t* u_host, const int64_t* sums_host, int32_t n, float* d_out);

/* ---- a rendered frame as 8-bit pixels (run_nerf_helpers.py:11 to8b = (255 * np.clip(x, 0, 1)).astype(np.uint8);
 * nerf_utils.py:322-325 render_path's rgb8 = to8b(rgbs[-1]) written as {i:03d}.png) ----  Quantised on the device, so that a
 * quarter of the frame's bytes cross to the host:
 *   out_dev[p * C + c] = (uint8) trunc(255.0f * min(max(x, 0), 1)),  x = rgb_dev[p * rgb_stride + c],  c = 0, 1, 2,
 * p in [0, n_pixels), C = out_channels: ONE fp32 multiply, then truncation -- numpy's bits on fp32 input for every finite x.
 * NaN gives 0 (numpy leaves the cast of NaN to the platform; here it is defined), as -0.0, everything below 0 and -inf do;
 * +inf gives 255.  rgb_stride as ns_image_sqerr's: in floats, 0 = packed 3, 3 or 4 (the interleaved [R,4] shard, whose fourth
 * float is never used).  out_channels is 3 or 4; with 4 the fourth byte is the same map of alpha_dev[p] (packed [n_pixels]), or
 * 255 when alpha_dev is NULL; alpha_dev with 3 channels is ignored.  rgb_dev and alpha_dev need no more than a float's
 * alignment and out_dev none (a row band of a frame): a thread converts four pixels and stores their 12 or 16 bytes as whole
 * dwords when out_dev is 4-byte aligned, and as bytes otherwise and for the last pixels of a count that is no multiple of 4;
 * it loads float4s when rgb_dev is 16-byte aligned and single floats otherwise.  Nothing outside out_dev[0 .. n_pixels * C) is
 * written.  One launch on `stream`.  Checked before the launch (NS_E_INVALID): n_pixels < 0, n_pixels * 4 >= 2^31, a stride
 * other than 0, 3 or 4, out_channels other than 3 or 4, and for n_pixels > 0 rgb_dev or out_dev NULL.  n_pixels == 0 does
 * nothing and returns NS_OK.                                                                                              */
int ns_frame_to8b(const float* rgb_dev, int64_t rgb_stride, const float* alpha_dev, int64_t n_pixels, uint8_t* out_dev,
                  int out_channels, void* stream);

/* ---- the maximum of per-ray maps, kept on the device  (Trainer.py:371-376: the i_video branch writes
 * to8b(disps / np.max(disps)), one divisor for ALL frames of the spiral) ----  state_dev is two floats in device memory:
 *   state[0] = the maximum over the values seen that are not NaN, -inf when there are none,
 *   state[1] = 1.0f if a NaN was seen, otherwise 0.0f.
 * map_dev[i * stride], i in [0, n), is a per-ray fp32 map; stride is in floats: 1 = packed [R], 4 = the [:, 3] column of the
 * interleaved [R,4] shard, whose base lies 12 bytes into the shard -- map_dev needs no more than a float's alignment (a packed
 * map on a 16-byte boundary is read as float4s, everything else one dword per value).  accumulate == 0 initialises the state
 * from this map alone; accumulate != 0 folds this map into the state already there, so that calls over the frames of a
 * sequence leave the state of their concatenation and nothing is read back in between.  n == 0 writes (-inf, 0) under
 * accumulate == 0 and leaves the state as it is otherwise (map_dev and workspace_dev may then be NULL).  (np.max itself
 * returns NaN when any value is NaN -- a ray without opacity has disparity 0 / 0 -- and the reference's disp.mp4 is then
 * black; the flag reports that case and the maximum stays usable.)  The sign of a zero maximum is not specified.
 * Shaped as ns_image_sqerr: workgroup g folds the 2048 values from g * 2048 on into one (max, flag) pair of workspace_dev
 * (ns_map_max_workspace_bytes(n) bytes, 8-byte aligned), and a second launch of ONE workgroup folds the pairs and, under
 * accumulate, the old state.  A maximum does not depend on the order of its comparisons: no atomics, the same bits on every
 * call.  Checked before any HIP call (NS_E_INVALID): n < 0, n >= 2^31, a stride other than 1 or 4, state_dev NULL or not
 * 4-byte aligned, workspace_dev not 8-byte aligned, and for n > 0 map_dev or workspace_dev NULL.
 * ns_map_max_workspace_bytes is 0 for n <= 0 and for a count that would be refused.                                        */
int64_t ns_map_max_workspace_bytes(int64_t n);
int ns_map_max(const float* map_dev, int64_t stride, int64_t n, int accumulate, float* state_dev, void* workspace_dev,
               void* stream);

/* ---- a per-ray map as 8-bit pixels, divided by a number in device memory  (Trainer.py:371-376
 * to8b(disps / np.max(disps)); run_nerf_helpers.py:11 to8b) ----
 *   out_dev[i] = (uint8) trunc(255.0f * min(max(q, 0), 1)),  q = map_dev[i * stride] / *denom_dev,  i in [0, n):
 * ONE correctly rounded fp32 division -- numpy's float32 / float32, never a reciprocal and a multiply, which differ in the
 * last bit often enough to move a pixel -- then ns_frame_to8b's clip (comparisons), multiply and truncation.  A NaN quotient
 * gives 0: a NaN value, 0 / 0, inf / inf, a NaN divisor.  denom_dev == NULL: no division (q is the value itself).  denom_dev
 * is any 4-byte aligned float in device memory, read by the kernel -- the state of ns_map_max itself, so that the divisor of
 * a sequence never crosses to the host.  stride as ns_map_max's.  A thread converts four consecutive values and stores their
 * bytes as one dword when out_dev is 4-byte aligned, and as bytes otherwise and for the last values of a count that is no
 * multiple of 4; nothing outside out_dev[0 .. n) is written.  One launch on `stream`.  Checked before the launch
 * (NS_E_INVALID): n < 0, n >= 2^31, a stride other than 1 or 4, denom_dev not 4-byte aligned, and for n > 0 map_dev or
 * out_dev NULL.  n == 0 does nothing and returns NS_OK.                                                                    */
int ns_map_to8b(const float* map_dev, int64_t stride, int64_t n, const float* denom_dev, uint8_t* out_dev, void* stream);

/* ---- a2 find_intersection_points_with_sphere / solve_quadratic_equation (utils.py:159-217)
 * t [R,2] (minus-sqrt root first) and points [R,2,3]; NaN where the line misses the sphere.  */
int ns_sphere_intersect(const float* o_dev, const float* d_dev, int64_t R, float radius,
                        float* t_dev, float* pts_dev, void* stream);
/* element-wise quadratic roots: out [2,n] */
int ns_solve_quadratic(const float* a_dev, const float* b_dev, const float* c_dev, int64_t n,
                       float* out_dev, void* stream);

/* ---- a3  Embedder.embed (run_nerf_helpers.py:15-63): x [M,d] -> [M, d*(1+2L)] ------------- */
int ns_posenc(const float* x_dev, int64_t M, int d, int n_freqs, float* out_dev, void* stream);

/* ---- packed network weights ------------------------------------------------------------
 * Host-side packers: take the reference state-dict tensors (HOST fp32, row-major
 * [out,in] weights as nn.Linear stores them) and build the device-resident MFMA weight
 * stream.  Handles own device memory; destroy with ns_weights_destroy.                      */
typedef struct ns_weights ns_weights; /* opaque */

/* NeRF(D, W, input_ch=63, input_ch_views=27, skips=[skip], use_viewdirs=True)
 * (run_nerf_helpers.py:67-134).  w/b: arrays of D + 4 host pointers in the order
 * pts_linears.0..D-1, feature_linear, alpha_linear, views_linears.0, rgb_linear.
 * skip = index i after which the embedded input is re-concatenated (4), or -1 for none.
 * feature_linear (no activation) is composed with views_linears.0 at pack time, in fp64.   */
int ns_pack_nerf(int D, int W, int skip, const float* const* w, const float* const* b, int dtype,
                 ns_weights** out);
/* The full signature of the reference's NeRF (run_nerf_helpers.py:67-134): any `skips` list (bit i of skip_mask set
 * <=> i in skips; every skip must precede the last layer, D <= 32) and both head variants.  use_viewdirs != 0: as
 * ns_pack_nerf (w/b: D + 4 tensors; raw has 4 channels whatever output_ch says, :126-131).  use_viewdirs == 0: the
 * head is output_linear (W -> output_ch, :132-133; w/b: D + 1 tensors, pts_linears.0..D-1 then output_linear), the
 * network takes no view directions, and raw has output_ch channels (create_nerf builds 5 with N_importance > 0,
 * nerf_utils.py:405-406).  W: any width from 2 to 256 (netwidth, nerf_utils.py:409-423): the kernels are instantiated
 * for 128 and 256 and the packer zero-pads every tensor to the next of the two -- a padded unit is relu(0) = 0 and feeds
 * zero columns, so the real units sum the same products plus exact zeros.                                           */
int ns_pack_nerf_ex(int D, int W, uint32_t skip_mask, int use_viewdirs, int output_ch,
                    const float* const* w, const float* const* b, int dtype, ns_weights** out);
/* channels of the raw output of a packed NeRF (4, or output_ch without view directions) */
int ns_nerf_out_channels(const ns_weights* net);
/* DepthNet(hidden_sizes, cat_hidden_sizes, multires=10) (depth_net.py:10-169).  w/b: 3*n_branch + n_trunk + 1
 * host pointers in the order origin_layers.0.., direction_layers.0.., intersection_layers.0.., cat_layers.0,2,..,
 * to_depth.0.  hidden_sizes [n_branch]: widths of the three skip branches (any); cat_sizes [n_trunk]: trunk widths,
 * each <= 256 (class defaults [128]*6 / [128,128,128,128,256] and the production 10 x 256 both qualify).
 * The skip branches are affine (the reference constructs nn.LeakyReLU(x) and never applies it, depth_net.py:140,148,
 * 156), so the packer composes them with the first trunk layer, in fp64, into one 252 -> cat_sizes[0] layer; trunk
 * layers are zero-padded to one width in {128, 256}.                                                          */
int ns_pack_depthnet_ex(int n_branch, const int* hidden_sizes, int n_trunk, const int* cat_sizes,
                        const float* const* w, const float* const* b, int dtype, ns_weights** out);
/* the uniform case: hidden_sizes = cat_hidden_sizes = [width] * n_layers */
int ns_pack_depthnet(int n_layers, int width, const float* const* w, const float* const* b,
                     int dtype, ns_weights** out);
/* The pack-time folds on their own (HOST only, no device touched; tests check them against the literal chain):
 * F_out [c0, 252] and bias_out [c0] of the folded DepthNet front end on cat[gamma(o), gamma(d), gamma(isect)]
 * (w/b: the 3*n_branch branch tensors followed by cat_layers.0);                                              */
int ns_fold_depthnet_front(int n_branch, const int* hidden_sizes, int c0, const float* const* w,
                           const float* const* b, float* F_out, float* bias_out);
/* w_out [W/2, W+27], b_out [W/2] of views_linears[0] o feature_linear (run_nerf_helpers.py:119-125)             */
int ns_fold_nerf_views(int W, const float* w_feature, const float* b_feature, const float* w_views,
                       const float* b_views, float* w_out, float* b_out);
/* The weight stream and the bias image ns_pack_nerf_ex builds, into HOST buffers (no device touched; tests compare the two
 * orders): sigma_first = 0 the stream every kernel walks, 1 the render kernel's sigma-first twin (NS_E_UNSUPPORTED unless
 * the network is a 16-bit production field: 8 x 256, skips = [4], view directions, bf16 / f16).  The sizes always come back
 * in *stream_bytes / *bias_floats; stream_out / bias_out may be NULL to ask for them alone.                            */
int ns_pack_nerf_host_image(int D, int W, uint32_t skip_mask, int use_viewdirs, int output_ch, const float* const* w,
                            const float* const* b, int dtype, int sigma_first, void* stream_out, int64_t stream_cap,
                            float* bias_out, int64_t bias_cap, int64_t* stream_bytes, int64_t* bias_floats);
void ns_weights_destroy(ns_weights* w);
/* Tells the dispatch that the caller packed the handle's hidden units in descending firing rate (NeRF.packed() does, for the
 * production 16-bit fields): a hint for the choice of kernel ("kblock_suffix" = 2), never for results.                 */
int ns_weights_set_unit_ordered(ns_weights* w, int unit_ordered);
/* bytes of the device weight stream (for roofline accounting) */
int64_t ns_weights_stream_bytes(const ns_weights* w);

/* ---- a4  DepthNet.forward (depth_net.py:117-169): (o,d) [R,3] -> z [R] in [near,far] -------- */
int ns_depthnet_forward(const ns_weights* net, const float* o_dev, const float* d_dev, int64_t R,
                        float near_, float far_, float sphere_radius, float* z_dev, void* stream);

/* ---- a5  sample_points_around_mean (utils.py:220-244) ---------------------------------------
 * mean [R]; noise [R,N-1] standard-normal draws (GAUSSIAN only, else NULL); outputs z [R,N]
 * and pts [R,N,3] (either may be NULL).  DEPTH_ONLY ignores N (treated as 1).               */
int ns_place_samples(int mode, const float* o_dev, const float* d_dev, const float* mean_dev,
                     const float* noise_dev, int64_t R, int N, float std_, float* pts_dev,
                     float* z_dev, void* stream);

/* ---- a6+a7  Trainer.run_network + NeRF.forward (Trainer.py:789-806, helpers :67-134) --------
 * pts [R,N,3], viewdirs [R,3] -> raw [R,N,C] = (rgb pre-sigmoid, sigma pre-relu[, ...]), C = ns_nerf_out_channels(net)
 * (4 for every network with view directions).  viewdirs_dev is ignored (may be NULL) for a network packed with
 * use_viewdirs == 0.  If pts_dev is NULL the points are formed in-kernel as o + d*z from o,d [R,3], z [R,N].     */
int ns_nerf_forward(const ns_weights* net, const float* pts_dev, const float* o_dev,
                    const float* d_dev, const float* z_dev, const float* viewdirs_dev, int64_t R,
                    int N, float* raw_dev, void* stream);
/* NeRF.forward on an already embedded input x [M,90] (x [M,63] without view directions) -> [M,C] */
int ns_nerf_forward_embedded(const ns_weights* net, const float* x_dev, int64_t M, float* raw_dev,
                             void* stream);

/* ---- a8  raw2alpha + DepthNetTrainer.raw2outputs (nerf_utils.py:27-42, sampling_trainer.py
 * :153-230).  raw [R,N,4], z [R,N], rays_d [R,3]; noise [R,N] already multiplied by
 * raw_noise_std, or NULL.  Outputs (any may be NULL): rgb [R,3], disp/acc/depth [R],
 * alphas/weights [R,N].  (density is raw[...,3], a view, and has no output here.)
 * N == 1 reproduces the reference exactly: its dists/alphas/weights are then EMPTY ([R,0]), so
 * rgb = sigmoid(raw rgb), acc = depth = 0, disp = 1e10 and alphas/weights are not written.    */
int ns_raw2outputs(const float* raw_dev, const float* z_dev, const float* rays_d_dev,
                   const float* noise_dev, int64_t R, int N, int white_bkgd, float* rgb_dev,
                   float* disp_dev, float* acc_dev, float* depth_dev, float* alphas_dev,
                   float* weights_dev, void* stream);
/* the same with the per-ray rgb / disp outputs at caller-chosen strides (in floats; rgb of ray r at
 * rgb_dev + r*rgb_stride, >= 3; disp at disp_dev + r*disp_stride, >= 1): lets a renderer write straight
 * into an interleaved [R,4] = (r,g,b,disp) frame shard, the unit the multi-GPU all-gather moves
 * (no reference counterpart: the reference returns separate tensors and has no multi-GPU path)      */
int ns_raw2outputs_strided(const float* raw_dev, const float* z_dev, const float* rays_d_dev,
                           const float* noise_dev, int64_t R, int N, int white_bkgd, float* rgb_dev,
                           int64_t rgb_stride, float* disp_dev, int64_t disp_stride, float* acc_dev,
                           float* depth_dev, float* alphas_dev, float* weights_dev, void* stream);

/* Backward of ns_raw2outputs: what torch autograd gives for DepthNetTrainer.raw2outputs (sampling_trainer.py:153-230,
 * raw2alpha nerf_utils.py:27-42) from the forward's INPUTS -- raw [R,N,4], z [R,N], rays_d [R,3], noise [R,N] or NULL,
 * white_bkgd, as ns_raw2outputs took them; the forward is re-run inside, nothing of it is saved.  Upstream gradients, any
 * NULL (that output takes no part in the loss): g_rgb [R,3], g_disp / g_acc / g_depth [R], g_alphas / g_weights [R,N]
 * (ignored for N == 1, where those outputs are [R,0]).  Outputs, each NULL when not wanted: d_raw [R,N,4] (rgb and sigma
 * channels; the noise is a constant), d_z [R,N] (through the distances and depth_map), d_rays_d [R,3] (through |d|).
 * torch's conventions where it has one: relu's subgradient at 0 is 0, torch.maximum splits the gradient in half on a tie
 * (the disp floor), NaN propagates as through torch's own backward formulas.  N <= 4096.                                 */
int ns_raw2outputs_backward(const float* raw_dev, const float* z_dev, const float* rays_d_dev, const float* noise_dev,
                            int64_t R, int N, int white_bkgd, const float* g_rgb_dev, const float* g_disp_dev,
                            const float* g_acc_dev, const float* g_depth_dev, const float* g_alphas_dev,
                            const float* g_weights_dev, float* d_raw_dev, float* d_z_dev, float* d_rays_d_dev, void* stream);
/* Backward of ns_place_samples w.r.t. the mean: d_z [R,N] -> d_mean [R].  Every sample is the mean plus a constant and the
 * sort only permutes them, so d_mean is the sum of d_z over the ray (the merged mean included); UNIFORM masks the samples
 * torch.clamp(., 2, 6) clipped (inclusive bounds, and a NaN mean gets 0 there, as torch's clamp backward gives).       */
int ns_place_samples_backward(int mode, const float* mean_dev, int64_t R, int N, float std_, const float* d_z_dev,
                              float* d_mean_dev, void* stream);

/* ---- a11 vanilla hierarchical pieces (Trainer.py:579-710, run_nerf_helpers.py:250-293) ------ */
/* stratified coarse depths: near/far [R]; t_rand [R,N] uniform draws or NULL (perturb==0)    */
int ns_coarse_z(const float* near_dev, const float* far_dev, int64_t R, int N, int lindisp,
                const float* t_rand_dev, float* z_dev, void* stream);
/* inverse-CDF sampling: bins [R,Nb], weights [R,Nb-1], u [R,Nf] or NULL (= linspace(0,1,Nf)) */
int ns_sample_pdf(const float* bins_dev, const float* weights_dev, int64_t R, int Nb, int Nf,
                  const float* u_dev, float* samples_dev, void* stream);
/* z_mid + sample_pdf(weights[1:-1]) + sort(cat[z, samples]) in one pass: z [R,Nc],
 * weights [R,Nc] -> z_out [R,Nc+Nf] ascending (Trainer.py:672-685)                         */
int ns_importance_z(const float* z_dev, const float* weights_dev, int64_t R, int Nc, int Nf,
                    const float* u_dev, float* z_out_dev, void* stream);
/* ascending sort of every row of x [R,N] (torch.sort(x,-1).values), N <= 2048 */
int ns_sort_rows(const float* x_dev, int64_t R, int N, float* out_dev, void* stream);
/* pts = o + d*z : o,d [R,3], z [R,N] -> [R,N,3] */
int ns_points_along_rays(const float* o_dev, const float* d_dev, const float* z_dev, int64_t R,
                         int N, float* pts_dev, void* stream);
/* per-ray argmax of weights [R,N] and the gathered z / weight / sigmoid(raw rgb)
 * (nerf_utils.py:813-819); any output may be NULL                                           */
int ns_argmax_gather(const float* weights_dev, const float* z_dev, const float* raw_dev, int64_t R,
                     int N, float* max_z_dev, float* max_w_dev, float* max_rgb_dev, void* stream);

/* ---- a9  the DepthNet branch of render_rays_test as one call (nerf_utils.py:836-865) --------
 * rays come either from (o,d,viewdirs) device arrays or, if o_dev is NULL, are generated in
 * place from the camera (rows [row0,row1) of an HxW image).  Runs DepthNet -> placement ->
 * NeRF MLP -> compositing on `stream` with intermediates in the caller-provided workspace.
 * Outputs rgb [R,3], disp [R] always; z/weights/pts (per-sample extras) only if non-NULL.
 * depth_dev / acc_dev [R] (packed, NULL = not produced): the expected depth sum_i w_i z_i and the opacity sum_i w_i of every
 * ray, exactly what ns_raw2outputs writes to its depth_dev / acc_dev for the call's own raw, z and rays_d -- acc before the
 * white-background add, from the guard's sigma under a guard, 0 for N == 1 (depth_only), NaN for a ray that misses the
 * sphere.  Both renderers produce them; the workspace sizes do not change.                                                */
typedef struct ns_render_args {
  const ns_weights* depthnet;
  const ns_weights* nerf;
  /* rays: explicit ... */
  const float* o_dev;
  const float* d_dev;
  const float* viewdirs_dev;
  int64_t R;
  /* ... or camera (used when o_dev == NULL) */
  int H, W, row0, row1;
  float fx, fy, cx, cy;
  float c2w[12];
  /* sampling set-up */
  int mode;    /* NS_MODE_* */
  int N;       /* trainer.n_depth_samples */
  float std_;  /* trainer.distance */
  const float* noise_dev; /* [R,N-1], GAUSSIAN only */
  float near_, far_, sphere_radius;
  int white_bkgd;
  /* workspace: ns_render_workspace_bytes(R,N) bytes of device memory */
  void* workspace_dev;
  /* outputs */
  float* rgb_dev;
  float* disp_dev;
  float* z_dev;       /* [R,N] or NULL */
  float* weights_dev; /* [R,N] or NULL */
  float* pts_dev;     /* [R,N,3] or NULL */
  /* optional hipEvent_t pair recorded on `stream` immediately before / after the NeRF-MLP kernel
   * (the dominant kernel), so a harness can time it inside its own timed region; NULL = none   */
  void* ev_mlp_begin;
  void* ev_mlp_end;
  /* strides (in floats) of the rgb / disp outputs; 0 = packed (3 / 1).  rgb_stride = disp_stride = 4 with
   * disp_dev = rgb_dev + 3 writes an interleaved [R,4] shard directly                                  */
  int64_t rgb_stride;
  int64_t disp_stride;
  /* PSNR guard (optional, NS_MODE_UNIFORM only; NULL = off).  The reference composites the LAST sample of a ray with
   * dist = 1e10 (sampling_trainer.py:176-180): alpha_last = step(sigma_last), so with 16-bit operands a sigma_last near
   * zero flips a ray's colour.  With a second handle of the SAME network packed NS_DTYPE_F16X3 (fp32-grade) here, the
   * last sample of every ray is evaluated a second time through it (R of the R*N samples, ~5 % of the frame) and its
   * sigma replaces the 16-bit one before compositing.  Pair it with an F16X3 DepthNet handle for fp32-grade depths.  */
  const ns_weights* nerf_guard;
  /* (Two options of guard_threshold, which follows them and stays the last field of the guard block.)
   * Rays of several 64-sample chunks (N a multiple of 64 in [128, 512]).  0 (the default): they take the every-ray guard whatever
   * guard_threshold says.  1: with guard_threshold > 0, an F16X3 layout-16 guard handle and a 16-bit field they take the
   * selective form as well -- the kernel flags the finished rays, the fix-up repeats the last chunk's additions from a
   * 192-byte record per flagged ray, and the workspace is ns_render_fused_guard_long_workspace_bytes(R) bytes (a call the
   * field is ignored for needs ns_render_fused_workspace_bytes(R) as before; the larger one serves both).  Ignored everywhere else (N <= 64, an F16X3 field, threshold 0, another guard packing,
   * ns_render_rays_depthnet): the call does what it does with 0.                                                        */
  int guard_long_selective;
  /* NULL, or one uint32 on the device: when the selective form ran (either ray length), the number of flagged rays is copied
   * there after the fix-up, device to device on `stream`; otherwise it is left as it is.                               */
  uint32_t* guard_count_dev;
  /* 0: the guard re-evaluates the last sample of EVERY ray.  > 0 (ns_render_rays_fused; N <= 64, or a multiple of 64 up to 512
   * with guard_long_selective above): only of the rays whose own 16-bit sigma of that sample lies within this distance of zero
   * -- the only ones whose step can flip: a sigma beyond it composites to alpha = 0 or 1 either way -- found by the kernel
   * itself, re-evaluated afterwards on a compacted list (three small launches; the count never leaves the device) and their
   * pixels re-added from the kernel's partial sums, bit for bit what the every-ray guard gives wherever
   * |sigma16 - sigma32| < guard_threshold.  The five-launch chain (ns_render_rays_depthnet), and the one-kernel renderer on
   * an F16X3 field, ignore it and guard every ray.                                                                        */
  float guard_threshold;
  float* depth_dev; /* [R] or NULL: expected depth sum_i w_i z_i (see above) */
  float* acc_dev;   /* [R] or NULL: opacity sum_i w_i, before the white-background add */
} ns_render_args;
int64_t ns_render_workspace_bytes(int64_t R, int N);
int ns_render_rays_depthnet(const ns_render_args* args, void* stream);
/* The same operator as ONE kernel per ray tile (the reference's chain nerf_utils.py:836-865):
 * rays -> DepthNet -> [sample placement + radiance-field MLP + raw2outputs in one persistent kernel].  Sample depths are
 * evaluated in-kernel from the DepthNet depth (no z array), raw stays in the CU and is composited in the MLP kernel's
 * epilogue by the same wave scan ns_raw2outputs runs: rgb / disp (and z / weights / pts when asked for) are BIT-IDENTICAL
 * to ns_render_rays_depthnet.  Three launches per call (ray generation, DepthNet, the fused kernel); HBM traffic is the
 * rays, 4 B + 16 B per ray and the weight streams.  Supported (ns_render_fused_supported != 0): mode NS_MODE_UNIFORM,
 * a bf16, f16 or f16x3 NeRF handle with view directions, N a power of two in [2, 64] or a multiple of 64 up to 512 (a ray is then
 * several 64-sample chunks composited side by side); anything else returns NS_E_UNSUPPORTED and
 * is served by ns_render_rays_depthnet.  Workspace: ns_render_fused_workspace_bytes(R) bytes, 256-byte aligned.        */
int ns_render_fused_supported(const ns_weights* nerf, int mode, int N);
int64_t ns_render_fused_workspace_bytes(int64_t R);
int64_t ns_render_fused_guard_long_workspace_bytes(int64_t R); /* with guard_long_selective = 1: 192-byte records, 288 B per ray */
int ns_render_rays_fused(const ns_render_args* args, void* stream);
/* The one-kernel renderer with forward-mode tangents in the DepthNet depth m of every ray.  In uniform placement every sample
 * depth is m + a constant, clipped to [2, 6], so a ray's composited outputs depend on m alone and their Jacobian is six numbers
 * per ray, carried through placement, encoding, field and compositing in the same kernel: nothing per sample is stored, and the
 * gradient of a loss in rgb / disp / depth / acc w.r.t. m is sum_k g_k J_k per ray.  The conventions are those of torch
 * autograd through ns_place_samples -> the NeRF -> ns_raw2outputs (ns_place_samples_backward's clip mask, relu'(0) = 0, half of
 * torch.maximum's tangent on a tie); a zero tangent contributes exactly 0, so a ray without a depth tangent (a NaN mean, every
 * sample clipped) has J = 0.  rgb / disp / depth / acc are bit-identical to ns_render_rays_fused on the same handle and mean.
 * What J means depends on the field.  On an F16X3 handle it is the fp32-grade Jacobian of that chain.  On an F16 handle it is
 * the derivative carried through that field's 16-bit arithmetic: the field's weights and activations are fp16 and so is the
 * tangent of every layer (relu' taken from the fp32 pre-activation), so J is the Jacobian of the f16 field, which differs from the
 * fp32-grade one where the field's rounding moves a kink.
 * NS_MODE_DEPTH_ONLY (the DepthNet branch of the training operator, nerf_utils.py:692-715): a ray is ONE sample at z = m, not
 * clipped (utils.py:220-244), its tangent 1; args->N is ignored and treated as 1, as ns_place_samples does, and std_ is ignored.
 * The outputs are what ns_raw2outputs documents for N == 1 -- rgb = sigmoid(raw rgb) whatever white_bkgd says, disp = 1e10,
 * depth = acc = 0 -- bit-identical to ns_render_rays_depthnet in this mode on the same handle and mean.  The Jacobian is
 * d rgb = rgb (1 - rgb) d raw rgb / d m (relu' conventions as above; a plain product, as torch's sigmoid backward: a NaN mean
 * gives a NaN rgb and a NaN d rgb for that ray only) and d disp = d depth = d acc = 0 exactly; sigma takes no part.  A group of
 * 64 samples is 64 rays, each finished by the lanes that hold it; F16X3 handles only (training wants the fp32-grade Jacobian).
 * Supported (ns_render_tangent_supported != 0): NS_MODE_UNIFORM with an F16X3 or F16 NeRF handle with view directions and N as in
 * ns_render_fused_supported; NS_MODE_DEPTH_ONLY with an F16X3 NeRF handle with view directions, at any N (ns_render_fused_supported
 * stays 0 for this mode); both ray sources, both mean sources, the rgb / disp strides, depth_dev / acc_dev.  Not supported
 * (NS_E_UNSUPPORTED or NS_E_INVALID before any launch): nerf_guard, z_dev / weights_dev / pts_dev, noise, a BF16 or F32 field,
 * an F16 field in NS_MODE_DEPTH_ONLY, NS_MODE_GAUSSIAN.  Workspace: ns_render_tangent_workspace_bytes(R) bytes, 256-byte aligned.  */
typedef struct ns_tangent_args {
  const float* mean_dev; /* [R] DepthNet depth supplied by the caller, or NULL: run args->depthnet as ns_render_rays_fused does */
  float* d_rgb_dev;      /* [R,3] d rgb / d mean, or NULL */
  float* d_disp_dev;     /* [R] */
  float* d_depth_dev;    /* [R] */
  float* d_acc_dev;      /* [R] */
} ns_tangent_args;
int ns_render_tangent_supported(const ns_weights* nerf, int mode, int N);
int64_t ns_render_tangent_workspace_bytes(int64_t R);
int ns_render_rays_fused_tangent(const ns_render_args* args, const ns_tangent_args* tangent, void* stream);

/* ---- a11 as one call: sample_as_in_NeRF (nerf_utils.py:497-611) = coarse pass, inverse-CDF importance
 * sampling, sorted merge, fine pass.  Rays explicit or generated from the camera (o_dev == NULL).
 * Outputs of the FINE pass: rgb [R,3], disp [R] always; z / weights [R,Nc+Nf] and raw [R,Nc+Nf,4] if
 * non-NULL.  t_rand [R,Nc] (stratified jitter) and u [R,Nf] (inverse-CDF draws) are NULL for the
 * deterministic perturb == 0 path.
 * The max-weight fine sample (nerf_utils.py:813-819: argmax of the fine weights, first index on ties, NaN the largest):
 * max_z [R,1], max_w [R,1] and max_rgb [R,3] (sigmoid of the sample's raw rgb), all three or none, bit-identical to
 * ns_argmax_gather on the call's own weights / z / raw; they need Nf > 0 and a workspace of
 * ns_hier_max_workspace_bytes(R, Nc, Nf) bytes.  A fine pass that composites in the MLP kernel reduces them in its epilogue;
 * otherwise ns_argmax_gather runs on the fine arrays (weights into weights_dev, or into the workspace).
 * depth_dev / acc_dev [R] (packed, NULL = not produced): the expected-depth and opacity maps of the FINE pass (of the coarse
 * pass when Nf == 0), exactly what ns_raw2outputs writes to its depth_dev / acc_dev for that pass's z and raw (acc before the
 * white-background add).  The workspace sizes do not change.                                                              */
typedef struct ns_hier_args {
  const ns_weights* coarse;
  const ns_weights* fine; /* NULL: the coarse network is used for both passes */
  const float* o_dev;
  const float* d_dev;
  const float* viewdirs_dev;
  int64_t R;
  int H, W, row0, row1;
  float fx, fy, cx, cy;
  float c2w[12];
  int Nc, Nf;
  int lindisp, white_bkgd;
  float near_, far_;
  const float* t_rand_dev;
  const float* u_dev;
  void* workspace_dev; /* ns_hier_workspace_bytes(R, Nc, Nf) bytes (ns_hier_max_workspace_bytes with max_*), 256-byte aligned */
  float* rgb_dev;
  float* disp_dev;
  float* z_dev;
  float* weights_dev;
  float* raw_dev;
  void* ev_mlp_begin; /* optional hipEvent_t pair around the FINE-pass MLP kernel */
  void* ev_mlp_end;
  int64_t rgb_stride; /* as in ns_render_args; 0 = packed */
  int64_t disp_stride;
  void* ev_coarse_begin; /* optional hipEvent_t pair around the COARSE-pass MLP kernel */
  void* ev_coarse_end;
  float* depth_dev;   /* [R] or NULL: expected depth of the fine pass (see above) */
  float* acc_dev;     /* [R] or NULL: its opacity */
  float* max_z_dev;   /* [R,1] or NULL: the max-weight fine sample (see above) */
  float* max_w_dev;   /* [R,1] or NULL */
  float* max_rgb_dev; /* [R,3] or NULL */
} ns_hier_args;
int64_t ns_hier_workspace_bytes(int64_t R, int Nc, int Nf);
/* the workspace of a call with the max-weight sample: ns_hier_workspace_bytes plus one [R, Nc+Nf] fp32 slice (256-aligned) */
int64_t ns_hier_max_workspace_bytes(int64_t R, int Nc, int Nf);
int ns_render_rays_hierarchical(const ns_hier_args* args, void* stream);

/* ---- training step of the DepthNet (Trainer.core_optimization_loop, Trainer.py:506-544) -------------
 * Batches are N_rand = 1024 rays, so these are small fp32 kernels (exact-fp32 MFMA products), not the
 * fused inference path.  One strided GEMM serves nn.Linear forward (y = x W^T + b), grad-input
 * (dx = dy W) and grad-weight (dW = dy^T x):
 *   C[i,j] (+)= sum_k A[i*sa0 + k*sa1] * B[j*sb0 + k*sb1] (+ bias[j]),  C row-major with leading dim ldc */
int ns_gemm_strided(const float* A_dev, int64_t sa0, int64_t sa1, const float* B_dev, int64_t sb0,
                    int64_t sb1, const float* bias_dev, float* C_dev, int64_t ldc, int M, int N, int K,
                    int accumulate, void* stream);
/* The same GEMM with fused epilogues (a training step is launch-bound: every elementwise kernel beside a GEMM costs as much
 * as a small GEMM): act != 0 applies an activation to the result (0 none, 1 relu, 2 leaky 0.01, 3 sigmoid: a forward
 * layer); dact != 0 multiplies the result by the derivative of activation `dact` evaluated from its OUTPUT
 * dact_ref[i*ld_ref + j] (the grad-input GEMM of the layer above carries the backward through this layer's activation);
 * a_rowsum [M], if non-NULL, receives sum_k A[i,k] (the bias gradient when A = dy^T, i.e. of the grad-weight GEMM).      */
int ns_gemm_fused(const float* A_dev, int64_t sa0, int64_t sa1, const float* B_dev, int64_t sb0,
                  int64_t sb1, const float* bias_dev, float* C_dev, int64_t ldc, int M, int N, int K,
                  int accumulate, int act, int dact, const float* dact_ref_dev, int64_t ld_ref,
                  float* a_rowsum_dev, void* stream);
/* Up to four such GEMMs in ONE launch (the three skip branches of the DepthNet run the same layer side by side); all
 * problems of a launch share their operand layout (sa1 == 1 or not, sb1 == 1 or not).  problems_host: HOST array.     */
typedef struct ns_gemm_problem {
  const float* A_dev; int64_t sa0, sa1;
  const float* B_dev; int64_t sb0, sb1;
  const float* bias_dev;
  float* C_dev; int64_t ldc;
  int M, N, K;
  int accumulate, act, dact;
  const float* dact_ref_dev; int64_t ld_ref;
  float* a_rowsum_dev;
} ns_gemm_problem;
int ns_gemm_fused_batched(const ns_gemm_problem* problems_host, int count, void* stream);
/* out[j] = sum_i X[i*ld + j]  (bias gradient) */
int ns_colsum(const float* X_dev, int64_t ld, int M, int N, float* out_dev, void* stream);
/* Grad-weight GEMM of the field fit, split over workgroups along the reduced dimension (split-K):
 *   dW[n*ldw + k] (+)= sum_m dy[m*dy_row_stride + n*dy_col_stride] * x[m*x_row_stride + k],   db[n] = sum_m dy[m, n]
 * for m < rows in [1, 2^31), n < N <= 512, k < K <= 512 (larger N or K: NS_E_UNSUPPORTED); x is contiguous along k.  accumulate
 * (0 / 1) adds to dW; db_dev may be NULL and is overwritten otherwise.  The rows are cut into ns_gemm_wgrad_splits slices, a pure
 * function of (rows, N, K) -- not of the device -- that is 1 for rows <= 1024; each workgroup reduces one slice for one output
 * tile.  With one split dW and db are written directly; otherwise the partial tiles go to workspace_dev (at least
 * ns_gemm_wgrad_workspace_bytes(rows, N, K) = splits * (N * K + N) * 4 rounded up to 256 bytes; 0 and unused with one split) and
 * a second launch sums them in split order: no floating-point atomics, the same bits on every call.                          */
int ns_gemm_wgrad_splits(int64_t rows, int N, int K);
int64_t ns_gemm_wgrad_workspace_bytes(int64_t rows, int N, int K);
int ns_gemm_wgrad(const float* dy_dev, int64_t dy_row_stride, int64_t dy_col_stride, const float* x_dev,
                  int64_t x_row_stride, int64_t rows, int N, int K, float* dW_dev, int64_t ldw, int accumulate,
                  float* db_dev, void* workspace_dev, void* stream);
/* Tall GEMM of the field fit: the layer forwards and the grad-input products over rows = rays x samples,
 *   C[i*ldc + j] (+)= sum_k A[i*lda + k] * B[j*sb0 + k*sb1] (+ bias[j]),  then act, then dact (both as in ns_gemm_fused)
 * for i < rows in [1, 2^31), j < N <= 512, k < K <= 512 (larger N or K: NS_E_UNSUPPORTED); A is contiguous along k with
 * lda >= K, ldc >= N, and dact_ref_dev[i*ld_ref + j] (ld_ref >= N) is read when dact != 0.  A, C and dact_ref may be column
 * slices of wider buffers (4-byte alignment is all that is asked); B is W (sb1 == 1, a forward layer) or the W^T view
 * (sb0 == 1, grad-input).  One workgroup owns 128 rows and all N columns, so a row of A is fetched once; B is re-read per
 * slab through L2 and LDS.  The order of the sum over k depends on K alone: the same bits on every call, no atomics.      */
int ns_gemm_tall(const float* A_dev, int64_t lda, const float* B_dev, int64_t sb0, int64_t sb1,
                 const float* bias_dev, float* C_dev, int64_t ldc, int64_t rows, int N, int K, int accumulate,
                 int act, int dact, const float* dact_ref_dev, int64_t ld_ref, void* stream);
/* activations in place: act 0 none, 1 ReLU, 2 LeakyReLU(0.01), 3 sigmoid; backward scales dy by act'(.)
 * evaluated from the activation OUTPUT y                                                            */
int ns_act_forward(float* y_dev, int64_t n, int act, void* stream);
int ns_act_backward(float* dy_dev, const float* y_dev, int64_t n, int act, void* stream);
/* gradient of Embedder.embed w.r.t. its input: x [M,d], de [M,d(1+2L)] -> dx [M,d] */
int ns_posenc_backward(const float* x_dev, const float* de_dev, int64_t M, int d, int n_freqs,
                       float* dx_dev, void* stream);
/* gradient of pts = o + d*z w.r.t. z: dpts [R,N,3], d [R,3] -> dz [R,N] */
int ns_points_backward(const float* dpts_dev, const float* d_dev, int64_t R, int N, float* dz_dev,
                       void* stream);
/* torch.optim.Adam update (no weight decay / amsgrad), step counted from 1 */
int ns_adam_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr,
                 float beta1, float beta2, float eps, int step, void* stream);
/* the same update with the step count read from *step_dev (>= 1) and, when lr_dev is not NULL, the learning rate from
 * *lr_dev: nothing in the launch changes from step to step, so a captured hipGraph of the whole training step
 * (forward, backward, update) can be replayed; ns_add_i32 advances the counter on the stream                       */
int ns_adam_step_dev(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr,
                     const float* lr_dev, float beta1, float beta2, float eps, const int* step_dev,
                     void* stream);
int ns_add_i32(int* x_dev, int delta, void* stream);
/* ns_adam_step_dev for EVERY parameter tensor of the optimiser in one launch: table_dev = n_tensors rows {p, g, m, v, n}
 * in device memory, max_n = the largest n (82 launches per DepthNet step become one)                                  */
typedef struct ns_adam_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} ns_adam_tensor;
int ns_adam_step_multi_dev(const ns_adam_tensor* table_dev, int n_tensors, int64_t max_n, float lr,
                           const float* lr_dev, float beta1, float beta2, float eps, const int* step_dev,
                           void* stream);

/* ---- timing helpers (hipEvent_t as void*) used by bench.py for the live roofline figure --------- */
int ns_event_create(void** ev);
void ns_event_destroy(void* ev);
int ns_event_record(void* ev, void* stream);
/* work submitted to `stream` after this call waits for `ev` (hipStreamWaitEvent): lets a copy stream start a frame
 * chunk's device-to-host copies exactly when the NEXT chunk's NeRF-MLP kernel starts (ev = its ev_mlp_begin)      */
int ns_stream_wait_event(void* stream, void* ev);
/* milliseconds between two recorded events; blocks until `end` has completed */
int ns_event_elapsed_ms(void* begin, void* end, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* NERF_SAMPLING_HIP_H */
