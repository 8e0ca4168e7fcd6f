/*
 * mvip_nerf.h — C ABI of libmvipnerf.so, the MI355X (gfx950) implementation of MVIP-NeRF's
 * volume-rendering + SDS hot path.
 *
 * The reference has no FFI on this path (it is stock PyTorch ops called from Python, SURVEY.md
 * §8b), so each entry point below names the reference Python call site it replaces
 * (paths relative to the reference checkout).  A maintainer binds these with ctypes; the binding
 * is shown in INTEGRATION.md and shipped in mvip_nerf_amd/_lib.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless the name ends in _host or the type
 *     says otherwise; tensors are dense row-major with the shapes given in the comments;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued
 *     on it, nothing synchronises, nothing allocates, no global mutable state: re-entrant per
 *     stream and capturable into a hipGraph;
 *   - return value: MVIP_OK (0) or a negative MVIP_E* code; mvip_strerror() names it.  Launch
 *     errors are read back with hipGetLastError() and reported as MVIP_ELAUNCH.
 *   - "nullable" arguments switch an optional input/output off.
 */
#ifndef MVIP_NERF_H
#define MVIP_NERF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVIP_OK        0
#define MVIP_EINVAL   -1   /* bad size / null pointer / unsupported configuration */
#define MVIP_ELAUNCH  -2   /* hipLaunch / runtime error (see mvip_last_hip_error) */
#define MVIP_EUNSUP   -3   /* shape outside what the kernels are built for */

#define MVIP_ABI_VERSION 5      /* 2: `prec` on the SDS operand producers / contractions, operand-sink entry points;
                                   3: prec = 2 (two products for fp16-exact weights), mvip_packed_weights_two_product,
                                      mvip_build_is_experiment;
                                   4: mvip_mlp_*_f16x3_w16 (two-waves-per-SIMD split-precision forward) added,
                                      mvip_mlp_forward_rays16_persistent removed;
                                   5: LayerNorm statistics from the producing GEMM's epilogue (mvip_gemm_ln_segments,
                                      mvip_gemm_f16x3_ws_ln, mvip_layernorm_split_planes_stats), GroupNorm moments
                                      from the unsplit convolution's epilogue (mvip_conv3x3_f16x3_tile_moments) */

int         mvip_abi_version(void);
int         mvip_build_is_experiment(void); /* 1: compiled with a -DMVIP_EXPERIMENT_* macro (timing build, WRONG results) */
const char *mvip_strerror(int code);
const char *mvip_last_hip_error(void);      /* text of the last HIP error seen by this thread */
int         mvip_device_info(int *n_cu, int *lds_bytes, char *arch_out, int arch_cap);

/* ------------------------------------------------------------------------------------------
 * a1  get_rays                         DS_NeRF/run_nerf_helpers.py:249-260
 * c2w [3,4].  Writes the (y0..y0+h, x0..x0+w) window of the H x W frame (the `patch` crop of
 * DS_NeRF/run.py:1174-1177; pass 0,0,H,W for the full frame): rays_o, rays_d [h,w,3].
 */
int mvip_get_rays(const float *c2w, int H, int W, float focal, int y0, int x0, int h, int w,
                  float *rays_o, float *rays_d, void *stream);

/* a2  ray-row assembly of render()     DS_NeRF/run.py:1182-1207
 * rays_o, rays_d [B,3] -> rows [B,11] = (o, d, near, far, d/|d|).  viewdirs_src nullable: when
 * given ([B,3]) viewdirs come from it instead of rays_d (the c2w_staticcam case, run.py:1185). */
int mvip_ray_rows(const float *rays_o, const float *rays_d, const float *viewdirs_src,
                  float near, float far, int64_t B, float *rows, void *stream);

/* a1+a2 fused: rows straight from a pose; selects pixels by an optional int64 index list
 * (`sel` [B] flat y*W+x indices, nullable -> all H*W pixels in raster order).  Replaces
 * get_rays + the masked gather of DS_NeRF/run.py:869-884 + the row assembly. */
int mvip_ray_rows_from_pose(const float *c2w, int H, int W, float focal, float near, float far,
                            const int64_t *sel, int64_t B, float *rows, void *stream);

/* a3  stratified depths                DS_NeRF/run.py:1759-1781
 * rows [B,ncols] (near, far in columns 6,7); t_vals [S] = torch.linspace(0,1,S) (passed in so
 * it is bit-identical to torch's); t_rand [B,S] uniforms, nullable (perturb == 0). z [B,S]. */
int mvip_stratified_z(const float *rows, int ncols, int64_t B, int S, const float *t_vals,
                      int lindisp, const float *t_rand, float *z, void *stream);

/* a4  Embedder.embed                   DS_NeRF/run_nerf_helpers.py:22-52
 * x [N,3] -> y [N, 3+6L]  (x, then per octave: sin(x*2^k) xyz, cos(x*2^k) xyz). */
int mvip_posenc(const float *x, int64_t N, int L, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * a5/a6  NeRF.forward behind run_network   DS_NeRF/run_nerf_helpers.py:104-127, run.py:1108-1124
 *
 * The 8x256 MLP (D=8, W=256, skip at 4, 63+27 encoded inputs, use_viewdirs) evaluated by ONE
 * kernel per call: encoding, all 11 linear layers and the activations stay on chip; weights are
 * streamed from a packed image (2.3 MB) through LDS.
 *
 * mvip_mlp_packed_floats(): size of the packed image in floats.
 * mvip_mlp_pack(): params_host is a HOST array of 24 device pointers in state-dict order
 *   pts_linears.{0..7}.{weight,bias}, views_linears.0.{weight,bias}, feature_linear.{weight,bias},
 *   alpha_linear.{weight,bias}, rgb_linear.{weight,bias}   (run_nerf_helpers.py:86-100).
 * mvip_mlp_unpack_grads(): the inverse mapping (packed-layout image -> 24 tensors).
 */
int64_t mvip_mlp_packed_floats(void);
int mvip_mlp_pack(const float *const *params_host, float *packed, void *stream);
/* image for precision 1; packed_f32 = the image mvip_mlp_pack() wrote for the same parameters
 * (its fp32 bias / head section is shared). */
int mvip_mlp_pack_f16x3(const float *const *params_host, float *image, const float *packed_f32,
                        void *stream);
int mvip_mlp_forward_rays_f16x3(const float *image, const float *rows, const float *z, int64_t B, int S,
                                float *raw, void *stream);
int mvip_mlp_forward_points_f16x3(const float *image, const float *pts, const float *dirs, int64_t P,
                                  float *raw, void *stream);

/* Round 5: the split-precision forward with TWO waves per SIMD (csrc/mlp_fwd16_f16x3.hip: 16 points per wave on
 * v_mfma_f32_16x16x32_f16, one weight ring per 8-wave workgroup) -- the kernel behind NeRF.forward under no_grad at
 * inference_precision = 1 (run_network, DS_NeRF/run.py:1108-1124; DS_NeRF/run_nerf_helpers.py:104-127).  Its own image
 * (mvip_mlp_packed_floats() floats: fp16 hi / lo A fragments in 16x16x32 order + section B of the fp32 image); values equal
 * mvip_mlp_forward_*_f16x3's up to fp32 summation order.  Forward only. */
int mvip_mlp_pack_f16x3_w16(const float *const *params_host, const float *packed_f32, float *image, void *stream);
int mvip_mlp_forward_rays_f16x3_w16(const float *image, const float *rows, const float *z, int64_t B, int S,
                                    float *raw, void *stream);
int mvip_mlp_forward_points_f16x3_w16(const float *image, const float *pts, const float *dirs, int64_t P,
                                      float *raw, void *stream);
/* ... and its stash-writing TRAINING form (train_precision = 1): raw + the activation stash of mvip_mlp_stash_floats(B*S) floats
 * that mvip_mlp_backward_stash(precision = 1) consumes (same layout and values as mvip_mlp_forward_rays_stash(precision = 1) writes,
 * up to fp32 summation order).  Renders under loss.backward(), DS_NeRF/run.py:948-974, :1030. */
int mvip_mlp_forward_rays_stash_f16x3_w16(const float *image, const float *rows, const float *z, int64_t B, int S,
                                          float *raw, float *stash, void *stream);

/* Forward from geometry: rows [B,11], z [B,S] -> raw [B,S,4]; points are o + d*z, view dirs
 * are rows[:,8:11] (run.py:1783, :1787).
 * precision 0: exact fp32 MFMA, `packed` from mvip_mlp_pack().
 * precision 1: "f16x3" split precision -- fp16 MFMA on W = Wh+Wl, X = Xh+Xl with the three leading
 *   products (Wh.Xh + Wh.Xl + Wl.Xh) accumulated in fp32; `packed` must be the image written by
 *   mvip_mlp_pack_f16x3() (same size).  Forward only; ~1e-6 relative deviation from precision 0. */
int mvip_mlp_forward_rays(const float *packed, const float *rows, const float *z, int64_t B, int S,
                          float *raw, int precision, void *stream);

/* Forward from explicit points: pts [P,3], dirs [P,3] (already normalised) -> raw [P,4]; this is
 * network_query_fn / run_network for arbitrary inputs (run.py:1530-1533). */
int mvip_mlp_forward_points(const float *packed, const float *pts, const float *dirs, int64_t P,
                            float *raw, int precision, void *stream);

/* Inference-only forward with two waves per SIMD (csrc/mlp_fwd16.hip): 16 points per wave on
 * v_mfma_f32_16x16x4_f32, exact fp32, same results to rounding as mvip_mlp_forward_* with precision 0.
 * packed16 (mvip_mlp_packed_floats() floats) = the same weights in the 16-point block order, built from the 24
 * parameter tensors and the small-vector section of an up-to-date mvip_mlp_pack image. */
int mvip_mlp_pack16(const float *const *params_host, const float *packed, float *packed16, void *stream);
int mvip_mlp_forward_rays16(const float *packed16, const float *rows, const float *z, int64_t B, int S,
                            float *raw, void *stream);
int mvip_mlp_forward_points16(const float *packed16, const float *pts, const float *dirs, int64_t P,
                              float *raw, void *stream);
/* Test probe of the 16-point kernels' input encoding: pts, dirs [P,3] -> out_old, out_new [P,96] (64 position channels,
 * then 32 direction channels, zero padded), by the per-channel reference route and by the once-per-wave route the kernels run. */
int mvip_mlp_encode16_probe(const float *pts, const float *dirs, int64_t P, float *out_old, float *out_new, void *stream);

/* Folded inference image (ops.mlp_pack16 / NeRF.packed_w16, NeRF.fold_feature_inference): feature_linear has no
 * activation, so a no-grad forward evaluates the view layer as relu(W' h + Wv[:, 256:] e_dir + b') with
 * W' = Wv[:, :256] Wf and b' = Wv[:, :256] bf + bv and skips the feature layer (11 % of the matrix work).  sigma is
 * bit-identical to the unfolded entries, rgb equal to rounding.
 * mvip_mlp_packed_fold_floats(): size of the EXTENDED image = [the mvip_mlp_pack16 image, unchanged | folded view blocks |
 *   a copy of the small-vector section carrying b'].  Its head drives every entry that takes a plain packed16.
 * mvip_mlp_fold_pack16(): fills the tail of an extended image whose head mvip_mlp_pack16 has written on the same
 *   stream; W' and b' are accumulated in fp64 in a fixed order and rounded once (deterministic, identical on every rank).
 * mvip_*_fold: the four inference launches on an extended image; arguments as their unfolded twins. */
int64_t mvip_mlp_packed_fold_floats(void);
int mvip_mlp_fold_pack16(const float *const *params_host, float *packed16_ext, void *stream);
int mvip_mlp_forward_rays16_fold(const float *packed16_ext, const float *rows, const float *z, int64_t B, int S,
                                 float *raw, void *stream);
int mvip_mlp_forward_points16_fold(const float *packed16_ext, const float *pts, const float *dirs, int64_t P,
                                   float *raw, void *stream);

/* ------------------------------------------------------------------------------------------
 * a10 (row g)  render_rays as TWO launches per chunk (DS_NeRF/run.py:1703-1847), no-grad renders of the native 8x256
 * networks with 64 coarse + <= 64 fine samples: the same device functions as the stand-alone entry points, fused behind
 * the network so that no raw / weights / depth tensor of the coarse pass and no z tensor of its samples ever exists.
 * Every output is BIT-IDENTICAL to the unfused chain (tests/test_render.py).
 * mvip_render_coarse_fused: rows [B,11] -> stratified depths (t_vals [64] = linspace(0,1,64); t_rand [B,64] or NULL) ->
 *   coarse network (packed16 of mvip_mlp_pack16) -> raw2outputs (noise [B,64] or NULL; flags MVIP_COMP_*) ->
 *   inverse-CDF resampling with Nf <= 64 uniforms (u [B,Nf], or one row of Nf when u_is_row) -> sort(cat[z, z_samples]).
 *   Outputs rgb0 [B,3], disp0 [B], acc0 [B], z_merged [B,64+Nf], z_std [B]; depth0 [B], weights0 [B,64], alpha0 [B,64]
 *   optional (NULL = not wanted).
 * mvip_render_fine_fused: network at the 128 depths z [B,128] -> raw2outputs; outputs as mvip_composite_forward plus
 *   raw [B,128,4] (NULL = not wanted), alpha optional. */
int mvip_render_coarse_fused(const float *packed16, const float *rows, int64_t B, const float *t_vals, int lindisp,
                             const float *t_rand, const float *noise, const float *u, int u_is_row, int Nf, int flags,
                             float *rgb0, float *disp0, float *acc0, float *depth0, float *weights0, float *alpha0,
                             float *z_merged, float *z_std, void *stream);
int mvip_render_fine_fused(const float *packed16, const float *rows, const float *z, int64_t B, const float *noise,
                           int flags, float *raw, float *rgb, float *disp, float *acc, float *depth, float *weights,
                           float *alpha, void *stream);
/* the same two launches with the folded network (run.py render_rays when NeRF.fold_feature_inference); packed16_ext is an
 * extended image with its tail filled (mvip_mlp_fold_pack16) */
int mvip_render_coarse_fused_fold(const float *packed16_ext, const float *rows, int64_t B, const float *t_vals, int lindisp,
                                  const float *t_rand, const float *noise, const float *u, int u_is_row, int Nf, int flags,
                                  float *rgb0, float *disp0, float *acc0, float *depth0, float *weights0, float *alpha0,
                                  float *z_merged, float *z_std, void *stream);
int mvip_render_fine_fused_fold(const float *packed16_ext, const float *rows, const float *z, int64_t B, const float *noise,
                                int flags, float *raw, float *rgb, float *disp, float *acc, float *depth, float *weights,
                                float *alpha, void *stream);

/* Backward: d_raw [P,4] -> the 24 parameter gradients.  grads_host is a HOST array of 24 device
 * pointers (state-dict order, natural [out][in] shapes) that are ACCUMULATED into with fp32
 * atomics (zero them, or pass .grad buffers).  Inputs are re-encoded and activations recomputed
 * on chip in tiles of `tile_points` (>=128); `workspace` must hold
 * mvip_mlp_backward_workspace_bytes(tile_points) bytes.  Gradients w.r.t. pts/dirs are not
 * produced (the reference never needs them: SURVEY.md 8b "Autograd"). */
int64_t mvip_mlp_backward_workspace_bytes(int64_t tile_points);
int mvip_mlp_backward_rays(const float *packed, const float *rows, const float *z, int64_t B, int S,
                           const float *d_raw, float *const *grads_host, void *workspace,
                           int64_t tile_points, int precision, void *stream);
int mvip_mlp_backward_points(const float *packed, const float *pts, const float *dirs, int64_t P,
                             const float *d_raw, float *const *grads_host, void *workspace,
                             int64_t tile_points, int precision, void *stream);
/* Training fast path: the forward also writes every activation to `stash`
 * (mvip_mlp_stash_floats(P) floats, ~9.9 KB per point) and the backward consumes it instead of
 * recomputing -- 2.9 instead of 3.9 forward-equivalents per training step when HBM has room
 * (288 GB: a 2.6 M-point step needs 26 GB). */
int64_t mvip_mlp_stash_floats(int64_t P);
int mvip_mlp_forward_rays_stash(const float *packed, const float *rows, const float *z, int64_t B,
                                int S, float *raw, float *stash, int precision, void *stream);
int mvip_mlp_forward_points_stash(const float *packed, const float *pts, const float *dirs, int64_t P,
                                  float *raw, float *stash, int precision, void *stream);
/* mvip_mlp_forward_rays_stash (precision 0) on the two-waves-per-SIMD kernel: `packed16` from mvip_mlp_pack16, the
 * stash layout and size are the same, so mvip_mlp_backward_stash (given the 32-point `packed` image) consumes it. */
int mvip_mlp_forward_rays_stash16(const float *packed16, const float *rows, const float *z, int64_t B, int S,
                                  float *raw, float *stash, void *stream);
int mvip_mlp_backward_stash(const float *packed, const float *stash, int64_t P, const float *d_raw,
                            float *const *grads_host, void *workspace, int64_t tile_points,
                            int precision, void *stream);
/* packed-layout image -> 24 tensors (inverse of mvip_mlp_pack; += when accumulate != 0). */
int mvip_mlp_unpack_grads(const float *grad_packed, float *const *grads_host, int accumulate,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * a7  raw2outputs                      DS_NeRF/run_nerf_helpers.py:350-404
 * raw [B,S,4], z [B,S], rows [B,ncols] (direction in columns 3..5), noise [B,S] nullable
 * (already multiplied by raw_noise_std).  Outputs: rgb [B,3], disp/acc/depth [B], weights [B,S],
 * alpha [B,S] nullable.  flags: bit0 white_bkgd.
 */
#define MVIP_COMP_WHITE   1
#define MVIP_COMP_DETACHW 2   /* detach_weights: no gradient from rgb_map into the weights */
int mvip_composite_forward(const float *raw, const float *z, const float *rows, int ncols,
                           const float *noise, int64_t B, int S, int flags, float *rgb, float *disp,
                           float *acc, float *depth, float *weights, float *alpha, void *stream);
/* Backward of the above.  Upstream gradients (each nullable = zero): g_rgb [B,3], g_disp, g_acc,
 * g_depth [B], g_weights [B,S], g_alpha [B,S].  Output d_raw [B,S,4]. */
int mvip_composite_backward(const float *raw, const float *z, const float *rows, int ncols,
                            const float *noise, int64_t B, int S, int flags, const float *g_rgb,
                            const float *g_disp, const float *g_acc, const float *g_depth,
                            const float *g_weights, const float *g_alpha, float *d_raw, void *stream);

/* a8+a9  sample_pdf + sort(cat)        DS_NeRF/run_nerf_helpers.py:304-347, run.py:1809-1816, :1836
 * z [B,Nc] coarse depths, weights [B,Nc] coarse weights (the kernel forms the Nc-1 midpoints
 * and uses weights[:,1:-1] itself), u [B,Nf] uniforms or, when u_is_row != 0, one row [Nf]
 * shared by all rays (det: torch.linspace(0,1,Nf)).  Outputs: z_samples [B,Nf], z_merged
 * [B,Nc+Nf] ascending, z_std [B] (population std of z_samples), inds int64 [B,Nf] nullable
 * (= #{cdf <= u}, searchsorted right=True), cdf [B,Nc-1] nullable.
 * z_std contract: two-pass (mean, then squared deviations) fp32 wave-tree sums; 1/Nf and the square root are
 * v_rcp_f32 / v_sqrt_f32 (<= 1 ulp each, 1/Nf exact for powers of two): within 3e-6 relative of
 * torch.std(z_samples, -1, unbiased=False) evaluated in fp64, not correctly rounded
 * (tests/test_hip_kernels.py::test_z_std_contract_non_power_of_two).
 * Nc = Nf = 64 (the reference configuration) runs two rays per wavefront; every output equals the one-ray-per-wavefront
 * kernel's bit for bit (a NaN equals a NaN), also for rows with NaN / negative / unsorted entries, which take the general route
 * (MVIP_SAMPLE_PAIR=0 selects the one-ray kernel for A/B; tests/test_hip_kernels.py::test_rays_per_wave_routes_are_bit_identical). */
int mvip_sample_pdf_merge(const float *z, const float *weights, const float *u, int u_is_row,
                          int64_t B, int Nc, int Nf, float *z_samples, float *z_merged,
                          float *z_std, int64_t *inds, float *cdf, void *stream);
/* Standalone sample_pdf for arbitrary bins/weights (bins [B,Nb], weights [B,Nb-1]). */
int mvip_sample_pdf(const float *bins, const float *weights, const float *u, int u_is_row,
                    int64_t B, int Nb, int Nf, float *samples, int64_t *inds, float *cdf,
                    void *stream);

/* ------------------------------------------------------------------------------------------
 * a12  depth2xyz_torch                 DS_NeRF/run.py:1909-1922
 * depth [H,W] -> points [H,W,3]: x=(w-cx)*z/fx, y=(h-cy)*z/fy, z.  Backward: g_points -> d_depth. */
int mvip_depth2xyz(const float *depth, int H, int W, float fx, float fy, float cx, float cy,
                   float *points, void *stream);
int mvip_depth2xyz_backward(const float *g_points, int H, int W, float fx, float fy, float cx,
                            float cy, float *d_depth, void *stream);

/* a12  depth2normal_geo                DS_NeRF/run.py:1924-1940
 * points PLANAR [3,H,W]; k odd window (31).  normals [3,H,W]: n = (A^T A)^-1 A^T 1 over the
 * zero-padded k x k window.  `moments` [9,H,W] receives the window sums (kept for the backward);
 * `scratch` is [9,H,W] for the forward and [18,H,W] for the backward. */
int mvip_normal_fit_forward(const float *points, int H, int W, int k, float *moments, float *scratch,
                            float *normals, void *stream);
int mvip_normal_fit_backward(const float *points, const float *moments, const float *normals,
                             const float *g_normals, int H, int W, int k, float *scratch,
                             float *d_points, void *stream);

/* ------------------------------------------------------------------------------------------
 * a13/a14  elementwise core of the SDS step   DS_NeRF/guidance/sd_utils.py:406-413, :29-37
 * latents = sqrt(abar)*x0 + sqrt(1-abar)*noise                       (scheduler.add_noise)
 * grad    = nan_to_num((1-abar) * (e_u + s*(e_c - e_u) - noise))     (CFG + SDS weight)
 * all [n] fp32. */
int mvip_sds_add_noise(const float *x0, const float *noise, float sqrt_abar, float sqrt_1m_abar,
                       int64_t n, float *latents, void *stream);
int mvip_sds_grad(const float *eps_uncond, const float *eps_cond, const float *noise,
                  float guidance_scale, float w, int64_t n, int accumulate, float *grad,
                  void *stream);

/* Posterior sample of the VAE encoder and its adjoint (the pipeline's _encode_vae_image: scaling_factor *
 * latent_dist.sample(), reached from DS_NeRF/guidance/sd_utils.py:207): moments [N][2C][HW] = (mean | logvar),
 * noise / out / d_out [N][C][HW], d_moments [N][2C][HW];  out = sf * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise).
 * One launch each instead of the ~7 / ~15 elementwise launches of the torch expression and its autograd backward. */
int mvip_vae_sample(const float *moments, const float *noise, float scaling_factor, int64_t N, int64_t C,
                    int64_t HW, float *out, void *stream);
int mvip_vae_sample_backward(const float *moments, const float *noise, const float *d_out, float scaling_factor,
                             int64_t N, int64_t C, int64_t HW, float *d_moments, void *stream);

/* Sinusoidal timestep embedding in front of the UNet's time MLP (diffusers get_timestep_embedding with
 * flip_sin_to_cos=True; the unet(...) call of DS_NeRF/guidance/sd_utils.py:390-403): out [N][2 half] =
 * (cos(t_n f_k) | sin(t_n f_k)), t [N] on the device (graph-replayable), freqs [half] computed once by the caller. */
int mvip_timestep_sincos(const float *t, const float *freqs, int64_t N, int64_t half, float *out, void *stream);

/* The same two kernels with the timestep-dependent scalars read from device memory
 * (scal = {sqrt(abar), sqrt(1-abar), 1-abar}), so that ONE captured hipGraph of the SDS step
 * serves every timestep. */
int mvip_sds_add_noise_dev(const float *x0, const float *noise, const float *scal, int64_t n,
                           float *latents, void *stream);
int mvip_sds_grad_dev(const float *eps_uncond, const float *eps_cond, const float *noise,
                      float guidance_scale, const float *scal, int64_t n, int accumulate, float *grad,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * The 2D inpainting sampler of the prior (StableDiffusion.produce_latents / decode_latents / prompt_to_img,
 * DS_NeRF/guidance/sd_utils.py:602-666, and the inpaint preview built on the SDS step's conditioning).
 *
 * Decoder head: conv_norm_out -> SiLU -> conv_out of AutoencoderKL's decoder plus decode_latents' post-processing
 * (DS_NeRF/guidance/sd_utils.py:624-631) in one launch:
 *   img[n,o,y,x] = clamp((conv3x3(silu(gamma[c] (x - mean[n,g]) rstd[n,g] + beta[c]), weight)[o] + bias[o]) / 2 + 0.5, 0, 1)
 * x [N, C, H, W] (dtype 0 = fp32, 1 = fp16 storage), mean / rstd [N, G] from mvip_groupnorm_stats, gamma / beta [C],
 * weight [3, C, 3, 3], bias [3]; stride 1, zero padding 1 of the ACTIVATED input.  img [N, 3, H, W] fp32; img_u8
 * (nullable) [N, H, W, 3] = rint(255 img), round half to even (prompt_to_img's `.round()`).  prec 0 / 2: fp32 products;
 * 1: the reference's --fp16 mode (activations and weights rounded to fp16, fp32 sums).  C % 32 == 0, C % G == 0,
 * any H, W >= 1 (H * W <= 2^27). */
int mvip_vae_decoder_head(const void *x, const float *mean, const float *rstd, const float *gamma, const float *beta,
                          const float *weight, const float *bias, int64_t N, int64_t C, int64_t H, int64_t W, int G,
                          int dtype, float *img, uint8_t *img_u8, int prec, void *stream);
/* One DDIM update, eta = 0 (the scheduler.step of produce_latents, DS_NeRF/guidance/sd_utils.py:617-620), with the
 * classifier-free guidance in front of it (:613-614).  eps [2, 4, hw] = (uncond, cond) when cfg, else [1, 4, hw];
 * x [1, 4, hw] updated in place; scal (device) = {g, sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev),
 * t_next}:  e = e_u + g (e_c - e_u);  x <- sqrt(abar_prev) (x - sqrt(1 - abar_t) e) / sqrt(abar_t) + sqrt(1 - abar_prev) e.
 * unet_in (nullable) [1 + cfg, in_ch, hw]: channels 0..3 of every batch entry receive the new x (the next UNet input,
 * whose mask / masked-image channels the caller wrote once); t_out (nullable): one float, receives t_next. */
int mvip_ddim_cfg_step(const float *eps, int cfg, const float *scal, float *x, int64_t hw, float *unet_in,
                       int64_t in_ch, float *t_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * a14-a16  bilinear resize, align_corners = False: F.interpolate(pred_rgb, (512, 512), mode='bilinear') in front of
 * vae.encode (DS_NeRF/guidance/sd_utils.py:282-284, :449-452) and its adjoint.  x [planes, H, W] -> y [planes, OH, OW]
 * with torch's source-index convention (scale = in/out, src = scale*(dst+0.5)-0.5 clamped at 0); the backward gathers
 * (deterministic), dx [planes, H, W] = J^T dy. */
int mvip_resize_bilinear(const float *x, int64_t planes, int64_t H, int64_t W, int64_t OH, int64_t OW, float *y,
                         void *stream);
int mvip_resize_bilinear_backward(const float *dy, int64_t planes, int64_t H, int64_t W, int64_t OH, int64_t OW,
                                  float *dx, void *stream);

/* ------------------------------------------------------------------------------------------
 * a14-a16  GroupNorm (+ fused SiLU) of the SDS networks: the `norm -> silu -> conv` prologue of every
 * ResNet block inside vae.encode / unet (call sites DS_NeRF/guidance/sd_utils.py:148, :162, :189,
 * :212; the blocks themselves live in `diffusers`, absent from the reference tree -- published
 * SD-1.5 architecture, parity checked against torch.nn.functional.group_norm in fp32).
 * x, y, dy, dx: [N, C, HW] contiguous (NCHW); gamma, beta: [C] or NULL; dtype 0 = fp32, 1 = fp16
 * (storage type of x/y/dy/dx/gamma/beta; arithmetic fp32, statistics fp64).
 *   forward : y = act((x - mean_g) * rstd_g * gamma[c] + beta[c]),  act = SiLU if `silu` else identity;
 *             mean, rstd [N, G] fp32 are written for the backward.
 *   backward: dx only (the SDS networks are frozen; gradients flow to the rendered image).
 * workspace: mvip_groupnorm_workspace_bytes(N, C, HW) bytes, 16-byte aligned. */
int64_t mvip_groupnorm_workspace_bytes(int64_t N, int64_t C, int64_t HW);
int mvip_groupnorm_forward(const void *x, const void *gamma, const void *beta, int64_t N, int64_t C,
                           int64_t HW, int G, float eps, int silu, int dtype, void *y, float *mean,
                           float *rstd, void *workspace, void *stream);
int mvip_groupnorm_backward(const void *x, const void *dy, const void *gamma, const void *beta,
                            const float *mean, const float *rstd, int64_t N, int64_t C, int64_t HW, int G,
                            int silu, int dtype, void *dx, void *workspace, void *stream);
/* The same backward with the two passes that used to follow it folded in (the VAE encoder's data-gradient chain,
 * vae.encode under autograd at DS_NeRF/guidance/sd_utils.py:207): dx = backward(...) + dx_add (dx_add [N, C, HW] or NULL: the
 * gradient arriving over a ResNet block's identity shortcut, which autograd would add in a separate pass), and
 * maxima[mvip_groupnorm_backward_maxima(N, C, HW)] (or NULL) receives one max|dx| per workgroup (plain stores; NaN / Inf
 * skipped as mvip_absmax_scale skips them).  mvip_absmax_scale_from_maxima turns them into the scale2 = {s, 1/s} that
 * mvip_absmax_scale(dx) would compute -- the same power of two, without re-reading dx. */
int64_t mvip_groupnorm_backward_maxima(int64_t N, int64_t C, int64_t HW);
int mvip_groupnorm_backward_fused(const void *x, const void *dy, const void *gamma, const void *beta,
                                  const float *mean, const float *rstd, int64_t N, int64_t C, int64_t HW, int G,
                                  int silu, int dtype, const void *dx_add, void *dx, float *maxima, void *workspace,
                                  void *stream);
int mvip_absmax_scale_from_maxima(const float *maxima, int64_t count, float *scale2, void *stream);
/* statistics only (mean, rstd [N, G]); the normalised tensor is then produced by another kernel.  mean == rstd == NULL:
 * only the fp64 moment partials are left in `workspace`, for mvip_groupnorm_split_planes_moments. */
int mvip_groupnorm_stats(const void *x, int64_t N, int64_t C, int64_t HW, int G, float eps, int dtype,
                         float *mean, float *rstd, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * a14-a16  3x3 / stride 1 / pad 1 convolution of the SDS networks (the ResNet-block convolutions inside
 * vae.encode / unet: DS_NeRF/guidance/sd_utils.py:148, :162, :189, :212; layers from the published SD-1.5
 * architecture) as an implicit GEMM on the fp16 matrix cores in split precision: both operands are
 * split into fp16 hi + lo terms and Wh.Xh + Wh.Xl + Wl.Xh is accumulated in fp32 (~1e-6 relative).
 *
 * Activations travel in "split planes": xs[N][Cin/16][2][2][H][W][8] fp16 (N*Cin*H*W*4 bytes), written
 * by mvip_groupnorm_split_planes (GroupNorm + optional SiLU fused) or mvip_split_planes (x * scale2[0]).
 * Weights are packed once per layer by mvip_conv3x3_pack into mvip_conv3x3_packed_bytes(Cout, Cin)
 * bytes; transpose = 1 packs the data-gradient operator (then the conv maps dY [N,Cout,H,W] -> dX
 * [N,Cin,H,W]: call mvip_conv3x3_f16x3 with Cin and Cout swapped).
 * scale2 = {s, 1/s, scratch, scratch} (device, 16 bytes): power-of-two scale from the absolute maximum
 * (mvip_absmax_scale; zero_words2 nullable: two caller-owned 32-bit scratch words, zero on entry and on exit, make it
 * ONE launch -- maximum by atomics, the last workgroup writes the scale -- instead of zero + reduce + scale).
 *   y[n,co,h,w] = conv(x, W)[n,co,h,w] / (s_w s_x) + bias[co] + chan_add[n,co] + residual[n,co,h,w]
 * (bias, chan_add, residual, x_scale2 may be NULL).  Supported: Cout % 32 == 0, Cin % 16 == 0,
 * (H % 8 == 0 and W % 32 == 0) or (H % 16 == 0 and W % 16 == 0) or H == W == 8 (mvip_conv3x3_supported); anything
 * else returns MVIP_EINVAL.
 * mvip_conv3x3_f16x3_ws takes a caller-owned workspace of mvip_conv3x3_workspace_bytes(N, Cin, Cout, H, W) bytes (0 for
 * most shapes; workspace may then be NULL): layers whose (pixel tile, 32-row block) grid would occupy a fraction of the
 * chip -- the UNet's 1280-channel levels at 16x16 and 8x8, whose weights are 59-118 MB per layer -- are split over the
 * input channels, each workgroup writing raw partial sums, and a second launch adds the splits in index order
 * (deterministic) and applies the epilogue.  Results equal mvip_conv3x3_f16x3's up to fp32 summation order. */
int mvip_conv3x3_supported(int64_t Cout, int64_t Cin, int64_t H, int64_t W);
int64_t mvip_conv3x3_packed_bytes(int64_t Cout, int64_t Cin);
int mvip_conv3x3_pack(const float *weight, int64_t Cout, int64_t Cin, int transpose, void *packed, void *stream);
/* Pack-time query (round 4): *two_product_host = 1 when every lo fragment of a packed WEIGHT image is zero, i.e. the
 * (power-of-two scaled) weights are exact fp16 values -- true for every weight the reference loads
 * (DS_NeRF/guidance/sd_utils.py:69-74: `revision="fp16"`, cast up to fp32 in the default mode).  Such an image may be
 * contracted with prec = 2.  fragment_bytes = the image's size without its 256-byte tail: Cout * Cin * 36
 * (mvip_conv3x3_pack) or M * K * 4 (mvip_gemm_pack_a).  Synchronises `stream` and reads one word back: not for the step. */
int mvip_packed_weights_two_product(const void *packed, int64_t fragment_bytes, int *two_product_host, void *stream);
int mvip_absmax_scale(const float *x, int64_t n, float *scale2, void *zero_words2, void *stream);
int mvip_split_planes(const float *x, int64_t N, int64_t C, int64_t HW, const float *scale2, void *xs,
                      int prec, void *stream);
int mvip_groupnorm_split_planes(const float *x, const float *gamma, const float *beta, const float *mean,
                                const float *rstd, int64_t N, int64_t C, int64_t HW, int G, int silu, void *xs,
                                int prec, void *stream);
/* mvip_groupnorm_split_planes reading the statistics from the moment partials of mvip_groupnorm_stats(mean = rstd = NULL)
 * (`moments` = that call's workspace): every workgroup reduces the partials of the <= 5 groups its 16 channels touch in
 * the order mvip_groupnorm_stats itself uses, so the planes are bit-identical -- one launch less per GroupNorm when
 * mean / rstd are not kept for a backward.  C / G >= 4. */
int mvip_groupnorm_split_planes_moments(const float *x, const float *gamma, const float *beta, const void *moments,
                                        float eps, int64_t N, int64_t C, int64_t HW, int G, int silu, void *xs,
                                        int prec, void *stream);
/* The same, also writing mean / rstd [N, G] (the bits mvip_groupnorm_stats itself would write) for a backward that needs them
 * (vae.encode under autograd, DS_NeRF/guidance/sd_utils.py:207): no separate finalize launch in the forward (round 4). */
int mvip_groupnorm_split_planes_moments_out(const float *x, const float *gamma, const float *beta, const void *moments,
                                            float eps, int64_t N, int64_t C, int64_t HW, int G, int silu, void *xs,
                                            float *mean_out, float *rstd_out, int prec, void *stream);
int mvip_conv3x3_f16x3(const void *xs, const void *packed, const float *bias, const float *chan_add,
                       const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                       int64_t H, int64_t W, float *y, int prec, void *stream);
int64_t mvip_conv3x3_workspace_bytes(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W);
/* Channel-split launches can leave the GroupNorm moments of their OUTPUT (the norm -> silu -> conv chains of the ResNet
 * blocks): mvip_conv3x3_f16x3_ws_moments's reduction launch also writes `row_moments` [N][Cout][2] fp64 = {sum, sum of
 * squares} of every output row -- the layout mvip_groupnorm_stats(mean = rstd = NULL) leaves in its workspace for
 * H * W <= 4096, so mvip_groupnorm_split_planes_moments(y, ..., row_moments, ...) needs no pass over y for its statistics.
 * mvip_conv3x3_row_moments_doubles: N * Cout * 2 when the shape qualifies (channel-split launch; H * W = 64, 256, 1024 or
 * 4096), else 0 (then only mvip_conv3x3_f16x3_ws applies).  y is bit-identical to mvip_conv3x3_f16x3_ws's. */
int64_t mvip_conv3x3_row_moments_doubles(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W);
int mvip_conv3x3_f16x3_ws_moments(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                  const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                                  int64_t H, int64_t W, float *y, void *workspace, void *row_moments, int prec,
                                  void *stream);
/* Unsplit launches (mvip_conv3x3_workspace_bytes == 0, images wider than 8 pixels): the same moments from partials the
 * convolution's epilogue leaves per (image, channel, pixel tile, wave) -- fp32 sum and sum of squares of 64 finished values
 * about a shift (one of the 64 values, kept with them: a row whose mean is many standard deviations loses no variance to
 * the rounding of raw squares), turned into raw moments and added in fp64 in index order by a second, small launch
 * (N * Cout rows) -- instead of a pass over y (DS_NeRF/guidance/sd_utils.py:330-352,
 * :390-403: the resnet chains of the VAE encoder and the UNet).  tile_scratch: mvip_conv3x3_tile_moments_scratch_bytes(...)
 * bytes (0 = this shape cannot: use mvip_conv3x3_f16x3_ws / _ws_moments); moments: mvip_groupnorm_workspace_bytes(N, Cout,
 * H * W) bytes in mvip_groupnorm_stats' workspace layout (what mvip_groupnorm_split_planes_moments reads). */
int64_t mvip_conv3x3_tile_moments_scratch_bytes(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W);
int mvip_conv3x3_f16x3_tile_moments(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                    const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                                    int64_t H, int64_t W, float *y, void *tile_scratch, void *moments, int prec,
                                    void *stream);
int mvip_conv3x3_f16x3_ws(const void *xs, const void *packed, const float *bias, const float *chan_add,
                          const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                          int64_t H, int64_t W, float *y, void *workspace, int prec, void *stream);

/* The same split-precision machinery as a plain GEMM (1x1 convolutions and the products of the VAE
 * mid-block attention, vae.encode at DS_NeRF/guidance/sd_utils.py:207):
 *   Y[n][m][p] = sum_k A[m][k] X[n][k][p] / (s_a s_x) + bias[m] + chan_add[n][m] + residual[n][m][p]
 * A[m][k] = src[m*sm + k*sk] (src a dense block of M*K floats) is packed by mvip_gemm_pack_a into
 * mvip_gemm_packed_bytes(M, K) bytes; X travels as split planes [N][K/16][2][2][P][8], written by
 * mvip_split_planes_strided from x[n*sn + k*sc + p*sp] (times scale2[0] if given).
 * M % 32 == 0, K % 32 == 0, P % 256 == 0. */
int64_t mvip_gemm_packed_bytes(int64_t M, int64_t K);
int mvip_gemm_pack_a(const float *src, int64_t M, int64_t K, int64_t sm, int64_t sk, void *packed, void *stream);
int mvip_split_planes_strided(const float *x, int64_t N, int64_t C, int64_t HW, int64_t sn, int64_t sc, int64_t sp,
                              const float *scale2, void *xs, int prec, void *stream);
/* The same planes for the 2x nearest-neighbour up-sampled image [N][C][2H][2W] of x [N][C][H][W] (Upsample2D of the UNet:
 * F.interpolate(scale_factor=2, mode='nearest') in front of a 3x3 convolution), without materialising it. */
int mvip_split_planes_upsample2(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, const float *scale2, void *xs,
                                int prec, void *stream);
/* Row softmax P = softmax(scale * S) over the last axis of S [rows][cols] (cols <= 8192) and its adjoint
 * dS = scale * P * (dP - rowsum(dP * P)): the score matrix of AutoencoderKL's single-head mid-block attention inside
 * vae.encode (DS_NeRF/guidance/sd_utils.py:207) and its data gradient. */
int mvip_softmax_rows(const float *s, int64_t rows, int64_t cols, float scale, float *p, void *stream);
int mvip_softmax_rows_backward(const float *p, const float *dp, int64_t rows, int64_t cols, float scale, float *ds,
                               void *stream);
/* General convolution as this GEMM -- the stride-2 down-samplers of the UNet and the VAE encoder and the layers with 3,
 * 4, 8 or 9 channels (conv_in, conv_out, quant_conv; DS_NeRF/guidance/sd_utils.py:207, :240), which do not fit the 3x3
 * stride-1 kernel's operand tiles:
 *   X_col[k = ci*KH*KW + ky*KW + kx][p = oy*OW + ox] = x[n][ci][oy*stride + ky - pad_top][ox*stride + kx - pad_left]
 * is written directly as split planes [N][KP/16][2][2][PP][8] (KP >= Cin*KH*KW a multiple of 32, PP >= OH*OW a multiple
 * of 256, zero filled), so y = mvip_gemm_f16x3(xs, pack(weight as [Cout][Cin*KH*KW]), ...) with K = KP, P = PP.
 * Data gradient: col[N][KP][PP] = mvip_gemm_f16x3 with the transposed weight on dY's split planes, then
 * mvip_col2im gathers dx[n][ci][iy][ix] (deterministic). */
int mvip_im2col_split_planes(const float *x, int64_t N, int64_t Cin, int64_t H, int64_t W, int KH, int KW, int stride,
                             int pad_top, int pad_left, int64_t OH, int64_t OW, int64_t KP, int64_t PP,
                             const float *scale2, void *xs, int prec, void *stream);
int mvip_col2im(const float *col, int64_t N, int64_t Cin, int64_t H, int64_t W, int KH, int KW, int stride, int pad_top,
                int pad_left, int64_t OH, int64_t OW, int64_t KP, int64_t PP, float *dx, void *stream);
int mvip_gemm_f16x3(const void *xs, const void *packed, const float *bias, const float *chan_add,
                    const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                    float *y, int prec, void *stream);
/* The feed-forward's first projection with the GEGLU in the epilogue (the [N][2R][P] intermediate never exists):
 * out [N][R][P] = (W_v x + b_v) * gelu(W_g x + b_g) for columns < L, zero beyond; `packed` / `bias` hold the M2 = 2R
 * rows interleaved in 32-row tiles (value rows of tile t, then the gate rows of tile t); M2 % 64 == 0.  scale2 and
 * zero_word as in mvip_geglu. */
int mvip_gemm_geglu_f16x3(const void *xs, const void *packed, const float *bias, const float *x_scale2, int64_t N,
                          int64_t K, int64_t M2, int64_t P, int64_t L, float *out, float *scale2, void *zero_word,
                          int prec, void *stream);
/* the same with the workgroup tile forced (timing switch; identical arithmetic per output element up to the k order
 * inside a stage, which is the same): cfg 0 = by shape (what mvip_gemm_f16x3 does), 1 = 32/64 rows x 256 columns,
 * 2 = 128 x 256 (M % 128 == 0), 3 = 128 x 128 (M % 128 == 0), 4 = 64 x 128 (M % 64 == 0). */
int mvip_gemm_f16x3_cfg(const void *xs, const void *packed, const float *bias, const float *chan_add,
                        const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                        float *y, int cfg, int prec, void *stream);
/* mvip_gemm_f16x3 with a caller-owned workspace of mvip_gemm_workspace_bytes(N, K, M, P) bytes (0 for most shapes;
 * workspace may then be NULL): launches with fewer workgroups than CUs and a long contraction (the UNet's 1280-channel
 * transformer blocks at 16x16 and 8x8) are split over K, each workgroup writing raw partial sums, and a second launch
 * adds the splits in index order and applies the epilogue. */
int64_t mvip_gemm_workspace_bytes(int64_t N, int64_t K, int64_t M, int64_t P);
int mvip_gemm_f16x3_ws(const void *xs, const void *packed, const float *bias, const float *chan_add,
                       const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                       float *y, void *workspace, int prec, void *stream);
/* The same GEMM leaving, besides y, the LayerNorm statistics of y over its M rows (the unet(...) call,
 * DS_NeRF/guidance/sd_utils.py:390-403: BasicTransformerBlock's norm1 / norm2 / norm3 read the residual stream a
 * projection has just written): ln_part[((n * S + g) * 2 + {0, 1}) * P + p] = fp64 sum / sum of squares of the finished
 * rows of segment g for column p, S = mvip_gemm_ln_segments(N, K, M, P, prec) segments of M / S rows each
 * (N * S * 2 * P doubles).  mvip_gemm_ln_segments returns 0 for shapes whose launch cannot leave them (split-K
 * launches, the square-tile kernel); mvip_gemm_f16x3_ws_ln then returns MVIP_EINVAL and the caller keeps
 * mvip_layernorm_split_planes' own statistics pass. */
int64_t mvip_gemm_ln_segments(int64_t N, int64_t K, int64_t M, int64_t P, int prec);
int mvip_gemm_f16x3_ws_ln(const void *xs, const void *packed, const float *bias, const float *chan_add,
                          const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                          float *y, void *workspace, void *ln_part, int prec, void *stream);

/* ------------------------------------------------------------------------------------------
 * a14-a16  transformer blocks of the SD UNet (unet(...) at DS_NeRF/guidance/sd_utils.py:390-403 and :240;
 * the block structure is the published SD-1.5 one: LayerNorm -> 8-head self-attention -> LayerNorm ->
 * cross-attention onto the 77 prompt tokens -> LayerNorm -> GEGLU feed-forward).  Activations stay
 * channel-major [N][C][LP] (LP = tokens padded to a multiple of 256), so every linear layer is
 * mvip_gemm_f16x3 with the weight as the A operand and no layout transposes; these entry points produce
 * its operands and run the attention itself, all in split precision (fp16 hi/lo operands, three products,
 * fp32 accumulation: fp32-grade results).
 *
 * mvip_attention_f16x3: flash-style multi-head attention, nothing of size [Lq, Lk] touches memory.
 *   qs, ks : split planes [N][heads*NCH][2][2][Lq | LkP][8] (mvip_split_planes_strided), NCH = ceil(D/16),
 *            head h = chunks h*NCH.., channels beyond D zero; scaled by q_scale2[0] / k_scale2[0];
 *   vp     : mvip_attention_pack_v output (mvip_attention_v_bytes bytes), scaled by v_scale2[0];
 *   out    : fp32 [N][heads*D][LqP], columns < Lq written;
 *   out[n, h*D + d, i] = sum_j softmax_j(softmax_scale q_i . k_j)[j < Lk] v_j[d].
 *   D in {40, 80, 160} (mvip_attention_supported), Lq % 32 == 0, LkP % 64 == 0, LkP >= Lk.
 *   flags (tuning switches, same results): bit 0 = 64-key LDS tiles for D = 40, bit 1 = never use the 256-query
 *   workgroup.
 * mvip_attention_pack_v: v[n*sn + (h*DP + d)*sr + key*sk], d < D <= DP, key < Lk -> A fragments whose k order
 *   is the accumulator-row order of the score tile (so the probabilities feed the second product from
 *   registers), zero padded to LkP.
 * mvip_absmax_scale_sections: x [outer][sections][len] -> scale2[s] = {2^k, 2^-k, -, -} per section
 *   (|x|max 2^k in [2^9, 2^10)), sections <= 63; ONE launch for the q / k / v thirds of a fused projection (the last
 *   workgroup writes the scales).
 *   zero_words64: 64 caller-owned 32-bit scratch words that are ZERO on entry and left zero on exit (allocate
 *   zeroed once per stream; the maxima are collected there with atomics, which saves a zeroing launch per use). */
int mvip_attention_supported(int64_t D);
int64_t mvip_attention_v_bytes(int64_t N, int64_t heads, int64_t D, int64_t LkP);
int mvip_attention_pack_v(const float *v, int64_t N, int64_t heads, int64_t D, int64_t DP, int64_t Lk, int64_t LkP,
                          int64_t sn, int64_t sr, int64_t sk, const float *scale2, void *vp, int prec, void *stream);
int mvip_absmax_scale_sections(const float *x, int64_t outer, int64_t sections, int64_t len, float *scale2,
                               void *zero_words64, void *stream);
int mvip_attention_f16x3(const void *qs, const void *ks, const void *vp, const float *q_scale2, const float *k_scale2,
                         const float *v_scale2, int64_t N, int64_t heads, int64_t D, int64_t Lq, int64_t LqP,
                         int64_t Lk, int64_t LkP, float softmax_scale, int flags, float *out, int prec, void *stream);
/* `prec` (round 3) on the operand producers and the contractions of this section and the next: 0 = split precision
 * ("f16x3": fp16 hi + lo halves of both operands, three products, fp32 accumulate -- fp32-grade results, the default of
 * the fp32 networks); 1 = the reference's --fp16 mode (DS_NeRF/guidance/sd_utils.py:66, DS_NeRF/run.py:251): ONE fp16
 * product per step, fp32 accumulate -- producers write the hi planes only, contractions fetch hi planes / hi weight
 * fragments only (a third of the matrix work, half the operand traffic; ~1e-3 relative, fp16-grade).  Operand buffers have
 * the same size and layout in both modes.
 * 2 (round 4; the CONTRACTIONS that take a packed weight image: mvip_conv3x3_f16x3*, mvip_gemm_f16x3*,
 * mvip_gemm_geglu_f16x3*, mvip_gemm_f16x3_sinks, mvip_gemm_f16x3_planes_ws) = TWO products, Wh.Xh + Wh.Xl: the caller
 * asserts that the image's lo fragments are zero (mvip_packed_weights_two_product said 1).  The third product of prec 0
 * would add exact zeros, so every output bit equals prec 0's, with a third less matrix work and half the weight-operand
 * bytes.  Activations are split and fetched as for prec 0 (producers take 0 or 1, and treat 2 as 0); a launch shape
 * without a two-product instantiation silently runs the three-product kernel (same result).  With prec = 1 a shape
 * without a single-product instantiation returns MVIP_EUNSUP (its lo planes were never written). */
/* Contractions that hand each other OPERANDS (round 3; same call sites: the unet(...) call of
 * DS_NeRF/guidance/sd_utils.py:390-403 / :240).  Between two contractions of a transformer block the reference
 * materialises an fp32 tensor; rounds 1-2 of this library followed it with an absolute-maximum pass and a split pass.
 * Here the PRODUCER's epilogue writes the consumer's operand format, scaled by a power of two that the caller fixes
 * BEFORE the launch from a rigorous bound of the result (|W x| <= |x|max * max_row ||W||_1; |LayerNorm(x)| <=
 * sqrt(C) |gamma|max + |beta|max; |softmax(..) V| <= |V|max; |a gelu(g)| <= |a| |g|): no overflow by construction, and the
 * fp16 hi + lo pair keeps ~2^-25 of the scaled range, i.e. fp32-grade accuracy relative to the tensor's maximum for
 * bounds up to ~2^15 too wide.
 * mvip_gemm_f16x3_sinks: Y = W X + bias with the M rows cut into nsec <= 3 consecutive sections of sec_rows[i] rows
 *   (multiples of 64).  Section i leaves as (Y * sec_scale[i]) in format sec_kind[i]:
 *     1  split planes [N][sec_rows/16][2][2][P][8 halves] -- the B operand of mvip_gemm_f16x3 / the Q or K operand of
 *        mvip_attention_f16x3_sink;
 *     2  attention V fragments [N][heads][v_dt][P/16][2][64][8 halves], sec_rows = heads * v_dt * 32 (head h's rows at
 *        h * v_dt * 32 .., zero rows beyond its D channels); only as the LAST section (computed with the MFMA operands
 *        swapped, i.e. transposed, in a launch of its own).
 * mvip_gemm_geglu_f16x3_sink: mvip_gemm_geglu_f16x3 whose product leaves as planes [N][(M2/2)/16][2][2][P][8] * out_scale.
 * mvip_attention_f16x3_sink: mvip_attention_f16x3 on operands written by mvip_gemm_f16x3_sinks (q_stride / k_stride tokens
 *   per plane, v_groups 16-key groups per V block) whose result leaves as the output projection's operand planes
 *   [N][heads*D/16][2][2][LqP][8 halves] scaled by v_scale2[0]; columns >= Lq are not written. */
int mvip_gemm_f16x3_sinks(const void *xs, const void *packed, const float *bias, const float *x_scale2, int64_t N,
                          int64_t K, int64_t M, int64_t P, int nsec, const int64_t *sec_rows, const int *sec_kind,
                          void *const *sec_ptr, const float *sec_scale, int v_dt, int prec, void *stream);
/* (W X + bias + residual) * out_scale as ONE section of split planes [N][M/16][2][2][P][8 halves]: the second
 * feed-forward projection handing the finished residual stream to proj_out as its operand.  Split-K as in
 * mvip_gemm_f16x3_ws (workspace of mvip_gemm_workspace_bytes(N, K, M, P) bytes, NULL when that is 0); M % 32 == 0. */
int mvip_gemm_f16x3_planes_ws(const void *xs, const void *packed, const float *bias, const float *residual,
                              const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P, void *out_planes,
                              float out_scale, void *workspace, int prec, void *stream);
int mvip_gemm_geglu_f16x3_sink(const void *xs, const void *packed, const float *bias, const float *x_scale2, int64_t N,
                               int64_t K, int64_t M2, int64_t P, int64_t L, void *out_planes, float out_scale,
                               int prec, void *stream);
int mvip_attention_f16x3_sink(const void *qs, const void *ks, const void *vp, const float *q_scale2, const float *k_scale2,
                              const float *v_scale2, int64_t N, int64_t heads, int64_t D, int64_t Lq, int64_t LqP,
                              int64_t Lk, int64_t LkP, int64_t q_stride, int64_t k_stride, int64_t v_groups,
                              float softmax_scale, int flags, void *out_planes, int prec, void *stream);
/* LayerNorm over the channel axis of x [N][C][LP] for tokens < L, times out_scale (a power of two), written as
 * split planes [N][C/16][2][2][LP][8] (zero for tokens >= L).  C % 64 == 0, LP % 256 == 0; workspace of
 * mvip_layernorm_workspace_bytes(N, C, LP) bytes (fp64 partial moments), 8-byte aligned. */
int64_t mvip_layernorm_workspace_bytes(int64_t N, int64_t C, int64_t LP);
int mvip_layernorm_split_planes(const float *x, const float *gamma, const float *beta, int64_t N, int64_t C,
                                int64_t L, int64_t LP, float eps, float out_scale, void *workspace, void *xs,
                                int prec, void *stream);
/* The normalise + split half alone, from statistics `part` = [N][segments][2][LP] fp64 (sum, sum of squares) over
 * `segments` disjoint channel ranges covering C -- what mvip_gemm_f16x3_ws_ln leaves: one launch, no pass over x for
 * its moments.  C % 16 == 0. */
int mvip_layernorm_split_planes_stats(const float *x, const float *gamma, const float *beta, const void *part,
                                      int64_t segments, int64_t N, int64_t C, int64_t L, int64_t LP, float eps,
                                      float out_scale, void *xs, int prec, void *stream);
/* GEGLU: y [N][2R][LP] -> out [N][R][LP] = y[:, :R] * gelu(y[:, R:]) (erf form) for tokens < L, zero beyond;
 * scale2 = {2^k, 2^-k, -, -} from the result's absolute maximum; zero_word: one scratch word as in
 * mvip_absmax_scale_sections (zero on entry, zero on exit). */
int mvip_geglu(const float *y, int64_t N, int64_t R, int64_t L, int64_t LP, float *out, float *scale2, void *zero_word,
               void *stream);
/* y [NB][M] = act(x [NB][K]) W[M][K]^T + b  (act_in: 0 identity, 1 SiLU), NB <= 8: the timestep-embedding MLP and
 * the ResNet blocks' time projections (published SD-1.5 UNet), exact fp32, one wavefront per output feature. */
int mvip_linear_small(const float *x, const float *W, const float *b, int64_t NB, int64_t M, int64_t K, int act_in,
                      float *y, void *stream);
/* The same for several layers sharing the input x (the UNet's 22 ResNet time projections all read silu(temb)): W [M][K]
 * and b [M] hold the layers' rows one after the other, layer_off (n_layers + 1 device ints) their first rows, and layer
 * l's result is its own contiguous [NB][C_l] block at y + layer_off[l] * NB. */
int mvip_linear_small_grouped(const float *x, const float *W, const float *b, int64_t NB, int64_t M, int64_t K, int act_in,
                              const int *layer_off, int64_t n_layers, float *y, void *stream);

/* ------------------------------------------------------------------------------------------
 * encodings of the reference's second model NeRF_TCNN
 * (DS_NeRF/run_nerf_helpers_tcnn.py:36-46 hash grid, :63-69 spherical harmonics, :91-101 forward), which
 * the reference takes from tiny-cuda-nn (absent from the reference tree; published algorithm restated).
 * x [P,3] raw coordinates, mapped to [0,1] by (x + bound)/(2 bound) when bound > 0; table [n_entries,2];
 * levels [16][4] 32-bit words {scale (fp32 bits), resolution, offset, size} in DEVICE memory;
 * features / d_features [32][P] level-major (row 2l+f = feature f of level l); d_table is accumulated
 * into (zero it first).  mvip_sh4: dirs [P,3] in [-1,1] -> out [16][P]. */
int mvip_hashgrid_forward(const float *x, const float *table, const void *levels, int64_t P, float bound,
                          float *features, void *stream);
int mvip_hashgrid_backward(const float *x, const float *d_features, const void *levels, int64_t P, float bound,
                           float *d_table, void *stream);
int mvip_sh4(const float *dirs, int64_t P, float *out, void *stream);
/* Opt-in table gradient with tiny-cuda-nn's own arithmetic for the scattered contributions (half-precision pair
 * atomics): scale2 = {s, 1/s} from mvip_absmax_scale(d_features); d_table (fp32) and d_table_h2 ([n_entries] fp16
 * pairs) zeroed by the caller; gradient = d_table + d_table_h2 * (16 * scale2[1]). */
int mvip_hashgrid_backward_half2(const float *x, const float *d_features, const void *levels, int64_t P, float bound,
                                 const float *scale2, float *d_table, void *d_table_h2, void *stream);

/* Fused no-grad NeRF_TCNN.forward (run_nerf_helpers_tcnn.py:88-112): x [P,3], dirs [P,3] -> raw [P,4] =
 * (colour 0..2, sigma), in exact fp32 on the matrix pipe.  sigma_params = [64x32 | 16x64] floats, colour_params =
 * [64x32 | 64x64 | 16x64] floats ([out][in] row-major, layer order = the tiny-cuda-nn `params` vectors);
 * mvip_hashgrid_mlp_pack writes the kernel's operand image (mvip_hashgrid_mlp_packed_floats() floats). */
int64_t mvip_hashgrid_mlp_packed_floats(void);
int mvip_hashgrid_mlp_pack(const float *sigma_params, const float *colour_params, float *img, void *stream);
int mvip_hashgrid_nerf_forward(const float *x, const float *dirs, const float *table, const void *levels,
                               const float *img, int64_t P, float bound, float *raw, void *stream);

/* Weight gradient of one bias-free layer of that model's MLPs (what autograd derives for the reference's
 * tcnn.Network calls, run_nerf_helpers_tcnn.py:96-108): dW[M][N] = sum_p dY[m][p] X[n][p], operands channel-major
 * [C][P], 1 <= M, N <= 64, P % 64 == 0.  Writes mvip_skinny_wgrad_slabs(P) partial [M][N] slabs; their sum in
 * index order is dW. */
int64_t mvip_skinny_wgrad_slabs(int64_t P);
int mvip_skinny_wgrad(const float *dY, const float *X, int64_t M, int64_t N, int64_t P, float *slabs, void *stream);
/* Forward / data gradient of the same layers: Y[M][P] = act(W X), W[m][n] = w[m*w_sm + n*w_sn] (the data gradient passes
 * the same weight with the two strides swapped), X [N][P] channel-major, 1 <= M, N <= 64, P % 4 == 0, X / Y 16-byte
 * aligned; relu != 0 applies max(., 0) (the activation of tcnn's hidden layers).  Exact fp32 on the matrix pipe, one
 * streaming pass: (N + M) x 4 bytes per point. */
int mvip_skinny_linear(const float *w, int64_t w_sm, int64_t w_sn, const float *X, int64_t M, int64_t N, int64_t P,
                       int relu, float *Y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Marching-cubes mesh extraction (beyond the reference: it has no mesh export; csrc/mcubes.hip,
 * mvip_nerf_amd/mesh.py).  grid [nx,ny,nz] fp32, C-contiguous (z fastest), 2 <= n <= 768 per axis;
 * point (i,j,k) sits at bmin + (i,j,k) * (bmax - bmin) / (n - 1).  A corner is inside iff v >= iso
 * (iso > 0); an edge crosses iff exactly one end is inside; t = (iso - v0) / (v1 - v0),
 * p = p0 + t (p1 - p0).  Vertices are ordered by (point linear index, axis x < y < z), triangles by
 * (cell linear index, table slot), faces counter-clockwise seen from outside (decreasing sigma).
 * tri_table: 256 x 16 int8 (-1 terminated; corner c = dx + 2 dy + 4 dz, edge e = 4 axis + r), 16-byte
 * aligned DEVICE memory, the table of mvip_nerf_amd/mesh.py.
 *
 * mvip_mcubes_groups: G, the workgroup count of a grid (-1 for a shape outside the limits).
 * mvip_mcubes_count: flags [nx*ny*nz] uint16 (cube index | edge flags << 8), wg [G,2] int64 (vertex and
 *   triangle offsets of each workgroup), totals [3] int64 = (vertices, triangles, non-finite flag).  The
 *   caller reads totals back once to allocate the outputs.  No empty form (every axis has >= 2 points).
 * mvip_mcubes_emit: from count's flags / wg and its totals (n_verts, n_tris): vid [nx*ny*nz] int32 (first
 *   vertex id of each point), verts / normals [n_verts,3] (normals: -grad sigma, central differences at
 *   the edge ends, interpolated, normalised), faces [n_tris,3] int32.  n_verts = n_tris = 0 is the empty
 *   call (MVIP_OK, nothing written); n_tris must be <= 2^31 - 1. */
int64_t mvip_mcubes_groups(int nx, int ny, int nz);
int mvip_mcubes_count(const float *grid, int nx, int ny, int nz, float iso, const void *tri_table, void *flags,
                      int64_t *wg, int64_t *totals, void *stream);
int mvip_mcubes_emit(const float *grid, int nx, int ny, int nz, float iso, float x0, float y0, float z0, float x1,
                     float y1, float z1, const void *tri_table, const void *flags, const int64_t *wg, int64_t n_verts,
                     int64_t n_tris, int *vid, float *verts, float *normals, int *faces, void *stream);
/* mvip_mcubes_count_valid: mvip_mcubes_count restricted to observed cells (beyond the reference, which has no mesh export;
 * mesh.fuse_depths).  valid [nx,ny,nz] bytes, non-zero = observed.  A cell is live iff its eight corners are valid; a cell
 * that is not live gets cube index 0 (no triangles), and a point's owned edge keeps its crossing flag iff the values cross
 * and at least one of the up to four cells sharing the edge is live: every vertex mvip_mcubes_emit then writes is
 * referenced by a triangle, and every triangle's vertices exist.  The non-finite flag looks at valid points only (a point
 * that is not valid may hold anything).  flags / wg / totals as mvip_mcubes_count, and mvip_mcubes_emit takes them
 * unchanged; its normals are central differences of the grid and read the fill value of a point that is not valid within
 * one lattice step of it.  valid all non-zero: the flags of mvip_mcubes_count, bit for bit.  A NULL operand is MVIP_EINVAL. */
int mvip_mcubes_count_valid(const float *grid, const void *valid, int nx, int ny, int nz, float iso, const void *tri_table,
                            void *flags, int64_t *wg, int64_t *totals, void *stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy-grid empty-space skipping for no-grad renders (beyond the reference: it evaluates every
 * sample; csrc/occupancy.hip, mvip_nerf_amd/occupancy.py).  A grid is a box cut into cells = (cx,cy,cz),
 * 1 <= c <= 512 per axis, one bit per cell: linear cell l = (ix*cy + iy)*cz + iz (z fastest), bit l & 31
 * of int32 word l >> 5, (cx*cy*cz + 31) / 32 words in DEVICE memory, unused tail bits zero.  Entry points
 * that test points take the grid as box = {bmin[3], inv[3]} (6 floats, HOST memory; inv = cells /
 * (bmax - bmin) > 0, rounded to fp32 by the caller), cells (3 ints, HOST memory) and words.  Cell of a
 * point p, per axis in fp32: f = floorf((p - bmin) * inv); p is inside the box iff 0 <= f < c on all
 * three axes (NaN / infinite coordinates: outside); keep(p) = outside the box, or bit set.
 *
 * mvip_occupancy_build: sigma [cx*k+1, cy*k+1, cz*k+1] fp32 (k = samples_per_cell, 1..8; z fastest) ->
 *   words: cell (i,j,l) owns points i*k .. (i+1)*k on each axis and is occupied iff any of them has
 *   !(sigma <= threshold) (NaN counts as occupied); threshold >= 0, finite.
 * mvip_occupancy_dilate: words_out = OR over the <= 27 cells at Chebyshev distance <= 1 of words_in
 *   (clipped at the faces); the two arrays must differ.
 * mvip_occupancy_groups: G, the workgroup count of a chunk of B rays x S samples (-1 when S < 1 or
 *   B*S exceeds 2^31 - 1).
 * mvip_occupancy_count: rows [B,11], z [B,S]; flat sample s = ray*S + j has the point
 *   rows[0:3] + rows[3:6] * z (the expression of the mvip_mlp_forward_rays* kernels).  wg [G] int32
 *   receives the exclusive offsets of the kept samples of each workgroup, total [1] int64 their number
 *   K; the caller reads total back once to allocate mvip_occupancy_emit's outputs.  Optional (NULL to
 *   skip): mask [B,S] uint8 = keep, pts_full [B,S,3].  B == 0: MVIP_OK, nothing launched or written.
 * mvip_occupancy_emit: from count's wg and K: in ascending s, idx [K] int32 = s, pts [K,3] the sample
 *   points, dirs [K,3] = rows[8:11].  B == 0 or K == 0: MVIP_OK, nothing launched.
 * mvip_scatter_raw: raw [n,4] = 0, then raw[idx[j]] = raw_k[j] for j < K (idx ascending, distinct, < n;
 *   K <= n <= 2^31 - 1; raw and raw_k 16-byte aligned).  The zero fill is part of the operation (K == 0
 *   fills only); n == 0: MVIP_OK, nothing launched.
 * mvip_occupancy_lookup: out [P] uint8 = keep(pts[p]), pts [P,3].  P == 0: MVIP_OK, nothing launched.
 * No atomics anywhere: the outputs are reproducible bit for bit. */
int mvip_occupancy_build(const float *sigma, int cx, int cy, int cz, int samples_per_cell, float threshold, int *words,
                         void *stream);
int mvip_occupancy_dilate(const int *words_in, int cx, int cy, int cz, int *words_out, void *stream);
int64_t mvip_occupancy_groups(int64_t B, int S);
int mvip_occupancy_count(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                         const int *words, int *wg, int64_t *total, void *mask, float *pts_full, void *stream);
int mvip_occupancy_emit(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                        const int *words, const int *wg, int64_t K, int *idx, float *pts, float *dirs, void *stream);
int mvip_scatter_raw(const float *raw_k, const int *idx, int64_t K, int64_t n, float *raw, void *stream);
int mvip_occupancy_lookup(const float *pts, int64_t P, const float *box, const int *cells, const int *words, void *out,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Regions: 3D-consistent inpainting masks (beyond the reference, which takes its masks as given;
 * csrc/region.hip, mvip_nerf_amd/region.py).  A region is a set of cells of a box, stored exactly as an
 * occupancy grid above (box = {bmin[3], inv[3]} and cells in HOST memory, words in DEVICE memory, the
 * same cell, bit and tail conventions).  The one difference: inside(p) = in the box AND bit set.
 *
 * mvip_region_mark: pts [P,3]; every point in the box ORs its bit into words (in/out: bits already set
 *   stay set).  Uses a vector atomic OR on the word: OR is commutative and idempotent, so the words do
 *   not depend on the order of execution and the result is reproducible bit for bit.  P == 0: MVIP_OK,
 *   nothing launched.
 * mvip_region_accumulate: rows [B,11], z [B,S], weights [B,S] -> out [B] = sum over j of
 *   (inside(rows[0:3] + rows[3:6] * z[b,j]) ? weights[b,j] : 0), the point in the expression of the
 *   mvip_mlp_forward_rays* kernels.  A select: a NaN weight outside the region does not reach the sum.
 *   Fixed summation order: one wave per ray, lane t adds j = t, t + 64, ... in ascending j, then one fixed
 *   six-step DPP tree; a ray's result does not depend on B or on its neighbours.  S >= 1,
 *   B*S <= 2^31 - 1.  B == 0: MVIP_OK, nothing launched.
 * mvip_region_lookup: out [P] uint8 = inside(pts[p]), pts [P,3].  P == 0: MVIP_OK, nothing launched. */
int mvip_region_mark(const float *pts, int64_t P, const float *box, const int *cells, int *words, void *stream);
int mvip_region_accumulate(const float *rows, const float *z, const float *weights, int64_t B, int S, const float *box,
                           const int *cells, const int *words, float *out, void *stream);
int mvip_region_lookup(const float *pts, int64_t P, const float *box, const int *cells, const int *words, void *out,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of a bit array (beyond the reference, which has no geometry clean-up;
 * csrc/components.hip, mvip_nerf_amd/bitgrid.py and mesh.py).  The array is [nx,ny,nz], z fastest,
 * 1 <= n <= 768 per axis (the cells of a grid above, or the lattice points of marching cubes); element
 * l = (i*ny + j)*nz + k is bit l & 31 of int32 word l >> 5, (nx*ny*nz + 31) / 32 words in DEVICE
 * memory, unused tail bits zero.  Two set elements are neighbours at connectivity 6 if they differ by
 * one step on one axis, at connectivity 26 if by at most one step on every axis; a neighbour exists
 * only inside the array.  Components are numbered 1, 2, ... by ascending lowest linear index of their
 * elements.
 *
 * mvip_components_pack: values [n] fp32 -> words [(n + 31) / 32], bit l = values[l] >= threshold (NaN
 *   value: clear); 0 <= n <= 768^3, threshold not NaN.  n == 0: MVIP_OK, nothing launched.
 * mvip_components_groups: G, the workgroup count of an array (-1 for a shape outside the limits).
 * mvip_components_label: union-find over the set elements; parent [nx*ny*nz] int32 receives -1 for a
 *   clear bit and else the lowest linear index of the element's component, wg [G] int32 the exclusive
 *   offsets of the component roots of each workgroup, total [1] int64 the number of components; the
 *   caller reads total back once to allocate mvip_components_rank's outputs.  connectivity: 6 or 26.
 *   The unions use a vector atomic minimum; every link points to a lower index, so the root of a
 *   component is its lowest index whatever order the unions ran in and the outputs are reproducible
 *   bit for bit.
 * mvip_components_rank: from label's parent / wg and n_components: labels [nx*ny*nz] int32 (0 for a
 *   clear bit, else the component's number), sizes [n_components] int32 (integer atomic adds: exact
 *   in any order), first [n_components] int32 (lowest linear index).  n_components == 0: MVIP_OK,
 *   nothing launched or written.
 * mvip_components_select: labels [n] and keep [n_components + 1] uint8 (keep[0] is not read: label 0
 *   is never kept) -> words [(n + 31) / 32]: bit l set iff keep[labels[l]] != 0.  n == 0: MVIP_OK,
 *   nothing launched. */
int mvip_components_pack(const float *values, int64_t n, float threshold, int *words, void *stream);
int64_t mvip_components_groups(int nx, int ny, int nz);
int mvip_components_label(const int *words, int nx, int ny, int nz, int connectivity, int *parent, int *wg, int64_t *total,
                          void *stream);
int mvip_components_rank(const int *parent, int nx, int ny, int nz, const int *wg, int64_t n_components, int *labels,
                         int *sizes, int *first, void *stream);
int mvip_components_select(const int *labels, int64_t n, const void *keep, int64_t n_components, int *words, void *stream);

/* ------------------------------------------------------------------------------------------
 * Ray distortion loss (mip-NeRF 360, eq. 15; beyond the reference, which has no regulariser of this kind and
 * no call site this replaces; csrc/distortion.hip).  rows [B,ncols] (ncols 8 or 11; near = column 6,
 * far = column 7), z [B,S] in ascending order along the ray, weights [B,S].
 *   s_j = (z_j - near) / (far - near), with lindisp != 0 (1/z_j - 1/near) / (1/far - 1/near), in fp32;
 *   sample j < S-1 owns [s_j, s_{j+1}] (midpoint m_j, width d_j), the last sample the point s_{S-1} (d = 0);
 *   loss[b] = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_j w_j^2 d_j
 *   grad[b,k] = d loss[b] / d w_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k d_k      (optional: NULL = loss only)
 * One launch, one wave per ray, sums of non-negative terms in a fixed order; a ray's result does not depend
 * on B or on its neighbours, and the loss does not depend on whether grad is asked for.  A non-finite
 * weight or depth (or far == near) makes that ray's loss and gradient row non-finite and touches no other.
 * S >= 1, B*S <= 2^31 - 1.  B == 0: MVIP_OK, nothing launched. */
int mvip_distortion_loss(const float *rows, int ncols, const float *z, const float *weights, int64_t B, int S, int lindisp,
                         float *loss, float *grad, void *stream);

/* ------------------------------------------------------------------------------------------
 * Harmonic hole filling of disparity maps and 2D mask dilation (beyond the reference; stands in for
 * --prepare + LaMa, which produce its Depth_inpainted/ targets; csrc/harmonic.hip, mvip_nerf_amd/prepare.py).
 * values [N,H,W] fp32, masks [N,H,W] bytes (0 / non-zero), out [N,H,W] fp32 (not values), all DEVICE memory.
 * Per image: U = masked or non-finite pixels, K the rest, N(p) the 4-neighbours inside the image, deg = |N(p)|;
 *   for p in U: deg(p) u_p - sum_{q in N(p), q in U} u_q = sum_{q in N(p), q in K} values_q;
 *   out = values bit for bit on K and u on U.  U empty: out = values, no iteration.  U = the whole image:
 *   singular, out = values.  Solved by Jacobi-preconditioned conjugate gradients from u = 0, per image
 *   until r.z <= eps^2 r0.z0; every sum in a fixed order, no float atomics: image n of a batch equals the
 *   single-image call bit for bit, and a call equals its repetition.
 * The caller provides workspace (mvip_harmonic_workspace_bytes(N,H,W) bytes, DEVICE) and state [N,16] int32
 * (DEVICE): word 0 active tiles, 1 unknowns, 2 singular, 3 done, 4 iterations, 5..7 r0.z0 and r.z (fp32 bits),
 * 8 true residual (fp32 bits), 9 converged.  Nothing is allocated or synchronised inside; the caller reads
 * state back between the calls.  1 <= H, W <= 16384, N * tiles <= 2^31 - 1; a bad shape (or, with N > 0, a NULL
 * operand) is MVIP_EINVAL before anything is touched; N == 0: MVIP_OK, nothing launched.
 * mvip_harmonic_tiles: tiles of 64 x 16 pixels per image (-1 for a bad shape).
 * mvip_harmonic_setup: marks U, copies values to out, lists each image's active tiles, fills state words 0..4.
 * mvip_harmonic_init: u = 0, the right-hand side, r0.z0 partials; max_act >= every image's active tile count
 *   (max_act == 0: nothing launched).
 * mvip_poisson_init: mvip_harmonic_init with a guidance field (gradient-domain / Poisson blending; between
 *   mvip_harmonic_setup and mvip_harmonic_iterate, in mvip_harmonic_init's place).  guide [N,H,W] fp32, labels
 *   [N,H,W] int32, DEVICE.  An edge (p, q), q in N(p), is guided iff labels_p >= 0, labels_q == labels_p and
 *   guide_p, guide_q are both finite; the right-hand side of p in U is
 *     sum_{q in N(p), q in K} values_q + sum_{q in N(p), (p,q) guided} (guide_p - guide_q)
 *   (each sum in fp32 in the order up, left, right, down from 0, the second added to the first).  With no guided
 *   edge it is mvip_harmonic_init's bit for bit.  NULL values / guide / labels / out / workspace / state, or
 *   out == values: MVIP_EINVAL.
 * mvip_harmonic_iterate: CG iterations first_iteration .. first_iteration + iterations - 1, two launches each;
 *   a converged image is frozen (it divides nothing) and sets its done word.  0 <= eps < 1.
 * mvip_harmonic_finish: state word 8 = max over U of |sum_{N(p)} out_q - deg out_p| / deg, word 9 = converged.
 * mvip_mask_dilate2d: one round; out = 1 iff any pixel at Chebyshev distance <= 1 is non-zero, clipped at the
 *   border; masks_out must differ from masks_in. */
int64_t mvip_harmonic_tiles(int H, int W);
int64_t mvip_harmonic_workspace_bytes(int64_t N, int H, int W);
int mvip_harmonic_setup(const float *values, const void *masks, int64_t N, int H, int W, float *out, void *workspace,
                        int *state, void *stream);
int mvip_harmonic_init(const float *values, int64_t N, int H, int W, float *out, void *workspace, const int *state,
                       int64_t max_act, void *stream);
int mvip_poisson_init(const float *values, const float *guide, const int *labels, int64_t N, int H, int W, float *out,
                      void *workspace, const int *state, int64_t max_act, void *stream);
int mvip_harmonic_iterate(int64_t N, int H, int W, float *out, void *workspace, int *state, int64_t max_act,
                          int first_iteration, int iterations, float eps, void *stream);
int mvip_harmonic_finish(int64_t N, int H, int W, const float *out, void *workspace, int *state, int64_t max_act, float eps,
                         void *stream);
int mvip_mask_dilate2d(const void *masks_in, int64_t N, int H, int W, void *masks_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Reference-view propagation: backward depth warping (beyond the reference, which has no counterpart: its
 * RGB_inpainted/ images are independent 2D inpaintings; csrc/warp.hip, ops.warp_views,
 * prepare.propagate_reference).  All operands DEVICE memory, dense:
 *   tgt_disp [N,H,W] fp32, tgt_pose [N,3,4] (camera-to-world, get_rays' convention), tgt_mask [N,H,W] bytes
 *   (0 / non-zero: the pixels to compute); src_rgb [S,H,W,3], src_disp [S,H,W], src_pose [S,3,4];
 *   order [N,S] int32: per target the sources in order of preference, an entry outside [0,S) is skipped.
 * A masked target pixel with a finite disparity > 0 is lifted to its world point at planar depth 1/disp and
 * projected into each source of its order row in turn; the source's disparity d_s and colour are read
 * bilinearly (taps x0 = min(floor(u), W-2), y0 = min(floor(v), H-2)); the first source with t_s > 0,
 * 0 <= u <= W-1, 0 <= v <= H-1, d_s finite and > 0, |t_s d_s - 1| <= tol and finite colours is taken (the
 * operation order is written out in csrc/warp.hip and tests/warp_numpy.py).
 *   rgb [N,H,W,3], index [N,H,W] int32 (the source, or -1), resid [N,H,W] (t_s d_s - 1); every pixel of every
 *   target is written: 0 / -1 / 0 where the pixel is unmasked, invalid, or no source is taken.
 * One launch, one thread per target pixel, a pure gather: no atomics, every index bounded in the kernel, a
 * pixel's result independent of the rest of the batch (bit-reproducible).  2 <= H, W <= 16384, N, S >= 0,
 * N * ceil(W/64) * ceil(H/4) <= 2^31 - 1, focal and tol finite and > 0, else MVIP_EINVAL before anything is
 * touched; N == 0: MVIP_OK, nothing launched; with N > 0 a NULL target or output operand is MVIP_EINVAL, and
 * so is a NULL source operand or order unless S == 0 (then every pixel gets 0 / -1 / 0). */
int mvip_warp_views(const float *tgt_disp, const float *tgt_pose, const void *tgt_mask, int64_t N, int H, int W,
                    const float *src_rgb, const float *src_disp, const float *src_pose, int S, const int *order,
                    float focal, float tol, float *rgb, int *index, float *resid, void *stream);

/* ------------------------------------------------------------------------------------------
 * Structural similarity (SSIM, Wang et al. 2004) with its gradient (beyond the reference: DS_NeRF/evaluation.py
 * takes its metrics from pyiqa, so there is no reference call site this replaces; csrc/ssim.hip, ops.ssim,
 * mvip_nerf_amd/evaluate.py, the trainer's reference_ssim_lambda).  All operands DEVICE memory, dense:
 *   x, y [N,H,W,C] fp32 channel-last, C in 1..4; mask [N,H,W] bytes (0 / non-zero) or NULL (every pixel).
 * Window: 11 taps g_k ~ exp(-(k-5)^2 / (2 1.5^2)), normalised in fp64 and rounded to fp32, separable, "valid"
 * extent: the map is [N,H-10,W-10,C] and map pixel (i,j) is centred on image pixel (i+5,j+5).  Per channel, with
 * mu the windowed means and sigma the biased window-weighted second moments from raw moments,
 *   s = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2)),
 * C1 = 1e-4, C2 = 9e-4 (data range 1); no luminance conversion and no downsampling (not pyiqa's Y-channel
 * preprocessing).  A map pixel counts iff the mask is set at its centre; count[n] = counted map pixels,
 * ssim[n] = mean of s over counted pixels and channels; count[n] == 0: ssim[n] = 1 exactly.  The operation order
 * is written out in csrc/ssim.hip and tests/ssim_numpy.py.
 * mvip_ssim_tiles: map tiles of 32 x 16 per image = workgroups per image of the forward (-1 for a bad shape).
 * mvip_ssim_forward: two launches (tiles; a fixed-order fp64 reduction per image).  map [N,H-10,W-10,C] or NULL;
 *   stash [3,N,H-10,W-10,C] or NULL: the planes mvip_ssim_backward reads; partials [N*tiles] fp64 and
 *   partial_counts [N*tiles] int32: workspace; ssim [N] fp32, count [N] int32.
 * mvip_ssim_backward: one launch, a gather per image pixel (no atomics):
 *   gx[n] = d(gout[n] ssim[n]) / d x[n]  [N,H,W,C]; count[n] == 0: an all-zero gradient.  gx is neither x nor y.
 * Every output is bit-reproducible and an image's results do not depend on the rest of the batch.
 * 11 <= H, W <= 16384, 1 <= C <= 4, N >= 0, N * ceil(W/32) * ceil(H/16) <= 2^31 - 1, else MVIP_EINVAL before anything is
 * touched; N == 0: MVIP_OK, nothing launched; with N > 0 a NULL operand other than mask / map / stash is MVIP_EINVAL. */
int64_t mvip_ssim_tiles(int H, int W);
int mvip_ssim_forward(const float *x, const float *y, const void *mask, int64_t N, int H, int W, int C, float *map,
                      float *stash, double *partials, int *partial_counts, float *ssim, int *count, void *stream);
int mvip_ssim_backward(const float *x, const float *y, const float *stash, const float *gout, const int *count, int64_t N,
                       int H, int W, int C, float *gx, void *stream);

/* ------------------------------------------------------------------------------------------
 * Exemplar-based (PatchMatch) image inpainting (beyond the reference, whose RGB_inpainted/ images are made elsewhere;
 * csrc/exemplar.hip, ops.exemplar_fill, prepare.inpaint_views).  A pyramid, then nearest-neighbour-field search
 * alternating with voting, coarse to fine, in integers on 8-bit colours; the definition is written out in
 * csrc/exemplar.hip and tests/exemplar_numpy.py, which agree bit for bit.  All operands DEVICE memory, dense:
 *   images [N,H,W,3] fp32, masks [N,H,W] bytes (0 / non-zero), sources [N,H,W] bytes or NULL (every known pixel
 *   may serve as an exemplar), out [N,H,W,3] fp32 (not images), nnf [N,H,W,2] int32 = (sy, sx) or -1 off the targets.
 * The caller provides workspace (mvip_exemplar_workspace_bytes bytes), meta (mvip_exemplar_meta_words int32 words,
 * 8-byte aligned) and, after reading meta back once, lists (int32).  meta: words 0..47 = totals[level][c] as int64
 * (c: 0 targets, 1 hole pixels, 2 sources; over the batch), 48..95 = where each list starts, then 32 words per
 * image: 0 levels used (0: singular, no source at level 0: returned unchanged), 1 singular, 2..3 the energy (uint64:
 * the summed SSD of the final field), 4 + 3 level + c the image's counts.
 * mvip_exemplar_levels: the pyramid's level count from the geometry (levels are added while min(h,w)/2 >= 4 patch;
 *   max_levels 0: no cap beyond 8), -1 for a bad shape.  It is the `levels` of the other entry points.
 * mvip_exemplar_setup: quantise, build the pyramid and the target / source sets, count them, plan.
 * mvip_exemplar_lists: the compacted lists; capacity = the sum of all totals (or more).
 * mvip_exemplar_level: one level's schedule (initial field, vote, rounds x (iters searches, vote); at level 0 the
 *   energy); call it for level = levels - 1 down to 0 with n_targets / n_holes = that level's totals, and the same
 *   rounds, iters and seed throughout.  Both totals 0: nothing launched.
 * mvip_exemplar_finish: out and nnf.
 * patch odd in 3..9, patch <= H, W <= 16384, N >= 0, 1 <= levels <= mvip_exemplar_levels(H,W,patch,0), the pixels of all
 * levels of the batch <= (2^31 - 1) / 4, rounds, iters >= 0, else MVIP_EINVAL (-1 from the size queries) before anything is
 * touched; N == 0: MVIP_OK, nothing launched; with N > 0 a NULL operand other than sources is MVIP_EINVAL. */
int mvip_exemplar_levels(int H, int W, int patch, int max_levels);
int64_t mvip_exemplar_meta_words(int64_t N);
int64_t mvip_exemplar_workspace_bytes(int64_t N, int H, int W, int patch, int levels);
int mvip_exemplar_setup(const float *images, const void *masks, const void *sources, int64_t N, int H, int W, int patch,
                        int levels, void *workspace, int *meta, void *stream);
int mvip_exemplar_lists(int64_t N, int H, int W, int patch, int levels, void *workspace, const int *meta, int *lists,
                        int64_t capacity, void *stream);
int mvip_exemplar_level(int64_t N, int H, int W, int patch, int levels, int level, int64_t n_targets, int64_t n_holes,
                        int rounds, int iters, unsigned seed, void *workspace, int *meta, const int *lists, void *stream);
int mvip_exemplar_finish(const float *images, int64_t N, int H, int W, int patch, int levels, int rounds, int iters,
                         void *workspace, const int *meta, float *out, int *nnf, void *stream);

/* ------------------------------------------------------------------------------------------
 * TSDF fusion of depth maps (beyond the reference, which renders depth images but has no mesh export and never fuses
 * them; csrc/tsdf.hip, ops.tsdf_fuse, mesh.fuse_depths).  All operands DEVICE memory, dense:
 *   disp [V,H,W] fp32 (disparity = 1 / planar depth, as prepare.render_disparities returns it), pose [V,3,4] row-major
 *   camera-to-world [R | o] (the camera of mvip_warp_views: no half-pixel offset, looking down -z), mask [V,H,W] bytes
 *   (0: ignore the pixel) or NULL; tsdf [nx,ny,nz] fp32 and count [nx,ny,nz] int32, z fastest; lattice point (i,j,k)
 *   sits at x0 + i hx, ..., hx = (x1 - x0) / (nx - 1) in fp32 (the lattice of mvip_mcubes_emit).
 * Per lattice point, over the views in ascending order: project into the view, take the NEAREST pixel (floor(u + .5),
 * floor(w + .5)); the view counts iff the point is in front of the camera, the pixel is inside the image, its mask byte
 * is set, its disparity d is finite and > 0 and sdf = 1/d - z >= -trunc (z: the point's planar depth); then it adds
 * min(1, sdf / trunc).  tsdf = the mean over the counted views, or 1 when there are none; count = their number (the
 * operation order is written out in csrc/tsdf.hip and tests/tsdf_numpy.py).
 * One launch, one thread per lattice point, a pure gather: no atomics, every index bounded in the kernel, every element of
 * both outputs written, a point's result independent of the others (bit-reproducible).  2 <= nx, ny, nz <= 768,
 * 1 <= H, W <= 16384, V >= 0, the box finite and increasing, focal and trunc finite and > 0, else MVIP_EINVAL before
 * anything is touched; a NULL output is MVIP_EINVAL, and so is a NULL disp or pose unless V == 0 (then tsdf = 1,
 * count = 0 everywhere). */
int mvip_tsdf_fuse(const float *disp, const float *pose, const void *mask, int V, int H, int W, float focal, int nx, int ny,
                   int nz, float x0, float y0, float z0, float x1, float y1, float z1, float trunc, float *tsdf, int *count,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh clean-up: vertex normals from the faces, Taubin smoothing, simplification by vertex clustering (beyond the
 * reference, which has no mesh export; csrc/mesh_ops.hip, ops.mesh_corner_table / mesh_vertex_normals / mesh_smooth /
 * mesh_cluster, mesh.vertex_normals / smooth / simplify).  The definitions, with their operation order, are written out
 * in csrc/mesh_ops.hip and tests/mesh_ops_numpy.py.  All operands DEVICE memory, dense, except box / cells (host):
 *   verts [V,3] fp32, faces [F,3] int32, colors [V,3] bytes or NULL; box = (origin[3], inv[3]) and cells[3] of the bit
 *   grid above, inv = fp32(1 / cell) on all three axes; `cell` the same edge as a double.
 * Every count is >= 0 and every V, 3 F, item and list count <= 2^31 - 1 (one more for the lists), a NULL operand that a
 * non-zero count makes necessary, a bad box / cells / cell / placement / dedupe: MVIP_EINVAL (-1 from the size queries)
 * before any device call.  Every launch goes on the caller's stream; no float atomics: all outputs are bit-reproducible.
 * mvip_mesh_list_scratch_words: int32 words of `scratch` below (8-byte aligned).
 * mvip_mesh_corner_table: for keys [n_items] in [0, n_lists): offsets [n_lists + 1], items [n_items];
 *   items[offsets[k] : offsets[k+1]] = the i with keys[i] == k, ascending.  keys = the flattened faces, n_lists = V:
 *   the corner table (corner c = 3 f + k is vertex faces[f,k]).  flag[0] = 1 iff a key lies outside [0, n_lists) (then
 *   offsets / items are not to be used), else 0: the caller's one read.
 * mvip_mesh_vertex_normals: normals [V,3] = normalised fp64 sum of (p1 - p0) x (p2 - p0) over the vertex's corners,
 *   (0,0,0) for an empty list or a zero sum.  offsets / corners: the corner table of these faces, flag 0.
 * mvip_mesh_smooth_pass: out = v + weight L(v), L(v) = (sum over v's corners of the two other vertices of the corner's
 *   face) / (2 n_corners) - v in fp64; a vertex without corners is copied.  out is not verts; weight finite.
 * mvip_mesh_rank_groups: workgroups of a rank pass over n items = int32 words of the `*_wg` workspaces (-1: bad n).
 * mvip_mesh_cluster_assign: words [n_words(cells)] = the bits of the occupied cells; cell_of_vertex [V] (the linear cell,
 *   -1 outside the box, which also sets flag[0]); word_rank [n_words], wg [rank_groups(n_words)]: workspace;
 *   total[0] = the number of clusters; cluster_of_vertex [V] = rank of the vertex's cell among the set bits.
 * mvip_mesh_gather: out[i] = map[idx[i]] (-1 where idx[i] is outside [0, n_map)): the faces remapped to clusters.
 * mvip_mesh_cluster_place: rep [K,3] and rep_colors [K,3] (NULL iff colors is) per cluster from its member list
 *   (mem_offsets / members: the table of keys = cluster_of_vertex) and corner list (cor_offsets / corners: the table of
 *   keys = the remapped faces); placement 0 = mean, 1 = quadric with both fallbacks to the mean.
 * mvip_mesh_cluster_faces: keep [F] (1: no two ids equal and, with dedupe, no earlier face with the same directed cycle),
 *   referenced [K], their ranks face_rank [F] / cluster_rank [K] (workspaces face_wg, cluster_wg), totals[0] = faces kept,
 *   totals[1] = clusters referenced: the caller's one read.
 * mvip_mesh_cluster_emit: out_faces [n_out_faces,3] (kept faces in input order, renumbered), out_verts / out_colors
 *   [n_out_verts,3] (referenced clusters in order), cluster_of_vertex [V] rewritten in place to the new numbering, -1 for
 *   the vertices of dropped clusters. */
int64_t mvip_mesh_list_scratch_words(int64_t n_items, int64_t n_lists);
int mvip_mesh_corner_table(const int *keys, int64_t n_items, int64_t n_lists, int *offsets, int *items, int *scratch,
                           int *flag, void *stream);
int mvip_mesh_vertex_normals(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const int *offsets,
                             const int *corners, float *normals, void *stream);
int mvip_mesh_smooth_pass(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const int *offsets,
                          const int *corners, double weight, float *out, void *stream);
int64_t mvip_mesh_rank_groups(int64_t n);
int mvip_mesh_cluster_assign(const float *verts, int64_t n_verts, const float *box, const int *cells, int *words,
                             int *cell_of_vertex, int *word_rank, int *wg, int64_t *total, int *cluster_of_vertex, int *flag,
                             void *stream);
int mvip_mesh_gather(const int *idx, int64_t n, const int *map, int64_t n_map, int *out, void *stream);
int mvip_mesh_cluster_place(const float *verts, const void *colors, const int *faces, int64_t n_verts, int64_t n_faces,
                            const float *box, const int *cells, double cell, int64_t n_clusters, const int *mem_offsets,
                            const int *members, const int *cor_offsets, const int *corners, const int *cell_of_vertex,
                            int placement, float *rep, void *rep_colors, void *stream);
int mvip_mesh_cluster_faces(const int *cluster_faces, int64_t n_faces, int64_t n_clusters, const int *cor_offsets,
                            const int *corners, int dedupe, int *keep, int *referenced, int *face_wg, int *face_rank,
                            int *cluster_wg, int *cluster_rank, int64_t *totals, void *stream);
int mvip_mesh_cluster_emit(const int *cluster_faces, int64_t n_faces, const int *keep, const int *face_rank, const float *rep,
                           const void *rep_colors, int64_t n_clusters, const int *referenced, const int *cluster_rank,
                           int64_t n_verts, int64_t n_out_faces, int64_t n_out_verts, int *cluster_of_vertex, float *out_verts,
                           void *out_colors, int *out_faces, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh rasterisation: per view the disparity, face-id and colour maps a mesh presents (beyond the reference, which has no
 * mesh export and no rasteriser: neither entry point has a reference call site; csrc/raster.hip, ops.mesh_rasterize,
 * mesh.render_views / visible_faces).  The definition, in fp64 and integers with its operation order, is written out in
 * csrc/raster.hip and tests/raster_numpy.py: the conventions of mvip_tsdf_fuse (poses [V,3,4] camera-to-world, looking
 * down -z, no half-pixel offset, disparity = 1 / planar depth), 8 sub-pixel bits, the top-left fill rule, no near-plane
 * clipping (a face with a vertex nearer than znear or outside the guard band of 16,384 pixels is dropped whole).  All
 * operands DEVICE memory, dense: verts [Nv,3] fp32, faces [F,3] int32, poses [V,3,4] fp32, colors [Nv,3] bytes or NULL,
 * keys [V,H,W] 64-bit words.  MVIP_EINVAL before any device call for: a negative count, Nv, 3 F or V > 2^31 - 1, H or W
 * outside 1..16384, focal or znear not finite and > 0, cull not 0 (none) or 1 (back-facing dropped), a NULL operand that a
 * non-zero count makes necessary, rgb given without colors (Nv > 0).  V = 0, F = 0 and Nv = 0 are valid.  Every
 * launch goes on the caller's stream; integer atomics only: the outputs are bit-reproducible.
 * mvip_raster_fragments: clears keys, flag[0] and stats, then leaves in keys[v,y,x] the largest
 *   (bits(D) << 32) | (0xFFFFFFFF - face) over the fragments of the pixel, 0 where there is none.  flag[0] = 1 iff a face
 *   index lies outside [0, Nv) (such a face is dropped): the caller's one read.  stats: NULL, or two 64-bit words that
 *   receive the fragments that passed every test and the atomics actually sent (a measuring variant of the kernel).
 * mvip_raster_resolve: disp [V,H,W] fp32 (0 where empty), face [V,H,W] int32 (-1 where empty) and, iff rgb is not NULL,
 *   rgb [V,H,W,3] bytes (0 where empty) from the keys of mvip_raster_fragments for the same mesh, poses and camera. */
int mvip_raster_fragments(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *poses,
                          int64_t n_views, int H, int W, double focal, double znear, int cull, void *keys, int *flag,
                          void *stats, void *stream);
int mvip_raster_resolve(const void *keys, const float *verts, const int *faces, const void *colors, int64_t n_verts,
                        int64_t n_faces, const float *poses, int64_t n_views, int H, int W, double focal, double znear,
                        float *disp, int *face, void *rgb, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh texturing: colours for the points of a mesh baked from the views it was built from, a per-face texture atlas, and the
 * textured mesh rendered back into a camera (beyond the reference: no entry point has a reference call site; csrc/texture.hip,
 * ops.mesh_bake_points / mesh_bake_atlas / mesh_texture_resolve, mesh.bake_texture / colors_from_views / render_textured).
 * The definition, in fp64 and integers with its operation order, is written out in csrc/texture.hip and
 * tests/texture_numpy.py: the cameras and the projection of mvip_raster_* (one definition, csrc/raster_device.h); a view
 * contributes to a point iff the point projects inside the image at z >= znear, faces the camera (cull 1: nrm . (o - p) > 0,
 * cull 0: != 0) and the rasterised disparity D of the same mesh satisfies |D z - 1| <= tol at all four pixels of the bilinear
 * footprint (and masks, if not NULL, is non-zero there); weight = cos^2 of incidence; mode 0 blends by weight, mode 1 takes the
 * view of largest weight.  The atlas: faces 2k and 2k + 1 share a block of (texels + 3)^2 texels, blocks row-major,
 * ceil(sqrt(ceil(F / 2))) per row.  All operands DEVICE memory, dense: images [V,H,W,3] bytes, disp [V,H,W] fp32, masks
 * [V,H,W] bytes or NULL, poses [V,3,4] fp32, verts [Nv,3] fp32, faces [F,3] int32.  Outputs per sample point: rgb 3 bytes,
 * wsum fp32 (the sum of the weights; 0 = no view), best int32 (the view of largest weight or -1).  MVIP_EINVAL before any
 * device call for: a negative count, a count > 2^31 - 1 (3 F for faces), H or W outside 1..16384, texels outside 1..32, a
 * texture side over 16,384, focal or znear not finite and > 0, tol not finite or < 0, cull, mode or order not 0 or 1, a NULL
 * operand that a non-zero count makes necessary.  N = 0, F = 0, V = 0 are valid.  Every launch on the caller's stream.
 * mvip_texture_bake_points: points, normals [N,3] fp32 -> rgb [N,3], wsum [N], best [N].
 * mvip_texture_bake_atlas: one sample point per texel of the atlas [Ht,Wt] of (F, texels), derived from the texel index;
 *   rgb [Ht,Wt,3], wsum [Ht,Wt], best [Ht,Wt]; texels without an owner hold 0 / 0 / -1.  order: how texels map to lanes
 *   (0 texture row-major, 1 block-major), the same output.  flag[0] is cleared, then set to 1 iff a face index lies outside
 *   [0, Nv) (the texels of such a face hold 0 / 0 / -1).
 * mvip_texture_resolve: face [V,H,W] int32 of mvip_raster_resolve for the same mesh, poses and camera -> rgb [V,H,W,3]: the
 *   bilinear value of atlas [Ht,Wt,3] at the winner's perspective-correct barycentrics, 0 where face < 0 or >= F. */
int mvip_texture_bake_points(const float *points, const float *normals, int64_t n_points, const void *images, const float *disp,
                             const void *masks, const float *poses, int64_t n_views, int H, int W, double focal, double znear,
                             double tol, int cull, int mode, void *rgb, float *wsum, int *best, void *stream);
int mvip_texture_bake_atlas(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, int texels, int order,
                            const void *images, const float *disp, const void *masks, const float *poses, int64_t n_views, int H,
                            int W, double focal, double znear, double tol, int cull, int mode, void *rgb, float *wsum, int *best,
                            int *flag, void *stream);
int mvip_texture_resolve(const int *face, const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                         const void *atlas, int texels, const float *poses, int64_t n_views, int H, int W, double focal,
                         double znear, void *rgb, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh-to-mesh distance: the closest point of a triangle mesh to each of N query points on a uniform grid of face lists, and
 * deterministic surface samples (beyond the reference, which has no mesh export: no entry point has a reference call site;
 * csrc/mesh_distance.hip, ops.mesh_face_grid / mesh_closest_point / mesh_sample_faces, evaluate.mesh_distance_metrics).  The
 * definition, in fp64 with its operation order, is written out in csrc/mesh_distance.hip and tests/mesh_distance_numpy.py;
 * the result does not depend on the grid.  All operands DEVICE memory, dense, except box / cells (host): verts [V,3] fp32,
 * faces [F,3] int32; box = (bmin[3], inv[3]) and cells[3] (each 1..512) of the bit grid above.  MVIP_EINVAL (-1 from the size
 * query) before any device call for: a count < 0, V, 3 F, N or a pair / sample count > 2^31 - 1, F = 0 (V = 0), a bad box /
 * cells, k outside 1..1024, a NULL operand that a non-zero count makes necessary.  N = 0 is valid.  Every launch goes on the
 * caller's stream; integer atomics only: the outputs are bit-reproducible.
 * mvip_mesh_distance_grid_count: clears flag[0]; face_offsets [F] 64-bit = the exclusive scan, in face order, of the number of
 *   cells each face's bounding box overlaps (cell range of its fp32 minimum and maximum by the bit grid's rule, clamped to the
 *   grid); total[0] = the number of (cell, face) pairs; flag[0] bit 0: a face index outside [0, V), bit 1: a NaN or infinite
 *   vertex of a face (such a face counts 0 pairs).  total and flag are the caller's one read; a total above 2^31 - 1 is the
 *   caller's error (mvip_mesh_distance_grid_scratch_words and mvip_mesh_distance_grid_fill answer it with -1 / MVIP_EINVAL).
 * mvip_mesh_distance_grid_scratch_words: int32 words of `scratch` of mvip_mesh_distance_grid_fill (8-byte aligned).
 * mvip_mesh_distance_grid_fill: from face_offsets and n_pairs = total[0] of the count for the same mesh and grid:
 *   cell_offsets [n_cells + 1], cell_faces [n_pairs]; cell_faces[cell_offsets[l] : cell_offsets[l+1]] = the faces entered in
 *   linear cell l, ascending.  The lists are those of mvip_mesh_corner_table over the pairs' cell keys.
 * mvip_mesh_distance_query: face [N] (-1 for a query with a NaN or infinite coordinate), point [N,3], dist [N] (NaN there).
 *   stats: NULL, or two 64-bit words that are cleared and receive the number of point-face tests and, summed over the waves,
 *   64 times the tests of the wave's busiest lane (a counting variant; their ratio is the lane utilisation of the face loop).
 * mvip_mesh_sample_faces: the k^2 centroids of the uniform subdivision of every face, face-major: points [F k^2, 3] fp32,
 *   face_of_sample [F k^2] int32, weights [F k^2] fp64 (area(f) / k^2).  Clears flag[0]; bit 0: a face index outside [0, V)
 *   (its samples are 0 with weight 0). */
int mvip_mesh_distance_grid_count(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                                  const int *cells, int64_t *face_offsets, int64_t *total, int *flag, void *stream);
int64_t mvip_mesh_distance_grid_scratch_words(int64_t n_pairs, const int *cells);
int mvip_mesh_distance_grid_fill(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                                 const int *cells, const int64_t *face_offsets, int64_t n_pairs, int *cell_offsets,
                                 int *cell_faces, int *scratch, void *stream);
int mvip_mesh_distance_query(const float *points, int64_t n_points, const float *verts, const int *faces, int64_t n_verts,
                             int64_t n_faces, const float *box, const int *cells, const int *cell_offsets,
                             const int *cell_faces, int64_t n_pairs, int *face, float *point, float *dist, void *stats,
                             void *stream);
int mvip_mesh_sample_faces(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, int k, float *points,
                           int *face_of_sample, double *weights, int *flag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh ray casting: the first face each of N rays hits, occlusion, and per face the number of directions in which it sees
 * nothing (beyond the reference, which has no mesh export: no entry point has a reference call site; csrc/mesh_raycast.hip,
 * ops.mesh_cast_rays / mesh_occluded / mesh_face_openness, mesh.cast_rays / cast_views / face_openness / drop_interior).  The
 * definition -- the watertight ray-triangle test in fp64 with its operation order, the tie rule, invalid rays -- is written out
 * in csrc/mesh_raycast.hip and tests/mesh_raycast_numpy.py; the result does not depend on the grid.  The mesh and its face
 * grid are the operands of mvip_mesh_distance_query (cell_offsets / cell_faces of mvip_mesh_distance_grid_fill for the same
 * box and cells); bounds[6] (HOST) = the fp32 minimum[3] and maximum[3] of the vertices, or any box that holds every face.
 * One launch each on the caller's stream (plus one that clears stats), one thread per ray / per face, no atomics outside the
 * stats: bit-reproducible.  MVIP_EINVAL before any device call for: a count < 0, V, 3 F, 3 N, 4 F or the pair count > 2^31 - 1,
 * F = 0 (V = 0), a bad box / cells, bounds NULL, not finite or with minimum > maximum, any_hit not 0 / 1, n_dirs outside
 * 0..255, max_dist NaN or < 0, a NULL operand that a non-zero count makes necessary.  N = 0 is valid.
 * mvip_mesh_raycast: origins / dirs [N,3] fp32; tmin / tmax [N] fp32 or NULL (then tmin_all / tmax_all for every ray); skip [N]
 *   int32 or NULL (the face that never counts for the ray, -1: none).  face [N] (-1: a miss or an invalid ray), t [N] or NULL
 *   (+inf: a miss, NaN: an invalid ray), bary [N,2] or NULL (the weights of the face's second and third vertex; NaN without a
 *   hit).  any_hit = 1: the traversal stops at the first accepted hit, face is that face and t / bary are its.
 *   stats: NULL, or three 64-bit words that are cleared and receive the number of ray-face tests, summed over the waves 64
 *   times the tests of the wave's busiest lane, and the number of cells visited (a counting variant of the kernel).
 * mvip_mesh_face_openness: directions [K,3] fp32 (DEVICE), counts [4,F] int32 = front_open, front_total, back_open,
 *   back_total per face; the rays (centroid, d_k, 0, max_dist) with the face itself skipped, generated in the kernel.  A face
 *   with an index outside [0, V) gets zeros.  stats as above. */
int mvip_mesh_raycast(const float *origins, const float *dirs, const float *tmin, const float *tmax, float tmin_all,
                      float tmax_all, const int *skip, int64_t n_rays, const float *verts, const int *faces, int64_t n_verts,
                      int64_t n_faces, const float *box, const int *cells, const float *bounds, const int *cell_offsets,
                      const int *cell_faces, int64_t n_pairs, int any_hit, int *face, float *t, float *bary, void *stats,
                      void *stream);
int mvip_mesh_face_openness(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                            const int *cells, const float *bounds, const int *cell_offsets, const int *cell_faces,
                            int64_t n_pairs, const float *directions, int n_dirs, float max_dist, int *counts, void *stats,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * Quantile termination depth of a ray, and agreement / free-space violations of depth maps across views (beyond the
 * reference, which renders only the expected depth and never compares views: no entry point has a reference call site;
 * csrc/ray_depth.hip, csrc/depth_consistency.hip, ops.ray_quantile_depth / depth_consistency, prepare.consistency_mask).
 * One launch each on the caller's stream, no atomics, bit-reproducible.
 * mvip_ray_quantile_depth: z [B,S] ascending along the ray and weights [B,S] DEVICE, levels[Q] HOST, depth [B,Q] DEVICE.
 *   Per ray and level q, in integers and fp64 (shared word for word with tests/ray_depth_numpy.py):
 *     Lq = (int64) floor((double) q 2^40);  W_j = (int64) floor(clamp((double) w_j, 0, 1) 2^40);  C_j = sum_{i<=j} W_i, C_{-1} = 0;
 *     k = the smallest j with C_j >= Lq.  No k: depth = +inf.  k = S-1: depth = z_{S-1}.  Otherwise
 *     f = (double)(Lq - C_{k-1}) / (double) W_k;  depth = (float)((double) z_k + f * ((double) z_{k+1} - (double) z_k)).
 *   A ray with any non-finite weight gets NaN at every level; a non-finite z at the crossing propagates by the arithmetic; a
 *   ray's result does not depend on B or its neighbours.  MVIP_EINVAL before anything is touched for: B < 0, S outside
 *   1..4096, B S > 2^31 - 1, Q outside 1..8, levels NULL, a level outside 0 < q < 1 or with Lq < 1, a NULL device operand
 *   while B > 0.  B = 0: MVIP_OK, no launch.
 * mvip_depth_consistency: disp [V,H,W] fp32 (1 / planar depth), pose [V,3,4] camera-to-world (the camera of mvip_warp_views:
 *   no half-pixel offset, looking down -z), agree / violated [V,H,W] int32, every element written.  In fp64 on the fp32
 *   inputs, with mvip_warp_views' expressions (written out in csrc/depth_consistency.hip and
 *   tests/depth_consistency_numpy.py): a pixel of view n with a finite disparity > 0 is lifted to its world point and
 *   projected into every other view s (t_s, u, v); where t_s > 0, 0 <= u <= W-1, 0 <= v <= H-1 and all four bilinear taps
 *   of view s are finite and > 0, resid = t_s d_s - 1 with d_s the bilinear disparity; agree counts the views with
 *   |resid| <= tol, violated those with resid < -tol (resid > tol: occluded, nothing counted).  Other pixels get 0 / 0.
 *   MVIP_EINVAL for: V < 0, H or W outside 2..16384, focal or tol not finite and > 0, a grid beyond 2^31 - 1 workgroups, a
 *   NULL operand while V > 0.  V = 0: MVIP_OK, no launch; V = 1: all zeros. */
int mvip_ray_quantile_depth(const float *z, const float *weights, int64_t B, int S, const float *levels, int Q, float *depth,
                            void *stream);
int mvip_depth_consistency(const float *disp, const float *pose, int V, int H, int W, float focal, float tol, int *agree,
                           int *violated, void *stream);

/* ------------------------------------------------------------------------------------------
 * Topology of an indexed triangle mesh (beyond the reference, which has no mesh at all: no entry point has a reference call
 * site; csrc/mesh_topology.hip, ops.mesh_edge_table / mesh_components / mesh_boundary_loops / mesh_cap_loops,
 * mesh.topology / keep_components / boundary_loops / close_holes).  The definitions are stated once, in the header comment of
 * csrc/mesh_topology.hip, and restated in tests/mesh_topology_numpy.py.  faces [F,3] int32, 3 F <= 2^31 - 1; half-edge
 * h = 3 f + k runs from faces[f,k] to faces[f,(k+1)%3].  Integer work only (plus one fp64 sum per capped loop): no float
 * atomics, every output bit-reproducible.  The lists are those of mvip_mesh_corner_table, built by the caller; the `*_wg`
 * workspaces hold mvip_mesh_rank_groups(n) words for the n items ranked.  A negative count, 3 F > 2^31 - 1, an output count
 * above its bound or a NULL operand that a non-zero count makes necessary: MVIP_EINVAL before any device call.  F = 0:
 * MVIP_OK, nothing launched (the caller returns empty tensors).  Every launch goes on the caller's stream.
 * mvip_mesh_topology_keys: keys [3F] = min(a, b) of each half-edge, -1 for the half-edges of a face that names a vertex
 *   twice or an index outside [0, V); flag[0] = 1 iff such an index exists, else 0.
 * mvip_mesh_topology_edges_find: offsets [V+1] / items: the lists of `keys` over V lists.  Per half-edge: rep [3F] the lowest
 *   half-edge of its edge (-1: none), hcount / hforward [3F] the edge's half-edges and those of them that run lo -> hi,
 *   twin [3F]; rank [3F] = representatives below h, total[0] = E: the caller's one read.
 * mvip_mesh_topology_edges_emit: edge_of [3F], edges [E,2] = (lo, hi), first / count / forward [E].
 * mvip_mesh_topology_components_label: connectivity 0 = 'edge', 1 = 'vertex'; offsets / corners: the corner table.  parent
 *   [F] = the lowest face of each face's component (-1: degenerate), is_root / rank [F]: workspace, total[0] = C.
 * mvip_mesh_topology_components_emit: labels [F] (1..C by lowest face, 0: degenerate), table [C,6] = faces, vertices, edges,
 *   boundary, non-manifold, inconsistent edges.
 * mvip_mesh_topology_loops_label: ends [V]: workspace; next [3F]; parent [3F] = the lowest half-edge of each boundary
 *   half-edge's loop (-1 off the boundary); is_root / rank [3F]: workspace; total[0] = L.
 * mvip_mesh_topology_loops_emit: loop_of [3F] (-1 off the boundary), first / sizes / closed [L].
 * mvip_mesh_topology_cap_plan: capped [L] = closed and 3 <= size <= max_edges; keys [3F] = the loop of a half-edge of a capped
 *   loop, else -1; loop_rank [L] / he_rank [3F] = capped loops / cap faces below; totals[0] = caps, totals[1] = cap faces.
 * mvip_mesh_topology_cap_emit: loop_offsets [L+1] / loop_items: the lists of those keys over L lists.  new_verts [n_caps,3]
 *   (fp64 mean of the origins in list order, rounded once), new_colors [n_caps,3] or NULL with colors NULL (integer mean
 *   (2 sum + n) / (2 n)), new_faces [n_cap_faces,3] = (b, a, V + cap number) in ascending half-edge order. */
int mvip_mesh_topology_keys(const int *faces, int64_t n_faces, int64_t n_verts, int *keys, int *flag, void *stream);
int mvip_mesh_topology_edges_find(const int *faces, int64_t n_faces, int64_t n_verts, const int *keys, const int *offsets,
                                  const int *items, int *rep, int *hcount, int *hforward, int *twin, int *wg, int *rank,
                                  int64_t *total, void *stream);
int mvip_mesh_topology_edges_emit(const int *faces, int64_t n_faces, const int *rep, const int *hcount, const int *hforward,
                                  const int *rank, int64_t n_edges, int *edge_of, int *edges, int *first, int *count,
                                  int *forward, void *stream);
int mvip_mesh_topology_components_label(const int *faces, int64_t n_faces, int64_t n_verts, int connectivity, const int *rep,
                                        const int *offsets, const int *corners, int *parent, int *is_root, int *wg, int *rank,
                                        int64_t *total, void *stream);
int mvip_mesh_topology_components_emit(const int *faces, int64_t n_faces, int64_t n_verts, const int *parent, const int *rank,
                                       int64_t n_components, const int *rep, const int *hcount, const int *hforward,
                                       const int *offsets, const int *corners, int *labels, int *table, void *stream);
int mvip_mesh_topology_loops_label(const int *faces, int64_t n_faces, int64_t n_verts, const int *rep, const int *hcount,
                                   const int *offsets, const int *corners, int *ends, int *next, int *parent, int *is_root,
                                   int *wg, int *rank, int64_t *total, void *stream);
int mvip_mesh_topology_loops_emit(int64_t n_faces, const int *parent, const int *rank, const int *next, int64_t n_loops,
                                  int *loop_of, int *first, int *sizes, int *closed, void *stream);
int mvip_mesh_topology_cap_plan(int64_t n_faces, const int *loop_of, int64_t n_loops, const int *sizes, const int *closed,
                                int64_t max_edges, int *capped, int *keys, int *loop_wg, int *loop_rank, int *he_wg,
                                int *he_rank, int64_t *totals, void *stream);
int mvip_mesh_topology_cap_emit(const float *verts, const void *colors, const int *faces, int64_t n_verts, int64_t n_faces,
                                int64_t n_loops, const int *keys, const int *capped, const int *loop_rank, const int *he_rank,
                                const int *loop_offsets, const int *loop_items, int64_t n_caps, int64_t n_cap_faces,
                                float *new_verts, void *new_colors, int *new_faces, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh voxelisation: an indexed triangle mesh as a bit grid in the convention of the occupancy / region grids above, as the
 * cells its faces touch (conservative) and as the cells inside it (column parity from up to three axes with a majority vote)
 * (beyond the reference, which has no mesh export: no entry point has a reference call site; csrc/mesh_voxel.hip,
 * ops.mesh_voxelize_surface / mesh_voxelize_solid, mesh.voxelize, Region.from_mesh, OccupancyGrid.from_mesh).  The
 * definitions -- lattice coordinates, the snapped integer coverage with its ownership rule, the crossing cell, the exact
 * triangle-box overlap with its margin -- are written out in csrc/mesh_voxel.hip and tests/voxel_numpy.py; everything is
 * fp64 and integers, every mark an integer OR / XOR: the result does not depend on the order of the atomics.
 * box = (bmin[3], inv[3]) and cells[3] in HOST memory as for the grids above; words [(cx cy cz + 31) / 32] int32.
 * axes: 0, 1, 2 = the column axis x, y, z alone, 3 = all three with the majority.  counters [5] int32 (DEVICE): [0] a flag,
 * non-zero when a face index lies outside [0, Nv) (that face is dropped), [1] the dropped faces, [2..4] the columns of odd
 * total parity per axis (0 for an axis not walked); mvip_voxel_surface and mvip_voxel_crossings clear all five.
 * scratch: mvip_voxel_scratch_words(cells, axes) int32 words (-1 for bad arguments), the crossing grids of the walked axes:
 * per axis [cx, cy, (cz + 31) / 32] words, bit iz & 31 of word iz >> 5 of row (ix, iy).
 * Every launch on the caller's stream.  MVIP_EINVAL before any device call for: a NULL operand (verts / faces only where
 * their count is non-zero), a negative count, Nv or 3 F > 2^31 - 1, cells outside 1..512, a non-finite or non-positive inv, a
 * non-finite bmin, axes outside 0..3.  F = 0 and Nv = 0 are valid and give an all-clear grid.
 * mvip_voxel_surface: clears words and counters, then one thread per face ORs the cells the face overlaps into words.
 * mvip_voxel_crossings: clears scratch and counters, then one thread per (face, walked axis) XORs the crossing bits.
 * mvip_voxel_fill: the prefix parity of scratch along each walked axis in place (counters [2..4] receive the odd columns),
 *   then one thread per word of words writes the single axis or the majority. */
int64_t mvip_voxel_scratch_words(const int *cells, int axes);
int mvip_voxel_surface(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                       const int *cells, int *words, int *counters, void *stream);
int mvip_voxel_crossings(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                         const int *cells, int axes, int *scratch, int *counters, void *stream);
int mvip_voxel_fill(int *scratch, const int *cells, int axes, int *words, int *counters, void *stream);

/* ------------------------------------------------------------------------------------------
 * Signed mesh distance: the closest point of mvip_mesh_distance_query with a sign from the angle-weighted pseudonormal of the
 * closest feature (Baerentzen and Aanaes 2005), for N points or for the points of a lattice generated in the kernel (beyond
 * the reference, which has no mesh export: no entry point has a reference call site; csrc/mesh_sdf.hip,
 * ops.mesh_vertex_pseudonormals / mesh_signed_distance / mesh_signed_distance_lattice, mesh.signed_distance / sdf_grid /
 * remesh, the `margin` of Region.from_mesh / OccupancyGrid.from_mesh).  The definition -- the feature code, the three
 * pseudonormals, the sign, the band, the lattice coordinates -- is written out in csrc/mesh_sdf.hip and
 * tests/mesh_sdf_numpy.py; the result does not depend on the grid.  The mesh and its face grid are the operands of
 * mvip_mesh_distance_query.  One launch each on the caller's stream, one thread per vertex / per query, no atomics:
 * bit-reproducible given pseudonormals.  MVIP_EINVAL before any device call for: a count < 0, V, 3 F, N or the pair count
 * > 2^31 - 1, F = 0 (V = 0) in the query, a bad box / cells, max_dist NaN or < 0, a lattice with a count < 1, a non-finite
 * lo or a step that is not finite and > 0, `point` given with 3 N > 2^31 - 1, a NULL operand that a non-zero count makes
 * necessary.  N = 0 is valid.
 * mvip_mesh_vertex_pseudonormals: offsets [V+1] / corners [3F]: the corner table of mvip_mesh_corner_table over faces.
 *   pseudonormals [V,3] fp64 = per vertex the sum, in list order, of angle x unit face normal over its corners (unnormalised;
 *   zeros for a vertex without a corner; a corner of a face with an index outside [0, V) adds nothing).  F = 0 is valid.
 * mvip_mesh_signed_distance: points [N,3] fp32, or NULL with lattice_lo[3], lattice_h[3] (fp32) and lattice_counts[3] in HOST
 *   memory: then N must be their product and point (i, j, k), k fastest, is fp32(fp32(i) h) + lo per axis.  twin [3F] of
 *   mvip_mesh_topology_edges_find; pseudonormals [V,3] fp64.  max_dist: the band B (+inf: none).  sdist [N] fp32 (negative
 *   inside a closed, outward-oriented mesh), face [N]; point [N,3] and feature [N] (0 interior, 1..3 edge ab / bc / ca, 4..6
 *   vertex a / b / c of `face`) or NULL.  A query with a NaN or infinite coordinate, or farther than B: face -1, feature -1,
 *   sdist and point NaN.  stats: NULL, or two 64-bit words as for mvip_mesh_distance_query (a counting variant of the kernel). */
int mvip_mesh_vertex_pseudonormals(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const int *offsets,
                                   const int *corners, double *pseudonormals, void *stream);
int mvip_mesh_signed_distance(const float *points, const float *lattice_lo, const float *lattice_h, const int *lattice_counts,
                              int64_t n_points, const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                              const float *box, const int *cells, const int *cell_offsets, const int *cell_faces,
                              int64_t n_pairs, const int *twin, const double *pseudonormals, double max_dist, float *sdist,
                              int *face, float *point, int *feature, void *stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MVIP_NERF_H */
