/* libsvolsdf_hip.so -- C-ABI of the MI355X-native S-VolSDF volume-rendering hot path.
 *
 * The reference (cvlab-stonybrook/s-volsdf) is pure Python: it has no FFI of its own, so each entry point
 * below names the reference function (file:line, relative to the reference root) whose arithmetic it
 * replaces.  The binding a maintainer adds on the reference side is the ctypes stub shown in INTEGRATION.md
 * (s-volsdf_amd/svs_hip/lib.py is that stub, s-volsdf_amd/volsdf/ the drop-in classes that call it).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float32 / int32 data unless stated otherwise; tensors are
 *     contiguous row-major; `hip_stream` is a hipStream_t (NULL = default stream);
 *   - calls are asynchronous (stream-ordered); none allocates, frees or synchronises; all outputs and
 *     workspaces are caller-allocated (size queries: *_bytes);
 *   - return 0 on success, < 0 for an argument/shape error, > 0 = hipError_t of a failed launch;
 *     svs_last_error_string() describes the last failure on the calling thread.
 */
#ifndef SVOLSDF_HIP_H
#define SVOLSDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* This file is the one declaration of the ABI: every translation unit of the library is compiled against it
 * (csrc/svs_common.h includes it), and the Python binding (svs_hip/lib.py) derives its ctypes table, its two Structure
 * classes and its constants from this text.  It therefore keeps to a small subset of C: #define of an integer, one enum,
 * typedef struct, and prototypes over int, float, double, size_t, long long and pointers. */

/* Return codes (see "Conventions"): 0, a HIP error code (> 0), or one of these. */
#define SVS_EINVAL (-1)    /* an argument: a null pointer, a misaligned buffer, a count or a setting out of range */
#define SVS_ESHAPE (-2)    /* a size the kernels do not handle */
#define SVS_ENOCONV (-3)   /* an iteration did not settle within its round limit (svs_mesh_components) */
#define SVS_EOVERFLOW (-4) /* an operand of the fp16x2 3x3 convolution does not fit fp16 (svs_conv3x3_mfma, svs_lpips_score) */

/* Marks a pointer parameter as host memory read or written during the call -- a small array of parameters, a table of
 * device pointers, a result the host reads at once.  Unmarked pointers follow the convention above: device memory, or an
 * address the call only hands on.  (Eight pointer tables that are host memory too travel unmarked: `weights`, `biases` and
 * `wfrags` of svs_featurenet_fpn / _fpn2 / _unet, which bindings pass as plain addresses.)  Expands to nothing. */
#define SVS_HOST

/* ABI version: svs_version() returns SVS_ABI_VERSION.  101 (round 6): svs_set_deterministic / svs_get_deterministic,
 * svs_conv2d_mfma*, svs_featurenet_fpn2 added.  100 -> 101 also marks the argument lists that changed during round 5
 * without a version signal: svs_sdf_bwd_a lost `a2max`, svs_sdf_bwd_b gained `ubuf`, and in
 * fp16x2 svs_sdf_outputs writes records BEHIND gbuf's 8 blocks -- size gbuf with svs_sdf_gbuf_bytes(), not svs_sdf_hbuf_bytes().
 * A host binding should refuse a library whose version differs from the one it was written against (svs_hip/lib.py, which
 * reads the macro from this file, does). */
#define SVS_ABI_VERSION 101
int svs_version(void);
const char* svs_last_error_string(void);

/* Deterministic accumulation of the weight gradients (process-wide, off by default; returns the previous setting).
 * The reference's CPU path (torch autograd on one thread, volsdf/vsdf.py:21) gives the same gradient for the same inputs
 * every time; svs_wgrad / svs_wgrad_multi / svs_lin8_row0_grad add their workgroups' partial sums with float atomics, in
 * arrival order.  With the switch on, the workgroups that add into one accumulator do so in launch order (csrc/svs_ticket.h):
 * one fixed summation order, bit-identical results run to run, at the cost of serialised flushes.  Launches that add into the
 * same accumulator must then be ordered by the caller (one stream). */
int svs_set_deterministic(int on);
int svs_get_deterministic(void);

/* ---- a1  rays ---------------------------------------------------------------------------------------
 * rend_util.get_camera_params + lift (volsdf/utils/rend_util.py:60-95,143-156) and the depth_scale of
 * VolSDFNetwork.forward (volsdf/model/network.py:213-217).
 * uv (n_rays,2) pixel (x,y); pose (4,4) camera-to-world; intrinsics (4,4).
 * -> ray_dirs (n_rays,3) unit, cam_loc (3), depth_scale (n_rays) */
int svs_rays_from_uv(const float* uv, const float* pose, const float* intrinsics, int n_rays, float* ray_dirs,
                     float* cam_loc, float* depth_scale, void* hip_stream);

/* The eikonal points of a train-mode forward (volsdf/model/network.py:258-266; BG model: network_bg.py:128-138):
 * points[0..n_rays) = uniform_points (the host's uniform draws in the bounding sphere, (n_rays,3)),
 * points[n_rays + r] = cam_loc + z_eik[r] * ray_dirs[r] (the sampler's extra depth per ray, ray_sampler.py:200-208).
 * points: DEVICE float[2 n_rays][3], the tail of the point list the fused SDF launch evaluates. */
int svs_eikonal_points(const float* uniform_points, const float* cam_loc, const float* z_eik, const float* ray_dirs,
                       int n_rays, float* points, void* hip_stream);
/* The small per-step inputs of VolOpt.train_step (volsdf/vsdf.py:196-204: `model_input[...].cuda()`, and the train-mode
 * draws of the sampler): `bytes` (a multiple of 4) from a PINNED HOST buffer (hipHostMalloc / torch pin_memory: mapped
 * into the device's address space) to device memory by a kernel on hip_stream; both 16-byte aligned.  The host must not
 * rewrite the buffer before the launch has run (the callers keep a ring of staging buffers and an event per slot). */
int svs_stage_in(const void* pinned_host, void* device, size_t bytes, void* hip_stream);
/* BG model (volsdf/model/network_bg.py:60-62): z (n_rays, n) -> head (n_rays, n - 1) = z[:, :-1] dense, last (n_rays) =
 * z[:, -1] (the sphere exit depth), one launch. */
int svs_split_last(const float* z, int n_rays, int n, float* head, float* last, void* hip_stream);

/* ---- a5/a6  weight packing --------------------------------------------------------------------------
 * Weight-norm materialisation w = g*v/||v|| (nn.utils.weight_norm, volsdf/model/network.py:64-65) and the
 * permutation into the MFMA consumption order.  weight_v/weight_g/bias: HOST arrays of 9 (SDF) / 5 (radiance)
 * device pointers in layer order, shapes as in the checkpoint (`implicit_network.lin{l}.weight_v` ...);
 * weight_g == NULL for networks without weight-norm.  workspace: svs_pack_workspace_bytes().
 * which: 0 SDF forward, 1 SDF full (forward + feature head + input-gradient pass), 2 SDF training backward,
 *        3 radiance forward, 4 radiance backward (5..8: the background networks, see below).  Like every entry point,
 *        svs_pack_stream allocates and copies nothing on its own: the stream's chunk table (<= 2.2 KB) travels in the
 *        kernel arguments.
 * precision: how the kernels that consume the stream evaluate the layer products (the same value is passed to them):
 *   SVS_MMA_F32   v_mfma_f32_32x32x2_f32 on float32 operands (exact float32 products);
 *   SVS_MMA_F16X2 v_mfma_f32_32x32x16_f16 on operands split into two fp16 pieces, a = hi + mid, three products
 *                 per term (22-bit significands, float32 accumulation: float32-class accuracy at 2.8x the speed;
 *                 operands must stay below 65504) -- forward AND backward: the activation blocks the training backward
 *                 keeps in memory hold both pieces, parameter gradients agree with float64 autograd to < 1e-5 of a
 *                 tensor's largest entry (the float32-MFMA kernels: 3e-6);
 *   SVS_MMA_F16X2_HALF  the same kernels with the gradient-only blocks of the backward (ghat, u, a2, abar, zbar, fbar)
 *                 stored as ONE fp16 piece under a per-point scale and one-product weight-gradient GEMMs: half the
 *                 backward's block bytes, parameter gradients 2e-4 ... 8e-4 off (a mixed-precision training mode; the
 *                 forward is identical).  Packs the same streams as SVS_MMA_F16X2.
 * Stream sizes do not depend on the precision. */
enum { SVS_MMA_F32 = 0, SVS_MMA_F16X2 = 1, SVS_MMA_F16X2_HALF = 2 };
size_t svs_stream_bytes(int which);
int svs_pack_stream(int which, int precision, const float* const SVS_HOST* weight_v,
                    const float* const SVS_HOST* weight_g, const float* const SVS_HOST* bias, float* workspace,
                    float* stream_out, void* hip_stream);
size_t svs_pack_workspace_bytes(void);

/* ---- a5  SDF MLP ------------------------------------------------------------------------------------
 * Sample positions of a launch = the ray samples cam + z*dir (n_rays x S, row-major, may be 0 rays) followed by
 * n_points explicit points (may be 0).  cam_stride 0 = one camera centre, 3 = one per ray.
 *
 * svs_sdf_vals: ImplicitNetwork.get_sdf_vals (volsdf/model/network.py:125-131) -> sdf (P).
 *   sphere clamp min(sdf, scale*(radius-|x|)) on points [0, clamp_n) (clamp_n < 0: all) when radius > 0.
 *   gate: optional device flags, one per group of gate_points points (a multiple of 128; <= 0: one group), gate_stride
 *   ints apart: the points of a group are skipped when its flag is 0 (sampler rounds, one flag per convergence
 *   group of rays). */
int svs_sdf_vals(const float* points, int n_points, const float* cam, int cam_stride, const float* dirs, const float* z,
                 int S, int n_rays, const float* stream, int precision, float sphere_radius, float sphere_scale,
                 int clamp_n, float* sdf, const int* gate, int gate_points, int gate_stride, void* hip_stream);
/* svs_sdf_outputs: ImplicitNetwork.get_outputs (network.py:105-123) and .gradient (:90-103):
 *   sdf (P), grad = d sdf/dx (P,3), feat_tiles (svs_feat_tiles_bytes; wave-tile layout, may be NULL),
 *   hbuf (svs_sdf_hbuf_bytes): the activations h_1..h_8 kept for the gradient pass / training backward;
 *   gbuf (svs_sdf_gbuf_bytes, may be NULL): ghat_l = g(h_{l+1}) * softplus'(a_l), l = 0..7, of the gradient pass, and -- fp16x2
 *   precisions -- behind the 8 blocks of every tile their records [1.0 x 32][max_r |ghat_l| of point 0..31] (the layout of
 *   "Records" below), which svs_sdf_bwd_b reads; clamp_mask (P bytes, may be NULL): 1 where the sphere clamp is active -- both
 *   are only needed by the training backward. */
size_t svs_sdf_hbuf_bytes(int n_points_total);
size_t svs_feat_tiles_bytes(int n_points_total);
int svs_sdf_outputs(const float* points, int n_points, const float* cam, int cam_stride, const float* dirs,
                    const float* z, int S, int n_rays, const float* stream, int precision, float sphere_radius,
                    float sphere_scale, int clamp_n, float* sdf, float* grad, float* feat_tiles, float* hbuf,
                    float* gbuf, unsigned char* clamp_mask, void* hip_stream);
/* feature vectors in row-major (P,256), for callers outside the fused pipeline */
int svs_tiles_to_rows(const float* tiles, int n_points, int precision, float* rows, void* hip_stream);

/* ---- a6  radiance MLP -------------------------------------------------------------------------------
 * RenderingNetwork.forward, mode 'idr' (volsdf/model/network.py:170-190): rgb (P,3) =
 * sigmoid(MLP(cat[x, PE1(view), normal, feature])).  view_dirs: (n_rays,3) when view_S == S, (P,3) when 0. */
int svs_rgb_eval(const float* points, int n_points, const float* cam, int cam_stride, const float* dirs, const float* z,
                 int S, int n_rays, const float* normals, const float* view_dirs, int view_S, const float* feat_tiles,
                 const float* stream, int precision, float* rgb, float* rbuf, void* hip_stream);
/* rbuf (svs_rgb_rbuf_bytes, may be NULL): post-ReLU activations + the 16 extra input rows, kept for svs_rgb_bwd */
size_t svs_rgb_rbuf_bytes(int n_points_total);

/* ---- a2/a3/a4  error-bounded sampler ------------------------------------------------------------------
 * ErrorBoundSampler.get_z_vals / get_error_bound, UniformSampler.get_z_vals
 * (volsdf/model/ray_sampler.py:22-43, 67-219, 221-229).  One call sequence per batch:
 *   svs_sampler_init;  for round i < max_iters: svs_sdf_vals(samples -> samples_sdf, gate = ctl.active[i]),
 *   svs_sampler_round(phase 0), svs_sampler_round(phase 1);   max_iters == 0: svs_sampler_round(phase 2).
 * Buffers: z, sdf (n_rays, svs_sampler_cap()); samples, samples_sdf (n_rays, svs_sampler_max_new());
 * beta, far (n_rays); ctl (svs_sampler_ctl_bytes(n_rays, group_rays): per convergence group of group_rays rays
 * (<= 0: all rays form one group) int conv_flag[8], active[8], final_round -- the reference tests convergence per
 * forward call, i.e. per chunk of split_n_pixels rays; one launch can cover many chunks); err_flag (1 int,
 * set on a bounding-sphere miss).  Random draws (train mode) are inputs: jitter (n_rays,n_eval),
 * u_final (n_rays,n_final), extra_idx (n_extra int), eik_idx (n_rays int); NULL = eval mode.
 * beta0 = |*beta_param| + beta_min is read on the device (volsdf/model/density.py:28-30). */
size_t svs_sampler_ctl_bytes(int n_rays, int group_rays);
int svs_sampler_ctl_stride(void);   /* ints per group record; active[i] is int 8 + i of a record */
int svs_sampler_cap(void);
int svs_sampler_max_new(void);
int svs_sampler_init(const float* cam, int cam_stride, const float* dirs, int n_rays, int n_eval, float near_, float far_,
                     int sphere_far, float sphere_radius, const float* jitter, float inv_4log, int max_iters,
                     float* samples, float* beta, float* far_out, void* ctl, int group_rays, int* err_flag,
                     void* hip_stream);
int svs_sampler_round(int phase, int n_rays, int round, int max_iters, int n_eval, int n_final, int n_extra,
                      const float* beta_param, float beta_min, float eps, int beta_iters, float add_tiny, float near_,
                      const float* far_, float* z, float* sdf, float* beta, float* samples, const float* samples_sdf,
                      void* ctl, int group_rays, const float* u_final, const int* extra_idx, const int* eik_idx, float* z_final,
                      float* z_eik, int* dbg_samples_idx, int* dbg_inds, float* dbg_cdf, float* dbg_weights,
                      void* hip_stream);

/* ---- a8  alpha compositing ----------------------------------------------------------------------------
 * VolSDFNetwork.volume_rendering (volsdf/model/network.py:281-295) and the reductions of :237-256,270-276.
 * z (R,S), sdf (R*S), rgb (R*S,3), normals (R*S,3) or NULL, depth_scale (R) -> weights (R,S), rgb_values (R,3),
 * depth_values (R), depth_vals (R,S), normal_map (R,3) or NULL. */
int svs_composite(int n_rays, int n_samples, const float* z, const float* sdf, const float* rgb, const float* normals,
                  const float* depth_scale, const float* beta_param, float beta_min, float* weights, float* rgb_values,
                  float* depth_values, float* depth_vals, float* normal_map, void* hip_stream);

/* a8 backward: gradients of a scalar loss through the compositing (hand-derived reverse pass of network.py:281-295
 * and :237-243).  d_weights / d_depth_values may be NULL.  -> d_sdf (R*S), d_rgb (R*S,3), d_beta_param (1) =
 * d loss / d density.beta; d_beta_ray (R) is workspace. */
int svs_composite_bwd(int n_rays, int n_samples, const float* z, const float* sdf, const float* rgb,
                      const float* depth_scale, const float* beta_param, float beta_min, const float* d_rgb_values,
                      const float* d_weights, const float* d_depth_values, float* d_sdf, float* d_rgb,
                      float* d_beta_ray, float* d_beta_param, void* hip_stream);

/* ---- a9 (config 4)  inverted-sphere background model, VolSDFNetworkBG (volsdf/model/network_bg.py) -----------
 * precision = SVS_MMA_F16X2 / SVS_MMA_F16X2_HALF (csrc/svs_bg_h2.hip; selects the format of the blocks kept for / written by
 * the backward) or SVS_MMA_F32 (csrc/svs_bg_f32.hip: float32 MFMAs, every block a float32 block; same buffer sizes).  Streams: svs_pack_stream which = 5 (bg implicit forward), 6 (bg implicit backward), 7 (bg radiance
 * forward), 8 (bg radiance backward); weight arrays of 9 / 2 device pointers, weight_g = NULL (no weight-norm).
 *   svs_bg_points     UniformSampler(1,0,n_bg,far=1) * (1/radius), flipped (ray_sampler.py:22-43,215-216;
 *                     network_bg.py:79-82) + depth2pts_outside (:182-214): jitter (n_rays,n_bg) train draws or NULL
 *                     -> z_bg (n_rays,n_bg), pts (n_rays*n_bg,4), depth_real (n_rays,n_bg)
 *   svs_bg_sdf_eval   bg_implicit_network (:85-88): pts (P,4) -> out0 (P) = output[:,0] (density = |out0|),
 *                     feat_tiles; training: hbuf (svs_sdf_hbuf_bytes) + ghat7 + pebuf (svs_block_bytes(P,1) each), all
 *                     or none
 *   svs_bg_rgb_eval   bg_rendering_network, mode 'nerf' (:91-93): view_dirs (n_rays,3) with view_S points per ray
 *                     (or (P,3) with view_S = 0) -> rgb (P,3); rbuf (svs_bg_rbuf_bytes, training) or NULL
 *   svs_composite_bg  volume_rendering / bg_volume_rendering and the composition (:76-125,147-180) */
int svs_bg_points(const float* cam, int cam_stride, const float* dirs, int n_rays, int n_bg, const float* jitter,
                  float radius, float* z_bg, float* pts, float* depth_real, void* hip_stream);
int svs_bg_sdf_eval(const float* pts, int n_points, const float* stream, int precision, float* out0, float* feat_tiles,
                    float* hbuf, float* ghat7, float* pebuf, void* hip_stream);
size_t svs_bg_rbuf_bytes(int n_points);
int svs_bg_rgb_eval(int n_points, const float* view_dirs, int view_S, const float* feat_tiles, const float* stream,
                    int precision, float* rgb, float* rbuf, void* hip_stream);
/* training backward of the background networks (per-point scaling as in the fg sweeps; absmax: 3 floats, caller
 * zeroes once per step: [0] max |abar|, [1] max |zbar|, [2] max |feat_bar|):
 *   svs_bg_rgb_bwd  d_rgb (P,3), rgb (P,3), rbuf, stream (which = 8) -> zbuf (svs_block_bytes(P,2): zbar_0, zbar_1 per
 *                   tile; ZERO-INITIALISED by the caller once), feat_bar (svs_block_bytes(P,1))
 *   svs_bg_sdf_bwd  d_out0 (P), feat_bar, hbuf, ghat7, stream (which = 6) -> abuf (8 blocks/tile), sbar_out (padded P);
 *                   n_points must be a multiple of 32 (n_rays * 32 is)
 * Weight gradients: svs_wgrad_multi with A = abuf / feat_bar / zbuf blocks and B = pebuf / hbuf / rbuf blocks;
 * svs_lin8_row0_grad with ubuf = NULL; svs_unpack_wgrad maps 3 (bg lin4) and 4 (bg radiance lin0). */
int svs_bg_rgb_bwd(int n_points, const float* d_rgb, const float* rgb, const float* rbuf, const float* stream, int precision,
                   float* zbuf, float* feat_bar, float* absmax, void* hip_stream);
int svs_bg_sdf_bwd(int n_points, const float* d_out0, const float* feat_bar, const float* hbuf, const float* ghat7,
                   const float* stream, int precision, float* abuf, float* sbar_out, float* absmax, void* hip_stream);
int svs_composite_bg(int n_rays, int n_samples, int n_bg, const float* z, const float* z_max, const float* sdf,
                     const float* rgb, const float* normals, const float* depth_scale, const float* beta_param,
                     float beta_min, const float* z_bg, const float* bg_out0, const float* bg_rgb, const float* bg_depth,
                     float* weights, float* bg_trans, float* bg_weights, float* rgb_values, float* depth_values,
                     float* depth_values_all, float* depth_vals, float* normal_map, void* hip_stream);
/* backward of svs_composite_bg: d_weights / d_depth_values (gradient of the fg depth, network_bg.py:109-110) /
 * d_depth_all (gradient of depth_values_all, :105-107 -- what VolSDFLoss's sparsity term reads, loss.py:72-73; needs
 * bg_depth) may be NULL; d_beta_ray (n_rays) is workspace */
int svs_composite_bg_bwd(int n_rays, int n_samples, int n_bg, const float* z, const float* z_max, const float* sdf,
                         const float* rgb, const float* depth_scale, const float* beta_param, float beta_min,
                         const float* z_bg, const float* bg_out0, const float* bg_rgb, const float* d_rgb_values,
                         const float* d_weights, const float* d_depth_values, const float* d_depth_all,
                         const float* bg_depth, float* d_sdf, float* d_rgb,
                         float* d_bg_out0, float* d_bg_rgb, float* d_beta_ray, float* d_beta_param, void* hip_stream);

/* ---- a12  weight-gradient contraction of the training backward ---------------------------------------------------
 * dW[256][ldw] += sum over points of A(:,p) B(:,p)^T for one or two operand pairs stored as wave-tile activation
 * blocks (128*64 floats per 32 points; s* = floats between consecutive blocks).  b_extra: optional 16 extra B rows
 * per block (dW columns
 * 256..271, ldw >= 272: the radiance MLP's first layer).  db[256] += row sums of pair 0's A (bias gradient).
 * dW / db are accumulated with float atomics: the caller zeroes them.
 * precision SVS_MMA_F16X2 / _HALF: the gradient-like operands (A of pair 0, B of pair 1) are scaled blocks: every point
 * carries a power-of-two scale, kept in the block's 64-float RECORD (rec0: records of a0's blocks, rec1: of b1's; [tile][64]
 * floats, see the buffer layout below); the contraction re-scales them to one power of two per launch derived from
 * *absmax (device float: their maximum magnitude, published by the fp16x2 sweeps below; NULL = operands are unscaled and
 * no records are read).  SVS_MMA_F16X2 multiplies both fp16 pieces of both operands (three products), _HALF the hi
 * pieces. */
typedef struct svs_wgrad_job {
  const float *a0, *b0; long long sa0, sb0;   /* pair 0 */
  const float *a1, *b1; long long sa1, sb1;   /* pair 1, a1 == NULL: one pair */
  const float* b_extra; long long s_extra;    /* optional 16 extra B rows of pair 0 (1024 floats per tile) */
  int n_points, ldw;
  float *dW, *db;                             /* db may be NULL */
  const float* absmax;                        /* fp16x2 scaling, may be NULL */
  const float *rec0, *rec1;                   /* fp16x2 with absmax: scale records of a0's / b1's blocks, 64 floats per tile */
} svs_wgrad_job;
/* The weight gradients of several layers (<= 20 jobs, one with b_extra counts twice) in one call.  SVS_MMA_F16X2: ONE
 * launch, ~one workgroup per CU in total, split between the jobs in proportion to their work (so each layer flushes
 * ~256/n_jobs partial sums instead of 256); SVS_MMA_F32: one launch per job. */
int svs_wgrad_multi(const svs_wgrad_job* jobs, int n_jobs, int precision, void* hip_stream);
/* single job */
int svs_wgrad(const float* a0, const float* b0, long long sa0, long long sb0, const float* a1, const float* b1,
              long long sa1, long long sb1, const float* b_extra, long long s_extra, int n_points, int precision,
              const float* absmax, const float* rec0, const float* rec1, float* dW, int ldw, float* db, void* hip_stream);

/* ---- a12  training backward of the fused MLPs (hand-written reverse mode; the reference uses torch.autograd,
 * loss.backward() at volsdf/vsdf.py:215, incl. the double backward through network.py:115-121) -------------------
 * Buffers are wave-tile activation blocks; svs_block_bytes(n_points, k) = bytes of k blocks per 32-point tile INCLUDING
 * their records (below).
 * Layout of the multi-block buffers (hbuf, gbuf, ubuf, a2buf, abuf, rbuf, zbuf): [block][wave tile][128*64 floats], the tile
 * count T padded to whole workgroups (T = 4 * ceil(n_points / 128)): block b of tile t starts at float (b * T + t) *
 * 8192 -- what a launch touches at one time and what one weight-gradient job reads is contiguous (for svs_wgrad:
 * pointer = buffer + b * T * 8192, stride 8192).  The radiance buffers use the same layout: rbuf = [4 blocks][tile]
 * followed by the 1024-float extras of every tile, zbuf = [5 blocks][tile]; the background networks' two small
 * buffers (bg rbuf, bg zbuf) are [tile][block].
 * Records (fp16x2): a buffer of k scaled blocks per tile (ubuf, a2buf, abuf, zbuf, feat_bar) is followed by k * T records
 * of 64 floats ([scale of point 0..31][max |value| of point 0..31]), in the order of the slots: the record of block b of
 * tile t is at float k * T * 8192 + (b * T + t) * 64 (also for bg zbuf, whose slots are [tile][block]).
 *   svs_rgb_bwd : d_rgb (P,3), rgb (P,3), rbuf, radiance backward stream (svs_pack_stream which=4)
 *                 -> zbuf (5 blocks/tile, ZERO-INITIALISED by the caller once), feat_bar (1 block/tile), d_normals (P,3)
 *   svs_sdf_bwd_a: second-order sweep (forward mode: u_0 = J_PE nbar, u_{l+1} = (W_l u_l) s'(a_l)).  points/rays as in
 *                 svs_sdf_outputs; d_grad (P,3) = dL/d(d sdf/dx); hbuf, gbuf from svs_sdf_outputs; stream = SDF training
 *                 stream (which=2) -> ubuf (9 blocks/tile), pebuf (1), and with SVS_MMA_F32 the second-order source blocks
 *                 a2_l = (W_l u_l) ghat_l 100 (1 - s'(a_l)) -> a2buf (8).  fp16x2 (since round 5): gbuf is not read and a2buf
 *                 not written (both may be NULL); the second half of the record of u_{l+1} holds max_r |(W_l u_l)| 100 (1 - s')
 *   svs_sdf_bwd_b: backprop.  d_sdf (P) or NULL, feat_bar for the first n_feat_points points (multiple of 32)
 *                 -> abuf (8 blocks/tile), sbar_out (32 floats per tile).  SVS_MMA_F32 reads a2buf (ubuf may be NULL); fp16x2
 *                 re-forms a2_l = u_{l+1} ghat_l 100 (1 - s') / s' from ubuf (with pass A's records) and gbuf (with the records
 *                 svs_sdf_outputs wrote behind it: max_r |ghat_l| per point; svs_sdf_gbuf_bytes) -- a2buf may be NULL: 8 KB
 *                 per point less HBM traffic than storing a2 in pass A and reading it here
 *   svs_lin8_row0_grad: out257[0..255] += dL/dW8[0,:], out257[256] += dL/db8[0] (caller zeroes)
 *   precision SVS_MMA_F16X2 (streams packed with the same precision): every point carries its own power-of-two
 *                 scale through the sweeps (gradients are far below fp16's range); all buffers hold true float32
 *                 values.  Extra arguments, NULL for SVS_MMA_F32: absmax (3 floats, caller zeroes once per step:
 *                 [0] max |abar|,|u|, [1] max |zbar|, [2] max |feat_bar| -- the scales of svs_wgrad).
 *   svs_unpack_wgrad: kernel-order dW (from svs_wgrad) -> parameter gradients incl. weight-norm backward
 *                 (w = g v/|v|, network.py:64-65).  map: 0 identity, 1 SDF lin4 (skip splice, 1/sqrt2),
 *                 2 radiance lin0, 3 bg lin4, 4 bg radiance lin0.  row_off: first parameter row covered by dWk (SDF lin8: 1, with row0 = out257). */
size_t svs_block_bytes(int n_points, int blocks_per_tile);
size_t svs_rgb_zbuf_bytes(int n_points);
size_t svs_sdf_ubuf_bytes(int n_points);
size_t svs_sdf_gbuf_bytes(int n_points);      /* gbuf of svs_sdf_outputs: 8 blocks per tile + their records */
int svs_rgb_bwd(int n_points, const float* d_rgb, const float* rgb, const float* rbuf, const float* stream, int precision,
                float* zbuf, float* feat_bar, float* d_normals, float* absmax, void* hip_stream);
int svs_sdf_bwd_a(const float* points, int n_points, const float* cam, int cam_stride, const float* dirs, const float* z,
                  int S, int n_rays, const float* d_grad, const unsigned char* clamp_mask, const float* hbuf,
                  const float* gbuf, const float* stream, int precision, float* ubuf, float* a2buf, float* pebuf,
                  float* absmax, void* hip_stream);
int svs_sdf_bwd_b(int n_points, const float* d_sdf, const unsigned char* clamp_mask, const float* feat_bar,
                  int n_feat_points, const float* hbuf, const float* gbuf, const float* a2buf, const float* ubuf,
                  const float* stream, int precision, float* abuf, float* sbar_out, float* absmax, void* hip_stream);
int svs_lin8_row0_grad(const float* hbuf, const float* ubuf, const float* sbar, int n_points, int precision, float* out257,
                       void* hip_stream);
int svs_unpack_wgrad(const float* dWk, const float* dbk, int ldw, int map, int rows, int cols, int row_off,
                     const float* weight_v, const float* weight_g, const float* row0, float* grad_v, float* grad_g,
                     float* grad_b, void* hip_stream);
/* the same for all layers of a step (<= 24 jobs) in ONE launch */
typedef struct svs_unpack_job {
  const float *dWk, *dbk;
  int ldw, map, rows, cols, row_off;
  const float *weight_v, *weight_g, *row0;
  float *grad_v, *grad_g, *grad_b;
} svs_unpack_job;
int svs_unpack_wgrad_multi(const svs_unpack_job* jobs, int n_jobs, void* hip_stream);

/* ---- a12  optimiser step ---------------------------------------------------------------------------------------
 * clip_grad_norm_(1.0) + NaN/Inf guard + Adam of VolOpt.train_step (volsdf/vsdf.py:214-219,454-463,101-102) on flat
 * float32 buffers, no host sync.  step: 1-based Adam step count; when step_counter (device int) is not NULL the launch
 * increments that counter and uses the new value instead, so that a captured launch sequence (hipGraph) replays with
 * an advancing step.  lr / betas / eps are float64 like torch's hyper-parameters (1 - beta, the bias corrections and
 * lr / bias_correction1 are formed in float64 and rounded once, as torch does).  A non-finite gradient is zeroed and
 * the Adam step still runs (torch 1.9 zero_grad semantics).  info (2 floats, may be NULL): gradient norm before
 * clipping, gradient dropped (0/1). */
size_t svs_adam_workspace_bytes(void);
int svs_clip_guard_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step,
                        int* step_counter, double max_norm, double lr, double beta1, double beta2, double eps,
                        void* workspace, float* info, void* hip_stream);

/* ---- a10  MVS prior lookup ----------------------------------------------------------------------------
 * VolOpt.cost_mapping (volsdf/vsdf.py:382-452).  Points: xyz (n_points,3) or, when xyz == NULL, cam + z*dir with
 * z (n_points/S, S).  view_params: HOST float array, 17 per view: fx, fy, cx, cy, sk, c2w rows (3x4).
 * cost / z_near / z_far: HOST arrays of device pointers per view: probability volume (D,H,W), depth hypotheses
 * [0] and [-1] (H,W); dims: HOST int array D,H,W per view.  same_view: index of the rendered view (-> pi).
 * img_w, img_h: SceneDataset resolution used for the normalisation (vsdf.py:397,414-415).
 * same_view_dev (device int, may be NULL): overrides same_view at run time, so that a captured launch sequence
 * (hipGraph) can be replayed for another rendered view.
 * -> pj (n_points), pi (n_points), valid (n_points, uint8) */
int svs_cost_lookup(const float* xyz, const float* cam, const float* dirs, const float* z, int S, int n_points,
                    int n_views, int same_view, int inverse_depth, float img_w, float img_h,
                    const float SVS_HOST* view_params, const float* const SVS_HOST* cost,
                    const float* const SVS_HOST* z_near, const float* const SVS_HOST* z_far, const int SVS_HOST* dims,
                    float* pj, float* pi, unsigned char* valid, const int* same_view_dev, void* hip_stream);

/* ---- a11  loss ----------------------------------------------------------------------------------------
 * VolSDFLoss.forward (volsdf/model/loss.py:80-114) and the gradient of the total w.r.t. the model outputs.
 * rgb_target = ground_truth['rgb'], or 'rgb_smooth' with annealed = 1 (loss.py:103-105); pi/pj NULL = no MVS terms.
 * losses[5] = rgb, eikonal, mvs, sparse, total.  n_rays_norm / n_eik_norm (0 = n_rays / n_eik): denominators of the
 * means when a batch is processed in several ray groups (the groups' losses and gradients then simply add).
 * anneal_dev (device, 2 floats, may be NULL): {annealed, anneal_sparse} read at run time instead of the two by-value
 * arguments (captured launch sequences replayed while the annealing advances). */
int svs_loss(int n_rays, int n_samples, int n_eik, const float* rgb_values, const float* rgb_target,
             const float* grad_theta, const float* weights, const float* pi, const float* pj, const float* depth_values,
             float rgb_weight, float eikonal_weight, float mvs_weight, float sparse_weight, float gce, float confi,
             int annealed, float anneal_sparse, int n_rays_norm, int n_eik_norm, float* losses, float* d_rgb_values,
             float* d_grad_theta, float* d_weights, float* d_depth_values, double* workspace, const float* anneal_dev,
             void* hip_stream);
size_t svs_loss_workspace_bytes(int n_rays, int n_eik);

/* ---- f1  FeatureNet convolutions (models/CasMVSNet.py:24-55,338-439) ---------------------------------------------
 * out (Cout,Ho,Wo) = [add +] relu?(conv2d(in (Cin,H,W), weight) + bias), k in {1,3,5}, padding k/2, stride in {1,2};
 * BatchNorm(eval) folded into weight / bias by the caller.  weight is PACKED for scalar loads: [ceil(Cout/8)][Cin][k][k][8]
 * floats, entry [g][ci][ky][kx][c] = W[8 g + c][ci][ky][kx], zero for 8 g + c >= Cout, 32-byte aligned (the caller packs
 * once per weight tensor; svs_hip/costvol.py: conv2d_pack).  add: optional (Cout,Ho,Wo) tensor added
 * AFTER the activation; add_upsample2 != 0: add is (Cout,Ho/2,Wo/2) and enters nearest-up-sampled by 2 (the FPN's
 * top-down path, :413-431). */
int svs_conv2d(const float* in, const float* weight, const float* bias, const float* add, int add_upsample2, float* out,
               int Cin, int Cout, int H, int W, int k, int stride, int relu, void* hip_stream);
/* The whole 'fpn' FeatureNet (models/CasMVSNet.py:338-439, num_stage 3) for one image (3,H,W), H and W multiples of 4,
 * enqueued by one call: weights[i] / biases[i] (biases[i] may be null), i = conv0.0, conv0.1, conv1.0, conv1.1, conv1.2,
 * conv2.0, conv2.1, conv2.2 (BatchNorm folded), out1, inner1, out2, inner2, out3; weights packed as for svs_conv2d.
 * stage1 (4b,H/4,W/4), stage2 (2b,H/2,W/2), stage3 (b,H,W), b = base_channels. */
size_t svs_featurenet_fpn_workspace_bytes(int base_channels, int H, int W);
int svs_featurenet_fpn(const float* image, int H, int W, int base_channels, const float* const* weights,
                       const float* const* biases, float* workspace, float* stage1, float* stage2, float* stage3,
                       void* hip_stream);
/* The 3x3 (stride 1; Cin in {8,16,32}) and 5x5 (stride 2; Cin in {8,16}) layers of the pyramid, Cout <= 32, on the fp16 matrix
 * cores with two-piece fp16 operands and float32 accumulation (csrc/svs_conv2d_mfma.hip: the float32 accuracy class, 2e-7
 * relative per layer): out (Cout,Ho,Wo) = relu?(conv2d(in (Cin,H,W), k x k, padding k / 2, stride) + bias).  The weights
 * (Cout,Cin,k,k) float32, BatchNorm folded, are packed once per tensor by svs_conv2d_mfma_pack into svs_conv2d_mfma_wfrag_bytes
 * bytes of MFMA A fragments.  svs_featurenet_fpn2 = svs_featurenet_fpn with an optional table of 13 fragment pointers: layer i
 * runs on the matrix cores where wfrags[i] is not null (and the shape is supported), on the float32 kernels otherwise. */
int svs_conv2d_mfma_supported(int Cin, int Cout, int k, int stride);
size_t svs_conv2d_mfma_wfrag_bytes(int Cin, int Cout, int k);
int svs_conv2d_mfma_pack(const float* weight, int Cin, int Cout, int k, void* wfrag, void* hip_stream);
int svs_conv2d_mfma(const float* in, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int H, int W, int k,
                    int stride, int relu, void* hip_stream);
/* The lateral step of the FPN (models/CasMVSNet.py:425-431) fused into the 3x3 layer behind it (out3): the layer's 32-channel
 * input X[c][y][x] = sum_ci W1[c][ci] lat_in[ci][y][x] + lat_bias[c] + lat_add[c][y / 2][x / 2] (ci < 8) is formed while the
 * kernel converts its input windows -- the float32 1x1 kernel's operations in its order, bit for bit -- and never exists in
 * memory.  lat_weight: (32,8,1,1) in svs_conv2d's packed layout; wfrag: (Cout <= 16, 32, 3, 3) packed by svs_conv2d_mfma_pack;
 * H, W even.  svs_featurenet_fpn2 uses it for inner2 + out3 when base_channels = 8 and wfrags[12] is given. */
int svs_conv2d_mfma_lateral(const float* lat_in, const float* lat_weight, const float* lat_bias, const float* lat_add,
                            const void* wfrag, const float* bias, float* out, int Cout, int H, int W, int relu, void* hip_stream);
int svs_featurenet_fpn2(const float* image, int H, int W, int base_channels, const float* const* weights,
                        const float* const* biases, const void* const* wfrags, float* workspace, float* stage1, float* stage2,
                        float* stage3, void* hip_stream);

/* ---- a13/a14  homography warp + variance --------------------------------------------------------------------
 * homo_warping (models/CasMVSNet.py:280-315) for every source view fused with the variance aggregation of
 * DepthNet.forward (:611-642): variance (C,D,H,W) = sum(f^2)/V - (sum(f)/V)^2 over the reference feature (C,H,W)
 * and the n_src warped source features.  Source features are passed channel-last (H,W,C) -- svs_chw_to_hwc.
 * rot_trans: HOST float array, 12 per source view: rows of (src_proj @ inv(ref_proj))[:3,:3], then [:3,3], with
 * proj = K[:3,:3] @ E[:3,:4] (:622-625).  depth_values (D,H,W) per-pixel hypotheses.  C in {8,16,32}.
 * raw_warp != 0: write the warped volume of source 0 instead (homo_warping on its own). */
int svs_chw_to_hwc(const float* in, float* out, int C, int H, int W, void* hip_stream);
int svs_warp_variance(const float* ref_feature, const float* const SVS_HOST* src_features_hwc,
                      const float SVS_HOST* rot_trans, int n_src, int C, int D, int H, int W, const float* depth_values,
                      float* variance, int raw_warp, void* hip_stream);

/* ---- a15  3-D regularisation blocks ----------------------------------------------------------------------------
 * Conv3d / Deconv3d blocks of CostRegNet (models/CasMVSNet.py:107-186,441-472) with BatchNorm(eval) folded:
 * out = [skip +] relu?(conv(in, weight) + bias).  weight: [Cin][27][Cout], tap = (kd*3+kh)*3+kw, BN scale folded
 * in; bias: BN shift (NULL for the final `prob` conv).  transposed: ConvTranspose3d(k3,s2,p1,output_padding 1). */
int svs_conv3d(const float* in, const float* weight, const float* bias, const float* skip, float* out, int Cin, int Cout,
               int Di, int Hi, int Wi, int stride, int transposed, int relu, void* hip_stream);
/* The stride-1 convolutions with Cin in {8,16,32} and Cout <= 16 (conv0, conv2, prob: 79 % of the U-Net's MACs at
 * stage 1) on the fp16 matrix cores with two-piece split operands (float32-class accuracy).
 * wfrag (svs_conv3d_mfma_wfrag_bytes(Cin)): the folded [Cin][27][Cout] weights (float32, on the device) as fp16 hi / mid A
 * fragments of v_mfma_f32_16x16x32_f16, written by svs_conv3d_mfma_pack (asynchronous, allocates nothing; the layout:
 * convmfma::WeightMap, csrc/svs_conv_mfma.hip). */
size_t svs_conv3d_mfma_wfrag_bytes(int Cin);
int svs_conv3d_mfma_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream);
int svs_conv3d_mfma(const float* in, const void* wfrag, const float* bias, const float* skip, float* out, int Cin,
                    int Cout, int D, int H, int W, int relu, void* hip_stream);

/* conv0 of CostRegNet (C -> 8 at full resolution, models/CasMVSNet.py:444,460; 68 / 52 / 35 % of the U-Net's MACs at
 * stage 1 / 2 / 3) fused with the producer of its input.  The variance volume travels between the two kernels as a
 * "split volume": fp16 hi and mid parts (v = hi + mid to float32 accuracy) in channel-last 16-byte units with a zero
 * border, [D+2][Hp][2 pieces][C/8][Wp] units, voxel (z,y,x) at (z+1,y+1,x+1), Hp = 4 ceil(H/4) + 2,
 * Wp = 32 ceil(W/32) + 4.  svs_split_volume_dims returns its size in bytes (dims[0..1] = Hp, Wp); the caller zero-fills
 * the buffer once, the producers write the interior only.
 *   svs_warp_variance_split  = svs_warp_variance writing that form (DepthNet.forward steps 1-2, CasMVSNet.py:611-642);
 *     SVS_ESHAPE where svs_split_volume_dims is 4 GiB or more or a feature map 2 GiB or more (32-bit byte offsets);
 *   svs_split_volume_pack    = the same form from a float32 (C,D,H,W) volume (tests, other callers);
 *   svs_conv3d_pair          = relu?(conv3d(volume, 3x3x3, stride 1, padding 1) + bias), Cin in {8,16,32}, Cout <= 8:
 *     the 16 rows of v_mfma_f32_16x16x32_f16 are 8 output channels x 2 neighbouring x positions, a column is that pair
 *     of positions, K = 3 kd x 3 kh x 4 input columns x Cin (27 of 36 products useful; 27 of 54 with channels only).
 *     wfrag (svs_conv3d_pair_wfrag_bytes(Cin)): written by svs_conv3d_pair_pack from the folded [Cin][27][Cout] weights
 *     (the layout: convpair::PairMap, csrc/svs_conv_pair.hip). */
size_t svs_split_volume_dims(int C, int D, int H, int W, int SVS_HOST* dims);
/* The final `prob` layer (Cin -> 1, CasMVSNet.py:458,471): float32 fused multiply-adds on the vector ALUs (a one-row
 * matrix-core tile would be 1/16 full).  weight [Cin][27][1]. */
int svs_conv3d_c1(const float* in, const float* weight, const float* bias, const float* skip, float* out, int Cin, int D,
                  int H, int W, int relu, void* hip_stream);
int svs_split_volume_pack(const float* in, void* split, int C, int D, int H, int W, void* hip_stream);
int svs_warp_variance_split(const float* ref_feature, const float* const SVS_HOST* src_features_hwc,
                            const float SVS_HOST* rot_trans, int n_src, int C, int D, int H, int W,
                            const float* depth_values, void* split, void* hip_stream);
size_t svs_conv3d_pair_wfrag_bytes(int Cin);
int svs_conv3d_pair_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream);
int svs_conv3d_pair(const void* split, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int D, int H,
                    int W, int relu, void* hip_stream);

/* Every other 3x3x3 layer of the U-Net (stride 2, transposed, the 32/64-channel levels) as an implicit GEMM on the
 * same matrix-core instruction with both operands split: Cin in {8,16,32,64}, Cout <= 64
 * (svs_conv3d_gemm_supported).  One wave = 16 output voxels along x times all output channels; the transposed form
 * runs as 8 GEMMs, one per output parity class, over only the taps that class uses.
 * wfrag: svs_conv3d_gemm_wfrag_bytes(Cin, Cout, transposed), filled once per layer by svs_conv3d_gemm_pack from the
 * folded [Cin][27][Cout] weights (the layout: convgemm::GemmMap, csrc/svs_conv_gemm.hip). */
int svs_conv3d_gemm_supported(int Cin, int Cout);
size_t svs_conv3d_gemm_wfrag_bytes(int Cin, int Cout, int transposed);
int svs_conv3d_gemm_pack(const float* weight, int Cin, int Cout, int transposed, void* wfrag, void* hip_stream);
int svs_conv3d_gemm(const float* in, const void* wfrag, const float* bias, const float* skip, float* out, int Cin, int Cout,
                    int Di, int Hi, int Wi, int stride, int transposed, int relu, void* hip_stream);
/* conv1 of CostRegNet (8 -> 2b channels, stride 2, from the full-resolution volume: CasMVSNet.py:445,461): a lane group
 * owns whole (kz,ky) input rows, one 8-byte load per (row, channel) serves the taps kx = 1, 2 and the neighbour lane's
 * value the tap kx = 0.  Cout <= 16, Wi even.  wfrag (svs_conv3d_s2c8_wfrag_bytes()): written by svs_conv3d_s2c8_pack from the
 * folded [8][27][Cout] weights (the layout: convgemm::S2c8Map, csrc/svs_conv_gemm.hip). */
size_t svs_conv3d_s2c8_wfrag_bytes(void);
int svs_conv3d_s2c8_pack(const float* weight, int Cout, void* wfrag, void* hip_stream);
/* split_out != NULL (Cout = 16, no skip): the output leaves as a split volume (svs_split_volume_dims(16, Do, Ho, Wo)) instead
 * of float32 to `out` -- the input form of svs_conv3d_rows (conv2). */
int svs_conv3d_s2c8(const float* in, const void* wfrag, const float* bias, const float* skip, float* out, void* split_out,
                    int Cout, int Di, int Hi, int Wi, int relu, void* hip_stream);
/* conv2 of CostRegNet (2b -> 2b at half resolution, CasMVSNet.py:446,462) from a split volume: slice ring + LDS-DMA as
 * svs_conv3d_pair, the 16 MFMA rows = output channels.  Cin = 16, Cout <= 16.  wfrag (svs_conv3d_rows_wfrag_bytes(Cin)):
 * written by svs_conv3d_rows_pack from the folded [16][27][Cout] weights (the layout: convpair::RowsMap, csrc/svs_conv_pair.hip). */
size_t svs_conv3d_rows_wfrag_bytes(int Cin);
int svs_conv3d_rows_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream);
int svs_conv3d_rows(const void* split, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int D, int H,
                    int W, int relu, void* hip_stream);

/* ---- a14 tail  softmax over D, depth regression, photometric confidence (models/CasMVSNet.py:648-663) ---------
 * reg, depth_values (D,H,W) -> prob (D,H,W), depth (H,W), conf (H,W), index (H,W int, may be NULL). */
int svs_prob_depth_conf(const float* reg, const float* depth_values, int D, int H, int W, float* prob, float* depth,
                        float* conf, int* index, void* hip_stream);

/* ---- a16  depth hypotheses (models/CasMVSNet.py:519-595,733-751) -------------------------------------------------
 * prev_depth == NULL: D planes dmin..dmax (inverse != 0: uniform in 1/depth); else the previous stage's depth
 * (Hp,Wp) -> +-(D/2)*pix_interval around its bilinear resize to the image, resized to (D, H_img/scale, W_img/scale). */
int svs_depth_hypotheses(const float* prev_depth, int Hp, int Wp, int H_img, int W_img, int D, int scale, float dmin,
                         float dmax, float pix_interval, int inverse, float* out, void* hip_stream);

/* ---- UCSNet, the second MVS backbone (models/ucsnet.py; csrc/svs_ucsnet.hip) ------------------------------------------
 * svs_version() stays 101: entries are only added.
 *
 * Deconv2dUnit of the "unet" feature extractor (models/ucsnet.py:114-149, 225-226):
 *   out (Cout,2H,2W) = relu?(conv_transpose2d(in (Cin,H,W), weight (Cin,Cout,3,3), stride 2, padding 1, output_padding 1) + bias)
 * BatchNorm(eval) folded into weight / bias by the caller.  Channel c of the result is written at out + c * out_channel_stride
 * floats (even, >= 4 H W; out 8-byte aligned), so that it can land in the first half of a concatenation buffer.
 * svs_deconv2d: float32 vector kernel, any Cin / Cout, weight in torch's layout.  svs_deconv2d_mfma: the four output parity
 * classes as implicit GEMMs on v_mfma_f32_16x16x32_f16 with two-piece fp16 operands and float32 accumulation, Cin in {16,32},
 * Cout <= 16 (svs_deconv2d_mfma_supported); the weights are packed once per tensor by svs_deconv2d_mfma_pack into
 * svs_deconv2d_mfma_wfrag_bytes bytes.  The fp16 split is NOT scaled: good for |activation|, |weight| < 65504 (beyond: inf,
 * and NaN through the zero-padded k-step); an operand below 0.125 has its mid piece in the fp16 subnormals and carries 3e-8
 * absolute (a weight of 1e-2: 3e-6 relative) instead of 22 bits. */
int svs_deconv2d(const float* in, const float* weight, const float* bias, float* out, long long out_channel_stride, int Cin,
                 int Cout, int H, int W, int relu, void* hip_stream);
int svs_deconv2d_mfma_supported(int Cin, int Cout);
size_t svs_deconv2d_mfma_wfrag_bytes(int Cin, int Cout);
int svs_deconv2d_mfma_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream);
int svs_deconv2d_mfma(const float* in, const void* wfrag, const float* bias, float* out, long long out_channel_stride, int Cin,
                      int Cout, int H, int W, int relu, void* hip_stream);
/* The whole FeatExtNet (models/ucsnet.py:237-302, num_stage 3) for one image (3,H,W), H and W multiples of 4, enqueued by one
 * call.  15 layers, weights[i] / biases[i] (biases[i] may be null), BatchNorm folded: i = conv0.0, conv0.1, conv1.0, conv1.1,
 * conv1.2, conv2.0, conv2.1, conv2.2, out1, deconv1.deconv, deconv1.conv, out2, deconv2.deconv, deconv2.conv, out3.  The
 * convolutions' weights are packed as for svs_conv2d; the two transposed layers' (9, 12) are (Cin,Cout,3,3) as for svs_deconv2d.
 * wfrags: null, or 15 entries: wfrags[i] != null -> layer i runs on the matrix cores (svs_conv2d_mfma_pack, or
 * svs_deconv2d_mfma_pack for 9 and 12).  torch.cat((x, x_pre)) of :233 is never copied: the workspace
 * (svs_featurenet_unet_workspace_bytes) holds both concatenations, the transposed layer writes channels [0,C) and the encoder's
 * last layer of that level (conv1.2, conv0.1) channels [C,2C).  -> stage1 (4b,H/4,W/4), stage2 (2b,H/2,W/2), stage3 (b,H,W). */
size_t svs_featurenet_unet_workspace_bytes(int base_channels, int H, int W);
int svs_featurenet_unet(const float* image, int H, int W, int base_channels, const float* const* weights,
                        const float* const* biases, const void* const* wfrags, float* workspace, float* stage1, float* stage2,
                        float* stage3, void* hip_stream);
/* compute_depth's tail (models/ucsnet.py:381-394): svs_prob_depth_conf (the same device code: prob, depth, conf and index are
 * bit-identical on the same input) and variance (H,W) = lamb * sqrt(sum_d prob_d (depth_values_d - depth)^2). */
int svs_prob_depth_conf_var(const float* reg, const float* depth_values, int D, int H, int W, float lamb, float* prob,
                            float* depth, float* conf, int* index, float* variance, void* hip_stream);
/* uncertainty_aware_samples at stages 2 and 3 (models/ucsnet.py:450-452, 59-70): both maps (Hd,Wd) = (Hv,Wv) resized
 * bilinearly (align_corners=False) to (Hs,Ws), then out[i] = ((cur + low) + step * i) + 1e-12 with low = -min(cur, var),
 * step = (var - low) / (D - 1), in float32 in that order.  D < 2 or maps of different sizes: an error code, nothing launched.
 * Stage 1 (:47-57) is svs_depth_hypotheses(prev_depth = NULL). */
int svs_uncertainty_hypotheses(const float* prev_depth, int Hd, int Wd, const float* prev_var, int Hv, int Wv, int Hs, int Ws,
                               int D, float* out, void* hip_stream);

/* ---- TransMVSNet, the third MVS backbone (models/TransMVSNet.py; csrc/svs_transmvs.hip) --------------------------------
 * svs_version() stays 101: entries are only added.  float32 vector kernels throughout; a matrix-core form of the deformable
 * convolution does not exist yet.  Every argument is checked before the first launch.
 *
 * svs_deform_conv2d: DCN.forward behind its conv_offset_mask (models/dcn.py:68-80: torchvision.ops.deform_conv2d, 3x3, stride 1,
 * padding 1, dilation 1, one offset group, modulated) with the BatchNorm(eval) and ReLU that follow it in FeatureNet
 * (models/module.py:364-397):  out (Cout,H,W) = relu?(scale * (deform_conv(in (32,H,W)) + bias) + shift).
 * offset_mask (27,H,W) is conv_offset_mask's raw output: for tap k = 3 ky + kx, channels 2k and 2k+1 are dy and dx (the
 * torch.cat((o1, o2)) of :68-69 is the first 18 channels in order) and sigmoid(channel 18+k) is the mask.  The tap samples
 * (y + ky - 1 + dy, x + kx - 1 + dx) by torchvision's rule: 0 when y <= -1, y >= H, x <= -1 or x >= W, else four weighted
 * corners of which one outside the image contributes 0; an offset that is not a number samples 0.  weight_packed: the layout of
 * svs_conv2d, [ceil(Cout/8)][32][3][3][8].  bias, scale + shift (both or neither) may be null.  Cout in 1..32. */
int svs_deform_conv2d(const float* in, const float* offset_mask, const float* weight_packed, const float* bias, const float* scale,
                      const float* shift, float* out, int Cout, int H, int W, int relu, void* hip_stream);
/* The Feature Matching Transformer (models/FMT.py), tokens channel-last (L,32), d_model 32, 8 heads of 4.
 * svs_fmt_tokens_in: (32,H,W) + PositionEncodingSine(32, temp_bug_fix=True) (models/position_encoding.py:39-60; positions count
 *   from 1) -> (H*W,32); div_term: HOST array of the 8 frequencies of :43.  svs_fmt_tokens_out: (H*W,32) -> (32,H,W).
 *   (The einops.rearrange calls of :147-172.)
 * svs_fmt_kv: LinearAttention's sums over the S source tokens (:23-32): K = elu(W_k s + b_k) + 1, V = W_v s + b_v,
 *   kvsum[16 h + 4 m + d] = sum_s K[s,h,d] V[s,h,m], kvsum[128 + 4 h + d] = sum_s K[s,h,d] (160 floats).  Per-workgroup
 *   partial sums go to `workspace` (svs_fmt_kv_workspace_bytes) and one last workgroup adds them in index order: no atomics,
 *   the same bits on every launch.  Weights (32,32) row-major as nn.Linear holds them.
 * svs_fmt_layer: EncoderLayer.forward (:96-111) per query token, given its source's kvsum: Q = elu(W_q x + b_q) + 1,
 *   Z = 1 / (Q . Ksum + 1e-6) per head, attention, out-projection, LayerNorm1(x + .), 32 -> 64 -> 32 with ReLU, LayerNorm2
 *   (eps 1e-5).  weights: HOST array of 12 device pointers: query_projection.{weight,bias}, out_projection.{weight,bias},
 *   linear1.{weight,bias}, linear2.{weight,bias}, norm1.{weight,bias}, norm2.{weight,bias}. */
int svs_fmt_tokens_in(const float* chw, int H, int W, const float SVS_HOST* div_term, float* tokens, void* hip_stream);
int svs_fmt_tokens_out(const float* tokens, int H, int W, float* chw, void* hip_stream);
size_t svs_fmt_kv_workspace_bytes(int S);
int svs_fmt_kv(const float* source, int S, const float* k_w, const float* k_b, const float* v_w, const float* v_b, float* workspace,
               float* kvsum, void* hip_stream);
int svs_fmt_layer(const float* x, int L, const float* kvsum, const float* const SVS_HOST* weights, float* out,
                  void* hip_stream);
/* _upsample_add(dim_reduction(x), y) of the pathway (models/FMT.py:196-223): out (Cin/2,2h,2w) = bilinear_x2(conv1x1(x (Cin,h,w)))
 * + y, align_corners=False, the reduction before the up-sampling as in the reference.  weight (Cin/2,Cin), Cin 32 or 16. */
int svs_pathway_step(const float* x, const float* weight, const float* y, float* out, int Cin, int h, int w, void* hip_stream);
/* DepthNet.forward steps 1-2 (models/TransMVSNet.py:52-91): per source view sim_v[d,y,x] = mean_c warped_v[c,d,y,x] ref[c,y,x],
 * similarity (D,H,W) = sum_v sim_v w_v / (1e-5 + sum_v w_v).  The warp is the homo_warping of models/module.py:285-324, NOT
 * CasMVSNet's: grid_sample with align_corners=True, and a hypothesis whose projected z is below 1e-6 samples 0 (:310-315).
 * Arguments as svs_warp_variance: ref_feature (C,H,W), src_features_hwc: HOST array of n_src <= 4 DEVICE (H,W,C) maps,
 * rot_trans: HOST, 12 floats per source; C in {8,16,32}.  prev_weights null (stage 1): w_v = max_d sigmoid(pixel_wise_net(
 * sim_v)) with net = 177 floats, BatchNorm folded: scale0[16] shift0[16] W1[8][16] shift1[8] w2[8] b2 (:17-30); else
 * prev_weights (n_src,H/2,W/2) is read at (y/2, x/2), the nearest x2 of :208 (H and W even).  weights_out (n_src,H,W) receives
 * the weights at this stage's size either way.  workspace: svs_warp_similarity_workspace_bytes (the per-view similarities). */
size_t svs_warp_similarity_workspace_bytes(int n_src, int D, int H, int W);
int svs_warp_similarity(const float* ref_feature, const float* const SVS_HOST* src_features_hwc,
                        const float SVS_HOST* rot_trans, int n_src, int C, int D, int H, int W, const float* depth_values,
                        const float* prev_weights, const float* net, float* workspace, float* similarity,
                        float* weights_out, void* hip_stream);
/* TransMVSNet's tail (models/TransMVSNet.py:100-109, 225-227), the device code of svs_prob_depth_conf with a flag
 * (csrc/svs_costvol.hip): prob is bit-identical to that entry's; index = the first plane that holds the maximum logit
 * (torch.argmax's rule on exact ties), depth = depth_values[index], conf = prob[index]. */
int svs_prob_wta(const float* reg, const float* depth_values, int D, int H, int W, float* prob, float* depth, float* conf,
                 int* index, void* hip_stream);

/* ---- f3  depth-map fusion (helpers/utils.py:75-132, runner.py:301-386) -------------------------------------------
 * svs_fuse_view: reproject_with_depth + check_geometric_consistency of ONE reference view against n_src <= 16 source
 * views, then the aggregation of filter_depth: geo_mask_sum, depth_est_averaged = (sum of the masked reprojected
 * depths + ref depth) / (geo_mask_sum + 1) (float64, as numpy promotes it), photo_mask = confidence > conf,
 * geo_mask = geo_mask_sum >= thres_view, final = photo & geo [& extra_mask].
 * mats: DEVICE float64, svs_fuse_mats_per_src() = 68 per source view, row-major:
 *   inv(K_ref) (9), E_src @ inv(E_ref) (16), K_src (9), inv(K_src) (9), E_ref @ inv(E_src) (16), K_ref (9)
 *   -- formed by the host in float32 exactly as the reference forms them, then widened.
 * The source depth is sampled like cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0): 5-bit fixed-point coordinates.
 * Optional per-source outputs (all four or none, (n_src,H,W)): the tuple check_geometric_consistency returns.
 * svs_fuse_points: the surviving pixels in row-major order -> world xyz float32 (count,3) and, if ref_img (H,W,3
 * float32 in [0,1]) is given, uint8 colours (count,3) = trunc(img * 255).  mats: inv(K_ref) (9), inv(E_ref) (16).
 * offset_ws: H*W ints; xyz / rgb sized for H*W points; *count (device int) receives the number written.
 * Both entries check every argument before their first launch: a rejected call (SVS_EINVAL: a null pointer, a null entry
 * of src_depths, an incomplete set of per-source outputs; SVS_ESHAPE: n_src outside 0..16, H or W below 1, or H * W above
 * 2^31 - 256, the range of the kernels' int pixel index and grid size) writes nothing. */
int svs_fuse_mats_per_src(void);
int svs_fuse_view(const float* ref_depth, const float* confidence, const float* const SVS_HOST* src_depths,
                  const double* mats, int n_src, int H, int W, float conf, double filter_dist, float filter_diff, int thres_view,
                  const uint8_t* extra_mask, double* depth_avg, uint8_t* photo_mask, uint8_t* geo_mask, uint8_t* final_mask,
                  uint8_t* src_mask, float* src_depth_reproj, float* src_x, float* src_y, void* hip_stream);
int svs_fuse_points(const double* depth_avg, const uint8_t* final_mask, const float* ref_img, const double* mats, int H, int W,
                    int* offset_ws, float* xyz, uint8_t* rgb, int* count, void* hip_stream);

/* ---- f5  image-based rendering of an evaluation view (simple_ibr.py:116-235) -----------------------------------------
 * One reference (evaluation) view, n_src in 1..16 source (training) views, H and W positive multiples of 8 (the
 * reference's pyrUp(g_i) must match g_(i-1)'s shape).  float32 throughout; workspace: svs_ibr_workspace_bytes(), shared
 * by both entries (stream-ordered).  Both entries check every argument before their first launch: a rejected call
 * (SVS_EINVAL: null pointer or n_src out of range; SVS_ESHAPE: H or W) writes nothing, and the size query answers 0
 * for every n_src, H, W that they reject.
 * svs_ibr_weights: simple_ibr.py:171-214 -- per source, cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0) of the image and of
 *   the direction field at map_x / map_y (5-bit fixed point, OpenCV's A = -0.75 cubic), the sampled direction
 *   normalised, cos_dir = dot with ref_dir, nan_to_num, times geo_mask; the constant 0.2 of the render appended;
 *   softmax(20 w) over the n_src+1 entries; fill_j = img_j w_j + pred (1 - w_j) (entry n_src: the render itself);
 *   masks_j = erode(w_j > 0.2, 5x5) w_j for the sources, w_last + 1e-2 for the render, divided by their sum.
 *   src_imgs / src_dirs: HOST arrays of n_src DEVICE pointers to (H,W,3); ref_dir, pred_img (H,W,3); geo_mask (uint8),
 *   map_x, map_y (n_src,H,W): the per-source outputs of svs_fuse_view.  -> fill (n_src+1,H,W,3), masks (n_src+1,H,W):
 *   one mask value per pixel (the reference's three channels are identical).
 * svs_ibr_laplacian_blend: Laplacian_Blending(fill, masks, num_levels=4) (simple_ibr.py:80-136): Gaussian pyramids by
 *   cv2.pyrDown (levels 1..3), per level sum_j m_jl (g_jl - pyrUp(g_j,l+1)) (the coarsest: sum_j m_j3 g_j3),
 *   reconstruction out_l = pyrUp(out_l+1) + LS_l, clip(0, 1).  -> out (H,W,3). */
size_t svs_ibr_workspace_bytes(int n_src, int H, int W);
int svs_ibr_weights(const float* const SVS_HOST* src_imgs, const float* const SVS_HOST* src_dirs, const float* ref_dir,
                    const float* pred_img, const uint8_t* geo_mask, const float* map_x, const float* map_y, int n_src, int H, int W,
                    void* workspace, float* fill, float* masks, void* hip_stream);
int svs_ibr_laplacian_blend(const float* fill, const float* masks, int n_src, int H, int W, void* workspace, float* out,
                            void* hip_stream);

/* ---- f5  novel-view scores (eval_vsdf.py:186-212, --result_from blend|default) --------------------------------------
 * V evaluation views of one size (H, W >= 7: the SSIM window) in one call and two launches.  pred, gt, mask: device
 * (V,H,W,3) uint8 -- the rendered PNG codes, the 8-bit ground-truth codes (load_rgb = code / 255), the mask per channel
 * (nonzero: inside).  -> out: device double (V,3) per view: the masked sum of squared code differences over the whole
 * image, the masked element count (psnr = -10 log10(sse / 255^2 / count) on the host: +inf for a perfect match, NaN for
 * an empty mask, as torch.mean gives them), and structural_similarity(pred_fg, gt_fg, multichannel=True) of
 * scikit-image 0.17.2 on the white-composited images x m + (1 - m): win 7, cov_norm 49/48, data_range = 2 (float32's
 * dtype_range (-1, 1); the reference passes none), S cropped by 3 pixels, the three channel means averaged.  Exact
 * integer window moments, float64 S, fixed-order sums: bit-identical run to run.  workspace: svs_nvs_workspace_bytes().
 * Every argument is checked before the first launch: a rejected call (SVS_EINVAL: null pointer or V < 1; SVS_ESHAPE:
 * H or W < 7, or too large) writes nothing. */
size_t svs_nvs_workspace_bytes(int V, int H, int W);
int svs_nvs_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask, int V, int H, int W, void* workspace,
                  double* out, void* hip_stream);

/* ---- f5b  LPIPS, the third novel-view score (eval_vsdf.py:178, 208-209 -> lpips_tf.py:29-90) ------------------------
 * The reference runs a downloaded frozen graph; the network is restated from the published LPIPS v0.1 model (net-lin,
 * vgg): svs_hip/lpips.py holds the definition and what is not pinned (csrc/svs_lpips.hip).  Added without a version
 * change: nothing that existed changed, and svs_version() stays the 101 every binding checks for.
 * Every argument is checked before the first launch: a rejected call (SVS_EINVAL: null pointer, misaligned buffer, V < 1;
 * SVS_ESHAPE: an unsupported (Cin, Cout) or a size) writes nothing.
 * SVS_EOVERFLOW: an operand of the fp16x2 convolution -- a scaled weight, an input value, a layer's output that feeds the
 * next layer -- is above 65504 in magnitude or not a number.  It is replaced by 0 (no inf or NaN is produced) and the call
 * returns this code.  svs_conv3x3_mfma_pack, svs_conv3x3_mfma and svs_lpips_score read a device flag for it and therefore
 * SYNCHRONISE the stream; the first two keep that flag in one device word per process, made at their first use, so they
 * are not for concurrent use from several threads.
 * svs_conv3x3_mfma: out (Cout,H,W) = relu?(conv2d(in (Cin,H,W), 3x3, padding 1, stride 1) + bias), float32 in and out,
 *   Cin in {3, 64, 128, 256, 512}, Cout in {64, 128, 256, 512} (svs_conv3x3_mfma_supported), two-piece fp16 operands with
 *   float32 accumulation.  weight (Cout,Cin,3,3) float32 is packed once by svs_conv3x3_mfma_pack into
 *   svs_conv3x3_mfma_wfrag_bytes (0: unsupported) bytes, scaled per output channel by a power of two the kernel undoes.
 *   bias may be NULL.  H, W >= 1, H*W <= 2^26.
 * svs_maxpool2: out (C,H/2,W/2) = 2x2 max-pool, stride 2, floor mode, of in (C,H,W) float32; H, W >= 2.
 * svs_lpips_head: *out (device double) = mean over the pixels of sum_c w[c] (n(f0)_c - n(f1)_c)^2 with
 *   n(f) = f / (sqrt(sum_c f_c^2) + 1e-10); f0, f1 (C,H,W) float32, w [C]; C a multiple of 64 in 64..512.  float64, fixed
 *   order.  One workgroup: meant for one tap at test sizes; svs_lpips_score runs the same kernel over many.
 * svs_lpips_score: pred, gt, mask as for svs_nvs_score, H, W >= 16 (relu5_3 needs one pixel), H*W <= 2^24.  -> out: device
 *   double [V], the LPIPS distance of each view's white-composited images.  packed_net: svs_lpips_net_bytes() bytes, 16-byte
 *   aligned; svs_lpips_net_offset(what, index) is the byte offset of (what 0) the packed weights of convolution index
 *   0..12, (1) its float32 bias, (2) the float32 lin weights of tap index 0..4; (size_t)-1 otherwise.  workspace:
 *   svs_lpips_workspace_bytes() (0: rejected sizes), 16-byte aligned.  Bit-identical run to run. */
int svs_conv3x3_mfma_supported(int Cin, int Cout);
size_t svs_conv3x3_mfma_wfrag_bytes(int Cin, int Cout);
int svs_conv3x3_mfma_pack(const float* weight, int Cin, int Cout, void* wfrag, void* hip_stream);
int svs_conv3x3_mfma(const float* in, const void* wfrag, const float* bias, float* out, int Cin, int Cout, int H, int W,
                     int relu, void* hip_stream);
int svs_maxpool2(const float* in, float* out, int C, int H, int W, void* hip_stream);
int svs_lpips_head(const float* f0, const float* f1, const float* w, int C, int H, int W, double* out, void* hip_stream);
size_t svs_lpips_net_bytes(void);
size_t svs_lpips_net_offset(int what, int index);
size_t svs_lpips_workspace_bytes(int V, int H, int W);
int svs_lpips_score(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask, int V, int H, int W, const void* packed_net,
                    void* workspace, double* out, void* hip_stream);

/* ---- f6  scene loading: the image work of SceneDataset (volsdf/datasets/scene_dataset.py:163-206) --------------------
 * V views of one source size (Hs,Ws) to one destination size (H,W) per call; H, W >= 16 (the 31-tap smoothing reflects
 * once), V >= 1.  Every argument is checked before the first launch: a rejected call (SVS_EINVAL: null pointer, V < 1,
 * divisor <= 0; SVS_ESHAPE: a size) writes nothing.  The per-axis tables are DEVICE arrays the host builds
 * (svs_hip/scene.py::cubic_table / linear_table, as OpenCV builds its own): xofs (W) / yofs (H) int32, the index of the
 * first tap (it may lie outside the image: every tap index is clamped on its own), xcoef / ycoef float32 (W,taps) /
 * (H,taps).  The coordinate is fx = (float)((d + 0.5) * scale - 0.5), scale = 1 / (dst / src) in double; s = floor(fx),
 * t = fx - s; cubic: first tap s - 1, Keys' weights with A = -0.75 at t; linear: first tap s, weights (1 - t, t).
 * svs_scene_resize_cubic: scene_dataset.py:163-169 -- load_rgb's code * (1/255) (float32 multiply) and
 *   cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC), no prefilter.  codes: (V,Hs,Ws,3) uint8 -> out (V,H,W,3)
 *   float32.  Hs == H and Ws == W: code * (1/255) alone (the reference skips the resize; the tables may be null).
 * svs_scene_smooth: scene_dataset.py:172 -- cv2.GaussianBlur(img, (31,31), 90): separable, float32 weights of
 *   exp(-(i-15)^2 / (2 90^2)) normalised in float64, BORDER_REFLECT_101, rows then columns.  img, out: (V,H,W,3) float32
 *   (out may not alias img); workspace: svs_scene_workspace_bytes() (the float32 intermediate).
 * svs_scene_mask: scene_dataset.py:178-206 -- cv2.resize(mask, (W,H), cv2.INTER_NEAREST) and > 0.5.  The third
 *   positional parameter of cv2.resize is dst, so the default INTER_LINEAR is what runs (UNPINNED):
 *   2 taps per axis.  mask: (V,Hs,Ws) uint8, read as code / divisor in float32 (1 for a 0/1 mask, 255 for an alpha
 *   channel) -> out (V,H,W,3) float32 0/1, the three channels equal. */
size_t svs_scene_workspace_bytes(int V, int H, int W);
int svs_scene_resize_cubic(const uint8_t* codes, int V, int Hs, int Ws, int H, int W, const int* xofs, const float* xcoef,
                           const int* yofs, const float* ycoef, float* out, void* hip_stream);
int svs_scene_smooth(const float* img, int V, int H, int W, void* workspace, float* out, void* hip_stream);
int svs_scene_mask(const uint8_t* mask, float divisor, int V, int Hs, int Ws, int H, int W, const int* xofs,
                   const float* xcoef, const int* yofs, const float* ycoef, float* out, void* hip_stream);

/* ---- f9  the MVS loader's image work (datasets/general_eval.py:157-176, 220-232, 254, 267-268; runner.py:106) -------
 * V views of one source size (Hs,Ws) with C = 3 or 4 channels to one destination size (H,W) per call.  src: (V,Hs,Ws,C),
 * uint8 codes (src_is_float = 0) or float32 (src_is_float = 1: the second pass of the x2_mvsres chain).  A code's value
 * is helpers/utils.py:27's np.float32(code) / 255. -- a float32 DIVISION, one ulp from f6's multiply at some codes --
 * read from code_table, a DEVICE array of the 256 values the host computes (it may be null for a float32 source).  The
 * per-axis tables are f6's cubic tables.  Every argument is checked before the launch: a rejected call (SVS_EINVAL: null
 * pointer, V < 1, C not 3 or 4, src_is_float not 0 or 1; SVS_ESHAPE: a size below 1, H or V above 65535, more than 2^26
 * pixels) writes nothing.  Neither synchronises nor allocates; one launch each.
 * svs_mvs_resize_cubic: general_eval.py:174 -- cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC) of the float32
 *   image -> out (V,H,W,C) float32; svs_scene_resize_cubic's kernel (csrc/svs_resize.h) with another code-to-float rule.
 *   Hs == H and Ws == W: a copy of the values (the tables may be null).
 * svs_mvs_resize_pack: the same resize fused with general_eval.py:254, 267-268 -> imgs (V,3,H,W), masks (V,1,H,W)
 *   float32 planes; C = 4: rgb * alpha (the product after the resize) and alpha; C = 3: rgb and ones.
 * svs_mvs_codes: runner.py:106 -- np.clip(img * 255, 0, 255).astype(np.uint8) of img (3,H,W) float32 planes ->
 *   codes (H,W,3) uint8: float32 multiply, clip, truncation toward zero; NaN -> 0. */
int svs_mvs_resize_cubic(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                         int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* out,
                         void* hip_stream);
int svs_mvs_resize_pack(const void* src, int src_is_float, const float* code_table, int V, int Hs, int Ws, int C, int H,
                        int W, const int* xofs, const float* xcoef, const int* yofs, const float* ycoef, float* imgs,
                        float* masks, void* hip_stream);
int svs_mvs_codes(const float* img, int H, int W, uint8_t* codes, void* hip_stream);

/* ---- f8  from the MVS network's outputs to the default-config point cloud (runner.py:267-271, :362-368) --------------
 * The evaluation mask of filter_depth (eval_mask: true in config/base.yaml) and the confidence map it thresholds, which
 * the reference computes on the host with scikit-image and OpenCV.  Every argument is checked before the first launch: a
 * rejected call (SVS_EINVAL: null pointer, misaligned workspace, V < 1 or > 65535, radius outside 0..32; SVS_ESHAPE: a
 * size below 1, more than 65535 rows or more than 2^26 pixels) writes nothing.  Per-axis tables as in f6 (linear).
 * svs_mask_dilate_disk: runner.py:365 -- skimage.morphology.binary_dilation(mask, disk(radius)) =
 *   scipy.ndimage.binary_dilation(mask != 0, structure=disk(radius)), border value 0; disk(r) = x^2 + y^2 <= r^2 on the
 *   integer grid (441 taps for r = 12).  mask (V,Hs,Ws) uint8, a pixel is set iff its code is non-zero -> out (V,Hs,Ws)
 *   uint8 0/1 (out may alias mask); radius 0: out = mask != 0.  workspace: svs_mask_dilate_workspace_bytes(), 8-byte
 *   aligned (the bit-packed rows and their dilation).  Bit-exact.
 * svs_mask_resize_any: runner.py:366-368 -- cv2.resize(mask * 1., (W,H)) > 0. for a 0/1 mask (float64 INTER_LINEAR of
 *   non-negative values with non-negative weights: no cancellation), i.e. a destination pixel is set iff one of its
 *   2x2 taps is set and that tap's row and column weights are both non-zero.  mask (V,Hs,Ws) uint8 -> out (V,H,W) uint8
 *   0/1.  Hs == H and Ws == W: out = mask != 0 (the tables may be null).  Bit-exact against that rule.
 * svs_mvs_confidence: runner.py:267-271 -- conf_final = cv2.resize(conf_1, (W,H)) * cv2.resize(conf_2, (W,H)) *
 *   cv2.resize(photometric_confidence, (W,H)).  conf_k (Hk,Wk) float32 with its own linear tables to (H,W) -> out (H,W)
 *   float32 = (r1 * r2) * r3; r_k: the horizontal pass S[x0] a0 + S[x1] a1 on both source rows, then R0 b0 + R1 b1, each
 *   product and sum rounded to float32 on its own (no fma); a map of size (H,W) is taken as it is (its tables may be
 *   null).  One launch.  UNPINNED: whether OpenCV's own float32 path contracts to fma depends on its build
 *   (INTEGRATION.md gives the call to check it against). */
size_t svs_mask_dilate_workspace_bytes(int V, int Hs, int Ws);
int svs_mask_dilate_disk(const uint8_t* mask, int V, int Hs, int Ws, int radius, void* workspace, uint8_t* out,
                         void* hip_stream);
int svs_mask_resize_any(const uint8_t* mask, int V, int Hs, int Ws, int H, int W, const int* xofs, const float* xcoef,
                        const int* yofs, const float* ycoef, uint8_t* out, void* hip_stream);
int svs_mvs_confidence(const float* conf1, int H1, int W1, const int* xofs1, const float* xcoef1, const int* yofs1,
                       const float* ycoef1, const float* conf2, int H2, int W2, const int* xofs2, const float* xcoef2,
                       const int* yofs2, const float* ycoef2, const float* conf3, int H3, int W3, const int* xofs3,
                       const float* xcoef3, const int* yofs3, const float* ycoef3, int H, int W, float* out,
                       void* hip_stream);

/* ---- f9  the save tail of a scan run (runner.py:283-290; csrc/svs_preview.hip) ---------------------------------------
 * Added without a version change: nothing that existed changed, and svs_version() stays 101.  Every argument is checked
 * before the first launch; a rejected call (SVS_EINVAL: null pointer, misaligned workspace, a count or a rank out of
 * range; SVS_ESHAPE: a size) writes nothing.
 * svs_select_sorted_pairs: exact order statistics of x (n float32 on the device, 1 <= n < 2^31).  ranks: HOST array of
 *   n_ranks (1..4) zero-based ranks k_j in 0..n-1 -> values (2 n_ranks float32, device): values[2j] is the k_j-th
 *   smallest element and values[2j+1] the min(k_j + 1, n - 1)-th, the pair numpy's `linear` quantile interpolates
 *   between; counts (3 x uint32, device): how many elements are NaN, +inf, -inf.  The order is total: -inf < negatives <
 *   -0.0 < +0.0 < positives < +inf < NaN (a NaN comes back as the quiet NaN 0x7fffffff); apart from the order of the two
 *   zeros, which np.sort leaves open, values are bit for bit what np.sort(x) holds at those ranks.  Radix selection over
 *   the order-preserving integer key, four passes of 8 bits shared by all ranks, histograms in LDS, integer atomics only,
 *   every decision on the device: the same result from run to run, no host round trip.  8 launches and one memset;
 *   x is read four times.  workspace: svs_select_workspace_bytes() bytes, 8-byte aligned.
 * svs_depth_preview: helpers/utils.py::visualize_depth (:197-224) for n_maps (1..3) float32 maps of n_k pixels (1..2^26)
 *   that share the bounds lo, hi: invalid = NaN or infinite; d clamped to [lo, hi], invalid -> hi; s = (d - lo) / (hi - lo)
 *   and s * 255 each rounded to float32 on its own (IEEE division), c = the truncation.  direct != 0: out_k (n_k) uint8
 *   = c; direct == 0: out_k (n_k,3) uint8 = row 255 - c of table (256,3) uint8 on the device (cv2.applyColorMap's
 *   look-up: the table decides the channel order).  Invalid pixels are 0.  hi <= lo or a NaN bound: the reference
 *   divides by zero and casts NaN to uint8, which is platform-defined; here every code is 0.  One launch.  Unused maps
 *   may be null. */
size_t svs_select_workspace_bytes(void);
int svs_select_sorted_pairs(const float* x, long long n, const long long SVS_HOST* ranks, int n_ranks, void* workspace,
                            float* values, unsigned int* counts, void* hip_stream);
int svs_depth_preview(const float* map0, int n0, uint8_t* out0, const float* map1, int n1, uint8_t* out1, const float* map2,
                      int n2, uint8_t* out2, int n_maps, float lo, float hi, int direct, const uint8_t* table,
                      void* hip_stream);

/* ---- f7  the finish of an evaluation view (eval_vsdf.py:230-262, volsdf/utils/plots.py:392-468) ----------------------
 * What the reference does in numpy on the host after merge_output, on the render's device tensors.  Every argument is
 * checked before the launch: a rejected call (SVS_EINVAL: null pointer; SVS_ESHAPE: a size) writes nothing.
 * svs_view_finish: one pass over weights (n_pixels,n_samples) float32.  rgb_values, normal_map (n_pixels,3),
 *   depth_values (n_pixels) float32 ->
 *   rgb_codes (n_pixels,3) uint8 = (rgb * 255).astype(np.uint8) (eval_vsdf.py:245): float32 multiply, then x86 numpy's
 *     cast: truncation toward zero to int32, low 8 bits kept (outside the int32 range and for NaN: 0);
 *   normal_codes (n_pixels,3) uint8 = (((n + 1) / 2) * 255).astype(np.uint8), float32 in that order (:251-254), the same
 *     cast (normal_map is not bounded by 1: -1.5 -> 255, 300.7 -> 44);
 *   depth_est (n_pixels) float32 = depth_values * scale_factor, one float32 multiply (:240);
 *   acc (n_pixels) float32 = the row sums of weights (:258) in one fixed order (it depends on n_samples and the row
 *     index modulo 4 only): bit-identical run to run, within (S-1) 2^-24 sum|w| of the exact sum.
 *   n_pixels in 1..2^26, n_samples in 1..16384.  weights is read with 16-byte loads when it is 16-byte aligned.
 * svs_view_depth_colors: the colour step of visualize_depth / visualize_cmap / matte (plots.py:392-468) for an image of
 *   `width` columns (n_pixels a multiple of it).  depth (n_pixels) float32: the UNSCALED depth_values; acc (n_pixels);
 *   lo, hi: the two bounds in depth units (weighted percentile -/+ float32 eps, found by the caller);
 *   table (table_len,3) float64 DEVICE: the colour table (matplotlib's turbo: 256 rows) -> codes (n_pixels,3) uint8:
 *   v = nan_to_num(clip((c(depth) - min(c(lo),c(hi))) / |c(hi) - c(lo)|, 0, 1)) with c(x) = -log(x + eps_f32), row
 *   int(v * table_len) of the table (v = 1: the last row), times acc plus the 8-pixel checker (0.8 / 1.0) times the
 *   float32 (1 - acc), times 255, the cast above.  Evaluated in float64, as numpy evaluates it. */
int svs_view_finish(const float* rgb_values, const float* normal_map, const float* depth_values, const float* weights,
                    int n_pixels, int n_samples, float scale_factor, uint8_t* rgb_codes, uint8_t* normal_codes,
                    float* depth_est, float* acc, void* hip_stream);
int svs_view_depth_colors(const float* depth, const float* acc, int n_pixels, int width, double lo, double hi,
                          const double* table, int table_len, uint8_t* codes, void* hip_stream);

/* ---- f4  Chamfer evaluator on point clouds (evals/eval_dtu.py:100-176) ---------------------------------------------
 * All clouds are (n,3) float64 (what open3d hands the reference).  One structure serves both neighbour problems:
 * points sorted by uniform-grid cell + a hash from cell to its run; grid_ws: svs_cloud_grid_bytes(n_points of the
 * cloud the grid is built over); origin: HOST double[3], <= every coordinate of both clouds, (max - origin)/cell < 2^21.
 * svs_cloud_nn: sklearn NearestNeighbors(n_neighbors=1).fit(ref).kneighbors(query) (:150-152,:174-175): dist
 *   (float64, same arithmetic as the kd-tree) and idx (may be NULL).  Exact for neighbours closer than max_radius;
 *   a result >= max_radius is an upper bound (+inf / -1 if none met) -- the protocol drops distances >= max_dist.
 * svs_cloud_downsample_*: the greedy radius down-sampling (:104-118) = the lexicographically-first maximal
 *   independent set of the radius graph in index order.  _begin builds the grid (cell = radius) and clears state;
 *   every _round settles more points (state: 0 undecided, 1 kept, 2 dropped; *undecided = points still open after
 *   the round); repeat until *undecided == 0.
 * svs_cloud_obs_filter: bounding-box-plus-patch test and ObsMask lookup (:124-135).  bb: HOST float[6] (BB rows),
 *   obs_mask: uint8 (d0,d1,d2) C order.  inbound[i] = inside the padded box; in_obs[i] = inbound & grid-inbound & mask.
 * svs_cloud_plane_side: (P . [x,y,z,1]) > 0 (:165-167), plane: HOST double[4].
 * svs_cloud_compact: rows with mask != 0, order kept; offset_ws: n ints; *count (device int).
 * svs_cloud_mean_below: mean of dist[dist < max_dist] (:153,:176) -> mean_count[0], and the number of terms
 *   -> mean_count[1]; deterministic two-level sum.  workspace: svs_cloud_mean_workspace_bytes(). */
size_t svs_cloud_grid_bytes(int n_points);
int svs_cloud_nn(const double* ref, int n_ref, const double* query, int n_query, const double SVS_HOST* origin, double cell,
                 double max_radius, void* grid_ws, double* dist, int* idx, void* hip_stream);
int svs_cloud_downsample_begin(const double* pts, int n, const double SVS_HOST* origin, double radius, void* grid_ws, uint8_t* state,
                               void* hip_stream);
int svs_cloud_downsample_round(const double SVS_HOST* origin, int n, double radius, void* grid_ws, uint8_t* state, int* undecided,
                               void* hip_stream);
int svs_cloud_obs_filter(const double* pts, int n, const float SVS_HOST* bb, double res, double patch, const uint8_t* obs_mask,
                         int d0, int d1, int d2, uint8_t* inbound, uint8_t* in_obs, void* hip_stream);
int svs_cloud_plane_side(const double* pts, int n, const double SVS_HOST* plane, uint8_t* above, void* hip_stream);
int svs_cloud_compact(const double* pts, const uint8_t* mask, int n, int* offset_ws, double* out, int* count, void* hip_stream);
size_t svs_cloud_mean_workspace_bytes(void);
/* svs_cloud_bounds: lo_hi[0..2] = per-axis minimum, lo_hi[3..5] = per-axis maximum of pts (n >= 1; DEVICE double[6]) -- the
 * origin and extent of the search grids (the evaluator took them from two column reductions of torch: 2.6 ms per 4 M-point
 * cloud, as long as the neighbour search itself).  workspace: svs_cloud_bounds_workspace_bytes(). */
size_t svs_cloud_bounds_workspace_bytes(void);
int svs_cloud_bounds(const double* pts, int n, double* workspace, double* lo_hi, void* hip_stream);
int svs_cloud_mean_below(const double* dist, int n, double max_dist, double* workspace, double* mean_count, void* hip_stream);

/* ---- f4b  BlendedMVS Chamfer evaluator and the error clouds of both evaluators (csrc/svs_chamfer.hip) -------------------
 * svs_cloud_prepare: the PLY's coordinates -> the cloud the kd-tree sees (evals/eval_bmvs.py:127,129-134,196-197).
 *   pts: DEVICE (n,3) float32 (is_f64 == 0) or float64; out: DEVICE (n,3) float64; matrix: HOST double[16] row-major, or NULL.
 *   matrix == NULL (every scan but 5; :127,:196-197): out = (double)((float)x / (float)scale), one IEEE float32 division --
 *   `astype('float32')` followed by the in-place `/= relative_scale[scan]` of a float32 array.
 *   matrix != NULL (scan 5; :129-134,:197): p = (double)(float)x, t_a = ((m_a0 p_0 + m_a1 p_1) + m_a2 p_2) + m_a3,
 *   out = t / scale, all float64, left to right, no contraction.  The reference forms t with a BLAS dot whose summation
 *   order is the host library's, so this mode agrees with it up to the last bits only.
 *   n == 0 is not an error; scale must be > 0.  Denormal float32 inputs are outside the contract.
 * svs_cloud_error_colors: the colour step (evals/eval_bmvs.py:232-246, evals/eval_dtu.py:173-187) over a cloud of n_full
 *   rows of which n_dist were evaluated.  select == NULL: row i has dist[i] (n_full == n_dist).  Otherwise select[i] == 0
 *   is blue (0,0,1) and else the row has dist[rank[i]], rank[i] = number of selected rows before i (the offsets
 *   svs_cloud_compact computes; a rank outside [0, n_dist) is never read: blue).  d >= max_dist (inf included): green
 *   (0,1,0); else a = min(d, vis_dist) / vis_dist and the colour is (a + (1 - a), 1 - a, 1 - a) in float64 -- numpy's
 *   R * a + W * (1 - a).  rgb_f64: (n_full,3) float64; rgb_u8: (n_full,3) = (uint8) rint(min(1, max(0, c)) * 255), what the
 *   PLY stores; either may be NULL. */
int svs_cloud_prepare(const void* pts, int is_f64, int n, const double SVS_HOST* matrix, double scale, double* out,
                      void* hip_stream);
int svs_cloud_error_colors(const double* dist, int n_dist, const uint8_t* select, const int* rank, int n_full, double max_dist,
                           double vis_dist, double* rgb_f64, uint8_t* rgb_u8, void* hip_stream);

/* Evaluator --mode mesh (evals/eval_dtu.py:14-23 sample_single_tri, :62-90): the points the script samples on every
 * triangle of the predicted mesh before it proceeds as in point-cloud mode.  tri: DEVICE double[n_tri][11] =
 * [n1, n2, v1(3), v2(3), p0(3)] per triangle of non-zero area (:70-83; integer-valued n1 = floor(l1 / thr), n2).
 * svs_mesh_sample_count: counts[t] = number of grid entries ((i + 0.5) / max(n1, 1e-7), (j + 0.5) / max(n2, 1e-7)),
 *   i = 0..n1, j = 0..n2, whose coordinates sum to less than 1 (:22).
 * svs_mesh_sample_points: out[offsets[t] + m] = v1 c0 + v2 c1 + p0 (:23) for the m-th such entry in row-major order;
 *   offsets = exclusive prefix sum of counts, out: DEVICE double[sum(counts)][3].  Each product and sum is rounded
 *   separately, as numpy's. */
int svs_mesh_sample_count(const double* tri, int n_tri, long long* counts, void* hip_stream);
int svs_mesh_sample_points(const double* tri, int n_tri, const long long* offsets, double* out, void* hip_stream);

/* ---- f4c  cleaning a fused cloud: k nearest neighbours, statistical outliers, oriented normals (csrc/svs_cloudknn.hip) ----
 * This project's own arithmetic, after the common remove_statistical_outlier / PCA-normal recipe (svs_hip/clouds.py,
 * svs_hip/cloudclean.py; restated in float64 numpy by tests/cloudclean_oracle.py).  Clouds are (n,3) float64 as in f4.
 * svs_cloud_knn: for every query the k nearest reference points, 1 <= k <= 32, over the grid of f4 (built here, in
 *   grid_ws: svs_cloud_grid_bytes(n_ref); origin: HOST double[3], <= every coordinate of both clouds, (max - origin)/cell
 *   < 2^21; cell > 0: the grid's cell size).
 *   dist (n_query,k) float64, ascending; idx (n_query,k) int32, original indices.  Neighbours are ordered by (d2, index),
 *   d2 = ex*ex + ey*ey + ez*ez in float64 without contraction (svs_cloud_nn's expression: k = 1 returns its bits wherever
 *   its result is below max_radius), so ties go to the lower index; dist = sqrt(d2).  A slot whose neighbour is not strictly
 *   closer than max_radius holds +inf / -1, and so does a slot that does not exist (fewer than k candidates): the output is
 *   a function of the inputs alone.  0 < max_radius <= 4096 cells (SVS_ESHAPE otherwise): the search walks rings of cells
 *   outwards until the list is full and its k-th entry is <= (ring * cell + margin to the home cell's walls)^2, or
 *   through ring ceil(max_radius / cell) + 1.
 *   exclude_same_index: 0, every reference counts; e > 0, reference (e - 1) + j is skipped for query j -- 1 when the query
 *   cloud is the reference cloud, 1 + first row when it is a range of the reference's rows.
 *   mean_dist (n_query) float64: the mean of the finite slots of the row, summed in ascending slot order, +inf if there
 *   are none.  Each of dist, idx, mean_dist may be NULL, not all three.  With query == ref and n_query == n_ref the queries
 *   are walked in the grid's sorted order (neighbouring lanes, neighbouring cells); the rows written are the same.
 *   n_query == 0 returns 0; n_ref == 0 fills the outputs.
 * svs_cloud_outlier_stats: over the finite entries of mean_dist (n), one fixed two-level summation order, no atomics:
 *   out[0] = their number, out[1] = their mean (0 if there are none), out[2] = their sample standard deviation
 *   (denominator count - 1, two passes: the deviations are taken about out[1]; 0 when count < 2).  out: DEVICE double[3];
 *   workspace: svs_cloud_outlier_workspace_bytes().
 * svs_cloud_outlier_mask: keep[i] = mean_dist[i] <= threshold, 0 for an entry that is not finite; keep (n) uint8.
 * svs_cloud_normals: for point i the set S = {pts[j] : j = idx[i, s], 0 <= j < n} (idx (n,k) int32, 1 <= k <= 32: what
 *   svs_cloud_knn wrote, -1 = no neighbour) plus pts[i] itself when include_self != 0.  The float64 covariance of S about
 *   its centroid, its eigenvectors by cyclic Jacobi (8 sweeps, rotations in the order (0,1), (0,2), (1,2)); the normal is
 *   the eigenvector of the smallest eigenvalue l0, curvature = l0 / (l0 + l1 + l2) (0 for a zero trace; an l0 that
 *   rounding left below 0 counts as 0, so 0 <= curvature <= 1/3).  Of equal smallest entries of the rotated diagonal the
 *   lowest index is taken; a covariance that is diagonal as summed is not rotated, so its normal is the positive axis of
 *   its smallest diagonal entry, the lowest axis among equal ones (all points coincident: (1,0,0), curvature 0).
 *   centres (n_views,3) float64 DEVICE or NULL: NULL leaves the normal as the solver gave it; otherwise it is negated when
 *   n . (c - p) < 0, c = centres[view_index[i]] (view_index (n) int32, clamped to [0, n_views)) or, with view_index NULL,
 *   the centre nearest to the point (the lowest index on a tie).  normals (n,3) float32, unit length; curvature (n)
 *   float32, may be NULL.  Fewer than 3 points in S: normal (0,0,0), curvature 0. */
int svs_cloud_knn(const double* ref, int n_ref, const double* query, int n_query, const double SVS_HOST* origin, double cell, int k,
                  double max_radius, int exclude_same_index, void* grid_ws, double* dist, int* idx, double* mean_dist,
                  void* hip_stream);
size_t svs_cloud_outlier_workspace_bytes(void);
int svs_cloud_outlier_stats(const double* mean_dist, int n, double* workspace, double* out, void* hip_stream);
int svs_cloud_outlier_mask(const double* mean_dist, int n, double threshold, uint8_t* keep, void* hip_stream);
int svs_cloud_normals(const double* pts, int n, const int* idx, int k, int include_self, const int* view_index,
                      const double* centres, int n_views, float* normals, float* curvature, void* hip_stream);

/* ---- surface mesh of a checkpoint (svs_hip.mesh; eval_vsdf.py:111-154 --eval_mesh, volsdf/utils/plots.py:108-333) ------
 * What scikit-image's marching_cubes and trimesh do for the reference on the host.  The case table is generated
 * (csrc/svs_mc_table.h, tools/gen_mc_table.py): scikit-image's vertex set (one vertex per sign-changing grid edge, without
 * the rare interior vertices Lewiner adds), a triangulation and an orientation of this project's own.
 *
 * svs_grid_points: points [start, start + count) of np.meshgrid(x, y, z) raveled as plots.py:294-295 / :328-329 do
 *   (point p = (iy * nx + ix) * nz + iz is (x[ix], y[iy], z[iz])), out DEVICE float[count][3].  x, y, z: DEVICE float32 axes,
 *   computed on the host as get_grid / get_grid_uniform compute them.  rotation (HOST float[9], row-major vecs) and shift
 *   (HOST float[3]), both or neither: the point becomes vecs^T p + shift (plots.py:153-157).  The SDF of the chunk is
 *   svs_sdf_vals with radius 0: implicit_network(x)[:, 0].
 * svs_mc_tile: tile[3] = the classify workgroup's extent along axes 0, 1, 2.
 * svs_mc_classify: volume (n0,n1,n2) float32 with element strides (stride0, stride1, 1), inside = value < level.  Per NODE
 *   (it stands for the cell at whose minimum corner it sits and owns the three grid edges towards +0, +1, +2):
 *   cell[(i*n1 + j)*n2 + k] = case | triangles << 8 | owned-edge mask << 12.  Replaces the classification half of
 *   measure.marching_cubes (plots.py:120-126, :171-177, :207-213, :260-266).
 * svs_mc_emit: active = the ascending node indices whose word is > 255 (n_active of them), vert_base / tri_base = exclusive
 *   prefix sums of their vertex (bits of the mask) and triangle counts.  Writes every vertex once, float32
 *   index * spacing with the crossing at p0 + t * spacing, t = (level - v0) / (v1 - v0) in float32, and faces as int32
 *   triples: node order, then axis / table order, no atomics.  spacing: HOST float[3]. */
int svs_grid_points(const float* x, const float* y, const float* z, int nx, int ny, int nz, long long start, int count,
                    const float SVS_HOST* rotation, const float SVS_HOST* shift, float* out, void* hip_stream);
int svs_mc_tile(int SVS_HOST* tile);
int svs_mc_classify(const float* volume, int n0, int n1, int n2, long long stride0, long long stride1, float level,
                    short* cell, void* hip_stream);
int svs_mc_emit(const float* volume, int n0, int n1, int n2, long long stride0, long long stride1, float level,
                const float SVS_HOST* spacing, const short* cell, const int* active, int n_active, const int* vert_base,
                const int* tri_base, float* verts, int* faces, void* hip_stream);
/* trimesh's slice_plane without a cap (plots.py:278-285: six calls for the DTU box), one half-space n . x + d >= 0
 * (plane: HOST double[4]), in two steps around a weld the caller does (unique of the int64 keys):
 * svs_mesh_clip_count: dist (n_verts) double, inside (n_verts) uint8; per face counts = triangles it becomes (0, 1, 2) and
 *   keys[f][2] = lo * n_verts + hi of its two cut edges (-1: none).
 * svs_mesh_clip_emit: vert_remap = new index of every kept vertex, offsets = exclusive prefix sum of counts, cut_index[f][2]
 *   = index of the face's keys among the n_cut unique cut_keys.  out_verts: the n_kept kept vertices unchanged, then one
 *   vertex per cut edge (interpolated in float64 from the edge's ordered ends, rounded once); out_faces: triangles wholly
 *   inside copied (re-indexed), crossing ones as one or two triangles of the same orientation. */
int svs_mesh_clip_count(const float* verts, int n_verts, const int* faces, int n_faces, const double SVS_HOST* plane, double* dist,
                        uint8_t* inside, int* counts, long long* keys, void* hip_stream);
int svs_mesh_clip_emit(const float* verts, int n_verts, const int* faces, int n_faces, const double* dist,
                       const uint8_t* inside, const int* vert_remap, const int* offsets, const int* cut_index,
                       const long long* cut_keys, int n_cut, int n_kept, float* out_verts, int* out_faces, void* hip_stream);
/* trimesh's split(only_watertight=False) + area (eval_vsdf.py:143-146, plots.py:131-134, :218-220): labels[v] = the smallest
 * vertex id of v's component, by minimum-label propagation over the faces (roots hooked with atomicMin) and pointer jumping.  Every round reads one
 * device flag (workspace: svs_mesh_components_workspace_bytes()).  *rounds = the rounds run.  Returns 0, SVS_ENOCONV when
 * the labels still change after max_rounds, or the HIP error code (positive), as every entry point does.  Synchronises the
 * stream.
 * svs_mesh_face_areas: area[f] in float64; face_label[f] = labels[first corner] (both may be NULL together). */
size_t svs_mesh_components_workspace_bytes(void);
int svs_mesh_components(const int* faces, int n_faces, int n_verts, int max_rounds, int* labels, int* workspace,
                        int SVS_HOST* rounds, void* hip_stream);
int svs_mesh_face_areas(const float* verts, const int* faces, int n_faces, const int* labels, double* area, int* face_label,
                        void* hip_stream);

/* ---- TSDF fusion of a scan's depth maps (svs_hip.tsdf; csrc/svs_tsdf.hip) ---------------------------------------------
 * The volume between fusion.fuse_view's per-view depth and svs_mc_classify / svs_mc_emit.  The reference has no such step;
 * the arithmetic below is this project's (tests/tsdf_oracle.py restates it in numpy float64).
 *
 * svs_tsdf_integrate: integrates n_views <= 16 views into the volume in one launch.  tsdf (n0,n1,n2) float32 (initially 1),
 *   weight (n0,n1,n2) float32 (initially 0), rgb planar (3,n0,n1,n2) float32 or NULL; last axis contiguous, 64-bit indexing.
 *   origin: HOST double[3]; voxel, trunc > 0.  depths: HOST array of n_views DEVICE float (H,W) maps (as svs_fuse_view's
 *   src_depths); masks: the same of DEVICE uint8 (H,W), NULL or NULL entries = no mask; images: DEVICE float (H,W,3) in
 *   [0,1], required for every view when rgb is given and ignored otherwise.  mats: DEVICE double[n_views][21] = K row-major
 *   (9), then the top three rows of E (12).  Per voxel p = origin + (i,j,k) * voxel and per view, all in float64:
 *   cam = E (p,1), z = cam.z, skipped if z <= 0; pix = K cam, u = pix.x / pix.z + 0.5, v = pix.y / pix.z + 0.5, iu = floor(u),
 *   iv = floor(v), skipped outside [0,W) x [0,H); d = depth[iv,iu], skipped if the mask is 0 there or d is not finite or
 *   d <= 0; sdf = d - z, skipped if sdf < -trunc; t = min(1, sdf / trunc).  With n = the views that counted:
 *   w_new = w_old + n, tsdf = (w_old * tsdf_old + sum t) / w_new, colours likewise from image[iv,iu], rounded to float32 once
 *   per launch; a voxel with n = 0 is not written.  SVS_ESHAPE for more than 16 views or H * W == 0, SVS_EINVAL for
 *   voxel or trunc <= 0.  16 B accesses need 16 B aligned arrays (and, for the colour planes, a voxel count that is a
 *   multiple of 4); other volumes take scalar accesses.
 * svs_tsdf_face_keep: cells[f] = the node index (i*n1 + j)*n2 + k of the cell face f came from (svs_mc_emit's active node,
 *   repeated per triangle); keep[f] = 1 iff all eight nodes of that cell have weight >= min_weight: the rule that drops the
 *   faces a TSDF grows between observed and never-observed space.
 * svs_tsdf_vertex_colors: verts DEVICE float[n_verts][3] in volume index units -> out DEVICE float[n_verts][3]: trilinear
 *   over the eight nodes around the vertex in float64 (base index clamped to [0, n-2]), over the nodes with weight > 0 only,
 *   normalised by the sum of their trilinear weights; 0 where that sum is 0. */
int svs_tsdf_integrate(float* tsdf, float* weight, float* rgb, int n0, int n1, int n2, const double SVS_HOST* origin, double voxel,
                       double trunc, const float* const SVS_HOST* depths, const uint8_t* const SVS_HOST* masks,
                       const float* const SVS_HOST* images, const double* mats, int n_views, int H, int W, void* hip_stream);
int svs_tsdf_face_keep(const float* weight, int n0, int n1, int n2, const int* cells, int n_faces, float min_weight,
                       uint8_t* keep, void* hip_stream);
int svs_tsdf_vertex_colors(const float* rgb, const float* weight, int n0, int n1, int n2, const float* verts, int n_verts,
                           float* out, void* hip_stream);

/* ---- a mesh seen from a scan's cameras (svs_hip.meshview; csrc/svs_meshview.hip) -----------------------------------------
 * Depth, face ids, normals and a shaded picture of a triangle mesh per view, and the per-vertex visibility that cuts a mesh
 * to what the cameras and the evaluation masks see.  The reference has no such step; the arithmetic below is this
 * project's (tests/meshview_oracle.py restates it in numpy float64).  Cameras as svs_tsdf_integrate takes them: mats DEVICE
 * double[n_views][21] = K row-major, then the top three rows of E; n_views <= 16 per call.  Per vertex p, in float64 without
 * contraction: cam = E (p,1), z = cam.z, pix = K cam, x = pix.x / pix.z, y = pix.y / pix.z.  Pixel (ix, iy) has its centre
 * at x = ix, y = iy, so the nearest pixel of a point is floor(x + 0.5): the TSDF rule.
 *
 * svs_mesh_raster: verts DEVICE float[n_verts][3], faces DEVICE int[n_faces][3], zbuf DEVICE uint64 (n_views,H,W), which
 *   the CALLER fills with all-ones bits first: calls (chunks of faces, several meshes) compose into one buffer.  Per view
 *   and face f, in this order:
 *   1. skipped if a vertex index is outside [0, n_verts);
 *   2. skipped if a vertex has z <= near or a z, x or y that is not finite (no near-plane clipping: a documented limit);
 *   3. A = (x1-x0)(y2-y0) - (y1-y0)(x2-x0); skipped if A == 0 or A is not finite.  Both orientations are drawn;
 *   4. candidate pixels: the integer points of the bounding box, ceil(min) .. floor(max) per axis,
 *   5. clamped to [0, W-1] x [0, H-1] in float64, before any conversion to int;
 *   6. centre c is covered iff s * e_k(c) >= 0 for k = 0, 1, 2, with e_k(c) = (x_q-x_p)(c.y-y_p) - (y_q-y_p)(c.x-x_p),
 *      (p,q) = (k+1,k+2) mod 3, s = sign(A): inclusive, no top-left rule;
 *   7. b_k = e_k / A, zc = 1 / (b_0/z_0 + b_1/z_1 + b_2/z_2) (summed left to right); a pixel whose float32(zc) is not a
 *      positive finite number is skipped;
 *   8. key = (bits of float32(zc)) << 32 | (face_base + f);
 *   9. zbuf holds the minimum key per pixel (64-bit unsigned atomic minimum): the smallest float32 depth wins, the smaller
 *      id at equal depth; the result does not depend on the order of faces, threads or launches.
 *   A clamped box of at most svs_mesh_raster_small_box() pixels is walked by the lane that set the face up; larger ones go
 *   through a device list to a second kernel whose waves stride one box each.  work: DEVICE int[work_ints], work_ints >=
 *   4 + n_views * n_faces (n_views * n_faces < 2^31: chunk the faces); the call zeroes work[0..3] and leaves work[0] = the
 *   list's length (the (view, face) pairs on the large path).  An empty mesh or no views: nothing is touched,
 *   work included.  flags: 0; for measurements 1 = also count work[1] = the pairs
 *   walked by the small path and the uint64 at work[2] = atomics issued, 2 = the list is built but not drawn, 4 = only the
 *   list is drawn.  face_base >= 0, face_base + n_faces < 2^31.
 * svs_mesh_raster_resolve: per pixel depth DEVICE float (n_views,H,W) = the key's high word as float32, 0 where empty;
 *   face DEVICE int (n_views,H,W) = the low word, -1 where empty.  normal DEVICE float (n_views,H,W,3) or NULL: the unit
 *   normal cross(P1-P0, P2-P0) of the winner's camera-space corners in float64, flipped so that n.z <= 0, 0 where empty.
 *   shade DEVICE uint8 (n_views,H,W,3) or NULL: g = 0.2 + 0.8 |n.z|, code = floor(255 g colour + 0.5) clamped to [0,255],
 *   colour = sum_k (b_k / z_k * zc) * vert_rgb[i_k] / 255 with b_k, zc of the winner at this pixel in float64, or 1 when
 *   vert_rgb (DEVICE uint8[n_verts][3]) is NULL; 255 where empty.  The winner is faces[id - face_base]; ids outside
 *   [face_base, face_base + n_faces) belong to another call's mesh: their normal and shade are left untouched.
 * svs_mesh_vertex_visibility: depth DEVICE float (n_views,H,W); masks: HOST array of n_views DEVICE uint8 (H,W) pointers,
 *   NULL or NULL entries = no mask.  seen, off_mask DEVICE int[n_verts] are ACCUMULATED (the caller zeroes them; more than
 *   16 views: several calls).  Per vertex and view: skipped if z <= near, z, x or y is not finite, or (iu, iv) =
 *   (floor(x+0.5), floor(y+0.5)) is outside the image; off_mask += 1 if the mask is 0 there; otherwise, with d =
 *   depth[iv,iu], seen += 1 iff d == 0 or z <= d * (1 + rel) + abs_tol.
 * SVS_ESHAPE for more than 16 views or H * W == 0, SVS_EINVAL for near <= 0 or a negative tolerance; an empty mesh is not
 * an error.  Bad input (indices out of range, NaN vertices, faces behind the camera) is skipped, never dereferenced. */
int svs_mesh_raster_small_box(void);
int svs_mesh_raster(const float* verts, int n_verts, const int* faces, int n_faces, const double* mats, int n_views, int H,
                    int W, double near, int face_base, unsigned long long* zbuf, int* work, long long work_ints, int flags,
                    void* hip_stream);
int svs_mesh_raster_resolve(const unsigned long long* zbuf, const float* verts, int n_verts, const int* faces, int n_faces,
                            const double* mats, int n_views, int H, int W, int face_base, const uint8_t* vert_rgb, float* depth,
                            int* face, float* normal, uint8_t* shade, void* hip_stream);
int svs_mesh_vertex_visibility(const float* verts, int n_verts, const double* mats, int n_views, int H, int W, double near,
                               const float* depth, const uint8_t* const SVS_HOST* masks, double rel, double abs_tol, int* seen,
                               int* off_mask, void* hip_stream);

/* ---- a mesh painted from a scan's photographs (svs_hip.meshpaint; csrc/svs_meshpaint.hip) --------------------------------
 * Vertex colours for a mesh that has none: every view projects into it, the depth maps of svs_mesh_raster_resolve decide
 * occlusion, views are weighted by viewing angle, vertices no view sees are filled from their neighbours over the mesh's
 * edges.  The reference has no such step; the arithmetic below is this project's (tests/meshpaint_oracle.py restates it in
 * numpy float64).  Cameras, projection, pixel convention, near and the 16 views per call are those of
 * svs_mesh_vertex_visibility; all arithmetic is float64 without contraction.
 *
 * svs_mesh_vertex_normals: accum DEVICE double[n_verts][3], which the CALLER zeroes first: calls (chunks of faces) compose.
 *   Per face with indices inside [0, n_verts) and finite corners, the unnormalised cross(P1-P0, P2-P0) in float64 (area
 *   weighting) is added to accum of each of its three vertices with float64 atomic adds (the last bits of the sum depend
 *   on their order).  Then, unless normals (DEVICE float[n_verts][3]) is NULL, normals = float32(accum / |accum|),
 *   |accum| = sqrt(x x + y y + z z); (0,0,0) where the sum is zero or not finite.  accum is left for the caller.
 * svs_mesh_paint: acc DEVICE double[n_verts][4] = (r, g, b, w), ACCUMULATED (the caller zeroes it; more than 16 views:
 *   several calls).  normals DEVICE float[n_verts][3] or NULL; depth DEVICE float (n_views,H,W) as svs_mesh_raster_resolve
 *   writes it; images: HOST array of n_views DEVICE uint8 (H,W,3) pointers, all required; masks: as in visibility.
 *   cos_min in [0,1], power in [0,8], flags: SVS_PAINT_BEST | SVS_PAINT_ONE_SIDED.  Per vertex p, the views in index
 *   order (one thread walks them: no atomics, one fixed order of the sum, the same bits in every run):
 *   1. projected as visibility does; skipped if z <= near or z, x or y is not finite;
 *   2. skipped unless 0 <= x <= W-1 and 0 <= y <= H-1: the bilinear footprint lies inside the image;
 *   3. (iu, iv) = (floor(x+0.5), floor(y+0.5)); skipped if the mask is 0 there;
 *   4. d = depth[iv,iu]; skipped unless d == 0 or z <= d * (1 + rel) + abs_tol: the visibility rule;
 *   5. with normals: eye_k = -(E[0][k] E[0][3] + E[1][k] E[1][3] + E[2][k] E[2][3]) once per view, t = eye - p,
 *      c = (n.x t.x + n.y t.y + n.z t.z) / sqrt(t.x t.x + t.y t.y + t.z t.z), c = |c| unless SVS_PAINT_ONE_SIDED; a vertex
 *      whose normal is zero or not finite is skipped in every view, a view with c < cos_min (or NaN) is skipped;
 *      w = 1 * c * c ... (power factors, multiplied left to right; no pow; power 0: w = 1).  Without normals w = 1;
 *   6. x0 = floor(x), x1 = min(x0+1, W-1), fx = x - x0, likewise y; per channel on the uint8 codes as float64
 *      colour = ((1-fx) I[y0,x0] + fx I[y0,x1]) (1-fy) + ((1-fx) I[y1,x0] + fx I[y1,x1]) fy, in exactly that order;
 *   7. blend (default): acc.rgb += w colour, acc.w += w.  SVS_PAINT_BEST: acc = (colour, w) iff w > acc.w (strict: the
 *      earlier view wins a tie, across calls too).
 * svs_mesh_paint_finish: where acc.w > 0, rgb (DEVICE uint8[n_verts][3]) = floor(acc.c / acc.w + 0.5) per channel (blend)
 *   or floor(acc.c + 0.5) (SVS_PAINT_BEST), clamped to [0,255], and painted (DEVICE int[n_verts]) = 1; elsewhere rgb is left
 *   as the caller filled it and painted = 0.
 * svs_mesh_paint_spread: one Jacobi round of hole filling in integers; round counts from 1.  work DEVICE int[n_verts][4]
 *   and changed DEVICE int[1] are zeroed by the call.  For every face with indices inside [0, n_verts) and each ordered
 *   pair (a, b) of two different corners of it: if 0 < painted[a] <= round and painted[b] == 0, rgb[a] (three ints) and 1
 *   are added to work[b] atomically.  An edge shared by two faces is met in both and COUNTS TWICE, a boundary edge once:
 *   that is the rule, not an accident.  Then per vertex with count = work[b][3] > 0:
 *   rgb = (2 sum + count) / (2 count) by integer division (the rounded mean), painted = round + 1, *changed = 1.
 *   Integer sums do not depend on their order: the result is exact and the same in every run.  An empty mesh (no vertices
 *   or no faces): nothing is touched, changed included.
 * SVS_ESHAPE for more than 16 views, H * W == 0 or a negative count; SVS_EINVAL for near <= 0, a negative tolerance,
 * cos_min outside [0,1], power outside [0,8], an unknown flag, round < 1 or a null required pointer, with the entry's name
 * in the message; every check comes before any HIP call.  An empty mesh is not an error.  Bad input (indices out of range,
 * NaN or infinite vertices or normals) is skipped, never dereferenced. */
#define SVS_PAINT_BEST 1
#define SVS_PAINT_ONE_SIDED 2
int svs_mesh_vertex_normals(const float* verts, int n_verts, const int* faces, int n_faces, double* accum, float* normals,
                            void* hip_stream);
int svs_mesh_paint(const float* verts, int n_verts, const float* normals, const double* mats, int n_views, int H, int W,
                   double near, const float* depth, const uint8_t* const SVS_HOST* images, const uint8_t* const SVS_HOST* masks,
                   double rel, double abs_tol, double cos_min, int power, int flags, double* acc, void* hip_stream);
int svs_mesh_paint_finish(const double* acc, int n_verts, int flags, uint8_t* rgb, int* painted, void* hip_stream);
int svs_mesh_paint_spread(const int* faces, int n_faces, int n_verts, int round, uint8_t* rgb, int* painted, int* work,
                          int* changed, void* hip_stream);

/* ---- a mesh made smaller: vertex clustering with quadric error metrics (svs_hip.meshsimplify; csrc/svs_meshsimplify.hip) --
 * After Lindstrom, "Out-of-core simplification of large polygonal models" (2000): the vertices of a cell of a uniform grid
 * become one vertex, placed where the planes of the faces that touch the cell meet best.  The reference has no such step;
 * the arithmetic below is this project's (tests/meshsimplify_oracle.py restates it in numpy float64).  All arithmetic is
 * float64 without contraction.  verts DEVICE float[n_verts][3], faces DEVICE int[n_faces][3], colors DEVICE
 * uint8[n_verts][3] or NULL; origin: HOST double[3], <= every coordinate, (max - origin) / h < 2^21; h > 0: the cell size;
 * tol in (0,1).  n_faces <= (2^31 - 1) / 3.
 *
 * A face is VALID when its three indices lie in [0, n_verts), its corners (float32 widened) are finite, and
 * n = cross(P1-P0, P2-P0) has L = sqrt(n.x n.x + n.y n.y + n.z n.z) finite and > 0.  Invalid faces contribute nothing, are
 * never dereferenced past the index check and are absent from the output.
 *
 * svs_mesh_cluster_cells: a corner's cell is per axis floor((p - origin) * (1 / h)) clamped to [0, 2^21), its key
 *   ix | iy << 21 | iz << 42 (csrc/svs_cloud_grid.h).  The occupied cells are those that hold a corner of a valid face;
 *   they are ranked by ascending key.  vert_cell DEVICE int[n_verts] = the rank of v's cell, -1 when no valid face uses v.
 *   *n_cells (HOST int) = the number of occupied cells; output vertex r belongs to cell rank r.  Synchronises the stream.
 *   More than 2^21 occupied cells: SVS_ESHAPE (a face's duplicate key packs three 21-bit ranks).
 * svs_mesh_cluster_solve: every valid face contributes once per corner to that corner's cell -- a face with two corners in
 *   one cell contributes TWICE to it: that is the rule.  With c = origin + (cell index + 0.5) h per axis and
 *   d = -(n.x (P0.x-c.x) + n.y (P0.y-c.y) + n.z (P0.z-c.z)), corner k of face f adds: A_ij += n_i n_j / L (six entries,
 *   (n_i n_j) / L), b_i += (n_i d) / L, e += (d d) / L, m += P_k - c, count += 1, and the colour codes of vertex faces[f][k]
 *   to three integer sums.  ORDER of the float64 sums, a function of the input alone: the pairs (f,k) of a cell ascending in
 *   f, then k, are cut into segments of 64 consecutive pairs; each segment is summed left to right from zero; the segment
 *   sums are summed left to right from zero.  No float atomics.
 *   Solve: eigenvalues l_i and eigenvectors v_i of A by cyclic Jacobi (8 sweeps, rotations (0,1), (0,2), (1,2):
 *   csrc/svs_jacobi3.h, shared with svs_cloud_normals); kept: l_i > tol * max l; mean = m / count;
 *   g_i = -b_i - (A_i0 mean_0 + A_i1 mean_1 + A_i2 mean_2); x = mean + sum over kept i (in index order) of
 *   v_i ((v_i . g) / l_i).  If a component of x is not finite or |x_k| > h (farther than one cell size from the cell's
 *   centre along an axis): x = mean and the fallback bit is set.  out_verts DEVICE float[n_cells][3] = float32(c + x);
 *   info DEVICE int[n_cells] = kept directions (0..3) | fallback << 2; err DEVICE double[n_cells] = x^T A x + 2 b.x + e;
 *   out_colors DEVICE uint8[n_cells][3] (given iff colors is) = (2 sum + count) / (2 count) by integer division.
 *   vert_cell, n_cells: what svs_mesh_cluster_cells gave for the same mesh, origin and h.
 * svs_mesh_cluster_faces_count: a valid face becomes the three ranks of its corners in its own corner order; it is dropped
 *   when two ranks are equal; among faces with the same SET of three ranks the one with the lowest input index survives,
 *   whatever its orientation.  keep DEVICE uint8[n_faces] = 1 for a survivor, offsets DEVICE int[n_faces] = survivors
 *   before f, *count (DEVICE int) = their number.
 * svs_mesh_cluster_faces_emit: out_faces DEVICE int[count][3]: the survivors in input order.
 * workspace: svs_mesh_cluster_workspace_bytes(n_verts, n_faces) bytes serve all three entries that take one; nothing is
 *   kept in it between calls.  Every check comes before any HIP call: SVS_ESHAPE for a negative count, too many faces or
 *   cells, SVS_EINVAL for a null required pointer, h <= 0 or not finite, an origin that is not finite, tol outside (0,1),
 *   colours without their output, with the entry's name in the message.  An empty mesh is not an error. */
size_t svs_mesh_cluster_workspace_bytes(int n_verts, int n_faces);
int svs_mesh_cluster_cells(const float* verts, int n_verts, const int* faces, int n_faces, const double SVS_HOST* origin, double h,
                           void* workspace, int* vert_cell, int SVS_HOST* n_cells, void* hip_stream);
int svs_mesh_cluster_solve(const float* verts, int n_verts, const int* faces, int n_faces, const uint8_t* colors,
                           const double SVS_HOST* origin, double h, double tol, const int* vert_cell, int n_cells, void* workspace,
                           float* out_verts, uint8_t* out_colors, int* info, double* err, void* hip_stream);
int svs_mesh_cluster_faces_count(const float* verts, int n_verts, const int* faces, int n_faces, const int* vert_cell, int n_cells,
                                 void* workspace, uint8_t* keep, int* offsets, int* count, void* hip_stream);
int svs_mesh_cluster_faces_emit(const int* faces, int n_faces, const int* vert_cell, const uint8_t* keep, const int* offsets,
                                int* out_faces, void* hip_stream);

/* ---- a surface from an oriented point cloud: Poisson reconstruction on one dense grid (svs_hip.poisson; csrc/svs_poisson.hip)
 * After Kazhdan, Bolitho and Hoppe, "Poisson surface reconstruction" (2006), on one dense grid; screening is opt-in (below).  The
 * reference has no such step; the arithmetic below is this project's (tests/poisson_oracle.py restates it in numpy float64).
 * The grid is node-centred with shape (n0,n1,n2), last axis contiguous, node (i,j,k) at origin + (i,j,k) h; origin: HOST
 * double[3], finite; h > 0.  Two nodes along every axis, fewer than 2^31 nodes.  Volumes are float32; every per-element
 * computation is float64 without contraction, rounded once on store.
 *
 * A point COUNTS when its three coordinates and (in the splat) its three normal components are finite and, per axis,
 * g = (p - origin) / h, b = floor(g) has 0 <= b <= n - 2; t = g - b.  Corner c = 4 di + 2 dj + dk of its cell (b0,b1,b2) is
 * node (b0+di, b1+dj, b2+dk) and has weight (wx * wy) * wz with w = t for d = 1 and 1 - t for d = 0.
 *
 * svs_poisson_splat: pts DEVICE double[n][3], normals DEVICE float[n][3] (used as given, never renormalised) -> field DEVICE
 *   float planar (4,n0,n1,n2): Vx, Vy, Vz, W.  Corner c of a counted point's cell receives w (nx, ny, nz, 1) (products
 *   w * nx ...).  ORDER of the float64 sums, a function of the input alone: the counted points of a cell ascending by
 *   index are cut into segments of 64; each segment is summed left to right from zero, per corner and component; the
 *   segment sums are summed left to right from zero; a node adds, from zero and in ascending corner order, corner c's sum of
 *   cell (node - (di,dj,dk)) over the cells that exist and hold a point; float32 once.  No float atomics.  counts HOST int[2]
 *   = counted, skipped.  Synchronises the stream.  n >= 1.
 * svs_poisson_divergence: rhs = -(((Vx[i+1] - Vx[i-1]) + (Vy[j+1] - Vy[j-1])) + (Vz[k+1] - Vz[k-1])) / (2 h), values beyond the
 *   grid 0: the solution is smaller inside, like the SDFs svs_mc_classify takes.
 * svs_poisson_apply: y = A x, A x = (6 x - s) / (h h), s = (((((x[i-1] + x[i+1]) + x[j-1]) + x[j+1]) + x[k-1]) + x[k+1]),
 *   0 beyond the grid (Dirichlet).  x and y may not be the same array.  16-byte accesses when n2 % 4 == 0 and both bases
 *   are 16-byte aligned, scalar ones otherwise; the same values either way.  svs_poisson_tile: tile HOST int[3] = the
 *   stencil workgroup's extent along axes 0, 1, 2.
 * svs_poisson_cg: conjugate gradients for A x = rhs from x = 0: r = rhs, p = r, rr = bb = r.r; repeat: q = A p;
 *   alpha = rr / p.q; x += alpha p; r -= alpha q; rn = r.r; beta = rn / rr; rr = rn; p = r + beta p (alpha = 0 when p.q <= 0,
 *   beta = 0 when rr <= 0).  Vectors float32 (x + alpha p etc. in float64, rounded once); dot products float64 over the
 *   stored float32 values: per-workgroup partial sums, then one pass over the partials, one fixed order (the same bytes in
 *   every run).  alpha, beta, rr stay on the device; every check_every iterations and at max_iter the host downloads rn
 *   (8 bytes) and stops when rn <= tol^2 bb.  iterations, residual = sqrt(rn / bb), converged: HOST.  bb == 0 (or not finite):
 *   SVS_EINVAL, "no normal field".  tol in (0,1), max_iter >= 1, check_every >= 1.  Synchronises the stream.
 * svs_poisson_sample: vals DEVICE double[n] = sum over the corners, ascending from zero, of weight * x[node], NaN for a point
 *   that does not count; level HOST = the mean over the counted points (sums per workgroup of 256 points by a binary tree,
 *   thread t of the last pass adding the partials t, t + 256, ... from zero, then the same tree), 0 when none counts;
 *   counted HOST.  Synchronises the stream.  n >= 1.
 * svs_poisson_face_keep: cells[f] = the node index (i*n1 + j)*n2 + k of the cell face f came from (svs_mc_emit's active
 *   node); keep[f] = 1 iff the float64 sum, in corner order from zero, of W over the cell's eight nodes is >= min_density
 *   (a node on an upper face or an index out of range: 0).  Not svs_tsdf_face_keep's rule: a trilinear splat leaves the
 *   far nodes of a surface cell nearly empty.
 *
 * SCREENING (opt-in; after Kazhdan and Hoppe, "Screened Poisson surface reconstruction", 2013, with the point term lumped):
 * the system A + diag(weight W), W the splat's weight plane field[3] (the row sums of S^T S for the trilinear sampling
 * matrix S), used as given and never read back: values that are not negative keep the operator positive definite.
 * tests/poisson_screen_oracle.py restates what follows in numpy float64.
 * svs_screened_apply: a = (6 x - s) / (h h) with s exactly as svs_poisson_apply sums it and 0 beyond the grid,
 *   b = (weight * W) * x, y = float32(a + b).  The operator's diagonal is d = 6 / (h h) + weight * W.  x and y may not be the
 *   same array.  16-byte accesses when n2 % 4 == 0 and x, y and W are 16-byte aligned (field[3] lies 3 n0 n1 n2 floats into
 *   its buffer and need not be), scalar ones otherwise; the same values either way.
 * svs_screened_pcg: conjugate gradients preconditioned by that diagonal for (A + diag(weight W)) x = rhs from x = 0:
 *   r = rhs, p = float32(r / d), rz = sum r (r / d), bb = rn = sum r r; repeat: q = float32(A_s p); alpha = rz / p.q (0 when
 *   p.q <= 0); x = float32(x + alpha p); r = float32(r - alpha q); rn = r.r; rzn = sum r (r / d); beta = rzn / rz (0 when
 *   rz <= 0); rz = rzn; p = float32(r / d + beta p).  z = r / d is never stored: it is formed from W where it is needed.
 *   Dot products float64 over the stored float32 values in svs_poisson_cg's order (per-workgroup partials, then one
 *   workgroup over the partials: a function of the shape alone, the same bytes in every run); the scalars stay on the
 *   device.  The stopping rule, check_every, the three HOST outputs and the 8-byte download are svs_poisson_cg's:
 *   rn <= tol^2 bb; bb == 0 (or not finite): SVS_EINVAL, "no normal field".  Synchronises the stream.
 *   At weight == 0 svs_screened_apply gives svs_poisson_apply's bytes; svs_screened_pcg is then svs_poisson_cg with every
 *   direction scaled by h h / 6: the same iterates up to rounding, not the same bytes.
 * Their checks are svs_poisson_apply's and svs_poisson_cg's, and: weight finite and >= 0 (SVS_EINVAL, "weight" in the
 * message), W not null.
 *
 * Every check comes before any HIP call: SVS_ESHAPE for a grid with fewer than two nodes along an axis or 2^31 nodes or
 * more, n < 1, a negative face count; SVS_EINVAL for a null required pointer, h <= 0 or not finite, an origin that is not
 * finite, with the entry's name in the message. */
int svs_poisson_tile(int SVS_HOST* tile);
size_t svs_poisson_splat_workspace_bytes(int n, int n0, int n1, int n2);
int svs_poisson_splat(const double* pts, const float* normals, int n, int n0, int n1, int n2, const double SVS_HOST* origin, double h,
                      void* workspace, float* field, int SVS_HOST* counts, void* hip_stream);
int svs_poisson_divergence(const float* field, int n0, int n1, int n2, double h, float* rhs, void* hip_stream);
int svs_poisson_apply(const float* x, int n0, int n1, int n2, double h, float* y, void* hip_stream);
size_t svs_poisson_cg_workspace_bytes(int n0, int n1, int n2);
int svs_poisson_cg(const float* rhs, int n0, int n1, int n2, double h, double tol, int max_iter, int check_every, void* workspace,
                   float* x, int SVS_HOST* iterations, double SVS_HOST* residual, int SVS_HOST* converged, void* hip_stream);
size_t svs_poisson_sample_workspace_bytes(int n);
int svs_poisson_sample(const float* x, int n0, int n1, int n2, const double SVS_HOST* origin, double h, const double* pts, int n,
                       void* workspace, double* vals, double SVS_HOST* level, int SVS_HOST* counted, void* hip_stream);
int svs_poisson_face_keep(const float* W, int n0, int n1, int n2, const int* cells, int n_faces, double min_density, uint8_t* keep,
                          void* hip_stream);
int svs_screened_apply(const float* x, const float* W, int n0, int n1, int n2, double h, double weight, float* y, void* hip_stream);
size_t svs_screened_pcg_workspace_bytes(int n0, int n1, int n2);
int svs_screened_pcg(const float* rhs, const float* W, int n0, int n1, int n2, double h, double weight, double tol, int max_iter,
                     int check_every, void* workspace, float* x, int SVS_HOST* iterations, double SVS_HOST* residual,
                     int SVS_HOST* converged, void* hip_stream);

/* ---- numeric-contract self tests (used by tests/test_gpu_parity.py) --------------------------------------- */
int svs_selftest_exp(const float* x, float* y_exp, float* y_expm1, int n, void* hip_stream);
int svs_selftest_arith(const float* a, const float* b, float* quotient, float* sqrt_abs_a, int n, void* hip_stream);
int svs_selftest_cumsum(const float* x, float* y, float* total, int rows, int m, void* hip_stream);
/* total[r] = torch.sum(x[r, :m], -1) of a float32 row in ATen's cascade_sum order (the order of the reference's
 * `pdf / torch.sum(pdf, -1, keepdim=True)`, volsdf/model/ray_sampler.py:149,161, and of `(dists ** 2.).sum(-1)`, :77);
 * svs_selftest_exp evaluates the restated Sleef_expf8_u10 / Sleef_expm1f8_u10 (torch.exp pinned / torch.expm1,
 * ray_sampler.py:130-146,225-227, volsdf/model/density.py:26).  1 <= m <= 16000. */
int svs_selftest_rowsum(const float* x, float* total, int rows, int m, void* hip_stream);

/* ---- host: the training pixels of a step (volsdf/datasets/scene_dataset.py:275-279 `change_sampling_idx`, called by
 * volsdf/vsdf.py:234 after every step) ------------------------------------------------------------------------------
 * out[0..k) = torch.randperm(n)[:k] for the CPU generator whose serialised state (torch.get_rng_state(): 5056 HOST bytes)
 * is rng_state, which is advanced exactly as torch.randperm(n) advances it (n - 1 draws of at::mt19937): the first k
 * iterations of ATen's forward Fisher-Yates shuffle, the remaining draws skipped without being formed -- O(k + n / 624)
 * instead of a shuffle of all n pixels.  HOST pointers; n < 2^32 / 20 (ATen's small-n algorithm). */
int svs_randperm_prefix(unsigned char* rng_state, size_t state_bytes, long long n, long long k, long long* out);

/* ---- launch plans: the device part of a step enqueued by one call --------------------------------------------
 * The launch sequence of VolOpt.train_step (volsdf/vsdf.py:196-235: forward, prior lookup, loss, backward) contains no host
 * decision; the host records it once per configuration with a stream capture and hands the captured hipGraph_t to
 * svs_plan_build, which reads its nodes and edges (kernel, memcpy, memset and empty nodes; anything else: SVS_EINVAL) into
 * a plan: the nodes in a topological order, each on one of <= 12 HIP streams (chains of the dependency graph), one event
 * per edge that crosses streams.  The critical chain (every node hands its stream to the successor with the longest way
 * to the end) is the first chain; side_streams: optional hipStream_t handles of the caller for the 2nd, 3rd ... chain
 * (which hardware queue a stream maps to is decided when it is created -- a caller whose eager schedule runs well hands in
 * the streams of that schedule); chains beyond them get streams the plan creates.  svs_plan_run enqueues the plan with plain launches -- first chain on `hip_stream`, the
 * others on streams the plan owns, ordered behind what `hip_stream` held when the call was made and joined back into it
 * before the call returns -- and does not synchronise.  The graph is never instantiated or launched; it must outlive the
 * plan (the kernel arguments stay in its nodes).  svs_plan_info: counts[8] = nodes, kernels, copies, memsets, empty
 * nodes, streams, events, side streams that start at the entry. */
int svs_plan_build(void* hip_graph, void* const SVS_HOST* side_streams, int n_side_streams, void* SVS_HOST* plan_out);
int svs_plan_run(void* plan, void* hip_stream);
int svs_plan_info(void* plan, int* counts);
/* one line per node in issue order: "<position> s<stream> kernel <name> grid .. | memcpy .. | memset .. | empty", followed by
 * " w<event>" per event waited for in front of it and " r<event>" when an event is recorded behind it (HOST text buffer) */
int svs_plan_describe(void* plan, char* text, size_t capacity);
int svs_plan_destroy(void* plan);

/* ---- a mesh made smoother: connectivity, Taubin smoothing, bilateral normal filtering (svs_hip.meshsmooth;
 * csrc/svs_meshsmooth.hip) ---------------------------------------------------------------------------------------------------
 * Taubin, "A signal processing approach to fair surface design" (1995); Zheng et al., "Bilateral normal filtering for mesh
 * denoising" (2011, local scheme) with the vertex update of Sun et al., "Fast and effective feature-preserving mesh
 * denoising" (2007), Tukey biweights in place of the Gaussians.  The reference has no such step; the arithmetic below is
 * this project's (tests/meshsmooth_oracle.py restates it in numpy float64).  All arithmetic is float64 without contraction,
 * IEEE division and sqrt, no library function.  No float atomics: every sum has one order that depends on the input alone.
 * verts DEVICE float[n_verts][3], faces DEVICE int[n_faces][3].  n_faces <= (2^31 - 1) / 6.
 *
 * A face is VALID exactly as in the svs_mesh_cluster_* section (indices in [0, n_verts), corners finite, cross(P1-P0, P2-P0)
 * of finite length > 0), so it has three different indices.  Invalid faces contribute nothing and are never dereferenced
 * past the index check.  An EDGE is an unordered pair {a, b} of a valid face; its use = the number of (valid face, side)
 * pairs that name it (a face listed twice counts twice); BOUNDARY: use == 1; NON-MANIFOLD: use > 2.
 *
 * svs_mesh_adjacency: flags DEVICE int[n_verts] = SVS_MESH_USED (a corner of a valid face) | SVS_MESH_BOUNDARY (an end of a
 *   boundary edge) | SVS_MESH_NONMANIFOLD (an end of a non-manifold edge).  nbr_start DEVICE int[n_verts + 1], nbr DEVICE
 *   int[6 n_faces] (nbr_start[n_verts] entries written): each distinct neighbour of a vertex once, ascending by index;
 *   nbr_boundary DEVICE uint8, parallel to nbr: 1 where that edge is a boundary edge.  face_start DEVICE int[n_verts + 1],
 *   vert_face DEVICE int[3 n_faces] (face_start[n_verts] entries written): the valid faces of a vertex, ascending by face
 *   index.  face_valid DEVICE uint8[n_faces].  counts HOST int[4] = edges, boundary edges, non-manifold edges, valid faces.
 *   Built from a radix sort of the directed pairs keyed a << 32 | b, run-length passes and scans; integer atomics only
 *   (flags, counts).  Synchronises the stream.  workspace: svs_mesh_smooth_workspace_bytes(n_verts, n_faces) bytes; nothing
 *   is kept in it between calls.
 * svs_mesh_taubin: x DEVICE double[n_verts][3] in and out (the result is in x whatever the parity of the pass count), tmp
 *   DEVICE double[n_verts][3].  iters >= 0, lambda in (0,1], mu in [-2,0], boundary one of SVS_SMOOTH_FIXED / CURVE / FREE.
 *   One iteration = a pass with factor lambda, then a pass with factor mu (skipped when mu == 0: plain Laplacian).  A pass
 *   with factor s is Jacobi (it reads only the previous positions), one lane per vertex i: not USED: y = x; a BOUNDARY vertex
 *   under FIXED: y = x; a BOUNDARY vertex under CURVE: N = its neighbours across boundary edges; FREE or an interior vertex:
 *   N = all neighbours; N empty: y = x; else per component m = the sum of x[j] over N in ascending j, left to right from
 *   zero, and y = x + s * (m / count - x).
 * svs_mesh_face_frames: per valid face from x DEVICE double[n_verts][3]: n = cross(P1-P0, P2-P0), L = sqrt(n.x n.x + n.y n.y
 *   + n.z n.z), normals DEVICE double[n_faces][3] = n / L per component, areas DEVICE double[n_faces] = 0.5 L, centroids
 *   DEVICE double[n_faces][3] = ((P0 + P1) + P2) / 3; zeros for an invalid face.
 * svs_mesh_normal_filter: iters Jacobi passes over normals (in and out; tmp DEVICE double[n_faces][3]); areas and centroids
 *   stay as given.  Per valid face f: s = area_f * n_f; for corner k = 0, 1, 2 each face g of vert_face of that corner,
 *   ascending, g != f: d2 = dx dx + dy dy + dz dz of the centroids, q2 the same of n_f - n_g, a = 1 - d2 / (rs rs),
 *   b = 1 - q2 / (rn rn); skipped unless a > 0 and b > 0; w = (area_g * (a a)) * (b b); s += w * n_g per component.  A face
 *   that shares an edge with f is met at two corners and COUNTS TWICE: that is the rule.  Ls = sqrt(s.s); the new normal is
 *   s / Ls when Ls is finite and > 0, else the old one.  rs > 0 (the spatial support), rn in (0,2] (the support on |n_f - n_g|).
 * svs_mesh_vertex_update: iters Jacobi passes over x (x, tmp as in svs_mesh_taubin) with the normals as given; centroids are
 *   those of the pass's input positions (the expression above).  Per USED vertex i that is not a BOUNDARY vertex under
 *   FIXED, its faces f ascending: d = c_f - x_i, t = (n.x d.x + n.y d.y) + n.z d.z, acc += n_f * t per component;
 *   y = x + acc / count.  SVS_SMOOTH_FIXED or SVS_SMOOTH_FREE only.
 * The arrays nbr_start .. flags are those svs_mesh_adjacency wrote for the same mesh; they are trusted.  nbr, nbr_boundary and
 * vert_face may be null for a mesh without a valid face: they are then never read.
 * Every check comes before any HIP call: SVS_ESHAPE for a negative count or too many faces, SVS_EINVAL for a null required
 * pointer, iters < 0 or a parameter outside its range, with the entry's name in the message.  An empty mesh is not an error. */
#define SVS_MESH_USED 1
#define SVS_MESH_BOUNDARY 2
#define SVS_MESH_NONMANIFOLD 4
#define SVS_SMOOTH_FIXED 0
#define SVS_SMOOTH_CURVE 1
#define SVS_SMOOTH_FREE 2
size_t svs_mesh_smooth_workspace_bytes(int n_verts, int n_faces);
int svs_mesh_adjacency(const float* verts, int n_verts, const int* faces, int n_faces, void* workspace, int* nbr_start, int* nbr,
                       uint8_t* nbr_boundary, int* face_start, int* vert_face, uint8_t* face_valid, int* flags, int SVS_HOST* counts,
                       void* hip_stream);
int svs_mesh_taubin(double* x, double* tmp, int n_verts, const int* nbr_start, const int* nbr, const uint8_t* nbr_boundary,
                    const int* flags, int iters, double lambda, double mu, int boundary, void* hip_stream);
int svs_mesh_face_frames(const double* x, int n_verts, const int* faces, const uint8_t* face_valid, int n_faces, double* normals,
                         double* areas, double* centroids, void* hip_stream);
int svs_mesh_normal_filter(const int* faces, const uint8_t* face_valid, int n_faces, int n_verts, const int* face_start,
                           const int* vert_face, const double* areas, const double* centroids, double* normals, double* tmp, int iters,
                           double rs, double rn, void* hip_stream);
int svs_mesh_vertex_update(double* x, double* tmp, int n_verts, const int* faces, int n_faces, const int* face_start,
                           const int* vert_face, const int* flags, const double* normals, int iters, int boundary, void* hip_stream);

/* ---- a texture atlas baked from a scan's photographs (svs_hip.meshtexture; csrc/svs_meshtexture.hip) ----------------------
 * One chart per valid face, two charts per square cell of the atlas: no unwrapping, no seam pass (the meshes this is for are
 * marching-cubes meshes and their clustered simplifications, whose faces are near-uniform in size).  The reference has no
 * such step; the arithmetic below is this project's (tests/meshtexture_oracle.py restates it in numpy float64).  Cameras,
 * projection, pixel convention and the 16 views per call are those of svs_mesh_paint; all arithmetic is float64 without
 * contraction.  verts DEVICE float[n_verts][3], faces DEVICE int[n_faces][3].
 *
 * THE ATLAS is S x S texels, c <= S <= 32768; texel (i, j) has its centre at x = i, y = j and row 0 is the top row of the
 * picture.  A cell is c x c texels, c >= 6; n = S / c (integer division) cells fit per row; columns and rows from n c on
 * are an unused margin.  Slot s lies in cell q = s >> 1, half h = s & 1, with the cell's origin at (ox, oy) =
 * ((q % n) c, (q / n) c).  Chart corners in the cell's local texel coordinates:
 *   lower (h = 0): A0 = (1, 1), A1 = (c-4, 1), A2 = (1, c-4);    upper (h = 1): A0 = (c-2, c-2), A1 = (2, c-2), A2 = (c-2, 2).
 * Local texel (i, j) BELONGS to the lower chart iff i + j <= c - 2, otherwise to the upper one.  At every point of a
 * chart's closed triangle every bilinear tap with a non-zero weight (step 6 of svs_mesh_paint) is a texel of the same cell
 * that belongs to the same chart (tests/test_meshtexture_cpu.py checks it in exact rationals for c = 6 .. 40).
 *
 * svs_mesh_atlas_slots: a face is VALID exactly as in the svs_mesh_cluster_* section.  Its slot is its rank among the valid
 *   faces in index order (an exclusive scan of the flags, csrc/svs_scan.h).  Its rotation r puts the longest edge on the
 *   chart's hypotenuse: with d_k = dx dx + dy dy + dz dz of P_((k+2)%3) - P_((k+1)%3) in float64, r = 0, then r = 1 if
 *   d_1 > d_r, then r = 2 if d_2 > d_r (strict: the first corner wins a tie).  chart DEVICE int[n_faces] = slot * 4 + r,
 *   -1 for a face that is not valid.  counts DEVICE int[2] = valid faces, the others.  work DEVICE uint8[n_faces]: scratch.
 *   Does not depend on S or c.  n_faces <= (2^31 - 1) / 4.
 * svs_mesh_atlas_uv: n_slots = counts[0].  Face corner (r + k) % 3 sits at A_k.  uv DEVICE float[n_faces][3][2] per face
 *   corner in the OBJ convention, with (x, y) the corner's texel: u = float32((x + 0.5) / S), v = float32(1 - (y + 0.5) / S),
 *   computed in float64; zeros for a face with chart -1.  slot_face DEVICE int[n_slots]: the face of every slot.
 * svs_mesh_atlas_bake: acc DEVICE double[rows][S][4] = (r, g, b, w) per texel, ACCUMULATED as in svs_mesh_paint (the caller
 *   zeroes it; more than 16 views: several calls); rows = ceil(ceil(n_slots / 2) / n) c: only the rows that hold charts.
 *   normals DEVICE float[n_verts][3] (what svs_mesh_vertex_normals gives) or NULL.  Per texel (i, j): its cell, its half by
 *   the ownership rule, its slot; a slot >= n_slots or a column >= n c: not touched.  Else f = slot_face[slot], r from
 *   chart[f], and with (li, lj) the local texel the barycentrics of its centre against A0, A1, A2:
 *     lower: b1 = (li - 1) / (c - 5), b2 = (lj - 1) / (c - 5);   upper: b1 = ((c-2) - li) / (c - 4), b2 = ((c-2) - lj) / (c - 4);
 *     b0 = 1 - b1 - b2.  Gutter texels (outside the triangle; bilinear sampling reads them) are clamped onto it:
 *     b_k = max(b_k, 0), s = b0 + b1 + b2 (left to right), b_k = b_k / s.
 *   p = b0 P_r + b1 P_(r+1) + b2 P_(r+2) per component (corner indices mod 3, float32 widened, summed left to right).  With
 *   normals: m = the same combination of the three vertex normals, L = sqrt(m.x m.x + m.y m.y + m.z m.z), n = m / L; a
 *   texel whose m is not finite or whose L is zero or not finite is skipped in every view.  Then steps 1 to 7 of
 *   svs_mesh_paint for the point p and the normal n, the views in index order (one lane per texel: no atomics, one fixed
 *   order, the same bytes in every run).  near .. flags: as in svs_mesh_paint; SVS_ATLAS_CELL_MAJOR may be added to flags:
 *   lanes then walk the atlas cell by cell instead of row by row (for measurements: the bytes written are the same).
 * svs_mesh_atlas_finish: atlas DEVICE uint8[S][S][3], which the CALLER fills with the fill colour first; covered DEVICE
 *   uint8[S][S], zeroed by the caller.  acc as baked, or NULL; vert_rgb DEVICE uint8[n_verts][3] or NULL.  Per texel that
 *   has a face: acc.w > 0: the code of svs_mesh_paint_finish (blend or SVS_PAINT_BEST), covered = 1; else with vert_rgb:
 *   floor(b0 C_r + b1 C_(r+1) + b2 C_(r+2) + 0.5) per channel, clamped to [0,255], with the clamped b of the bake and C the
 *   codes of the three vertices, covered = 2; else left as filled.  A texel without a face is left as filled.  acc NULL:
 *   every texel takes the vertex-colour branch.
 * svs_mesh_atlas_render: face DEVICE int (n_views,H,W) as svs_mesh_raster_resolve wrote it; rgb DEVICE uint8 (n_views,H,W,3),
 *   which the CALLER fills first.  Per pixel whose id lies in [face_base, face_base + n_faces) with chart >= 0: the three
 *   corners projected, b_k and zc at the pixel as the resolve step takes them, w_k = b_k / z_k * zc; the atlas position
 *   X = w_0 T_0 + w_1 T_1 + w_2 T_2 per axis (left to right), T_k the texel of face corner k recomputed from chart, S and c
 *   in integers; X clamped to [0, S-1] (NaN: 0); then the bilinear formula of step 6 of svs_mesh_paint on the atlas codes,
 *   in that order, and floor(. + 0.5) clamped to [0,255].  No shading factor.  Other pixels are left untouched.
 * SVS_ESHAPE with the entry's name for 2 n n < n_slots, c < 6, S < c, S > 32768, more than 16 views, H * W == 0 or a negative
 * count; SVS_EINVAL as in svs_mesh_paint; every check comes before any HIP call.  An empty mesh and zero views touch nothing
 * (svs_mesh_atlas_slots still writes counts).  Bad input (indices out of range, NaN vertices) is skipped, never dereferenced. */
#define SVS_ATLAS_CELL_MAJOR 256
int svs_mesh_atlas_slots(const float* verts, int n_verts, const int* faces, int n_faces, uint8_t* work, int* chart, int* counts,
                         void* hip_stream);
int svs_mesh_atlas_uv(const int* chart, int n_faces, int n_slots, int S, int c, float* uv, int* slot_face, void* hip_stream);
int svs_mesh_atlas_bake(const float* verts, int n_verts, const float* normals, const int* faces, int n_faces, const int* chart,
                        const int* slot_face, int n_slots, int S, int c, const double* mats, int n_views, int H, int W, double near,
                        const float* depth, const uint8_t* const SVS_HOST* images, const uint8_t* const SVS_HOST* masks, double rel,
                        double abs_tol, double cos_min, int power, int flags, double* acc, void* hip_stream);
int svs_mesh_atlas_finish(const double* acc, const int* faces, int n_faces, int n_verts, const int* chart, const int* slot_face,
                          int n_slots, int S, int c, const uint8_t* vert_rgb, int flags, uint8_t* atlas, uint8_t* covered,
                          void* hip_stream);
int svs_mesh_atlas_render(const int* face, const float* verts, int n_verts, const int* faces, int n_faces, int face_base,
                          const int* chart, const double* mats, int n_views, int H, int W, const uint8_t* atlas, int S, int c,
                          uint8_t* rgb, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SVOLSDF_HIP_H */
