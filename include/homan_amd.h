/*
 * homan_amd.h -- C ABI of libhoman_amd.so: the MI355X-native leaves of HOMan's joint-optimisation hot path.
 *
 * The reference (hassony2/homan) is pure Python; the native code on its hot path lives in third-party CUDA /
 * PyTorch extensions (`neural_renderer`, `sdf`, `mano`) bound through pybind torch extensions.  This header is the
 * drop-in boundary for that native layer: plain C, device pointers + sizes, no torch types.  Each entry point names
 * the reference call site (file:line under /root/reference) whose arithmetic it carries.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP, gfx950) unless stated otherwise; tensors are dense, row-major, fp32 /
 *     int32; the caller owns every buffer (outputs and workspaces), the library allocates nothing;
 *   - all work is enqueued on `stream` and is asynchronous w.r.t. the host (capturable in a hipGraph), except
 *     hm_bench_raster_fwd and the hm_debug_* helpers;
 *   - return value: HM_OK (0) or a negative error code; nothing throws across the ABI;
 *   - re-entrant per (workspace, stream).  State outside the caller's buffers: the four hm_tune_* LAUNCH HINTS (the edge
 *     sweeps' grid, the rasteriser's LDS ballast and workgroup order, the metric-only search's LDS ballast: scheduling only,
 *     never results), which are PER CALLING THREAD (thread-local) and read when an
 *     entry point is called or captured - a thread sets them, issues or captures its launches, restores them; threads do not
 *     see each other's values; and the process-wide hm_debug_* hooks (timing events, capacity overrides: test tools);
 *   - workspaces that hold a reduction ticket (hm_reduce_workspace_bytes, hm_sil_workspace_bytes,
 *     hm_collision_workspace_bytes) must be zero-filled ONCE before first use; the ticket resets itself;
 *   - ALIGNMENT.  A pointer must be aligned to its element type: 4 bytes for fp32 / int32, 8 for double and for 64-bit words,
 *     1 for bytes; a `void*` that stands for typed elements (stated at the entry point) to that type.  A contiguous view into a
 *     larger buffer satisfies this and nothing more.  Where a kernel makes a wider access through a caller's pointer, the entry
 *     point's comment names the parameter and the bytes ("ALIGNMENT: ..."), and every workspace states the alignment of its base
 *     (4, 8 or 16 bytes; what *_workspace_bytes returns is exact, nothing is touched outside it).  A pointer that violates an
 *     ALIGNMENT note, a misaligned workspace base, or a misaligned typed `void*` is refused with HM_ERR_BAD_ARG before anything
 *     is enqueued, set or copied: every access wider than its element type that a kernel makes through a caller's pointer is
 *     covered by such a note and such a check.  NULL optional arguments pass.  The
 *     audit behind the notes (parameter, bytes, kernel and line) is the table of DESIGN.md section 9.
 *
 * `hipStream_t` is declared as an opaque pointer so that the header is usable from plain C hosts (ctypes, cgo...).
 */
#ifndef HOMAN_AMD_H
#define HOMAN_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
typedef struct ihipStream_t* hipStream_t;
#endif

#define HM_OK 0
#define HM_ERR_BAD_ARG (-1)
#define HM_ERR_LAUNCH (-2)
#define HM_ERR_UNSUPPORTED (-3)

/* ------------------------------------------------------------------ rigid transforms
 * reference homan/utils/geometry.py:9-27 (rot6d_to_matrix) + homan/utils/camera.py:108-139
 * (compute_transformation_persp), called from homan/homan.py:298-307 (object) and :341-382 (hand).
 *   verts[n,v,:] = (s * mesh[n,v,:]) @ R(rot6d[n]) + trans[n]      s = |scale[0]| if abs_scale else scale[0]
 * mesh (N,V,3), rot6d (N,3,2), trans (N,3), scale (1), rotmat (N,3,3) optional output, verts (N,V,3). */
int hm_rigid_fwd(const float* mesh, const float* rot6d, const float* trans, const float* scale, int abs_scale, int N,
                 int V, float* rotmat, float* verts, hipStream_t stream);
/* g_terms / weights: HOST arrays of n_terms (<= 5) device pointers (N,V,3) and factors, read at launch; their weighted sum
 * is d/dverts reaching mesh, scale, R, t (NULL entries are skipped).  g_rigid (N,V,3) and g_frame (one 3-vector per
 * frame at g_frame + n*frame_stride, times frame_scale, applied to every vertex) reach R, t only: gradients w.r.t. the
 * mesh-detached twin of the vertices.  Outputs: g_mesh (N,V,3) optional, g_rot6d (N,3,2), g_trans (N,3), g_scale_part (N)
 * optional (sum = d/dscale). */
int hm_rigid_bwd(const float* mesh, const float* rot6d, const float* scale, int abs_scale, const float* const* g_terms,
                 const float* weights, int n_terms, const float* g_rigid, const float* g_frame, int frame_stride,
                 float frame_scale, int N, int V, float* g_mesh, float* g_rot6d, float* g_trans, float* g_scale_part,
                 void* workspace, hipStream_t stream);
/* workspace of hm_rigid_bwd / hm_rigid_bwd_sil (zero-filled once; per-frame tickets reset themselves): with it the frame
 * is split over ceil(V/256) workgroups and the last one finishes; NULL = one workgroup per frame.
 * ALIGNMENT: workspace base 8 bytes (records of doubles behind the tickets), every hm_rigid_bwd* entry; sil_parts 16 bytes in
 * hm_rigid_bwd_sil and hm_rigid_bwd_sil_clips (a face's six doubles are read as three 16-byte pairs; what hm_sil_parts returns
 * for a conforming workspace is so aligned). */
size_t hm_rigid_workspace_bytes(int N);
/* hm_rigid_bwd with the silhouette gradient as one more full term, gathered on the fly from the per-(face, corner) NDC
 * gradients of the edge sweeps (sil_parts = hm_sil_parts(workspace) after an hm_sil_bwd called with grad_verts == NULL;
 * adj_off / adj_items / cam_verts / K / orig_size / F as given to that call): no gather launch, no (N,V,3) round trip. */
int hm_rigid_bwd_sil(const float* mesh, const float* rot6d, const float* scale, int abs_scale, const float* const* g_terms,
                     const float* weights, int n_terms, const double* sil_parts, const int* adj_off, const int* adj_items,
                     const float* cam_verts, const float* K, float orig_size, int F, int N, int V, float* g_rot6d,
                     float* g_trans, float* g_scale_part, void* workspace, int sum_log2q, hipStream_t stream);
/* ORDER-INDEPENDENT SUMS (sum_log2q).  Every reduction on the object's gradient chain - the per-(face, corner) sums of the
 * edge sweeps, the vertex gather, the per-frame sums of the rigid backward - rounds its addends to multiples of the quantum
 * 2^sum_log2q (0 = the default 2^-44; -60 <= sum_log2q <= 0) and adds them in double, which is exact while |sum| < 2^53
 * quanta: the result is a function of the SET of addends, independent of launch geometry, unit composition and atomics'
 * arrival order, and the CPU oracle (oracle/csrc/objchain.c) reproduces it bit for bit.  With the per-term arithmetic in
 * IEEE operations this makes the free-running object trajectory of reference homan/jointopt.py:158-192 bit-equal to the
 * CPU path's.  Callers whose gradients are O(1) or larger (pose initialisation: unnormalised sums of squares) pass a
 * coarser grid, e.g. -24; both calls of a backward (hm_sil_bwd*, hm_rigid_bwd_sil*) must be given the same value. */
/* Off-screen penalty of the object-pose initialisation, reference homan/pose_optimization.py:112-135: hinge on the six
 * clipping planes of the projected vertices (K: ONE (3,3) camera, normalised, orig_size 1), per candidate pose:
 * out[n] = weight * sum_v (...), grad (N,V,3) = d out[n] / d verts[n]. */
int hm_offscreen_fwd(const float* verts, const float* K, int N, int V, float zfar, float weight, float* out, float* grad,
                     hipStream_t stream);
/* Best-ever bookkeeping of the pose initialisation's loop, reference homan/pose_optimization.py:340-353, in one launch:
 * losses_out[i] = sums[i * stride] + extra[i]; if the first minimum (torch.argmin) is < best_loss[0], candidate ind's CURRENT
 * rot6d (6) / trans (3) and the minimum are copied to best_rot6d / best_trans / best_loss (one float, start it at +inf). */
int hm_pose_keep_best(const float* sums, int stride, const float* extra, int n, const float* rot6d, const float* trans,
                      float* best_loss, float* best_rot6d, float* best_trans, float* losses_out, hipStream_t stream);
/* The same evaluation WITHOUT touching a best-ever state, for a caller that walks the candidates of one fit as several independent
 * loops (own Adam state and step counter each, their launches overlapping on separate streams) and applies the rule of :340-353
 * over all of them afterwards: row step[0] - 1 of log (max_steps, 16) receives {minimum of this loop's candidates, its index
 * (int bits; -1: none), 1.0 if some loss is NaN, that candidate's CURRENT rot6d (6) and trans (3), 0 x 4}; step = the device
 * counter of hm_adam_step, read after the step that followed the evaluation. */
int hm_pose_keep_best_log(const float* sums, int stride, const float* extra, int n, const float* rot6d, const float* trans,
                          const int* step, int max_steps, float* log, float* losses_out, hipStream_t stream);
/* One-way edge-chamfer term of the pose initialisation, reference homan/pose_optimization.py:74-88,136-150 (csrc/poseedge.hip).
 * hm_edge_edt: the distance-transform image of a target mask.  ref: (size, size) samples, 0 / 1, `stride` floats per row
 *   (stride >= size; size <= 2048).  Edge band = maxpool_k(ref) - ref > 0 with the window clipped to `size`; d2 = the exact
 *   squared Euclidean distance to the nearest band sample (integer arithmetic); edt[y * stride + x] = float(pow((double) d2,
 *   power)) - power 0.25, the reference's default, as sqrt(sqrt(d2)): its `distance_transform_edt(...) ** (power * 2)` bit
 *   for bit.  band_count (one device int) receives the number of band samples; a mask without any (empty or full target) has
 *   no defined transform (scipy returns distances to a corner there): edt is then all zero and the term vanishes.  Samples
 *   outside (size, size) are not written.  kernel_size odd, <= 7, else HM_ERR_UNSUPPORTED. */
int hm_edge_edt(const float* ref, int size, int stride, int kernel_size, float power, float* edt, int* band_count,
                hipStream_t stream);
/* hm_pose_edge_terms: one pass over the un-pooled coverage alpha (N, stride, stride) of hm_sil_fwd (`alpha_full`) with the
 *   shared keep / ref / edt images (`stride` floats per row, the top-left (size, size) block counts), image = keep * alpha:
 *   terms (N,4) = {mask + lw_chamfer * chamfer, IoU, mask, chamfer} with mask = sum (image - ref)^2, IoU = batch_mask_iou
 *   (+ 1e-6; both as hm_sil_reduce's frame_out on binary masks), chamfer = sum (maxpool_k(image) - image) * edt; terms[4 i]
 *   is what the loop minimises before the off-screen penalty joins (hm_pose_keep_best with stride 4);
 *   grad (N, stride, stride) = d terms[4 i] / d alpha_i = 2 keep (image - ref) + lw_chamfer keep (sum_{q: argmax(q) = p} edt[q]
 *   - edt[p]), zero outside (size, size): the input of hm_sil_bwd mode 3.  argmax(q) is torch's max-pool rule: the first
 *   sample, in row-major order of the window clipped to the image, that holds the window's maximum (an all-zero window
 *   names its top-left sample).  Fixed summation order, no floating-point atomics: two calls agree bit for bit.
 *   kernel_size odd, 3..7, else HM_ERR_UNSUPPORTED; N <= 65535.  workspace: hm_pose_edge_workspace_bytes(N, stride) bytes,
 *   zero-filled once (self-resetting tickets).  ALIGNMENT: workspace base 4 bytes. */
size_t hm_pose_edge_workspace_bytes(int N, int stride);
int hm_pose_edge_terms(const float* alpha, const float* keep, const float* ref, const float* edt, int N, int size, int stride,
                       int kernel_size, float lw_chamfer, float* terms, float* grad, void* workspace, hipStream_t stream);
/* out = s[0] * in   (backward of the losses whose unit gradient is produced forward) */
int hm_scale_by(const float* in, const float* s, long n, float* out, hipStream_t stream);

/* ------------------------------------------------------------------ MANO linear blend skinning
 * reference homan/manomodel.py:84-151 (ManoModel.forward_pca, right hand) + the `mano` layer it calls
 * (manomodel.py:119-123) + "+ mano_trans" of homan/homan.py:356.
 * model: host array of 8 device pointers {v_template (778,3), M (145,2334) = [posedirs ; shapedirs^T],
 *   J_template (16,3), J_shapedirs (16,3,10), lbs_weights (778,16), pca components (16,45), hand_mean (45),
 *   parents (16) int32}.   pca (B,pca_dim>=16; the first 16 columns drive the mesh), rot (B,3), betas (B,10),
 *   trans (B,3) or NULL.  verts (B,778,3); joints (B,16,3) optional.
 *   verts_world (B,778,3) optional: the rigid hand transform of hm_rigid_fwd (rigid_rot6d (B,3,2), rigid_trans (B,3),
 *   rigid_scale (1), no abs) applied in the same launch.
 *   state (hm_mano_state_bytes(B)) optional: kinematic-chain state + posed vertices kept for hm_mano_bwd.
 *   ALIGNMENT: model[4] (lbs_weights) 16 bytes - its rows of 16 weights are read as four float4 - in every hm_mano_* entry. */
int hm_mano_fwd(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas,
                const float* trans, int B, float* verts, float* joints, const float* rigid_rot6d, const float* rigid_trans,
                const float* rigid_scale, float* verts_world, float* state, hipStream_t stream);
size_t hm_mano_workspace_bytes(int B);      /* zero-filled once by the caller (self-resetting per-frame tickets); ALIGNMENT: base 4 bytes */
size_t hm_mano_state_bytes(int B);
/* g_pca_extra (B,pca_dim) optional: g_pca = d/d pca through the mesh + w_extra * g_pca_extra (e.g. the PCA prior).
 * state: what hm_mano_fwd stored for the SAME parameters, or NULL (the chain is then recomputed). */
int hm_mano_bwd(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas, int B,
                const float* g_verts, const float* g_pca_extra, float w_extra, float* g_pca, float* g_rot, float* g_betas,
                float* g_trans, const float* state, void* workspace, hipStream_t stream);
/* hm_rigid_bwd_clips of the hand + hm_mano_bwd in ONE launch (no mesh-gradient buffer in between): mesh = the forward's
 * model-space vertices (B,778,3), rigid_rot6d / rigid_scale = the hand's rigid pose (scale: one per clip of clip_len frames),
 * g_terms .. frame_scale as hm_rigid_bwd_clips, g_rigid_rot6d (B,3,2) / g_rigid_trans (B,3) receive the rigid pose's gradients.
 * Replaces the hand branch of loss.backward() through reference homan/homan.py:341-382 (rigid transform) and
 * homan/manomodel.py:84-151 (LBS).  Same expressions as the two launches; the sums of dR / dt are formed per vertex chunk. */
int hm_mano_bwd_rigid_clips(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas, int B,
                            const float* g_pca_extra, float w_extra, float* g_pca, float* g_rot, float* g_betas,
                            float* g_trans, const float* state, void* workspace, const float* mesh, const float* rigid_rot6d,
                            const float* rigid_scale, const float* const* g_terms, const float* weights, int n_terms,
                            const float* g_rigid, const float* g_frame, int frame_stride, float frame_scale,
                            float* g_rigid_rot6d, float* g_rigid_trans, int clip_len, hipStream_t stream);

/* ------------------------------------------------------------------ silhouette rasteriser + fused masked-MSE / IoU
 * reference homan/losses.py:183-197 (compute_sil_loss_object) and the `neural_renderer` call inside it
 * (losses.py:187; renderer built at losses.py:73-77): projection with the ROI intrinsics K (orig_size), fill_back,
 * hard z-buffer raster at 2S x 2S samples, vertical flip, 2x2 average pool, NMR edge-sweep pseudo-gradient.
 *   verts (B,V,3) camera space; faces (F,3) int32 shared by all frames (faces_bstride = 0) or (B,F,3) (= 3F);
 *   K (B,3,3); pooled (B,S,S) silhouettes out.
 *   Fused loss (all four non-NULL): keep/ref (B,S,S), keep_sum (1) = sum(keep);
 *     loss_out[0] = sum((keep*sil - ref)^2) / keep_sum / B ; loss_out[1] = mean_b IoU_b   (losses.py:188-196).
 *   work_order: B*(S/16)^2 int32 entries (frame << 16 | region) = dispatch order of the (frame, 32x32-sample region)
 *     workgroups (a permutation; expensive ones first), or NULL for frame-major order.
 *   pooled_depth (B,S,S) optional: the depth image nr.Renderer.render returns beside the silhouette (reference
 *     homan/homan.py:391,406): z-buffer (zfar where empty), flipped, 2x2 average pooled.
 *   alpha_full (B,2S,2S) optional: the un-pooled coverage image, vertically flipped like the output = what
 *     nr.Renderer(image_size=2S, anti_aliasing=False) returns (reference homan/pose_optimization.py:89-96); its
 *     backward is hm_sil_bwd mode 3.  With keep / ref given as well, they are (2S,2S)-resolution images and the fused loss is
 *     per SAMPLE (reference homan/pose_optimization.py:140-143); per-frame sums come from hm_sil_reduce(frame_out), the
 *     backward is hm_sil_bwd mode 4.
 *   mask_shared: bit 0 - keep / ref have no batch dimension (one mask for every frame); bit 1 (with (2S,2S) keep / ref) - the
 *     per-sample loss WITHOUT its per-sample outputs: alpha_full may be NULL, nothing of (B,2S,2S) size is written; the masks
 *     must be binary (0 / 1) and the backward is hm_sil_bwd mode 5 (the pose initialisation's loop: 500 candidates write
 *     260 MB less per step).
 *   rigid_rot6d (B,3,2) / rigid_trans (B,3) / rigid_scale (1) / rigid_abs optional: `verts` are then mesh-space and the
 *     rigid transform of hm_rigid_fwd is applied in the face-setup kernel (same arithmetic), so the silhouette chain does
 *     not wait for a separate transform launch; hm_sil_bwd still takes the camera-space vertices.
 *   persistent_outputs != 0: the caller passes the SAME pooled / pooled_depth / keep / ref buffers as in the previous call on
 *     this workspace (a fixed optimisation loop); regions that were background then and are background now are not
 *     rewritten.  0 = every output is written.
 *   S must be a multiple of 16 (32 and <= 512 for the silhouette backward).
 *   ALIGNMENT (hm_sil_fwd and its _clips / _phase_clips / _multi forms): workspace base 16 bytes, in every entry point that takes
 *     this workspace (every hm_sil_*, hm_depth_bwd*, hm_shade_rgb, hm_bench_sil_kernels; hm_sil_parts returns NULL); alpha_full 8 bytes (written as float2); keep and ref 8 bytes in the
 *     per-sample mode, i.e. when given together with alpha_full or with mask_shared bit 1 (read as float2) - the pooled-mode
 *     keep / ref (B,S,S) need 4. */
size_t hm_sil_workspace_bytes(int B, int V, int F, int S);
int hm_sil_fwd(const float* verts, const int* faces, int faces_bstride, const float* K, int B, int V, int F, int S,
               float orig_size, float znear, float zfar, const float* keep, const float* ref,
               const float* keep_sum, float* pooled, float* loss_out, const int* work_order, float* pooled_depth,
               float* alpha_full, int mask_shared, const float* rigid_rot6d, const float* rigid_trans,
               const float* rigid_scale, int rigid_abs, int persistent_outputs, void* workspace, hipStream_t stream);
/* scheduling hint (no reference counterpart, no effect on results): winding class (0: faces as stored, 1: the reversed
 * copies of fill_back) that holds the camera-facing surface of the mesh rendered on this workspace.  hm_sil_fwd rasterises
 * it first and rejects the units of the other class against per-block hidden depths before any per-sample work. */
int hm_sil_hint_near_winding(void* workspace, int winding, hipStream_t stream);
/* deferred loss / IoU reduction of an hm_sil_fwd called with keep/ref but loss_out == NULL (off the critical path) */
int hm_sil_reduce(int B, int V, int F, int S, const float* keep_sum, float* loss_out, float* frame_out, void* workspace,
                  hipStream_t stream);       /* frame_out (B,2) optional: per-frame {sum of squares, IoU}; loss_out may be NULL then */
/* mode 3: grad_pooled is (B,2S,2S) = dL/d alpha_full (rendering without anti-aliasing).
 * mode 4: fused per-sample L2 without anti-aliasing: upstream (B) = dL/d(per-frame sums of squares), all > 0.
 * mode 5: mode 4 for BINARY keep / ref masks: keep (keep alpha - ref) is -1 at every uncovered sample that pulls and +1 at every
 *   covered one that pushes, so the line pass reads no per-sample gradient (same results as mode 4 on such masks, bit for bit).
 * mode 1: upstream (1) = dL/d loss_out[0]; mode 2: same with upstream[0] > 0 guaranteed by the caller (the forward's
 * sweep planes are reused, one launch less); mode 0: grad_pooled (B,S,S) = dL/d pooled.  adj_off (V+1), adj_items (3F):
 * CSR vertex -> (face*3 + corner).  grad_verts (B,V,3) overwritten, or NULL to skip the vertex gather (the
 * per-corner gradients stay in the workspace: hm_sil_parts / hm_rigid_bwd_sil); grad_ndc (B,V,3) optional.
 * ALIGNMENT: workspace base 16 bytes; grad_pooled 8 bytes in mode 3 (read as float2; 4 in mode 0). */
int hm_sil_bwd(const float* verts, const float* K, int B, int V, int F, int S, float orig_size, float eps, int mode,
               const float* upstream, const float* grad_pooled, const float* keep_sum, const int* adj_off,
               const int* adj_items, float* grad_verts, float* grad_ndc, void* workspace,
               int sum_log2q, hipStream_t stream);
/* Backward of the depth image (neural_renderer backward_depth_map, reached from reference homan/homan.py:391,406):
 * grad_pooled_depth (B,S,S) -> grad_verts (B,V,3), for the frame state the last hm_sil_fwd left in `workspace`. */
int hm_depth_bwd(const float* verts, const float* K, int B, int V, int F, int S, float orig_size,
                 const float* grad_pooled_depth, const int* adj_off, const int* adj_items, float* grad_verts,
                 void* workspace, hipStream_t stream);
/* The same with the NON-ZERO STRUCTURE of the upstream image handed over (gflags, optional; S % 64 == 0): B * S * (S / 64) bytes,
 * one per (frame, pixel row, 64-pixel segment), non-zero wherever some pixel of the segment has a non-zero gradient (as
 * hm_ordinal_depth_bwd_flags writes them; a set byte over an all-zero segment is harmless).  An ordinal depth term is zero
 * wherever render and annotation agree on the order - nearly everywhere -, and faces / frames that touch no flagged segment
 * get their exact zeros without being walked.  Same result as hm_depth_bwd.
 * ALIGNMENT: workspace base 16 bytes; gflags 4 bytes (scanned four bytes at a time). */
int hm_depth_bwd_sparse(const float* verts, const float* K, int B, int V, int F, int S, float orig_size,
                        const float* grad_pooled_depth, const int* adj_off, const int* adj_items, float* grad_verts,
                        const unsigned char* gflags, void* workspace, hipStream_t stream);
/* Ordinal depth loss between two rendered layers (0 = object, 1 = hand): reference homan/homan.py:384-419 +
 * homan/lossutils.py:133-169 (as the method intends; the reference call site raises before reaching it).
 * d0, d1 / a0, a1: depth / silhouette renders (B,S,S) f32; m0, m1: instance masks (B,S,S) u8.  frame_part: B*8 floats (8-byte aligned),
 * ZERO-filled once by the caller (per-frame integer records of the chunk workgroups; the call leaves them zero again);
 * rec: 5 floats {num_pairs, n01, sum01, n10, sum10} kept for the backward; out1[0] = loss.
 * workspace: the reduce workspace (see the small losses below), zero-filled once. */
int hm_ordinal_depth_fwd(const float* d0, const float* d1, const float* a0, const float* a1, const unsigned char* m0,
                         const unsigned char* m1, int B, int S, float* frame_part, float* rec, float* out1,
                         void* workspace, hipStream_t stream);
int hm_ordinal_depth_bwd(const float* d0, const float* d1, const float* a0, const float* a1, const unsigned char* m0,
                         const unsigned char* m1, int B, int S, const float* rec, const float* upstream, float* g0,
                         float* g1, hipStream_t stream);
/* ... and the per-segment non-zero flags of both gradient images (flags0 / flags1, see hm_depth_bwd_sparse; both or neither) */
int hm_ordinal_depth_bwd_flags(const float* d0, const float* d1, const float* a0, const float* a1, const unsigned char* m0,
                               const unsigned char* m1, int B, int S, const float* rec, const float* upstream, float* g0,
                               float* g1, unsigned char* flags0, unsigned char* flags1, hipStream_t stream);
/* scheduling hint (no reference counterpart, no effect on results): persistent workgroups of the edge-sweep kernel,
 * default 1280; 768 suits loops whose other streams carry the longer chain (collision + contact terms).  Per calling thread (thread-local),
 * read when hm_sil_bwd is called or captured.  Returns the previous value; blocks <= 0 only queries. */
int hm_tune_sweep_blocks(int blocks);
/* Scheduling hint, no effect on results: bytes of unused dynamic LDS added to every rasteriser launch (3072 caps a CU at 5
 * rasteriser workgroups instead of 6, which leaves registers / LDS for the kernels of the caller's other stream).  Per calling thread (thread-local),
 * read when hm_sil_fwd is called (or captured).  Returns the previous value; bytes < 0 only queries. */
int hm_tune_raster_lds_pad(int bytes);
/* Scheduling hint, no effect on results: adaptive launch order of the rasteriser's workgroups.  While on, the forward launches
 * record the time every workgroup took and the backward's first launch re-sorts the order, longest first, for the next forward
 * of the same workspace (the `work_order` argument only seeds it): what is expensive moves during a fit.  enable > 0 / 0 / < 0
 * (query).  Per calling thread (thread-local), read when hm_sil_fwd / hm_sil_bwd are called (or captured).  Returns the previous value. */
int hm_tune_raster_reorder(int enable);
/* Same for the metric-only nearest-vertex search (small latency-bound workgroups that otherwise take every wave slot of a CU
 * next to the kernel they overlap): 65536 = two search workgroups per CU. */
int hm_tune_nn_lds_pad(int bytes);
/* test hook: cap > 0 shrinks the capacity tables of the sweep work list so that small inputs take the beyond-capacity
 * paths (binary search for a unit's first face, atomically accumulated faces); 0 restores the defaults.  Returns the
 * previous value. */
int hm_debug_sweep_caps(int cap);
/* rgb output of nr.renderer.Renderer.render for the reference's texture_size-1 per-face colours (reference
 * homan/homan.py:535-538 render_limem, light set at :173-176, colours from homan/meshutils.py:7-51): (B,3,S,S) image of
 * the LAST hm_sil_fwd on this workspace (same verts / faces), flat lighting ambient + directional * relu(<n, dir>) on the
 * camera-space face normals, background where no face covers, vertical flip and 2x2 average as the other outputs.
 * textures (B,F,3); light_dir, background: HOST float[3]. */
int hm_shade_rgb(const float* verts, const int* faces, int faces_bstride, const float* textures, int B, int V, int F, int S,
                 const float* light_dir, float intensity_ambient, float intensity_directional, const float* background,
                 float* rgb, void* workspace, hipStream_t stream);
/* device pointer to the (B,F,3,2) DOUBLES left in `workspace` by the last hm_sil_bwd: per-(face, corner) NDC gradients as
 * exact sums on the grid 2^sum_log2q */
const double* hm_sil_parts(const void* workspace, int B, int V, int F, int S);
/* forward intermediates kept in the workspace (tests): face-index map (B,2S,2S) int32, packed NDC faces (B,F,9) */
int hm_sil_read_idx_map(const void* workspace, int B, int V, int F, int S, int* out, hipStream_t stream);
int hm_sil_read_faces9(const void* workspace, int B, int V, int F, int S, float* out, hipStream_t stream);
/* hm_sil_fwd(persistent_outputs = 1) leaves the epilogue of an empty region out when its outputs already hold the empty
 * pattern, which depends on keep / ref.  After loading ANOTHER clip's masks into the same buffers (a resident stepper fitting
 * a stream of clips, reference fit_vid_dataset.py:190-379) call this once: the next forward writes every region again. */
int hm_sil_invalidate_outputs(void* workspace, int B, int V, int F, int S, hipStream_t stream);
/* the (B,F,3,2) doubles of hm_sil_parts copied to a caller's device buffer (tests) */
int hm_sil_read_parts(const void* workspace, int B, int V, int F, int S, double* out, hipStream_t stream);
/* per-face screen boxes (B,F) x 8 bytes {x0|winding<<14, y0, x1, y1} u16 */
int hm_sil_read_boxes(const void* workspace, int B, int V, int F, int S, void* out, hipStream_t stream);
/* "owns at least one sample" flags of the last forward, (B,2,F) bytes: [b][0][f] face f as stored, [b][1][f] its reversed copy */
int hm_sil_read_owned(const void* workspace, int B, int V, int F, int S, void* out, hipStream_t stream);

/* ------------------------------------------------------------------ soft silhouettes (NON-PARITY extra; csrc/softsil.hip)
 * Liu, Li, Chen, Li, "Soft Rasterizer: A Differentiable Renderer for Image-based 3D Reasoning", ICCV 2019, silhouette branch:
 * an image formation of its own that stands BESIDE the hard rasteriser the reference calls at homan/losses.py:187 - the
 * reference has no counterpart, nothing here is compared against it.  What it buys: a true gradient (the hard path's is NMR's
 * pseudo-gradient of a piecewise constant image), also along the camera-space z, and a blur radius the caller can anneal.
 *   verts (B,V,3) camera space, faces (F,3) int32 shared by the frames, K (B,3,3), orig_size: projected exactly as by hm_sil_fwd.
 *   Pixel (row r, column c) of the (B,S,S) image has its centre at x = (2c + 1 - S) / S, y = (S - 1 - 2r) / S (NDC; what the hard
 *   rasteriser gives that pixel without anti-aliasing, output flip included).
 *   A face takes part if its three camera-space z lie strictly inside (znear, zfar), |twice its signed NDC area| >= 1e-10 and its
 *   indices are inside [0, V); winding plays no role.  Other faces contribute nothing and receive a zero gradient.
 *   Per pixel p and face j: d2 = squared NDC distance from p to the nearest of the three edge segments, x = +d2 / sigma if p is
 *   in the closed triangle, else -d2 / sigma; D = sigmoid(x).  An outside pair with d2 >= 16 sigma is dropped exactly (D = 0,
 *   no gradient; sigmoid(-16) = 1.13e-7).  alpha_p = 1 - prod_j (1 - D_jp), the factors 1 - D formed as sigmoid(-x) and
 *   multiplied in ascending face index.
 *   sigma: DEVICE pointer to one float, read by the kernels when they RUN - a captured hipGraph follows a value changed in place
 *   between replays.  A value that is not a positive finite number renders an empty image (alpha = 0, gradient 0).
 *   Backward, the true derivative: d alpha_p / d x_jp = (1 - alpha_p) D_jp, d x / d d2 = +-1 / sigma, d2 to the two end points of
 *   the nearest segment (one of them at a clamped end), then through the projection to all three coordinates of the vertices;
 *   sigma receives none.  alpha = the forward's output for the same arguments; grad_alpha (B,S,S); adj_off (V+1) / adj_items (3F)
 *   as for hm_sil_bwd; grad_verts (B,V,3) is overwritten.
 *   Any S in 1..4096, F >= 1, B >= 1 (else HM_ERR_BAD_ARG, like a NULL pointer: nothing is launched, outputs stay untouched).
 *   workspace: hm_softsil_workspace_bytes bytes (0 for shapes outside that range), no initialisation needed; ALIGNMENT: its base
 *   4 bytes.  Every sum has a
 *   fixed order and no result goes through an atomic: two calls on the same inputs return the same bits. */
size_t hm_softsil_workspace_bytes(int B, int V, int F, int S);
int hm_softsil_fwd(const float* verts, const int* faces, const float* K, int B, int V, int F, int S, float orig_size,
                   float znear, float zfar, const float* sigma, float* alpha, void* workspace, hipStream_t stream);
int hm_softsil_bwd(const float* verts, const int* faces, const float* K, int B, int V, int F, int S, float orig_size,
                   float znear, float zfar, const float* sigma, const float* alpha, const float* grad_alpha,
                   const int* adj_off, const int* adj_items, float* grad_verts, void* workspace, hipStream_t stream);
/* Soft mode of the object-pose initialisation (csrc/softpose.hip; homan_amd/pose_optimization.py, sil_mode="soft").
 * hm_softsil_pose_terms: one pass over the soft images alpha (N,S,S) of hm_softsil_fwd - the candidates of one fit, rendered at
 *   the mask's own size S, orig_size 1 - with ONE shared keep / ref image (S,S) each (0 / 1: keep = mask >= 0, ref = mask > 0),
 *   image = keep * alpha:  terms (N,2) = {mask, IoU}, mask = sum (image - ref)^2, IoU = sum image ref / (sum clamp(image + ref,
 *   0, 1) + 1e-6) - hm_sil_reduce's frame_out layout, so hm_pose_keep_best(_log) takes it with stride 2;
 *   grad (N,S,S) = d mask_i / d alpha_i = 2 keep (keep alpha_i - ref), every sample written: the grad_alpha of hm_softsil_bwd.
 *   alpha is read once and grad written once, with 16-byte accesses where S * S is a multiple of 4 and the four images are
 *   16-byte aligned; the samples are dealt to lanes in the same way otherwise.  Per-workgroup partial sums are added by the
 *   candidate's last workgroup in ascending workgroup index, no floating-point atomics: a candidate's row of terms and its grad
 *   are the same bits whatever N is and from call to call.
 *   1 <= S <= 4096, 1 <= N <= 65535, no NULL pointer, else HM_ERR_BAD_ARG: nothing is launched, the outputs stay untouched.
 *   workspace: hm_softsil_pose_workspace_bytes(N, S) bytes (0 for shapes outside that range), zero-filled once (self-resetting
 *   tickets).  ALIGNMENT: workspace base 4 bytes; alpha, keep, ref, grad 4 bytes (16 selects the vector path, nothing else).
 * hm_sigma_anneal: sigma[0] <- max(sigma[0] * decay, sigma_min) in float32, one multiply and one max, on the stream: the blur
 *   schedule of a captured loop (sigma is the device float the soft kernels read when they run).  0 < decay <= 1,
 *   0 <= sigma_min < inf, else HM_ERR_BAD_ARG.  A sigma that underflows to 0 renders empty, see above. */
size_t hm_softsil_pose_workspace_bytes(int N, int S);
int hm_softsil_pose_terms(const float* alpha, const float* keep, const float* ref, int N, int S, float* terms, float* grad,
                          void* workspace, hipStream_t stream);
int hm_sigma_anneal(float* sigma, float decay, float sigma_min, hipStream_t stream);

/* ------------------------------------------------------------------ small losses (value + unit gradient in one launch)
 * workspace for all of them: hm_reduce_workspace_bytes(), zero-filled once; ALIGNMENT: base 4 bytes, here and wherever a reduce
 * workspace is taken (hm_nn_fwd*, hm_contact_fwd*, hm_ordinal_depth_fwd, the ws_* of hm_pair_terms_fwd_clips, the *_clips forms). */
size_t hm_reduce_workspace_bytes(void);
/* reference homan/losses.py:141-164: out2[0] = mean sum_xy (proj - ref/image_size)^2, out2[1] = mean px distance */
int hm_v2d_fwd(const float* verts, const float* camintr, int hand_nb, const float* ref2d, float image_size, int N,
               int V, float* unit_grad, float* out2, void* workspace, hipStream_t stream);
/* reference homan/lossutils.py:18-36: temporal smoothness of verts (N,V,3), frames interleaved by hand_nb */
int hm_smooth_fwd(const float* verts, int N, int V, int hand_nb, float* unit_grad, float* out1, void* workspace,
                  hipStream_t stream);
/* reference homan/lossutils.py:39-40 and :107-109: out3 = {mean(pca^2), (s_obj-m_obj)^2, (s_hand-m_hand)^2} */
int hm_priors_fwd(const float* pca, long npca, const float* s_obj, const float* m_obj, const float* s_hand,
                  const float* m_hand, float* g_pca, float* g_sobj, float* g_shand, float* out3, hipStream_t stream);
/* reference homan/losses.py:199-242 ('centroid') with the gating of :98-139 (project_bbox :20-49, compute_iou
 * utils/bbox.py:111-135, compute_dist_z utils/geometry.py:69-86).  out1 = un-normalised sum; frame_rec (B,8). */
int hm_inter_fwd(const float* verts_hand, const float* verts_obj, const float* camintr, int B, int Vh, int Vo,
                 float expansion, float zthresh, float* frame_rec, float* out1, void* workspace, hipStream_t stream);
int hm_inter_bwd(const float* frame_rec, const float* upstream, int B, int Vh, int Vo, float* g_hand, float* g_obj,
                 hipStream_t stream);

/* ------------------------------------------------------------------ contact (Chamfer direction hand -> object)
 * reference homan/interactions/contactloss.py:60-79,162-163 (pairwise distances, arg-min over the object) and the
 * metric of homan/losses.py:225-241: metric_out[0] = max_b sqrt(min_ij |h_i - o_j|^2).  nn_idx = nn_d2 = NULL: metric only
 * (the same exact value; object-vertex groups that cannot hold the minimum are skipped by a bounding-sphere test). */
int hm_nn_fwd(const float* verts_hand, const float* verts_obj, int B, int Vh, int Vo, int* nn_idx, float* nn_d2,
              float* metric_out, void* workspace, hipStream_t stream);
/* reference homan/lossutils.py:112-130 -> contactloss.py:149-309 as executed: out1 = mean thresh*tanh(|nn-h|/thresh) */
int hm_contact_fwd(const float* verts_hand, const float* verts_obj, const int* nn_idx, int B, int Vh, int Vo,
                   float thresh, float* g_hand, float* g_obj, float* out1, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------ evaluation point metrics
 * reference homan/eval/pointmetrics.py:17-99 (pytorch3d chamfer_distance, scipy cKDTree): exact brute-force nearest
 * neighbours between x (B,N,3) and y (B,M,3), both directions, d2 = (dx*dx + dy*dy) + dz*dz in fp32, ties to the lowest
 * index.  aff_x / aff_y (B,5) optional per-frame affine applied on load: p' = ((p - c) / div) * mul, row (cx,cy,cz,div,mul).
 * x_d2 / x_idx (B,N) and y_d2 / y_idx (B,M) optional per-point outputs.  out4 (B,4) double: mean d2 x->y, mean d2 y->x,
 * mean distance x->y, mean |x_i - y_i| (NaN when N != M).  workspace: hm_cloud_metrics_workspace_bytes(B, N, M) bytes, no
 * initialisation needed; ALIGNMENT: workspace base 8 bytes (doubles).
 * A frame's values do not depend on the other frames of the call. */
size_t hm_cloud_metrics_workspace_bytes(int B, int N, int M);
int hm_cloud_metrics(const float* x, const float* y, int B, int N, int M, const float* aff_x, const float* aff_y, float* x_d2,
                     int* x_idx, float* y_d2, int* y_idx, double* out4, void* workspace, hipStream_t stream);
/* reference pointmetrics.py:61-90: hands (B*hands, V, 3), frame-major.  From the first hand of each frame: centroids and
 * scales (double, rounded to fp32); pred_centroid_from_gt != 0 centres the prediction on the ground truth's centroid as the
 * reference does (:68).  aff_gt (B,5) = (c_gt, 1, 1), aff_pred (B,5) = (c_pred, s_pred, s_gt) for hm_cloud_metrics;
 * hand_mean (B*hands) double = mean vertex distance of the aligned hands. */
int hm_align_stats(const float* gt_hand, const float* pred_hand, int B, int hands, int V, int pred_centroid_from_gt,
                   float* aff_gt, float* aff_pred, double* hand_mean, hipStream_t stream);

/* ------------------------------------------------------------------ sequence evaluation: key-frame interpolation
 * reference homan/eval/ho3devalutils.py:53-96 (interpolate_res) followed by the per-frame `.dot(camextr)[unorder_idxs]
 * .astype(np.float32)` of evalho3drecons.py:126-127,154-158, for one key of one sequence in one launch (csrc/seqinterp.hip).
 *   key_vals (K,N,3) fp32 device; key_frames: HOST int[K], strictly increasing, key_frames[0] == 0, key_frames[K-1] <= frame_nb;
 *   gather: HOST int[M] rows of N (repeats allowed) or NULL (then M == N); signs: HOST float[3], each +1 or -1 (the diagonal
 *   of camextr); out (frame_nb, M, 3) device, fp32 (out_f64 == 0) or fp64.
 * Frame f with k_j <= f < k_{j+1} receives s + (e - s) * w: the difference in fp32, w = (double)(f - k_j) * (1.0 / (double)(k_{j+1}
 * - k_j)) (np.linspace's weights), product and sum in double, each operation rounded once; frames at or after the last key
 * receive that key's value (K == 1: every frame; the reference raises a NameError there).  The sign is applied to the double,
 * then the fp32 output rounds once; the fp64 output with signs (1,1,1) is what interpolate_res returns.
 * The host arrays are checked first (HM_ERR_BAD_ARG: order, first and last key, gather range, signs) and nothing is enqueued
 * when they fail.  Then they are copied, on `stream`, into the caller's device buffers key_frames_dev (K ints) and gather_dev
 * (M ints; NULL without gather), which the kernel reads: the host arrays are read during the call only (pageable memory), so
 * the call is stream-ordered but not capturable in a hipGraph.  `out` is a typed void pointer: 4 bytes (fp32) or 8 (fp64). */
int hm_keyframe_interp(const float* key_vals, const int* key_frames, int K, int N, int frame_nb, const int* gather, int M,
                       const float* signs, int out_f64, int* key_frames_dev, int* gather_dev, void* out, hipStream_t stream);

/* ------------------------------------------------------------------ hand protocol metrics (csrc/evalalign.hip)
 * The FreiHAND / HO-3D evaluation arithmetic.  The protocol's script is not in the reference tree: the formulas below ARE the
 * definition, pinned by the float64 NumPy restatement of tests/handmetrics_ref.py.  Every floating-point
 * sum is a double formed in a fixed order by the frame's own workgroup: two calls return the same bits, and a frame's values
 * do not depend on the other frames of the call.
 *
 * hm_procrustes_align: pred, gt (B,N,3) fp32 -> aligned (B,N,3) fp32, err (B,N) double = |aligned_i - gt_i| taken on the
 * double value of the aligned point before it is rounded for `aligned`, xform (B,13) double {s, R row-major, t} with
 * aligned = s * pred * R^T + t (row vectors).  Each output is optional (NULL).
 *   mode 0, similarity with an orthogonal factor (reflections allowed; scipy's orthogonal_procrustes on normalised sets):
 *     mu_g, mu_p the means, a = (gt - mu_g) / s1, b = (pred - mu_p) / s2 with s1 = |gt - mu_g|_F + 1e-8, s2 = |pred - mu_p|_F
 *     + 1e-8, M = b^T a = U S V^T, Q = U V^T, sigma = trace S, aligned = (b Q) * sigma * s1 + mu_g;
 *   mode 1, the same with a proper rotation: det(U V^T) < 0 flips the last column of U and the smallest singular value;
 *   mode 2, scale and translation off two anchor points: k = |gt[b] - gt[a]| / |pred[b] - pred[a]| (1 when the denominator is
 *     0), aligned = k * (pred - pred[a]) + gt[a]; R = I.  anchor_a, anchor_b must lie in [0, N) (read in mode 2 only).
 * The SVD is a one-sided Jacobi iteration in double: sweeps over the column pairs (0,1), (0,2), (1,2) until one sweep finds
 * every pair orthogonal to (p.q)^2 <= 2^-100 |p|^2 |q|^2, 30 sweeps at most.  A rank-deficient M (N = 1, collinear or coplanar
 * sets, zero) has its left vectors completed to an orthogonal U: the outputs are finite and a minimiser; N = 1 gives gt.
 * B < 1, N < 1, a NULL input, a mode outside 0..2 or an anchor out of range: HM_ERR_BAD_ARG, nothing launched. */
int hm_procrustes_align(const float* pred, const float* gt, int B, int N, int mode, int anchor_a, int anchor_b, float* aligned,
                        double* err, double* xform, hipStream_t stream);
/* counts[k] = number of dist_i <= t_k, t = np.linspace(0, val_max, steps): t_k = k * (val_max / (steps - 1)) in double and
 * t_{steps-1} = val_max.  dist: n values on the device, fp32 (is_f64 == 0) or double; val_max: HOST pointer to one double
 * (> 0, finite), read during the call; counts: `steps` unsigned 64-bit integers on the device.  Exact: the bin guessed by a
 * division is corrected by comparing against t_k itself.  NaN counts nowhere.  2 <= steps <= 1024; n == 0 is HM_OK, all
 * zero.  PCK = counts / n and AUC = trapz(PCK, t) / val_max are the host's to form from the integers.  Typed void pointers:
 * counts 8 bytes (64-bit words, targets of integer atomics), dist 4 bytes (fp32) or 8 (double). */
int hm_threshold_counts(const void* dist, long n, int is_f64, const double* val_max, int steps, void* counts, hipStream_t stream);
/* F-scores off the squared fp32 nearest-neighbour distances hm_cloud_metrics writes: x_d2 (B,N) of the prediction, y_d2 (B,M)
 * of the ground truth; thresholds: HOST float[T], 1 <= T <= 8, read during the call.  out (B,T,3) double = {precision, recall,
 * F}: precision = #(sqrt((double)x_d2) < (double)th) / N, recall the same over y_d2 / M, F = 2 p r / (p + r), 0 when
 * p + r = 0.  Strict <. */
int hm_fscore(const float* x_d2, const float* y_d2, int B, int N, int M, const float* thresholds, int T, double* out,
              hipStream_t stream);

/* ------------------------------------------------------------------ solid voxels, overlap counts, mesh volume (csrc/solidvox.hip)
 * The hand-object intersection volume of the ObMan protocol.  Not in the reference tree: the rules below ARE the definition
 * (DESIGN.md section 7), pinned bit for bit by the fp32 NumPy restatement of tests/volmetrics_ref.py.
 *
 * Lattice: world-anchored, pitch h (fp32); the centre of voxel index i on any axis is ((float)i + 0.5f) * h, i may be negative.
 * Inside test: the rule of csrc/sdf.hip (csrc/inside_test.h).  Row (j, k) with centre (cy, cz) tests a triangle only if cy and
 * cz lie in the closed fp32 [min, max] of its three vertices' y and z; ray_x_crosses(cy, cz, ...) then gives xhit, every
 * operation fp32 IEEE without contraction; voxel i of the row is inside iff the number of crossings with xhit > centre(i),
 * strictly, is odd.  A face that names a vertex outside [0, V) is skipped.
 *
 * hm_solid_voxels: verts (B,V,3) fp32 and faces (F,3) int32 on the device; boxes: HOST int[B*6] = {i0, j0, k0, nx, ny, nz} per
 * frame, read during the call and copied, on `stream`, into the caller's device buffer boxes_dev (B*6 ints), which the kernels
 * read (pageable memory: stream-ordered, not capturable in a hipGraph).  words (B, NZ, NY, NWX) uint32 on the device: bit t of
 * word w in row (k, j) of frame b is voxel (i0 + 32w + t, j0 + j, k0 + k); every bit outside the frame's own nx, ny, nz is 0;
 * an empty box (an extent of 0) gives zeros.  The call clears `words` itself.  Two calls return the same bits, a frame does not
 * depend on the others, and a voxel does not depend on the box that asked for it.
 * HM_ERR_BAD_ARG, nothing enqueued, outputs untouched: B, V or F < 1, a NULL pointer, a pitch that is not finite and positive,
 * a negative dimension or extent, nx > 32 * NWX, ny > NY, nz > NZ, an index outside [-2^22, 2^22].  `words` is a typed void
 * pointer: 4 bytes. */
int hm_solid_voxels(const float* verts, const int* faces, int B, int V, int F, float pitch, const int* boxes, int NWX, int NY,
                    int NZ, int* boxes_dev, void* words, hipStream_t stream);
/* a (a_sets, B, words_per_frame) and b (B, words_per_frame) uint32 on the device -> counts (B,3) unsigned 64-bit integers
 * {popcount(A & b), popcount(A), popcount(b)} per frame with A the OR of the a_sets arrays of a: two hands are voxelised
 * separately and OR-ed, since parity over a merged mesh would cancel where the hands overlap each other.
 * words_per_frame == 0 is HM_OK, all zero.  Typed void pointers: a, b 4 bytes; counts 8 bytes. */
int hm_voxel_overlap(const void* a, int a_sets, const void* b, int B, long words_per_frame, void* counts, hipStream_t stream);
/* out[b] = |sum_f det(p1 - r, p2 - r, p3 - r)| / 6 with r the frame's vertex 0: differences and determinant in double from the
 * fp32 vertices; thread t of the frame's 256-thread workgroup sums the faces t, t + 256, ... in that order and the 256 sums are
 * folded by a halving tree (s[t] += s[t + w], w = 128 ... 1): the same bits on every call and at every batch position. */
int hm_mesh_volume(const float* verts, const int* faces, int B, int V, int F, double* out, hipStream_t stream);

/* ------------------------------------------------------------------ exact point-to-mesh distance and sign (csrc/surfdist.hip)
 * The surface metrics of homan_amd/pointmetrics.py get_surface_metrics.  Not in the reference tree: the rules below ARE the
 * definition, pinned bit for bit by the fp32 NumPy restatement of tests/surfmetrics_ref.py.  Every
 * operation is fp32 IEEE without contraction; a dot product is (x*x + y*y) + z*z.
 *
 * points (B,N,3), verts (B,V,3) fp32 and faces (F,3) int32 (one topology for all frames) on the device.  Outputs, each optional
 * (NULL) but not all four: d2 (B,N) fp32, face_idx (B,N) int32, inside (B,N) int32 0 / 1, closest (B,N,3) fp32.
 *
 * Distance to a face (a, b, c), Ericson 5.1.5: ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c; d1 = ab.ap, d2 = ac.ap,
 * d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp; vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first region
 * that holds gives the closest point q:
 *   A   d1 <= 0 and d2 <= 0                             q = a
 *   B   d3 >= 0 and d4 <= d3                            q = b
 *   AB  vc <= 0 and d1 >= 0 and d3 <= 0                 q = a + (d1 / (d1 - d3)) ab
 *   C   d6 >= 0 and d5 <= d6                            q = c
 *   AC  vb <= 0 and d2 >= 0 and d6 <= 0                 q = a + (d2 / (d2 - d6)) ac
 *   BC  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0       q = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) (c - b)
 *   interior otherwise: s = (va + vb) + vc              q = (a + (vb / s) ab) + (vc / s) ac
 * and D = |p - q|^2.  A face whose cross product (ab_y ac_z - ab_z ac_y, ab_z ac_x - ab_x ac_z, ab_x ac_y - ab_y ac_x) is
 * exactly (0, 0, 0) is its three segments ab, bc, ca: per segment u -> v, t = ((p - u).(v - u)) / |v - u|^2 clamped to [0, 1]
 * (t = 0 when |v - u|^2 is not positive), q = u + t (v - u); the smallest D wins, ties in the order ab, bc, ca.
 * Per point: d2 = the minimum of D over the faces, face_idx = the lowest face that attains it, closest = that face's q.
 * inside = 1 iff the number of faces with ray_x_crosses(p_y, p_z, a, b, c, &xhit) (csrc/inside_test.h, the voxeliser's rule)
 * and xhit > p_x, strictly, is odd: it means "inside" for a closed mesh only.
 * A face that names a vertex outside [0, V) or has a non-finite coordinate is skipped for distance and sign.  A non-finite
 * point, or a mesh whose every face is skipped, gives d2 = +inf, face_idx = -1, inside = 0, closest = 0.
 * Two calls return the same bits and a frame's values depend neither on B nor on its place in the batch: the minimum and the
 * parity are merged through integer operations only (csrc/surfdist.hip).  workspace: hm_point_mesh_workspace_bytes(B, N, F)
 * bytes (0 for batches large enough that the faces of a frame are not split; NULL is then accepted); the call initialises it
 * on `stream`.  HM_ERR_BAD_ARG, nothing enqueued, outputs untouched: B, N, V or F < 1, a NULL input, all four outputs NULL, a
 * NULL workspace where bytes are needed.  Every index is a 64-bit product of the int sizes: no size is refused for overflow.
 * ALIGNMENT: workspace base 8 bytes (64-bit words, targets of atomicMin). */
size_t hm_point_mesh_workspace_bytes(int B, int N, int F);
int hm_point_mesh_distance(const float* points, const float* verts, const int* faces, int B, int N, int V, int F, float* d2,
                           int* face_idx, int* inside, float* closest, void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------ generalised winding number (csrc/winding.hip)
 * The inside-outside sign for meshes that are not closed (Jacobson et al. 2013): w = the signed solid angle of all faces seen
 * from the point, over 4 pi; 1 inside a closed mesh, 0 outside, and it degrades smoothly where faces are missing.  The opt-in
 * sign of the surface metrics (pointmetrics.get_surface_metrics_signed, sign="winding"); the parity rule above stays the default.
 * Not in the reference tree: the rules below ARE the definition, pinned bit for bit by the NumPy restatement
 * of tests/winding_ref.py.  Every operation is IEEE double from the fp32 inputs, without contraction, in the order written.
 *
 * points (B,N,3), verts (B,V,3), faces (F,3) as hm_point_mesh_distance.  Per point p and face (a, b, c):
 *   A = (double)a - (double)p, B and C likewise; a dot product is (x*x + y*y) + z*z; la = sqrt(A.A), lb = sqrt(B.B), lc = sqrt(C.C);
 *   B x C = (B_y C_z - B_z C_y, B_z C_x - B_x C_z, B_x C_y - B_y C_x); num = (A_x (B x C)_x + A_y (B x C)_y) + A_z (B x C)_z;
 *   den = ((((la lb) lc + (A.B) lc) + (B.C) la) + (C.A) lb)                                    (Van Oosterom and Strackee 1983);
 *   omega = 0 when num == 0 (a point in the face's plane or at one of its vertices), else 2 hm_atan2(num, den).
 * hm_atan2(y, x) (csrc/hm_common.h) is a DEFINED function of plain double + - * / and compares, within 2^-44 rad of atan2:
 *   mx = max(|x|, |y|), mn = min(|x|, |y|); 0 when mx == 0; u = (mn - mx) / (mn + mx) and base = pi/4 when mn > tan(pi/8) mx,
 *   else u = mn / mx and base = 0; z = u u; q = c_19, then q = c_k + z q for k = 18 ... 1 with c_k the double nearest to
 *   (-1)^k / (2k + 1); r = base + (u + (u z) q); r = pi/2 - r when |y| > |x|; r = pi - r when x < 0; r = -r when y < 0
 *   (tan(pi/8) = 0.41421356237309503, pi/4 = 0.7853981633974483, pi/2 = 1.5707963267948966, pi = 3.141592653589793).
 * Exact sum: every omega is rounded to the grid 2^log2q, to nearest with ties to even ((omega + magic) - magic in double with
 * magic = 1.5 * 2^(52 + log2q)), and the quanta are added as a signed 64-bit INTEGER: count (B,N) depends neither on the order
 * of the faces, nor on how they are dealt to workgroups, nor on the batch; two calls return the same bits.  No floating-point
 * atomics.  w = count * 2^log2q / (4 pi).  log2q is the caller's: |omega| < 8, so log2q = max(-44, ceil(log2(F)) - 59)
 * (ops.winding_log2q) keeps F addends below 2^62 quanta; admitted are max(-47, ceil(log2(F)) - 59) <= log2q <= 0 (below -47 the
 * rounding add leaves its exact range).
 * Sign: inside = 1 iff |count| > T with T = (long long)rint(ldexp(6.283185307179586, -log2q)), formed on the host in double:
 * |w| > 0.5, decided in integers; the absolute value makes the rule indifferent to a mesh that is consistently wound the other
 * way.  For a point exactly on the surface the result is deterministic and equal to the restatement, but not meaningful.
 * Counts for nothing: a face that hm_point_mesh_distance skips (a vertex outside [0, V), a non-finite coordinate), and a face of
 * zero area as the search defines it (the fp32 cross product (b - a) x (c - a) is exactly (0, 0, 0): the faces it treats as
 * three segments).  A non-finite point gets count = 0, inside = 0.
 * count: B*N signed 64-bit words, required - it is the accumulator: the call clears it on `stream` where workgroups share a
 * point (the caller zero-fills nothing) and they merge with one 64-bit integer atomicAdd per point.  inside (B,N) int32, optional.
 * No workspace.  Every launch goes on `stream`, nothing is allocated or synchronised.  HM_ERR_BAD_ARG, nothing enqueued, outputs
 * untouched: B, N, V or F < 1, a NULL input, a NULL or misaligned count, a log2q outside the admitted range.  Every index is a
 * 64-bit product of the int sizes.
 * ALIGNMENT: count 8 bytes (typed void pointer: signed 64-bit words, targets of atomicAdd). */
int hm_point_mesh_winding(const float* points, const float* verts, const int* faces, int B, int N, int V, int F, int log2q,
                          void* count, int* inside, hipStream_t stream);

/* ------------------------------------------------------------------ mesh preparation: surface nets on a sign lattice (csrc/remesh.hip)
 * From a raw object mesh (holes, missing caps, any face count) to the closed, oriented mesh of about a thousand vertices that the
 * fits, the collision grid, the voxeliser and the parity sign assume: homan_amd/meshprep.py make_watertight / simplify_mesh, in
 * place of the reference's external ManifoldPlus + ACVD stage (meshprocess/simplifymesh.py).  The rules below ARE the definition
 * (DESIGN.md section 7), pinned bit for bit by the NumPy restatement of tests/meshprep_ref.py.  The topology is a pure function of
 * the sign field (integers only); every floating-point operation is fp32 IEEE without contraction.
 *
 * Lattice.  Corners (i, j, k), 0 <= i < nx and so on, at origin + (float)index * h per axis (one multiply, one add); a flag or a
 * position of corner (i, j, k) is element (k * ny + j) * nx + i.  For a source mesh (ops.lattice_signs): lo, hi = the fp32 bounding
 * box of the vertices named by a face that hm_point_mesh_distance does not skip; R cells along the longest extent, 2 <= R <= 256:
 * h = max(hi - lo) / (float)R, refused unless positive and finite; origin = lo - 1.381966f * h (the offset keeps axis-aligned
 * planes at simple fractions of the box off the lattice planes); n = (int)floorf((hi - lo) / h) + 5 corners per axis, so that two
 * corner layers lie below lo and the last two at least 0.6 h and 1.6 h above hi: the outermost layer is strictly outside the box.
 * Signs.  A corner is inside iff its flag is non-zero and it is not on the outermost layer (an index 0 or n - 1), which is forced
 * outside.  The flags are the caller's: hm_point_mesh_winding's `inside` (|w| > 0.5) for sources that need not be closed, the
 * parity of hm_point_mesh_distance, or any field of one's own.
 * Repair.  A unit lattice face whose corners are a checkerboard (s00 == s11 != s10 == s01) would put four quads on one mesh edge.
 * A pass reads the old field and sets all four corners of every such face (Jacobi: new = old OR marks, no order); passes repeat
 * until one changes nothing.  report[0] = the number of passes that changed something, report[1] = the corners set, report[2] = 1
 * if pass 65 still changed something (the caller's error: the field is not settled), else 0.  The outer layer is never set: a
 * face that touches it has two adjacent corners on it.  Two inside corners diagonally opposite across a CELL are left alone: they
 * give a pinched vertex (two sheets meeting in a point), not an edge with four faces.  With the repair every edge of the output
 * has exactly two faces, of opposite direction: closed and oriented.
 * Vertices.  A cell (ci, cj, ck), corners (ci..ci+1, cj..cj+1, ck..ck+1), is active iff its 8 corners are not all equal; its
 * vertex index is its rank among the active cells in row-major order, ci fastest, then cj, then ck.  With S = the sum over its
 * sign-changing edges of the edge's midpoint in half-cell units (an x-edge from corner (i, j, k): (2i + 1, 2j, 2k); integers, so
 * exact and free of order) and n their count: position_a = origin_a + ((float)S_a / (float)n) * (0.5f * h).
 * Faces.  Every lattice edge whose two ends differ emits one quad.  For an edge along axis a from base corner p, the cells are p
 * shifted by (-1,-1), (0,-1), (0,0), (-1,0) along the axes ((a + 1) % 3, (a + 2) % 3): c0, c1, c2, c3 when p is inside, and the
 * reversed cycle c3, c2, c1, c0 when p is outside, so that normals point from inside to outside and the signed volume is positive;
 * the quad (q0, q1, q2, q3) is the triangles (q0, q1, q2), (q0, q2, q3).  Order: all x-edges, then all y-edges, then all z-edges,
 * each by base corner in row-major order, i fastest.  The order comes from per-row popcounts and an exclusive scan over the rows:
 * no atomic decides a position, two calls give the same bits.
 * Snap.  out = closest (hm_point_mesh_distance's) iff d2 <= (snap_limit * snap_limit) * (h * h), compared in fp32, else the lattice
 * position; snap_limit is in cells, default the cell diagonal 1.7320508f (meshprep.SNAP_LIMIT).  Over a hole the half level of the
 * winding number spans the gap like a film; the limit keeps the film's vertices on the film instead of collapsing onto the rim.
 * Left out: feature-preserving placement (no QEF, no sharp edges), decimation other than through h (the second stage, hm_decimate_*, is the caller's choice), components thinner than a
 * cell (they vanish).  The sign search stays brute force over every corner.
 *
 * The packed field: corner (i, j, k) is bit i & 63 of 64-bit word (k * ny + j) * W + (i >> 6), W = ceil(nx / 64);
 * hm_lattice_words = ny * nz * W (-1 for dimensions that are refused).  Admitted: 2 <= nx, ny, nz <= 512, so that the
 * largest possible output, 6 nx ny nz triangles, and every count and index fit an int.
 * hm_lattice_repair: flags (nz, ny, nx) int32 -> bits: 2 * hm_lattice_words words, the first half is the repaired field (the
 * second is the passes' other buffer); report: 73 ints, cleared by the call ([8 + p] = corners set by pass p).  Atomics: one
 * integer add per changed word into the pass's counter.
 * hm_surface_nets_count: bits -> cell_bits (hm_lattice_words words: the active cells in the field's layout), row_offsets
 * (4 * ny * nz ints: per row k * ny + j the exclusive offsets of its active cells, then of the x-, y-, z-edges it bases) and
 * totals (4 ints: active cells, x-, y-, z-edges).  vertices = totals[0], triangles = 2 * (totals[1] + totals[2] + totals[3]).
 * hm_surface_nets_emit: vertices (max_vertices, 3) fp32 and triangles (max_triangles, 3) int32; the caller sizes them from the
 * totals (one host read); an element beyond a capacity is not written; a capacity of 0 skips that output (its pointer may be
 * NULL).  hm_lattice_snap: lattice, closest (n, 3), d2 (n) -> out (n, 3), snapped (n) int32 0 / 1, optional; n = 0 is HM_OK.
 * Every launch goes on `stream`; nothing is allocated or synchronised.  HM_ERR_BAD_ARG, nothing enqueued, outputs untouched: a
 * NULL pointer (other than the optional ones), a dimension outside the admitted range, a non-finite origin, an h or snap_limit
 * that is not positive and finite, a negative capacity or n, a misaligned bits or cell_bits.
 * ALIGNMENT: bits and cell_bits 8 bytes (typed void pointers: 64-bit words). */
long hm_lattice_words(int nx, int ny, int nz);
int hm_lattice_corners(int nx, int ny, int nz, float ox, float oy, float oz, float h, float* points, hipStream_t stream);
int hm_lattice_repair(const int* flags, int nx, int ny, int nz, void* bits, int* report, hipStream_t stream);
int hm_surface_nets_count(const void* bits, int nx, int ny, int nz, void* cell_bits, int* row_offsets, int* totals,
                          hipStream_t stream);
int hm_surface_nets_emit(const void* bits, const void* cell_bits, const int* row_offsets, const int* totals, int nx, int ny, int nz,
                         float ox, float oy, float oz, float h, int max_vertices, int max_triangles, float* vertices,
                         int* triangles, hipStream_t stream);
int hm_lattice_snap(const float* lattice, const float* closest, const float* d2, long n, float snap_limit, float h, float* out,
                    int* snapped, hipStream_t stream);

/* ------------------------------------------------------------------ mesh preparation, second stage: edge-collapse decimation (csrc/decimate.hip)
 * A closed, oriented mesh (the surface nets of a FINE lattice, or a scan that is already closed) brought down to a vertex budget by
 * memoryless quadric edge collapses in deterministic parallel rounds: ops.collapse_round / ops.decimate_mesh, meshprep.decimate and
 * meshprep.make_watertight_detail.  With it, parts thinner than a cell of the budget lattice (a mug's wall and handle, a
 * blade) survive the budget.  The rules below ARE the definition, pinned bit for bit by the NumPy restatement
 * of tests/decimate_ref.py.  Floating point: doubles formed from the fp32 coordinates, one IEEE add or multiply at a time in the
 * order written; no division, no square root, no contraction, no floating-point atomic.  The output is a function of the input
 * alone, the same bits on every call.
 *
 * State: verts (n, 3) fp32, faces (m, 3) int32, closed and oriented (every undirected edge on exactly two faces, run once in each
 * direction), no face repeats a vertex, every index in range, every vertex named by a face, coordinates finite: the CALLER's
 * contract (the wrappers check it on the host, after dropping the vertices that no face names); 4 <= n <= 2^20, 4 <= m <= 2^22, m even.  E = 3m / 2 edges.  One round:
 *  1 Face quadric.  a, b, c the face's corners in stored order, as doubles: N = (b - a) x (c - a), each component e1y e2z - e1z e2y
 *    (cyclic); d = -((Nx ax + Ny ay) + Nz az); the ten numbers (NxNx, NxNy, NxNz, NyNy, NyNz, NzNz, Nx d, Ny d, Nz d, d d).  No
 *    normalisation: the weight is the squared doubled area.
 *  2 Vertex quadric.  Q_v = the sum over the faces at v in ascending face index, sequential adds from 0.
 *  3 Edges.  Undirected, a < b, numbered in ascending (a, b); c = the third vertex of the face that runs a -> b, d = of the face
 *    that runs b -> a.
 *  4 Placement and cost.  Candidates in fp32: V[a], V[b], (V[a] + V[b]) * 0.5f.  With q = Q_a + Q_b (one add each) and p = (x, y, z)
 *    a candidate as doubles: err = (((((((((q0 x) x + (q3 y) y) + (q5 z) z) + 2 ((q1 x) y)) + 2 ((q2 x) z)) + 2 ((q4 y) z)) + 2 (q6 x))
 *    + 2 (q7 y)) + 2 (q8 z)) + q9.  choice = the first minimum in the order a, b, mid (a later one wins only if strictly less).
 *    l2 = (dx dx + dy dy) + dz dz of b - a in double.  cost = err + (double)regularity * ((l2 l2) l2): the regulariser has the
 *    quadric's units and, where every err is rounding noise (flat regions), sends the shortest edge first.
 *  5 Validity.  All of: cost finite; m > 4; |N(a) & N(b)| == 2 (the neighbour runs are ascending, intersected by a merge);
 *    valence(c) > 3 and valence(d) > 3 (distinct neighbours); for every face that holds exactly one of a, b, with that corner moved
 *    to the chosen candidate: (Nox Nnx + Noy Nny) + Noz Nnz > 0 for the normals of rule 1 before and after (a face of zero area
 *    before or after refuses the edge).
 *  6 Rank.  The valid edges in ascending (cost, l2, edge index) get 0, 1, ...; an invalid edge has rank 2^31 - 1.
 *  7 Selection.  m1[v] = the least rank of a valid edge at v (integer atomicMin: order-independent); m2[w] = min(m1[w], m1[v] for
 *    v in N(w)); an edge is selected iff m2[a] == m2[b] == its rank.  No other selected edge then has an end in N[a] | N[b].
 *  8 Budget.  need = n - target.  Of the selected edges the `need` of lowest rank stay selected.
 *  9 Apply.  V[a] = the candidate; b becomes a in every face; the faces that now repeat a vertex (two per collapse) and the
 *    vertices b are dropped; vertices and faces are compacted in their order.
 * 10 Stop (the caller's loop): n <= target; a round that selects nothing (stuck; not an error); the round limit.
 *
 * Between the entry points the caller sorts and scans (plumbing: ascending sorts of 64-bit signed keys, stable where stated;
 * inclusive scans of int32 flags).  Keys and orders are typed void pointers to signed 64-bit words.
 * hm_decimate_keys: faces -> he_keys (3m words: (u n + w) n + c for the half-edge u -> w of corner u with third vertex c) and
 *   corner_keys (3m words: u 3m + corner index).  Both are then sorted ascending (the keys are distinct).
 * hm_decimate_offsets: he_sorted -> vertex_offsets (n + 1 ints: where vertex v's run starts in BOTH sorted arrays; the run of
 *   he_sorted lists N(v) ascending, the run of corner_sorted its corners in ascending face index) and is_edge (3m ints: u < w).
 *   edge_scan = the inclusive scan of is_edge: the half-edge at slot i with u < w is edge edge_scan[i] - 1.
 * hm_decimate_costs: rules 1-5 -> quadrics (n, 10) doubles, edges (E, 4) ints a b c d, choice (E) 0 / 1 / 2, cost (E), l2 (E)
 *   doubles, valid (E) 0 / 1, cost_keys and l2_keys (E words each: the doubles' bits in an order-preserving signed form; 2^63 - 1
 *   for an invalid edge).  order (E words) = the edge indices sorted stably by l2_keys, then stably by cost_keys.
 * hm_decimate_select: rules 6-7 -> rank (E), m1, m2 (n), selected (E) 0 / 1, selected_by_rank (E: the flag of the edge of rank r
 *   at r, else 0), and the cleared remap (n: v), vertex_keep (n: 1), moved (n: -1).  selected_scan = the inclusive scan of
 *   selected_by_rank.
 * hm_decimate_mark: rules 8-9, first half: selected is cleared where selected_scan[rank] > need; for those that stay remap[b] = a,
 *   vertex_keep[b] = 0, moved[a] = the edge; face_keep (m) = 0 for a face two of whose mapped corners agree.  vertex_scan,
 *   face_scan = the inclusive scans of the keeps; vertex_scan[n - 1] is the new n (the round's ONE host read).
 * hm_decimate_compact: out_verts (max_vertices, 3) and out_faces (max_faces, 3): kept vertex v at vertex_scan[v] - 1, with the
 *   candidate's position if moved[v] names an edge; kept face f at face_scan[f] - 1, corners vertex_scan[remap[.]] - 1.  An element
 *   at or beyond a capacity is not written; a capacity of 0 skips that output (its pointer may be NULL).
 * Every launch goes on `stream`; nothing is allocated, synchronised or read back.  HM_ERR_BAD_ARG, nothing enqueued, outputs
 * untouched: a NULL pointer (other than the optional ones), n or m outside the admitted range or m odd, a regularity that is not
 * finite and >= 0, a negative need or capacity, a misaligned key or order array.
 * ALIGNMENT: he_keys, corner_keys, he_sorted, corner_sorted, cost_keys, l2_keys, order 8 bytes (typed void pointers: 64-bit words). */
int hm_decimate_keys(const int* faces, int n, int m, void* he_keys, void* corner_keys, hipStream_t stream);
int hm_decimate_offsets(const void* he_sorted, int n, int m, int* vertex_offsets, int* is_edge, hipStream_t stream);
int hm_decimate_costs(const float* verts, const int* faces, const void* he_sorted, const void* corner_sorted,
                      const int* vertex_offsets, const int* edge_scan, int n, int m, float regularity, double* quadrics, int* edges,
                      int* choice, double* cost, double* l2, int* valid, void* cost_keys, void* l2_keys, hipStream_t stream);
int hm_decimate_select(const int* edges, const int* valid, const void* order, const void* he_sorted, const int* vertex_offsets, int n,
                       int m, int* rank, int* m1, int* m2, int* selected, int* selected_by_rank, int* remap, int* vertex_keep,
                       int* moved, hipStream_t stream);
int hm_decimate_mark(const int* faces, const int* edges, const int* rank, const int* selected_scan, int need, int n, int m,
                     int* selected, int* remap, int* vertex_keep, int* moved, int* face_keep, hipStream_t stream);
int hm_decimate_compact(const float* verts, const int* faces, const int* edges, const int* choice, const int* remap, const int* moved,
                        const int* vertex_keep, const int* vertex_scan, const int* face_keep, const int* face_scan, int n, int m,
                        int max_vertices, int max_faces, float* out_verts, int* out_faces, hipStream_t stream);

/* ------------------------------------------------------------------ surface contact loss (csrc/surfcontact.hip)
 * Attraction of the points outside a mesh and repulsion of the points inside it, each a tanh-saturated exact distance to the
 * surface (the loss of ObMan, Hasson et al. 2019, on the search above), with both gradients.  Not in the reference tree: the
 * rules below ARE the definition, pinned bit for bit by the fp32 NumPy restatement of
 * tests/surfcontact_ref.py.  Every fp32 operation is IEEE without contraction.
 *
 * points (B,N,3), verts (B,V,3), faces (F,3) as above; weights (N) fp32 >= 0 or NULL (= 1); c_a = contact_thresh and c_r =
 * collision_thresh, positive and finite.  The search is hm_point_mesh_distance's: (D, face, inside) per point.  Per point p:
 *   q, D, the barycentric weights (w0, w1, w2) of q on the winning face (a, b, c), and dv = p - q (world space, as D was formed
 *   from it) come from ONE walk, the search's own (csrc/surfdist_walk.h), so q and D are the bits of hm_point_mesh_distance:
 *     A, B, C give a unit weight; AB (1 - t, t, 0), AC (1 - t, 0, t), BC (0, 1 - t, t) with the region's t; the interior
 *     ((1 - tv) - tw, tv, tw) with tv = vb / s, tw = vc / s; a degenerate face the winning segment's (1 - t, t) on that segment's
 *     own ends u -> v (ab, bc, ca: ca runs from c to a) and 0 on the third vertex.
 *   d = sqrtf(D), c = inside ? c_r : c_a, t = hm_tanh(d / c) (csrc/hm_common.h: IEEE double operations, rounded to fp32),
 *   om = inside ? 1 : weights[i]: the weights belong to the ATTRACTION (a caller restricts attraction to contact zones with
 *   them; repulsion always counts every point),
 *   value u = om * (c * t), slope phi = om * (1 - t * t), g[a] = (phi * dv[a]) / d.
 *   u = 0 and g = 0 when face < 0 (non-finite point, no valid face) or D == 0; the weights are 0 when face < 0.
 * Losses A = sum over the outside points of u / (B N), R = the same over the inside points: the normaliser is B N for both (not
 * the count of either set), both vanish at the surface, so A + R is continuous when a point crosses it.
 * Unit gradients, by the envelope theorem (q minimises the distance over the face: the weights' own derivative drops out):
 *   grad_points[b,i,a] = (float)((double)g[a] / (B N)), for A if the point is outside and for R if it is inside (`inside` tells);
 *   grad_verts_attr / grad_verts_rep [b, faces[face][k], a] = sum over the outside / inside points of the fp32 products
 *   -(w_k * g[a]) (a zero weight adds nothing), / (B N).
 * Sums are exact: every fp32 addend is rounded to the grid 2^log2q (round to nearest even, in double) and added as a 64-bit
 * integer count of quanta; the total is converted as (float)(((double)count * 2^log2q) / (double)(B N)).  The loss adds its B
 * per-frame counts as hi = sum(count >> 32) and lo = sum(count & (2^32 - 1)) and converts (double)hi * 2^32 + (double)lo.  Two
 * calls return the same bits, and a frame's counts depend neither on B nor on its place in the batch.  No floating-point atomics.
 * log2q is the caller's: with M = max(max weights, 1) * max(c_a, c_r, 1), which bounds every addend up to rounding,
 *   log2q = ceil(log2(N M)) - 50
 * keeps N addends of one frame below 2^51 quanta (exact as a double, and as hm_quant's input): N = 778 points on one face at
 * unit weights give -40 (ops.surface_contact_log2q).
 * Outputs: out[2] = (A, R); grad_points (B,N,3); inside (B,N) int32; grad_verts_attr, grad_verts_rep (B,V,3); optional (NULL)
 * per-point detail value (B,N) = u, bary (B,N,3), d2 (B,N), face_idx (B,N).  workspace: hm_surface_contact_workspace_bytes(B, N,
 * V, F) bytes, the caller's; the call zeroes what it needs on `stream`.  Every launch goes on `stream`, nothing is allocated or
 * synchronised: the call can be captured in a hipGraph.  HM_ERR_BAD_ARG, nothing enqueued, outputs untouched: B, N, V or F < 1, a
 * NULL input, required output or workspace, a threshold that is not positive and finite, |log2q| > 100.
 * hm_surface_contact_bwd: the autograd backward, upstream (2) fp32 on the device = (dL/dA, dL/dR):
 *   grad_points[i] = (inside ? upstream[1] : upstream[0]) * unit_points[i]; grad_verts = upstream[0] * unit_verts_attr +
 *   upstream[1] * unit_verts_rep; either output may be NULL (its inputs are then not read).
 * ALIGNMENT: workspace base 8 bytes (64-bit accumulator words, targets of integer atomics, lie at the base; the search's words
 * follow at a multiple of 8). */
size_t hm_surface_contact_workspace_bytes(int B, int N, int V, int F);
int hm_surface_contact_fwd(const float* points, const float* verts, const int* faces, const float* weights, int B, int N, int V,
                           int F, float contact_thresh, float collision_thresh, int log2q, float* out, float* grad_points,
                           int* inside, float* grad_verts_attr, float* grad_verts_rep, float* value, float* bary, float* d2,
                           int* face_idx, void* workspace, hipStream_t stream);
int hm_surface_contact_bwd(const float* unit_points, const int* inside, const float* unit_verts_attr,
                           const float* unit_verts_rep, const float* upstream, long n_points, long n_verts, float* grad_points,
                           float* grad_verts, hipStream_t stream);

/* ------------------------------------------------------------------ observed-depth term (csrc/depthobs.hip)
 * The rendered depth of every layer against a sensor depth map registered with the instance masks.  Not in the reference tree:
 * the rule below IS the definition, pinned bit for bit by the fp32 NumPy restatement of
 * tests/depthobs_ref.py.  Every fp32 operation is IEEE without contraction.
 *
 * L = 1..3 layers; d_l / a_l: depth / silhouette renders (B,S,S) f32; m_l: instance masks (B,S,S) u8; depth_map D (B,S,S) f32,
 * metres, in the camera of the renders.  Pointers of layers >= L are not read (NULL).  Pixel p of frame b is VALID for layer l iff
 *   znear <= D[b,p] <= zfar (false for NaN, +-inf, negative and zero values)  and  m_l[b,p] != 0  and  a_l[b,p] == 1.0f
 *   and  0 <= d_l[b,p] <= zfar (a guard: the rasteriser's depth of a fully covered pixel always is).
 * For a valid pixel r = d_l - D, ar = |r|, rho = ar <= delta ? (0.5f * r) * r : delta * (ar - 0.5f * delta),
 * c_l[b,p] = min(max(r, -delta), delta); c_l = 0 exactly on every other pixel (written in full).
 * Sums are exact: rho and ar are rounded to the grid 2^-32 (in double, round to nearest even) and added as 64-bit integer counts
 * of quanta; with delta <= 1 and zfar <= 100 a frame of 1024^2 pixels stays below 2^59 quanta.  No floating-point atomics; two
 * calls return the same bits, a frame's record and images do not depend on its place in the batch, and the clip's values do not
 * depend on the order of the frames.
 *   records (L,B,2) f32: n[l,b] = valid pixels (exact), (float)((double)Q[l,b] / 2^32) with Q the quanta of sum rho;
 *   N = number of (l,b) with n > 0;  M[l,b] = rint((double)Q / (double)n) (the record's mean, in quanta; double division);
 *   out4[0] = loss = N ? (float)(((double)sum M / 2^32) / (double)N) : 0;
 *   out4[1] = mean |r| over all valid pixels = (float)((((double)hi * 2^32 + (double)lo) / 2^32) / (double)sum n), hi / lo the
 *             sums of the upper / lower 32 bits of the records' |r| quanta; 0 without a valid pixel;
 *   out4[2] = sum n / (pixels with m_l != 0 and a usable D, over all layers), in double, rounded to fp32; 0 when there are none;
 *   out4[3] = N.
 * frame_acc: hm_depth_obs_acc_bytes(L, B) bytes, ZERO-filled once by the caller; the call leaves it zero again (the records'
 * integer words and the ticket of the finishing workgroup).  One launch, nothing allocated or synchronised, no host read: the
 * call can be captured in a hipGraph.
 * hm_depth_obs_bwd (the forward writes the un-scaled c_l, the backward only scales them): upstream (1) fp32 on the device,
 *   g_l[b,p] = c_l[b,p] * w[l,b] with w = (upstream[0] / N) / n[l,b] in fp32, exactly 0 where c_l is 0 or n[l,b] = 0.
 * flags0..2 (for every layer or for none; S % 64 == 0): B * S * (S / 64) bytes per layer, 1 where some pixel of the 64-pixel
 * row segment has a non-zero g_l, else 0 - the `gflags` of hm_depth_bwd_sparse.
 * HM_ERR_BAD_ARG before any HIP call: L outside 1..3, B < 1, S < 1 or S > 1024, delta outside (0, 1], not 0 < znear < zfar <= 100,
 * a NULL buffer of a layer < L, a misaligned pointer.
 * ALIGNMENT: frame_acc 8 bytes.  When S * S is a multiple of 4 (every even S; the rasteriser's sizes are multiples of 16) the
 * kernels move four pixels at a time: d_l, a_l, c_l, g_l and depth_map 16 bytes, m_l 4 bytes.  Other S: element alignment. */
size_t hm_depth_obs_acc_bytes(int L, int B);
int hm_depth_obs_fwd(const float* d0, const float* d1, const float* d2, const float* a0, const float* a1, const float* a2,
                     const unsigned char* m0, const unsigned char* m1, const unsigned char* m2, const float* depth_map, int L,
                     int B, int S, float delta, float znear, float zfar, float* c0, float* c1, float* c2, void* frame_acc,
                     float* records, float* out4, hipStream_t stream);
int hm_depth_obs_bwd(const float* c0, const float* c1, const float* c2, int L, int B, int S, const float* records,
                     const float* out4, const float* upstream, float* g0, float* g1, float* g2, unsigned char* flags0,
                     unsigned char* flags1, unsigned char* flags2, hipStream_t stream);

/* ------------------------------------------------------------------ sensor depth onto the fit's pixel grid (csrc/depthprep.hip)
 * Raw depth frames of a sensor - its own resolution, units and camera - registered into the `depth_map` of hm_depth_obs_fwd:
 * (B,S,S) fp32 metres in the colour camera, exactly 0.0f where nothing was measured.  Not in the reference tree: the rule below
 * IS the definition, pinned bit for bit by the fp32 NumPy restatement of tests/depthprep_ref.py.  Every
 * fp32 operation is IEEE (division included), one rounding each, in the order written, without contraction.
 *
 * frames (B,Hd,Wd): uint16 (frames_f32 == 0) or fp32 (!= 0), a typed void pointer.  Kd, T, Kc: DEVICE arrays, row-major, read
 * by the kernel: Kd (3,3) the depth camera's PIXEL intrinsics, of which fxd = Kd[0], cxd = Kd[2], fyd = Kd[4], cyd = Kd[5] are
 * read (no skew); T (3,4) the rigid transform depth camera -> colour camera, t0..t11; Kc (3,3) the colour camera NORMALISED by
 * the image size as HOMan's `camintr`, of which Kc[0], Kc[2], Kc[4], Kc[5] are read.  *_stride is 0 (one matrix for every frame)
 * or 1 (frame b reads matrix b).  The matrices are not inspected on the host (the call reads nothing there); a non-finite entry
 * only ever drops pixels (every comparison below is false for a NaN).
 * Source validity: z = (float)raw * depth_scale; valid iff znear <= z <= zfar (false for NaN, +-inf, zero, negative values).
 * Edge filter (r = edge_radius, 0 = off): a valid source pixel is dropped if some VALID pixel zn of its (2r+1)^2 window inside
 *   the frame has |zn - z| > (edge_jump_rel * z) + edge_jump_abs.
 * Footprint of a surviving pixel (row v, column u), which covers [u, u+1) x [v, v+1): with S_f = (float)S,
 *   Fx = Kc[0] * S_f, Cx = Kc[2] * S_f, Fy = Kc[4] * S_f, Cy = Kc[5] * S_f;
 *   for (p, q) in {(u, v), (u + 1, v + 1), (u + 0.5, v + 0.5)} (exact in fp32):
 *     X = ((p - cxd) / fxd) * z,  Y = ((q - cyd) / fyd) * z,
 *     Xc = ((t0 * X + t1 * Y) + t2 * z) + t3,  Yc = ((t4 * X + t5 * Y) + t6 * z) + t7,  Zc = ((t8 * X + t9 * Y) + t10 * z) + t11;
 *   zc = Zc of the centre.  Dropped unless znear <= zc <= zfar and Zc >= znear at both corners.
 *   px = (Xc / Zc) * Fx + Cx, py = (Yc / Zc) * Fy + Cy at the two corners; dropped unless all four are within +-2^24.
 *   xa = min(px0, px1), xb = max(px0, px1) (a mirroring transform swaps the ends), likewise ya, yb.  The pixel covers the target
 *   pixels (row, col) whose CENTRE (col + 0.5, row + 0.5) lies in [xa, xb) x [ya, yb):
 *     c0 = max(ceil(xa - 0.5f), 0), c1 = min(ceil(xb - 0.5f), S), col in [c0, c1); rows likewise (clipped to the image).
 *   An empty range writes nothing.  c1 - c0 > max_splat or r1 - r0 > max_splat: the pixel is dropped and counted, not clamped.
 *   Target (row, col) is the pixel ops.depth_render calls (row, col) at size S under the same Kc.
 * Merge: a target pixel keeps the MINIMUM zc it received - an unsigned-integer atomicMin on the bit patterns (zc > 0) straight
 * into `out`, pre-filled with the pattern of +inf; the finish turns what is left of it into 0.0f.  No floating-point atomics: the
 * same bits on every run, at any place in the batch.
 * stats (B,4) int32, by integer adds: valid source pixels, dropped by the edge filter, dropped by the range / projection / splat
 * rules, valid target pixels.
 * Three launches (fill, splat, finish) on `stream`; nothing allocated or synchronised, no host read: capturable in a hipGraph.
 * `out` is the only scratch.
 * HM_ERR_BAD_ARG before any HIP call: a NULL pointer; B, Hd, Wd or S < 1; S > 1024 (the depth term's limit); B > 65535;
 * edge_radius outside 0..3; max_splat < 1; depth_scale not positive and finite; not 0 < znear < zfar <= 100; a negative or
 * non-finite edge_jump_abs / edge_jump_rel; a stride other than 0 or 1; a misaligned pointer.
 * ALIGNMENT: frames to its element (2 bytes uint16, 4 bytes fp32); out 16 bytes when S * S is a multiple of 4 (four pixels per
 * lane in fill and finish), else 4.  Source rows are read 16 bytes per lane where `frames` is 16-byte aligned and Wd is a multiple
 * of 8 (uint16) or 4 (fp32), element by element otherwise: the result is the same. */
int hm_depth_register(const void* frames, int frames_f32, int B, int Hd, int Wd, float depth_scale, const float* Kd, int Kd_stride,
                      const float* T, int T_stride, const float* Kc, int Kc_stride, int S, float znear, float zfar,
                      int edge_radius, float edge_jump_abs, float edge_jump_rel, int max_splat, float* out, int* stats,
                      hipStream_t stream);

/* ------------------------------------------------------------------ mask crops and target masks
 * detectron2 `BitMasks(masks).crop_and_resize(boxes, S)` as called at reference homan/lib2d/maskutils.py:29-30 and :61-64
 * and homan/prepare/gtmasks.py:87-101: ROIAlign (output (S,S), spatial_scale 1, sampling_ratio 0, aligned) of the mask
 * binarised as `!= 0`, in fp32, then >= 0.5.  masks (N,H,W): bytes (masks_f32 == 0) or fp32 (masks_f32 != 0); index (R) int32
 * = the mask of each ROI (NULL: ROI r crops mask r; an entry outside [0, N) gives an empty crop); boxes (R,4) fp32
 * x1 y1 x2 y2 in pixels; out (R,S,S) bytes 0 / 1.  Every operation is rounded to fp32 and the samples of an output pixel
 * are summed in one lane, rows then columns: the decision at an exact 0.5 tie is that of a scalar loop in that order.
 * R == 0 is HM_OK and launches nothing; S <= 0 and non-positive N, H, W are HM_ERR_BAD_ARG.  `masks` (and `target`, `occluders`
 * below) are typed void pointers: 1 byte (bytes) or 4 (fp32). */
int hm_mask_crop_resize(const void* masks, int masks_f32, int N, int H, int W, const int* index, const float* boxes, int R,
                        int S, unsigned char* out, hipStream_t stream);
/* The -1 / 0 / 1 fp32 targets of R ROIs in one launch, pixel for pixel the composition of hm_mask_crop_resize calls.
 *   mode 0, hand (reference maskutils.py:61-65 add_target_hand_occlusions): t = crop(target), then -1 wherever a cropped
 *     occluder is set (the occluder wins);
 *   mode 1, object (maskutils.py:29-36 add_occlusions): target (Nt,S,S) is cropped already; -1 wherever a cropped occluder
 *     is set, then 1 wherever the target is set (the object wins);
 *   mode 2, ground-truth masks (prepare/gtmasks.py:105-107): crop(target) - (any cropped occluder).
 * target (Nt,H,W) (mode 1: (Nt,S,S)) and occluders (No,H,W): bytes or fp32 as above; target_index (R) as `index` above;
 * occluder_index (R,K) int32: the occluder masks of each ROI, entries outside [0, No) are skipped (K == 0: no occluder,
 * the occluder pointers may be NULL); out (R,S,S) fp32. */
int hm_target_masks(int mode, const void* target, int target_f32, int Nt, const int* target_index, const void* occluders,
                    int occluders_f32, int No, const int* occluder_index, int K, int H, int W, const float* boxes, int R, int S,
                    float* out, hipStream_t stream);
/* Per-instance visibility off the face-index map of a render (hm_sil_read_idx_map: (B,2S,2S) int32): `renders[:, i]` of
 * reference prepare/gtmasks.py:77-92 (one-hot face colours, ambient light 1, directional 0) without the (B,3,S,S) float
 * image.  face_start: HOST int[I + 1], instance i owns faces [face_start[i], face_start[i+1]) (I <= 8, else
 * HM_ERR_UNSUPPORTED); out (B,I,S,S) bytes = how many of the pixel's 2x2 samples the instance owns: count / 4 is the
 * anti-aliased render value, count > 0 the instance mask. */
int hm_instance_masks(const int* idx_map, int B, int S, int F, const int* face_start, int I, unsigned char* out,
                      hipStream_t stream);

/* ------------------------------------------------------------------ SDF interpenetration
 * reference homan/lossutils.py:43-64 -> homan/interactions/scenesdf.py:77-148 and the `sdf` package (scenesdf.py:119).
 * Scene = {0: hand (closed faces), 1: object}.  out1[0] = sum of grid_sample(clamp(SDF_k,0), verts_l) over both
 * ordered pairs and all frames; g0 / g1 = d out / d verts0 / d verts1.  ALIGNMENT: workspace base 16 bytes (float4 triangle records), in
 * every hm_collision_* entry. */
size_t hm_collision_workspace_bytes(int B, int V0, int V1, int F0, int F1);
int hm_collision_fwd(const float* verts0, const int* faces0, int V0, int F0, const float* verts1, const int* faces1,
                     int V1, int F1, int B, float scale_factor, float* g0, float* g1, float* out1, void* workspace,
                     hipStream_t stream);
/* per-vertex penetration depths in world units (reference homan/interactions/scenesdf.py:141-146 `dist_values`, read by
 * homan/eval/pointmetrics.py:102-124): dv0 (B,V0) = clamp(SDF of mesh 1, 0) at the vertices of mesh 0 = dist_values[(1,0)],
 * dv1 (B,V1) = dist_values[(0,1)]; from the workspace of the last hm_collision_fwd on the same verts0 / verts1. */
int hm_collision_dist_values(const float* verts0, int V0, const float* verts1, int V1, int F0, int F1, int B, float* dv0,
                             float* dv1, void* workspace, hipStream_t stream);
/* clamp(SDF,0) on the full 32^3 grid of mesh `which`, from the workspace of the last hm_collision_fwd */
int hm_collision_read_grid(const int* faces, int V, int F, int B, int which, int V0, int V1, int F0, int F1, float* phi,
                           void* workspace, hipStream_t stream);
/* what the LAZY evaluation of the last hm_collision_fwd left for mesh `which` (read_grid recomputes every inside voxel): need_mask
 * (B,32,32) 32-bit words, bit i of word [z][y] <-> voxel (z,y,i) was touched by a sample and is inside; need_len (B) = length
 * of the voxel list (= set bits); phi (B,32,32,32) distances, defined only where the need bit is set.  Read-only. */
int hm_collision_read_needed(int B, int which, int V0, int V1, int F0, int F1, void* need_mask, int* need_len, float* phi,
                             void* workspace, hipStream_t stream);

/* ------------------------------------------------------------------ optimiser step + logging
 * reference homan/jointopt.py:138-151,192 (torch.optim.Adam, three groups) and :184-189 (loss_evolution).
 * slots: n_tensors records {float* p, g, m, v; long n; float lr; int pad} (hm_adam_slot_bytes() each);
 * step: TWO device int32 words {completed steps (incremented by the launch), ticket word (zero between launches)};
 * zero_grad != 0 clears g after the update.  `slots` is a typed void pointer: 8 bytes. */
size_t hm_adam_slot_bytes(void);
int hm_adam_step(const void* slots, int n_tensors, int* step, float beta1, float beta2, float eps, int zero_grad,
                 int blocks_per_tensor, hipStream_t stream);
/* hm_log_total_clips + hm_adam_step in one launch: the log row of the step being taken (weighted totals + every slot of
 * `vals`) is written by an extra grid row before the device step counter moves. */
int hm_adam_step_log(const void* slots, int n_tensors, int* step, float beta1, float beta2, float eps, int zero_grad,
                     int blocks_per_tensor, float* vals, const float* weights, int n, int max_steps, float* log, int nclips,
                     hipStream_t stream);
/* log[step[0]*n + i] = src[i] */
int hm_log_scalars(const float* src, int n, const int* step, int max_steps, float* log, hipStream_t stream);

/* ------------------------------------------------------------------ clip batches: C clips, ONE launch per kernel
 * reference: clips are independent optimisations (one HOMan + one Adam per clip, homan/jointopt.py:92-151); the only
 * sharding hook upstream is the strided sample selection of fit_vid_dataset.py:54-55,190.  Frames of one clip stay
 * coupled through the smoothness term (homan/lossutils.py:18-36) and the per-clip normalisers (sum(keep) and 1/B of
 * homan/losses.py:189-194, the means of losses.py:158 / lossutils.py:39-40 / contactloss.py:284-285, the per-clip
 * sums of losses.py:233-239 and scenesdf.py:147), so a batch concatenates whole clips along the frame axis:
 *   - N (or B) = clips * clip_len frames, clip c = frames [c*clip_len, (c+1)*clip_len); clip_len == 0: one clip;
 *   - every per-clip scalar input (scale, s_obj, m_obj, s_hand, m_hand, keep_sum, rigid_scale) is an array with one
 *     entry per clip; every per-clip scalar output is written at out + c*out_stride (+ the offsets of the plain call);
 *   - reduce workspaces hold `clips` slices of hm_reduce_workspace_bytes() back to back (zero-filled once);
 *   - the clips must share V, F, S and the face topology; vertices, masks, cameras are per frame as before.
 * Each clip's sums are formed by its own workgroups in the order of a single-clip launch: a batched call returns, per
 * clip, bit-identical results to the plain entry point called on that clip alone (tests/test_clip_batch_gpu.py).
 * The plain entry points above are these with clip_len = 0, out_stride = 0. */
int hm_rigid_fwd_clips(const float* mesh, const float* rot6d, const float* trans, const float* scale, int abs_scale, int N,
                       int V, float* rotmat, float* verts, int clip_len, hipStream_t stream);
int hm_rigid_bwd_clips(const float* mesh, const float* rot6d, const float* scale, int abs_scale,
                       const float* const* g_terms, const float* weights, int n_terms, const float* g_rigid,
                       const float* g_frame, int frame_stride, float frame_scale, int N, int V, float* g_mesh,
                       float* g_rot6d, float* g_trans, float* g_scale_part, void* workspace, int clip_len,
                       hipStream_t stream);
int hm_rigid_bwd_sil_clips(const float* mesh, const float* rot6d, const float* scale, int abs_scale,
                           const float* const* g_terms, const float* weights, int n_terms, const double* sil_parts,
                           const int* adj_off, const int* adj_items, const float* cam_verts, const float* K,
                           float orig_size, int F, int N, int V, float* g_rot6d, float* g_trans, float* g_scale_part,
                           void* workspace, int clip_len, int sum_log2q, const float* smooth_verts, float smooth_weight,
                           hipStream_t stream);
/*   smooth_verts (optional): camera-space vertices (N,V,3) of the same mesh; the gradient of smooth_weight * the temporal
 *   smoothness term of every clip (reference homan/lossutils.py:18-36) is formed inside the launch and added before g_terms -
 *   the floats hm_smooth_fwd_clips' unit gradient times the weight gives as a first term, without waiting for that launch. */
/* out[c] = w0 * sum(parts[c*n .. c*n+n)) + w1 * extra[c] */
int hm_sum_small_clips(const float* parts, int n, float w0, const float* extra, float w1, float* out, int nclips,
                       hipStream_t stream);
int hm_mano_fwd_clips(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas,
                      const float* trans, int B, float* verts, float* joints, const float* rigid_rot6d,
                      const float* rigid_trans, const float* rigid_scale, float* verts_world, float* state, int clip_len,
                      hipStream_t stream);
/* Two hands per frame arrive interleaved frame-major [h0_t0, h1_t0, h0_t1, ...] and hand i is the strided slice i::hand_nb of
 * every MANO parameter, through the MANO model of ITS side (reference homan/homan.py:62-63,343-358).  The *_rows entry points
 * evaluate such a slice in place: frame f of the launch is row row0 + f * row_stride of EVERY per-row array (parameters,
 * gradients, vertices, state; all sized for B * row_stride rows); clip_len counts rows. */
int hm_mano_fwd_rows(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas,
                     const float* trans, int B, float* verts, float* joints, const float* rigid_rot6d,
                     const float* rigid_trans, const float* rigid_scale, float* verts_world, float* state, int clip_len,
                     int row0, int row_stride, hipStream_t stream);
int hm_mano_bwd_rows(const void* const* model, const float* pca, int pca_dim, const float* rot, const float* betas, int B,
                     const float* g_verts, const float* g_pca_extra, float w_extra, float* g_pca, float* g_rot, float* g_betas,
                     float* g_trans, const float* state, void* workspace, int row0, int row_stride, hipStream_t stream);
int hm_sil_fwd_clips(const float* verts, const int* faces, int faces_bstride, const float* K, int B, int V, int F, int S,
                     float orig_size, float znear, float zfar, const float* keep, const float* ref,
                     const float* keep_sum, float* pooled, float* loss_out, const int* work_order, float* pooled_depth,
                     float* alpha_full, int mask_shared, const float* rigid_rot6d, const float* rigid_trans,
                     const float* rigid_scale, int rigid_abs, int persistent_outputs, void* workspace, int clip_len,
                     int out_stride, float* cam_verts_out, hipStream_t stream);
/*   cam_verts_out (B,V,3) optional (with the rigid_* arguments): the camera-space vertices = what hm_rigid_fwd returns for
 *   the same inputs (same arithmetic, same floats), written by extra workgroups of the face-setup launch. */
/* The same forward in two calls, for a caller that forks a second stream off the camera-space vertices: phases = 1 launches
 * the face setup only (cam_verts_out is complete when it ends), 2 the rasteriser (+ reduction) only, 3 both; both calls take
 * the same arguments. */
int hm_sil_fwd_phase_clips(const float* verts, const int* faces, int faces_bstride, const float* K, int B, int V, int F, int S,
                           float orig_size, float znear, float zfar, const float* keep, const float* ref,
                           const float* keep_sum, float* pooled, float* loss_out, const int* work_order, float* pooled_depth,
                           float* alpha_full, int mask_shared, const float* rigid_rot6d, const float* rigid_trans,
                           const float* rigid_scale, int rigid_abs, int persistent_outputs, void* workspace, int clip_len,
                           int out_stride, float* cam_verts_out, int phases, hipStream_t stream);
/* Several renders - their own meshes (V, F, vertices, faces), cameras, outputs and workspaces - as ONE face-setup launch and ONE
 * raster launch.  reference: the ordinal depth term renders the object twice per iteration (ROI silhouette homan/losses.py:187,
 * full-image depth homan/homan.py:391) and the hand once (homan.py:406); clips of a dataset come with their own meshes
 * (homan/datasets/core50.py:22-42) - a render per mesh is the per-frame mesh offset table of such a batch.  Every field means
 * what the argument of the same name means in hm_sil_fwd_clips (no alpha_full: anti-aliased renders only; the loss / IoU
 * reduction of a render with keep / ref: hm_sil_reduce_clips or the backward's loss_out).  The launch hints (hm_tune_raster_*)
 * apply as in hm_sil_fwd_clips: each render keeps its own (static or adaptive) order, render after render.
 * Results = n separate hm_sil_fwd_clips calls, bit for bit; each render's backward runs on its own workspace as before.
 * n <= 4; the workspaces must be distinct.  phases: 1 = face setup, 2 = raster, 3 = both. */
typedef struct HmSilRender {
    const float* verts; const int* faces; const float* K; const float* keep; const float* ref; float* pooled;
    const int* work_order; float* pooled_depth; const float* rigid_rot6d; const float* rigid_trans; const float* rigid_scale;
    float* cam_verts_out; void* workspace;
    int faces_bstride, B, V, F, S, mask_shared, rigid_abs, persistent_outputs, clip_len;
    float orig_size, znear, zfar;
} HmSilRender;
int hm_sil_fwd_multi(const HmSilRender* renders, int n, int phases, hipStream_t stream);
size_t hm_sil_render_bytes(void);      /* sizeof(HmSilRender) as the library was built: a binding checks its own layout against it */
int hm_sil_reduce_clips(int B, int V, int F, int S, const float* keep_sum, float* loss_out, float* frame_out,
                        void* workspace, int clip_len, int out_stride, hipStream_t stream);
int hm_sil_bwd_clips(const float* verts, const float* K, int B, int V, int F, int S, float orig_size, float eps, int mode,
                     const float* upstream, const float* grad_pooled, const float* keep_sum, const int* adj_off,
                     const int* adj_items, float* grad_verts, float* grad_ndc, void* workspace,
                     int clip_len, float* loss_out, int out_stride, int sum_log2q, hipStream_t stream);
/* The same backward in two calls (phases: bit 0 = masks + line expansion + work list, bit 1 = edge sweeps + vertex gather; 3 =
 * hm_sil_bwd_clips), for a caller whose other streams wait for the END of the line expansion. */
int hm_sil_bwd_phase_clips(const float* verts, const float* K, int B, int V, int F, int S, float orig_size, float eps, int mode,
                     const float* upstream, const float* grad_pooled, const float* keep_sum, const int* adj_off,
                     const int* adj_items, float* grad_verts, float* grad_ndc, void* workspace,
                     int clip_len, float* loss_out, int out_stride, int phases, int sum_log2q, hipStream_t stream);
/*   loss_out (optional, modes 1 / 2): the loss / IoU reduction of hm_sil_reduce_clips (same arithmetic) done by extra
 *   workgroups at the front of the backward's first launch, for a forward that was called with loss_out == NULL: the value
 *   is only logged, so it need not cost a launch on the chain raster -> lines -> sweeps. */
int hm_v2d_fwd_clips(const float* verts, const float* camintr, int hand_nb, const float* ref2d, float image_size, int N,
                     int V, float* unit_grad, float* out2, void* workspace, int clip_len, int out_stride,
                     hipStream_t stream);
int hm_smooth_fwd_clips(const float* verts, int N, int V, int hand_nb, float* unit_grad, float* out1, void* workspace,
                        int clip_len, int out_stride, hipStream_t stream);
/* npca = PCA entries of ONE clip (pca holds nclips * npca) */
int hm_priors_fwd_clips(const float* pca, long npca, const float* s_obj, const float* m_obj, const float* s_hand,
                        const float* m_hand, float* g_pca, float* g_sobj, float* g_shand, float* out3, int nclips,
                        int out_stride, hipStream_t stream);
/* hm_v2d_fwd + hm_smooth_fwd (+ hm_priors_fwd when pca != NULL) of the hand vertices in ONE launch (same outputs) */
int hm_hand_terms_fwd_clips(const float* verts, const float* camintr, int hand_nb, const float* ref2d, float image_size,
                            int N, int V, float* unit_v2d, float* out_v2d2, float* unit_smooth, float* out_smooth1,
                            const float* pca, long npca, const float* s_obj, const float* m_obj, const float* s_hand,
                            const float* m_hand, float* g_pca, float* g_sobj, float* g_shand, float* out_priors3,
                            void* workspace, int clip_len, int out_stride, hipStream_t stream);
int hm_inter_fwd_clips(const float* verts_hand, const float* verts_obj, const float* camintr, int B, int Vh, int Vo,
                       float expansion, float zthresh, float* frame_rec, float* out1, void* workspace, int clip_len,
                       int out_stride, hipStream_t stream);
/* Up to three terms of the frames' (hand, object) vertex pairs in ONE launch (csrc/pairterms.hip); every term is optional
 * (output pointer NULL) and returns what its own entry point returns on the same inputs:
 *   metric_out -> hm_nn_fwd_clips with nn_idx = nn_d2 = NULL (<= 4096 object vertices)          reduce workspace ws_nn
 *   out_inter  -> hm_inter_fwd_clips (frame records `frame_rec`)                                 reduce workspace ws_inter
 *   out_smooth -> hm_smooth_fwd_clips(verts_obj, ..., hand_nb = 1) (unit gradient `unit_smooth`) reduce workspace ws_smooth
 *   ht_out_v2d2 -> hm_hand_terms_fwd_clips(verts_hand, camintr, hand_nb = 1, ht_...) (one hand per frame)  workspace ws_hand
 * The workspaces must be distinct (the terms run side by side).  Replaces, in one go, reference homan/losses.py:199-242
 * (loss + logged distance) and the object half of homan/lossutils.py:18-36. */
int hm_pair_terms_fwd_clips(const float* verts_hand, const float* verts_obj, const float* camintr, int B, int Vh, int Vo,
                            float* metric_out, const int* obj_order, void* ws_nn, float expansion, float zthresh,
                            float* frame_rec, float* out_inter, void* ws_inter, float* unit_smooth, float* out_smooth,
                            void* ws_smooth,
                            const float* ht_ref2d, float ht_image_size, float* ht_unit_v2d, float* ht_out_v2d2,
                            float* ht_unit_smooth, float* ht_out_smooth1, const float* ht_pca, long ht_npca,
                            const float* ht_s_obj, const float* ht_m_obj, const float* ht_s_hand, const float* ht_m_hand,
                            float* ht_g_pca, float* ht_g_sobj, float* ht_g_shand, float* ht_out_priors3, void* ws_hand,
                            const float* obj_spheres, const float* obj_rot6d, const float* obj_trans, const float* obj_scale,
                            const int* hand_order, int* nn_idx, float* nn_d2, int* nn_seed,
                            int clip_len, int out_stride, hipStream_t stream);
/* obj_order (Vo) optional, metric-only calls: a permutation of the object vertices, visited in that order (a spatial sort of
 * the rigid mesh makes 64 consecutive vertices a compact patch: scheduling only, the result is the exact minimum) */
int hm_nn_fwd_clips(const float* verts_hand, const float* verts_obj, int B, int Vh, int Vo, int* nn_idx, float* nn_d2,
                    float* metric_out, void* workspace, int clip_len, int out_stride, const int* obj_order,
                    hipStream_t stream);
/* The metric-only search on a RIGID object: obj_spheres (B, ceil(Vo/64), 4) = centre + radius, in MESH space, of the groups of
 * 64 vertices taken in `obj_order` (built once by the caller); obj_rot6d (B,3,2) / obj_trans (B,3) / obj_scale (one per clip,
 * used as |s|) = the transform that produced verts_obj (hm_rigid_fwd with abs_scale).  A lane per group carries its sphere
 * into camera space instead of every workgroup reducing all the groups' vertices again.  Scheduling data only: the result is
 * the exact minimum (the spheres only decide which groups are scanned).  All four NULL = hm_nn_fwd_clips.
 * nn_seed (optional; also the last data argument of hm_pair_terms_fwd_clips): (2 + ceil(Vh / 128)) * B ints, zero-filled once by
 * the caller and handed to every call of a loop - the search keeps there, per frame, the vertex pair that held the minimum at the
 * previous call; that pair's distance NOW is an upper bound known before any scan, so that most workgroups scan nothing.  Any
 * content is valid (a pair is a pair); the result does not depend on it. */
int hm_nn_fwd_rigid_clips(const float* verts_hand, const float* verts_obj, int B, int Vh, int Vo, int* nn_idx, float* nn_d2,
                          float* metric_out, void* workspace, int clip_len, int out_stride, const int* obj_order,
                          const float* obj_spheres, const float* obj_rot6d, const float* obj_trans, const float* obj_scale,
                          const int* hand_order, int* nn_seed, hipStream_t stream);
int hm_contact_fwd_clips(const float* verts_hand, const float* verts_obj, const int* nn_idx, int B, int Vh, int Vo,
                         float thresh, float* g_hand, float* g_obj, float* out1, void* workspace, int clip_len,
                         int out_stride, hipStream_t stream);
int hm_collision_fwd_clips(const float* verts0, const int* faces0, int V0, int F0, const float* verts1, const int* faces1,
                           int V1, int F1, int B, float scale_factor, float* g0, float* g1, float* out1, void* workspace,
                           int clip_len, int out_stride, hipStream_t stream);
/* vals (nclips, n+1), log (max_steps, nclips, n+1): per clip the weighted total, then its row of the log */
int hm_log_total_clips(float* vals, const float* weights, int n, const int* step, int max_steps, float* log, int nclips,
                       hipStream_t stream);

/* ------------------------------------------------------------------ hand initialisation from keypoints (csrc/handinit.hip)
 * Fits MANO to 21 2-D (and optionally 3-D) keypoints per frame: homan_amd/handinit.py.  Not in the reference tree, whose hand
 * start comes from a pose network (homan/mocap.py:34-113): the rules below ARE the definition, pinned bit
 * for bit by the fp32 NumPy restatement of tests/handinit_ref.py.  Every operation is fp32 IEEE without contraction, written
 * below with its parentheses; a sum "from 0" starts at 0.0f and adds its addends one at a time in the stated order.
 *
 * A row is one frame of one candidate; clip c = rows [c * clip_len, (c + 1) * clip_len) is one candidate track, N = C * clip_len.
 * verts_world (N,778,3): the camera-space vertices hm_mano_fwd_clips writes.  W (21,778): the keypoint regressor of the hand's
 * side.  camintr (N,3,3) in pixels (fx, cx, fy, cy = entries 0, 2, 4, 5).  kp2d (N,21,2) pixels, c2 (N,21) >= 0, s (N) > 0 the
 * frame's box scale in pixels.  kp3d (N,21,3) metres relative to keypoint 0 and c3 (N,21): both or neither.
 *
 * Two sums are used throughout.  TREE64(a_0 .. a_63): a_l += a_(l ^ o) for o = 32, 16, 8, 4, 2, 1.  BLOCKSUM(x_0 .. x_(n-1)): thread
 * t of 256 adds x_t, x_(t+256), ... from 0; TREE64 over each of the four groups of 64 consecutive threads gives w0 .. w3; the
 * result is ((w0 + w1) + w2) + w3.
 *   X[n,k,c]  = TREE64 over l of (the sum from 0 over v = l, l + 64, ... < 778 of W[k,v] * verts_world[n,v,c])   -> keypoints (N,21,3)
 *   S2[clip]  = BLOCKSUM of the clip's clip_len * 21 values c2 in memory order, S3 the same of c3 (0 without kp3d)
 *   2-D term of (n,k), with (x, y, z) = X[n,k], only if c2 > 0 (otherwise cost 0, gradient 0, kp2d[n,k] is not read: it may be NaN):
 *     z > znear:  px = (fx * x) / z + cx, py = (fy * y) / z + cy, rx = (px - kp2d.x) / s[n], ry likewise, u = rx * rx + ry * ry,
 *                 den = sigma * sigma + u, cost = c2 * ((sigma * sigma * u) / den)          (Geman-McClure)
 *                 g = (c2 * (q * q)) * (lw_kp2d / S2) with q = sigma * sigma / den; gpx = g * ((2 * rx) / s[n]), gpy likewise;
 *                 dX = (gpx * (fx / z), gpy * (fy / z), -((gpx * (fx * x) + gpy * (fy * y)) / (z * z)))
 *     z <= znear: cost = c2 * (sigma * sigma), gradient 0 (a candidate cannot win by hiding keypoints behind the camera)
 *   3-D term of (n,k), only if c3 > 0: d = (X[n,k] - X[n,0]) - kp3d[n,k], cost = c3 * ((d.x * d.x + d.y * d.y) + d.z * d.z),
 *     h = ((2 * c3) * (lw_kp3d / S3)) * d; G[n,k] = dX + h, and G[n,0] then loses the sum from 0 over k = 0 .. 20 of h[n,k].
 *   lw / S is 0 where S == 0.
 *   unit_grad[n,v,c] = the sum from 0 over k = 0 .. 20 of W[k,v] * G[n,k,c] = d (lw_kp2d L2d + lw_kp3d L3d) / d verts_world: ONE
 *     entry of the g_terms of hm_mano_bwd_rigid_clips, weight 1.
 *   row_parts (N,2) = {TREE64 of the row's 21 costs (lanes 21 .. 63 hold 0), 2-D; the same, 3-D}
 *   out2[c * out_stride + 0] = L2d = BLOCKSUM(the clip's row_parts[.,0], rows ascending) / S2, 0 where S2 == 0; [+ 1] = L3d alike.
 * One launch, one workgroup per row; the clip's last workgroup (a ticket) forms L2d / L3d.  No floating-point atomics: the bits
 * do not depend on the run, nor on where a clip stands in the batch or how many clips there are.
 * row_parts: caller-owned (N,2) output.  clip_tickets: C ints, zero-filled ONCE by the caller (they reset themselves).
 * HM_ERR_BAD_ARG, nothing launched, outputs untouched: a NULL pointer other than the pair kp3d / c3 (or only one of that pair),
 * N <= 0, clip_len <= 0, N not a multiple of clip_len, sigma <= 0 (or NaN). */
int hm_keypoint_terms_clips(const float* verts_world, const float* W, const float* camintr, const float* kp2d, const float* c2,
                            const float* s, const float* kp3d, const float* c3, float sigma, float znear, float lw_kp2d,
                            float lw_kp3d, int N, int clip_len, float* keypoints, float* unit_grad, float* row_parts,
                            int* clip_tickets, float* out2, int out_stride, hipStream_t stream);
/* The tail of a step of the keypoint fit, one workgroup per clip.  vals (C, vals_stride >= 8): row c holds {L2d, L3d, Lpca, -, -,
 * Lsmooth, Lbeta, total}: slots 0 / 1 from hm_keypoint_terms_clips, 2 .. 4 from hm_priors_fwd_clips, 5 from hm_smooth_fwd_clips
 * (all called with out_stride = vals_stride).  betas (N,10): Lbeta = BLOCKSUM(the clip's betas squared, memory order) * inv with
 * inv = 1 / (10 clip_len); g_betas (N,10; optional) += lw_beta * ((2 * beta) * inv), after the MANO backward has written it;
 * total = (((lw_kp2d * L2d + lw_kp3d * L3d) + lw_pca * Lpca) + lw_beta * Lbeta) + lw_smooth * Lsmooth.  log (max_steps, C, 8)
 * optional: row min(step[0], max_steps - 1) receives the clips' eight values (step: the device counter of hm_adam_step, read
 * BEFORE that step's launch).  HM_ERR_BAD_ARG as above, and for vals_stride < 8 or a log without step / max_steps > 0. */
int hm_handinit_finish_clips(const float* betas, float* g_betas, int N, int clip_len, float* vals, int vals_stride,
                             float lw_kp2d, float lw_kp3d, float lw_pca, float lw_beta, float lw_smooth, const int* step,
                             int max_steps, float* log, hipStream_t stream);

/* ------------------------------------------------------------------ measurement / debug hooks (synchronous)
 * hm_bench_sil_kernels: one full silhouette forward + backward to populate the workspace, then `reps` launches of the
 * raster kernel, of the edge-sweep kernel and of the line-source kernel, each series bracketed by two HIP events on
 * `stream`; avg_ms[0..2] (HOST pointer) receive the average launch durations in milliseconds. */
int hm_bench_sil_kernels(const float* verts, const int* faces, const float* K, int B, int V, int F, int S,
                         const float* keep, const float* ref, const float* keep_sum, float* pooled, float* loss_out,
                         const int* work_order, const int* adj_off, const int* adj_items,
                         const float* upstream, float* grad_verts, void* workspace, int reps, float* avg_ms,
                         hipStream_t stream);
/* In-graph timing of k_raster_fwd / k_bwd_lines / k_bwd_sweep: every workgroup (every wave of the persistent sweep kernel)
 * stores the device wall clock (s_memrealtime) at entry and exit into a slot pair of its own inside the silhouette workspace
 * - for launches replayed from a captured hipGraph, where ROCm allows no events.  B, V, F, S as given to
 * hm_sil_workspace_bytes.  hm_sil_timestamps(..., 1, stream) switches on and arms (async memsets; call before every replay),
 * (..., 0, stream) switches off; hm_sil_timestamps_save copies the raw stamps (hm_sil_timestamps_bytes) to `dst` on the
 * device without synchronising; hm_sil_timestamps_read waits for `stream` and returns earliest-start-to-latest-end of the
 * three kernels in microseconds (HOST float[3]) from `saved` or, saved == NULL, from the workspace. */
size_t hm_sil_timestamps_bytes(int B, int V, int F, int S);
int hm_sil_timestamps(void* workspace, int B, int V, int F, int S, int enable, hipStream_t stream);
int hm_sil_timestamps_save(const void* workspace, int B, int V, int F, int S, void* dst, hipStream_t stream);
int hm_sil_timestamps_read(const void* workspace, int B, int V, int F, int S, const void* saved, float* us3, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HOMAN_AMD_H */
