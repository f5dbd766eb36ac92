/*
 * kaolin_amd.h -- C ABI of libkaolin_amd.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for Kaolin's DIB-R / 3D-metrics hot path.  Every
 * entry point replaces one function of the reference's pybind11 module
 * `kaolin._C` (kaolin/csrc/bindings.cpp:103-115); the reference binding each one
 * stands in for is cited next to it.  No torch / ATen type crosses this ABI:
 *
 *   - all pointers are DEVICE pointers into memory the caller owns (the Python
 *     shim allocates every output and workspace with torch, so the caching
 *     allocator and stream semantics of the reference are unchanged);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); kernels
 *     are only enqueued, no entry point synchronises the host;
 *   - every function returns a hipError_t as int (0 = hipSuccess) and never
 *     throws; argument-shape checking (the ATen `checkSize` strings the
 *     reference's tests match) is done by the host shim above this ABI;
 *   - functions are re-entrant and may be called concurrently from the forward
 *     thread and autograd's backward thread;
 *   - "accumulate" outputs must be zero-initialised by the caller exactly where
 *     the reference requires it (at::zeros / zeros_like in the .cpp wrappers).
 *
 * dtype suffixes: _f32 float, _f64 double, _f16 IEEE half (passed as uint16_t*).
 * Index tensors are int64_t as in the reference (at::kLong).
 */
#ifndef KAOLIN_AMD_H_
#define KAOLIN_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library identification. Returns a static string "kaolin_amd <ver> gfx950". */
const char* kamd_version(void);

/* ------------------------------------------------------------------------- */
/* metrics.sided_distance_forward_cuda(p1, p2) -> [dist, idx]                 */
/* reference: kaolin/csrc/metrics/sided_distance.cpp:65-89,                   */
/*            kaolin/csrc/metrics/sided_distance_cuda.cu:52-201,244-267       */
/* p1 (B,N,3), p2 (B,M,3) contiguous; dist (B,N); idx (B,N) int64.            */
/* dist[b,i] = min_j |p1[b,i]-p2[b,j]|^2, idx = lowest j attaining it.        */
/* `workspace` must hold kamd_sided_distance_forward_workspace(B,N,M,esize)   */
/* bytes (may be NULL when that size is 0).                                   */
/* ------------------------------------------------------------------------- */
size_t kamd_sided_distance_forward_workspace(int B, int N, int M, int elem_size);
int kamd_sided_distance_forward_f32(void* stream, int B, int N, int M,
                                    const float* p1, const float* p2,
                                    float* dist, int64_t* idx, void* workspace);
int kamd_sided_distance_forward_f64(void* stream, int B, int N, int M,
                                    const double* p1, const double* p2,
                                    double* dist, int64_t* idx, void* workspace);
int kamd_sided_distance_forward_f16(void* stream, int B, int N, int M,
                                    const uint16_t* p1, const uint16_t* p2,
                                    uint16_t* dist, int64_t* idx, void* workspace);
/* integer clouds (the reference dispatches Byte / Short / Int / Long as well, */
/* kaolin/csrc/utils.h:50-64): arithmetic in the element type, C promotions,   */
/* truncation at every assignment as in sided_distance_cuda.cu:83-86           */
int kamd_sided_distance_forward_u8(void* stream, int B, int N, int M, const uint8_t* p1, const uint8_t* p2,
                                   uint8_t* dist, int64_t* idx, void* workspace);
int kamd_sided_distance_forward_i16(void* stream, int B, int N, int M, const int16_t* p1, const int16_t* p2,
                                    int16_t* dist, int64_t* idx, void* workspace);
int kamd_sided_distance_forward_i32(void* stream, int B, int N, int M, const int32_t* p1, const int32_t* p2,
                                    int32_t* dist, int64_t* idx, void* workspace);
int kamd_sided_distance_forward_i64(void* stream, int B, int N, int M, const int64_t* p1, const int64_t* p2,
                                    int64_t* dist, int64_t* idx, void* workspace);

/* Both directions of chamfer_distance in one pass (kaolin/metrics/pointcloud.py */
/* :89-136 calls sided_distance(p1, p2) and sided_distance(p2, p1)): both clouds */
/* are binned once, each on its own grid, and serve as targets of one direction  */
/* and as queries of the other.  dist1/idx1 (B,N) are p1 -> p2, dist2/idx2 (B,M) */
/* are p2 -> p1, bit-identical to two kamd_sided_distance_forward calls.         */
/* The workspace query returns 0 when the shapes do not qualify (a cloud below   */
/* 8192 points, non-fp32): callers then issue the two calls.                     */
size_t kamd_sided_distance_pair_forward_workspace(int B, int N, int M, int elem_size);
int kamd_sided_distance_pair_forward_f32(void* stream, int B, int N, int M,
                                         const float* p1, const float* p2,
                                         float* dist1, int64_t* idx1,
                                         float* dist2, int64_t* idx2, void* workspace);
int kamd_sided_distance_pair_forward_f64(void* stream, int B, int N, int M,
                                         const double* p1, const double* p2,
                                         double* dist1, int64_t* idx1,
                                         double* dist2, int64_t* idx2, void* workspace);

/* Gradient of chamfer_distance (kaolin/metrics/pointcloud.py:120-136) w.r.t.   */
/* both clouds in one launch: grad (B) is the gradient of the (B) result; the    */
/* autograd chain weight -> mean -> [sqrt] -> sided_distance backward            */
/* (sided_distance_cuda.cu:203-242) of both directions is evaluated per point.  */
/* g1 (B,N,3) and g2 (B,M,3) are overwritten (no initialisation needed).         */
int kamd_chamfer_distance_backward_f32(void* stream, int B, int N, int M,
                                       const float* grad, float w1, float w2, int squared,
                                       const float* p1, const float* p2,
                                       const int64_t* idx1, const int64_t* idx2,
                                       const float* dist1, const float* dist2,
                                       float* g1, float* g2);

/* chamfer_distance as ONE operator (kaolin/metrics/pointcloud.py:89-136, fp32):  */
/* out (B) = w1 * mean_i f(dist1_i) + w2 * mean_j f(dist2_j), f = identity        */
/* (squared != 0) or sqrt, from workspace fill + build + search = 3 launches; the */
/* means are accumulated in double inside the search launch.  dist1/idx1/dist2/  */
/* idx2 are optional outputs (NULL = not wanted).  with_grad != 0: the search     */
/* also leaves d out / d p (per unit of upstream gradient) in the workspace,      */
/* which the caller then keeps alive until kamd_chamfer_distance_backward_fused   */
/* (one launch: g1 (B,N,3), g2 (B,M,3) = grad[b] * those, overwritten).           */
/* ..._workspace returns 0 when the shapes do not qualify (see pair_forward).     */
size_t kamd_chamfer_distance_forward_workspace(int B, int N, int M, int with_grad);
int kamd_chamfer_distance_forward_f32(void* stream, int B, int N, int M,
                                      const float* p1, const float* p2, float w1, float w2,
                                      int squared, int with_grad, float* out,
                                      float* dist1, int64_t* idx1, float* dist2, int64_t* idx2,
                                      void* workspace);
int kamd_chamfer_distance_backward_fused_f32(void* stream, int B, int N, int M, const float* grad,
                                             void* workspace, float* g1, float* g2);

/* metrics.sided_distance_backward_cuda(grad, p1, p2, idx) -> [g1, g2]        */
/* reference: sided_distance.cpp:91-122, sided_distance_cuda.cu:203-242       */
/* g1 (B,N,3) is overwritten; g2 (B,M,3) is accumulated (caller zeroes it).   */
int kamd_sided_distance_backward_f32(void* stream, int B, int N, int M,
                                     const float* grad, const float* p1, const float* p2,
                                     const int64_t* idx, float* g1, float* g2);
int kamd_sided_distance_backward_f64(void* stream, int B, int N, int M,
                                     const double* grad, const double* p1, const double* p2,
                                     const int64_t* idx, double* g1, double* g2);
int kamd_sided_distance_backward_f16(void* stream, int B, int N, int M,
                                     const uint16_t* grad, const uint16_t* p1, const uint16_t* p2,
                                     const int64_t* idx, uint16_t* g1, uint16_t* g2);
int kamd_sided_distance_backward_u8(void* stream, int B, int N, int M, const uint8_t* grad, const uint8_t* p1,
                                    const uint8_t* p2, const int64_t* idx, uint8_t* g1, uint8_t* g2);
int kamd_sided_distance_backward_i16(void* stream, int B, int N, int M, const int16_t* grad, const int16_t* p1,
                                     const int16_t* p2, const int64_t* idx, int16_t* g1, int16_t* g2);
int kamd_sided_distance_backward_i32(void* stream, int B, int N, int M, const int32_t* grad, const int32_t* p1,
                                     const int32_t* p2, const int64_t* idx, int32_t* g1, int32_t* g2);
int kamd_sided_distance_backward_i64(void* stream, int B, int N, int M, const int64_t* grad, const int64_t* p1,
                                     const int64_t* p2, const int64_t* idx, int64_t* g1, int64_t* g2);

/* ------------------------------------------------------------------------- */
/* render.mesh.packed_rasterize_forward_cuda(H, W, z, img, bbox, feat,        */
/*     first_idx_face_per_mesh, multiplier, eps) -> [feat, sel_idx, weights]  */
/* reference: kaolin/csrc/render/mesh/rasterization.cpp:49-104,               */
/*            rasterization_cuda.cu:43-236                                    */
/* Packed inputs over F' = first_idx[B] faces: z (F',3), img (F',3,2) already */
/* multiplied by `multiplier`, bbox (F',4) = [xmin,ymin,xmax,ymax],           */
/* feat (F',3,D); first_idx (B+1) int64 ON DEVICE.                            */
/* Outputs (fully written, no pre-fill needed): interp (B,H,W,D),             */
/* sel_idx (B,H,W) int64 relative to the mesh's first packed face (-1 none),  */
/* weights (B,H,W,3).  `workspace`: kamd_rasterize_forward_workspace bytes.   */
/* ------------------------------------------------------------------------- */
size_t kamd_rasterize_forward_workspace(int B, int H, int W, int64_t total_faces, int elem_size);
int kamd_packed_rasterize_forward_f32(void* stream, int B, int H, int W, int D,
                                      int64_t total_faces,
                                      const float* z, const float* img, const float* bbox,
                                      const float* feat, const int64_t* first_idx,
                                      float multiplier, float eps,
                                      float* interp, int64_t* sel_idx, float* weights,
                                      void* workspace);
int kamd_packed_rasterize_forward_f64(void* stream, int B, int H, int W, int D,
                                      int64_t total_faces,
                                      const double* z, const double* img, const double* bbox,
                                      const double* feat, const int64_t* first_idx,
                                      float multiplier, float eps,
                                      double* interp, int64_t* sel_idx, double* weights,
                                      void* workspace);

/* render.mesh.rasterize_backward_cuda(grad, interp, sel_idx, weights, img,   */
/*     feat, eps) -> [g_img, g_feat]                                          */
/* reference: rasterization.cpp:106-168, rasterization_cuda.cu:238-442        */
/* img (B,F,3,2) UNSCALED, feat (B,F,3,D), face_idx (B,H,W) mesh-relative.    */
/* g_img (B,F,3,2), g_feat (B,F,3,D) are accumulated (caller zeroes them).    */
/* Works for any B*H*W >= 1 (the reference launches 0 blocks below 512 px).   */
/* g_feat may be NULL when the caller does not need the feature gradient      */
/* (autograd's needs_input_grad): it is then not computed.                     */
int kamd_rasterize_backward_f32(void* stream, int B, int H, int W, int F, int D,
                                const float* grad, const int64_t* face_idx,
                                const float* weights, const float* img, const float* feat,
                                float eps, float* g_img, float* g_feat);
int kamd_rasterize_backward_f64(void* stream, int B, int H, int W, int F, int D,
                                const double* grad, const int64_t* face_idx,
                                const double* weights, const double* img, const double* feat,
                                float eps, double* g_img, double* g_feat);

/* ------------------------------------------------------------------------- */
/* render.mesh.dibr_soft_mask_forward_cuda(img*mult, large_bbox, sel_idx,     */
/*     sigmainv, knum, multiplier) -> [soft_mask, prob, idx, type]            */
/* reference: kaolin/csrc/render/mesh/dibr_soft_mask.cpp:48-108,              */
/*            dibr_soft_mask_cuda.cu:27-228                                   */
/* img (B,F,3,2) scaled, large_bbox (B,F,4), sel_idx (B,H,W) int64.           */
/* Outputs fully written: soft_mask (B,H,W), prob (B,H,W,K) (0 fill),         */
/* idx (B,H,W,K) int64 (-1 fill), type (B,H,W,K) uint8 (0 fill).              */
/* hit_count (B,H,W) uint8 is OPTIONAL (NULL = not produced; not part of the  */
/* reference's interface): number of K-buffer entries written per pixel,      */
/* saturated at 255; the backward uses it to skip pixels without hits.        */
/* work: kamd_dibr_soft_mask_work_words(B,H,W) 32-bit words receiving the      */
/* search's worklist (scratch for this operator).                             */
/* ------------------------------------------------------------------------- */
size_t kamd_dibr_soft_mask_forward_workspace(int B, int H, int W, int F, int K, int elem_size);
int kamd_dibr_soft_mask_forward_f32(void* stream, int B, int H, int W, int F, int K,
                                    const float* img, const float* large_bbox,
                                    const int64_t* sel_idx, float sigmainv, float multiplier,
                                    float* soft_mask, float* prob, int64_t* idx, uint8_t* type,
                                    void* workspace, uint8_t* hit_count, uint32_t* work);
int kamd_dibr_soft_mask_forward_f64(void* stream, int B, int H, int W, int F, int K,
                                    const double* img, const double* large_bbox,
                                    const int64_t* sel_idx, float sigmainv, float multiplier,
                                    double* soft_mask, double* prob, int64_t* idx, uint8_t* type,
                                    void* workspace, uint8_t* hit_count, uint32_t* work);

/* render.mesh.dibr_soft_mask_backward_cuda(grad, soft_mask, sel_idx, prob,   */
/*     idx, type, img*mult, sigmainv, multiplier) -> g_img                    */
/* reference: dibr_soft_mask.cpp:110-183, dibr_soft_mask_cuda.cu:230-402      */
/* g_img (B,F,3,2) is accumulated (caller zeroes it).                         */
int kamd_dibr_soft_mask_backward_f32(void* stream, int B, int H, int W, int F, int K,
                                     const float* grad, const float* soft_mask,
                                     const int64_t* sel_idx, const float* prob,
                                     const int64_t* idx, const uint8_t* type, const float* img,
                                     float sigmainv, float multiplier, float* g_img,
                                     const uint8_t* hit_count);
int kamd_dibr_soft_mask_backward_f64(void* stream, int B, int H, int W, int F, int K,
                                     const double* grad, const double* soft_mask,
                                     const int64_t* sel_idx, const double* prob,
                                     const int64_t* idx, const uint8_t* type, const double* img,
                                     float sigmainv, float multiplier, double* g_img,
                                     const uint8_t* hit_count);

/* Compact-list variant used by this package's own autograd Function (not part  */
/* of the reference's interface): same search, same soft_mask, but instead of   */
/* the (B,H,W,K) K-buffers the accepted (pixel, face) hits are kept as lists:   */
/*  hit_pair  (two int32 per record: the mesh-relative face, and (pixel of the  */
/*            sub-tile 0..63) << 16 | rank of the hit among the pixel's hits):  */
/*            what the search leaves for the evaluation, SEGMENTED: a work item */
/*            (a 16x4-pixel sub-tile that has hits to search), item = (32x32    */
/*            tile * B + b) * 16 + sub-tile, owns the records [item*64*K,        */
/*            item*64*K + item_count[item]), FACE-MAJOR (the pixels of one face  */
/*            are consecutive);                                                   */
/*  hit_rec / hit_prob  the evaluated hits as a flat list in 64 shards of equal    */
/*            capacity (capacity / 64 records each; shard s holds work[256 + 32 s]   */
/*            records; an item appends one contiguous range to shard item % 64):    */
/*            hit_rec = two int32 {(b*F + face) | which-of-six << 29, row << 16 |   */
/*            col}, hit_prob the probability -- all the backward pass reads (it     */
/*            streams the shards in rounds of 256 records, no items).               */
/*            Requires B*F < 2^29, H, W < 2^16.                                     */
/* item_count holds ceil(W/32)*ceil(H/32)*16*B ints.  `work`                      */
/* (kamd_dibr_soft_mask_work_words 32-bit words) receives the worklist: 8 sharded */
/* item counters (words 32 s), the flat list's 64 shard counts and the covered-tile */
/* list's 32, one per 128-byte line (same-line device atomics serialise), in a    */
/* 3328-word header, then the items {item, uncovered-pixel mask (2 words), pairs  */
/* the search accepted}.  The fused dibr_rasterization forward appends one byte   */
/* per (mesh, 16x16-pixel tile): does the tile hold a covered pixel; a copy of    */
/* the covered tile rows per view (2 words each); and the list of the tiles that  */
/* hold a covered pixel (32 shards of ceil(B/8)*ceil(tiles/4) words), which the   */
/* rasterizer's backward walks.  Word 1 of the header receives a signature of the  */
/* layout (a hash of B, H, W) from the forward's last launch: the fused backward  */
/* walks the covered-tile list only when it finds it there and visits every tile  */
/* otherwise.  Requires B*H*W < 2^31.                                              */
/* Records each of the three hit arrays must hold (64*K per sub-tile slot).       */
size_t kamd_dibr_soft_mask_lean_capacity(int B, int H, int W, int K);
size_t kamd_dibr_soft_mask_work_words(int B, int H, int W);
int kamd_dibr_soft_mask_forward_lean_f32(void* stream, int B, int H, int W, int F, int K,
                                         const float* img, const float* large_bbox,
                                         const int64_t* sel_idx, float sigmainv, float multiplier,
                                         float* soft_mask, int32_t* hit_pair,
                                         float* hit_prob, int32_t* hit_rec, int32_t* item_count,
                                         uint32_t* work, void* workspace);
int kamd_dibr_soft_mask_forward_lean_f64(void* stream, int B, int H, int W, int F, int K,
                                         const double* img, const double* large_bbox,
                                         const int64_t* sel_idx, float sigmainv, float multiplier,
                                         double* soft_mask, int32_t* hit_pair,
                                         double* hit_prob, int32_t* hit_rec, int32_t* item_count,
                                         uint32_t* work, void* workspace);
int kamd_dibr_soft_mask_backward_lean_f32(void* stream, int B, int H, int W, int F, int K,
                                          const float* grad, const float* soft_mask,
                                          const int32_t* hit_pair,
                                          const float* hit_prob, const int32_t* hit_rec,
                                          const int32_t* item_count, const uint32_t* work,
                                          const float* img,
                                          double img_scale, float sigmainv, float multiplier,
                                          float* g_img);
int kamd_dibr_soft_mask_backward_lean_f64(void* stream, int B, int H, int W, int F, int K,
                                          const double* grad, const double* soft_mask,
                                          const int32_t* hit_pair,
                                          const double* hit_prob, const int32_t* hit_rec,
                                          const int32_t* item_count, const uint32_t* work,
                                          const double* img,
                                          double img_scale, float sigmainv, float multiplier,
                                          double* g_img);
/* Fused front doors (ours): take the RAW operator inputs of the Python layer and */
/* fold its torch glue into the bin kernel -- rasterization.py:292-327 (packing   */
/* of valid faces with torch.where = a host sync, x multiplier, per-face min/max) */
/* and dibr.py:31-39 (x multiplier, boxes enlarged by margin = boxlen*multiplier).*/
/* valid: (B,F) bytes, NULL = all faces.  face_idx comes out mesh-relative.       */
/* In the lean backward, img_scale multiplies img on the fly (pass the multiplier */
/* with the unscaled vertices, or 1 with already scaled ones).                    */
int kamd_rasterize_forward_fused_f32(void* stream, int B, int H, int W, int F, int D,
                                     const float* z, const float* img, const float* feat,
                                     const uint8_t* valid, double multiplier, float eps,
                                     float* interp, int64_t* face_idx, float* weights,
                                     void* workspace);
int kamd_rasterize_forward_fused_f64(void* stream, int B, int H, int W, int F, int D,
                                     const double* z, const double* img, const double* feat,
                                     const uint8_t* valid, double multiplier, float eps,
                                     double* interp, int64_t* face_idx, double* weights,
                                     void* workspace);
/* _strided: z (B,F,3) and the optional per-face scalar `front` (B,F) are read in place through ELEMENT strides    */
/* (z[f * z_face_stride + k * z_vertex_stride], front[f * front_stride]; batch items must be F faces apart), e.g. */
/* the [..., 2] views of the camera-space vertices / face normals; a face is kept when valid[f] != 0 (if given)   */
/* and front[f] >= 0 (if given) -- the mask `face_normals_z >= 0` of dibr_rasterization (dibr.py:188).           */
int kamd_rasterize_forward_fused_strided_f32(void* stream, int B, int H, int W, int F, int D, const float* z,
                                             int64_t z_face_stride, int64_t z_vertex_stride,
                                             const float* img, const float* feat, const uint8_t* valid,
                                             const float* front, int64_t front_stride, double multiplier,
                                             float eps, float* interp, int64_t* face_idx, float* weights,
                                             void* workspace);
int kamd_rasterize_forward_fused_strided_f64(void* stream, int B, int H, int W, int F, int D, const double* z,
                                             int64_t z_face_stride, int64_t z_vertex_stride,
                                             const double* img, const double* feat, const uint8_t* valid,
                                             const double* front, int64_t front_stride, double multiplier,
                                             float eps, double* interp, int64_t* face_idx, double* weights,
                                             void* workspace);
int kamd_dibr_soft_mask_forward_fused_f32(void* stream, int B, int H, int W, int F, int K,
                                          const float* img, double multiplier, double margin,
                                          const int64_t* sel_idx, float sigmainv,
                                          float* soft_mask, int32_t* hit_pair,
                                          float* hit_prob, int32_t* hit_rec, int32_t* item_count,
                                          uint32_t* work, void* workspace);
int kamd_dibr_soft_mask_forward_fused_f64(void* stream, int B, int H, int W, int F, int K,
                                          const double* img, double multiplier, double margin,
                                          const int64_t* sel_idx, float sigmainv,
                                          double* soft_mask, int32_t* hit_pair,
                                          double* hit_prob, int32_t* hit_rec, int32_t* item_count,
                                          uint32_t* work, void* workspace);

/* ------------------------------------------------------------------------- */
/* kaolin.metrics.render.mask_iou(lhs, rhs) (kaolin/metrics/render.py:18-40),  */
/* fused: forward = one pass over both (B, H, W) masks, P = H * W (+ a one-     */
/* workgroup finish): sums (B, 2) doubles receive {sum(l*r), sum(l+r-l*r)} per  */
/* item, loss the scalar 1 - mean(I / (U + 1e-10)); backward = one elementwise  */
/* pass giving d loss / d(one mask) from the OTHER mask and the sums.           */
/* workspace: kamd_mask_iou_workspace(B) bytes.                                 */
/* ------------------------------------------------------------------------- */
size_t kamd_mask_iou_workspace(int B);
int kamd_mask_iou_forward_f32(void* stream, int B, int64_t P, const float* lhs, const float* rhs, void* workspace,
                              double* sums, float* loss);
int kamd_mask_iou_forward_f64(void* stream, int B, int64_t P, const double* lhs, const double* rhs, void* workspace,
                              double* sums, double* loss);
int kamd_mask_iou_backward_f32(void* stream, int B, int64_t P, const float* grad_loss, const float* other,
                               const double* sums, float* grad);
int kamd_mask_iou_backward_f64(void* stream, int B, int64_t P, const double* grad_loss, const double* other,
                               const double* sums, double* grad);
/* The linear loss sum(x1 * w1) + sum(x2 * w2) over two G-buffers of one render  */
/* (image features and soft mask against fixed weights; no reference operator -- */
/* in torch: two dots, an add, two full-size products backward).  Forward: one   */
/* pass over the four arrays + a one-workgroup finish, out = the scalar; n2 = 0  */
/* for a single pair.  Backward: g1 = grad_out[0] * w1, g2 = grad_out[0] * w2 in */
/* one pass (a NULL gradient is skipped).  workspace: kamd_weighted_sum2_workspace() bytes. */
size_t kamd_weighted_sum2_workspace(void);
int kamd_weighted_sum2_forward_f32(void* stream, int64_t n1, const float* x1, const float* w1, int64_t n2,
                                   const float* x2, const float* w2, void* workspace, float* out);
int kamd_weighted_sum2_forward_f64(void* stream, int64_t n1, const double* x1, const double* w1, int64_t n2,
                                   const double* x2, const double* w2, void* workspace, double* out);
int kamd_weighted_sum2_backward_f32(void* stream, const float* grad_out, int64_t n1, const float* w1, float* g1,
                                    int64_t n2, const float* w2, float* g2);
int kamd_weighted_sum2_backward_f64(void* stream, const double* grad_out, int64_t n1, const double* w1, double* g1,
                                    int64_t n2, const double* w2, double* g2);
/* kaolin.render.mesh.texture_mapping (kaolin/render/mesh/utils.py:23-76), one  */
/* gather kernel each way: uv (B, N, 2) OpenGL-style in [0, 1] (clamped), tex   */
/* (B, C, TH, TW), out (B, N, C); grid_sample arithmetic (align_corners=False,  */
/* border padding), bilinear != 0 or nearest.  Backward accumulates into the    */
/* caller-zeroed g_tex (NULL: not needed) and writes g_uv (B, N, 2) (NULL: not  */
/* needed; zero for nearest).                                                   */
int kamd_texture_mapping_forward_f32(void* stream, int B, int64_t N, int C, int TH, int TW, int bilinear,
                                     const float* uv, const float* tex, float* out);
int kamd_texture_mapping_forward_f64(void* stream, int B, int64_t N, int C, int TH, int TW, int bilinear,
                                     const double* uv, const double* tex, double* out);
int kamd_texture_mapping_backward_f32(void* stream, int B, int64_t N, int C, int TH, int TW, int bilinear,
                                      const float* uv, const float* tex, const float* grad_out, float* g_tex,
                                      float* g_uv);
int kamd_texture_mapping_backward_f64(void* stream, int B, int64_t N, int C, int TH, int TW, int bilinear,
                                      const double* uv, const double* tex, const double* grad_out, double* g_tex,
                                      double* g_uv);

/* ------------------------------------------------------------------------- */
/* kaolin.render.lighting: the reduced spherical-gaussian inner product       */
/* (_C.render.sg.unbatched_reduced_sg_inner_product_{forward,backward}_cuda): */
/* out (num_sg, 3) = sum over the num_other lobes of the SG inner product.    */
/* Rows: amplitude (num_sg, 3), direction (num_sg, 3), sharpness (num_sg);    */
/* amplitude = sharpness = NULL selects the constant lobe (lobe_amplitude,    */
/* direction, lobe_sharpness) -- cosine_lobe_sg -- and then grad_amplitude /  */
/* grad_sharpness are not written (pass NULL).  Every output is fully         */
/* written; num_sg == 0 or num_other == 0 returns without a launch (the       */
/* caller's outputs are then zeros).  Deterministic: no atomics.  backward's  */
/* workspace: kamd_sg_reduced_inner_product_backward_workspace(num_sg,        */
/* num_other, elem_size) bytes (host-only).                                   */
/* ------------------------------------------------------------------------- */
size_t kamd_sg_reduced_inner_product_backward_workspace(int64_t num_sg, int num_other, int elem_size);
int kamd_sg_reduced_inner_product_forward_f32(void* stream, int64_t num_sg, int num_other, const float* amplitude,
                                              const float* direction, const float* sharpness, double lobe_amplitude,
                                              double lobe_sharpness, const float* other_amplitude,
                                              const float* other_direction, const float* other_sharpness, float* out);
int kamd_sg_reduced_inner_product_forward_f64(void* stream, int64_t num_sg, int num_other, const double* amplitude,
                                              const double* direction, const double* sharpness, double lobe_amplitude,
                                              double lobe_sharpness, const double* other_amplitude,
                                              const double* other_direction, const double* other_sharpness, double* out);
int kamd_sg_reduced_inner_product_backward_f32(void* stream, int64_t num_sg, int num_other, const float* grad_out,
                                               const float* amplitude, const float* direction, const float* sharpness,
                                               double lobe_amplitude, double lobe_sharpness, const float* other_amplitude,
                                               const float* other_direction, const float* other_sharpness, void* workspace,
                                               float* grad_amplitude, float* grad_direction, float* grad_sharpness,
                                               float* grad_other_amplitude, float* grad_other_direction,
                                               float* grad_other_sharpness);
int kamd_sg_reduced_inner_product_backward_f64(void* stream, int64_t num_sg, int num_other, const double* grad_out,
                                               const double* amplitude, const double* direction, const double* sharpness,
                                               double lobe_amplitude, double lobe_sharpness,
                                               const double* other_amplitude, const double* other_direction,
                                               const double* other_sharpness, void* workspace, double* grad_amplitude,
                                               double* grad_direction, double* grad_sharpness,
                                               double* grad_other_amplitude, double* grad_other_direction,
                                               double* grad_other_sharpness);

/* ------------------------------------------------------------------------- */
/* dibr_rasterization in one call (ours; kaolin/render/mesh/dibr.py:119-209   */
/* = rasterize with valid faces + dibr_soft_mask over all faces).  Same       */
/* kernels as the separate entry points, sharing one binning pass: the faces  */
/* are binned for both operators in one launch per phase, and the rasterizer's */
/* tile kernel classifies the pixels for the soft mask.  The two backward      */
/* kernels do not depend on each other; they are enqueued one after the other  */
/* on `stream` (with KAMD_BWD_SIDE_STREAM=1 the soft mask's goes to an         */
/* internal side stream forked from / joined to `stream` with events: still    */
/* stream-ordered for the caller).  g_img (zeroed by the caller)               */
/* receives BOTH gradient contributions; g_feat may be NULL (feature gradient  */
/* not needed: not computed).  workspace: kamd_dibr_rasterization_workspace.   */
/* `weights` is meaningful only where face_idx >= 0 (background tiles do not write */
/* it: the backward reads it only there).                                         */
/* `work` of ..._backward is the forward's, unchanged in between; the backward   */
/* uses a part of it as scratch (per-XCD partial sums of the gradients of faces  */
/* whose enlarged box spans more than 8 x 8 soft tiles; left cleared).           */
/* grad_img_to_zero (optional, (B,F,3,2)): cleared by the forward's one fill      */
/* launch so that the caller can hand it to ..._backward as g_img without a fill */
/* launch of its own.                                                            */
/* ------------------------------------------------------------------------- */
size_t kamd_dibr_rasterization_workspace(int B, int H, int W, int F, int K, int elem_size);
int kamd_dibr_rasterization_forward_f32(void* stream, int B, int H, int W, int F, int D, int K,
                                        const float* z, int64_t z_face_stride, int64_t z_vertex_stride,
                                        const float* img, const float* feat, const uint8_t* valid,
                                        const float* front, int64_t front_stride, double multiplier,
                                        float eps, float sigmainv, double margin, float* interp,
                                        int64_t* face_idx, float* weights, float* soft_mask,
                                        int32_t* hit_pair, float* hit_prob,
                                        int32_t* hit_rec, int32_t* item_count, uint32_t* work,
                                        void* workspace, float* grad_img_to_zero);
int kamd_dibr_rasterization_forward_f64(void* stream, int B, int H, int W, int F, int D, int K,
                                        const double* z, int64_t z_face_stride, int64_t z_vertex_stride,
                                        const double* img, const double* feat, const uint8_t* valid,
                                        const double* front, int64_t front_stride, double multiplier,
                                        float eps, float sigmainv, double margin, double* interp,
                                        int64_t* face_idx, double* weights, double* soft_mask,
                                        int32_t* hit_pair, double* hit_prob,
                                        int32_t* hit_rec, int32_t* item_count, uint32_t* work,
                                        void* workspace, double* grad_img_to_zero);
int kamd_dibr_rasterization_backward_f32(void* stream, int B, int H, int W, int F, int D, int K,
                                         const float* grad_feat, const float* grad_soft,
                                         const int64_t* face_idx, const float* weights,
                                         const float* soft_mask, const int32_t* hit_pair,
                                         const float* hit_prob,
                                         const int32_t* hit_rec, const int32_t* item_count,
                                         uint32_t* work, const float* img, const float* feat,
                                         double multiplier, float eps, float sigmainv,
                                         float* g_img, float* g_feat);
int kamd_dibr_rasterization_backward_f64(void* stream, int B, int H, int W, int F, int D, int K,
                                         const double* grad_feat, const double* grad_soft,
                                         const int64_t* face_idx, const double* weights,
                                         const double* soft_mask, const int32_t* hit_pair,
                                         const double* hit_prob,
                                         const int32_t* hit_rec, const int32_t* item_count,
                                         uint32_t* work, const double* img, const double* feat,
                                         double multiplier, float eps, float sigmainv,
                                         double* g_img, double* g_feat);
/* The backward of the linear loss sum(features * w_feat) + sum(soft_mask *    */
/* w_soft) of the forward's two outputs, through the forward: the arguments of  */
/* ..._backward with (grad_loss, w_feat, w_soft) in place of the two output      */
/* gradients.  grad_loss: the loss' gradient, ONE device scalar (read on the     */
/* device: no host sync); w_feat (B,H,W,D) and w_soft (B,H,W): the weights, laid */
/* out as the outputs; w_soft may be NULL (no soft-mask term).  The output       */
/* gradients grad_loss * w are formed where the kernels read them: the same      */
/* values ..._backward would consume from materialised gradients.                */
int kamd_dibr_weighted_sum_backward_f32(void* stream, int B, int H, int W, int F, int D, int K,
                                        const float* grad_loss, const float* w_feat,
                                        const float* w_soft,
                                        const int64_t* face_idx, const float* weights,
                                        const float* soft_mask, const int32_t* hit_pair,
                                        const float* hit_prob,
                                        const int32_t* hit_rec, const int32_t* item_count,
                                        uint32_t* work, const float* img, const float* feat,
                                        double multiplier, float eps, float sigmainv,
                                        float* g_img, float* g_feat);
int kamd_dibr_weighted_sum_backward_f64(void* stream, int B, int H, int W, int F, int D, int K,
                                        const double* grad_loss, const double* w_feat,
                                        const double* w_soft,
                                        const int64_t* face_idx, const double* weights,
                                        const double* soft_mask, const int32_t* hit_pair,
                                        const double* hit_prob,
                                        const int32_t* hit_rec, const int32_t* item_count,
                                        uint32_t* work, const double* img, const double* feat,
                                        double multiplier, float eps, float sigmainv,
                                        double* g_img, double* g_feat);

/* ------------------------------------------------------------------------- */
/* render.mesh.prepare_vertices, fused (the reference is     */
/* pure torch: kaolin/render/mesh/utils.py:128-175).  vertices (Bv,V,3) with    */
/* batch stride `vstride` elements (0 = one mesh shared by all B views),        */
/* faces (F,3) int64, proj (3); camera either rot (B,3,3) + trans (B,3) or      */
/* transform (B,4,3) (the other pointers NULL).  Outputs fv_cam (B,F,3,3),      */
/* fv_img (B,F,3,2), unit normals (B,F,3).  Backward: gradient w.r.t. the       */
/* vertices only, g_vertices (B,V,3) fully written; any of g_cam / g_img /      */
/* g_nrm may be NULL; adj_offsets (V+1) / adj_entries (3F, values face*3+k)     */
/* list each vertex's incident face corners.                                    */
/* ------------------------------------------------------------------------- */
int kamd_prepare_vertices_forward_f32(void* stream, int B, int V, int F, const float* vertices,
                                      int64_t vstride, const int64_t* faces, const float* proj,
                                      const float* rot, const float* trans, const float* transform,
                                      float* fv_cam, float* fv_img, float* normals);
int kamd_prepare_vertices_forward_f64(void* stream, int B, int V, int F, const double* vertices,
                                      int64_t vstride, const int64_t* faces, const double* proj,
                                      const double* rot, const double* trans, const double* transform,
                                      double* fv_cam, double* fv_img, double* normals);
int kamd_prepare_vertices_backward_f32(void* stream, int B, int V, int F, const float* vertices,
                                       int64_t vstride, const int64_t* faces, const float* proj,
                                       const float* rot, const float* trans, const float* transform,
                                       const int32_t* adj_offsets, const int32_t* adj_entries,
                                       const float* g_cam, const float* g_img, const float* g_nrm,
                                       float* g_vertices);
int kamd_prepare_vertices_backward_f64(void* stream, int B, int V, int F, const double* vertices,
                                       int64_t vstride, const int64_t* faces, const double* proj,
                                       const double* rot, const double* trans, const double* transform,
                                       const int32_t* adj_offsets, const int32_t* adj_entries,
                                       const double* g_cam, const double* g_img, const double* g_nrm,
                                       double* g_vertices);

/* ------------------------------------------------------------------------- */
/* render.mesh.deftet_sparse_render_forward_cuda(face_vertices_z,             */
/*     face_vertices_image, face_bboxes, pixel_coords, pixel_depth_ranges,    */
/*     knum, eps) -> [face_idx, pixel_depths, w0, w1]                          */
/* (reference: kaolin/csrc/render/mesh/deftet.cpp:47-108,   */
/* deftet_cuda.cu:31-232).  face_vertices_z (B,F,3), face_vertices_image      */
/* (B,F,3,2), face_bboxes (B,F,4) = (xmin,ymin,xmax,ymax), pixel_coords and    */
/* pixel_depth_ranges (B,P,2).  Outputs (B,P,K), FULLY written here (the       */
/* reference pre-fills them: -1 / -inf / 0 / 0): per pixel the first K faces   */
/* in mesh order whose box [min,max) and triangle contain the pixel with       */
/* min_depth <= depth < max_depth, unsorted.  workspace: sorted pixels, cell    */
/* table, per-pixel counters and two work lists,                               */
/* kamd_deftet_forward_workspace(B,F,P,elem_size) bytes (elem_size = 4 | 8),   */
/* data-independent, no initialisation needed.                                 */
/*                                                                             */
/* _forward_fused = the whole of DeftetSparseRenderer.forward                  */
/* (kaolin/render/mesh/deftet.py:269-315): the operator above, then hits       */
/* sorted by depth (descending, equal depths keep mesh order),                 */
/* w2 = 1 - (w0 + w1), corner features weighted and summed.  tmp_* (B,P,K) and */
/* hit_count (B,P) int32 are uninitialised scratch; sorted_face_idx (B,P,K),   */
/* weights (B,P,K,3), interpolated_features (B,P,K,D) are fully written.       */
/*                                                                             */
/* render.mesh.deftet_sparse_render_backward_cuda(grad, face_idx, weights,    */
/*     face_vertices_image, face_features, eps) -> [g_image, g_features]       */
/* (deftet.cpp:110-161, deftet_cuda.cu:240-449): grad (B,P,K,D), face_idx      */
/* (B,P,K), weights (B,P,K,3); both gradients ACCUMULATE: caller zero-fills    */
/* (the reference wrapper allocates them with zeros_like).                     */
/* ------------------------------------------------------------------------- */
size_t kamd_deftet_forward_workspace(int B, int F, int P, int elem_size);
int kamd_deftet_sparse_render_forward_f32(void* stream, int B, int F, int P, int K, const float* face_vertices_z,
        const float* face_vertices_image, const float* face_bboxes, const float* pixel_coords,
        const float* pixel_depth_ranges, float eps, int64_t* face_idx, float* pixel_depths, float* w0, float* w1,
        void* workspace, size_t workspace_bytes);
int kamd_deftet_sparse_render_forward_fused_f32(void* stream, int B, int F, int P, int K, int D,
        const float* face_vertices_z, const float* face_vertices_image, const float* face_bboxes,
        const float* pixel_coords, const float* pixel_depth_ranges, const float* face_features, float eps,
        int64_t* tmp_face_idx, float* tmp_depths, float* tmp_w0, float* tmp_w1, int32_t* hit_count,
        int64_t* sorted_face_idx, float* weights, float* interpolated_features, void* workspace,
        size_t workspace_bytes);
int kamd_deftet_sparse_render_backward_f32(void* stream, int B, int F, int P, int K, int D,
        const float* grad_interpolated_features, const int64_t* face_idx, const float* weights,
        const float* face_vertices_image, const float* face_features, float eps,
        float* grad_face_vertices_image, float* grad_face_features);
int kamd_deftet_sparse_render_forward_f64(void* stream, int B, int F, int P, int K, const double* face_vertices_z,
        const double* face_vertices_image, const double* face_bboxes, const double* pixel_coords,
        const double* pixel_depth_ranges, float eps, int64_t* face_idx, double* pixel_depths, double* w0, double* w1,
        void* workspace, size_t workspace_bytes);
int kamd_deftet_sparse_render_forward_fused_f64(void* stream, int B, int F, int P, int K, int D,
        const double* face_vertices_z, const double* face_vertices_image, const double* face_bboxes,
        const double* pixel_coords, const double* pixel_depth_ranges, const double* face_features, float eps,
        int64_t* tmp_face_idx, double* tmp_depths, double* tmp_w0, double* tmp_w1, int32_t* hit_count,
        int64_t* sorted_face_idx, double* weights, double* interpolated_features, void* workspace,
        size_t workspace_bytes);
int kamd_deftet_sparse_render_backward_f64(void* stream, int B, int F, int P, int K, int D,
        const double* grad_interpolated_features, const int64_t* face_idx, const double* weights,
        const double* face_vertices_image, const double* face_features, float eps,
        double* grad_face_vertices_image, double* grad_face_features);

/* ------------------------------------------------------------------------- */
/* ops.conversions.mesh_to_spc_cuda(face_vertices, level)                      */
/*     -> [octree uint8 (num_nodes), face_ids int64 (num_voxels),              */
/*         barycoords float (num_voxels, 2)]                                   */
/* (reference: kaolin/csrc/ops/conversions/mesh_to_spc/      */
/* mesh_to_spc.cpp:27-42, mesh_to_spc_cuda.cu:98-467, ops/spc/spc_cuda.cu:46-160)*/
/* face_vertices (F,3,3) float32 in [-1,1]^3.  Result sizes depend on the data, */
/* the library never allocates, so the operator is a short host sequence:      */
/*  1. proposals = (Morton code 0, triangle f) for every f; level_from = 0.     */
/*  2. stage_count(level_from, level_to = min(level_from + stage_levels(),     */
/*     level)): counts + offsets (n + 1, offsets[n] = total, read by the host); */
/*     stage_emit writes the `total` surviving (code, triangle) pairs at        */
/*     level_to; repeat from level_to with tested = 1 until level_to == level.  */
/*     Both return hipErrorInvalidValue, before any launch, unless              */
/*     0 <= level_from <= level_to <= 15 and                                    */
/*     level_to - level_from <= stage_levels() (the walker keeps 8 bits per     */
/*     depth in one 32-bit word): the rule of kamd_gs_to_spc_stage_*.           */
/*  3. build: stable sort by code, first triangle of every voxel, all octree    */
/*     levels, into the workspace; sizes[0] = voxels, sizes[1 + l] = nodes of   */
/*     octree level l (device int64[1 + level], read by the host).              */
/*  4. results: face_ids, barycoords of the point of the triangle closest to    */
/*     the voxel centre, octree bytes (levels concatenated root first).         */
/* ------------------------------------------------------------------------- */
int kamd_mesh_to_spc_stage_levels(void);
size_t kamd_mesh_to_spc_scan_workspace(int64_t n);
int kamd_mesh_to_spc_stage_count(void* stream, int64_t n, const float* face_vertices, const int64_t* morton,
                                 const int64_t* triangle_id, int level_from, int level_to, int tested,
                                 int32_t* counts, int64_t* offsets, void* scan_workspace);
int kamd_mesh_to_spc_stage_emit(void* stream, int64_t n, const float* face_vertices, const int64_t* morton,
                                const int64_t* triangle_id, int level_from, int level_to, int tested,
                                const int64_t* offsets, int64_t* morton_out, int64_t* triangle_id_out);
size_t kamd_mesh_to_spc_build_workspace(int64_t n, int level);
int kamd_mesh_to_spc_build(void* stream, int64_t n, int level, const int64_t* morton,
                           const int64_t* triangle_id, void* workspace, size_t workspace_bytes,
                           int64_t* sizes);
int kamd_mesh_to_spc_results(void* stream, int64_t n, int level, const float* face_vertices,
                             const void* workspace, int64_t num_voxels, int64_t octree_bytes,
                             uint8_t* octree, int64_t* face_ids, float* barycoords);

/* ------------------------------------------------------------------------- */
/* ops.conversions.gs_to_spc_cuda(means3D, scales, rotations, iso, tol, level) */
/*     -> [points int16 (N, 3), gaus_id int64 (N), pack_boundary bool (N),     */
/*         cov3d_invs float (G, 6)]                                            */
/* ops.conversions.integrate_gs_cuda(points, gaus_id, means3D, cov3d_invs,     */
/*     opacities, level, step) -> float (N)                                    */
/* (reference: kaolin/csrc/ops/conversions/gs_to_spc/gs_to_spc.cpp,            */
/* gs_to_spc_cuda.cu:146-804).  means3D (G,3), scales (G,3), rotations (G,4)   */
/* float32.  One (voxel, Gaussian) pair per voxel of `level` that the iso       */
/* ellipsoid of a Gaussian overlaps, ordered by (Morton code, Gaussian id).     */
/* The host sequence (the library never allocates):                            */
/*  1. prepare: cov3d_invs (G,6) and `prepared` (prepare_workspace(G) bytes:    */
/*     AABB and contact points of every Gaussian).                             */
/*  2. proposals = (Morton code 0, Gaussian g) for every g; level_from = 0,     */
/*     tested = 0 (the root is tested too).  stage_count(level_from, level_to = */
/*     min(level_from + stage_levels(), level)): counts + offsets (n + 1,       */
/*     offsets[n] = total, read by the host); stage_emit writes the `total`     */
/*     surviving pairs at level_to (no slot >= total is written); repeat from   */
/*     level_to with tested = 1 until level_to == level.                        */
/*  3. finish: stable sort by code on 3 * level bits, points, gaus_id and       */
/*     pack_boundary (one byte per pair: 1 at the first pair of a voxel).       */
/* integrate_gs is ONE launch and reads nothing back (graph-capturable); a      */
/* gaus_id outside [0, G) integrates to 0.  1 <= step <= 1024.                  */
/* ------------------------------------------------------------------------- */
int kamd_gs_to_spc_stage_levels(void);
size_t kamd_gs_to_spc_prepare_workspace(int64_t G);
int kamd_gs_to_spc_prepare(void* stream, int64_t G, const float* means3D, const float* scales,
                           const float* rotations, float iso, float tol, int level, float* cov3d_invs,
                           void* prepared);
size_t kamd_gs_to_spc_scan_workspace(int64_t n);
int kamd_gs_to_spc_stage_count(void* stream, int64_t n, int64_t G, const float* means3D, const float* cov3d_invs,
                               const void* prepared, float iso, const int64_t* morton, const int64_t* gaus_id,
                               int level_from, int level_to, int tested, int32_t* counts, int64_t* offsets,
                               void* scan_workspace);
int kamd_gs_to_spc_stage_emit(void* stream, int64_t n, int64_t G, const float* means3D, const float* cov3d_invs,
                              const void* prepared, float iso, const int64_t* morton, const int64_t* gaus_id,
                              int level_from, int level_to, int tested, const int64_t* offsets, int64_t total,
                              int64_t* morton_out, int64_t* gaus_id_out);
size_t kamd_gs_to_spc_finish_workspace(int64_t n);
int kamd_gs_to_spc_finish(void* stream, int64_t n, int level, const int64_t* morton, const int64_t* gaus_id,
                          void* workspace, size_t workspace_bytes, int16_t* points, int64_t* gaus_id_out,
                          uint8_t* pack_boundary);
int kamd_integrate_gs(void* stream, int64_t n, int64_t G, const int16_t* points, const int64_t* gaus_id,
                      const float* means3D, const float* cov3d_invs, const float* opacities, int level, int step,
                      float* values);

/* ------------------------------------------------------------------------- */
/* ops.mesh.unbatched_mesh_intersection_cuda(points, v1, v2, v3) -> result     */
/* (reference: kaolin/csrc/ops/mesh/mesh_intersection.cpp,  */
/* mesh_intersection_cuda.cu:101-253).  points (N,3); v1,v2,v3 (F,3) = the      */
/* faces' three vertices; result (N) fully written = number of faces the +x ray */
/* from each point crosses (check_sign takes its parity).                       */
/* ------------------------------------------------------------------------- */
int kamd_mesh_intersection_f32(void* stream, int N, int F, const float* points, const float* v1,
                               const float* v2, const float* v3, float* result);
int kamd_mesh_intersection_f64(void* stream, int N, int F, const double* points, const double* v1,
                               const double* v2, const double* v3, double* result);

/* ------------------------------------------------------------------------- */
/* metrics.unbatched_triangle_distance_forward_cuda(points, faces, dist,      */
/*     face_idx, dist_type) -> void                                           */
/* reference: kaolin/csrc/metrics/unbatched_triangle_distance.cpp:43-72,      */
/*            unbatched_triangle_distance_cuda.cu:237-317,418-443             */
/* points (N,3), faces (F,3,3); caller-allocated dist (N), face_idx (N) int64,*/
/* dist_type (N) int32 (0 plane, 1-3 vertex, 4-6 edge).                       */
/* ------------------------------------------------------------------------- */
size_t kamd_triangle_distance_forward_workspace(int N, int F, int elem_size);
int kamd_triangle_distance_forward_f32(void* stream, int N, int F,
                                       const float* points, const float* faces,
                                       float* dist, int64_t* face_idx, int32_t* dist_type,
                                       void* workspace);
int kamd_triangle_distance_forward_f64(void* stream, int N, int F,
                                       const double* points, const double* faces,
                                       double* dist, int64_t* face_idx, int32_t* dist_type,
                                       void* workspace);

/* metrics.unbatched_triangle_distance_backward_cuda(grad, points, faces,     */
/*     face_idx, dist_type, g_points, g_faces) -> void                        */
/* reference: unbatched_triangle_distance.cpp:74-114, .cu:319-416,445-474     */
/* g_points (N,3) overwritten; g_faces (F,3,3) accumulated (caller zeroes).   */
int kamd_triangle_distance_backward_f32(void* stream, int N, int F,
                                        const float* grad, const float* points,
                                        const float* faces, const int64_t* face_idx,
                                        const int32_t* dist_type, float* g_points,
                                        float* g_faces);
int kamd_triangle_distance_backward_f64(void* stream, int N, int F,
                                        const double* grad, const double* points,
                                        const double* faces, const int64_t* face_idx,
                                        const int32_t* dist_type, double* g_points,
                                        double* g_faces);

/* ------------------------------------------------------------------------- */
/* ops.conversions.trianglemeshes_to_voxelgrids (dense) -- the reference has  */
/* NO native kernel here (pure torch: kaolin/ops/conversions/trianglemesh.py: */
/* 29-110, ops/mesh/trianglemesh.py:410-458, ops/conversions/pointcloud.py:   */
/* 42-75); this entry point fuses subdivide-until-dense + point binning.      */
/* vertices (B,V,3) RAW, faces (F,3) int64 shared by the batch.  origin (B,3)  */
/* and scale (B) of the normalisation (v - origin) / scale, either may be NULL:*/
/* then origin = per-mesh minimum, scale = largest extent above the origin     */
/* (trianglemesh.py:84-96).  norm: scratch of                                 */
/* kamd_trianglemeshes_to_voxelgrids_workspace(B,V,elem_size) bytes (its first */
/* 4*B scalars return origin xyz + scale per mesh).  grid (B,R,R,R) is fully   */
/* written (0/1 in dtype).                                                     */
/* ------------------------------------------------------------------------- */
size_t kamd_trianglemeshes_to_voxelgrids_workspace(int B, int V, int elem_size);
int kamd_trianglemeshes_to_voxelgrids_f32(void* stream, int B, int V, int F, int R,
                                          const float* vertices, const int64_t* faces,
                                          const float* origin, const float* scale, float* norm,
                                          float* grid);
int kamd_trianglemeshes_to_voxelgrids_f64(void* stream, int B, int V, int F, int R,
                                          const double* vertices, const int64_t* faces,
                                          const double* origin, const double* scale, double* norm,
                                          double* grid);

/* The same marks as one BIT per voxel (the sparse result of trianglemeshes_to_voxelgrids(return_sparse=True): the reference builds  */
/* its COO tensor from the unique voxel indices and never allocates R^3 scalars, kaolin/ops/conversions/pointcloud.py:66-73).       */
/* bits: B * kamd_trianglemeshes_to_voxelbits_words(R) uint32 words, cleared by the call; voxel ((x R + y) R + z) of mesh b = bit     */
/* (lin & 31) of word b * words + (lin >> 5).  norm: as kamd_trianglemeshes_to_voxelgrids_*.                                          */
size_t kamd_trianglemeshes_to_voxelbits_words(int R);
int kamd_trianglemeshes_to_voxelbits_f32(void* stream, int B, int V, int F, int R, const float* vertices,
                                         const int64_t* faces, const float* origin, const float* scale, float* norm,
                                         uint32_t* bits);
int kamd_trianglemeshes_to_voxelbits_f64(void* stream, int B, int V, int F, int R, const double* vertices,
                                         const int64_t* faces, const double* origin, const double* scale, double* norm,
                                         uint32_t* bits);

/* ------------------------------------------------------------------------- */
/* ops.voxelgrid.fill(voxelgrids) -> bool (N,X,Y,Z): the walls (value != 0:    */
/* NaN is a wall, -0.0 is empty) and every empty voxel with no path of         */
/* face-adjacent empty voxels to an empty voxel of the six boundary faces.     */
/* The reference runs SciPy's binary_fill_holes on the host and raises on a    */
/* GPU tensor (kaolin/ops/voxelgrid.py:143-206); this is an exact flood fill   */
/* over two bit grids (csrc/voxelgrid_fill.hip).  voxelgrids: element strides  */
/* stride_n/x/y/z (any layout); filled: N*X*Y*Z contiguous bytes of 0/1, fully */
/* written; workspace: kamd_voxelgrid_fill_workspace(N,X,Y,Z) bytes, 4-byte    */
/* aligned.  The call launches passes until one changes nothing and reads a    */
/* word back every few passes: it SYNCHRONISES the stream (not capturable in a */
/* graph).  host_stats (host int32[3], may be NULL): passes that worked,       */
/* passes launched, host reads.  f16: voxelgrids points to IEEE half values.   */
/* ------------------------------------------------------------------------- */
size_t kamd_voxelgrid_fill_workspace(int64_t N, int X, int Y, int Z);
int kamd_voxelgrid_fill_u8(void* stream, int64_t N, int X, int Y, int Z, const uint8_t* voxelgrids, int64_t stride_n,
                           int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                           int32_t* host_stats);
int kamd_voxelgrid_fill_i32(void* stream, int64_t N, int X, int Y, int Z, const int32_t* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                            int32_t* host_stats);
int kamd_voxelgrid_fill_i64(void* stream, int64_t N, int X, int Y, int Z, const int64_t* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                            int32_t* host_stats);
int kamd_voxelgrid_fill_f16(void* stream, int64_t N, int X, int Y, int Z, const void* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                            int32_t* host_stats);
int kamd_voxelgrid_fill_f32(void* stream, int64_t N, int X, int Y, int Z, const float* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                            int32_t* host_stats);
int kamd_voxelgrid_fill_f64(void* stream, int64_t N, int X, int Y, int Z, const double* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, uint8_t* filled, void* workspace,
                            int32_t* host_stats);

/* ------------------------------------------------------------------------- */
/* ops.conversions.marching_tetrahedra, one item of the batch (reference: ~25  */
/* torch kernels, kaolin/ops/conversions/tetmesh.py; csrc/marching_tetrahedra  */
/* .hip has the pipeline).  tets: (T,4) int64 contiguous, 16-byte aligned;     */
/* vertices (V,3), sdf (V) contiguous; V < 2^32.  A vertex is occupied when    */
/* sdf > 0; a tet with a corner outside [0,V) is ignored (the shim raises      */
/* before it gets here).  Result sizes depend on the data, so the sequence is  */
/*   1. classify: workspace <- occupancy bits, the case of every tet, scanned  */
/*      counts; host_counts[0..1] <- tets that emit one / two triangles.       */
/*   2. edges (skip when both are 0): edges_workspace <- the valid tets in tet */
/*      order, the sorted unique crossing edges; *host_num_unique <- their     */
/*      number = the number of output vertices.                                */
/*   3. emit: verts (num_unique,3), edges (num_unique,2) int64 = the (a,b),    */
/*      a < b, each vertex interpolates, faces (n_one + 2 n_two, 3) int64,     */
/*      tet_idx (n_one + 2 n_two) int64 or NULL.                               */
/* Steps 1 and 2 each read a count back: they SYNCHRONISE the stream (not      */
/* capturable in a graph).  The *_workspace queries are host arithmetic; 0 =   */
/* nothing to do.  backward: grad_vertices (V,3) and grad_sdf (V) must be      */
/* zeroed by the caller; accumulated with fp atomic adds.                      */
/* ------------------------------------------------------------------------- */
size_t kamd_marching_tetrahedra_workspace(int64_t T, int64_t V);
size_t kamd_marching_tetrahedra_edges_workspace(int64_t n_one, int64_t n_two);
int kamd_marching_tetrahedra_classify_f32(void* stream, int64_t T, int64_t V, const int64_t* tets, const float* sdf,
                                          void* workspace, int64_t* host_counts);
int kamd_marching_tetrahedra_classify_f64(void* stream, int64_t T, int64_t V, const int64_t* tets, const double* sdf,
                                          void* workspace, int64_t* host_counts);
int kamd_marching_tetrahedra_edges(void* stream, int64_t T, int64_t V, const int64_t* tets, const void* workspace, int64_t n_one,
                                   int64_t n_two, void* edges_workspace, int64_t* host_num_unique);
int kamd_marching_tetrahedra_emit_f32(void* stream, int64_t V, const int64_t* tets, const float* vertices, const float* sdf,
                                      const void* edges_workspace, int64_t n_one, int64_t n_two, int64_t num_unique,
                                      float* verts, int64_t* edges, int64_t* faces, int64_t* tet_idx);
int kamd_marching_tetrahedra_emit_f64(void* stream, int64_t V, const int64_t* tets, const double* vertices, const double* sdf,
                                      const void* edges_workspace, int64_t n_one, int64_t n_two, int64_t num_unique,
                                      double* verts, int64_t* edges, int64_t* faces, int64_t* tet_idx);
int kamd_marching_tetrahedra_backward_f32(void* stream, int64_t num_edges, int64_t V, const int64_t* edges, const float* vertices,
                                          const float* sdf, const float* grad_verts, float* grad_vertices, float* grad_sdf);
int kamd_marching_tetrahedra_backward_f64(void* stream, int64_t num_edges, int64_t V, const int64_t* edges, const double* vertices,
                                          const double* sdf, const double* grad_verts, double* grad_vertices, double* grad_sdf);

/* ------------------------------------------------------------------------- */
/* ops.mesh.subdivide_tetmesh (reference: torch.unique(dim=0) over the 6 T     */
/* edge rows and a chain of gathers / cats / stacks, kaolin/ops/mesh/tetmesh   */
/* .py; csrc/subdivide_tetmesh.hip has the pipeline).  tets: (T,4) int64       */
/* contiguous, 16-byte aligned, every id in [0,V) (the shim raises before it   */
/* gets here), V < 2^32.  Topology, once per call:                             */
/*   1. edges: workspace <- the 6 T keys min << 32 | max, sorted, and the      */
/*      unique ones; *host_num_edges <- E.  Reads E back: SYNCHRONISES the     */
/*      stream (not capturable in a graph).                                    */
/*   2. emit: edges (E,2) int64 = the (min,max) pairs in ascending order,      */
/*      new_tets (8 T,4) int64: eight blocks of T rows in tet order, edge e    */
/*      being vertex V + e.  Both 16-byte aligned, fully written.              */
/* The workspace query is host arithmetic; 0 = nothing to do (T = 0).          */
/* Midpoints, the whole batch per call; vertices (B,V,3) and features (B,V,D)  */
/* with contiguous items `*_batch_stride` elements apart (0: an expanded       */
/* batch), features may be NULL (D ignored):                                   */
/* `edges` (E,2): every id in [0,V), gathered by UNCHECKED (the shim checks    */
/* edges that do not come from step 2):                                       */
/*   forward: new_vertices (B,V+E,3), new_features (B,V+E,D) contiguous, rows  */
/*      [0,V) copied, row V + e = (x[min] + x[max]) * 0.5; one launch.         */
/*   backward: grad_new_* (B,V+E,.) contiguous, either may be NULL (its        */
/*      result is then not touched); grad_* (B,V,.) fully written: g[v] + the  */
/*      halves of the edges with min = v (a plain store), then fp atomic adds  */
/*      of the halves into the max ends.                                       */
/* ------------------------------------------------------------------------- */
size_t kamd_subdivide_tetmesh_workspace(int64_t T, int64_t V);
int kamd_subdivide_tetmesh_edges(void* stream, int64_t T, int64_t V, const int64_t* tets, void* workspace,
                                 int64_t* host_num_edges);
int kamd_subdivide_tetmesh_emit(void* stream, int64_t T, int64_t V, const int64_t* tets, const void* workspace, int64_t num_edges,
                                int64_t* edges, int64_t* new_tets);
int kamd_tetmesh_midpoints_forward_f32(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const float* vertices,
                                       int64_t vertices_batch_stride, const float* features, int64_t features_batch_stride,
                                       const int64_t* edges, float* new_vertices, float* new_features);
int kamd_tetmesh_midpoints_forward_f64(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const double* vertices,
                                       int64_t vertices_batch_stride, const double* features, int64_t features_batch_stride,
                                       const int64_t* edges, double* new_vertices, double* new_features);
int kamd_tetmesh_midpoints_backward_f32(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const float* grad_new_vertices,
                                        const float* grad_new_features, const int64_t* edges, float* grad_vertices,
                                        float* grad_features);
int kamd_tetmesh_midpoints_backward_f64(void* stream, int64_t B, int64_t V, int64_t E, int64_t D, const double* grad_new_vertices,
                                        const double* grad_new_features, const int64_t* edges, double* grad_vertices,
                                        double* grad_features);

/* ------------------------------------------------------------------------- */
/* ops.mesh.subdivide_trianglemesh: one iteration of Loop subdivision with a   */
/* per-vertex alpha (reference: two torch.unique, a sparse bmm, two sorts and  */
/* a chain of gathers, kaolin/ops/mesh/trianglemesh.py; csrc/                  */
/* subdivide_trianglemesh.hip has the pipeline and the rules).  faces: (F,3)   */
/* int64 contiguous, every id in [0,V) (the shim raises before it gets here),  */
/* V < 2^32.  Topology, once per iteration:                                    */
/*   1. edges: workspace <- the 3 F keys min << 32 | max, sorted, and the      */
/*      unique ones; *host_num_edges <- E.  Reads E back: SYNCHRONISES the     */
/*      stream (not capturable in a graph).                                    */
/*   2. emit, all fully written except `opp`: edges (E,2) int64 = the          */
/*      (min,max) pairs in ascending order; new_faces (4 F,3) int64, four rows */
/*      per face, edge e being vertex V + e; count (E) int32 = face slots per  */
/*      edge; opp (E,2) int64 = the opposite corners of the first two slots    */
/*      claimed (valid where count == 2; read there only); tlist (E,2) int64 = */
/*      (min end, edge id) in ascending (max,min) order; runs (V+1,2) int64 =  */
/*      where the runs of vertex v start in edges / tlist; valence (V) int32.  */
/*      The int64 results and the workspace are 16-byte aligned.               */
/* The workspace query is host arithmetic; 0 = nothing to do (F = 0).          */
/* Values, the whole batch per call; vertices (B,V,3) and alpha (B,V) with     */
/* contiguous items `*_batch_stride` elements apart (0: an expanded batch);    */
/* alpha NULL = the Loop weights from the valences.  The topology tensors are  */
/* gathered by UNCHECKED: they come from step 2.                               */
/*   forward: new_vertices (B,V+E,3), new_alpha (B,V+E; NULL with alpha NULL)  */
/*      contiguous, fully written by one launch; no floating-point atomics.    */
/*   backward: grad_new_vertices (B,V+E,3), grad_new_alpha (B,V+E) or NULL;    */
/*      grad_vertices (B,V,3), grad_alpha (B,V) or NULL, fully written: a      */
/*      gather with plain stores, then fp atomic adds of the opposite-corner   */
/*      terms.                                                                 */
/* ------------------------------------------------------------------------- */
size_t kamd_subdivide_trianglemesh_workspace(int64_t F, int64_t V);
int kamd_subdivide_trianglemesh_edges(void* stream, int64_t F, int64_t V, const int64_t* faces, void* workspace,
                                      int64_t* host_num_edges);
int kamd_subdivide_trianglemesh_emit(void* stream, int64_t F, int64_t V, const int64_t* faces, void* workspace, int64_t num_edges,
                                     int64_t* edges, int64_t* new_faces, int32_t* count, int64_t* opp, int64_t* tlist, int64_t* runs,
                                     int32_t* valence);
int kamd_trianglemesh_loop_forward_f32(void* stream, int64_t B, int64_t V, int64_t E, const float* vertices,
                                       int64_t vertices_batch_stride, const float* alpha, int64_t alpha_batch_stride,
                                       const int64_t* edges, const int32_t* count, const int64_t* opp, const int64_t* tlist,
                                       const int64_t* runs, const int32_t* valence, float* new_vertices, float* new_alpha);
int kamd_trianglemesh_loop_forward_f64(void* stream, int64_t B, int64_t V, int64_t E, const double* vertices,
                                       int64_t vertices_batch_stride, const double* alpha, int64_t alpha_batch_stride,
                                       const int64_t* edges, const int32_t* count, const int64_t* opp, const int64_t* tlist,
                                       const int64_t* runs, const int32_t* valence, double* new_vertices, double* new_alpha);
int kamd_trianglemesh_loop_backward_f32(void* stream, int64_t B, int64_t V, int64_t E, const float* grad_new_vertices,
                                        const float* grad_new_alpha, const float* vertices, int64_t vertices_batch_stride,
                                        const float* alpha, int64_t alpha_batch_stride, const int64_t* edges, const int32_t* count,
                                        const int64_t* opp, const int64_t* tlist, const int64_t* runs, const int32_t* valence,
                                        float* grad_vertices, float* grad_alpha);
int kamd_trianglemesh_loop_backward_f64(void* stream, int64_t B, int64_t V, int64_t E, const double* grad_new_vertices,
                                        const double* grad_new_alpha, const double* vertices, int64_t vertices_batch_stride,
                                        const double* alpha, int64_t alpha_batch_stride, const int64_t* edges, const int32_t* count,
                                        const int64_t* opp, const int64_t* tlist, const int64_t* runs, const int32_t* valence,
                                        double* grad_vertices, double* grad_alpha);

/* ------------------------------------------------------------------------- */
/* ops.conversions.voxelgrids_to_cubic_meshes (reference: conv3d, nonzero,     */
/* repeat_interleave and a torch.unique(dim=0) per item, kaolin/ops/           */
/* conversions/voxelgrid.py; csrc/cubic_meshes.hip has the sort-free pipeline). */
/* voxelgrids: (B,X,Y,Z) with ELEMENT strides (any layout, read in place);     */
/* u8 also serves bool, f16 is the raw half.  (X+1)(Y+1)(Z+1) < 2^31 per item. */
/* One `workspace` of kamd_cubic_meshes_workspace(B,X,Y,Z) bytes (host         */
/* arithmetic; 0 = an empty batch or a lattice beyond the 32-bit range),       */
/* 16-byte aligned, carries the state from step to step:                       */
/*   1. classify_*: a code byte per lattice point and four counts per          */
/*      workgroup (vertices, faces of axis 0, 1, 2).                           */
/*   2. scan: exclusive scans of the counts; host_totals (B,4) uint32 <- per   */
/*      item the vertices and the faces of axis 0, 1, 2.  Reads them back:     */
/*      SYNCHRONISES the stream (not capturable in a graph).                   */
/*   3. emit_vertices: verts (sum V_b, 3) float32, the items one after the     */
/*      other, lattice coordinates in lexicographic order.                     */
/*   4. emit_faces: faces int64, the items one after the other, ids local to   */
/*      the item: (sum N_b, 4) quads, or with is_trimesh (2 sum N_b, 3), item  */
/*      b holding corners [0,3,1] of its quads in rows [0,N_b) and [2,1,3] in  */
/*      [N_b, 2 N_b).  Needs step 3 (the rank of every vertex).                */
/* Steps 3 and 4 are skipped by the caller when nothing is to be written.      */
/* ------------------------------------------------------------------------- */
size_t kamd_cubic_meshes_workspace(int64_t B, int X, int Y, int Z);
int kamd_cubic_meshes_classify_u8(void* stream, int64_t B, int X, int Y, int Z, const uint8_t* voxelgrids, int64_t stride_n,
                                  int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace);
int kamd_cubic_meshes_classify_f16(void* stream, int64_t B, int X, int Y, int Z, const void* voxelgrids, int64_t stride_n,
                                   int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace);
int kamd_cubic_meshes_classify_f32(void* stream, int64_t B, int X, int Y, int Z, const float* voxelgrids, int64_t stride_n,
                                   int64_t stride_x, int64_t stride_y, int64_t stride_z, void* workspace);
int kamd_cubic_meshes_scan(void* stream, int64_t B, int X, int Y, int Z, void* workspace, uint32_t* host_totals);
int kamd_cubic_meshes_emit_vertices(void* stream, int64_t B, int X, int Y, int Z, void* workspace, float* verts);
int kamd_cubic_meshes_emit_faces(void* stream, int64_t B, int X, int Y, int Z, const void* workspace, int is_trimesh,
                                 int64_t* faces);

/* ------------------------------------------------------------------------- */
/* ops.conversions.voxelgrids_to_trianglemeshes: marching cubes (reference:    */
/* kaolin/csrc/ops/conversions/unbatched_mcube; csrc/mcube.hip has the         */
/* pipeline, csrc/mcube_table.h the generated case table).  voxelgrids:        */
/* (B,X,Y,Z), X,Y,Z >= 1, with ELEMENT strides (any layout, read in place); u8 */
/* also serves bool, f16 is the raw half.  border != 0: the field is the grid  */
/* inside a border of zeros, voxel n at coordinate n + 1, a lattice of         */
/* (X+1)(Y+1)(Z+1) cells; border == 0: the grid as given, the cells between    */
/* its points, a lattice of X Y Z points.  3 x lattice < 2^31 per item.        */
/* iso_value must not be NaN.  One `workspace` of kamd_mcube_workspace(...)    */
/* bytes (host arithmetic; 0 = nothing to do or beyond the 32-bit range),      */
/* 16-byte aligned, carries the state from step to step:                       */
/*   1. classify_*: the case byte per cell and two counts per workgroup        */
/*      (own vertices, triangles).                                             */
/*   2. scan: exclusive scans of the counts; host_totals (B,2) uint32 <- per   */
/*      item the vertices and the triangles.  Reads them back: SYNCHRONISES    */
/*      the stream (not capturable in a graph).                                */
/*   3. emit_vertices_*: verts (verts_rows = sum V_b, 3) float32, the items    */
/*      one after the other, ordered by the lower end of the vertex' lattice   */
/*      edge in raster order, then by axis; and every cell's first vertex id.  */
/*   4. emit_faces: faces (faces_rows = sum F_b, 3) int64, ids local to the    */
/*      item, cells in raster order.  Needs step 3.                            */
/* Steps 3 and 4 are skipped by the caller when nothing is to be written.      */
/*   backward_*: after steps 1-3 with border != 0, on the same grid and        */
/*      workspace: grad_voxelgrids (B,X,Y,Z) contiguous, of the grid's type,   */
/*      <- the gradient of the vertex positions, float32 accumulation in a     */
/*      fixed order; fully written, one launch, no atomics.                    */
/* ------------------------------------------------------------------------- */
size_t kamd_mcube_workspace(int64_t B, int X, int Y, int Z, int border);
int kamd_mcube_classify_u8(void* stream, int64_t B, int X, int Y, int Z, int border, const uint8_t* voxelgrids, int64_t stride_n,
                           int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace);
int kamd_mcube_classify_f16(void* stream, int64_t B, int X, int Y, int Z, int border, const void* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace);
int kamd_mcube_classify_f32(void* stream, int64_t B, int X, int Y, int Z, int border, const float* voxelgrids, int64_t stride_n,
                            int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace);
int kamd_mcube_scan(void* stream, int64_t B, int X, int Y, int Z, int border, void* workspace, uint32_t* host_totals);
int kamd_mcube_emit_vertices_u8(void* stream, int64_t B, int X, int Y, int Z, int border, const uint8_t* voxelgrids, int64_t stride_n,
                                int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                int64_t verts_rows);
int kamd_mcube_emit_vertices_f16(void* stream, int64_t B, int X, int Y, int Z, int border, const void* voxelgrids, int64_t stride_n,
                                 int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                 int64_t verts_rows);
int kamd_mcube_emit_vertices_f32(void* stream, int64_t B, int X, int Y, int Z, int border, const float* voxelgrids, int64_t stride_n,
                                 int64_t stride_x, int64_t stride_y, int64_t stride_z, float iso_value, void* workspace, float* verts,
                                 int64_t verts_rows);
int kamd_mcube_emit_faces(void* stream, int64_t B, int X, int Y, int Z, int border, const void* workspace, int64_t* faces,
                          int64_t faces_rows);
int kamd_mcube_backward_f16(void* stream, int64_t B, int X, int Y, int Z, const void* voxelgrids, int64_t stride_n, int64_t stride_x,
                            int64_t stride_y, int64_t stride_z, float iso_value, const void* workspace, const float* grad_verts,
                            int64_t verts_rows, void* grad_voxelgrids);
int kamd_mcube_backward_f32(void* stream, int64_t B, int X, int Y, int Z, const float* voxelgrids, int64_t stride_n, int64_t stride_x,
                            int64_t stride_y, int64_t stride_z, float iso_value, const void* workspace, const float* grad_verts,
                            int64_t verts_rows, float* grad_voxelgrids);

/* ------------------------------------------------------------------------- */
/* ops.conversions.FlexiCubes: differentiable dual marching cubes, float32     */
/* (the reference is pure PyTorch, kaolin/ops/conversions/flexicubes; no _C    */
/* operator).  csrc/flexicubes.hip has the pipeline, csrc/flexicubes_table.h   */
/* the generated case tables.  vertices (V,3) and sdf (V,) contiguous float32, */
/* V < 2^31; cube_idx (C,8) int64 with ELEMENT strides, C = rx ry rz cubes laid */
/* out x ry rz + y rz + z, 12 C < 2^31; beta (C,12), alpha (C,8), gamma (C,)   */
/* raw weights, contiguous, NULL = ones.  Steps, in this order:                */
/*   1. classify: the case byte per cube (ambiguity rule applied) into         */
/*      `workspace` (kamd_flexicubes_workspace(C) bytes, 16-byte aligned), and */
/*      host_totals[9] <- per count class k = 1..4 the cubes [k-1] and the      */
/*      (dual vertex, edge) incidences [4+k-1]; [8] != 0: an id of cube_idx     */
/*      lies outside [0, V) (nothing was read through it; stop here).          */
/*      S = sum cubes, num_vd = sum k cubes_k.  HOST READ: synchronises.       */
/*   2. edges (S > 0): surf (S,4) int32 <- per surface cube (cube, case, first */
/*      dual vertex, first incidence); the pairs of its 12 edges sorted into   */
/*      `edges_workspace` (kamd_flexicubes_edges_workspace(S) bytes);          */
/*      *host_num_quads <- crossed edges shared by four cubes.  HOST READ.     */
/*   3. faces (num_quads > 0): quads (Q,4) int32 dual-vertex ids, quad_of      */
/*      (12 S) int32 <- 4 quad + corner of (surface cube, edge) or -1, faces   */
/*      (faces_rows,3) int64, faces_rows = 2 Q, or 4 Q with training (centre   */
/*      vertex num_vd + quad).                                                 */
/*   4. forward: out_vertices rows [0, num_vd), vd_gamma (num_vd), l_dev       */
/*      (num_incidences).  No atomics.  centers (training, Q > 0):             */
/*      out_vertices rows [num_vd, num_vd + Q).                                */
/*   backward: grad_x (V,3), grad_sdf (V,), grad_beta, grad_alpha, grad_gamma  */
/*      (shapes of the weights; NULL with its weight) must arrive ZEROED.      */
/*      grad_x / grad_sdf are accumulated with float atomics; the weights'     */
/*      rows are written by their owner.  grad_gamma only with training.       */
/* Not capturable in a graph (two host reads).                                 */
/* ------------------------------------------------------------------------- */
size_t kamd_flexicubes_workspace(int64_t C);
int kamd_flexicubes_classify(void* stream, int64_t V, int64_t C, int rx, int ry, int rz, const float* sdf, const int64_t* cube_idx,
                             int64_t stride_cube, int64_t stride_corner, void* workspace, uint32_t* host_totals);
size_t kamd_flexicubes_edges_workspace(int64_t S);
int kamd_flexicubes_edges(void* stream, int64_t V, int64_t C, int64_t S, const float* sdf, const int64_t* cube_idx, int64_t stride_cube,
                          int64_t stride_corner, const void* workspace, int32_t* surf, void* edges_workspace, int64_t* host_num_quads);
int kamd_flexicubes_faces(void* stream, int64_t C, int64_t S, int64_t num_vd, int64_t num_quads, const float* gamma, float weight_scale,
                          int training, const int32_t* surf, const void* edges_workspace, int32_t* quads, int32_t* quad_of,
                          int64_t* faces, int64_t faces_rows);
int kamd_flexicubes_forward(void* stream, int64_t V, int64_t C, int64_t S, int64_t num_vd, int64_t num_incidences, const float* vertices,
                            const float* sdf, const int64_t* cube_idx, int64_t stride_cube, int64_t stride_corner, const float* beta,
                            const float* alpha, const float* gamma, float weight_scale, const int32_t* surf, float* out_vertices,
                            float* vd_gamma, float* l_dev);
int kamd_flexicubes_centers(void* stream, int64_t num_vd, int64_t num_quads, const int32_t* quads, const float* vd_gamma,
                            float* out_vertices);
int kamd_flexicubes_backward(void* stream, int64_t V, int64_t C, int64_t S, int64_t num_vd, int64_t num_incidences, int64_t num_quads,
                             const float* vertices, const float* sdf, const int64_t* cube_idx, int64_t stride_cube, int64_t stride_corner,
                             const float* beta, const float* alpha, const float* gamma, float weight_scale, int training,
                             const int32_t* surf, const int32_t* quads, const int32_t* quad_of, const float* out_vertices,
                             const float* vd_gamma, const float* grad_vertices, const float* grad_l_dev, float* grad_x, float* grad_sdf,
                             float* grad_beta, float* grad_alpha, float* grad_gamma);

/* ------------------------------------------------------------------------- */
/* metrics.tetmesh: tetrahedron_volume, equivolume, amips (reference: chains   */
/* of 10-20 torch kernels, kaolin/metrics/tetmesh.py; csrc/tetmesh_metrics.hip */
/* has the kernels).  tet_vertices (B,T,4,3): every item's (T,4,3) block is    */
/* contiguous, items are batch_stride ELEMENTS apart (>= 0; 0 = one item read  */
/* B times).  16-byte loads are used when the base and the batch stride allow, */
/* scalar loads otherwise.  Nothing reads back or synchronises: capturable.    */
/*   volume:     volumes (B,T) = ((A-D).((B-D)x(C-D)))/6; backward takes       */
/*               grad_volumes (B,T) and fully writes grad_tet_vertices.        */
/*   equivolume: loss (B) = mean_t |v - mean[0]|^power, power in 1..16; mean   */
/*               is ONE device element.  backward: grad_loss (B); either of    */
/*               grad_tet_vertices (B,T,4,3) and grad_mean (1) may be NULL.    */
/*   amips:      inverse_offset_matrix (B,T,3,3), items inverse_batch_stride   */
/*               elements apart (0 broadcasts one item); loss (B).  backward:  */
/*               grad_loss (B); either of grad_tet_vertices and                */
/*               grad_inverse_offset_matrix (B,T,3,3, per item: the caller     */
/*               sums a broadcast batch) may be NULL.                          */
/* The losses (and grad_mean) are reduced without atomics: one double partial  */
/* per workgroup in `workspace` (kamd_tetmesh_reduce_workspace(B,T) bytes,     */
/* 8-byte aligned), then a second launch adds them in a fixed order.           */
/* ------------------------------------------------------------------------- */
size_t kamd_tetmesh_reduce_workspace(int64_t B, int64_t T);
int kamd_tetmesh_volume_forward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                    float* volumes);
int kamd_tetmesh_volume_backward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                     const float* grad_volumes, float* grad_tet_vertices);
int kamd_tetmesh_equivolume_forward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                        const float* mean, int power, float* loss, void* workspace);
int kamd_tetmesh_equivolume_backward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                         const float* mean, int power, const float* grad_loss, float* grad_tet_vertices,
                                         float* grad_mean, void* workspace);
int kamd_tetmesh_amips_forward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                   const float* inverse_offset_matrix, int64_t inverse_batch_stride, float* loss, void* workspace);
int kamd_tetmesh_amips_backward_f32(void* stream, int64_t B, int64_t T, const float* tet_vertices, int64_t batch_stride,
                                    const float* inverse_offset_matrix, int64_t inverse_batch_stride, const float* grad_loss,
                                    float* grad_tet_vertices, float* grad_inverse_offset_matrix);
int kamd_tetmesh_volume_forward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                    double* volumes);
int kamd_tetmesh_volume_backward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                     const double* grad_volumes, double* grad_tet_vertices);
int kamd_tetmesh_equivolume_forward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                        const double* mean, int power, double* loss, void* workspace);
int kamd_tetmesh_equivolume_backward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                         const double* mean, int power, const double* grad_loss, double* grad_tet_vertices,
                                         double* grad_mean, void* workspace);
int kamd_tetmesh_amips_forward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                   const double* inverse_offset_matrix, int64_t inverse_batch_stride, double* loss, void* workspace);
int kamd_tetmesh_amips_backward_f64(void* stream, int64_t B, int64_t T, const double* tet_vertices, int64_t batch_stride,
                                    const double* inverse_offset_matrix, int64_t inverse_batch_stride, const double* grad_loss,
                                    double* grad_tet_vertices, double* grad_inverse_offset_matrix);

/* ------------------------------------------------------------------------- */
/* ops.spc: the core of the structured point cloud (SPC) operators (reference: */
/* kaolin/csrc/ops/spc/{spc,query,feature_grids,point_utils}*; csrc/spc.hip).  */
/* Morton layout: bit 3i = z_i, 3i+1 = y_i, 3i+2 = x_i, 15 bits a coordinate.  */
/* points are int16 (N,3), codes int64, octrees uint8, exsum int32 in the      */
/* current layout (per octree the inclusive sum of the bit counts, num_bytes   */
/* entries).  Every kernel receives the sizes of the buffers it indexes and    */
/* compares each data-derived index with them: an index out of range is a miss */
/* (query) or a skipped write (the others), never an access.                   */
/*   points_to_morton / morton_to_points / points_to_corners: one launch each. */
/*   octree_build: codes (any order, duplicates allowed) are                   */
/*     masked to 3*level bits, sorted (keys-only radix sort, 8 bits a pass),   */
/*     made unique, and every level is built bottom-up in the workspace        */
/*     `sorted` promises ascending codes and skips the sort only: the unique   */
/*     pass still runs, so equal neighbours are allowed (pointcloud.hip passes */
/*     its sorted keys with their duplicates and reads U from host_sizes[0])   */
/*     (kamd_spc_octree_workspace(n, level) bytes).  host_sizes (HOST memory,  */
/*     1 + level int64: unique codes, then nodes per level root first) is the  */
/*     one host read: the call synchronises the stream.  octree_gather then    */
/*     writes the octree_bytes = sum of the level sizes bytes.  1 <= level <=  */
/*     15, n >= 1.                                                             */
/*   scan_octrees: octrees (total_bytes) of B items, starts (DEVICE, B + 1      */
/*     int64, starts[0] = 0, starts[B] = total_bytes, items non-empty);        */
/*     total_bytes * 8 < 2^31.  Writes exsum (total_bytes) and reads back, once */
/*     for the batch, host_pyramids (HOST memory, B x 35 int32: the (2, 17)    */
/*     pyramid of the item, then its depth).  The walk of an item clamps its   */
/*     index to the item's length.  workspace: kamd_spc_scan_workspace bytes.  */
/*   generate_points: meta (DEVICE, B x (2 + 2 (max_level + 2)) int64: the     */
/*     item's first octree byte, its first point, pyramid[0][:], pyramid[1][:]).*/
/*     max_level launches (grid.y = item), no host read.  num_bytes and         */
/*     num_points bound every index.  B <= 65535.                              */
/*   query / query_multiscale: coords (Q,3) half / float / double in [-1,1],   */
/*     read in place; result int64 (Q) / (Q, level + 1); -1 = miss.  One       */
/*     launch, no host read, no allocation: capturable.  level <= 15.          */
/*   to_dense: points = the packed point hierarchy (num_points rows), meta     */
/*     (DEVICE, 2 B + 1 int64: the B + 1 prefix of the items' rows at the       */
/*     level, then every item's first point of the level); features (rows, C), */
/*     grid (B, C, E, E, E), E = 2^level.  forward = zero fill + one thread     */
/*     per (row, channel); backward = the matching gather.  No atomics.        */
/* ------------------------------------------------------------------------- */
int kamd_spc_points_to_morton(void* stream, int64_t n, const int16_t* points, int64_t* morton);
int kamd_spc_morton_to_points(void* stream, int64_t n, const int64_t* morton, int16_t* points);
int kamd_spc_points_to_corners(void* stream, int64_t n, const int16_t* points, int16_t* corners);
size_t kamd_spc_octree_workspace(int64_t n, int level);
int kamd_spc_octree_build(void* stream, int64_t n, int level, const int64_t* morton, int sorted, void* workspace,
                          size_t workspace_bytes, int64_t* host_sizes);
int kamd_spc_octree_gather(void* stream, int64_t n, int level, const void* workspace, int64_t octree_bytes, uint8_t* octree);
size_t kamd_spc_scan_workspace(int64_t total_bytes, int64_t B);
int kamd_spc_scan_octrees(void* stream, int64_t total_bytes, int64_t B, const uint8_t* octrees, const int64_t* starts,
                          int32_t* exsum, void* workspace, int32_t* host_pyramids);
int kamd_spc_generate_points(void* stream, int64_t B, int max_level, int64_t num_bytes, int64_t num_points,
                             const uint8_t* octrees, const int32_t* exsum, const int64_t* meta, int64_t max_level_nodes,
                             int16_t* points);
int kamd_spc_query_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const void* coords, int64_t* pidx);
int kamd_spc_query_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const float* coords, int64_t* pidx);
int kamd_spc_query_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const int32_t* exsum,
                       const double* coords, int64_t* pidx);
int kamd_spc_query_multiscale_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const void* coords, int64_t* pidx);
int kamd_spc_query_multiscale_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const float* coords, int64_t* pidx);
int kamd_spc_query_multiscale_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree,
                                  const int32_t* exsum, const double* coords, int64_t* pidx);
int kamd_spc_to_dense_forward_f32(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                  const int16_t* points, const int64_t* meta, const float* features, float* grid);
int kamd_spc_to_dense_forward_f64(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                  const int16_t* points, const int64_t* meta, const double* features, double* grid);
int kamd_spc_to_dense_backward_f32(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                   const int16_t* points, const int64_t* meta, const float* grad_grid, float* grad_features);
int kamd_spc_to_dense_backward_f64(void* stream, int64_t B, int64_t C, int level, int64_t rows, int64_t num_points,
                                   const int16_t* points, const int64_t* meta, const double* grad_grid, double* grad_features);

/* ------------------------------------------------------------------------- */
/* ops.spc feature grids: dual octree, trinkets, trilinear interpolation     */
/* (reference: kaolin/ops/spc/spc.py make_dual / make_trinkets, points.py    */
/* InterpolateTrilinear, point_utils_cuda.cu; csrc/spc_trilinear.hip).       */
/*   dual_build: points = ONE point hierarchy (num_points rows), host_first  */
/*     (HOST, max_level + 2 int64) = row 1 of its pyramid.  One key          */
/*     level << 48 | Morton(corner) per (point, corner), ONE radix sort over */
/*     the 3 (max_level + 1) code bits and the level bits, heads + scan, and */
/*     the one host read: host_starts (HOST, max_level + 2 int64) = row 1 of */
/*     the dual pyramid; the call synchronises the stream.  dual_emit then   */
/*     writes the num_dual = host_starts[max_level + 1] int16 rows from the  */
/*     same workspace (kamd_spc_dual_workspace bytes).  max_level <= 14: a   */
/*     corner of level l reaches 2^l.                                        */
/*   trinkets: (num_points, 8) int32, the index of every corner in its level */
/*     of the dual, relative to the level; parents (num_points) int32, the   */
/*     absolute index of point >> 1, -1 for the root.  host_first /          */
/*     host_first_dual: row 1 of the two pyramids (HOST).  One launch, no    */
/*     host read; a corner or parent that is not found is -1.                */
/*   trilinear_coeffs: coords (n,3) in [-1,1], points (n,3) -> (n,8), corner */
/*     order c000, c001, ... (z fastest).                                    */
/*   interpolate: coords (N,S,3) float32, pidx (N) int32 (-1 = miss), points */
/*     (num_points,3), trinkets (num_points,8), feats (num_feats,D) -> out   */
/*     (N,S,D).  backward_feats accumulates with float atomics into a buffer */
/*     it zeroes first (f16: `sums` is a float buffer of num_feats * D,      */
/*     rounded once into grad_feats); backward_coords writes the derivative  */
/*     by the LOCAL cell coordinate, (N,S,3) float32.  One launch each (two  */
/*     and three with the fill and the rounding); no host read: capturable.  */
/*     A pidx outside [0, num_points) or a trinket outside [0, num_feats) is */
/*     a miss: zeros, no access.  trinkets must be 16-byte aligned.          */
/* ------------------------------------------------------------------------- */
size_t kamd_spc_dual_workspace(int64_t num_points, int max_level);
int kamd_spc_dual_build(void* stream, int64_t num_points, int max_level, const int16_t* points, const int64_t* host_first,
                        void* workspace, size_t workspace_bytes, int64_t* host_starts);
int kamd_spc_dual_emit(void* stream, int64_t num_points, int max_level, const void* workspace, int64_t num_dual,
                       int16_t* points_dual);
int kamd_spc_trinkets(void* stream, int64_t num_points, int64_t num_dual, int max_level, const int16_t* points,
                      const int16_t* points_dual, const int64_t* host_first, const int64_t* host_first_dual, int32_t* trinkets,
                      int32_t* parents);
int kamd_spc_trilinear_coeffs_f16(void* stream, int64_t n, int level, const void* coords, const int16_t* points, void* coeffs);
int kamd_spc_trilinear_coeffs_f32(void* stream, int64_t n, int level, const float* coords, const int16_t* points, float* coeffs);
int kamd_spc_trilinear_coeffs_f64(void* stream, int64_t n, int level, const double* coords, const int16_t* points, double* coeffs);
int kamd_spc_interpolate_forward_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const void* feats, void* out);
int kamd_spc_interpolate_forward_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const float* feats, float* out);
int kamd_spc_interpolate_forward_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                     const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                     const double* feats, double* out);
int kamd_spc_interpolate_backward_feats_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                            const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                            const void* grad_out, float* sums, void* grad_feats);
int kamd_spc_interpolate_backward_feats_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                            const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                            const float* grad_out, float* grad_feats);
int kamd_spc_interpolate_backward_feats_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                            const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                            const double* grad_out, double* grad_feats);
int kamd_spc_interpolate_backward_coords_f16(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                             const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                             const void* feats, const void* grad_out, float* grad_coords);
int kamd_spc_interpolate_backward_coords_f32(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                             const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                             const float* feats, const float* grad_out, float* grad_coords);
int kamd_spc_interpolate_backward_coords_f64(void* stream, int64_t N, int64_t S, int64_t D, int level, int64_t num_points, int64_t num_feats,
                                             const float* coords, const int32_t* pidx, const int16_t* points, const int32_t* trinkets,
                                             const double* feats, const double* grad_out, float* grad_coords);

/* ------------------------------------------------------------------------- */
/* ops.spc sparse convolutions (reference: kaolin/csrc/ops/spc/convolution*    */
/* and minkowski_conv.cu; csrc/spc_conv.hip).  The whole batch at once, no     */
/* host read, no atomics: bit-identical from run to run.                       */
/*   conv_map: map (K, n) int32, map[k][i] = the packed row, among the         */
/*     num_targets points of the target level of the batch, of the neighbour   */
/*     of row i under kernel_vectors[k] ((K, 3) int16), or -1.  The n rows are */
/*     the points of `row_level` of the B items.  transposed == 0: the target  */
/*     level is row_level + jump and the neighbour of p is (p << jump) + v;    */
/*     else it is row_level - jump and the neighbour is (p - v) >> jump, where */
/*     p - v >= 0 in every component and divisible by 2^jump.  A neighbour     */
/*     outside the grid is a miss.  meta (device, int64): the B + 1 prefix of  */
/*     the rows per item, then 6 per item: first octree byte, octree bytes,    */
/*     index in `points` of its first row point, index in ITS hierarchy of its */
/*     first target point, its target points, packed row of its first target.  */
/*     One thread per (k, row) walks the item's octree (exsum in the current   */
/*     layout).  K <= 65535, K * n < 2^31.  One launch.                        */
/*   conv_gather: Y (n, N) = sum_k A[map[k][i]] . W[k], A (a_rows, C), W       */
/*     (K, C, N); transpose_w != 0: W is (K, N, C) and W[k]^T is used.  Misses */
/*     and entries >= a_rows contribute nothing (the row is never fetched).    */
/*     Every element of Y is stored exactly once.  One launch.                 */
/*   conv_wgrad: grad_weight (K, cin, cout) = sum over the rows j with a       */
/*     neighbour of X[j]^T . G[map[k][j]], X (n, cin), G (g_rows, cout): one   */
/*     partial per (k, row slice) in the workspace                             */
/*     (kamd_spc_conv_workspace(K, cin, cout, sizeof(T)) bytes, host only),    */
/*     then the slices summed in index order.  Two launches.                   */
/* ------------------------------------------------------------------------- */
int kamd_spc_conv_map(void* stream, int transposed, int64_t B, int64_t K, int64_t n, int row_level, int jump, int64_t num_bytes,
                      int64_t num_points, int64_t num_targets, const uint8_t* octrees, const int32_t* exsum, const int16_t* points,
                      const int16_t* kernel_vectors, const int64_t* meta, int32_t* map);
int kamd_spc_conv_gather_f32(void* stream, int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w,
                             const int32_t* map, const float* A, const float* W, float* Y);
int kamd_spc_conv_gather_f64(void* stream, int64_t n, int64_t K, int64_t a_rows, int64_t C, int64_t N, int transpose_w,
                             const int32_t* map, const double* A, const double* W, double* Y);
size_t kamd_spc_conv_workspace(int64_t K, int64_t cin, int64_t cout, int elem_bytes);
int kamd_spc_conv_wgrad_f32(void* stream, int64_t n, int64_t K, int64_t g_rows, int64_t cin, int64_t cout, const int32_t* map,
                            const float* X, const float* G, void* workspace, size_t workspace_bytes, float* grad_weight);
int kamd_spc_conv_wgrad_f64(void* stream, int64_t n, int64_t K, int64_t g_rows, int64_t cin, int64_t cout, const int32_t* map,
                            const double* X, const double* G, void* workspace, size_t workspace_bytes, double* grad_weight);

/* ------------------------------------------------------------------------- */
/* render.spc: octree ray tracing and the packed ray operators (reference:     */
/* kaolin/csrc/render/spc; csrc/spc_raytrace.hip).                             */
/*   raytrace: N rays (origin, direction (N,3) float32) through ONE octree     */
/*     (num_bytes bytes, exsum in the current layout, points = its hierarchy,  */
/*     num_points rows) down to `level` <= 15.  One thread per ray walks its   */
/*     subtree depth-first; the result is the sequence of the reference's      */
/*     level-by-level expansion: rays in input order, a ray's hits front to    */
/*     back.  raytrace_count: the count walk, the scan of the counts, and the  */
/*     one host read -- *host_total (HOST memory) = the number of hits; the    */
/*     call synchronises the stream.  with_exit != 0: a hit also needs an exit */
/*     depth > 0.  raytrace_emit (same arguments, the same workspace           */
/*     untouched in between, total = *host_total): repeats the walk and writes */
/*     nuggets (total, 2) int32 = (ray, point) and, depth_mode 1, depths       */
/*     (total) float32 = entry, depth_mode 2, depths (total, 2) = entry, exit  */
/*     (count must have run with with_exit != 0 exactly when depth_mode == 2). */
/*     4 launches in all, whatever `level`.  workspace:                        */
/*     kamd_spc_raytrace_workspace(N) bytes.  1 <= N < 2^31.  A node index is  */
/*     compared with num_points, a byte index with num_bytes, an output row    */
/*     with total: a failed comparison ends that branch / skips that write.    */
/*   pack_scan: feats (n, C), boundaries (n) bytes (non-zero = the element     */
/*     starts a pack; element 0 always does) -> out (n, C): the cumulative sum */
/*     (prod != 0: product) inside every pack, sequentially in index order     */
/*     (reverse: from the pack's end) in T; exclusive: the identity first.     */
/*     One launch, no host read, no allocation: capturable.                    */
/*   pack_reduce: inclusive_sum (n) int32 = the inclusive sum of boundaries    */
/*     (element i belongs to pack inclusive_sum[i] - 1) -> out (num_packs, C), */
/*     each row accumulated from the pack's first element on in index order:   */
/*     no atomics, bit-identical run to run.  Rows no pack names are left      */
/*     untouched.  One launch.                                                 */
/* ------------------------------------------------------------------------- */
size_t kamd_spc_raytrace_workspace(int64_t N);
int kamd_spc_raytrace_count(void* stream, int64_t N, int level, int64_t num_bytes, int64_t num_points, const uint8_t* octree,
                            const int32_t* exsum, const int16_t* points, const float* origin, const float* direction, int with_exit,
                            void* workspace, int64_t* host_total);
int kamd_spc_raytrace_emit(void* stream, int64_t N, int level, int64_t num_bytes, int64_t num_points, const uint8_t* octree,
                           const int32_t* exsum, const int16_t* points, const float* origin, const float* direction, int depth_mode,
                           const void* workspace, int64_t total, int32_t* nuggets, float* depths);
int kamd_spc_pack_scan_f32(void* stream, int64_t n, int64_t C, const float* feats, const uint8_t* boundaries, int prod, int exclusive,
                           int reverse, float* out);
int kamd_spc_pack_scan_f64(void* stream, int64_t n, int64_t C, const double* feats, const uint8_t* boundaries, int prod,
                           int exclusive, int reverse, double* out);
int kamd_spc_pack_reduce_f32(void* stream, int64_t n, int64_t C, int64_t num_packs, const float* feats, const int32_t* inclusive_sum,
                             int prod, float* out);
int kamd_spc_pack_reduce_f64(void* stream, int64_t n, int64_t C, int64_t num_packs, const double* feats,
                             const int32_t* inclusive_sum, int prod, double* out);

/* ------------------------------------------------------------------------- */
/* ops.spc Bayesian-fusion reconstruction (csrc/spc_bf.hip): the operators of  */
/* the reference's bf.cpp / recon.cpp, the empty-aware query of query.cpp, and */
/* bf_cells (no reference counterpart).  One thread per point, node or pixel;  */
/* no atomics.  float32 arithmetic, one rounding per operation, no FMA,        */
/* correctly rounded divide and square root (DESIGN.md has the contract).      */
/*   T16: the 16 floats (host memory, row major) of T = M * cam.               */
/*   mip: (mip_size, 2) floats, coarsest level first; level l starts at        */
/*     (h >> L)(w >> L)(4^l - 1) / 3.  h and w are multiples of 2^L.            */
/*   build_mip2d with true_depth converts depth IN PLACE (pixels equal to      */
/*     max_depth stay).  L launches.                                           */
/*   oracle / oracle_final: level 0 answers occupancy 1, state 2.              */
/*   inclusive_sum: workspace of kamd_spc_bf_scan_workspace(n) bytes.          */
/*   subdivide / compactify / compactify_nodes: pass = the scan's last entry,  */
/*     read by the caller; a slot outside [0, pass) is skipped.                */
/*   process_final_voxels: the pointers are those of the tail to write;        */
/*     nvsum entries are compared with prev_size.                              */
/*   merge / merge_empty / query: the walk compares every node index with      */
/*     num_bytes (octree, empty and exsum have num_bytes entries each) and a   */
/*     row of probs / colors with rows; a failed comparison answers empty.     */
/*   query: >= 0 the point index, -1 empty or outside, -2 - depth unseen.      */
/*   cells_count: every cell of `level` that query does not answer with -1 is  */
/*     counted (level + 3 launches); host2 = {K, bytes the levels account      */
/*     for}: the one host read.  cells_emit: the K cells (K, 3) int16 in       */
/*     ascending Morton order, one thread per cell, from the same workspace    */
/*     (kamd_spc_bf_cells_workspace(num_bytes) bytes).                         */
/* ------------------------------------------------------------------------- */
int64_t kamd_spc_bf_mip_size(int h, int w, int mip_levels);
int kamd_spc_bf_build_mip2d(void* stream, int h, int w, int mip_levels, float fx, float fy, float cx, float cy, float max_depth,
                            int true_depth, float* depth, float* mip);
int kamd_spc_bf_oracle(void* stream, int64_t n, const int16_t* points, int level, const float* T16, float sigma, const float* depth,
                       int h, int w, int mip_levels, const float* mip, int32_t* occupancy, int32_t* state);
int kamd_spc_bf_oracle_final(void* stream, int64_t n, const int16_t* points, int level, const float* T16, float sigma,
                             const float* depth, int h, int w, int32_t* occupancy, int32_t* state, float* probabilities);
int kamd_spc_bf_colors_final(void* stream, int64_t n, const int16_t* points, const float* T16, float sigma, const float* image,
                             const float* depth, int h, int w, const float* probabilities, uint8_t* colors, float* normals);
size_t kamd_spc_bf_scan_workspace(int64_t n);
int kamd_spc_bf_inclusive_sum(void* stream, int64_t n, const int32_t* in, int32_t* out, void* workspace);
int kamd_spc_bf_subdivide(void* stream, int64_t n, int64_t pass, const int16_t* points, const int32_t* insum, int16_t* new_points,
                          int32_t* nvsum);
int kamd_spc_bf_compactify(void* stream, int64_t n, int64_t pass, const int16_t* points, const int32_t* insum, int16_t* new_points,
                           int64_t* nvsum);
int kamd_spc_bf_process_final_voxels(void* stream, int64_t num_nodes, const int32_t* state, const int32_t* nvsum, int64_t prev_size,
                                     int32_t* occupancies, int32_t* prev_state, uint8_t* octree, uint8_t* empty);
int kamd_spc_bf_compactify_nodes(void* stream, int64_t n, int64_t pass, const int32_t* insum, const uint8_t* octree, const uint8_t* empty,
                                 uint8_t* new_octree, uint8_t* new_empty);
int kamd_spc_bf_merge_empty(void* stream, int64_t n, const int16_t* points, int level, int64_t num_bytes0, int64_t num_bytes1,
                            const uint8_t* octree0, const uint8_t* octree1, const uint8_t* empty0, const uint8_t* empty1,
                            const int32_t* exsum0, const int32_t* exsum1, int32_t* occupancy, int32_t* state);
int kamd_spc_bf_merge(void* stream, int64_t n, const int16_t* points, int level, int64_t num_bytes0, int64_t num_bytes1,
                      const uint8_t* octree0, const uint8_t* octree1, const uint8_t* empty0, const uint8_t* empty1, const int32_t* exsum0,
                      const int32_t* exsum1, int64_t offset0, int64_t offset1, int64_t rows0, int64_t rows1, const float* probs0,
                      const float* probs1, const uint8_t* colors0, const uint8_t* colors1, int32_t* occupancy, int32_t* state,
                      float* probabilities, uint8_t* colors);
int kamd_spc_bf_query_f16(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const void* coords, int32_t* out);
int kamd_spc_bf_query_f32(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const float* coords, int32_t* out);
int kamd_spc_bf_query_f64(void* stream, int64_t Q, int level, int64_t num_bytes, const uint8_t* octree, const uint8_t* empty,
                          const int32_t* exsum, const double* coords, int32_t* out);
size_t kamd_spc_bf_cells_workspace(int64_t num_bytes);
int kamd_spc_bf_cells_count(void* stream, int64_t num_bytes, int level, const uint8_t* octree, const uint8_t* empty, void* workspace,
                            int64_t* host2);
int kamd_spc_bf_cells_emit(void* stream, int64_t num_bytes, int level, const uint8_t* octree, const uint8_t* empty, const void* workspace,
                           int64_t K, int16_t* cells);

/* ------------------------------------------------------------------------- */
/* ops.conversions.pointcloud (csrc/pointcloud.hip; the reference's versions   */
/* are pure PyTorch, these entry points exist only on our side).               */
/* unbatched_pointcloud_to_spc, in this order:                                 */
/*   spc_build_*: n points (f32 / f64 with element strides, quantised as       */
/*     ops.spc.quantize_points does; i16: (n, 3) contiguous, quantised by the  */
/*     caller) -> (Morton key, index) pairs, the stable pair sort on 3 * level */
/*     bits, run heads, scan, run starts, then kamd_spc_octree_build on the    */
/*     sorted keys.  host_sizes (1 + level): unique cells U, then the nodes of */
/*     every level -- the ONE host read; the call synchronises the stream.     */
/*     workspace: kamd_pointcloud_spc_workspace(n, level) bytes, kept for the  */
/*     next two calls.                                                         */
/*   spc_octree: the sum(host_sizes[1:]) bytes of the octree.                  */
/*   spc_mean: features (n, D) with element strides, dtype 0..8 = bool, u8,    */
/*     i8, i16, i32, i64, f16, f32, f64 -> out (U, D) contiguous, row r = the  */
/*     mean of the r-th cell in Morton order: double sums in a fixed order     */
/*     (pointcloud.hip states it), one division, rint for the integer types,   */
/*     one cast.  No atomics.  mean_workspace:                                 */
/*     kamd_pointcloud_spc_mean_workspace(n, D) bytes.  Two launches.          */
/* voxelgrids_*: points (B, P, 3), origin (B, 3), scale (B) contiguous; mult = */
/*   R - 1 rounded to the dtype.  sparse == 0: out = (B, R, R, R) grid of the  */
/*   dtype, zeroed here, 1 where round_half_even(((p - origin) / scale) mult)  */
/*   lies in [0, R - 1]^3, every operation rounded in the dtype.  sparse != 0: */
/*   out = (B, ceil(R^3 / 32)) 32-bit words, zeroed here, bit (lin & 31) of    */
/*   word lin / 32 for the voxel lin = (x R + y) R + z.  One launch.           */
/* ------------------------------------------------------------------------- */
size_t kamd_pointcloud_spc_workspace(int64_t n, int level);
int kamd_pointcloud_spc_build_f32(void* stream, int64_t n, int level, const float* points, int64_t stride_n, int64_t stride_c,
                                  void* workspace, size_t workspace_bytes, int64_t* host_sizes);
int kamd_pointcloud_spc_build_f64(void* stream, int64_t n, int level, const double* points, int64_t stride_n, int64_t stride_c,
                                  void* workspace, size_t workspace_bytes, int64_t* host_sizes);
int kamd_pointcloud_spc_build_i16(void* stream, int64_t n, int level, const int16_t* points, void* workspace, size_t workspace_bytes,
                                  int64_t* host_sizes);
int kamd_pointcloud_spc_octree(void* stream, int64_t n, int level, const void* workspace, int64_t octree_bytes, uint8_t* octree);
size_t kamd_pointcloud_spc_mean_workspace(int64_t n, int64_t D);
int kamd_pointcloud_spc_mean(void* stream, int dtype, int64_t n, int level, int64_t U, int64_t D, const void* features,
                             int64_t stride_n, int64_t stride_d, const void* workspace, void* mean_workspace, void* out);
int kamd_pointcloud_voxelgrids_f16(void* stream, int64_t B, int64_t P, int R, double mult, const void* points, const void* origin,
                                   const void* scale, int sparse, void* out);
int kamd_pointcloud_voxelgrids_f32(void* stream, int64_t B, int64_t P, int R, double mult, const float* points,
                                   const float* origin, const float* scale, int sparse, void* out);
int kamd_pointcloud_voxelgrids_f64(void* stream, int64_t B, int64_t P, int R, double mult, const double* points,
                                   const double* origin, const double* scale, int sparse, void* out);

/* ------------------------------------------------------------------------- */
/* ops.mesh per-vertex sums / means of per-face-corner features               */
/* (csrc/vertex_features.hip: average_face_vertex_features,                    */
/* compute_vertex_normals, the sum of vertex_tangents; the reference uses      */
/* scatter_add_, these entry points exist only on our side).                   */
/* faces: (F, K) int32 (faces_bytes 4) or int64 (8) with element strides; V    */
/* vertices; F, K, V >= 1, F K < 2^31 - 1, V < 2^31 - 1.                       */
/* corners_build: offsets (V + 1) and corners (K F) int32: corners[offsets[v]  */
/*   .. offsets[v + 1]) = the corners i = k F + f with faces[f, k] == v in     */
/*   ascending i (the stable keys-only sort over the low ceil(log2 V) bits of  */
/*   (i << 32) | v, a binary search per offset).  *host_bad = the number of    */
/*   ids outside [0, V) (they are filed under vertex 0: the caller raises) --  */
/*   the ONE host read; the call synchronises the stream.  workspace:          */
/*   kamd_vertex_corners_workspace(F, K, V) bytes (0: extents out of range).   */
/* gather_*: face_features (B, F, K, N) with element strides (0 allowed) ->    */
/*   out (B, V, N) contiguous: per (b, v, n) the sum over the vertex's corners */
/*   in list order, one rounded addition per corner from +0; mean != 0: one    */
/*   division by max(count, 1).  One launch, no atomics, no host read.         */
/* gather_backward_*: grad_out (B, V, N) with element strides -> grad          */
/*   (B, F, K, N) contiguous, grad[b, f, k, :] = grad_out[b, faces[f, k], :]   */
/*   (mean != 0: / max(count, 1), count = offsets[v + 1] - offsets[v]); an id  */
/*   outside [0, V) takes 0.  One launch.                                      */
/* ------------------------------------------------------------------------- */
size_t kamd_vertex_corners_workspace(int64_t F, int64_t K, int64_t V);
int kamd_vertex_corners_build(void* stream, int64_t F, int64_t K, int64_t V, const void* faces, int faces_bytes, int64_t stride_f,
                              int64_t stride_k, void* workspace, size_t workspace_bytes, int32_t* offsets, int32_t* corners,
                              int32_t* host_bad);
int kamd_vertex_gather_f32(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const float* face_features,
                           int64_t stride_b, int64_t stride_f, int64_t stride_k, int64_t stride_n, const int32_t* offsets,
                           const int32_t* corners, int mean, float* out);
int kamd_vertex_gather_f64(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const double* face_features,
                           int64_t stride_b, int64_t stride_f, int64_t stride_k, int64_t stride_n, const int32_t* offsets,
                           const int32_t* corners, int mean, double* out);
int kamd_vertex_gather_backward_f32(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const float* grad_out,
                                    int64_t stride_b, int64_t stride_v, int64_t stride_n, const void* faces, int faces_bytes,
                                    int64_t faces_stride_f, int64_t faces_stride_k, const int32_t* offsets, int mean, float* grad);
int kamd_vertex_gather_backward_f64(void* stream, int64_t B, int64_t F, int64_t K, int64_t V, int64_t N, const double* grad_out,
                                    int64_t stride_b, int64_t stride_v, int64_t stride_n, const void* faces, int faces_bytes,
                                    int64_t faces_stride_f, int64_t faces_stride_k, const int32_t* offsets, int mean, double* grad);

/* ------------------------------------------------------------------------- */
/* ops.mesh face_areas / sample_points (csrc/sample_points.hip; the reference  */
/* is pure torch, kaolin/ops/mesh/trianglemesh.py:30-311: these entry points   */
/* exist only on our side).  faces: int64 with element strides.  Items:        */
/* items == NULL (batched): item b is the F faces, vertices b of (B, V, 3)     */
/*   with element strides, areas / cdf row b of (B, F);                        */
/* items = B rows (face_begin, face_end, vertex_base) of int64 on the device   */
/*   (packed): item b is faces [face_begin, face_end) of the F packed faces,   */
/*   ids counted from vertex_base in the V packed vertices (vs_b unused),      */
/*   areas / cdf (F).  A face range is clipped to [0, F); a vertex id (+ base) */
/*   outside [0, V) gives NaN and takes no gradient.                           */
/* face_areas_*: one thread per face, sqrt((a + b) + c) 0.5 of the reference's */
/*   expression, one rounding per operation.  face_areas_backward_*: the       */
/*   per-corner gradient (B F | F, 3, 3) by plain stores (the reference's      */
/*   autograd expression; NaN at a zero-area face), to be summed per vertex by */
/*   kamd_vertex_gather_*.                                                     */
/* sample_cdf_*: cdf = the inclusive float64 sums of every item's areas in a   */
/*   fixed order: 1 launch when max_faces (the largest item) fits one tile of  */
/*   the scan, else 3.  workspace: kamd_sample_cdf_workspace(B, max_faces)     */
/*   bytes (host arithmetic; 0: out of range).                                 */
/* sample_points_*: N samples per item from r (B, N) float64 and uv (B, N, 2), */
/*   contiguous: t = min(r total, nextbelow(total)), the first face with       */
/*   cdf > t (and area > 0), u = sqrt(uv0), w = (1 - u, u (1 - uv1), u uv1),   */
/*   points (B, N, 3) = (w0 v0 + w1 v1) + w2 v2, face_choices (B, N) (packed:  */
/*   merged ids), features (B, N, D) from face_features (B, F, 3, D) with      */
/*   element strides (D = 0: none; batched only).  An item whose total is not  */
/*   positive and finite: NaN, choice face_begin.  One launch, no atomics.     */
/* sample_points_backward_*: one launch; w_k g added with float atomics to     */
/*   grad_vertices (B, V, 3 | V, 3) and grad_face_features (B, F, 3, D), both  */
/*   contiguous and zeroed by the caller, either may be NULL.                  */
/* ------------------------------------------------------------------------- */
int kamd_face_areas_f32(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const float* vertices, int64_t vs_b,
                        int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k, float* areas);
int kamd_face_areas_f64(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const double* vertices, int64_t vs_b,
                        int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k, double* areas);
int kamd_face_areas_backward_f32(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const float* vertices,
                                 int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k,
                                 const float* grad_areas, int64_t gs_b, int64_t gs_f, float* grad_corners);
int kamd_face_areas_backward_f64(void* stream, int64_t B, int64_t F, int64_t V, const int64_t* items, const double* vertices,
                                 int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f, int64_t fs_k,
                                 const double* grad_areas, int64_t gs_b, int64_t gs_f, double* grad_corners);
size_t kamd_sample_cdf_workspace(int64_t B, int64_t F);
int kamd_sample_cdf_f32(void* stream, int64_t B, int64_t F, int64_t max_faces, const int64_t* items, const float* areas, double* cdf,
                        void* workspace, size_t workspace_bytes);
int kamd_sample_cdf_f64(void* stream, int64_t B, int64_t F, int64_t max_faces, const int64_t* items, const double* areas, double* cdf,
                        void* workspace, size_t workspace_bytes);
int kamd_sample_points_f32(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                           const float* vertices, int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f,
                           int64_t fs_k, const void* areas, int areas_bytes, const double* cdf, const double* r, const float* uv,
                           const float* face_features, int64_t ff_b, int64_t ff_f, int64_t ff_k, int64_t ff_d, float* points,
                           int64_t* face_choices, float* features);
int kamd_sample_points_f64(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                           const double* vertices, int64_t vs_b, int64_t vs_v, int64_t vs_c, const int64_t* faces, int64_t fs_f,
                           int64_t fs_k, const void* areas, int areas_bytes, const double* cdf, const double* r, const double* uv,
                           const double* face_features, int64_t ff_b, int64_t ff_f, int64_t ff_k, int64_t ff_d, double* points,
                           int64_t* face_choices, double* features);
int kamd_sample_points_backward_f32(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                                    const int64_t* faces, int64_t fs_f, int64_t fs_k, const double* cdf, const float* uv,
                                    const int64_t* face_choices, const float* grad_points, const float* grad_features,
                                    float* grad_vertices, float* grad_face_features);
int kamd_sample_points_backward_f64(void* stream, int64_t B, int64_t F, int64_t V, int64_t N, int64_t D, const int64_t* items,
                                    const int64_t* faces, int64_t fs_f, int64_t fs_k, const double* cdf, const double* uv,
                                    const int64_t* face_choices, const double* grad_points, const double* grad_features,
                                    double* grad_vertices, double* grad_face_features);

/* ------------------------------------------------------------------------- */
/* ops.gaussians.transform_gaussians / transform_shs                           */
/* (csrc/gaussian_transform.hip; the reference is pure torch, kaolin/ops/      */
/* gaussians/transforms.py: these entry points exist only on our side).  N     */
/* Gaussians; every tensor contiguous.  transform: the first of the matrices,  */
/* transform_stride ELEMENTS apart (0: one matrix shared by all) with rows     */
/* transform_row_stride apart: (N or 1, 4, 4) is stride 16 or 0 and row 4.     */
/* flags: 1 = quaternions are xyzw (else wxyz), 2 = log scales, 4 = the        */
/* rotation is GIVEN: the matrices are R itself, (N or 1, 3, 3) = stride 9 or  */
/* 0 and row 3, and there is no geometry (transform_shs).  Otherwise A =       */
/* matrix[:3, :3], R = A / its column norms.                                   */
/* forward: positions (N,3), orientations (N,4), scales (N,3) and their three  */
/*   outputs are all given or all NULL; sh / new_sh (N, (degree + 1)^2, 3),    */
/*   0 <= degree <= 3, both given or both NULL.                                */
/* backward: every (grad_new_x, grad_x) pair is given or NULL, only the given  */
/*   ones are computed; orientations (the forward's input) is needed for       */
/*   grad_orientations.  No gradient with respect to the transform.            */
/* One launch each, no workspace, no atomics, no host read: capturable, and    */
/* the same bits on every call; the shared and the per-Gaussian transform give */
/* the same bits for the same matrix.  The file states the arithmetic.         */
/* ------------------------------------------------------------------------- */
int kamd_gaussian_transform_forward_f32(void* stream, int64_t N, int degree, int flags, const float* transform, int64_t transform_stride,
                                        int64_t transform_row_stride, const float* positions, const float* orientations,
                                        const float* scales, const float* sh, float* new_positions, float* new_orientations,
                                        float* new_scales, float* new_sh);
int kamd_gaussian_transform_forward_f64(void* stream, int64_t N, int degree, int flags, const double* transform, int64_t transform_stride,
                                        int64_t transform_row_stride, const double* positions, const double* orientations,
                                        const double* scales, const double* sh, double* new_positions, double* new_orientations,
                                        double* new_scales, double* new_sh);
int kamd_gaussian_transform_backward_f32(void* stream, int64_t N, int degree, int flags, const float* transform, int64_t transform_stride,
                                         int64_t transform_row_stride, const float* orientations, const float* grad_new_positions,
                                         const float* grad_new_orientations, const float* grad_new_scales, const float* grad_new_sh,
                                         float* grad_positions, float* grad_orientations, float* grad_scales, float* grad_sh);
int kamd_gaussian_transform_backward_f64(void* stream, int64_t N, int degree, int flags, const double* transform, int64_t transform_stride,
                                         int64_t transform_row_stride, const double* orientations, const double* grad_new_positions,
                                         const double* grad_new_orientations, const double* grad_new_scales, const double* grad_new_sh,
                                         double* grad_positions, double* grad_orientations, double* grad_scales, double* grad_sh);

/* ------------------------------------------------------------------------- */
/* Optional per-kernel timing (HIP events recorded on the launch stream).      */
/* Not part of the reference's interface: used by bench.py for its roofline    */
/* line; off by default.  kamd_profile_read synchronises the pending events.  */
/* ------------------------------------------------------------------------- */
int kamd_profile_enable(int on);
/* id >= 0: only that kernel is timed while profiling is on; -1: every kernel */
int kamd_profile_select(int id);
int kamd_profile_reset(void);
int kamd_profile_num_kernels(void);
const char* kamd_profile_kernel_name(int id);
int kamd_profile_read(int id, double* total_ms, int64_t* launches);

/* Work counters of the exact triangle-distance search (no reference counterpart; bench.py's VALU figure for C5).  While `on`,      */
/* every kamd_triangle_distance_forward_* call that takes the sweep counts its work and SYNCHRONISES to read the counts back;        */
/* out8 (optional) receives the last call's: tiles staged, tile walks (per wavefront), (query, tile) sphere tests, face steps (per   */
/* wavefront of 64 lanes), closest-point evaluations (unbatched_triangle_distance_cuda.cu:237-317, one per lane), sum of tiles       */
/* needed per query, queries needing > 48 tiles, hard queries.  Off by default: the product path counts nothing.                     */
int kamd_triangle_distance_work_counters(int on, unsigned long long* out8);

/* ---- self-test hook (no reference counterpart) ------------------------------------------------------------------ */
/* The 64 x 64 bit transpose of the soft mask's select kernel (csrc/tile_bins.h wave_transpose64: gfx950 lane-swap and DPP      */
/* instructions, no LDS) applied to `n_matrices` matrices of 64 uint64 rows each: out[m][j] = column j of matrix m.  With       */
/* reference != 0 the same through __shfl_xor, the form the fast one replaced.  tests/test_dibr_gpu.py checks both against numpy. */
int kamd_debug_transpose64(void* stream, int n_matrices, const uint64_t* in, uint64_t* out, int reference);

#ifdef __cplusplus
}
#endif
#endif  /* KAOLIN_AMD_H_ */
