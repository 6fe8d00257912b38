/*
 * avl_hip.h -- C ABI of libavl_hip.so: the MI355X (gfx950) implementation of the per-frame hot
 * path of AutonomousVehicleLaboratory/vision_semantic_segmentation.
 *
 * The reference has no FFI layer (it is pure Python); each entry point below names the reference
 * function whose arithmetic it replaces (file:line under the reference root).  The Python shim in
 * vision_semantic_segmentation_amd/ binds these with ctypes and keeps the reference's class and
 * method names; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     asynchronous on it, nothing synchronises, nothing allocates;
 *   - the caller owns every buffer, including scratch; the library keeps no pointer after return
 *     (plan objects excepted: they keep the op list they were given);
 *   - return value: 0 on success, a negative AVL_E_* code otherwise; avl_last_error() then holds
 *     a message for the calling thread.  Nothing throws.
 */
#ifndef AVL_HIP_H
#define AVL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVL_OK 0
#define AVL_E_ARG (-1)      /* bad argument (null pointer, non-positive size, bad enum) */
#define AVL_E_HIP (-2)      /* a HIP runtime call failed                                */
#define AVL_E_UNSUPPORTED (-3)

/* point / grid element types */
#define AVL_F32 0
#define AVL_F64 1
#define AVL_BF16 2
#define AVL_F16 3

/* vote-mask layout (one uint32 per grid cell, 0 between frames):
 *   bit i        (i < 16) : some point of map class i fell into the cell this frame
 *   bit 16 + i            : ... and one of them qualified for the intensity bonus (+2 on channel i) */
#define AVL_MAX_MAP_CLASSES 16

/* ---- library ---------------------------------------------------------------------------- */
const char* avl_version(void);
/* copies the calling thread's last error message into buf (NUL terminated); returns its length */
int avl_last_error(char* buf, int len);

/* ---- a7: SemanticMapping.project_pcd (src/mapping.py:357-389) ---------------------------- */

/* Projection only -- lines :367-383.  Point k's component c (0=x,1=y,2=z,3=intensity) is read at
 * pts + k*point_stride + c*comp_stride (bytes) as `dtype` and widened to double.
 * T (row-major 4x4) = T_origin_to_velodyne of :369, or NULL for pcd_frame_id == "velodyne" (:373).
 * P (row-major 3x4) = Camera.P (src/camera.py:28).
 * out_ixy int32[2][n] = dehomogenize(P Xv).astype(int32) (:375, INT_MIN for nan/inf/overflow),
 * out_mask uint8[n]   = the mask of :378-383.  Either may be NULL. */
int avl_project_points(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                       const double* P_host, const double* T_host, double range_max,
                       int img_w, int img_h, int32_t* out_ixy, uint8_t* out_mask, void* stream);

/* bytes of scratch avl_project_pcd needs for n points */
int64_t avl_project_pcd_scratch_bytes(int n);

/* Whole project_pcd: projection, mask, ORDER-PRESERVING compaction (:385) and label gather (:387).
 * image uint8[img_h][img_w][3].  Outputs have capacity n and leading dimension out_ld (>= n):
 * out_pcd double[4][out_ld] (the ORIGINAL-frame columns of pcd that passed, Q6),
 * out_label uint8[3][out_ld], out_count int32[1] = M. */
int avl_project_pcd(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                    const double* P_host, const double* T_host, double range_max,
                    const uint8_t* image, int img_w, int img_h,
                    double* out_pcd, uint8_t* out_label, int64_t out_ld, int32_t* out_count,
                    void* scratch, void* stream);

/* ---- a8: SemanticMapping.update_map (src/mapping.py:391-444) ------------------------------ */

typedef struct avl_grid {
    void* map;            /* [Hm][Wm][C] of map_dtype (AVL_F64 = the reference's type, or AVL_F32) */
    int map_dtype;
    int Hm, Wm, C;        /* Hm indexes x, Wm indexes y (src/mapping.py:115-116); C <= 16        */
    double off_x, off_y;  /* pcd_origin_offset (:404)                                             */
    double b00, b10;      /* map_boundary[0][0], map_boundary[1][0] (:408)                        */
    double resolution;    /* (:409)                                                               */
    uint32_t* cell_mask;  /* scratch uint32[Hm*Wm]; all zero on entry, all zero again on return   */
    int32_t* touched;     /* scratch int32[touched_cap]: cells first touched this frame           */
    int32_t touched_cap;  /* >= min(n points, Hm*Wm)                                              */
    int32_t* counter;     /* scratch int32[counter_len] (a block of its own); ints [0,4) are zeroed by the
                             calls that use them, ints [4, counter_len) must be zero on entry and are zero
                             again on return (per-list cursors of the partitioned touched lists)      */
    int32_t counter_len;  /* >= 4; >= AVL_COUNTER_INTS enables the partitioned lists of avl_fused_frame   */
} avl_grid;
#define AVL_COUNTER_INTS 256

/* update_map for points that already carry an RGB label (the reference's own signature).
 * pcd double[4][ld] (rows x,y,z,intensity), label uint8[3][ld]; the number of points is m_host,
 * or *m_dev when m_dev != NULL (then m_host is the capacity the launch is sized for).
 * label_colors_host uint8[C][3]; only R and G are compared (Q2).
 * cm_host double[C][C]: column i is added to every cell holding a class-i point, once (Q1).
 * bonus_classes: bit i set => class i gets +2 on channel i when a point with intensity < 2 or > 14
 * is present (:431-437); 0 when MAPPING.PCD.USE_INTENSITY is false. */
int avl_update_map(const avl_grid* g, const double* pcd, const uint8_t* label, int64_t ld,
                   int m_host, const int32_t* m_dev,
                   const uint8_t* label_colors_host, const double* cm_host, uint32_t bonus_classes,
                   void* stream);

/* The two stages of avl_update_map, separately.
 * avl_vote_points: :403-437 up to the `+=` -- every point ORs its vote into cell_mask[cell]; the
 * cells it turned non-zero are listed in g->touched[0 .. g->counter[0]).  (g->map is not touched.)
 * avl_grid_apply: the buffered `+=` (:424,:437) for the listed cells, then clears their masks.
 * rows == NULL: applied to g->map.  rows != NULL: row k of rows ([count][C], rows_dtype) stands for
 * cell touched[k] -- for callers whose grid lives in host memory and who move only touched rows. */
int avl_vote_points(const avl_grid* g, const double* pcd, const uint8_t* label, int64_t ld,
                    int m_host, const int32_t* m_dev, const uint8_t* label_colors_host,
                    uint32_t bonus_classes, void* stream);
int avl_grid_apply(const avl_grid* g, const double* cm_host, void* rows, int rows_dtype, void* stream);

/* ---- a9: one fused frame of SemanticMapping.mapping (src/mapping.py:314-319) --------------- */

/* semantic source kinds */
#define AVL_SRC_RGB 0       /* uint8[src_h][src_w][3] colour image, matched on R,G (the ROS topic)     */
#define AVL_SRC_CLASSMAP 1  /* uint8[src_h][src_w] network class ids + lut: the un-colourised argmax   */

/* project_pcd + update_map without materialising the intermediate point list: every point is
 * projected, its label fetched, its grid cell computed from the ORIGINAL coordinates, and its vote
 * OR-ed into cell_mask; then the touched cells are updated once.  For AVL_SRC_CLASSMAP the source is
 * sampled as cv2.resize(..., (img_w,img_h), INTER_NEAREST) would have enlarged it
 * (vision_semantic_segmentation_node.py:109-110) and lut_host uint32[256] maps a network class to its
 * vote bits (= R,G match of its palette colour against LABEL_COLORS). For AVL_SRC_RGB src_w/src_h must
 * equal img_w/img_h and label_colors_host is used instead of the lut. */
int avl_fused_frame(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride,
                    int64_t comp_stride, const double* P_host, const double* T_host, double range_max,
                    int src_kind, const uint8_t* src, int src_w, int src_h, int img_w, int img_h,
                    const uint32_t* lut_host, const uint8_t* label_colors_host,
                    const double* cm_host, uint32_t bonus_classes, void* stream);

/* The vote / apply path avl_fused_frame takes for a cloud of n points on grid g (host only: looks at sizes and pointer
 * values, never at memory).  AVL_E_ARG for a grid or n that avl_fused_frame refuses.
 *   path  vote mask                         apply                      chosen when
 *   0     32-bit, one touched list          list of touched cells      sparse cloud, byte mask not usable
 *   1     32-bit                            sweep of the whole mask    dense cloud, byte mask not usable
 *   2     byte                              sweep of the byte mask     dense cloud, byte mask usable
 *   3     byte, 64 partitioned lists        the 64 lists               sparse cloud, byte mask usable
 * The byte mask is usable when C + popcount(bonus_classes) <= 8, Hm*Wm % 16 == 0 and cell_mask is 16-byte aligned.
 * Path 3: counter_len >= 132, touched_cap >= 64 x (list capacity of n), n <= 250000 and 2n <= Hm*Wm.  Otherwise a sweep
 * (path 2 or 1) when Hm*Wm % 4 == 0, cell_mask is 16-byte aligned and n * (1024 with the byte mask, else 128) >= Hm*Wm;
 * path 0 when not. */
int avl_fused_frame_path(const avl_grid* g, int n, uint32_t bonus_classes);

/* ---- a9v: several synchronised cameras against one cloud ------------------------------------ */

/* The reference's mapper listens to /camera1/semantic and /camera6/semantic (src/mapping.py:57-58); image_callback picks the
 * calibration by frame_id (:273-276) and looks the cloud and the pose up by the message's stamp (:280-285), so cameras
 * triggered together project the SAME cloud with the SAME pose, once each.  This entry maps n_views such views in one pass:
 * the result equals n_views calls of avl_fused_frame in view order (view v: P_host + 12 v, src_host[v]) on the same cloud --
 * bit for bit, for AVL_F32 and AVL_F64 maps.  A point is loaded, moved by T_host and range-tested (:371,:378) once, and its grid
 * cell (:403-409, from the ORIGINAL coordinates, the same for every camera) is computed once; it is then projected through
 * every view's P (:375, float64, the truncation rules of avl_fused_frame) and that view's label is fetched as avl_fused_frame
 * fetches it.  The 32-bit word of cell_mask holds one vote byte per view (bit i = class i seen, bit C + r = lane bonus of the
 * r-th class of bonus_classes), OR-ed with one atomic per point; each touched cell is then updated once, view 0's votes first,
 * inside a view class i (+= CM[:, i], :424) and then its bonus (+2, :437), rounding to the map type after every addition.
 * Limits: 1 <= n_views <= AVL_MAX_VIEWS, and for n_views >= 2 also C + popcount(bonus_classes) <= 8 (AVL_E_ARG otherwise).
 * Source and image sizes are shared by the views (a batched plan has one size); src_host is a HOST array of n_views device
 * pointers.  n_views == 1 forwards to avl_fused_frame.  The scratch contract of avl_grid holds: cell_mask and counter[4 ..) are
 * all zero on return, so single-view and multi-view calls may alternate on one grid. */
#define AVL_MAX_VIEWS 4
int avl_fused_frame_views(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                          int n_views, const double* P_host /* [n_views][12] */, const double* T_host, double range_max,
                          int src_kind, const uint8_t* const* src_host /* n_views device pointers */,
                          int src_w, int src_h, int img_w, int img_h,
                          const uint32_t* lut_host, const uint8_t* label_colors_host,
                          const double* cm_host, uint32_t bonus_classes, void* stream);

/* The path avl_fused_frame_views takes (host only: sizes and pointer values).  AVL_E_ARG for what the call itself refuses of
 * g, n, n_views and bonus_classes.
 *   n_views == 1: the value of avl_fused_frame_path (0 .. 3).
 *   n_views >= 2:
 *   4     word mask, 64 partitioned lists   the 64 lists               counter_len >= 132, touched_cap >= 64 x (list capacity
 *                                                                      of n), n <= 250000 and 2n <= Hm*Wm
 *   5     word mask                         sweep of the whole mask    everything else (any grid size, any alignment) */
int avl_fused_frame_views_path(const avl_grid* g, int n, int n_views, uint32_t bonus_classes);

/* ---- a9o: occlusion culling -- occluded points do not vote (not in the reference) --------------- */

/* project_pcd keeps every point in front of the vehicle that lands inside the image (:378-383), so a map point behind a parked car
 * or a wall takes the label of what hides it.  The calls below give every view a coarse depth buffer in image space and let a point
 * vote only if it is not clearly behind the nearest point of its image neighbourhood.  THE RULE, for one view with a projection
 * image of img_w x img_h (the size points are projected to, not that of a smaller class map), s = cell_px, R = radius,
 * Wc = ceil(img_w / s), Hc = ceil(img_h / s):
 *   1. candidate: a point that passes the test of :378-383 as avl_fused_frame computes it (0 < v0 < range_max, 0 <= ix < img_w,
 *      0 <= iy < img_h).  Whether it falls on the grid plays no part: an off-grid wall hides what is behind it.
 *   2. depth: p2, the third row of P . v (the divisor of :375); its key q = (float)p2, rounded to nearest.  A candidate whose key
 *      is not finite and > 0 writes nothing to the buffer and is never culled.
 *   3. buffer: depth[cy][cx] = the minimum key over the candidates with cx = ix / s, cy = iy / s, held as the key's bit pattern in
 *      a uint32 (positive floats order as unsigned integers); an empty cell holds 0xFFFFFFFF.
 *   4. m = the minimum of depth over the cells (cx + dx, cy + dy), |dx|, |dy| <= R, clipped to the buffer.
 *   5. a candidate is culled iff (double)q > (double)m * k + abs_tol, k = 1.0 + rel_tol computed once on the host in double, the
 *      product and the sum two separately rounded double operations.  The nearest point of a neighbourhood is never culled.
 *   6. a culled candidate casts no vote in that view; everything else is avl_fused_frame's.
 * The grid after a call equals, bit for bit, what the call without culling does with the cloud from which that view's culled points
 * were removed.  Integer atomics only: the result does not depend on the order of the points.  Every call starts from an empty
 * buffer (it resets depth and culled itself), so calls are independent and may share one scratch. */
typedef struct avl_occlusion {
    int32_t cell_px;       /* s: edge of a depth cell in pixels of the projection image, 1..64                       */
    int32_t radius;        /* R: neighbourhood radius in cells, 0..2                                                 */
    double rel_tol;        /* >= 0                                                                                   */
    double abs_tol;        /* >= 0, in the unit of the depth (metres)                                                */
    uint32_t* depth;       /* scratch uint32[depth_words], 4-byte aligned; any content on entry                      */
    int64_t depth_words;   /* >= avl_occlusion_depth_words(img_w, img_h, cell_px, n_views)                           */
    int32_t* culled;       /* int32[n_views]: receives the number of culled candidates of each view; may be NULL     */
} avl_occlusion;

/* words of depth scratch for n_views views: n_views * Hc * Wc (host only; 0 for sizes the calls refuse) */
int64_t avl_occlusion_depth_words(int img_w, int img_h, int cell_px, int n_views);

/* avl_fused_frame / avl_fused_frame_views with the rule above: a depth pass over the cloud (one atomicMin per candidate and view),
 * then the vote with the cull test, then the same apply.  The path is avl_fused_frame_path's / avl_fused_frame_views_path's for n as
 * passed in, not for the number of survivors.  AVL_E_ARG, before any GPU work, for what the plain calls refuse and for a NULL occl,
 * cell_px outside 1..64, radius outside 0..2, a negative or NaN tolerance, a NULL, too short or misaligned depth scratch. */
int avl_fused_frame_occl(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride,
                         int64_t comp_stride, const double* P_host, const double* T_host, double range_max,
                         int src_kind, const uint8_t* src, int src_w, int src_h, int img_w, int img_h,
                         const uint32_t* lut_host, const uint8_t* label_colors_host,
                         const double* cm_host, uint32_t bonus_classes, const avl_occlusion* occl, void* stream);
int avl_fused_frame_views_occl(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                               int n_views, const double* P_host /* [n_views][12] */, const double* T_host, double range_max,
                               int src_kind, const uint8_t* const* src_host /* n_views device pointers */,
                               int src_w, int src_h, int img_w, int img_h,
                               const uint32_t* lut_host, const uint8_t* label_colors_host,
                               const double* cm_host, uint32_t bonus_classes, const avl_occlusion* occl, void* stream);

/* The rule alone, for 1 <= n_views <= AVL_MAX_VIEWS views of one cloud (points addressed as in avl_project_points): state
 * uint8[n_views][n] = 0 not a candidate of the view, 1 visible, 2 culled; key float[n_views][n] (or NULL) = the candidate's key,
 * 0 for a point that is no candidate.  occl->culled, when given, receives the number of state-2 points per view. */
int avl_occlusion_visibility(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                             const double* P_host /* [n_views][12] */, const double* T_host, double range_max,
                             int img_w, int img_h, const avl_occlusion* occl, uint8_t* state, float* key, void* stream);

/* ---- a9p: points labelled from interpolated logits, with a confidence gate (not in the reference) ---------- */

/* The class-map source gives a point the arg-max of the nearest pixel of the network's low-resolution output.  The reference model
 * predicts more finely: DeepLabV3Plus.forward(x, upsample_pred=True) interpolates the logits bilinearly (align_corners=True) to the
 * input's size and takes the arg-max there (deeplab_v3_plus.py:67-69).  The calls below read a plan's fp32 logits (h x w pixels of K
 * classes, `ld` floats from one pixel to the next) and evaluate that prediction only at the pixels the points project to; they also
 * know how sure the network was there and let a point abstain.  THE RULE, for one candidate point of one view (a candidate is a point
 * that passes the test of :378-383 as avl_fused_frame computes it); every float32 operation below is rounded on its own (no fused
 * multiply-add), which is what NumPy float32 arithmetic does:
 *   1. (ix, iy): the pixel of the img_w x img_h projection image, as avl_fused_frame computes it.
 *   2. (nx, ny): the pixel of the net_w x net_h network-input image that (ix, iy) stands for, by the cv2 INTER_NEAREST index rule of
 *      the class-map source: nx = ix when net_w == img_w, else min((int)floor((double)ix * ((double)net_w / (double)img_w)), net_w - 1);
 *      ny alike.
 *   3. scales, computed once on the host as avl_seg_eval_full_res computes them: sy = net_h > 1 ? (float)(h - 1) / (float)(net_h - 1)
 *      : 0, sx alike.  fy = sy * (float)ny and fx = sx * (float)nx, each rounded; y0 = min((int)fy, h - 1), y1 = y0 + (y0 < h - 1),
 *      ly = fy - (float)y0, hy = 1 - ly; x0, x1, lx, hx alike.
 *   4. z[k] = hy * (hx * a + lx * b) + ly * (hx * c + lx * d) for k = 0 .. K - 1, with a, b, c, d the logits of class k at
 *      (y0, x0), (y0, x1), (y1, x0), (y1, x1): seven operations, seven roundings.
 *   5. top = the first maximal index of z, a NaN counting as maximal (AVL_OP_ARGMAX's rule: k replaces the running best when
 *      z[k] > best, or when z[k] is a NaN and best is not).  margin = z[top] - max(z[k], k != top) in float32; +inf when K = 1.
 *   6. the point votes lut[top] iff !(margin < min_margin); otherwise it abstains: it casts no vote in that view, like a pixel of
 *      label 255.  So min_margin = 0 gates nothing, and a NaN margin (a NaN logit, or inf - inf) votes.
 * Everything else is avl_fused_frame's: the intensity bonus, the vote masks, the apply.  The grid after a call equals, bit for bit, what
 * the class-map call does when fed the net_h x net_w label map of rule 3 - 6 at every pixel (255 where the pixel abstains). */
typedef struct avl_point_logits {
    const float* logits[AVL_MAX_VIEWS]; /* per view: device fp32 [h][w] pixels of `ld` floats, the first K the classes; 4-byte aligned */
    int h, w, K;                        /* logits size; 1 <= K <= 254 (states 254 and 255 are taken)                                   */
    int64_t ld;                         /* floats from one pixel to the next, >= K                                                     */
    int net_h, net_w;                   /* the size the logits are interpolated to: the network's input                               */
    float min_margin;                   /* >= 0; a point whose margin is below it abstains                                             */
    int32_t* abstained;                 /* int32[n_views] or NULL: receives, per view, the abstentions of the call (below)            */
} avl_point_logits;

/* avl_fused_frame / avl_fused_frame_views with the logits as the semantic source, and with `occl` != NULL avl_fused_frame_occl /
 * avl_fused_frame_views_occl's culling between the projection and the rule above (a culled candidate is not evaluated).  lut_host:
 * uint32[256], network class -> vote bits.  The path is avl_fused_frame_path's / avl_fused_frame_views_path's for the same n; the
 * apply and sweep kernels are the plain calls'.  abstained[v] receives the number of view v's candidates that fall on the grid, are
 * not culled and abstain -- the votes the gate withheld; the call resets it itself (one integer atomic per wave that has any).
 * AVL_E_ARG, before any GPU work, for what the plain calls refuse and for a NULL pl, a NULL or misaligned logits pointer of a view in
 * use, K outside 1..254, ld < K, a non-positive size, a NaN or negative min_margin, a misaligned abstained, n_views outside
 * 1..AVL_MAX_VIEWS, and what avl_fused_frame_occl refuses of a non-NULL occl. */
int avl_fused_frame_logits(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                           const double* P_host, const double* T_host, double range_max, const avl_point_logits* pl,
                           int img_w, int img_h, const uint32_t* lut_host, const double* cm_host, uint32_t bonus_classes,
                           const avl_occlusion* occl, void* stream);
int avl_fused_frame_views_logits(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                 int n_views, const double* P_host /* [n_views][12] */, const double* T_host, double range_max,
                                 const avl_point_logits* pl, int img_w, int img_h, const uint32_t* lut_host, const double* cm_host,
                                 uint32_t bonus_classes, const avl_occlusion* occl, void* stream);

/* The rule alone, for 1 <= n_views <= AVL_MAX_VIEWS views of one cloud (points addressed as in avl_project_points), on the grid or
 * not: state uint8[n_views][n] = top for a candidate that votes, 254 for one that abstains, 255 for a point that is no candidate of
 * the view; margin float[n_views][n] (or NULL) = the candidate's margin, 0 where the state is 255.  pl->abstained, when given,
 * receives the number of state-254 points per view. */
int avl_point_labels(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                     const double* P_host /* [n_views][12] */, const double* T_host, double range_max, int img_w, int img_h,
                     const avl_point_logits* pl, uint8_t* state, float* margin, void* stream);

/* ---- a9g: dense ground fill -- cells on the ground plane take the cameras' labels (not in the reference) ---------- */

/* Everything above writes where a LiDAR point fell; beyond 15 - 20 m the rings of a spinning LiDAR lie metres apart and most road
 * cells get no vote in a frame.  The calls below go the other way: every cell of a window of the grid puts its centre on the ground
 * plane, projects it into each camera and takes that pixel's label as one Bayesian update -- one thread per cell, which owns the
 * cell's row of the map: no vote mask, no atomics on the map, no apply pass.  (The reference's own answer for "no depth",
 * update_map_planar, is avl_planar_update: a local map with four fixed anchors and a class test that is never true.)
 * Of the grid only map, map_dtype, Hm, Wm, C, off_*, b00, b10 and resolution are read; cell_mask, touched and counter are never
 * touched and may be NULL.  THE RULE, for every cell (i, j) of the window [x0, x0 + h) x [y0, y0 + w) clipped to the grid; every
 * float64 operation is rounded on its own (no fused multiply-add except where avl_fused_frame has one):
 *   1. point: x = (b00 + ((double)i + 0.5) * resolution) - off_x, y alike with j, b10, off_y: the cell's centre in the grid's frame,
 *      the frame of the clouds mapped onto the grid.  With the plane (a, b, c, d) in that same frame: t = a * x; t = t + b * y;
 *      t = t + d; z = (-t) / c, an IEEE division.
 *   2. candidate and pixel, per view: exactly avl_fused_frame's for the point (x, y, z): v = T_host . (x, y, z, 1) (the point itself
 *      when T_host is NULL), the test 0 < v0 < range_max with the fill's own range_max, then the pixel through that view's P with
 *      the truncation rules of avl_fused_frame and the test 0 <= ix < img_w, 0 <= iy < img_h.  A NaN anywhere makes the cell no
 *      candidate.
 *   3. occlusion, only when occl != NULL: the key q = (float)p2 is valid as in rule 2 of avl_occlusion, and the cell is culled in
 *      that view iff (double)q > (double)m * k + abs_tol, m the minimum of the depth buffer over the candidate's neighbourhood
 *      (rules 4 - 5 of avl_occlusion).  The buffer holds real points only: avl_occlusion_depth fills it from a cloud and the fill
 *      reads it; fill cells never write to it.  A neighbourhood without a real point (m = 0xFFFFFFFF, a NaN as a float) culls
 *      nothing: a comparison with a NaN is false.
 *   4. vote: bits = (the vote bits avl_fused_frame takes from that pixel of the view's source) & class_mask, bit i of class_mask
 *      set meaning that map class i may be filled.  A cell has no intensity, so there is never a lane bonus.  With logits a
 *      candidate whose margin is below min_margin abstains (rules 2 - 6 of avl_point_logits, unchanged).
 *   5. apply, in place, by the cell's own thread: view 0 first; inside a view class i ascending, and for every set bit i
 *      row[c] = (MapT)((double)row[c] + cm_host[c * C + i]) for all c: the sequence avl_fused_frame_views applies to a cell.  Any
 *      C <= AVL_MAX_MAP_CLASSES goes with any n_views <= AVL_MAX_VIEWS (a cell's votes are not packed into a mask word).
 *   6. counts, all optional, each reset by the call itself, one integer atomic per wave that has any: filled[v] = the cells with
 *      non-zero bits in view v; pl->abstained[v] = view v's candidates that are not culled and abstain; occl->culled[v] = view v's
 *      culled candidates.
 * The grid after a call equals, bit for bit and for AVL_F32 and AVL_F64 maps, what avl_fused_frame_views does with the VIRTUAL
 * CLOUD of the window's points of rule 1 (intensity 0, bonus_classes 0, the same range_max, a full class_mask, no occlusion),
 * provided every such point falls into its own cell by :404-411 -- it does on the grids tried (tests/test_ground_fill_cpu.py).  The
 * result does not depend on scheduling.  A cell that a LiDAR point also hit in the same frame gets both updates; a caller who
 * wants the fill to weigh less scales cm_host. */
typedef struct avl_ground_fill {
    int32_t x0, y0, h, w;    /* the window in cells: [x0, x0 + h) along Hm, [y0, y0 + w) along Wm; may hang over the grid's edges */
    double plane[4];         /* a, b, c, d of a x + b y + c z + d = 0 in the grid's frame; finite, c != 0                         */
    double range_max;        /* > 0: the fill's own range along the velodyne x axis                                              */
    uint32_t class_mask;     /* bit i set: map class i may be filled                                                             */
    int32_t* filled;         /* int32[n_views] or NULL: receives, per view, the cells that took a vote                           */
} avl_ground_fill;

/* The fill from byte sources (src_kind, src_host, src_w, src_h, lut_host, label_colors_host as avl_fused_frame_views takes them)
 * and from logits (pl, lut_host as avl_fused_frame_views_logits takes them).  T_host: grid frame -> velodyne, NULL when the grid is
 * in the velodyne frame -- exactly avl_fused_frame's T_host.  occl: NULL, or an avl_occlusion whose depth buffer
 * avl_occlusion_depth has filled for the same n_views, P_host, img_w and img_h.  One kernel launch; a window wholly off the grid (or
 * an empty one) succeeds, resets the counts and launches nothing.  AVL_E_ARG, before any GPU work, for a NULL g, gf or map, a bad
 * grid geometry, n_views outside 1..AVL_MAX_VIEWS, a negative h or w or more than 2^31 - 1 cells, a plane that is not finite or
 * has c == 0, a NaN or non-positive range_max, a misaligned filled, and what the frame calls refuse of P_host, the image size, the
 * sources, cm_host, pl and occl. */
int avl_ground_fill_views(const avl_grid* g, const avl_ground_fill* gf, int n_views, const double* P_host /* [n_views][12] */,
                          const double* T_host, int src_kind, const uint8_t* const* src_host /* n_views device pointers */,
                          int src_w, int src_h, int img_w, int img_h, const uint32_t* lut_host, const uint8_t* label_colors_host,
                          const double* cm_host, const avl_occlusion* occl, void* stream);
int avl_ground_fill_views_logits(const avl_grid* g, const avl_ground_fill* gf, int n_views, const double* P_host /* [n_views][12] */,
                                 const double* T_host, const avl_point_logits* pl, int img_w, int img_h, const uint32_t* lut_host,
                                 const double* cm_host, const avl_occlusion* occl, void* stream);

/* Rules 1 - 3 of avl_occlusion alone (points addressed as in avl_project_points): resets occl->depth and occl->culled, then fills
 * the buffer from the cloud.  After it occl->depth holds, per view, [Hc][Wc] words: the bit pattern of the nearest candidate's key,
 * 0xFFFFFFFF for an empty cell.  An empty cloud leaves every cell empty.  AVL_E_ARG as avl_occlusion_visibility. */
int avl_occlusion_depth(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, int n_views,
                        const double* P_host /* [n_views][12] */, const double* T_host, double range_max, int img_w, int img_h,
                        const avl_occlusion* occl, void* stream);

/* ---- a9h: height-aware mapping -- a ground-height vote gate and an elevation layer (not in the reference) ---------- */

/* update_map projects the cloud onto z = 0 (:403-406): a point 4 m up in a tree canopy votes "vegetation" into the road cell beneath
 * it, and a point on a car roof that took a "road" pixel through label bleed votes "road".  With the ground plane in the grid's
 * frame, the calls below let a class bit vote only while the point's height above the plane lies in that class's band, and
 * accumulate the same points' z per cell as the elevation of the drivable surface.  The two parts are independent.  THE RULE, for a
 * point that in view v is a candidate (:378-383 as avl_fused_frame computes it), falls on the grid, is not culled by occlusion, does
 * not abstain, and whose pixel gave the vote bits b (class bit i, its lane bonus at bit 16 + i); every float64 operation is rounded
 * on its own (no fused multiply-add):
 *   1. height: the plane (a, b, c, d) = plane[0..3] is in the frame of the cloud as passed in, which is the grid's frame; the CALLER
 *      normalises it in float64 to a unit normal with c > 0 (SemanticMapping.height_plane) and the library uses the four numbers as
 *      they are.  t = a * x; u = b * y; t = t + u; u = c * z; t = t + u; h = t + d, with x, y, z the point's coordinates as loaded
 *      (a float32 cloud converted to double): three products and three sums.
 *   2. slack: s = slope * v0, v0 the forward distance of :371/:378 (the first row of T_host . (x, y, z, 1); the point's own x when
 *      T_host is NULL): a plane fitted near the car drifts off a graded road.  For class i: lo_i = min_m[i] - s, hi_i = max_m[i] + s.
 *   3. gate, only when gate != 0: class bit i of b stays iff lo_i <= h && h <= hi_i, both bounds inclusive.  A NaN h removes every
 *      bit; max_m[i] = +inf never removes a bit above, min_m[i] = -inf never one below.  A removed class bit takes its bonus bit
 *      with it.
 *   4. count: gated[v] = the number of such points whose b was non-zero and is zero after rule 3 -- the votes the gate withheld.
 *      The call resets it itself; one integer atomic per wave that has any.
 *   5. elevation, only with a layer (elev_classes != 0 and the four arrays), whether the gate is on or not: a point contributes
 *      once per call, however many views see it, when the union over the call's views of its surviving class bits meets
 *      elev_classes.  q = rint(z / quantum): an IEEE division, then round half to even; a q outside int32 contributes nothing.
 *      Otherwise, at the point's cell: elev_sum += q (int64), elev_cnt += 1, elev_min = min(elev_min, q), elev_max = max(elev_max, q).
 *      The layer persists across calls; an empty cell holds sum 0, cnt 0, min INT32_MAX, max INT32_MIN (avl_elevation_reset).  Only
 *      integer atomics: the layer does not depend on the order of the points.
 *   6. everything else is avl_fused_frame_views's: the masks, the apply (inside a view class i ascending, each followed by its
 *      bonus), the path -- avl_fused_frame_views_path's for n as passed in -- and the scratch contract of avl_grid.  The apply and
 *      sweep kernels are the plain calls'.
 * The grid after a gated call equals, bit for bit, what the plain call does with the cloud from which that view's gated points were
 * removed (for a palette where every pixel gives one class). */
typedef struct avl_height {
    int32_t gate;                        /* 0 = no gate (plane, bounds, slope and gated are not read), 1 = rule 3                */
    double plane[4];                     /* a, b, c, d in the grid's frame; finite, c > 0, normalised by the caller               */
    double min_m[AVL_MAX_MAP_CLASSES];   /* per map class, metres; -inf = unbounded below; never a NaN; min_m[i] <= max_m[i]      */
    double max_m[AVL_MAX_MAP_CLASSES];   /* per map class, metres; +inf = unbounded above                                         */
    double slope;                        /* finite, >= 0: metres of extra tolerance per metre of forward distance                 */
    int32_t* gated;                      /* int32[n_views] or NULL: receives, per view, the votes the gate withheld               */
    uint32_t elev_classes;               /* bit i set: a point voting class i enters the layer; 0 = no layer                      */
    double quantum;                      /* finite, > 0: metres per integer step of the layer                                     */
    int64_t* elev_sum;                   /* [Hm * Wm], 8-byte aligned; all four arrays or none (none = no layer)                  */
    int32_t* elev_cnt;                   /* [Hm * Wm]                                                                             */
    int32_t* elev_min;                   /* [Hm * Wm]                                                                             */
    int32_t* elev_max;                   /* [Hm * Wm]                                                                             */
} avl_height;

/* avl_fused_frame_views with the rule above, for every source and with or without culling: pl == NULL takes the byte source
 * (src_kind, src_host, src_w, src_h, lut_host, label_colors_host as avl_fused_frame_views takes them), pl != NULL the logits (those
 * arguments but lut_host are then not read); occl == NULL means no culling.  n_views == 1 runs the single-view kernel.  AVL_E_ARG,
 * before any GPU work, for what the plain calls refuse (and avl_fused_frame_views_logits / _occl of a non-NULL pl / occl), a NULL ht,
 * a gate other than 0 or 1, and with the gate on a plane that is not finite or has c <= 0, a NaN bound or min_m[i] > max_m[i] for a
 * class i < C, a NaN, infinite or negative slope; a layer with some but not all of its four arrays, with elev_classes or arrays
 * given a quantum that is not finite and > 0 or class bits beyond C; a misaligned gated or layer array. */
int avl_fused_frame_views_height(const avl_grid* g, const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride,
                                 int n_views, const double* P_host /* [n_views][12] */, const double* T_host, double range_max,
                                 int src_kind, const uint8_t* const* src_host /* n_views device pointers */,
                                 int src_w, int src_h, int img_w, int img_h,
                                 const uint32_t* lut_host, const uint8_t* label_colors_host,
                                 const double* cm_host, uint32_t bonus_classes, const avl_point_logits* pl,
                                 const avl_occlusion* occl, const avl_height* ht, void* stream);

/* Rules 1 and 2 alone (points addressed as in avl_project_points), for every point, candidate or not: h double[n] and s double[n],
 * both NaN for a point with a non-finite coordinate.  Of ht only plane and slope are read, whatever gate says.  AVL_E_ARG for a NULL
 * ht, a plane or slope the frame call refuses, a NULL or misaligned h or s. */
int avl_point_heights(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, const double* T_host,
                      const avl_height* ht, double* h, double* s, void* stream);

/* The layer's mean: out[cell] = (float)(((double)sum[cell] / (double)cnt[cell]) * quantum), NaN where cnt[cell] == 0. */
int avl_elevation_mean(const int64_t* sum, const int32_t* cnt, int64_t ncell, double quantum, float* out, void* stream);

/* The four arrays to the empty state of rule 5: sum 0, cnt 0, min INT32_MAX, max INT32_MIN. */
int avl_elevation_reset(int64_t* sum, int32_t* cnt, int32_t* qmin, int32_t* qmax, int64_t ncell, void* stream);

/* a6: colourised full-resolution semantic image from the small argmax map
 * (vision_semantic_segmentation_node.py:102,109-116): nearest upscale + palette LUT.
 * labels uint8[lh][lw]; palette_host uint8[256][3]; out uint8[out_h][out_w][3]. */
int avl_colorize_labels(const uint8_t* labels, int lw, int lh, const uint8_t* palette_host,
                        uint8_t* out, int out_w, int out_h, void* stream);


/* ---- the node's image pre-processing (vision_semantic_segmentation_node.py:83-98) -----------
 * cv2.cvtColor(BGR2RGB) -> cv2.undistort(K, dist) -> cv2.resize(INTER_AREA) by an integer factor, fused.
 * bgr uint8[h][w][3]; K_host double[9] (row-major 3x3) and dist_host double[5] (k1,k2,p1,p2,k3), both NULL to
 * skip the undistortion; rgb_out uint8[h/factor][w/factor][3]. */
int avl_preprocess_image(const uint8_t* bgr, int h, int w, const double* K_host, const double* dist_host, int factor,
                         uint8_t* rgb_out, void* stream);
/* The same with cv2.resize(INTER_AREA) to ANY smaller size out_h x out_w (vision_semantic_segmentation_node.py:92-98 takes every
 * IMAGE_SCALE in (0, 1): width = int(W * scale), height = int(H * scale)): OpenCV's area decimation for a non-integer ratio -- partial first
 * and last source pixels weighted by their overlap, float accumulation row by row, round half to even.  Integer ratios should keep
 * avl_preprocess_image (OpenCV switches to integer box means there; for 2 x 2 it rounds half UP).  Parity unpinned (OpenCV absent). */
int avl_preprocess_image_area(const uint8_t* bgr, int h, int w, const double* K_host, const double* dist_host, int out_h, int out_w,
                              uint8_t* rgb_out, void* stream);

/* The same pre-processing INSIDE the network's first kernel: an AVL_OP_STEM op whose `in2` is set reads the RAW BGR camera
 * frame through `in` and applies BGR->RGB / undistort / INTER_AREA per pixel while it fills its LDS tile (the function
 * avl_preprocess_image applies, so the results are the same bytes), i.e. the RGB network input is never written or re-read.
 * Geometry of such an op: in_h x in_w = the NETWORK input (what avl_preprocess_image would have produced), in2_ld = src_w,
 * in_rows = src_h * src_w of the raw frame; the integer factor is src_w / in_w (in_h == src_h / factor is checked).
 * `in2` points at AVL_STEM_CAMERA_BYTES of DEVICE memory holding the camera model, written by avl_stem_camera_set()
 * (stream-ordered: a plan captured into a hipGraph serves camera1 and camera6 alike; K_host / dist_host as above, both NULL
 * = no undistortion).  Every activation type has such a stem: AVL_BF16 / AVL_F16 with w_layout 1 (the MFMA stem) and AVL_F32 with
 * w_layout 0 (the fp32 stem, same [ky][kx][ci][co] weights and fmaf chain as the plain one); a 16-bit stem with w_layout 0 is refused,
 * as is in_format AVL_IN_F32_CHW.
 * Two forms.  raw_batch = 0: ONE raw frame and one camera block; batch > 1 is refused (AVL_E_UNSUPPORTED).  raw_batch = 1: every image
 * of the batch is a raw frame of the same size with a camera model of its own -- `in` = uint8 [batch][src_h][src_w][3],
 * in_rows = batch * src_h * src_w, in2_ld = src_w, `in2` = batch camera blocks of AVL_STEM_CAMERA_BYTES each, block n for image n;
 * in_h x in_w stays the network input of one image and the integer factor is checked per image.  Image n's result is bit for bit
 * what the one-frame form gives on frame n with camera n; a block of all zeros means no undistortion for that image only, so one
 * batch may mix undistorted and plain views.
 * avl_stem_camera_set writes ONE block at camera_dev, which may be any 4-byte aligned device address: block n of a raw batch is
 * (char*)in2 + n * AVL_STEM_CAMERA_BYTES.  It is stream-ordered in both forms, so a captured plan can get new cameras, for one image
 * or for all, between two replays. */
#define AVL_STEM_CAMERA_BYTES 64
int avl_stem_camera_set(void* camera_dev, const double* K_host, const double* dist_host, void* stream);

/* ---- the semantic point cloud mapping() publishes (src/mapping.py:316-317) ---------------
 * create_point_cloud (src/utils/utils_ros.py:31-59) without its per-point struct.pack loop: record k (16 bytes,
 * point_step 16) = float32 x,y,z of pcd[0:3][k] and uint32 rgba = r | g<<8 | b<<16 | 255<<24 of label[:,k].
 * pcd double[4][ld], label uint8[3][ld] as avl_project_pcd returns them; count = m_host or *m_dev. */
int avl_pack_semantic_cloud(const double* pcd, const uint8_t* label, int64_t ld, int m_host, const int32_t* m_dev,
                            void* out_records, void* stream);

/* ---- the planar (no-LiDAR) mode, update_map_planar (src/mapping.py:465-488) -----------------
 * The semantic image is warped onto the grid by a homography (generate_homography, src/homography.py:22-76:
 * cv2.warpPerspective(image, H, (Wm, Hm)), INTER_LINEAR, zero border), every cell whose warped colour matches class i and
 * whose column is >= sep gets map[cell][i] += 1, then negative cells are clamped to 0 (:481).
 *   Hinv_host double[9]: the INVERSE homography (grid cell (x = column, y = row) -> image pixel), row-major;
 *   match_colour 0: the reference as written -- it compares a uint8 channel with the label NAME (:474), which is never
 *                   true, so nothing is added and only the clamp acts;  1: R,G colour match as in update_map (Q2).
 * OpenCV is absent here: float64 bilinear weights, round half to even (parity unpinned; oracle/planar_oracle.py). */
int avl_planar_update(void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* image, int img_h, int img_w,
                      const double* Hinv_host, int sep, const uint8_t* label_colors_host, int match_colour, void* stream);

/* pcd_callback (src/mapping.py:172-183) without its per-point Python loop: a sensor_msgs/PointCloud2 payload
 * (`data`, n_points records of point_step bytes, FLOAT32 fields x / y / z / intensity at the given byte offsets, all
 * multiples of 4) -> out_xyzi float32[n_points][4], the layout avl_fused_frame reads.  read_points(skip_nans=True)
 * (:179) drops every point with a NaN in ANY of the four fields; here such a point keeps its slot but gets x = NaN, which
 * the projection kernels reject, so frame results are identical and no compaction pass is needed.
 * n_valid (device int32, or NULL) receives the number of points read_points would have yielded. */
int avl_unpack_pointcloud2(const uint8_t* data, int64_t n_points, int point_step, int off_x, int off_y, int off_z, int off_i,
                           float* out_xyzi, int32_t* n_valid, void* stream);

/* ---- end-of-run rendering (src/renderer.py; called at src/mapping.py:332-334) ------------
 * map [Hm][Wm][C] of map_dtype (AVL_F64 | AVL_F32); colors_host uint8[C][3]; out uint8[Hm][Wm][3]. */
/* render_bev_map (renderer.py:32-59): colour of the arg-max channel, black where the channel sum is 0 */
int avl_render_bev_map(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host,
                       uint8_t* out, void* stream);
/* render_bev_map_with_thresholds (renderer.py:131-172); priority_host int32[C] (NULL = 0..C-1, low to high),
 * thresholds_host double[C] (NULL = 0.01 each) */
int avl_render_bev_map_thresholds(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host,
                                  const int32_t* priority_host, const double* thresholds_host, uint8_t* out, void* stream);
/* apply_filter (renderer.py:175-189): 3x3 mean, kernel float32(1/9), BORDER_REFLECT_101; dst != src */
int avl_grid_box_filter(const void* src, void* dst, int map_dtype, int Hm, int Wm, int C, void* stream);

/* ---- live vehicle-centred map: the renderer's remaining functions, fused over a window of the grid ----------------------------
 * The reference publishes its map once, at shutdown (pub_semantic_local_map, src/mapping.py:350); fill_black / resume_color
 * (src/renderer.py:62-105), fill_edge (:192-196, plain slicing in renderer.py) and add_car_to_map (src/mapping.py:490-526)
 * have no caller there.  avl_live_map writes out uint8[h][w][3], the window whose first cell is grid cell (x0, y0); the window
 * may lie partly or wholly outside the grid.  The result is DEFINED as the crop of this chain over the whole grid:
 *   F = avl_grid_box_filter(map) rounded to map_dtype (AVL_LIVE_FILTER; reflect-101 at the GRID's edge), else map;
 *   R = avl_render_bev_map(F), or avl_render_bev_map_thresholds(F, priority_host, thresholds_host) with AVL_LIVE_THRESHOLDS
 *       (priority_host NULL = 0..C-1; thresholds_host is required then);
 *   B = R, or with AVL_LIVE_FILL fill_black(R) as avl_fill_black computes it with colors_host and fill_priority_host
 *       [n_fill_priority], put back into an Hm x Wm frame with a one-cell black ring;
 *   out[i][j] = B[x0 + i][y0 + j] inside the grid, black outside;
 *   then, with car_host != NULL, the ego car: car_host = double[AVL_LIVE_CAR_DOUBLES] {cx, cy, cos yaw, sin yaw, u_lo, u_hi,
 *   v_lo, v_hi} in CELLS (cx, cy = the vehicle's un-truncated grid position).  Pixel (i, j) takes car_color_host (NULL =
 *   255, 0, 0) when, with gx = x0 + i, gy = y0 + j, dx = (gx + 0.5) - cx, dy = (gy + 0.5) - cy, u = c*dx + s*dy,
 *   v = c*dy - s*dx (float64, no contraction): u_lo <= u < u_hi and v_lo <= v < v_hi.  The car goes last: its red has the
 *   lane's R value and fill_black matches on R.  add_car_to_map's dimensions (4.0 m x 1.8 m), reference point (a quarter
 *   length from the rear: u_lo = -L/(4 res), u_hi = 3L/(4 res), v = -+W/(2 res)) and colour are the caller's to pass; its
 *   forward scatter of truncated pixels (holes under rotation, marked untested by its authors) is not reproduced.
 * The grid is only read.  1 <= h, w <= 32768; C <= AVL_MAX_MAP_CLASSES; the filter needs Hm, Wm >= 2, the fill Hm, Wm >= 3. */
#define AVL_LIVE_FILTER 1
#define AVL_LIVE_THRESHOLDS 2
#define AVL_LIVE_FILL 4
#define AVL_LIVE_CAR_DOUBLES 8
int avl_live_map(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, int x0, int y0, int h, int w,
                 int flags, const int32_t* priority_host, const double* thresholds_host, const int32_t* fill_priority_host,
                 int n_fill_priority, const double* car_host, const uint8_t* car_color_host, uint8_t* out, void* stream);
/* avl_live_view: the same picture through a matrix -- rotated, scaled, heading-up -- in one kernel.  The arguments are
 * avl_live_map's with x0, y0 replaced by matrix_host = double[6], the row-major 2 x 3 matrix M from output pixel centres to
 * continuous grid coordinates in cells.  With B the whole-grid picture defined above (F, R, B; Hm x Wm), pixel (i, j) of
 * out uint8[h][w][3] is, in float64, without contraction, in exactly this order:
 *   a  = (double)i + 0.5;  b = (double)j + 0.5;
 *   gx = (M[0][0]*a + M[0][1]*b) + M[0][2];      (grid row coordinate)
 *   gy = (M[1][0]*a + M[1][1]*b) + M[1][2];      (grid column coordinate)
 *   out[i][j] = 0.0 <= gx < (double)Hm && 0.0 <= gy < (double)Wm ? B[floor(gx)][floor(gy)] : black;
 * the range is tested on the doubles, before any conversion to an integer.  Nearest-cell sampling is deliberate: the filter and
 * the hole fill stay defined in the grid's frame.  Then, with car_host != NULL, the car block of avl_live_map is tested on the
 * pixel's continuous coordinates: dx = gx - cx, dy = gy - cy, u = c*dx + s*dy, v = c*dy - s*dx, painted when
 * u_lo <= u < u_hi and v_lo <= v < v_hi.  M = {1, 0, x0, 0, 1, y0} gives avl_live_map(x0, y0) byte for byte, the car included.
 * A heading-up view with the vehicle (cx, cy cells, heading c, s) at pixel centre (ai, aj) and k cells per pixel is
 *   M[0] = {-k*c, k*s, cx - (-k*c)*ai - (k*s)*aj},  M[1] = {-k*s, -k*c, cy - (-k*s)*ai - (-k*c)*aj}:
 * up is +heading, right is the vehicle's right seen from above, (s, -c) in grid (x, y).
 * Every entry of M must be finite, and |M[0][0]| + |M[0][1]| <= AVL_LIVE_VIEW_MAX_SPAN and |M[1][0]| + |M[1][1]| <=
 * AVL_LIVE_VIEW_MAX_SPAN (2.875 exactly; the kernel keeps the grid cells under one 32 x 32 output tile in a fixed array).  A
 * rotation by any angle at k cells per pixel has sums of at most k * sqrt(2), so every k <= 2.875 / sqrt(2) = 2.0329... is
 * admitted at every angle, 0.25 to 2 included; there is no lower limit, and a singular M (a zero 2 x 2 part paints one cell
 * everywhere) is legal.  All arguments are checked before anything touches the device.  The grid is only read. */
#define AVL_LIVE_VIEW_MAX_SPAN 2.875
int avl_live_view(const void* map, int map_dtype, int Hm, int Wm, int C, const uint8_t* colors_host, const double* matrix_host,
                  int h, int w, int flags, const int32_t* priority_host, const double* thresholds_host,
                  const int32_t* fill_priority_host, int n_fill_priority, const double* car_host, const uint8_t* car_color_host,
                  uint8_t* out, void* stream);
/* fill_black (src/renderer.py:62-98) with resume_color (:101-105), reproduced as written: img uint8[X][Y][3] (device) ->
 * out uint8[X-2][Y-2][3].  EVERY interior pixel, black or not (:91 is commented out), looks at the R channel of its 3 x 3
 * neighbourhood; label i is present if a neighbour's R equals colors_host[i][0]; the last present label of priority_host
 * [n_priority] (low to high; the reference's is 0, 3, 4, 2, 1) gives the pixel's R, none present gives 0; resume_color maps
 * that R to the colour of the LAST label with it (black if there is none).  Matching is on R only.  X, Y >= 3;
 * n_colors, n_priority <= AVL_MAX_MAP_CLASSES. */
int avl_fill_black(const uint8_t* img, int X, int Y, const uint8_t* colors_host, int n_colors, const int32_t* priority_host,
                   int n_priority, uint8_t* out, void* stream);
/* End-of-run evaluation (test/test_semantic_mapping.py, called at src/mapping.py:341-344): convert_labels (:6-19) and the
 * counting part of Test.iou (:127-161) in one pass over the rendered colour map.
 *   color_map uint8[H][W][3]; mask uint8[>=H][mask_ld] (0 = invalid) or NULL;
 *   labels_out uint8[H][W] or NULL: 1 road (128,64,128), 2 crosswalk (140,140,200), 3 lane (255,255,255),
 *                                   4 sidewalk (244,35,232), 5 vegetation (107,142,35), 0 anything else / masked;
 *   gt uint8[>=H][gt_ld] or NULL: ground-truth labels (pointer already at the shift_w/shift_h origin of :125-126);
 *   counts uint64[64] (device): counts[g * 8 + l] = pixels with ground truth g (values > 7 counted as 7) and label l.
 * IoU(c) = counts[c][c] / (sum_l counts[c][l] + sum_g counts[g][c] - counts[c][c]) etc. are formed on the host. */
int avl_eval_map(const uint8_t* color_map, int H, int W, const uint8_t* mask, int mask_ld, const uint8_t* gt, int gt_ld,
                 uint8_t* labels_out, unsigned long long* counts, void* stream);

/* ---- full-resolution predictions and validation (DeepLabV3Plus.forward(x, upsample_pred=True), deeplab_v3_plus.py:51,67-69) ----
 * Both read a plan's fp32 logits as the plan leaves them: NHWC [h*w][K], row stride ld (>= K) floats, h x w = the network's output.
 * The source coordinate is AVL_OP_BILINEAR's: src = dst * (in-1)/(out-1), 0 when out = 1 (F.interpolate(..., align_corners=True)). */
/* model(x) for a batch of one: out fp32 [K][H][W] (NCHW planes), K <= 256 (AVL_E_UNSUPPORTED above). */
int avl_upsample_logits(const float* logits, int h, int w, int K, int64_t ld, float* out, int H, int W, void* stream);
/* bytes of scratch avl_seg_eval_full_res needs for its loss at an H x W output (per-workgroup partials) */
int64_t avl_seg_eval_scratch_bytes(int H, int W);
/* The validation step of train.py:138-141 (distributed_train.py:175) for a batch of one, fused: every output pixel interpolates its K
 * logits (never written out), then
 *   labels_out uint8 [H][W] (or NULL): torch.argmax over the classes (AVL_OP_ARGMAX's rule: first maximal index, a NaN is maximal);
 *   confusion uint64 [K][K] (or NULL): MeanIOU.evaluate (models/metrics.py:29-59) -- confusion[gt][pred] += 1 for every pixel with
 *       gt < K (255 and every other value >= K skipped); ACCUMULATES across calls (the caller zeroes it);
 *   loss_out double[2], counts_out uint64[2], scratch (avl_seg_eval_scratch_bytes; the three together, or all NULL):
 *       CrossEntropyLoss(ignore_index) (models/loss.py, models/build.py:20) -- terms logsumexp(z) - z[gt] in fp32 for gt < K and
 *       gt != ignore_index, summed in a fixed order in fp64 (bitwise reproducible): loss_out = {sum, mean (NaN when no pixel counts)},
 *       counts_out = {pixels that contributed, ground-truth values neither < K nor ignore_index (torch's cross_entropy raises on those;
 *       they are skipped here and the caller decides)}.
 * gt uint8 [H][W] is needed by the confusion matrix and the loss.  K <= 64 (AVL_E_UNSUPPORTED above).  Two launches on `stream`. */
int avl_seg_eval_full_res(const float* logits, int h, int w, int K, int64_t ld, int H, int W, const uint8_t* gt, int ignore_index,
                          uint8_t* labels_out, unsigned long long* confusion, double* loss_out, unsigned long long* counts_out,
                          void* scratch, void* stream);
/* The two above for a batch of n images in ONE launch each (two with the loss: eval + finalize); the image index is blockIdx.z.
 * logits: image i starts image_rows rows (of ld floats) after image i-1; image_rows >= h * w, and = h * w for a batched plan's logits
 * buffer.  n >= 1.  gt and labels_out are uint8 [n][H][W], out is fp32 [n][K][H][W]; every size, K and ld are those of ONE image, and
 * the limits are the single-image ones (K <= 256 for the up-sample, K <= 64 for the eval).
 *   out[i], labels_out[i]: bit for bit what avl_upsample_logits / avl_seg_eval_full_res give on image i alone.
 *   confusion uint64 [K][K]: ONE matrix, += the counts of all n images (MeanIOU.evaluate on a batch).
 *   loss: CrossEntropyLoss's reduction='mean' over the BATCH.  The per-workgroup fp64 partials go to a slab [n][groups]; the finalize
 *       kernel sums image i's partials in exactly the single-image order, then adds the n image sums in image order 0 .. n-1 in fp64
 *       (no float atomics; bitwise reproducible).  loss_out = {that sum, sum / contributing pixels of the batch (NaN when there is
 *       none; NOT the mean of the images' means)}, counts_out = {contributing pixels, invalid ground-truth values} of the batch.
 *   image_loss_out double [n][2], image_counts_out uint64 [n][2] (both or neither; they need the loss trio): {sum, mean} and the two
 *       counts per image; image_loss_out[i][0] is bit-identical to loss_out[0] of avl_seg_eval_full_res on image i alone, and
 *       loss_out[0] is their left-to-right fp64 sum.
 *   scratch: avl_seg_eval_scratch_bytes_batch(n, H, W) bytes (= n times the single-image figure).
 * Arguments are checked before anything touches the device. */
int avl_upsample_logits_batch(const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, float* out, int H, int W,
                              void* stream);
int64_t avl_seg_eval_scratch_bytes_batch(int n, int H, int W);
int avl_seg_eval_full_res_batch(const float* logits, int n, int64_t image_rows, int h, int w, int K, int64_t ld, int H, int W,
                                const uint8_t* gt, int ignore_index, uint8_t* labels_out, unsigned long long* confusion, double* loss_out,
                                unsigned long long* counts_out, double* image_loss_out, unsigned long long* image_counts_out,
                                void* scratch, void* stream);

/* ---- semantic extraction: per-class connected components and convex hulls (src/semantic_convex_hull.py:17-91, called from
 * vision_semantic_segmentation_node.py:138-152; csrc/seg_hull.hip) ------------------------------------------------------------
 * maps uint8 [n][h][w] label maps on the device; classes int32[n_classes] on the HOST, each 1 .. 255 (0 is the background, as in the
 * reference, :33-35), n_classes 1 .. 64.  A plane is one (map, class) pair: plane p = image * n_classes + class position, P =
 * n * n_classes <= 65535 planes run in the same launches.  Any h, w >= 1 with h * w < 2^31 - 1, h < 2^20, w < 2^21.
 * Per plane: mask = (label == class) (:36-37); erode != 0: 3x3 erosion (:40-45), pixels outside the image do not erode (cv2.erode's
 * default border; cv2 is absent where this was built, so that border is an assumption, not a pinned fact); erode = 0: the mask is
 * taken as it is.  8-connected components (skimage.measure.label(connectivity=ndim), :51).
 * Everything runs on `stream` without host synchronisation, and results are bit-for-bit reproducible (integers only).
 * Argument errors (a NULL pointer, class 0 or above 255, top_number outside 1 .. 8, h or w below 1) return AVL_E_ARG before
 * anything touches the device.  The library keeps no pointer after a call. */
/* bytes of scratch avl_class_hulls needs (0 for sizes it refuses) */
int64_t avl_hull_scratch_bytes(int h, int w, int planes, int top_number);
/* labels_out int32 [P][h][w]: 0 = background, otherwise 1 + the smallest linear index y * w + x of the pixel's component.  skimage
 * numbers components 1, 2, ... in raster order of their first pixel (unpinned: skimage is absent); these labels have the same order.
 * scratch is not used by this entry point and may be NULL. */
int avl_label_components(const uint8_t* maps, int n, int h, int w, const int32_t* classes, int n_classes, int erode, int32_t* labels_out,
                         void* scratch, void* stream);
/* :59-76 for every plane: the top_number (1 .. 8) largest components ordered by (area descending, label ascending) -- the order of
 * Counter.most_common, which keeps first-seen (raster) order among equal counts -- of which those with area > area_threshold
 * (strict, :60) get a convex hull.  Slot k of plane p:
 *   roots int32 [P][top]      the component's label, 0 = no such component or area <= area_threshold;
 *   areas int32 [P][top]      its pixel count (0 likewise);
 *   n_vertices int32 [P][top] number of hull vertices, 0 for an empty slot;
 *   vertices int32 [P][top][2h+1][2]  (x = column, y = row), strict vertices only (no collinear points), starting at the smallest
 *       (x, then y) and running with positive cross products on (x, y) as stored: counter-clockwise for x right, y up, the lower
 *       chain of a monotone chain first.  cv2.convexHull's start and direction are unpinned (cv2 is absent).
 * drop_first != 0 (the reference): the raster-first pixel of the component -- the one whose index + 1 is the label -- is left out of
 * the hull (crosswalk_pts[1:], :71) though it counts for the area; a component of one pixel then has n_vertices 0.  One or two
 * remaining points, or collinear ones, give 1 or 2 vertices.  scratch: avl_hull_scratch_bytes(h, w, P, top_number) bytes, 8-aligned. */
int avl_class_hulls(const uint8_t* maps, int n, int h, int w, const int32_t* classes, int n_classes, int erode, int top_number,
                    int area_threshold, int drop_first, int32_t* vertices, int32_t* n_vertices, int32_t* areas, int32_t* roots,
                    void* scratch, void* stream);

/* ---- ground plane from the cloud: RANSAC around the reference's plane model (src/plane_3d.py; csrc/seg_plane.hip) ---------------
 * The reference has the model only: Plane3D.fit(data, "min") (plane_3d.py:45-63), normalize (:98-107), eval (:65-80) and
 * distance_to_plane (:82-88); its node receives the plane from another package (vision_semantic_segmentation_node.py:199-201).
 * One call hypothesises, scores, selects and sums the winner's moments on `stream` without host synchronisation; the library keeps
 * no pointer after it.  Integer atomics and fixed-order sums only: two runs give the same bits.
 * Argument errors (a NULL pointer, n < 3 or above 2^27, n_hyp outside 1 .. AVL_PLANE_MAX_HYP, norm not 1 or 2, tolerance <= 0, a bad dtype or
 * stride) return AVL_E_ARG before anything touches the device. */
#define AVL_PLANE_W_NONE 0             /* weight method "none" (plane_3d.py:76-77) */
#define AVL_PLANE_W_XNORM 1            /* weight method "x norm" (plane_3d.py:66-75) */
#define AVL_PLANE_MAX_HYP 1024
#define AVL_PLANE_RESULT_WORDS 24      /* 8-byte words, layout below */
/* bytes of scratch avl_plane_ransac needs (0 for sizes it refuses) */
int64_t avl_plane_scratch_bytes(int n, int n_hyp);
/* Points are addressed as in avl_project_points (f32 or f64, any strides, widened to double); with T_host (row-major 4x4) the fitted
 * frame is Xv = T [x, y, z, 1].  roi_host = xmin, xmax, ymin, ymax, zmin, zmax in the fitted frame (bounds included), or NULL.
 *  1. A point is USED when its three fitted coordinates are finite and inside the roi; the others take no part in anything (a
 *     departure: in the reference one NaN turns np.max of plane_3d.py:74, and with it every weight, into NaN).  For
 *     AVL_PLANE_W_XNORM recip_i = 1 / (|x_i - x0|^norm + 1) (plane_3d.py:67-73) and its maximum over the used points (:74, exact).
 *  2. Hypothesis h = Plane3D.fit of the points triples[h][0..2] (plane_3d.py:47-51) followed by normalize (:99-106), in float64 with
 *     the reference's expressions.  It is invalid -- plane (0, 0, 0, 0), count 0 -- when an index is outside [0, n), a point of the
 *     triple is not used, data[0] == data[1] (:47), s == 0 (:100) or, after normalisation, c < min_c (the cosine of the largest
 *     tilt the caller accepts).
 *  3. count[h] = number of used points with eval < tolerance (plane_3d.py:65-80):
 *     |a x + b y + c z + d| / sqrt(a^2 + b^2 + c^2) * w_i, w_i = recip_i / max recip (AVL_PLANE_W_XNORM) or 1 (AVL_PLANE_W_NONE).
 *  4. best = the hypothesis with the largest count, the lowest index among equals; -1 when every count is 0.
 *  5. Moments of the winner's inliers about p0 = the first point of its triple, delta = p - p0, in float64.
 * planes_out double [n_hyp][4] (32-byte aligned) and counts_out int32 [n_hyp] on the device, either may be NULL.
 * result, on the device, AVL_PLANE_RESULT_WORDS 8-byte words: 0 best (int64), 1 inlier count (int64), 2 used points (int64),
 * 3 valid hypotheses (int64), 4-7 the winner's plane a, b, c, d (double, as all that follow), 8-10 p0, 11 the moments' n,
 * 12-14 sum(delta), 15-20 sum(delta delta^T) as xx, xy, xz, yy, yz, zz, 21-23 zero.  best = -1: words 4-20 are zero.
 * scratch: avl_plane_scratch_bytes(n, n_hyp) bytes, 32-byte aligned. */
int avl_plane_ransac(const void* pts, int n, int dtype, int64_t point_stride, int64_t comp_stride, const double* T_host,
                     const double* roi_host, const int32_t* triples /* DEVICE int32 [n_hyp][3], point indices */, int n_hyp,
                     int weight_method, double x0, int norm /* 1 | 2 */, double tolerance, double min_c, double* planes_out,
                     int32_t* counts_out, void* result, void* scratch, void* stream);

/* ---- the prior point map, tiled and cropped per frame (not in the reference; csrc/seg_pointsmap.hip) ----------------------------
 * Replaces the /reduced_map subscription (src/mapping.py:61-62) and the unpacking of what arrives on it (pcd_callback, :172-183): in
 * the reference's deployment a node outside the package crops the site's point map around the vehicle and republishes the crop.
 * Here the whole map is on the device, stored as float32 [N'][4] (x, y, z, intensity; world frame) sorted by ground tile, and one
 * kernel per frame copies the tiles of a rectangle into a contiguous cloud for the frame entry points above.
 *
 * DROP RULE.  A point is dropped if any of its four fields is NaN, or if x or y is infinite.
 * TILE RULE.  ix = (int) floor(((double) x - ox) / tile_m), and the same for iy with oy.  ox = floor(min_x / tile_m) * tile_m over
 * the kept points, in float64, and the same for oy.  rows = ix_max + 1, cols = iy_max + 1, key = ix * cols + iy.  An index is
 * refused when rows * cols > 2^24 or N >= 2^31.
 * The points are sorted by key, stable: inside a tile they keep the input's order.  offsets int32 [rows * cols + 1]: tile `key`
 * is points[offsets[key] .. offsets[key + 1]).  Row r of a rectangle (r0..r1, c0..c1, both ends included) is therefore one run,
 * offsets[r * cols + c0] .. offsets[r * cols + c1 + 1].  A rectangle with r0 > r1 or c0 > c1 is empty; any other must lie inside
 * the index (AVL_E_ARG otherwise). */
/* keys[k] = the key of points[k] by the two rules, -1 for a dropped point (and for one outside rows x cols, which the rule's own
 * ox, oy, rows, cols never produce).  points float32 [n][4] on the device, 16-byte aligned; keys int32 [n] on the device. */
int avl_points_map_keys(const float* points, int64_t n, double ox, double oy, double tile_m, int rows, int cols, int32_t* keys, void* stream);
/* Host only, no HIP call: *m_out = the points of the rectangle (the sum of its run lengths), *runs_out = its non-empty runs. */
int avl_points_map_window(const int32_t* offsets_host, int rows, int cols, int r0, int r1, int c0, int c1, int64_t* m_out,
                          int32_t* runs_out);
/* dst[0 .. M) = the rectangle's runs in row order, M as avl_points_map_window counts it from offsets_host, the host's copy of
 * offsets_dev (sizes the launch; the kernel reads offsets_dev alone and never writes past M).  One lane copies one point as one
 * 16-byte load and one 16-byte store: points and dst (float32 [dst_capacity][4]) are 16-byte aligned.  Nothing is copied from the
 * host, allocated or waited for, so the call can be captured in a graph.  At most 1024 rows go into one launch, a taller rectangle
 * takes several.  M = 0 launches nothing; dst_capacity < M is AVL_E_ARG. */
int avl_points_map_gather(const float* points, const int32_t* offsets_dev, const int32_t* offsets_host, int rows, int cols, int r0, int r1,
                          int c0, int c1, float* dst, int64_t dst_capacity, void* stream);

/* ---- the scrolling grid: tile jobs (not in the reference; csrc/seg_scroll.hip, vision_semantic_segmentation_amd/scroll.py) --------
 * The reference's grid is the fixed rectangle of MAPPING.BOUNDARY (src/mapping.py:106-117) and a point outside it is dropped
 * (:410-411).  With MAPPING.SCROLL the device grid [Hm][Wm][C] is a window whose origin moves in whole tiles of T x T cells; tiles
 * that leave go to slabs of a tile store in HBM, tiles that enter come back from it or start empty.  A scroll, a reload, the assembly
 * of a site and a save are all tables of the one job below.  THE RULE:
 *   1. tile: T = tile_cells rows of T * bytes_per_cell bytes; row r of the source starts at src + r * src_pitch, of the destination
 *      at dst + r * dst_pitch (pitches in bytes: Wm * bytes_per_cell for a tile of a window, T * bytes_per_cell for a slab).
 *   2. copy: the destination tile becomes the source tile, byte for byte.  src == NULL: every 32-bit word of the destination tile
 *      becomes `fill`, the layer's empty word (0 for the map and the elevation layer's sum and count, 0x7fffffff for its minimum,
 *      0x80000000 for its maximum: avl_elevation_reset's state).  One call serves one layer.
 *   3. flag: with flag >= 0, flags[flag] = 1 iff some 32-bit word of the SOURCE tile differs from `fill` (0 for src == NULL), else
 *      flags[flag] = 0.  Bit patterns are compared: a tile that holds a -0.0 is not empty.  The call zeroes flags[0 .. n_flags) itself,
 *      stream-ordered, before the kernel; the kernel sets a flag with an integer atomic OR.  A flag index >= n_flags is ignored.
 *   4. no two jobs of a call write the same byte, and no job reads a byte another writes: the kernel orders nothing between jobs.
 * The caller owns the table's validity: every src, dst and pitch 16-byte aligned, every range inside the buffer it belongs to.  The
 * library cannot check a table that lives on the device; scroll.validate_jobs does, on the host, before the upload.  The same record
 * serves avl_tile_merge below, whose rule reads its last word. */
typedef struct avl_tile_job {
    const void* src;      /* first byte of the source tile, or NULL: the destination is filled with the fill word */
    int64_t src_pitch;    /* bytes between tile rows of the source                                               */
    void* dst;            /* first byte of the destination tile                                                  */
    int64_t dst_pitch;    /* bytes between tile rows of the destination                                          */
    int32_t flag;         /* >= 0: the flag that receives rule 3; < 0: none                                      */
    int32_t fresh;        /* read by avl_tile_merge only (!= 0: its rule 2), ignored by avl_tile_copy            */
} avl_tile_job;

/* Executes jobs_dev[0 .. n_jobs), a DEVICE array, by the rule above, in one launch on `stream`: 16 bytes per lane, a tile split over
 * enough workgroups that twenty jobs still fill the machine.  Nothing is allocated, copied from the host or waited for.  n_jobs == 0
 * only zeroes the flags.  AVL_E_ARG, before any GPU work: n_jobs < 0 or above 2^20, a NULL jobs_dev with n_jobs > 0, n_flags < 0, a
 * NULL flags with n_flags > 0, tile_cells outside 1 .. 16384, bytes_per_cell no multiple of 4 or outside 4 .. 128,
 * tile_cells * bytes_per_cell no multiple of 16. */
int avl_tile_copy(const avl_tile_job* jobs_dev, int n_jobs, int tile_cells, int bytes_per_cell, uint32_t fill, int32_t* flags, int n_flags,
                  void* stream);

/* ---- merging sites: tile merge jobs (not in the reference; csrc/seg_sitemerge.hip, scroll.TileStore.merge_site) -------------------
 * A frame's contribution never reads the grid, so the sum of two sites is the site of all their frames.  Another run's or another
 * rank's tiles are accumulated into this map's tiles where those live: the window buffer, a slab of the store.  THE RULE:
 *   1. tile: the record is struct avl_tile_job above, with its rule 1; src is never NULL, dst is accumulator and result, and
 *      bytes_per_cell is the DESTINATION's.  In AVL_MERGE_ADD_F32_TO_F64 the source tile is float32 and its rows hold half the
 *      destination row's bytes.
 *   2. merge: result = acc (+) src, element by element, written to the destination.  acc is the destination's old content, read and
 *      written in place by the same lane.  With fresh != 0, acc is the layer's fill word in every 32-bit word and the destination is
 *      NOT read: whatever bytes it holds do not reach the result.  A fresh tile is no byte copy -- +0.0 + -0.0 = +0.0 -- so the
 *      result never depends on whether the destination tile happened to exist before.
 *   3. (+) is the call's `op`; the adds are ONE IEEE-754 (round to nearest even, denormals kept) or two's-complement addition per
 *      element, no FMA:
 *        AVL_MERGE_ADD_F64          float64 + float64
 *        AVL_MERGE_ADD_F32          float32 + float32
 *        AVL_MERGE_ADD_F32_TO_F64   acc + (double)src, float32 source, float64 destination: the exchange form, half the payload
 *        AVL_MERGE_ADD_I64          int64 + int64, wraps          (the elevation layer's sum)
 *        AVL_MERGE_ADD_I32          int32 + int32, WRAPS: two counts whose sum passes 2^31 - 1 come out negative (its count)
 *        AVL_MERGE_MIN_I32          signed minimum                (its minimum, fill 0x7fffffff)
 *        AVL_MERGE_MAX_I32          signed maximum                (its maximum, fill 0x80000000)
 *      A NaN operand gives a NaN; which payload is not part of the rule.
 *   4. flag: with flag >= 0, flags[flag] = 1 iff some 32-bit word of the RESULT tile differs from `fill`, else 0; bit patterns are
 *      compared.  The mechanism is avl_tile_copy's: the call zeroes flags[0 .. n_flags), stream-ordered, before the kernel, which
 *      sets a flag with an integer atomic OR.  A flag index >= n_flags is ignored.
 *   5. no two jobs of a call name the same destination tile and no job's source is any job's destination: the kernel orders nothing
 *      between jobs.  (A job reading and writing its OWN destination in place is the merge itself.)
 * The caller owns the table's validity as for avl_tile_copy: every src, dst and pitch 16-byte aligned, no NULL src or dst, every range
 * inside the buffer it belongs to.  scroll.validate_jobs(..., merge=True) checks that on the host before the upload. */
#define AVL_MERGE_ADD_F64 0
#define AVL_MERGE_ADD_F32 1
#define AVL_MERGE_ADD_F32_TO_F64 2
#define AVL_MERGE_ADD_I64 3
#define AVL_MERGE_ADD_I32 4
#define AVL_MERGE_MIN_I32 5
#define AVL_MERGE_MAX_I32 6

/* Executes jobs_dev[0 .. n_jobs), a DEVICE array, by the rule above, in one launch on `stream`: 16 bytes per lane and memory
 * instruction, a tile split over workgroups by rows as in avl_tile_copy.  One call serves one layer.  Nothing is allocated, copied
 * from the host or waited for.  n_jobs == 0 only zeroes the flags.  AVL_E_ARG, before any GPU work: avl_tile_copy's list, an op
 * outside the seven above, bytes_per_cell no multiple of 8 for the 64-bit ops (ADD_F64, ADD_F32_TO_F64, ADD_I64), a destination row
 * -- or, for ADD_F32_TO_F64, the source row of half its bytes -- that is no multiple of 16 bytes. */
int avl_tile_merge(const avl_tile_job* jobs_dev, int n_jobs, int op, int tile_cells, int bytes_per_cell, uint32_t fill, int32_t* flags,
                   int n_flags, void* stream);

/* ---- the site overview: a reduced grid and its picture straight from the tiles (not in the reference; csrc/seg_overview.hip) ---------
 * A scrolled map's site lives in tiles: in the window buffer and in the store's slabs.  The overview reads them where they are and
 * writes a grid reduced by k x k cells per pixel and its picture; nothing of the site is assembled at full resolution.  THE RULE:
 *   1. geometry: k = cells per pixel, an integer >= 1 that divides T = tile_cells, so a pixel block never straddles a tile.  For a
 *      rectangle of nh x nw tiles the outputs have nh * T / k rows of nw * T / k pixels; pixel (p, q) covers the rectangle's cells
 *      [p * k, p * k + k) x [q * k, q * k + k).  The tile at (row, col) of the rectangle holds the cells [row * T, +T) x [col * T, +T).
 *   2. reduction: for every class c, R[p][q][c] is a left fold in the map's own type (f64 or f32): the accumulator starts at +0;
 *      di = 0 .. k-1 is the outer loop and dj = 0 .. k-1 the inner one; each step is acc = acc + cell[p*k + di][q*k + dj][c].  No FMA,
 *      no reassociation (the translation unit is built with -ffp-contract=off).  The order is part of the rule: it makes R
 *      reproducible bit for bit on a log confusion matrix.  (k = 1: R = +0 + cell, so a cell's -0.0 arrives as +0.)
 *   3. picture: pixel (p, q) is the render rule of csrc/avl_render.h -- the one statement that avl_render_bev_map(_thresholds),
 *      avl_live_map, avl_live_view and avl_site_finish call too -- on the row R[p][q][0 .. C): argmax_class, the colour of the first
 *      maximum (a NaN beats every number, the first NaN wins), black where np.sum of the row in NumPy's order (numpy_row_sum_of)
 *      is 0.  With thresholds it is thresholds_class instead: the share R[..][ch] / sum in the map's type against the threshold
 *      rounded to that type, priorities from low to high, later ones overwrite.
 *      For k = 1 the picture is byte-equal to avl_render_bev_map(_thresholds) on the assembled rectangle.
 *   4. absent tiles: a tile of the rectangle without a table entry (it is neither in the window nor in the store, or it is empty)
 *      gives black pixels and R = +0.
 * The caller owns the table's validity, as for avl_tile_job: src and src_pitch 16-byte aligned, every tile inside the buffer it
 * belongs to, row / col inside nh x nw, no (row, col) twice.  scroll.validate_sources checks that on the host before the upload. */
typedef struct avl_tile_src {
    const void* src;      /* first byte of the tile: T rows of T * C * sizeof(map type) bytes                                   */
    int64_t src_pitch;    /* bytes between tile rows: Wm * bytes_per_cell for a tile of the window, T * bytes_per_cell for a slab */
    int32_t row, col;     /* the tile's place inside the rectangle of nh x nw tiles                                              */
} avl_tile_src;

/* The overview of tiles_dev[0 .. n_tiles), a DEVICE array, by the rule above, in one launch on `stream`: picture uint8
 * [nh*T/k][nw*T/k][3], reduced (map type, or NULL: the picture only) [nh*T/k][nw*T/k][C].  colors_host uint8[C][3];
 * thresholds_host double[C] or NULL = the arg-max renderer; priority_host int32[C] or NULL = 0 .. C-1 (read with thresholds only).
 * The call zero-fills picture, and reduced if given, stream-ordered before the kernel, and launches only the listed tiles; it
 * allocates nothing, copies nothing from the host and waits for nothing.  n_tiles == 0 does the zero fill alone.  AVL_E_ARG, before
 * any GPU work: k < 1 or tile_cells % k != 0, tile_cells outside 1 .. 16384, C outside 1 .. AVL_MAX_MAP_CLASSES, a map_dtype that is
 * neither AVL_F64 nor AVL_F32, a tile row (tile_cells * C elements) that is no multiple of 16 bytes, nh or nw <= 0, n_tiles outside
 * 0 .. nh * nw, an output of 2^31 pixels or more, a NULL picture or colors_host, a NULL tiles_dev with n_tiles > 0, a tiles_dev that
 * is not 8-byte aligned, a reduced that is not aligned to its element, a priority outside 0 .. C-1. */
int avl_site_overview(const avl_tile_src* tiles_dev, int n_tiles, int nh, int nw, int tile_cells, int C, int map_dtype, int k,
                      const uint8_t* colors_host, const int32_t* priority_host, const double* thresholds_host, uint8_t* picture,
                      void* reduced, void* stream);

/* ---- the site finish: the filtered picture, the labels and the score of a scrolled site straight from its tiles (the reference's
 * finish_run chain, src/mapping.py:323-345, on a site instead of one grid; csrc/seg_sitefinish.hip) ------------------------------------
 * THE RULE.  For a rectangle of nh x nw tiles of T x T cells the result is DEFINED as this chain on the assembled rectangle:
 *   1. A [nh*T][nw*T][C] is the rectangle at full resolution: the tile at (row, col) holds the cells [row*T, +T) x [col*T, +T); a
 *      tile without data -- no record, or a record with src == NULL -- is +0.  This is what site_map(rect) assembles.
 *   2. F = avl_grid_box_filter(A) with Hm = nh*T, Wm = nw*T: avl::box_filter3_taps of csrc/avl_render.h, nine products by
 *      (double)(1.0f / 9.0f) accumulated in double from +0, dy outer and dx inner, BORDER_REFLECT_101 at the RECTANGLE's edge (never
 *      at a tile's), rounded to the map's type.  Without AVL_LIVE_FILTER in `flags` the filter is off: F = A, bit for bit.
 *   3. picture = avl_render_bev_map(F); with thresholds_host, avl_render_bev_map_thresholds(F, priority_host, thresholds_host)
 *      (the same device functions: argmax_class / thresholds_class of csrc/avl_render.h).
 *   4. labels = avl_eval_map's colour -> label table on picture (colour_label of csrc/avl_render.h), 0 where the mask is 0.
 *   5. counts[g * 8 + l] += 1 for every cell of every tile THAT HAS A RECORD, l its label and g the truth there (values above 7
 *      count as 7).  Truth is a raster gt uint8[Hg][gt_ld] whose element [0][0] lies at rectangle cell (gt_r0, gt_c0), either may be
 *      negative; the optional mask uint8[Hg][mask_ld] (0 = invalid) has the same geometry.  A cell outside the raster has g = 0 and
 *      is unmasked.  counts is uint64[64]; the call zeroes it, stream-ordered.  The cells of tiles without a record are the caller's
 *      to add (their label is 0): evaluation.SiteTruth.tile_hist.
 * RECORDS.  A record is an avl_tile_fin, a sibling of avl_tile_src that also carries the neighbour lookup: nb[(dr + 1) * 3 + (dc + 1)]
 * is the index of the record at (row + dr, col + dc), or -1 where there is none; nb[4] is the record's own index.  A record with
 * src == NULL is a tile that holds nothing but is computed, written and counted in full: the host lists one for every absent tile with
 * at least one present 8-neighbour, because the filter puts a ninth of the neighbour's border into that tile's outer ring.  Tiles
 * without a record keep the zero fill: black, label 0.  So every output byte has exactly one writer.  A NULL record or a missing
 * neighbour contributes +0 and none of its bytes is read -- a window tile that is masked out as empty may hold garbage.
 * The caller owns the table's validity as for avl_tile_src, plus the neighbour indices: scroll.validate_finish checks all of it on
 * the host before the upload.  (The kernel ignores an index outside 0 .. n_tiles-1.) */
typedef struct avl_tile_fin {
    const void* src;      /* first byte of the tile, or NULL: a tile of +0                                                         */
    int64_t src_pitch;    /* bytes between tile rows                                                                              */
    int32_t row, col;     /* the tile's place inside the rectangle of nh x nw tiles                                               */
    int32_t nb[9];        /* record index of the tile at (row + dr, col + dc) in nb[(dr + 1) * 3 + (dc + 1)], -1 = none; nb[4] = own */
    int32_t pad;
} avl_tile_fin;

/* The finish of tiles_dev[0 .. n_tiles), a DEVICE array, by the rule above, in one launch on `stream`.  Each output is optional
 * (NULL): picture uint8 [nh*T][nw*T][3], labels uint8 [nh*T][nw*T], counts uint64[64] (device; given exactly when gt is); at least
 * one must be given.  colors_host uint8[C][3]; thresholds_host double[C] or NULL = the arg-max renderer; priority_host int32[C] or
 * NULL = 0 .. C-1.  flags: AVL_LIVE_FILTER or 0.  gt / mask are DEVICE rasters of Hg x Wg elements (the geometry is needed when
 * either is given; a mask may come without gt, for labels).  The call zero-fills picture and labels and zeroes counts, stream-ordered
 * before the kernel, and launches only the listed tiles; it allocates nothing, copies nothing from the host and waits for nothing.
 * n_tiles == 0 does the fills alone.  AVL_E_ARG, before any GPU work: avl_site_overview's list (without k), tile_cells < 2, a flag
 * other than AVL_LIVE_FILTER, no output given, counts without gt or gt without counts, Hg or Wg <= 0 with a gt or a mask, gt_ld < Wg
 * or mask_ld < Wg (gt_r0 and gt_c0 may be any int), an output of 2^31 cells or more, a counts that is not 8-byte aligned. */
int avl_site_finish(const avl_tile_fin* tiles_dev, int n_tiles, int nh, int nw, int tile_cells, int C, int map_dtype, int flags,
                    const uint8_t* colors_host, const int32_t* priority_host, const double* thresholds_host, const uint8_t* gt,
                    int Hg, int Wg, int64_t gt_ld, int gt_r0, int gt_c0, const uint8_t* mask, int64_t mask_ld, uint8_t* picture,
                    uint8_t* labels, unsigned long long* counts, void* stream);

/* ---- the live cost map: class costs, lethal cells and an inflated margin over the live map's window (csrc/seg_costmap.hip) --------
 * The reference has no cost map; like avl_live_map this is a build-specific consumer of the grid: what the vehicle's planner
 * reads instead of a picture.  THE RULE.  The result for a window is DEFINED as the crop of the following, taken over the WHOLE
 * PLANE of cells, (gx, gy) any pair of integers:
 *   class   cls(gx, gy) is the class of grid cell (gx, gy) by avl_live_map's rule: the cell's row through avl::box_filter3_taps
 *           rounded to map_dtype with AVL_LIVE_FILTER (reflect-101 at the GRID's edge), then avl::argmax_class, or
 *           avl::thresholds_class with AVL_LIVE_THRESHOLDS (priority_host NULL = 0..C-1; thresholds_host is required then); all of
 *           csrc/avl_render.h.  A cell off the grid has no class.  AVL_LIVE_FILL is refused: the hole filler is a picture operation.
 *   base    b = cost_host[cls]; cost_host int8[C + 1], entry C the cost of a cell with no class -- empty or off the grid.  Legal
 *           values are 0 .. 100 and -1, "no information"; 100 is lethal (AVL_COST_LETHAL).
 *   ego     with car_host != NULL, avl_live_map's double[AVL_LIVE_CAR_DOUBLES], a cell whose centre lies in the ego rectangle --
 *           dx = (gx + 0.5) - cx, dy = (gy + 0.5) - cy, u = c*dx + s*dy, v = c*dy - s*dx (float64, no contraction), u_lo <= u < u_hi
 *           and v_lo <= v < v_hi -- gets b = 0 before anything else: a noisy label under the car must not inflate.
 *   d2      d2(gx, gy) = the minimum of dx*dx + dy*dy over the lethal cells (gx + dx, gy + dy) with |dx|, |dy| <= R, where that
 *           minimum is <= R*R; AVL_COST_FAR (65535) if there is no such cell.  An integer; R = radius_cells, 0 ..
 *           AVL_COST_MAX_RADIUS (32).  A lethal cell has d2 = 0.
 *   infl    v = infl_host[d2] when d2 <= R*R, else 0.  infl_host uint8[R*R + 1] is built on the host (renderer.inflation_table):
 *           infl_host[0] == 100, values 0 .. 100, non-increasing in d2.  The kernels see only the table: no floating point takes
 *           part in the distance or the inflation.
 *   result  out = max(b, v) when b >= 0;  out = v > 0 ? v : -1 when b == -1.
 * cost_out int8: element (i, j) of the window stands for grid cell (x0 + i, y0 + j) and sits at i * stride_i + j * stride_j
 * (elements).  (w, 1) is [h][w], the live map's order; (1, h) is [w][h], nav_msgs/OccupancyGrid's order, x fastest.  The strides
 * must address h * w distinct elements: both in 1 .. 2^40, and the larger steps over the other axis' whole extent (an axis of one
 * element asks nothing).  d2_out uint16, same addressing, or NULL: the clearance itself.
 * scratch: avl_cost_map_scratch_bytes(h, w, radius_cells) bytes of device memory, about (h + 2R)(w + 2R) -- the base cost of the
 * window and its ring of R cells; 0 for sizes the call refuses.  Two launches on `stream`; the call allocates nothing, copies
 * nothing and waits for nothing.  The grid is only read; the window may lie partly or wholly off it.  1 <= h, w <= 32768;
 * C <= AVL_MAX_MAP_CLASSES; the filter needs Hm, Wm >= 2.  AVL_E_ARG, before anything touches the device: a NULL map, cost_host,
 * infl_host, cost_out or scratch, a size, radius, flag, cost, table or pair of strides outside the above, a scratch_bytes below
 * avl_cost_map_scratch_bytes. */
#define AVL_COST_LETHAL 100
#define AVL_COST_FAR 65535
#define AVL_COST_MAX_RADIUS 32
int64_t avl_cost_map_scratch_bytes(int h, int w, int radius_cells);
int avl_cost_map(const void* map, int map_dtype, int Hm, int Wm, int C, int x0, int y0, int h, int w, int flags,
                 const int32_t* priority_host, const double* thresholds_host, const int8_t* cost_host, const double* car_host,
                 int radius_cells, const uint8_t* infl_host, int8_t* cost_out, int64_t stride_i, int64_t stride_j, uint16_t* d2_out,
                 void* scratch, int64_t scratch_bytes, void* stream);

/* ---- a1-a5: segmentation forward (DeepLabV3+ / ResNeXt-50 OS8, eval mode) -------------------
 *
 * The reference builds the network from torch modules (src/semantic_segmentation.py:21-57,
 * src/network/deeplab_v3_plus/models/{deeplab_v3_plus,aspp,decoder}.py, torchvision ResNet).  Here
 * the Python host folds BatchNorm into the convolutions, lays activations out as NHWC
 * ([H*W rows][channels], row stride `ld` elements, so channel slices of a wider buffer give
 * torch.cat for free) and hands the library a flat list of ops; avl_seg_plan_run() launches them in
 * order on one stream.  Activations are AVL_BF16 / AVL_F16 (16x16x32 MFMA, fp32 accumulate) or AVL_F32
 * (fp32-input MFMA, the reference's precision).  Biases are always fp32.
 *
 * Every buffer named by an op must stay allocated while the plan lives; `*_rows` is the number of
 * rows actually allocated (GEMM tiles read whole 128-row tiles, so M is padded up by the caller and
 * the plan checks it). */

#define AVL_OP_STEM 1        /* uint8 RGB [H][W][3] (or fp32 [3][H][W]: in_format) -> normalise (semantic_segmentation.py:35-39) -> 7x7 s2 p3 conv +bias+ReLU.
                                stride = 4 (16-bit MFMA stem, w_layout 1, not w_split): AVL_OP_MAXPOOL runs in the epilogue and out_h x out_w is the
                                POOLED size -- the bits of stem -> max-pool, the conv map never written */
#define AVL_OP_MAXPOOL 2     /* 3x3 s2 p1 (torchvision ResNet.maxpool)                                          */
#define AVL_OP_GEMM 3        /* 1x1 conv: out[m][n] = act(sum_k in[row(m)][k] w[n][k] + bias[n] (+ in2[m][n])) */
#define AVL_OP_GCONV 4       /* grouped or dense 3x3 conv, stride 1|2, dilation d, pad d, +bias+ReLU (Bottleneck.conv2; w_layout) */
#define AVL_OP_DWCONV 5      /* depthwise conv +bias+ReLU (core/nn/modules/conv.py:131); weight fp32 [ksize*ksize][C].
                                ksize 3: dilation d, pad p (ASPP, decoder).  ksize 1, 2, 4..7 (MODEL.DECODER.REFINE_KERNEL_SIZE,
                                seg_dwconv_k.hip): the decoder's geometry only -- stride 1, dil 1, pad 0, out = in - (ksize - 1),
                                no out_mx, in_lo / out_lo both set (split f16) or both unset, in2 unused                    */
#define AVL_OP_BILINEAR 6    /* F.interpolate(mode='bilinear', align_corners=True) (aspp.py:88, decoder.py:47)   */
#define AVL_OP_GAP 7         /* AdaptiveAvgPool2d((1,1)) -> fp32 [C] (aspp.py:69)                                */
#define AVL_OP_GEMV 8        /* out[n] = act(sum_k w[n][k] in[k] + bias[n]) on fp32 vectors (pooled branch)      */
#define AVL_OP_ARGMAX 9      /* torch.argmax(dim=1) over fp32 logits [M][C] -> uint8 (semantic_segmentation.py:56) */
#define AVL_OP_SUBSAMPLE 10  /* rows of a stride-s 1x1 conv's input (Bottleneck.downsample in layer2.0)          */
#define AVL_OP_DWPW 11       /* DepthwiseSeparableConv2d in ONE kernel (conv.py:103-141; the dilated ASPP branches):
                                depthwise 3x3 (dil d, pad d) +bias+ReLU -> 1x1 conv +bias+ReLU, 16-bit types only.
                                weight/bias = the 1x1 conv's (as AVL_OP_GEMM); in2 = depthwise parameters packed
                                [K/64][8][6][8] dwords: five tap pairs (taps 2p | 2p+1 << 16 in the activation type)
                                and the fp32 bias of each 8-channel chunk; then int32[ceil(H*W/128)]: the order in
                                which the 128-pixel tiles are visited (a permutation; tiles a dilation apart adjacent).
                                w_split = 3 (AVL_F16; what the "mixed" network emits): the EXACT depthwise stage -- FP32 depthwise
                                weights and a split depthwise result (three MFMA passes); in2 = float32 [K/64][8][10][8] per
                                8-channel chunk: rows 0 .. 8 = tap t of the chunk's eight channels, row 9 = the bias; then the
                                tile order as above.  `weight` is the 1x1 conv's [n][K/64][hi 64 | lo 64] as for w_split = 1.
                                (w_split = 2 -- depthwise weights as f16 pairs, rounds 3-5 -- is no longer accepted.)
                                With out_f32 (split input, w_split = 3, out_c = 256): the network's LAST 1x1 conv (decoder.py:42-43:
                                256 -> in3_c <= 32 classes, bias, no BN / ReLU) and torch.argmax (semantic_segmentation.py:56) run in the
                                epilogue on the block's result, which is never written: in3 = classifier weights f16 [hi | lo][32][256]
                                (rows >= in3_c zero), in2_lo = fp32 bias[32], out = fp32 logits [rows][in3_c] (out_ld = in3_c),
                                out_mx = uint8 labels[rows].
                                With in_lo (w_split = 3): the input is two f16 planes (the "mixed" decoder's refine blocks,
                                decoder.py:33-43; the ASPP branches of the complete hi + lo plan).  w_layout = 1 (with in_lo):
                                a tile is an 8 x 16 block of output pixels instead of 128 consecutive ones; the order array
                                then has ceil(out_h / 8) * ceil(out_w / 16) entries (tile = block row * ceil(out_w / 16) + block column). */

#define AVL_OP_BOTTLENECK 12 /* one torchvision Bottleneck of layer1 (backbone/resnet.py:24-43; stride 1, dilation 1, width 128 -> 256
                                channels) in ONE kernel, AVL_F16 "mixed" precision: conv1 1x1 +b+ReLU -> grouped 3x3 (32 groups, pad 1)
                                +b+ReLU -> conv3 1x1 +b (+ identity | + downsample 1x1) -> ReLU; the two intermediates live in LDS.
                                in (+ in_lo: enters the residual sum only) = block input, in_c = 256 (identity residual, w_layout 0)
                                or 64 (the block's downsample 1x1 runs as extra K steps of conv3: w_layout 1); out (+ out_lo).
                                Weights are f16 pairs hi + lo in MFMA FRAGMENT order ([...][hi, lo][lane 64][8], network.pack_bottleneck):
                                weight = conv1 [n 8][ks in_c/32], in2 = the 3x3 as block-diagonal 16-channel windows [window 8][ks 5]
                                (K = 32 = two taps x 16 channels), in3 = conv3 [wave 8][ks 4 (+ in_c/32 downsample steps)][nj 2];
                                in3_c = 128 (the width); bias = fp32 [b1 128 | b2 128 | b3 256 (+ downsample bias)].
                                w_split = 1 (in_c = 64 only): conv1's result keeps a lo plane in LDS (conv2 runs a third pass).
                                in_c = 512: an identity block of layer2 (width 256 -> 512 channels; in3_c = 256, w_layout = w_split = 0,
                                weight [n 16][ks 16], in2 [window 16][ks 5], in3 [wave 8][ks 8][nj 4]; bias [b1 256 | b2 256 | b3 512]),
                                the trunk in the MX form on both sides: in + in_mx (lo part only as FP4, in_lo NULL), out + out_mx (both
                                halves, out_lo NULL), mx_flags = AVL_MX_IN_LO | AVL_MX_OUT_LO, in_ld = out_ld = 512.  A conv1 result beyond
                                f16's range makes the whole tile's output non-finite (the plan's non-finite screen then names the block). */

typedef struct avl_seg_op {
    int32_t kind;            /* AVL_OP_*                                                        */
    int32_t dtype;           /* activation type of in/in2/out: AVL_BF16, AVL_F16 or AVL_F32      */
    const void* in;          /* input activation (STEM: uint8 image, or fp32 planes: in_format; GEMV/GAP-out: fp32) */
    const void* in2;         /* GEMM: residual added before the ReLU, or NULL; GAP: fp32 scratch [256][C];
                                DWCONV (ksize 3): 32 zero bytes (what a tap outside the image reads);
                                STEM: NULL, or the camera block of a pre-processing stem (avl_stem_camera_set; any dtype,
                                AVL_F32 with w_layout 0, AVL_BF16 / AVL_F16 with w_layout 1); `batch` blocks with raw_batch */
    void* out;
    const void* weight;      /* packed by the host, layout per kind (see network.py)            */
    const float* bias;       /* fp32 [out_c padded], or NULL                                    */
    int32_t in_h, in_w, in_c, in_ld, in_rows;
    int32_t out_h, out_w, out_c, out_ld, out_rows;
    int32_t in2_ld;
    int32_t ksize, stride, pad, dil, groups;
    int32_t relu;
    int32_t out_f32;         /* GEMM: write fp32 (the logits) instead of `dtype`.  With out_mx != NULL (N <= 32, no residual, no ReLU): out_mx is
                                uint8 labels[out_rows] and the epilogue also writes torch.argmax over each row's N logits there (first maximal
                                index wins, a NaN counts as maximal; semantic_segmentation.py:56) -- AVL_OP_ARGMAX without its launch */
    int32_t w_rows;          /* GEMM: rows of `weight` allocated (out_c padded to the N tile)   */
    int32_t w_layout;        /* DWPW:  0 = tiles of 128 consecutive pixels, 1 = 8 x 16-pixel blocks (split input only, see AVL_OP_DWPW)
                                GCONV: 0 = float [group][tap][ci][co] (direct kernel),
                                       1 = bf16 block-diagonal 32-channel windows [window][2][9][16][32] (MFMA kernel)
                                       2 = DENSE 3x3 as an implicit GEMM (k_conv3x3; channels per group % 64 == 0: the ResNet /
                                           wide ResNet conv2, ResNeXt-101's layer4): MFMA fragments [group][chunk][tap 9][cg/32]
                                           [nj 2][part][h 2][lane 64][16 B] (network.pack_conv3x3; a chunk = one 128-byte pixel row
                                           = 64 channels of a 16-bit type, 32 of fp32).  AVL_BF16 / AVL_F16 / AVL_F32 on one plane
                                           (fp32: v_mfma_f32_16x16x4_f32), or AVL_F16 with w_split = 1: weights as f16 pairs (part
                                           0 = hi, 1 = lo), optional in_lo (three passes Wh.xh + Wl.xh + Wh.xl), out (+ out_lo).
                                           relu = 1; no MX bundle in or out; stride 1 or 2, any dilation whose input tile fits LDS
                                STEM:  0 = float [7][7][3][64] (direct kernel), 1 = bf16 [4][6][16][32] (MFMA kernel)
                                GEMM:  0 = the library picks the kernel; 1 .. 4 force one tile configuration of the 16-bit
                                       kernels (tools/bench_gemm.py: 1 = 128 x 128 two-buffer kernel, 2 = 256 x 128 ring,
                                       3 = 256 x 256 ring, 4 = 256 x 128 on four waves); avl_seg_plan_create
                                       refuses any other value, and 1 .. 4 on an AVL_F32 GEMM */
    int32_t w_split;         /* "mixed" precision (AVL_F16 only): 1 = `weight` holds each folded weight as an f16 pair
                                hi = f16(w), lo = f16(w - hi), packed per 64-wide K block in the order the kernel
                                walks it (GEMM/DWPW: [n][K/64][hi 64 | lo 64], or [hi | lo | hi] when the input is
                                split too; GCONV: 18 taps = 9 hi + 9 lo).  hi + lo carries ~22 significant bits:
                                the MFMAs run on both parts and accumulate in fp32.                             */
    int32_t mx_flags;        /* w_split = 2 only, see below: AVL_MX_IN_LO | AVL_MX_RES_LO | AVL_MX_OUT_LO                     */
    /* split activations (w_split modes): a tensor may be stored as TWO f16 planes of identical shape and stride,
     * value = hi + lo.  NULL = the tensor is a single f16 plane.  in_lo: the GEMM / depthwise input's low plane;
     * in2_lo: the residual's; out_lo: where the low part of the result goes (the op then rounds nothing away). */
    const void* in_lo;
    const void* in2_lo;
    void* out_lo;
    /* w_split = 2 (GEMM on gfx950's block-scaled matrix cores): `weight` is the plain f16 hi part [w_rows][K]; the correction
     * products run on MX-FP4 copies (OCP e2m1 elements, element 2i in the low nibble of byte i, one E8M0 scale per 32 values
     * along K) at 4x the f16 rate: Q4(W lo) x Q4(in hi) and, when in_lo is set, Q4(W hi) x Q4(in lo).
     * The MX GEMM multiplies exactly what it is passed: `in` x `weight` in f16, the hi half of in_mx x the first half of w_mx, the
     * lo half of in_mx x the second half of w_mx.  It reads the input's lo part from the BUNDLE's lo half only: in_lo (like
     * AVL_MX_IN_LO) merely switches the second correction pass on, the plane it points to is never read (a NaN-filled plane gives
     * the same bytes: tests/test_gpu_gemm_exact.py).
     * An "MX bundle" of a [rows][C] tensor (C % 256 == 0, dense rows) is laid out
     *     [FP4 plane of the hi part: rows x C/2 bytes][its scales: C/256 x rows x 8 bytes][the same two for the lo part]
     * w_mx: bundle of the weights (rows = w_rows; first Q4(W lo), then Q4(W hi)); in_mx: bundle of the input (rows = in_rows);
     * the WEIGHT bundle's scale arrays are permuted inside every 16-row block (network.permute_w_scales): for a 256-wide K block
     * the 128 scale bytes of rows r0..r0+15 are stored [row & 3][k quarter kq 0..3][n-tile (row >> 2) & 3][k half kk 0..1], i.e.
     * byte ((row & 3) * 4 + kq) * 8 + 2 * ((row >> 2) & 3) + kk holds the scale of row r0 + (row) for K block 4 kk + kq of the
     * eight 32-wide blocks: the eight bytes a lane of the kernel needs in a sub-step are then one aligned 8-byte word.
     * Activation bundles keep the natural [C/256][rows][8] order.
     * out_mx (GEMM with w_split = 2, or GCONV with w_split = 1): the op also writes the bundle of its OUTPUT (rows = out_rows;
     * the lo half only if out_lo is set), which is what the next MX GEMM reads as in_mx.
     * A tensor may keep its lo part ONLY as the FP4 half of its bundle (no f16 lo plane: 3 instead of 5 bytes per element
     * for the residual trunk).  mx_flags then says so: AVL_MX_IN_LO = the input's lo part is in in_mx (in_lo NULL);
     * AVL_MX_RES_LO = the residual's lo part is the FP4 lo half of in2_mx (in2_lo NULL; the 10 % error of FP4 applies to a
     * term that is 2^-11 of the sum); AVL_MX_OUT_LO = write the lo half of out_mx although out_lo is NULL.
     * A SECOND input (GEMM, w_split = 2): in3 [rows][in3_c] (row stride in3_ld, bundle in3_mx, same rows as `in`) is appended
     * along K -- out = W[:, :in_c] . in + W[:, in_c:] . in3: a Bottleneck's conv3 and its downsample 1x1 (stride 1) in ONE
     * product, the identity tensor never exists.  `weight` / `w_mx` then hold the concatenated [w_rows][in_c + in3_c] matrix.
     * in3 must be a dense tensor of its own (in3_ld == in3_c: its bundle's planes are addressed with that pitch). */
    const void* w_mx;
    const void* in_mx;
    void* out_mx;
    const void* in2_mx;
    const void* in3;
    const void* in3_mx;
    int32_t in3_c, in3_ld;
    /* BATCH: the op runs on `batch` images at once (0 and 1 both mean one).  in_h x in_w / out_h x out_w stay the size of ONE image;
     * the images are packed densely: image n occupies pixel rows [n * h * w, (n + 1) * h * w) of every activation (in, in_lo, in2,
     * in2_lo, in3, out, out_lo; the uint8 labels of an arg-max), and *_rows counts the rows of all images (padding once, at the end).
     * MX bundles keep their layout: image n's FP4 rows and scales sit at row offset n * h * w inside each plane and each C/256 slab,
     * the slab stride stays the total row count.  GAP: in2 = fp32 scratch [batch][256][C], out = fp32 [batch][out_ld]; GEMV: in and out
     * are [batch] vectors with strides in_ld / out_ld.  Every spatial kernel keeps its halo inside its own image, and every image
     * computes exactly what a batch-1 op on it computes (bit for bit).  A pre-processing stem (in2 set) takes one image
     * (AVL_E_UNSUPPORTED otherwise) unless it asks for a batch of raw frames with raw_batch = 1 (below). */
    int32_t batch;
    /* GEMM only: `bias` is fp32 [batch][w_rows] and output row r uses image r / (out_h * out_w)'s vector (the ASPP projection, whose
     * bias comes from each image's pooling branch).  Such a GEMM runs as one launch per image, so in_rows must cover the last image's
     * whole row tiles: in_rows >= (batch - 1) * out_h * out_w + round_up(out_h * out_w, 256).  Not with the MX GEMM (w_split 2). */
    int32_t bias_per_image;
    /* STEM only (AVL_IN_*): the form of `in`.  AVL_IN_U8_HWC (0) = uint8 RGB [batch][in_h][in_w][3], normalised by the stem.
     * AVL_IN_F32_CHW = fp32 [batch][3][in_h][in_w], already normalised by the caller ((x / 255 - mean) / std): image n starts at
     * float n * 3 * in_h * in_w, each channel plane is in_h * in_w floats, in_rows = batch * in_h * in_w.  The stem converts each value
     * as it converts the fp32 value its uint8 table holds, so a float input equal to that value gives the u8 path's bits.  Not with a
     * pre-processing stem (in2 set); other ops must leave it 0. */
    int32_t in_format;
    /* STEM with in2 only (a pre-processing stem); other ops must leave it 0.  0 = `in` is ONE raw BGR frame [src_h][src_w][3] and in2
     * one camera block; batch > 1 is refused.  1 = every image of the batch is a raw frame: `in` = uint8 [batch][src_h][src_w][3],
     * in_rows = batch * src_h * src_w, in2_ld = src_w, in2 = `batch` camera blocks of AVL_STEM_CAMERA_BYTES each (block n for image n,
     * 4-byte aligned); in_h x in_w = the network input of one image.  batch 0 or 1 with raw_batch = 1 is one frame.  Not with
     * AVL_IN_F32_CHW.  Any other value is AVL_E_ARG. */
    int32_t raw_batch;
    /* GEMM on the 16-bit ring kernel only (not w_split = 2, not AVL_F32, not w_layout 1 or 4, no residual): a SECOND destination.
     * out2 != NULL: `weight` / `bias` hold the rows of two 1x1 convs of the same input one after the other, out_c = both widths together;
     * output columns [0, n_split) go to out (+ out_lo, row stride out_ld), columns [n_split, out_c) to out2 (+ out2_lo, row stride
     * out2_ld; out2 points at the column of its buffer where column n_split lands).  n_split is a multiple of the N tile the op runs with
     * (tile_n of avl_seg_gemm_route, which may be asked before the buffers exist), so an output tile belongs to one destination; each
     * value is what the conv alone computes, bit for bit.  out_rows counts the rows of the shorter of the two buffers.
     * A ring GEMM also takes stride = s > 1 (Bottleneck.downsample of a striding block): in_h x in_w is then the UN-sampled input image,
     * out_h x out_w = ((in_h - 1) / s + 1) x ((in_w - 1) / s + 1), and output row (oy, ox) of image n reads input pixel
     * n * in_h * in_w + oy * s * in_w + ox * s -- AVL_OP_SUBSAMPLE without its launch and its copy; in_rows >= batch * in_h * in_w. */
    void* out2;
    void* out2_lo;
    int32_t out2_ld, n_split;
} avl_seg_op;

#define AVL_IN_U8_HWC 0
#define AVL_IN_F32_CHW 1

#define AVL_MX_IN_LO 1
#define AVL_MX_RES_LO 2
#define AVL_MX_OUT_LO 4

typedef struct avl_seg_plan avl_seg_plan;

/* copies the op list, validates shapes/strides/allocated rows against what the kernels read */
int avl_seg_plan_create(const avl_seg_op* ops_host, int n_ops, avl_seg_plan** out_plan);
void avl_seg_plan_destroy(avl_seg_plan* plan);
/* launches every op on `stream` (no sync); after avl_seg_plan_capture: one hipGraphLaunch */
int avl_seg_plan_run(avl_seg_plan* plan, void* stream);
/* records the op list into a hipGraph (stream capture on `stream`, non-NULL; run the plan once before) */
int avl_seg_plan_capture(avl_seg_plan* plan, void* stream);
/* same, with a hipEvent pair around every op; blocks until done; ms_host[n_ops] = op durations.
 * flops_host / bytes_host (either may be NULL) receive each op's algorithmic flops and bytes. */
int avl_seg_plan_profile(avl_seg_plan* plan, void* stream, float* ms_host, double* flops_host, double* bytes_host);
int avl_seg_plan_num_ops(const avl_seg_plan* plan);
/* diagnostic: runs the ops one by one and counts the Inf / NaN values of every op's output planes where they are produced
 * (counts_host[n_ops]; blocks until done, never inside a capture).  The 16-bit precisions turn an fp32 accumulator beyond the
 * type's range into Inf in the producing op's epilogue; a later ReLU can hide that from the logits.  SemanticSegmentation's
 * load-time self-check (semantic_segmentation.py:28-32 loads real checkpoints) refuses a plan with a non-zero count. */
int avl_seg_plan_nonfinite(avl_seg_plan* plan, void* stream, unsigned long long* counts_host);

/* ---- which kernel an AVL_OP_GEMM runs -------------------------------------------------------- */
#define AVL_GEMM_PLAIN 0     /* k_gemm<T, WM, WN>: two LDS buffers, tiles of WM * 64 rows x WN * 64 columns, one workgroup per tile */
#define AVL_GEMM_RING 1      /* k_gemm_ring<T, WM, WN, MI, STAGES, NSUB, IO, AST, EXT>: tiles of WM * MI * 16 rows x WN * 64 columns   */
#define AVL_GEMM_RING_MX 2   /* k_gemm_ring_mx<IO, MI>: the MX GEMM (w_split 2), tiles of MI * 32 rows x 256 columns                   */
#define AVL_GEMM_MX_PIPE 3   /* k_gemm_mx_pipe<IO, MI, LATE>: the MX GEMM with the software-pipelined main loop, same tiles           */

/* What the launch of one AVL_OP_GEMM decides.  A template argument the kernel family does not have is 0. */
typedef struct avl_gemm_route {
    int32_t kernel;              /* AVL_GEMM_*                                                                          */
    int32_t dtype;               /* element type the kernel is instantiated for (AVL_F32 / AVL_BF16 / AVL_F16)          */
    int32_t tile_m, tile_n;      /* rows and columns of an output tile                                                  */
    int32_t wm, wn;              /* PLAIN, RING: waves along M and N                                                    */
    int32_t mi;                  /* RING, MX: 16-row MFMA blocks per wave along M                                       */
    int32_t stages;              /* RING: LDS stages of the weight ring                                                  */
    int32_t nsub;                /* RING (template argument NSUB), PLAIN (a kernel argument): passes per K block, 1 (w_split 0),
                                    2 (w_split 1: weights split) or 3 (w_split 1 with in_lo: the input split too)        */
    int32_t io;                  /* RING: 1 = split residual / output planes (with nsub > 1); MX: 1 = the epilogue also writes the
                                    output's MX bundle (out_mx set)                                                     */
    int32_t ast;                 /* RING: LDS stages of the activation tile                                             */
    int32_t ext;                 /* the op asks for strided input rows or a second destination (stride > 1, out2, out2_lo or n_split set):
                                    RING runs its EXT instantiation; no other kernel has one (avl_seg_plan_create refuses the op) */
    int32_t late;                /* MX_PIPE: LATE                                                                       */
    int32_t launches;            /* `batch` for an op with a per-image bias (each launch: one image as a batch-1 op), else 1 */
    int32_t m_tiles, n_tiles;    /* of ONE launch: row tiles over all the rows of the batch (or the one image), column tiles */
    int32_t workgroups;          /* of ONE launch: m_tiles * n_tiles for PLAIN, min(m_tiles * n_tiles, 256) for the others,
                                    whose workgroups walk their tiles */
} avl_gemm_route;

/* The kernel avl_seg_plan_run launches for `op` (host only: looks at sizes, flags and whether pointer fields are NULL, never at
 * memory), provided avl_seg_plan_create accepts the op; it does not run that validation, so the buffers need not exist yet.
 * AVL_E_ARG for a NULL argument or an op that is not AVL_OP_GEMM.
 *
 * With M1 = out_h * out_w (the rows of ONE image: a batch runs the kernel its batch-1 plan runs), M = M1 * batch, N = out_c,
 * K = in_c (+ in3_c with a second input) and t256 = ceil(M1 / 256) * (N / 256), the first row that applies:
 *
 *   condition                                            kernel     tile        template arguments
 *   w_split 2 (the MX GEMM)                              MX_PIPE where K >= 1024, else RING_MX; IO = (out_mx set)
 *     t256 < 192 or 256 < t256 < 384                                128 x 256   MI 4, LATE 1
 *     otherwise                                                     256 x 256   MI 8, LATE 0
 *   ring-eligible: a 16-bit dtype, w_layout != 1, N > 64, N % 128 == 0, out_f32 0 and in_rows >= M rounded up to 256
 *                                                        RING; NSUB = nsub; IO = (NSUB > 1); T = f16 with NSUB > 1, else dtype;
 *                                                        EXT = ext
 *     v = 3                                                         256 x 256   WM 2, WN 4, MI 8, STAGES 3 with NSUB 2 else 2, AST 2
 *     v = 4 and NSUB 1                                              256 x 128   WM 2, WN 2, MI 8, STAGES 3, AST 3 (four waves; no EXT form)
 *     otherwise                                                     256 x 128   WM 4, WN 2, MI 4, STAGES 3, AST 3
 *     where v = w_layout, or with w_layout 0: 3 if t256 >= 192 and N % 256 == 0 and w_rows % 256 == 0, else 2; a forced 3 falls back to
 *     2 unless N % 256 == 0 and w_rows % 256 == 0
 *   N <= 64                                              PLAIN      256 x 64    T = dtype, WM 4, WN 1
 *   otherwise (AVL_F32, w_layout 1, out_f32, ...)        PLAIN      128 x 128   T = dtype, WM 2, WN 2
 *
 * m_tiles = ceil(M / tile_m), n_tiles = ceil(N / tile_n).  An op with bias_per_image and batch > 1 runs `batch` launches, each the
 * route of one image (M = M1, that image's rows). */
int avl_seg_gemm_route(const avl_seg_op* op, avl_gemm_route* out);

#ifdef __cplusplus
}
#endif
#endif /* AVL_HIP_H */
