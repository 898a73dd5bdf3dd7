// depth_adjoint.h -- C ABI of the depth camera's adjoint (csrc/depth_adjoint.hip): the derivative of the depth images of
// dss_depth_render / dss_depth_render_grids (include/depth_camera.h) with respect to the bodies' poses, shape parameters and grid
// samples, exported by libdiffsdfsim_hip.so beside the functions of include/*.h, whose conventions it shares (device pointers
// into caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).
// Bound by world_abi.OPTIONAL_PROTOTYPES; diffsdfsim_amd/depth_camera.py (render_depth_diff) is the caller.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Pixel (row, col) of view v hit body b = seg at depth t.  Its ray is x(t) = o + t d_w, d_w = Rc (nx, -ny, -1) as in
 * depth_camera.h, and the hit satisfies F(t, theta) = phi_b(R(q)^T (x(t) - pos); prm, samples) = 0, so with n_w = R grad_p phi
 *
 *     d t / d theta = -(d F / d theta) / (n_w . d_w)
 *
 * and the call adds, per (view, body), g_depth[pixel] * d t / d theta over the body's pixels:
 *   g_pose [nview][nbody][7]   w.r.t. the four raw quaternion components and the position (the layout of pose)
 *   g_prm  [nview][nbody][3]   w.r.t. the three shape parameters (the corner radius prm[3] and a grid's scale are constants)
 *   g_grid                     pooled like grid_data: w.r.t. the samples of the 8 corners of the hit's cell, d F / d sample =
 *                              scale * the corner's trilinear weight; ADDED to what the caller put there (zero it first);
 *                              NULL: not wanted
 *   dropped [nview][nbody]     the body's pixels that were left out (below)
 * depth, seg [nview][H][W] are what the render returned for the same pose, shape_type, prm, cam, intrinsics and grids; g_depth
 * [nview][H][W] is the adjoint of depth.  The hit point is recomputed as o + t d_w; nothing is traced again.  For a body with a
 * grid (type DSS_SHAPE_GRID, and DSS_SHAPE_IGR seen through its value grid) grad_p phi is the gradient of the trilinear
 * interpolant in the hit's cell, the field whose zero the renderer's cell walk finds.
 *
 * This is the derivative of the visible surface at fixed visibility: the motion of a silhouette (a pixel that changes the body
 * it sees, or from hit to miss) is not modelled.  Pixels that contribute nothing: seg < 0 (no hit, or -2) or >= nbody, whatever
 * g_depth holds there; and, counted in `dropped`, a body's pixels whose hit point is not inside the body's query cube or whose
 * cosine of incidence |n_w . d_w| / (|n_w| |d_w|) is below min_cos (or not a number).
 *
 * Launch: the renderer's (a pixel per lane, a 16 x 16 tile per 256-thread workgroup); the view's bodies with their
 * dual-number shapes are built once per workgroup in LDS.  Pose and parameter terms take no atomics: per workgroup and body
 * they are reduced over the lanes whose seg is that body into a partial in the workspace, and a second kernel adds a (view,
 * body)'s partials in a fixed order -- two calls return the same bits.  The samples take fp64 global atomic adds: two calls
 * agree to the rounding of the sums, not in their bits.
 *
 * grid_id [nview][nbody], ngrid, grid_off, grid_dims, grid_data: the pooled table of dss_depth_render_grids; grid_id NULL and
 * ngrid 0: no grids.  workspace: dss_depth_adjoint_workspace_bytes(nview, nbody, W, H) bytes (0 for arguments the call refuses).
 * DSS_E_BADARG: a count < 1, a null pointer (grids, g_grid and stream aside), fx or fy 0, min_cos not in [0, 1], a grid id >=
 * ngrid, a dim < 2.  DSS_E_UNSUPPORTED: more than 8 bodies, images beyond 2^31 - 1 pixels, brick, bowl, a grid or neural body
 * without a grid.  DSS_E_WORKSPACE: the workspace is too small.  Nothing is launched and nothing written on any of them. */
size_t dss_depth_adjoint_workspace_bytes(int nview, int nbody, int W, int H);
int dss_depth_adjoint(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam, double fx,
                      double fy, double cx, double cy, int W, int H, const double *depth, const int *seg, const double *g_depth,
                      double min_cos, const int *grid_id, int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data,
                      double *g_pose, double *g_prm, double *g_grid, int *dropped, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
