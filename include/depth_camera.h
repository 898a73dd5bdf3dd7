// depth_camera.h -- C ABI of the depth camera (csrc/depth_camera.hip), exported by libdiffsdfsim_hip.so beside the functions
// of diffsdfsim_hip.h, whose conventions it shares (device pointers into caller-owned memory, double = binary64
// row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).  Part of the checked ABI: bound by
// world_abi.PROTOTYPES, which tests/test_abi.py holds to these declarations.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Ray-cast depth and segment images of nview views (a view = one scene at one frame) of nbody <= 8 SDF bodies each, all seen
 * by one pinhole camera: what Recorder3D(record_points=True, record_seg=True) records (sdf_physics/physics3d/utils.py), with
 * the bodies' exact surfaces in place of pyrender's triangles.
 *   pose [nview][nbody][7] (quaternion wxyz + position), shape_type [nview][nbody], prm [nview][nbody][4] (three shape
 *   parameters + the corner radius), cam [16] the camera-to-world matrix (row-major 4 x 4, OpenGL convention: the camera looks
 *   along its -z, +y is up; the upper 3 x 3 block a rotation), on the device like the rest.
 * The ray of pixel (row, col) starts at the camera's centre and runs along the camera-frame direction (nx, -ny, -1) t,
 * nx = (col + 0.5 - cx) / fx, ny = (row + 0.5 - cy) / fy: the ray Recorder3D.get_pointcloud back-projects along, so a hit at
 * parameter t has depth t along the optical axis.  Per body the ray is clipped against the query cube |p| <= scale of the
 * body frame (slab test) and sphere-traced through query_sdf from the entry point (not before znear) until phi <= 1e-10
 * (a hit), or it leaves the cube, passes zfar or passes the nearest hit so far (a miss).  A step is phi / |direction| or,
 * where longer, the step to the zero of the line through the last two samples: the bodies are convex, so neither passes
 * the surface, and a hit at cosine c of incidence lies within 1e-10 / c before the true one.  The nearest hit wins, ties go
 * to the lower body index.
 *   depth [nview][H][W]   depth of the hit, 0 where nothing is hit within [znear, zfar]
 *   seg   [nview][H][W]   index of the body hit, -1 for none, -2 (with depth 0) for a pixel one of whose traces used up its
 *                         512 iterations
 * No atomics: two calls on the same input return the same bits.  Boxes, spheres, cylinders and rounded boxes only (the fields
 * that are Euclidean distances, so the trace cannot overshoot): any other shape_type gives DSS_E_UNSUPPORTED and leaves the
 * outputs untouched.  The status depends on shape_type, so the call copies those nview * nbody ints to the host and waits
 * for the stream before it enqueues its kernel, as dss_pointcloud_loss does. */
int dss_depth_render(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam,
                     double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar, double *depth,
                     int *seg, void *stream);

/* Voxel-grid bodies in the camera.  The grids are pooled as in DssWorld: grid_off [ngrid] (offset of grid g's samples in
 * grid_data, in doubles), grid_dims [ngrid][3] (n0, n1, n2 >= 2 samples per axis, x slowest), grid_data.  Grid g's field at the
 * body-frame point p is scale * trilinear(samples) at index position (p / scale + 1) / 2 * (n_d - 1), the cell index clamped
 * to [0, n_d - 2]: the value of geom.h's SHAPE_GRID branch (scale = prm[3] of the body).
 *
 * dss_grid_block_min: for every block of DSS_GRID_BLOCK cells per axis (the last block of an axis may be partial) the least of
 * the block's corner samples (up to 5 x 5 x 5).  Grid g has prod_d ceil((n_d - 1) / DSS_GRID_BLOCK) blocks, x slowest;
 * blk_off [ngrid] are the caller's prefix sums of those counts, nblk their total, blk_min [nblk] the output.  The interpolant is
 * a convex combination of a cell's corners, so a block whose minimum is positive holds no point of the surface -- for any
 * samples; nothing is assumed about their Lipschitz constant. */
#define DSS_GRID_BLOCK 4
int dss_grid_block_min(int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off, int nblk,
                       double *blk_min, void *stream);

/* dss_depth_render with grid bodies: grid_id [nview][nbody], the grid of a body of type DSS_SHAPE_GRID or DSS_SHAPE_IGR (a neural
 * body is seen through the value grid its mesh is extracted from), read for those two types only.  Types 0-3 are traced as in
 * dss_depth_render, by the same code.  A grid body's ray is clipped against the query cube like any other, taken into index
 * coordinates and walked cell by cell (a 3-D DDA on two levels: a block whose blk_min is positive is left in one step).  Every
 * plane crossing comes from the plane's integer index, t = (k - x0_d) / dx_d, so the walk visits at most n0 + n1 + n2 cells: a
 * grid trace has no iteration cap and never gives seg = -2.  In a cell the 8 corners are loaded once and the interpolant is
 * evaluated at the parameters where the ray enters and leaves it.
 *   - the value at the slab entry is <= 0: a hit there;
 *   - otherwise the first cell with entry value > 0 and exit value <= 0 holds the hit: bisection on the 8 corners until the
 *     bracket is 4 ulp of t wide (at most 60 halvings), the end whose value is <= 0 is returned;
 *   - a dip below zero strictly inside ONE cell, both ends positive (the ray clips a corner of the surface within a cell), is
 *     not a hit: such a sliver is thinner than a cell, below the grid's resolution, as it is for marching cubes, whose
 *     triangles replace the interpolant's surface within a cell by planes.
 * Nearest hit, ties and outputs as in dss_depth_render; no atomics, the same bits in every call.  Brick, bowl, and a grid or
 * neural body with grid_id = -1 give DSS_E_UNSUPPORTED and leave the outputs untouched; a grid_id >= ngrid or a dim < 2 gives
 * DSS_E_BADARG.  The host reads shape_type, grid_id and grid_dims (and waits for the stream) before it enqueues; when no body
 * has a grid it enqueues dss_depth_render's own kernel. */
int dss_depth_render_grids(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam,
                           double fx, double fy, double cx, double cy, int W, int H, double znear, double zfar, const int *grid_id,
                           int ngrid, const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off,
                           const double *blk_min, double *depth, int *seg, void *stream);

/* The observed points of body `body` in nview depth / segment images: lines 168-187 of match_pointcloud
 * (experiments/trajectory_fitting/optim_pointcloud.py).  A pixel is selected if it and its four edge neighbours have
 * seg == body (scipy.ndimage.binary_erosion with its default structure; beyond the image border counts as unset) and its
 * depth is not 0; it gives the world-frame point cam (nx d, -ny d, -d, 1), nx and ny as above.  Points come in row-major pixel
 * order per view, views one after the other.
 *   dss_depth_points_count   row_count [nview * H]: the selected pixels of each image row
 *   dss_depth_points_emit    row_off [nview * H]: the exclusive prefix sum of row_count, made by the caller; pts [N][3], N its
 *                            total.  View v owns pts[row_off[v * H] : row_off[(v + 1) * H]] (N for the last view).
 * A wavefront per image row, ballot and prefix popcount; no atomics, the same bits in every call.  `depth` is an input (it may
 * carry noise added after the rendering). */
int dss_depth_points_count(int nview, int H, int W, int body, const double *depth, const int *seg, int *row_count, void *stream);
int dss_depth_points_emit(int nview, int H, int W, int body, const double *depth, const int *seg, const int *row_off,
                          const double *cam, double fx, double fy, double cx, double cy, double *pts, void *stream);

#ifdef __cplusplus
}
#endif
