// depth_camera.h -- C ABI of the depth camera (csrc/depth_camera.hip), exported by libdiffsdfsim_hip.so beside the functions
// of include/diffsdfsim_hip.h, whose conventions it shares (device pointers into caller-owned memory, double = binary64
// row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).  Bound by world_abi.OPTIONAL_PROTOTYPES;
// diffsdfsim_amd/depth_camera.py raises if the library does not export it.
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
