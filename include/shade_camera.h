// shade_camera.h -- C ABI of the colour camera (csrc/shade_camera.hip), exported by libdiffsdfsim_hip.so beside the depth
// camera's (depth_camera.h), whose conventions it shares.  Part of the checked ABI: bound by world_abi.PROTOTYPES, which
// tests/test_abi.py holds to these declarations.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Deferred shading of depth / segment images that dss_depth_render or dss_depth_render_grids produced for the same views:
 * the surface normal at every hit, Lambert shading by up to four directional lights with hard shadows, the body's colour.
 * The views are described as for dss_depth_render_grids (pose, shape_type, prm, cam, fx .. cy, W, H, zfar and the pooled
 * grids; ngrid = 0: no grids, the grid pointers are not read).  Further inputs:
 *   depth [nview][H][W], seg [nview][H][W]   the images to shade
 *   color [nview][nbody][3]                  the bodies' colours, doubles in [0, 1]
 *   light [nlight][4], nlight in 0..4        the world direction TOWARDS the light (any length > 0; normalised here) and the
 *                                            light's intensity
 *   ambient, background [3] (host memory: three doubles read by the call), shadows (0 / 1), shadow_bias > 0 (world units)
 * Per pixel, mapped to threads as in dss_depth_render (an 8 x 8 tile per wavefront, the view's tables in LDS):
 *   seg outside [0, nbody) (-1, -2, anything else): normal = 0, shade = 0, rgb = round(255 background), flags = 0; the body
 *   table is not indexed with such a value.
 *   Otherwise x = o + depth d on the pixel's ray, p = R^T (x - pos) clamped to the body's query cube, and the body-frame normal
 *     analytic body        the gradient query_sdf returns;
 *     grid / neural body   the gradient of the trilinear interpolant of the cell that holds p, from the cell's eight corners,
 *                          per axis divided by the cell's size, normalised;
 *     shorter than 1e-300  the negated unit ray direction instead, flags bit 1.
 *   n = R n_b.  For light k: c_k = n . l_k; where c_k > 0 and shadows is set, a shadow ray from x + shadow_bias n along l_k
 *   through every body of the view, the hit body included: slab test over [0, zfar], then the depth camera's own trace of that
 *   body.  The first body that reports a hit ends the search with V_k = 0; a trace that uses up its iteration cap counts as no
 *   hit and sets flags bit 0.  Without shadows V_k = 1.
 *   shade = min(1, ambient + sum_k I_k V_k max(0, c_k)),  rgb_c = (unsigned char) floor(255 color_c shade + 0.5).
 * Outputs: normal [nview][H][W][3] and shade [nview][H][W] (double), rgb [nview][H][W][3] and flags [nview][H][W] (unsigned char).
 * No atomics: every output is a function of the inputs alone, two calls return the same bits.
 * DSS_E_BADARG: a null pointer, a non-positive size, nlight outside 0..4, shadow_bias <= 0, ngrid < 0, a grid id >= ngrid,
 * a grid dim < 2.
 * DSS_E_UNSUPPORTED, every output untouched: nbody > 8, a brick or a bowl, a grid or neural body without a grid, images with
 * more than 2^31 - 1 pixels.  As in the depth camera the host reads shape_type (and grid_id, grid_dims) and waits for the
 * stream before it enqueues. */
int dss_shade_render(int nview, int nbody, const double *pose, const int *shape_type, const double *prm, const double *cam,
                     double fx, double fy, double cx, double cy, int W, int H, double zfar, const int *grid_id, int ngrid,
                     const int *grid_off, const int *grid_dims, const double *grid_data, const int *blk_off, const double *blk_min,
                     const double *depth, const int *seg, const double *color, int nlight, const double *light, double ambient,
                     const double *background, int shadows, double shadow_bias, double *normal, double *shade, unsigned char *rgb,
                     unsigned char *flags, void *stream);

#ifdef __cplusplus
}
#endif
