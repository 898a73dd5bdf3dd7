// sdf2d_contacts.h -- C ABI of the 2-D SDF contact search (csrc/sdf2d_contacts.hip): the reference's SDFContactHandler
// (sdf_physics/physics/contacts.py:31-141) for a batch of body pairs, with its vector-Jacobian product.  Exported by
// libdiffsdfsim_hip.so beside the functions of diffsdfsim_hip.h, whose conventions it shares (device pointers into
// caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_* return codes).
// Part of the checked ABI: bound by world_abi.PROTOTYPES, which tests/test_abi.py holds to these declarations.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

/* body kinds and their two shape parameters: circle (rad, -), rect (width, height), bowl (r, d), grid (-, -) */
#define DSS_SDF2D_CIRCLE 0
#define DSS_SDF2D_RECT 1
#define DSS_SDF2D_BOWL 2
#define DSS_SDF2D_GRID 3
/* contacts of one pair before thinning that the kernel can hold (LDS: 76 bytes each) */
#define DSS_SDF2D_MAXCAND 256
/* bits of status[p] */
#define DSS_SDF2D_OVER_CAP 1   /* more contacts after thinning than `cap`: count[p] = the number needed, no row written   */
#define DSS_SDF2D_OVER_CAND 2  /* more than DSS_SDF2D_MAXCAND contacts before thinning: count[p] = 0, no row written        */
#define DSS_SDF2D_MALFORMED 4  /* unknown kind, grid id outside the table, edge index outside its outline: count[p] = 0     */

/* Pooled table of the grid bodies' data, all arrays on the device, the struct itself on the host.  Grid g has
 * dims[2 g], dims[2 g + 1] samples along body x and y (row-major, x slowest) starting at vals[val_off[g]], the central
 * differences of the samples (zero on the border; two numbers per sample) at grads[2 val_off[g]], its outline's vertices
 * (body frame, unit scale) verts[2 vert_off[g] .. 2 vert_off[g + 1]) and its edges (pairs of vertex numbers local to the
 * grid) edges[2 edge_off[g] .. 2 edge_off[g + 1]). */
typedef struct DssSdf2dGrids {
    int ngrids;
    const int *dims, *val_off, *vert_off, *edge_off, *edges;
    const double *vals, *grads, *verts;
} DssSdf2dGrids;

/* Contacts of npairs pairs.  Arrays are [2][npairs]...: body 1 of every pair, then body 2.
 *   kind, grid_id [2][P]; pose [2][P][3] = (angle, x, y); prm [2][P][2]; scale [2][P]; grids: NULL if no body is a grid.
 *   out [P][cap][7] = normal (2, from body 2 to body 1), p1 (2, offset from body 1's position), p2 (2, from body 2's),
 *     penetration: the tuples the reference appends to world.contacts, in candidate order (the edges of body 1 against the
 *     SDF of body 2 in edge order, then the edges of body 2 against body 1); rows >= count[p] are zero.
 *   count, status [P]; tag [P][cap][2] = (direction 0 / 1, edge) and tpar [P][cap] = the position of the contact along its
 *     edge, x = (1 - t) a + t b: what the backward pass needs to rebuild a contact without searching again.
 *   ncand [P], cand [P][cand_cap][7], cand_tag [P][cand_cap][2]: the contacts before thinning (the first cand_cap of
 *     them); all three may be NULL.
 * One 64-lane workgroup per pair; no allocation, no atomics, the caller's stream.
 * DSS_E_BADARG: npairs < 0, cap < 1, cand_cap < 0, a null array.  Nothing is launched then. */
int dss_sdf2d_contacts_forward(int npairs, int cap, const int *kind, const double *pose, const double *prm, const double *scale,
                               const int *grid_id, const DssSdf2dGrids *grids, double eps, double *out, int *count, int *status,
                               int *tag, double *tpar, int cand_cap, int *ncand, double *cand, int *cand_tag, void *stream);
/* gout [P][cap][7] (rows >= count ignored), count / tag / tpar as the forward left them -> g_pose [2][P][3], g_prm [2][P][2],
 * g_scale [2][P].  Every kept contact is recomputed on dual numbers at its fixed edge coordinate (to autograd the search is
 * a constant convex combination of the edge's end points).  The table is a constant to this call; the gradient with respect to
 * it is dss_sdf2d_contacts_backward_grids. */
int dss_sdf2d_contacts_backward(int npairs, int cap, const int *kind, const double *pose, const double *prm, const double *scale,
                                const int *grid_id, const DssSdf2dGrids *grids, const int *count, const int *tag,
                                const double *tpar, const double *gout, double *g_pose, double *g_prm, double *g_scale,
                                void *stream);
/* The same, and the gradient with respect to the table's three float arrays, taken as three independent inputs (the caller
 * chains grads and verts back to the samples):
 *   g_vals [sum n0 n1], g_grads [sum n0 n1][2], g_verts [sum nv][2], pooled like vals, grads and verts.  The call ADDS into
 *   them: the caller zeroes them.  g_pose, g_prm, g_scale are written, with the bits dss_sdf2d_contacts_backward writes.
 * For a kept contact rebuilt at its (direction, edge, t), with O the body whose edge it lies on and Q the body queried: if Q is
 * a grid, the four samples of the cell receive d / d value (the bilinear weight times the scale into phi) and d / d central
 * difference (through the normalisation; an interpolated gradient that is exactly zero is passed through unnormalised, as the
 * forward does); if O is a grid, the two end vertices of the edge receive d / d unit vertex, through the scale, the rotation
 * and the convex combination, including what the moved point changes in the query of Q.
 * One 64-lane workgroup per pair, 16 table entries per contact in four passes of dual numbers.  Within a pair the
 * contributions are added in contact order, entry by entry, by one lane; across pairs they meet in double-precision atomic
 * adds to global memory.  So g_vals, g_grads and g_verts are bit-reproducible only when no grid is shared between pairs of
 * the launch; with a shared grid two calls agree to round-off.  No allocation.
 * A pair whose count is outside 0..cap, a grid id or an edge index outside the table contribute nothing.
 * DSS_E_BADARG: as dss_sdf2d_contacts_backward, or g_vals, g_grads or g_verts null while `grids` holds a grid. */
int dss_sdf2d_contacts_backward_grids(int npairs, int cap, const int *kind, const double *pose, const double *prm, const double *scale,
                                      const int *grid_id, const DssSdf2dGrids *grids, const int *count, const int *tag,
                                      const double *tpar, const double *gout, double *g_pose, double *g_prm, double *g_scale,
                                      double *g_vals, double *g_grads, double *g_verts, void *stream);

#ifdef __cplusplus
}
#endif
