// mesh_grid.h -- C ABI of the mesh voxeliser (csrc/mesh_grid.hip): the exact signed distance of closed triangle meshes on
// the samples of voxel grids, exported by libdiffsdfsim_hip.so beside the functions of include/*.h, whose conventions it shares
// (device pointers into caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_*
// return codes).  Bound by world_abi.OPTIONAL_PROTOTYPES; diffsdfsim_amd/mesh_grid.py is the caller.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

/* DSS_MESH_GRID_TILE       triangles per LDS tile = threads per workgroup: every thread stages one triangle of a tile
 *                          (diffsdfsim_amd/mesh_grid.py mirrors it as TILE; tests/test_emu_mesh_grid.py compares the two)
 * DSS_MESH_GRID_MALFORMED  status word of a mesh one of whose faces names a vertex outside [0, nv), or that has no face */
#define DSS_MESH_GRID_TILE 256
#define DSS_MESH_GRID_MALFORMED 1

/* Voxelise nmesh meshes into a pooled grid buffer of grids.GridTable's layout (off, dims, data).  Mesh m owns the vertices
 * verts[vert_off[m] : vert_off[m + 1]] ([.,3] rows) and the faces faces[face_off[m] : face_off[m + 1]] ([.,3] rows of vertex
 * numbers relative to vert_off[m], at most max_faces of them are read), and the grid of grid_dims[m] = (n0, n1, n2), every
 * entry >= 2, whose samples are grid_data[grid_off[m] : grid_off[m] + n0 n1 n2], x slowest (at most max_samples are written).
 *
 * Sample (i, j, k) sits at the body-frame point x = scale[m] * (-1 + 2 i / (n0 - 1), -1 + 2 j / (n1 - 1), -1 + 2 k / (n2 - 1))
 * and receives sign * dist / scale[m]:
 *   dist  the Euclidean distance from x to the nearest triangle: the closest point of each triangle by vertex, edge and face
 *         region, the least squared distance over the faces, one square root at the end;
 *   sign  -1 where the generalised winding number w = (1 / 4 pi) sum_f 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| +
 *         (b . c)|a| + (c . a)|b|) (a, b, c the corners minus x, the sum in face order) exceeds 1/2, else +1.
 * A triangle whose squared area is at most 1e-20 |ab|^2 |ac|^2 (all three corners on one line to within 1e-10 rad) counts
 * as zero-area: its distance is the least of its three edges' and it adds no solid angle, so it yields no NaN.
 * A face that names a vertex outside [0, nv) is never dereferenced: it is left out and status[m] = DSS_MESH_GRID_MALFORMED;
 * so for a mesh without faces (whose samples then hold +inf) and for a grid with an entry of grid_dims below 2 or more than
 * 2^31 - 1 samples (which is not written).  status[m] = 0 otherwise.  Every status word is written.
 *
 * Launch: 256-thread workgroups, ceil(max_samples / 256) per mesh on a flat grid, one lane per sample along the last grid
 * axis, the faces streamed through LDS DSS_MESH_GRID_TILE at a time.  A workgroup walks its mesh's whole face list: the face
 * range is not divided among workgroups.  No atomics: every output is a function of the input alone, two calls return the
 * same bits.
 * DSS_E_BADARG: nmesh, max_samples or max_faces < 1, a null pointer (stream aside).  DSS_E_UNSUPPORTED: the lanes launched, nmesh *
 * ceil(max_samples / 256) * 256 -- which bound the grid and nmesh * max_samples, the end of the last grid of a packed pool and so
 * of every grid_off[m] + samples -- do not fit an int.  Nothing is launched and nothing written on either. */
int dss_mesh_grid_sdf(int nmesh, const double *verts, const int *faces, const int *vert_off, const int *face_off, const int *grid_dims,
                      const int *grid_off, const double *scale, int max_samples, int max_faces, double *grid_data, int *status,
                      void *stream);

#ifdef __cplusplus
}
#endif
