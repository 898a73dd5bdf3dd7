// shape_args.h -- what every launcher whose status depends on the bodies' shape types refuses after its null, size and workspace
// checks, stated once ("Shared scene judge and camera launch shape"): the point-cloud losses (pointcloud_loss.hip,
// pointcloud_loss_grid_adj.hip) and the cameras (depth_camera.hip, shade_camera.hip, depth_adjoint.hip).  Host code only.
#pragma once
#include "../../include/diffsdfsim_hip.h"
#include "dss_device.h"

namespace dss {

// sets of shape types, a bit per DSS_SHAPE_*
constexpr unsigned SHAPES_CONVEX = 0x0f;        // box, sphere, cylinder, rounded box: what the cameras trace
constexpr unsigned SHAPES_ANALYTIC = 0x3f;      // those, brick and bowl: what the point-cloud losses evaluate
constexpr unsigned SHAPES_GRID = 1u << DSS_SHAPE_GRID, SHAPES_GRID_IGR = SHAPES_GRID | 1u << DSS_SHAPE_IGR;
inline bool shape_in(unsigned set, int type) { return type >= 0 && type < 32 && (set >> type & 1u); }

// The status that n bodies' shape types and, with a grid table, their grid ids and the grids' dims decide; *any_level_set: a body
// of a type in `level_sets` exists.  The host reads shape_type, grid_id where it is not NULL and grid_dims where ngrid > 0, and
// waits for `st` once, so nothing is enqueued by a refused call:
//   DSS_E_BADARG       a read failed, or a dim < 2
//   then per body in index order:
//   DSS_E_BADARG       a body of a type in `level_sets` whose id >= ngrid
//   DSS_E_UNSUPPORTED  one without an id (grid_id NULL, or id < 0: a level-set body without a grid), or a type that is in neither
//                      `level_sets` nor `analytic`
// (an analytic body's id is not judged).
inline int judge_shapes(size_t n, const int *shape_type, unsigned analytic, unsigned level_sets, const int *grid_id, int ngrid,
                        const int *grid_dims, hipStream_t st, bool *any_level_set = nullptr)
{
    HostInts host_types, host_ids, host_dims;
    if (!host_types.copy(shape_type, n, st) || (grid_id && !host_ids.copy(grid_id, n, st)) ||
        (ngrid > 0 && !host_dims.copy(grid_dims, 3 * (size_t)ngrid, st)) || !host_sync(st))
        return DSS_E_BADARG;
    const int *types = host_types.p, *ids = host_ids.p, *dims = host_dims.p;
    for (int g = 0; g < 3 * ngrid; ++g)
        if (dims[g] < 2) return DSS_E_BADARG;
    bool any = false;
    for (size_t i = 0; i < n; ++i) {
        if (shape_in(level_sets, types[i])) {
            if (ids && ids[i] >= ngrid) return DSS_E_BADARG;
            if (!ids || ids[i] < 0) return DSS_E_UNSUPPORTED;
            any = true;
        } else if (!shape_in(analytic, types[i])) {
            return DSS_E_UNSUPPORTED;
        }
    }
    if (any_level_set) *any_level_set = any;
    return DSS_OK;
}

}  // namespace dss
