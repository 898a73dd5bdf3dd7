// pointcloud_args.h -- what the point-cloud loss launchers (pointcloud_loss.hip, pointcloud_loss_grid_adj.hip) refuse after their
// null and workspace checks, stated once.  Host code only.
#pragma once
#include "../../include/diffsdfsim_hip.h"
#include "dss_device.h"

namespace dss {

// The status that the segments' shape types and, with a grid table (grid_id != nullptr), their grid ids and the grids' dims
// decide; *any_grid: a DSS_SHAPE_GRID segment exists.  The host reads the three arrays first (and waits for `st`), so nothing
// is enqueued by a refused call:
//   DSS_E_BADARG       the read failed, or a dim < 2
//   then per segment in index order, with a table:
//   DSS_E_BADARG       a DSS_SHAPE_GRID segment whose id >= ngrid
//   DSS_E_UNSUPPORTED  one whose id < 0 (a grid body without a grid), or a type that is neither 0-5 nor DSS_SHAPE_GRID (neural bodies)
//   without a table:   DSS_E_UNSUPPORTED for every type outside 0-5
inline int pc_judge_segments(int nseg, const int *shape_type, const int *grid_id, int ngrid, const int *grid_dims, hipStream_t st,
                             bool *any_grid = nullptr)
{
    HostInts host_types, host_ids, host_dims;
    if (!host_types.copy(shape_type, nseg, st) || (grid_id && !host_ids.copy(grid_id, nseg, st)) ||
        (ngrid > 0 && !host_dims.copy(grid_dims, 3 * (size_t)ngrid, st)) || !host_sync(st))
        return DSS_E_BADARG;
    const int *types = host_types.p, *ids = host_ids.p, *dims = host_dims.p;
    for (int g = 0; g < 3 * ngrid; ++g)
        if (dims[g] < 2) return DSS_E_BADARG;
    bool any = false;
    for (int s = 0; s < nseg; ++s) {
        if (ids && types[s] == DSS_SHAPE_GRID) {
            if (ids[s] >= ngrid) return DSS_E_BADARG;
            if (ids[s] < 0) return DSS_E_UNSUPPORTED;
            any = true;
        } else if (types[s] < DSS_SHAPE_BOX || types[s] > DSS_SHAPE_BOWL) {
            return DSS_E_UNSUPPORTED;
        }
    }
    if (any_grid) *any_grid = any;
    return DSS_OK;
}

}  // namespace dss
