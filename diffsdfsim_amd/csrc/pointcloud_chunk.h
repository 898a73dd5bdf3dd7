// pointcloud_chunk.h -- the launch shape of the point-cloud loss kernels (pointcloud_loss.hip, pointcloud_loss_grid_adj.hip):
// 256-thread workgroups, one workgroup per (segment, chunk of PC_CHUNK consecutive points of the segment) in a flat grid of
// nseg * chunks, segment-major; one lane per point in a strided loop over the chunk.
#pragma once
#include "dss_device.h"

namespace dss {

constexpr int PC_THREADS = 256, PC_CHUNK = 2048;

inline int pc_chunks(int max_seg_len) { return (max_seg_len + PC_CHUNK - 1) / PC_CHUNK; }

// the chunk of workgroup blockIdx.x: -> false if it holds nothing of its segment
__device__ __forceinline__ bool pc_chunk(int max_seg_len, int chunks, const int *__restrict__ seg_off, int &s, int &first, int &lo, int &hi)
{
    s = blockIdx.x / chunks;
    const int chunk = blockIdx.x - s * chunks;
    first = seg_off[s];
    int len = seg_off[s + 1] - first;
    if (len > max_seg_len) len = max_seg_len;      // the workspace was sized for max_seg_len
    lo = chunk * PC_CHUNK;
    if (lo >= len) return false;                    // (the whole workgroup: nothing of this segment in the chunk)
    hi = lo + PC_CHUNK < len ? lo + PC_CHUNK : len;
    return true;
}

}  // namespace dss
