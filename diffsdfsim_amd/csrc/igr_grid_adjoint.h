// igr_grid_adjoint.h -- C ABI of the chain from a neural (decode_igr) body's value grid to its latent code
// (csrc/igr_grid_adjoint.hip), exported by libdiffsdfsim_hip.so beside the functions of include/*.h, whose conventions it shares
// (device pointers into caller-owned memory, double = binary64 row-major, int = int32, stream = hipStream_t as void*, DSS_E_*
// return codes).  Bound by world_abi.OPTIONAL_PROTOTYPES; diffsdfsim_amd/igr.py (igr_lattice_values) is the caller.
#pragma once
#include <stddef.h>

#include "../../include/diffsdfsim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Grid g of a pooled table (grid_off [ngrid], grid_dims [ngrid][3], the layout of grids.GridTable: x slowest) holds the values
 * v[i] = f(x_i; z) of the network `net` with the latent code z = latents[lat_idx[g] * lat_stride : + L] (L = the network's latent
 * size) at the nodes of the lattice over [-1, 1]^3: sample (i0, i1, i2) lies at
 *
 *     u_k = fma((double)i_k, 2.0 / (double)(n_k - 1), -1.0)          (the step rounded once, then one fused multiply-add)
 *
 * which is torch.linspace(-1, 1, n_k)[i_k] up to an ulp or two of rounding.  g_grid, pooled like the table's data, is the adjoint of
 * those values (what dss_depth_adjoint and dss_pointcloud_loss_grids_adjoint return), and the call writes
 *
 *     g_latent[r][l] = sum over the grids g with lat_idx[g] == r, over their samples i:  g_grid[i] * d f(x_i; z) / d z_l
 *
 * for every row r < nlat ([nlat][DSS_IGR_LATENT_MAX]; written, not added to; slots l >= L and rows that no grid names are exactly
 * 0, and such a row's code is not read).  A grid with lat_idx[g] < 0 is not a neural grid: it is skipped and its g_grid is not read.
 *
 * g_grid is sparse (the corners of the cells that a visible hit fell into), and the network is the cost, so the non-zero samples
 * are compacted first and the MFMA kernel of igr_mlp.hip walks the compacted list alone.  Stages on `stream`:
 *   count    one 256-thread workgroup per (neural grid, 2048 consecutive samples), grid-major: ballot + popcount of the samples
 *            with !(g == 0) -- a NaN counts, so it propagates into g_latent instead of vanishing
 *   scan     one workgroup: exclusive prefix of the chunk counts; the total goes to n_nodes[0], unclamped
 *   (host)   reads n_nodes[0]: THE CALL BLOCKS until the stream has drained and cannot be captured into a graph; in return the
 *            network's launch shape follows the list, and an empty list launches no network.  total > cap: DSS_E_WORKSPACE is
 *            returned with n_nodes written and g_latent untouched -- call again with cap >= n_nodes[0]
 *   emit     (the chunks with a non-zero count: g_grid is read densely once, and a second time where it carries weight)
 *            slot = the chunk's offset + the non-zero samples before it in index order: (u, the grid's latent row, the weight g)
 *   network  DSS_IGR_LATENT over the list (two passes of its own for L = 4)
 *   reduce   per chunk, sum of weight * d f / d z_l over its entries: wavefront butterfly, fixed tree over the four wavefronts
 *   sum      per latent row, the chunk partials of its grids added in list (grid-major) order
 * No atomics: two calls on the same input return the same bits.
 *
 * The dims and lat_idx tables decide the status and the launch shapes, so the host reads them before anything is launched (a
 * first, short wait, as dss_depth_adjoint reads its tables); grid_off is not checked.
 * workspace: dss_igr_grid_adjoint_workspace_bytes(nsamples, cap, nlat) bytes, nsamples = the samples of all grids together (0 for
 * arguments the call refuses); it is a bound that holds however the samples are split into grids: the signature carries no
 * ngrid, a grid has at least 8 samples, and so the bound allows for nsamples / 2048 + nsamples / 8 chunks of 40 bytes each (a
 * partial, a count, an offset) -- about 10 MB for a 128^3 grid that uses 1024 chunks.  The call itself checks workspace_bytes
 * against the chunks the tables name, so a caller that knows its grids may pass less.
 * DSS_E_BADARG: a null pointer (stream aside; net's six pointers included), ngrid, nlat or cap < 1, lat_stride < L, a dim < 2, a
 * lat_idx >= nlat.  DSS_E_UNSUPPORTED: a network shape no kernel is built for, a grid of more than 2^31 - 1 - 2048 samples, 4 * cap past
 * an int.  DSS_E_WORKSPACE: the workspace is smaller than the call needs (n_nodes is not written), or the list is longer than cap
 * (n_nodes is written).  On BADARG, UNSUPPORTED and a workspace that is too small nothing is launched and nothing written. */
size_t dss_igr_grid_adjoint_workspace_bytes(int nsamples, int cap, int nlat);
int dss_igr_grid_adjoint(const DssIgrNet *net, int ngrid, const int *grid_off, const int *grid_dims,
                         const int *lat_idx /*[ngrid] row of `latents`; < 0: not a neural grid, skipped*/,
                         const double *latents, int lat_stride, int nlat, const double *g_grid /*pooled like GridTable.data*/,
                         int cap /*capacity of the compacted node list*/, double *g_latent /*[nlat][DSS_IGR_LATENT_MAX]*/,
                         int *n_nodes /*[1] device: non-zero nodes found, unclamped*/, void *workspace, size_t workspace_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
