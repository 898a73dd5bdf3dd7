// wrap2d.h -- the turn test of the 2-D gift wrap, with the Qhull-calibrated measure of "collinear", stated once for the thinning
// stage of the 3-D narrow phase (np_common.h, the 2-D branch of its hull) and for the 2-D SDF contacts (sdf2d_contacts.hip).
// np_common.h's tree reduction over lanes keeps its own comparison: it also breaks exact ties by candidate number.
//
// Around the current hull vertex, (bx, by) is the offset of the best candidate so far and (qx, qy) that of a challenger.
// The challenger wins if it lies clockwise of the best by more than round-off, or is collinear with it and farther:
// "collinear" means that the nearer of the two clears the line through the farther by no more than dtol, a few ulps of the
// cluster's extent (Qhull merges facets flatter than that and keeps every vertex that sticks out more).
#pragma once
#include <math.h>

namespace dss {
__host__ __device__ inline bool wrap2_better(double bx, double by, double qx, double qy, double dtol2)
{
    const double cr = bx * qy - by * qx, lb = bx * bx + by * by, lq = qx * qx + qy * qy;
    const double c2 = cr * cr, t2 = dtol2 * fmax(lb, lq);
    return (cr < 0.0 && c2 > t2) || (c2 <= t2 && lq > lb);
}
// the tolerances of a cluster whose largest coordinate magnitude is amax: duplicates closer than tolf, collinear within dtol
__host__ __device__ inline double wrap2_tolf(double amax) { return 1e-12 * (1.0 + amax); }
__host__ __device__ inline double wrap2_dtol(double amax) { return 2e-14 * (1.0 + amax); }
}  // namespace dss
