// diag_stamps.h -- wall-clock phase stamps (100 MHz) of the diagnostic build only: _lib.build(diag=True) compiles every
// source with -DDSS_DIAG (tools/lcp_phases.py, tools/np_phases.py).  A translation unit whose kernel is measured defines
// DSS_STAMPS to a short name before it includes this header and gets a device stamp pointer, NULL until the exported
//   void dss_diag_set_<name>_stamps(long long *p, void *stream)
// sets it, and the macros
//   DSS_STAMP(lead, at)       the lane for which `lead` holds writes the wall clock to p[at]
//   DSS_STAMP_INIT            declares the running time of DSS_STAMP_ADD
//   DSS_STAMP_ADD(lead, at)   the lane for which `lead` holds adds the time since the previous DSS_STAMP_ADD to p[at]
// Without DSS_DIAG or DSS_STAMPS they compile to nothing: the product library has no global state.
#pragma once
#include "dss_device.h"

#if defined(DSS_DIAG) && defined(DSS_STAMPS) && !defined(DSS_EMU)
namespace {
__device__ long long *g_dss_stamps = nullptr;
__global__ void dss_set_stamps_kernel(long long *p) { g_dss_stamps = p; }
}  // namespace
#define DSS_STAMPS_SETTER_(name) dss_diag_set_##name##_stamps
#define DSS_STAMPS_SETTER(name) DSS_STAMPS_SETTER_(name)
extern "C" void DSS_STAMPS_SETTER(DSS_STAMPS)(long long *p, void *stream)
{
    hipLaunchKernelGGL(dss_set_stamps_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p);
}
#define DSS_STAMP(lead, at) do { if (g_dss_stamps && (lead)) g_dss_stamps[at] = wall_clock64(); } while (0)
#define DSS_STAMP_INIT long long dss_t_last = wall_clock64()
#define DSS_STAMP_ADD(lead, at) do { \
    if (g_dss_stamps && (lead)) atomicAdd((unsigned long long *)&g_dss_stamps[at], (unsigned long long)(wall_clock64() - dss_t_last)); \
    dss_t_last = wall_clock64(); } while (0)
#else
#define DSS_STAMP(lead, at) do { } while (0)
#define DSS_STAMP_INIT do { } while (0)
#define DSS_STAMP_ADD(lead, at) do { } while (0)
#endif
