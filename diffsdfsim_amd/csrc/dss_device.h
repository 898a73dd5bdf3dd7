// dss_device.h -- the single include through which kernels see the HIP device API.
// Product builds (hipcc, gfx950) get <hip/hip_runtime.h>.  tests/emu compiles the same sources
// with g++ -DDSS_EMU to debug kernel logic on the CPU-only build container (tests/emu/README.md);
// that build is test infrastructure and is never loaded by the product.
#pragma once
#if defined(DSS_EMU)
#include "hip_emu.h"
// lanes of one emulated wavefront meet at every switch point
inline void dss_wave_sync() { dss_emu::yield(); }
inline int dss_uniform(int x) { return x; }
inline int dss_opaque(int x) { return x; }
inline double dss_rcp(double x) { return 1.0 / x; }
inline double dss_uniform(double x) { return x; }
template <int CTRL> __device__ __forceinline__ double dss_dpp_mov(double x)
{
    const int l = threadIdx.x & 63, q = l & ~3, i = l & 3;
    const int src = CTRL == 0x141 ? (l & ~7) | (7 - (l & 7)) : q | ((CTRL >> (2 * i)) & 3);
    return __shfl(x, src, 64);
}
template <int CTRL> __device__ __forceinline__ int dss_dpp_movi(int x)
{
    const int l = threadIdx.x & 63, q = l & ~3, i = l & 3;
    const int src = CTRL == 0x141 ? (l & ~7) | (7 - (l & 7)) : q | ((CTRL >> (2 * i)) & 3);
    return __shfl(x, src, 64);
}
template <int J> __device__ __forceinline__ double dss_gbc(double x) { return __shfl(x, (threadIdx.x & (64 - 8)) | J, 64); }
__device__ __forceinline__ double dss_wave_bcast(double x, int src_uniform) { return __shfl(x, src_uniform, 64); }
__device__ inline double dss_wave_first(double x) { return __shfl(x, 0, 64); }
#else
#include <hip/hip_runtime.h>

#include <vector>
#define DSS_DYN_LDS(type, name) extern __shared__ __align__(16) type name[]
// LDS written by one lane is visible to the other lanes of the SAME wavefront afterwards (no s_barrier: the LDS
// queue of a wavefront is in order; the fence only stops the compiler from moving accesses across)
__device__ __forceinline__ void dss_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the value, hidden from the optimiser (stops loop-invariant code motion of everything computed from it)
__device__ __forceinline__ int dss_opaque(int x) { asm volatile("" : "+v"(x)); return x; }
// 1 / x to within an ulp or two: v_rcp_f64 and two Newton steps (for arguments well inside the normal range)
__device__ __forceinline__ double dss_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
    return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}
// a value every lane of the wavefront agrees on, moved to scalar registers
__device__ __forceinline__ int dss_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double dss_uniform(double x)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// value of lane 0, for every lane (readfirstlane takes the first ACTIVE lane: lane 0 where the whole wavefront runs)
__device__ inline double dss_wave_first(double x) { return dss_uniform(x); }
// value of lane `src_uniform` (the same number in every lane), through scalar registers
__device__ __forceinline__ double dss_wave_bcast(double x, int src_uniform)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src_uniform);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src_uniform);
    return __hiloint2double(hi, lo);
}
// Cross-lane moves with COMPILE-TIME partners on the DPP path of the vector ALU (a few cycles, against > 100 for ds_bpermute /
// ds_swizzle through the LDS crossbar).  CTRL: a quad_perm pattern (partners inside a quad) or row_half_mirror (0x141: lane
// i <-> 7 - i of every 8).
template <int CTRL> __device__ __forceinline__ int dss_dpp_movi(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ double dss_dpp_mov(double x)
{
    return __hiloint2double(dss_dpp_movi<CTRL>(__double2hiint(x)), dss_dpp_movi<CTRL>(__double2loint(x)));
}
// broadcast of lane J of every group of eight, J a compile-time constant.  gfx90a+ moves 64 bits per DPP instruction with the
// row_newbcast controls (lane N of every row of 16 to the whole row); a row holds two groups, told apart by the bank mask
// (banks 0-1 = lanes 0-7, banks 2-3 = lanes 8-15): two instructions per double.
template <int J> __device__ __forceinline__ double dss_gbc(double x)
{
    const double lo = __builtin_amdgcn_update_dpp(x, x, 0x150 + J, 0xf, 0x3, false);          // lanes 8-15 of the row keep x for now
    return __builtin_amdgcn_update_dpp(lo, x, 0x150 + 8 + J, 0xf, 0xc, false);
}
#endif

// Ints of device memory that decide a status or a launch shape, read by the host before it enqueues more.  copy() enqueues the
// read on the stream (false where the runtime refused the pointer); after host_sync(), the call's one wait, p holds the values.
// The emulator's device memory is the host's: p is the pointer itself and there is nothing to wait for.
struct HostInts {
    const int *p = nullptr;      // (stays NULL without a copy)
#if defined(DSS_EMU)
    bool copy(const int *dev, size_t, hipStream_t) { p = dev; return true; }
#else
    int one;      // (a single int, such as a list's length, needs no allocation)
    std::vector<int> own;
    bool copy(const int *dev, size_t n, hipStream_t st)
    {
        int *host = &one;
        if (n > 1) { own.resize(n); host = own.data(); }
        p = host;
        return hipMemcpyAsync(host, dev, sizeof(int) * n, hipMemcpyDeviceToHost, st) == hipSuccess;
    }
#endif
};
#if defined(DSS_EMU)
inline bool host_sync(hipStream_t) { return true; }
#else
inline bool host_sync(hipStream_t st) { return hipStreamSynchronize(st) == hipSuccess; }
#endif

// A big by-value kernel argument (DssWorld, ~1 KB) whose address is handed to non-inlined device functions is copied by the
// compiler into every lane's private scratch memory (64 KB per wavefront of stores at kernel entry, and every later field
// access a scratch load).  Referring to it where it already lies -- the kernarg segment, readable by every lane -- avoids the
// copy.  `arg` must be the kernel's FIRST parameter (offset 0 of the segment).
#if defined(DSS_EMU)
#define DSS_KERNARG_REF(T, name, arg) const T &name = arg
#define DSS_KERNARG_REF_AT(T, name, arg, offset) const T &name = arg
#else
#define DSS_KERNARG_REF(T, name, arg) const T &name = *(const T *)__builtin_amdgcn_kernarg_segment_ptr(); (void)arg
// a later parameter: `offset` = its byte offset in the segment (parameters are laid out in order at their natural alignment)
#define DSS_KERNARG_REF_AT(T, name, arg, offset) \
    const T &name = *(const T *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + (offset)); (void)arg
#endif
