// host_device.h -- the two macros of the *_device.h headers, which hold a kernel's per-element arithmetic and are read by hipcc for
// the library and by a plain host compiler for the stand-alone checks of tools/*_host_check.cpp.  It includes nothing of HIP.
#pragma once

#if defined(__HIPCC__)
#define NAF_HD __host__ __device__ __forceinline__
#define NAF_UNROLL _Pragma("unroll")
#else
#define NAF_HD inline
#define NAF_UNROLL
#endif
