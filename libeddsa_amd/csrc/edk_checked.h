// edk_checked.h - the HIP calls of a verify pass that carry correctness (event records and stream waits that order the
// side stream against the caller's, the work-list reset, every launch) go through these macros: the first failure ends the
// pass and is returned (eddsa_amd.c: verify_on then waits for whatever was queued before the workspace is handed out again).
// edk_fault_tick() counts the checked calls and lets a test make the nth one fail (include/eddsa_amd_debug.h:
// eddsa_amd_debug_fail_hip_call; inert unless armed).  Host side of kernels.hip / rlc.hip only.
#pragma once
#include <hip/hip_runtime.h>

extern "C" int edk_fault_tick(void);   // kernels.hip: 1 when the armed fault falls on this call
// kernels.hip: k_verify_policy over the n verdicts ok[] of a pass (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*), one checked launch;
// policy 0 queues nothing.  Shared by edk_verify and edk_verify_rlc, which is why it is declared here and not in eddsa_kernels.h:
// the host library never calls it.
extern "C" hipError_t verify_policy_launch(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, const uint8_t* pubs, size_t pub_stride,
                                           size_t n, int policy, hipStream_t stream);

#define EDK_DO(expr) do { if (edk_fault_tick()) return hipErrorUnknown; \
    const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
#define EDK_LAUNCH(...) do { if (edk_fault_tick()) return hipErrorUnknown; \
    hipLaunchKernelGGL(__VA_ARGS__); const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)
