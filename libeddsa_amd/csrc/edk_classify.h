// edk_classify.h - the launcher of point classification (include/eddsa_amd.h: ed25519_point_classify_batch*,
// eddsa_amd_keyset_classify), beside eddsa_kernels.h, edk_keyed.h and edk_signer.h: a function of the HIP translation unit that the host
// side refers to WEAKLY (eddsa_amd.c), because the host side is also linked without it (tests/fake_hip, whose CPU launchers know no
// classification).  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `n` strings of 32 bytes at `points` (HBM, any alignment) -> one class byte each at `cls` (HBM): the EDDSA_AMD_POINT_* bits.  Needs no
 * table and no workspace.  Asynchronous on `stream`. */
hipError_t edk_point_classify(uint8_t* cls, const uint8_t* points, size_t n, hipStream_t stream);

#ifdef __cplusplus
}
#endif
