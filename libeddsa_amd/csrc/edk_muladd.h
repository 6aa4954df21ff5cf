// edk_muladd.h - the launcher of [m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch*), beside eddsa_kernels.h, edk_keyed.h,
// edk_signer.h and edk_classify.h: a function of the HIP translation unit that the host side refers to WEAKLY (eddsa_amd.c), because
// the host side is also linked without it (tests/fake_hip, whose CPU launchers know no such pass).  Not installed.
#pragma once
#include "eddsa_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `n` items (at most ws->capacity): points 32 bytes each, mul and add 32 bytes each or NULL (every m = 1, every a = 0), all HBM, any
 * alignment -> out[i] = the encoding of [mul_i]points_i + [add_i]B, or 02 00 .. 00 where points_i is no curve point.  `out` may be
 * `points`.  Uses digits, table, acc and flags of the verify workspace and base16's first half.  Asynchronous on `stream`. */
hipError_t edk_point_muladd(uint8_t* out, const uint8_t* points, const uint8_t* mul, const uint8_t* add, size_t n, const uint32_t* base16,
                            const edk_verify_ws* ws, hipStream_t stream);

#ifdef __cplusplus
}
#endif
