// edk_signer.h - the launchers of signer sets (include/eddsa_amd.h: eddsa_amd_signer_create*, ed25519_sign_keyed*), beside
// eddsa_kernels.h and edk_keyed.h: functions of the HIP translation unit that the host side refers to WEAKLY (eddsa_amd.c),
// because the host side is also linked without it (tests/fake_hip, whose CPU launchers know no signer sets).  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "eddsa_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what a keyed sign pass reads of a signer set, all in HBM: a mod l and the prefix as eight words per key, the encoded public
 * keys as 32 bytes per key */
typedef struct edk_signer_set {
  const uint32_t *a, *prefix;
  const uint8_t* pubs;
  size_t count;
} edk_signer_set;

/* `count` keys at `keys` (HBM; expanded == 0: 32-byte seeds, else 64 bytes of scalar | prefix) -> a, prefix (count * 8 words each)
 * and pubs (count * 32 bytes).  comb: the engine's image of the comb, as for edk_genpub.  Asynchronous on `stream`. */
hipError_t edk_signer_build(uint32_t* a, uint32_t* prefix, uint8_t* pubs, const uint8_t* keys, size_t count, int expanded,
                            const uint32_t* comb, hipStream_t stream);

/* edk_sign with item i's secret scalar, prefix and public key taken from `set` by key_idx[i] (HBM, like the other arrays of the
 * pass); ws->dom as in edk_sign.  An index outside the set gets 64 zero bytes. */
hipError_t edk_sign_keyed(uint8_t* sigs, const edk_signer_set* set, const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_off,
                          const uint64_t* msg_end, size_t msg_len, size_t n, const uint32_t* comb, const edk_fixed_ws* ws, hipStream_t stream);

#ifdef __cplusplus
}
#endif
