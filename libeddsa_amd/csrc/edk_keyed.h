// edk_keyed.h - the launchers that build a key set (include/eddsa_amd.h: eddsa_amd_keyset_create*), beside eddsa_kernels.h: the
// functions of the HIP translation unit that the host side refers to WEAKLY (eddsa_amd.c), because the host side is also
// linked without it (tests/fake_hip, whose CPU launchers know no key sets).  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `count` keys of 32 bytes at `keys` (HBM) -> table: count slots of VERIFY_ITEM_TABLE_WORDS words, 0..8 times -A in the layout of
 * a verify item's table slot; flags: one byte per key, 1 = the key decodes to a curve point.  Asynchronous on `stream`. */
hipError_t edk_keyset_build(uint32_t* table, uint8_t* flags, const uint8_t* keys, size_t count, hipStream_t stream);

/* ... -> comb: count slots of KEYSET_COMB_WORDS words (edk_layout.h), [key][row][m - 1] = m * 2^(2 COMB_W row) * (-A) in the cached
 * form of a verify table entry: what a comb key set holds on top (eddsa_amd_keyset_create_comb).  Asynchronous on `stream`. */
hipError_t edk_keyset_comb_build(uint32_t* comb, const uint8_t* keys, size_t count, hipStream_t stream);

#ifdef __cplusplus
}
#endif
