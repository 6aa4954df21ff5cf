// edk_scatter.h - the front of a scattered verify pass (include/eddsa_amd.h: ed25519_verify_scattered*), beside eddsa_kernels.h,
// edk_keyed.h, edk_signer.h, edk_classify.h and edk_muladd.h: functions of the HIP translation unit that the host side refers to
// WEAKLY (eddsa_amd.c), because the host side is also linked without it (tests/fake_hip, whose CPU launchers know no such pass).
// Not installed.
#pragma once
#include "eddsa_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `n` items (at most ws->capacity) given by four packed uint32 arrays (HBM) into data[0 .. data_len) (HBM, data_len < 2^32):
 * item i's 64 signature bytes -> ws->gsigs + 64 i, its 32 key bytes -> ws->keybytes + 32 i, SHA-512(R || A || M) -> ws->domdig + 64 i;
 * an item that is not entirely in the buffer is not read and gets the signature 00 .. 00, the digest 00 .. 00 and the key 02 00 .. 00,
 * which every route rejects (scatter_lanes.h).  From MSG_ORDER_MIN_N items on the lanes take the items longest message first
 * (ws->perm, ws->lenbins).  ws->gsigs must be allocated (eddsa_amd.c: verify_on does it for the slot).  The caller goes on with
 * edk_verify over a digest source on the same workspace.  Asynchronous on `stream`. */
hipError_t edk_scatter_challenge(const uint8_t* data, size_t data_len, const uint32_t* sig_off, const uint32_t* pub_off,
                                 const uint32_t* msg_off, const uint32_t* msg_len, size_t n, const edk_verify_ws* ws, hipStream_t stream);

/* the same span test over arrays in HOST memory (the host-pointer form checks before it uploads): 1 when every item lies in the
 * buffer, else 0.  Touches no device. */
int edk_scatter_spans_inside(size_t data_len, const uint32_t* sig_off, const uint32_t* pub_off, const uint32_t* msg_off,
                             const uint32_t* msg_len, size_t n);

#ifdef __cplusplus
}
#endif
