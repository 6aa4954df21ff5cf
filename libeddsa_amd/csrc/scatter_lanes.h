// scatter_lanes.h - the front kernel of ed25519_verify_scattered (include/eddsa_amd.h) as what ONE lane computes, like
// policy_lanes.h, classify_lanes.h and muladd_lanes.h, so that the same source compiles for the host under -DED_HOST_CHECK
// (tests/host_check/scatter_check.cpp): whether an item lies in the caller's buffer, and for one that does the gathering of its
// signature and key and the hash SHA-512(R || A || M) (lanes.h: verify_hash_lane's hash, kept as its 64 bytes).  What the lane
// leaves is packed input of a digest pass (ed25519_verify_digests): no kernel behind it learns about the offsets.
#pragma once
#include "lanes.h"
#ifndef ED_HOST_CHECK
#include "kernel_io.h"
#endif

namespace ed {

// (the launcher's translation unit also asks on the host, for the host-pointer form: scatter_spans_inside below)
#ifdef ED_HOST_CHECK
#define ED_HOST_DEV inline
#else
#define ED_HOST_DEV __host__ __device__ __forceinline__
#endif

// THE span test, the one place that decides: item (sig_off, pub_off, msg_off, msg_len) lies entirely in [0, data_len).  The sums
// are formed in 64 bits: 2^32 - 1 + 2^32 - 1 does not wrap.
ED_HOST_DEV bool scatter_item_inside(uint32_t sig_off, uint32_t pub_off, uint32_t msg_off, uint32_t msg_len, uint64_t data_len) {
  return (uint64_t)sig_off + 64 <= data_len && (uint64_t)pub_off + 32 <= data_len && (uint64_t)msg_off + msg_len <= data_len;
}

// the length the order of length sorts an item by: its message's, or 0 for an item outside the buffer, which hashes nothing
ED_DEV uint32_t scatter_item_len(uint32_t sig_off, uint32_t pub_off, uint32_t msg_off, uint32_t msg_len, uint64_t data_len) {
  return scatter_item_inside(sig_off, pub_off, msg_off, msg_len, data_len) ? msg_len : 0u;
}

// 32 bytes at p, any alignment, as eight little-endian words: kernel_io.h: load32, whose unaligned path reads bytes - the path the
// host build, which has no 16-byte vector type, always takes
ED_DEV void scatter_load32(uint32_t w[8], const uint8_t* p) {
#ifdef ED_HOST_CHECK
  for (int i = 0; i < 8; i++)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
#else
  load32(w, p, 0, 0);
#endif
}
// eight words to 16-byte aligned memory: two 16-byte stores
ED_DEV void scatter_store8(uint32_t* p, const uint32_t w[8]) {
  word4* o = reinterpret_cast<word4*>(p);
  o[0] = word4{w[0], w[1], w[2], w[3]};
  o[1] = word4{w[4], w[5], w[6], w[7]};
}

// One item -> its 16 signature words at sig, its 8 key words at key, the 16 words of SHA-512(R || A || M) at dig (the item's
// slots of ws->gsigs, ws->keybytes and ws->domdig: 16-byte aligned); returns whether the item lies in the buffer.
// An item outside the buffer reads NO byte of data and leaves the signature 00 .. 00, the digest 00 .. 00 and the key 02 00 .. 00
// (include/eddsa_amd.h: EDDSA_AMD_NO_POINT_BYTE0, y = 2: on no curve point).  t = 0 and S = 0: no route adds a multiple of the
// key, every cofactorless route gets the neutral element, whose encoding 01 00 .. 00 is not R = 00 .. 00, and the cofactored
// equation rejects a key that is no curve point - ok = 0 under every setting without a flag of its own.
// R and A are stored before the hash and S is fetched behind it: nothing but the prefix is held across the compression.
ED_DEV bool scatter_challenge_lane(uint32_t* sig, uint32_t* key, uint32_t* dig, const uint8_t* data, uint64_t data_len,
                                   uint32_t sig_off, uint32_t pub_off, uint32_t msg_off, uint32_t msg_len) {
  uint32_t pre[16], out[16];
  if (!scatter_item_inside(sig_off, pub_off, msg_off, msg_len, data_len)) {
#pragma unroll
    for (int q = 0; q < 8; q++) pre[q] = 0u;
    scatter_store8(sig, pre); scatter_store8(sig + 8, pre);
    scatter_store8(dig, pre); scatter_store8(dig + 8, pre);
    pre[0] = 2u;
    scatter_store8(key, pre);
    return false;
  }
  scatter_load32(pre, data + sig_off);
  scatter_load32(pre + 8, data + pub_off);
  scatter_store8(sig, pre);
  scatter_store8(key, pre + 8);
  sha512_prefix_msg<16>(out, pre, data + msg_off, msg_len);
  scatter_store8(dig, out); scatter_store8(dig + 8, out + 8);
  scatter_load32(pre, data + sig_off + 32);
  scatter_store8(sig + 8, pre);
  return true;
}

}  // namespace ed
