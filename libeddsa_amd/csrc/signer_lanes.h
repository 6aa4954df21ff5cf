// signer_lanes.h - what a lane of the signer-set kernels (signer_kernels.h) computes beyond lanes.h: plain words in, words out, so
// that the same source compiles for the host under -DED_HOST_CHECK (tests/host_check/signer_check.cpp, every limb bound asserted).
//
// A signer set (include/eddsa_amd.h: eddsa_amd_signer) holds, per registered key, the secret scalar a mod l, the 32-byte prefix
// of the nonce hash and the encoded public key A = (a mod l) B.  A keyed sign pass takes the three by key index where
// ed25519_sign_batch hashes the seed per item (lanes.h: sign_scalars_lane -> key_setup) and is handed A by its caller.
#pragma once
#include "lanes.h"

namespace ed {

// One key from its SEED: what sign_scalars_lane derives per item - h = SHA-512(seed), a = h[0..32) clamped and reduced mod l
// (the words sign_response_lane imports again), prefix = h[32..64).
ED_DEV void signer_seed_lane(uint32_t aw[8], uint32_t pw[8], const uint32_t sk[8]) {
  uint32_t h[16];
  key_setup(h, sk);
  sc a;
  sc_from_words<8>(a, h);
  sc_to_words(aw, a);
#pragma unroll
  for (int k = 0; k < 8; k++) pw[k] = h[8 + k];
}

// One key from its EXPANDED form, scalar | prefix: the scalar is any 256-bit little-endian integer, used mod l and NOT clamped
// (derived and blinded keys are no clamped integers).  sc_from_words<8> cuts all 256 bits into ten 26-bit limbs (the tenth holds
// bits 234..255) and reduces by the general Barrett step for x < 2^520 (sc25519.h: sc_barrett; q3 is at most 2 short, two
// masked subtractions of l follow), so every input - a >= 2^255, a = l, a = 2^256 - 1 - leaves a value below l.
ED_DEV void signer_expanded_lane(uint32_t aw[8], uint32_t pw[8], const uint32_t ew[16]) {
  sc a;
  sc_from_words<8>(a, ew);
  sc_to_words(aw, a);
#pragma unroll
  for (int k = 0; k < 8; k++) pw[k] = ew[8 + k];
}

// A = a B encoded, for a < l (a = 0: the neutral element, 01 00 .. 00).  comb: as in scale_base_lane.  The inversion is the
// lane's own: registration is not the hot path.
ED_DEV void signer_pub_lane(uint32_t Aw[8], const uint32_t aw[8], const uint32_t* comb) {
  ge A;
  scale_base_lane<1>(A, aw, comb);
  fe zinv;
  fe_inv(zinv, A.Z);                             // Z of a comb result is never 0
  encode_lane(Aw, A.X, A.Y, zinv);
}

// rw = r = H([dom2 ||] prefix || M') mod l as words: the second hash of sign_scalars_lane / sign_dom_scalars_lane with the prefix
// given.  dom, P: the prefix's words and its length (DOM only; sha512.h: sha512_dom_msg).
template <bool DOM>
ED_DEV void sign_keyed_nonce_lane(uint32_t rw[8], const uint32_t* dom, uint32_t P, const uint32_t pw[8], const uint8_t* m, size_t mlen) {
  uint32_t dig[16];
  if constexpr (DOM) sha512_dom_msg<8>(dig, dom, P, pw, m, mlen);
  else sha512_prefix_msg<8>(dig, pw, m, mlen);
  sc r;
  sc_from_words<16>(r, dig);
  sc_to_words(rw, r);
}

}  // namespace ed
