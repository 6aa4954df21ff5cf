// dom2_check.cpp - TEST BINARY: sha512_dom_msg (libeddsa_amd/csrc/sha512.h) and the lanes of the Ed25519ctx / Ed25519ph kernels
// built on it (lanes.h: verify_dom_hash_lane, sign_dom_scalars_lane, sign_dom_challenge_lane), compiled for the host CPU with
// -DED_HOST_CHECK (every bound asserted).  Built by tests/test_dom2_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

// the prefix as the kernels get it: little-endian words, zero behind byte p - 1 (eddsa_kernels.h: edk_dom)
static void dom_words(uint32_t w[EDK_DOM_WORDS], const uint8_t* dom, uint32_t p) {
  uint8_t bytes[4 * EDK_DOM_WORDS];
  memset(bytes, 0, sizeof(bytes));
  memcpy(bytes, dom, p);
  memcpy(w, bytes, sizeof(bytes));                              // little-endian host
}

extern "C" {

long d2_violations(void) { return g_violations.load(); }

// out = SHA-512(dom[0..p) || pre[0..4 npre) || msg[0..len)), npre 8 or 16; msg is used where it lies (any alignment)
int d2_hash(uint8_t out[64], int npre, const uint8_t* dom, uint32_t p, const uint8_t* pre, const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], pw[16], dig[16];
  dom_words(w, dom, p);
  memcpy(pw, pre, 4 * (size_t)npre);
  if (npre == 8) sha512_dom_msg<8>(dig, w, p, pw, msg, len);
  else if (npre == 16) sha512_dom_msg<16>(dig, w, p, pw, msg, len);
  else return -1;
  memcpy(out, dig, 64);
  return 0;
}

// a | r of sign_dom_scalars_lane, 32 bytes each
void d2_sign_scalars(uint8_t out[64], const uint8_t* dom, uint32_t p, const uint8_t sk[32], const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], skw[8], aw[8], rw[8];
  dom_words(w, dom, p);
  memcpy(skw, sk, 32);
  sign_dom_scalars_lane(aw, rw, w, p, skw, msg, len);
  memcpy(out, aw, 32); memcpy(out + 32, rw, 32);
}

// S of sign_dom_challenge_lane + sign_response_lane for (R, A, a, r)
void d2_sign_response(uint8_t out[32], const uint8_t* dom, uint32_t p, const uint8_t r_enc[32], const uint8_t a_enc[32],
                      const uint8_t a[32], const uint8_t r[32], const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], Rw[8], pub[8], aw[8], rw[8], Sw[8];
  dom_words(w, dom, p);
  memcpy(Rw, r_enc, 32); memcpy(pub, a_enc, 32); memcpy(aw, a, 32); memcpy(rw, r, 32);
  sc t;
  sign_dom_challenge_lane(t, w, p, Rw, pub, msg, len);
  sign_response_lane(Sw, t, aw, rw);
  memcpy(out, Sw, 32);
}

// the digit words the digest route leaves for an item of the verify kernel: verify_dom_hash_lane, then verify_digest_lane
void d2_verify_digits(uint8_t out[32], uint8_t digest[64], const uint8_t* dom, uint32_t p, const uint8_t r_enc[32], const uint8_t a_enc[32],
                      const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], rw[8], aw[8], dig[16], tw[8];
  dom_words(w, dom, p);
  memcpy(rw, r_enc, 32); memcpy(aw, a_enc, 32);
  verify_dom_hash_lane(dig, w, p, rw, aw, msg, len);
  verify_digest_lane(tw, dig);
  memcpy(digest, dig, 64); memcpy(out, tw, 32);
}

}  // extern "C"
