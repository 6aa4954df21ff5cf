// signer_check.cpp - TEST BINARY: the lane sequences of the signer-set kernels (libeddsa_amd/csrc/signer_kernels.h: k_signer_build,
// k_sign_keyed_scalars, the point kernel they share with Ed25519ctx / Ed25519ph, k_sign_keyed_finish) compiled for the host CPU
// with -DED_HOST_CHECK (every bound asserted), key by key and item by item in the kernels' order of steps, and beside them the
// unkeyed sequence of ed25519_sign_batch for the same seed.  Built by tests/test_sign_keyed_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "signer_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

// the comb of B in its global layout, as the engine's k_init_tables builds it (tests/host_check/host_check.cpp does the same)
static const uint32_t* comb() {
  static std::vector<uint32_t> t;
  if (t.empty()) {
    t.resize((size_t)TABLE_COMB_ENTRIES * TABLE_ENTRY_WORDS);
    for (int c = 0; c < TABLE_COMB_ENTRIES; c++)
      table_entry_lane(&t[(size_t)TABLE_ENTRY_WORDS * c], (uint32_t)(c % COMB_HALF) + 1, 2u * COMB_W * (uint32_t)(c / COMB_HALF));
  }
  return t.data();
}

// the prefix as the kernels get it: little-endian words, zero behind byte p - 1 (eddsa_kernels.h: edk_dom)
static void dom_words(uint32_t w[EDK_DOM_WORDS], const uint8_t* dom, uint32_t p) {
  uint8_t bytes[4 * EDK_DOM_WORDS];
  memset(bytes, 0, sizeof(bytes));
  memcpy(bytes, dom, p);
  memcpy(w, bytes, sizeof(bytes));                              // little-endian host
}

// the set as k_signer_build leaves it: a mod l | prefix | A, 32 bytes each per key
static std::vector<uint8_t> g_set;

extern "C" {

long sgc_violations(void) { return g_violations.load(); }

// k_signer_build<EXPANDED> over `count` keys of 32 (seeds) or 64 bytes (scalar | prefix); out: 96 bytes per key
void sgc_build(uint8_t* out, const uint8_t* keys, int count, int is_expanded) {
  g_set.resize(96 * (size_t)count);
  for (int k = 0; k < count; k++) {
    uint32_t aw[8], pw[8], Aw[8];
    if (is_expanded) {
      uint32_t ew[16];
      memcpy(ew, keys + 64 * (size_t)k, 64);
      signer_expanded_lane(aw, pw, ew);
    } else {
      uint32_t sk[8];
      memcpy(sk, keys + 32 * (size_t)k, 32);
      signer_seed_lane(aw, pw, sk);
    }
    signer_pub_lane(Aw, aw, comb());
    uint8_t* o = g_set.data() + 96 * (size_t)k;
    memcpy(o, aw, 32); memcpy(o + 32, pw, 32); memcpy(o + 64, Aw, 32);
  }
  memcpy(out, g_set.data(), g_set.size());
}

// one item through k_sign_keyed_scalars, k_sign_dom_point and k_sign_keyed_finish over the set of the last sgc_build.
// dom == NULL: Ed25519; else the p bytes of dom2(F, C).  aux (64 bytes): a | r as the first kernel leaves them.  An index
// outside the set: zeros in aux and 64 zero bytes of signature.
void sgc_sign(uint8_t sig[64], uint8_t aux[64], uint32_t key_idx, const uint8_t* msg, size_t len, const uint8_t* dom, uint32_t p) {
  const uint32_t count = (uint32_t)(g_set.size() / 96);
  const bool known = key_idx < count;
  uint32_t w[EDK_DOM_WORDS], aw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pw[8], pub[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (dom) dom_words(w, dom, p);
  if (known) {
    const uint8_t* key = g_set.data() + 96 * (size_t)key_idx;
    memcpy(pw, key + 32, 32);
    if (dom) sign_keyed_nonce_lane<true>(rw, w, p, pw, msg, len);
    else sign_keyed_nonce_lane<false>(rw, nullptr, 0, pw, msg, len);
    memcpy(aw, key, 32);
    memcpy(pub, key + 64, 32);
  }
  memcpy(aux, aw, 32); memcpy(aux + 32, rw, 32);
  ge R; fe zinv;
  scale_base_lane<1>(R, rw, comb());                          // k_sign_dom_point
  fe_inv(zinv, R.Z);
  uint32_t Rw[8], Sw[8];
  encode_lane(Rw, R.X, R.Y, zinv);
  sc t;
  if (dom) sign_dom_challenge_lane(t, w, p, Rw, pub, msg, len);
  else sign_challenge_lane(t, Rw, pub, msg, len);
  sign_response_lane(Sw, t, aw, rw);
  for (int j = 0; j < 8; j++) { Rw[j] = known ? Rw[j] : 0u; Sw[j] = known ? Sw[j] : 0u; }
  memcpy(sig, Rw, 32); memcpy(sig + 32, Sw, 32);
}

// the unkeyed sequence for the same item: k_sign_point and k_sign_finish of ed25519_sign_batch over (seed, pub)
void sgc_sign_unkeyed(uint8_t sig[64], uint8_t aux[64], const uint8_t seed[32], const uint8_t pubkey[32], const uint8_t* msg, size_t len) {
  uint32_t sk[8], pk[8], aw[8], rw[8], Rw[8], Sw[8];
  memcpy(sk, seed, 32); memcpy(pk, pubkey, 32);
  ge R; fe zinv;
  sign_point_lane(R, aw, rw, sk, msg, len, comb());
  memcpy(aux, aw, 32); memcpy(aux + 32, rw, 32);
  fe_inv(zinv, R.Z);
  encode_lane(Rw, R.X, R.Y, zinv);
  sign_finish_lane(Sw, Rw, aw, rw, pk, msg, len);
  memcpy(sig, Rw, 32); memcpy(sig + 32, Sw, 32);
}

// sc_from_words<8> alone: any 256-bit integer -> the value below l, as bytes (the import signer_expanded_lane relies on)
void sgc_reduce256(uint8_t out[32], const uint8_t in[32]) {
  uint32_t w[8], o[8];
  memcpy(w, in, 32);
  sc a;
  sc_from_words<8>(a, w);
  sc_to_words(o, a);
  memcpy(out, o, 32);
}

}  // extern "C"
