// keyed_forms_check.cpp - TEST BINARY: the lane sequences of the digest, Ed25519ctx and Ed25519ph forms of key-set verification
// (libeddsa_amd/csrc/keyed_kernels.h: k_verify_prepare_keyed<true>, k_dom_challenge_keyed; rlc_keyed.h: k_rlc_hash_keyed<true>),
// compiled for the host CPU with -DED_HOST_CHECK (every bound asserted), item by item in the kernels' order of steps, each beside
// the unkeyed sequence (kernels.hip: k_verify_prepare<true>, k_dom_challenge; rlc.hip: k_rlc_hash_digest) over the item's own key
// bytes.  Built by tests/test_keyed_forms_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rlc_keyed_lanes.h"

constexpr uint8_t VERIFY_WINDOWED = 1;   // kernel_io.h (device code only): the flag bit the prepare kernels set

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

// the key set as k_keyset_build leaves it: key bytes and one on-curve flag per key (the tables are not what these forms change)
static std::vector<uint8_t> g_keys, g_flags;

// the prefix as the kernels get it: little-endian words, zero behind byte p - 1 (eddsa_kernels.h: edk_dom)
static void dom_words(uint32_t w[EDK_DOM_WORDS], const uint8_t* dom, uint32_t p) {
  uint8_t bytes[4 * EDK_DOM_WORDS];
  memset(bytes, 0, sizeof(bytes));
  memcpy(bytes, dom, p);
  memcpy(w, bytes, sizeof(bytes));                              // little-endian host
}

// what one item's slot of the workspace holds behind a prepare kernel, as bytes: t digits | S digits | key bytes | flags |
// on the windowed list | on the exact list | ok (0xff: not written)
struct prepared { uint8_t t[32], s[32], key[32], flags, on, off, ok; };
static_assert(sizeof(prepared) == 100, "tests/test_keyed_forms_on_host.py reads this layout");

extern "C" {

long kfc_violations(void) { return g_violations.load(); }

// k_keyset_build over `count` keys
void kfc_keyset(const uint8_t* keys, int count) {
  alignas(128) static uint32_t tab[VERIFY_ITEM_TABLE_WORDS];
  g_keys.assign(keys, keys + 32 * (size_t)count);
  g_flags.resize((size_t)count);
  for (int k = 0; k < count; k++) {
    uint32_t aw[8];
    memcpy(aw, keys + 32 * (size_t)k, 32);
    g_flags[(size_t)k] = (uint8_t)keyset_build_lane(tab, aw);
  }
}
int kfc_key_flag(int k) { return g_flags[(size_t)k]; }

// k_verify_prepare_keyed<true> for one item: the key by index, t from the 64 bytes in the message slot, S, flags and lists
void kfc_prepare_keyed(prepared* out, const uint8_t sig[64], uint32_t key_idx, const uint8_t digest[64], int offcurve_mode) {
  const uint32_t count = (uint32_t)g_flags.size();
  const uint32_t k = key_idx;
  const bool known = k < count;
  uint32_t aw[8], sw[8], tw[8], dw[16];
  if (known) memcpy(aw, g_keys.data() + 32 * (size_t)k, 32); else keyed_no_key(aw);
  const uint32_t kf = known ? 1u | (g_flags[k] != 0 ? 2u : 0u) : 0u;
  memcpy(out->key, aw, 32);
  out->ok = known ? 0xff : 0;
  memcpy(dw, digest, 64);
  verify_digest_lane(tw, dw);
  memcpy(out->t, tw, 32);
  memcpy(sw, sig + 32, 32);
  verify_s_lane(sw);
  memcpy(out->s, sw, 32);
  const bool windowed = (kf & 2u) != 0 && offcurve_mode != 2;
  out->flags = (uint8_t)(windowed ? VERIFY_WINDOWED : 0);
  out->on = windowed;
  out->off = (kf & 1u) != 0 && !windowed;
}

// k_verify_prepare<true> for the same item with its key bytes given: the table is built here, its result is the on-curve flag
void kfc_prepare_unkeyed(prepared* out, const uint8_t sig[64], const uint8_t pub[32], const uint8_t digest[64], int all_exact) {
  alignas(128) static uint32_t tab[VERIFY_ITEM_TABLE_WORDS];
  uint32_t aw[8], sw[8], tw[8], dw[16];
  memcpy(aw, pub, 32);
  memcpy(dw, digest, 64);
  verify_digest_lane(tw, dw);
  memcpy(out->t, tw, 32);
  memcpy(sw, sig + 32, 32);
  verify_s_lane(sw);
  memcpy(out->s, sw, 32);
  const bool windowed = verify_table_lane(tab, aw) && !all_exact;
  memcpy(out->key, pub, 32);
  out->flags = (uint8_t)(windowed ? VERIFY_WINDOWED : 0);
  out->on = windowed;
  out->off = !windowed;
  out->ok = 0xff;
}

// k_dom_challenge_keyed for one item: SHA-512(dom2 || R || keys[key_idx] || M'), keyed_no_key's bytes outside the set
void kfc_dom_keyed(uint8_t out[64], const uint8_t* dom, uint32_t p, const uint8_t sig[64], uint32_t key_idx, const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], rw[8], aw[8], dig[16];
  dom_words(w, dom, p);
  if (key_idx < (uint32_t)g_flags.size()) memcpy(aw, g_keys.data() + 32 * (size_t)key_idx, 32); else keyed_no_key(aw);
  memcpy(rw, sig, 32);
  verify_dom_hash_lane(dig, w, p, rw, aw, msg, len);
  memcpy(out, dig, 64);
}

// k_dom_challenge for the same item with its key bytes given
void kfc_dom_unkeyed(uint8_t out[64], const uint8_t* dom, uint32_t p, const uint8_t sig[64], const uint8_t pub[32], const uint8_t* msg, size_t len) {
  uint32_t w[EDK_DOM_WORDS], rw[8], aw[8], dig[16];
  dom_words(w, dom, p);
  memcpy(aw, pub, 32);
  memcpy(rw, sig, 32);
  verify_dom_hash_lane(dig, w, p, rw, aw, msg, len);
  memcpy(out, dig, 64);
}

// k_rlc_hash_keyed<true> for one item: t | S mod l | leaf | the key bytes left for k_verify_policy, 32 bytes each
void kfc_rlc_hash_keyed(uint8_t out[128], const uint8_t sig[64], uint32_t key_idx, const uint8_t digest[64]) {
  uint32_t aw[8], sw[8], tw[8], lf[8], dw[16];
  if (key_idx < (uint32_t)g_flags.size()) memcpy(aw, g_keys.data() + 32 * (size_t)key_idx, 32); else keyed_no_key(aw);
  memcpy(out + 96, aw, 32);
  memcpy(dw, digest, 64);
  memcpy(sw, sig + 32, 32);
  rlc_digest_lane(tw, sw, lf, dw, sig + 32);
  memcpy(out, tw, 32); memcpy(out + 32, sw, 32); memcpy(out + 64, lf, 32);
}

// k_rlc_hash_digest for the same item: t | S mod l | leaf
void kfc_rlc_hash_unkeyed(uint8_t out[96], const uint8_t sig[64], const uint8_t digest[64]) {
  uint32_t sw[8], tw[8], lf[8], dw[16];
  memcpy(dw, digest, 64);
  memcpy(sw, sig + 32, 32);
  rlc_digest_lane(tw, sw, lf, dw, sig + 32);
  memcpy(out, tw, 32); memcpy(out + 32, sw, 32); memcpy(out + 64, lf, 32);
}

}  // extern "C"
