// crafted_check.cpp - TEST BINARY: one item of the digest forms of verification (include/eddsa_amd.h: ed25519_verify_digests*,
// ed25519_verify_keyed_digests*) through the lane steps of every evaluation - the full-length chain, the three half-length chains
// and the comb (libeddsa_amd/csrc/lanes.h, keyed_lanes.h) - compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).
// The digest is the caller's, so the challenge scalar is chosen: tests/crafted_scalars.py builds the items.  Built by
// tests/test_crafted_scalars_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "keyed_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
static char g_first[256];
static std::mutex g_mu;
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) {
    std::lock_guard<std::mutex> lk(g_mu);
    snprintf(g_first, sizeof(g_first), "%s:%d: %s", file, line, what);
  }
}
}  // namespace ed

using namespace ed;

namespace {
struct Words {
  std::vector<uint32_t> words;
  void size(size_t n, uint32_t fill) { words.assign(n + 32, fill); }
  uint32_t* at() { return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(words.data()) + 127) & ~(uintptr_t)127); }
};
// both halves of base16 and the base point's comb in its global layout, as k_init_tables fills them
struct Tables {
  Words base16, comb;
  Tables() {
    base16.size((size_t)2 * TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS, 0);
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++) table_entry_lane(base16.at() + (size_t)TABLE_ENTRY_WORDS * k, (uint32_t)k, 0);
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++)
      table_entry_lane(base16.at() + (size_t)TABLE_ENTRY_WORDS * (TABLE_BASE16_ENTRIES + k), (uint32_t)k, 128);
    comb.size((size_t)TABLE_COMB_ENTRIES * TABLE_ENTRY_WORDS, 0);
    for (int row = 0; row < COMB_ROWS; row++)
      for (int m = 1; m <= COMB_HALF; m++)
        table_entry_lane(comb.at() + (size_t)TABLE_ENTRY_WORDS * (COMB_HALF * row + m - 1), (uint32_t)m, (uint32_t)(2 * COMB_W * row));
  }
};
Tables& tables() { static Tables t; return t; }

// the comb key set: what k_keyset_build and k_keyset_comb_build leave (as tests/host_check/keyed_comb_check.cpp builds one)
struct Keyset {
  size_t count = 0;
  std::vector<uint8_t> flags;
  Words tab, comb;
};
Keyset g_ks;

// the prepare step of a digest pass: t from the digest, S, the table of -A; returns whether A is on the curve
bool prepare(uint32_t tw[8], uint32_t sw[8], uint32_t* tab, const uint8_t sig[64], const uint8_t pub[32], const uint8_t digest[64]) {
  uint32_t dw[16], aw[8];
  memcpy(dw, digest, 64); memcpy(aw, pub, 32); memcpy(sw, sig + 32, 32);   // little-endian host
  verify_digest_lane(tw, dw);
  verify_s_lane(sw);
  return verify_table_lane(tab, aw);
}

int encoded_verdict(const ge& acc, const uint8_t sig[64]) {
  if (fe_iszero(acc.Z)) return 0;
  uint32_t rw[8];
  memcpy(rw, sig, 32);
  fe zinv;
  fe_inv(zinv, acc.Z);
  return verify_encode_lane(acc.X, acc.Y, zinv, rw) ? 1 : 0;
}

// BITS / WINDOWS: one of the three half-length arrangements.  Returns 0 / 1 = the verdict, + 4 when the item is long and ran
// the long loop, + 8 when the integer check refused the search's pair; 2 (+ 8) = the item is handed to the exact path: a key off
// the curve, or a long item of the balanced arrangement, whose kernel has no long loop.  in_long_wave: the item runs the
// 64-window loop whatever it is, as a short item does in a wave that contains a long one
template <int BITS, int WINDOWS>
int half(const uint8_t sig[64], const uint8_t pub[32], const uint8_t digest[64], int in_long_wave, uint32_t* hd_out) {
  alignas(16) uint32_t tab[VERIFY_ITEM_TABLE_WORDS], rtab[VERIFY_ITEM_TABLE_WORDS];
  uint32_t rw[8], sw[8], tw[8], hd[HALF_DIGIT_WORDS];
  const bool oncurve = prepare(tw, sw, tab, sig, pub, digest);
  memcpy(rw, sig, 32);
  verify_half_scalars_lane<BITS>(hd, tw, sw);
  if (hd_out) memcpy(hd_out, hd, sizeof(hd));
  const bool rvalid = verify_half_point_lane(rtab, rw);
  const int refused = (hd[HALF_STATUS_WORD] & HALF_PAIR_REFUSED) ? 8 : 0;
  const bool is_long = (hd[HALF_STATUS_WORD] & HALF_LONG) != 0;
  if (!oncurve || (is_long && BITS == HALF_BITS_BALANCED && !in_long_wave)) return 2 + refused;
  const bool neutral = is_long || in_long_wave ? verify_half_main_lane<true, WINDOWS>(hd, tab, rtab, tables().base16.at(), true)
                                               : verify_half_main_lane<false, WINDOWS>(hd, tab, rtab, tables().base16.at(), false);
  return (neutral && rvalid ? 1 : 0) + (is_long ? 4 : 0) + refused;
}
}  // namespace

extern "C" {

long cc_violations(void) { return g_violations.load(); }
const char* cc_first_violation(void) { return g_first; }

// verify_digest_lane -> verify_s_lane -> verify_table_lane -> verify_main_lane and the encode compare: 0 / 1, 2 = key off the curve
int cc_full(const uint8_t sig[64], const uint8_t pub[32], const uint8_t digest[64]) {
  alignas(16) uint32_t tab[VERIFY_ITEM_TABLE_WORDS], digits[16];
  uint32_t sw[8], tw[8];
  if (!prepare(tw, sw, tab, sig, pub, digest)) return 2;
  memcpy(digits, tw, 32); memcpy(digits + 8, sw, 32);
  ge acc;
  verify_main_lane(acc, digits, tab, tables().base16.at());
  return encoded_verdict(acc, sig);
}

// bits: 134, 138, or 131 for the balanced search; hd_out (HALF_DIGIT_WORDS words, may be null): the item's digit words
int cc_half(int bits, const uint8_t sig[64], const uint8_t pub[32], const uint8_t digest[64], int in_long_wave, uint32_t* hd_out) {
  if (bits == HALF_BITS) return half<HALF_BITS, HALF_WINDOWS>(sig, pub, digest, in_long_wave, hd_out);
  if (bits == HALF_BITS_SMALL) return half<HALF_BITS_SMALL, HALF_WINDOWS_SMALL>(sig, pub, digest, in_long_wave, hd_out);
  if (bits == HALF_BITS_BALANCED) return half<HALF_BITS_BALANCED, HALF_WINDOWS_BALANCED>(sig, pub, digest, in_long_wave, hd_out);
  return -1;
}

// k_keyset_build and k_keyset_comb_build over `count` keys; returns the keys on the curve
long cc_comb_build(const uint8_t* keys, size_t count) {
  g_ks.count = count;
  g_ks.flags.assign(count, 0);
  g_ks.tab.size(count * VERIFY_ITEM_TABLE_WORDS, 0xa5a5a5a5u);
  g_ks.comb.size(count * KEYSET_COMB_WORDS, 0x5a5a5a5au);
  long on = 0;
  for (size_t k = 0; k < count; k++) {
    uint32_t aw[8];
    memcpy(aw, keys + 32 * k, 32);
    g_ks.flags[k] = (uint8_t)keyset_build_lane(g_ks.tab.at() + k * VERIFY_ITEM_TABLE_WORDS, aw);
    on += g_ks.flags[k];
    for (int row = 0; row < COMB_ROWS; row++)
      keyset_comb_row_lane(g_ks.comb.at() + comb_slot(k) + (size_t)row * COMB_HALF * VERIFY_ENTRY_WORDS, aw, row);
  }
  return on;
}

// one item of a keyed digest pass over the comb key set: verify_digest_lane, verify_s_lane, verify_comb_words_lane,
// verify_comb_lane and the encode compare: 0 / 1, 2 = key off the curve, -1 = no such key
int cc_comb(uint32_t key_idx, const uint8_t sig[64], const uint8_t digest[64]) {
  if (key_idx >= g_ks.count) return -1;
  if (!g_ks.flags[key_idx]) return 2;
  uint32_t dw[16], sw[8], tw[8], yt[9], ys[9];
  alignas(16) uint32_t digits[16];
  memcpy(dw, digest, 64); memcpy(sw, sig + 32, 32);
  verify_digest_lane(tw, dw);
  verify_s_lane(sw);
  memcpy(digits, tw, 32); memcpy(digits + 8, sw, 32);
  verify_comb_words_lane(yt, ys, 1, digits);
  ge acc;
  verify_comb_lane(acc, yt, ys, 1, g_ks.comb.at() + comb_slot(key_idx), g_ks.tab.at() + (size_t)key_idx * VERIFY_ITEM_TABLE_WORDS, tables().comb.at());
  return encoded_verdict(acc, sig);
}

}  // extern "C"
