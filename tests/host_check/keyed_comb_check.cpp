// keyed_comb_check.cpp - TEST BINARY: the lane steps of comb key sets (libeddsa_amd/csrc/keyed_lanes.h: keyset_comb_row_lane,
// verify_comb_words_lane, verify_comb_lane - what k_keyset_comb_build and k_verify_main_comb_keyed of keyed_kernels.h run),
// compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).  The items read ONE shared key set by key index, as the
// kernels do.  Built by tests/test_keyed_comb_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "keyed_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

namespace {
struct Words {
  std::vector<uint32_t> words;
  void size(size_t n, uint32_t fill) { words.assign(n + 32, fill); }
  uint32_t* at() { return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(words.data()) + 127) & ~(uintptr_t)127); }
};
// the first half of base16 (verify_main_lane reads no more) and the base point's comb in its global layout, as k_init_tables
// fills them
struct Tables {
  Words base16, comb;
  Tables() {
    base16.size((size_t)TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS, 0);
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++) table_entry_lane(base16.at() + (size_t)TABLE_ENTRY_WORDS * k, (uint32_t)k, 0);
    comb.size((size_t)TABLE_COMB_ENTRIES * TABLE_ENTRY_WORDS, 0);
    for (int row = 0; row < COMB_ROWS; row++)
      for (int m = 1; m <= COMB_HALF; m++)
        table_entry_lane(comb.at() + (size_t)TABLE_ENTRY_WORDS * (COMB_HALF * row + m - 1), (uint32_t)m, (uint32_t)(2 * COMB_W * row));
  }
};
Tables& tables() { static Tables t; return t; }

// the key set: what k_keyset_build and k_keyset_comb_build leave
struct Keyset {
  size_t count = 0;
  std::vector<uint8_t> keys, flags;
  Words tab, comb;
};
Keyset g_ks;

bool exact_from_table(uint32_t* tab, const uint32_t digits[16], const uint32_t rw[8]) {
  alignas(16) uint32_t bentry[VERIFY_ENTRY_WORDS];
  uint32_t dig[EXACT_DIGIT_WORDS];
  exact_bentry_store(bentry);
  verify_exact_setup_table_lane(tab, dig, 1, digits, tables().base16.at() + TABLE_ENTRY_WORDS);
  return verify_exact_chain_table_lane(rw, tab, bentry, dig, 1);
}

void comb_point(ge& acc, size_t k, const uint32_t digits[16]) {
  uint32_t yt[9], ys[9];
  verify_comb_words_lane(yt, ys, 1, digits);
  verify_comb_lane(acc, yt, ys, 1, g_ks.comb.at() + comb_slot(k), g_ks.tab.at() + k * VERIFY_ITEM_TABLE_WORDS, tables().comb.at());
}
}  // namespace

extern "C" {

long kcc_violations(void) { return g_violations.load(); }

// k_keyset_build and k_keyset_comb_build over `count` keys (one call of the row lane per (key, row)); returns the keys on the curve
long kcc_build(const uint8_t* keys, size_t count) {
  g_ks.count = count;
  g_ks.keys.assign(keys, keys + 32 * count);
  g_ks.flags.assign(count, 0);
  g_ks.tab.size(count * VERIFY_ITEM_TABLE_WORDS, 0xa5a5a5a5u);
  g_ks.comb.size(count * KEYSET_COMB_WORDS, 0x5a5a5a5au);
  long on = 0;
  for (size_t k = 0; k < count; k++) {
    uint32_t aw[8];
    memcpy(aw, keys + 32 * k, 32);                 // little-endian host
    g_ks.flags[k] = (uint8_t)keyset_build_lane(g_ks.tab.at() + k * VERIFY_ITEM_TABLE_WORDS, aw);
    on += g_ks.flags[k];
    for (int row = 0; row < COMB_ROWS; row++)
      keyset_comb_row_lane(g_ks.comb.at() + comb_slot(k) + (size_t)row * COMB_HALF * VERIFY_ENTRY_WORDS, aw, row);
  }
  return on;
}

int kcc_on_curve(size_t k) { return g_ks.flags[k]; }

// entry (row, m) of key k's comb: 32 words
void kcc_entry(uint32_t out[VERIFY_ENTRY_WORDS], size_t k, int row, int m) {
  memcpy(out, g_ks.comb.at() + comb_slot(k) + (size_t)VERIFY_ENTRY_WORDS * (COMB_HALF * row + m - 1), VERIFY_ENTRY_WORDS * 4);
}

// the comb's 44 signed digits of the scalar x (32 bytes, < 2^253) as the lane cuts them from the digit words x + pat32 * (1, ..)
void kcc_digits(int8_t out[COMB_DIGITS], const uint8_t x[32], uint32_t pat32) {
  uint32_t dw[8], y[9];
  memcpy(dw, x, 32);
  words_add_pattern(dw, pat32);
  comb_words_of_digits(y, dw, pat32);
  for (int row = 0; row < COMB_ROWS; row++) {
    const uint32_t two = comb_row_digits(y, 1, row);
    out[2 * row] = (int8_t)comb_digit(two, 0);
    out[2 * row + 1] = (int8_t)comb_digit(two, 1);
  }
}

// One item through the steps of a keyed pass over the comb key set in off-curve mode 1: k_verify_prepare_keyed, then
// k_verify_main_comb_keyed and k_verify_finish for a key on the curve, the exact path from the item's own table for a key off
// it.  Returns the verdict, + 2 when the exact path decided.
int kcc_verify(uint32_t key_idx, const uint8_t sig[64], const uint8_t* msg, size_t len) {
  alignas(128) static uint32_t own[VERIFY_ITEM_TABLE_WORDS];
  memset(own, 0x5a, sizeof(own));
  const bool known = key_idx < g_ks.count;
  uint32_t aw[8], rw[8], sw[8], tw[8];
  alignas(16) uint32_t digits[16];
  if (known) memcpy(aw, g_ks.keys.data() + 32 * (size_t)key_idx, 32); else keyed_no_key(aw);
  memcpy(rw, sig, 32); memcpy(sw, sig + 32, 32);
  verify_hash_lane(tw, rw, aw, msg, len);
  verify_s_lane(sw);
  memcpy(digits, tw, 32); memcpy(digits + 8, sw, 32);
  if (!known) return 0;
  if (!g_ks.flags[key_idx]) {
    verify_table_lane(own, aw);                    // k_keyed_exact_tables
    return (exact_from_table(own, digits, rw) ? 1 : 0) + 2;
  }
  ge acc;
  comb_point(acc, key_idx, digits);
  if (fe_iszero(acc.Z)) return 0;
  fe zinv;
  fe_inv(zinv, acc.Z);
  return verify_encode_lane(acc.X, acc.Y, zinv, rw) ? 1 : 0;
}

// S B + t (-A_k) through verify_comb_lane and through verify_main_lane, t and S (32 bytes each, < 2^253) given as they are:
// 1 when the two results are the same projective point with Z != 0
int kcc_same_point(uint32_t key_idx, const uint8_t t[32], const uint8_t s[32]) {
  alignas(16) uint32_t digits[16];
  memcpy(digits, t, 32); memcpy(digits + 8, s, 32);
  words_add_pattern(digits, 0x88888888u);
  words_add_pattern(digits + 8, 0x80008000u);
  ge a, b;
  comb_point(a, key_idx, digits);
  verify_main_lane(b, digits, g_ks.tab.at() + (size_t)key_idx * VERIFY_ITEM_TABLE_WORDS, tables().base16.at());
  if (fe_iszero(a.Z) || fe_iszero(b.Z)) return 0;
  fe l, r, d;
  fe_mul(l, a.X, b.Z); fe_mul(r, b.X, a.Z); fe_sub(d, l, r);
  if (!fe_iszero(d)) return 0;
  fe_mul(l, a.Y, b.Z); fe_mul(r, b.Y, a.Z); fe_sub(d, l, r);
  return fe_iszero(d) ? 1 : 0;
}

}  // extern "C"
