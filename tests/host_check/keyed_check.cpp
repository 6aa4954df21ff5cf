// keyed_check.cpp - TEST BINARY: the lane steps of key-set verification (libeddsa_amd/csrc/keyed_lanes.h and the lanes.h
// functions the keyed kernels of keyed_kernels.h call), compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).
// The items read tab_a from ONE shared table, by key index, as the kernels do; what they leave in their own slots is dirtied
// first.  Built by tests/test_keyed_on_host.py; not part of the product.
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
// both halves of base16, as kernels.hip: k_init_tables fills them
struct Table {
  std::vector<uint32_t> words;
  uint32_t* at() { return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(words.data()) + 127) & ~(uintptr_t)127); }
  Table() : words((size_t)2 * TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS + 32) {
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++) table_entry_lane(at() + (size_t)TABLE_ENTRY_WORDS * k, (uint32_t)k, 0);
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++) table_entry_lane(at() + (size_t)TABLE_ENTRY_WORDS * (TABLE_BASE16_ENTRIES + k), (uint32_t)k, 128);
  }
};
Table& base() { static Table t; return t; }

// the key set: what k_keyset_build leaves
struct Keyset {
  size_t count = 0;
  std::vector<uint8_t> keys, flags;
  std::vector<uint32_t> words;
  uint32_t* tab() { return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(words.data()) + 127) & ~(uintptr_t)127); }
};
Keyset g_ks;

size_t slot_of(size_t k) { return k * VERIFY_ITEM_TABLE_WORDS; }

// the exact path as the one-lane kernels run it, from the item's OWN table and its digit words (k_verify_exact_lane_*)
bool exact_from_table(uint32_t* tab, const uint32_t digits[16], const uint32_t rw[8]) {
  alignas(16) uint32_t bentry[VERIFY_ENTRY_WORDS];
  uint32_t dig[EXACT_DIGIT_WORDS];
  exact_bentry_store(bentry);
  verify_exact_setup_table_lane(tab, dig, 1, digits, base().at() + TABLE_ENTRY_WORDS);
  return verify_exact_chain_table_lane(rw, tab, bentry, dig, 1);
}
}  // namespace

extern "C" {

long kc_violations(void) { return g_violations.load(); }

// k_keyset_build over `count` keys; returns the number of keys on the curve
long kc_build(const uint8_t* keys, size_t count) {
  g_ks.count = count;
  g_ks.keys.assign(keys, keys + 32 * count);
  g_ks.flags.assign(count, 0);
  g_ks.words.assign(count * VERIFY_ITEM_TABLE_WORDS + 32, 0xa5a5a5a5u);
  long on = 0;
  for (size_t k = 0; k < count; k++) {
    uint32_t aw[8];
    memcpy(aw, keys + 32 * k, 32);                 // little-endian host
    g_ks.flags[k] = (uint8_t)keyset_build_lane(g_ks.tab() + slot_of(k), aw);
    on += g_ks.flags[k];
  }
  return on;
}

// the table and the flag of key k against verify_table_lane's for the same bytes: 1 = equal
int kc_table_matches(size_t k) {
  alignas(128) uint32_t tab[VERIFY_ITEM_TABLE_WORDS];
  uint32_t aw[8];
  memcpy(aw, g_ks.keys.data() + 32 * k, 32);
  const bool on = verify_table_lane(tab, aw);
  return memcmp(tab, g_ks.tab() + slot_of(k), sizeof(tab)) == 0 && on == (g_ks.flags[k] != 0);
}

// the bytes an item without a key is given
void kc_no_key(uint8_t out[32]) {
  uint32_t aw[8];
  keyed_no_key(aw);
  memcpy(out, aw, 32);
}

// One item through the keyed kernels' steps.  form 0: the half-length route (k_verify_prepare_keyed, k_verify_halve_keyed<BITS>,
// k_verify_main_half_keyed<WINDOWS>, wide != 0: 2^138 / 35 windows), an off-curve key and an item without a short pair through
// the exact path from the item's own table; form 1: the full-length route in reject mode (k_verify_main_keyed, k_verify_finish).
// Returns the verdict, + 2 when the exact path decided, + 4 when it did so for an item without a short pair.
int kc_verify(uint32_t key_idx, const uint8_t sig[64], const uint8_t* msg, size_t len, int form, int wide) {
  alignas(128) static uint32_t own[VERIFY_ITEM_TABLE_WORDS], rtab[VERIFY_ITEM_TABLE_WORDS];
  memset(own, 0x5a, sizeof(own));                  // a keyed pass must not depend on what the slot held
  memset(rtab, 0xa5, sizeof(rtab));
  const bool known = key_idx < g_ks.count;
  uint32_t aw[8], rw[8], sw[8], tw[8];
  alignas(16) uint32_t digits[16];
  if (known) memcpy(aw, g_ks.keys.data() + 32 * (size_t)key_idx, 32); else keyed_no_key(aw);
  memcpy(rw, sig, 32); memcpy(sw, sig + 32, 32);
  verify_hash_lane(tw, rw, aw, msg, len);
  verify_s_lane(sw);
  memcpy(digits, tw, 32); memcpy(digits + 8, sw, 32);
  if (!known) return 0;
  const bool oncurve = g_ks.flags[key_idx] != 0;
  const uint32_t* tab_a = g_ks.tab() + slot_of(key_idx);
  if (form == 1) {
    if (!oncurve) return 0;
    ge acc;
    verify_main_lane(acc, digits, tab_a, base().at());
    if (fe_iszero(acc.Z)) return 0;
    fe zinv;
    fe_inv(zinv, acc.Z);
    return verify_encode_lane(acc.X, acc.Y, zinv, rw) ? 1 : 0;
  }
  if (!oncurve) {
    verify_table_lane(own, aw);                    // k_verify_prepare_keyed: the item's own table
    return (exact_from_table(own, digits, rw) ? 1 : 0) + 2;
  }
  uint32_t hd[HALF_DIGIT_WORDS];
  if (wide) verify_half_scalars_lane<HALF_BITS_SMALL>(hd, tw, sw); else verify_half_scalars_lane<HALF_BITS>(hd, tw, sw);
  const bool rvalid = verify_half_point_lane(rtab, rw);
  if ((hd[HALF_STATUS_WORD] & HALF_LONG) != 0) {   // k_verify_halve_keyed: the key's entries into the item's slot
    keyed_table_copy(own, tab_a);
    return (exact_from_table(own, digits, rw) ? 1 : 0) + 2 + 4;
  }
  const bool neutral = wide ? verify_half_main_lane<false, HALF_WINDOWS_SMALL>(hd, tab_a, rtab, base().at(), false, 1, g_ks.tab())
                            : verify_half_main_lane<false, HALF_WINDOWS>(hd, tab_a, rtab, base().at(), false, 1, g_ks.tab());
  return neutral && rvalid ? 1 : 0;
}

// 1 when nothing of the key set changed since kc_build (no pass writes it)
int kc_keyset_untouched(void) {
  for (size_t k = 0; k < g_ks.count; k++)
    if (!kc_table_matches(k)) return 0;
  return 1;
}

}  // extern "C"
