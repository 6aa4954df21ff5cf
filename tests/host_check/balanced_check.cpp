// balanced_check.cpp - TEST BINARY: the balanced pair search (libeddsa_amd/csrc/halve.h: halve_balanced_lane) and the steps of
// a full-size verify pass that run on it (lanes.h: verify_half_scalars_lane<HALF_BITS_BALANCED>, verify_half_main_lane<false,
// HALF_WINDOWS_BALANCED>), compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).  Built by
// tests/test_balanced_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "lanes.h"

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
}  // namespace

extern "C" {

long bc_violations(void) { return g_violations.load(); }
const char* bc_first_violation(void) { return g_first; }
void bc_reset(void) { g_violations = 0; g_first[0] = 0; }

// halve_balanced_lane on n scalars t (32 bytes each); out48 per item as eddsa_amd_probe_halve writes it:
// v (20 bytes) | |u| (20) | u < 0 (1) | found (1) | 6 bytes of padding
void bc_halve(uint8_t* out48, const uint8_t* t32, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint32_t tw[8], vw[5], uw[5];
    memcpy(tw, t32 + 32 * i, 32);
    bool neg;
    const bool found = halve_balanced_lane(vw, uw, neg, tw);
    uint8_t* o = out48 + 48 * i;
    memcpy(o, vw, 20); memcpy(o + 20, uw, 20);
    o[40] = neg ? 1 : 0; o[41] = found ? 1 : 0;
    memset(o + 42, 0, 6);
  }
}

// fault injection into the pair search (halve.h: HALVE_FAULT, HALVE_FAULT_COFACTOR)
void bc_halve_fault(int n) { halve_fault = n; }

void bc_halve_counters(long out[2], int reset) {
  out[0] = halve_counters[0]; out[1] = halve_counters[1];
  if (reset) halve_counters[0] = halve_counters[1] = 0;
}

// One item as a full-size pass takes it (k_verify_prepare, k_verify_halve<HALF_BITS_BALANCED>, k_verify_main_half<33>):
// 0 / 1 = the verdict of the 33-window evaluation, 2 = the item goes to the exact path (key off the curve, or no pair);
// + 8: the search returned a pair that the integer check of verify_half_scalars_lane refused (then 2: the item is long).
// hd_out (HALF_DIGIT_WORDS words, may be null): the item's digit words
int bc_verify(const uint8_t sig[64], const uint8_t pub[32], const uint8_t* msg, size_t len, uint32_t* hd_out) {
  alignas(16) uint32_t tab[VERIFY_ITEM_TABLE_WORDS], rtab[VERIFY_ITEM_TABLE_WORDS];
  uint32_t rw[8], sw[8], aw[8], tw[8], hd[HALF_DIGIT_WORDS];
  memcpy(rw, sig, 32); memcpy(sw, sig + 32, 32); memcpy(aw, pub, 32);
  const bool oncurve = verify_prepare_lane(tw, sw, tab, rw, aw, msg, len);
  verify_half_scalars_lane<HALF_BITS_BALANCED>(hd, tw, sw);
  if (hd_out) memcpy(hd_out, hd, sizeof(hd));
  const bool rvalid = verify_half_point_lane(rtab, rw);
  const int refused = (hd[HALF_STATUS_WORD] & HALF_PAIR_REFUSED) ? 8 : 0;
  if (!oncurve || (hd[HALF_STATUS_WORD] & HALF_LONG) != 0) return 2 + refused;
  return (verify_half_main_lane<false, HALF_WINDOWS_BALANCED>(hd, tab, rtab, base().at(), false) && rvalid ? 1 : 0) + refused;
}

}  // extern "C"
