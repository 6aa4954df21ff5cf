// cofactor_check.cpp - TEST BINARY: verify_cofactored_lane (libeddsa_amd/csrc/cofactor_lanes.h) - the two lane steps of
// k_cofactor_points and k_cofactor_eval, the kernels behind the opt-in cofactored equation of include/eddsa_amd.h
// (eddsa_amd_set_verify_equation) - compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).  Built by
// tests/test_cofactor_lane_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cofactor_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

namespace {
// base16[k] = k * B, k = 0..32768, as kernels.hip: k_init_tables fills it (the half of the table the full-length windows read)
struct Table {
  std::vector<uint32_t> words;
  uint32_t* at() { return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(words.data()) + 127) & ~(uintptr_t)127); }
  Table() : words((size_t)TABLE_BASE16_ENTRIES * TABLE_ENTRY_WORDS + 32) {
    for (int k = 0; k < TABLE_BASE16_ENTRIES; k++) table_entry_lane(at() + (size_t)TABLE_ENTRY_WORDS * k, (uint32_t)k, 0);
  }
};
Table& table() { static Table t; return t; }
}  // namespace

extern "C" {

long cc_violations(void) { return g_violations.load(); }

// n items: sigs 64 bytes each (R | S), pubs 32 bytes each, digests 64 bytes each (SHA-512(prefix | R | A | M), the caller's)
// -> out[i] = the lane's verdict.  The digit words are made as the prepare kernels make them (lanes.h: verify_digest_lane,
// verify_s_lane); every item gets a table slot and an R slot of its own, dirtied first: the lane must rebuild what it reads.
void cc_cofactored(uint8_t* out, const uint8_t* sigs, const uint8_t* pubs, const uint8_t* digests, size_t n) {
  alignas(128) static uint32_t tab[VERIFY_ITEM_TABLE_WORDS], rslot[VERIFY_ITEM_TABLE_WORDS];
  for (size_t i = 0; i < n; i++) {
    uint32_t rw[8], sw[8], aw[8], dw[16];
    alignas(16) uint32_t digits[VERIFY_DIGIT_WORDS];
    memcpy(rw, sigs + 64 * i, 32);                             // little-endian host
    memcpy(sw, sigs + 64 * i + 32, 32);
    memcpy(aw, pubs + 32 * i, 32);
    memcpy(dw, digests + 64 * i, 64);
    uint32_t sd[8];
    memcpy(sd, sw, 32);
    verify_digest_lane(digits, dw);
    verify_s_lane(sd);
    memcpy(digits + 8, sd, 32);
    memset(tab, 0xa5, sizeof(tab));
    memset(rslot, 0x5a, sizeof(rslot));
    out[i] = (uint8_t)verify_cofactored_lane(rw, sw, aw, digits, tab, rslot, table().at());
  }
}

}  // extern "C"
