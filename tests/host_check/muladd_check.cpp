// muladd_check.cpp - TEST BINARY: the lane sequence of ed25519_point_muladd_batch (include/eddsa_amd.h) - point_muladd_prepare_lane
// (libeddsa_amd/csrc/muladd_lanes.h), then verify_main_lane and encode_lane (lanes.h), what k_point_muladd_prepare, k_verify_main and
// k_point_muladd_finish run - compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).  Built by
// tests/test_point_muladd_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "muladd_lanes.h"

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

long mc_violations(void) { return g_violations.load(); }

// n items of 32 bytes each -> out[i] = the 32 bytes of [mul_i]points_i + [add_i]B, flags[i] = the lane's flag byte.  mul / add NULL:
// m = 1 / a = 0, handed to the lane as the kernel hands them.  Every item gets a digit slot and a table dirtied first: the lane must
// write all it leaves for the chain.  The inversion is the item's own (fe_inv): the shared one is the finish kernel's business.
void mc_muladd(uint8_t* out, uint8_t* flags, const uint8_t* points, const uint8_t* mul, const uint8_t* add, size_t n) {
  alignas(128) static uint32_t tab[VERIFY_ITEM_TABLE_WORDS];
  for (size_t i = 0; i < n; i++) {
    uint32_t pw[8], mw[8] = {1, 0, 0, 0, 0, 0, 0, 0}, aw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8];
    alignas(16) uint32_t digits[VERIFY_DIGIT_WORDS];
    memcpy(pw, points + 32 * i, 32);                           // little-endian host
    if (mul) memcpy(mw, mul + 32 * i, 32);
    if (add) memcpy(aw, add + 32 * i, 32);
    memset(tab, 0xa5, sizeof(tab));
    memset(digits, 0x5a, sizeof(digits));
    flags[i] = point_muladd_prepare_lane(digits, tab, pw, mw, aw);
    ge acc;
    verify_main_lane(acc, digits, tab, table().at());
    if (flags[i] & MULADD_ON_CURVE) {
      fe zinv;
      fe_inv(zinv, acc.Z);
      encode_lane(w, acc.X, acc.Y, zinv);
    } else {
      if (!ge_is_neutral(acc)) bound_violation(__FILE__, __LINE__, "an item off the curve walks the neutral element");
      point_muladd_no_point(w);
    }
    memcpy(out + 32 * i, w, 32);
  }
}

// the centred scalar alone: mag = |m'| (32 bytes, little-endian), returns m' < 0
int mc_scalar(uint8_t mag[32], const uint8_t m[32]) {
  uint32_t mw[8], g[8];
  memcpy(mw, m, 32);
  const bool neg = point_muladd_scalar_lane(g, mw);
  memcpy(mag, g, 32);
  return (int)neg;
}

}  // extern "C"
