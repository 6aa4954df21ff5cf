// classify_check.cpp - TEST BINARY: point_classify_lane (libeddsa_amd/csrc/classify_lanes.h) - the lane of k_point_classify, the
// kernel behind ed25519_point_classify_batch and eddsa_amd_keyset_classify of include/eddsa_amd.h - compiled for the host CPU with
// -DED_HOST_CHECK (every bound asserted).  Built by tests/test_classify_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "classify_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

extern "C" {

long cc_violations(void) { return g_violations.load(); }

// n strings of 32 bytes -> cls[i] = point_classify_lane(the string)
void cc_classify(uint8_t* cls, const uint8_t* points, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint32_t w[8];
    memcpy(w, points + 32 * i, 32);                            // little-endian host
    cls[i] = (uint8_t)point_classify_lane(w);
  }
}

// the chain alone, for a string that decodes: -1 when it does not, else whether [l]P is the neutral element
int cc_mul_l_is_neutral(const uint8_t point[32]) {
  uint32_t w[8];
  memcpy(w, point, 32);
  ge p;
  bool oncurve;
  ge_frombytes(p, oncurve, w, false);
  return oncurve ? (int)ge_mul_l_is_neutral(p) : -1;
}

// the signed digits of l the chain walks: digits[i] in {-1, 0, 1} for i = 0 .. 255, as the lane reads them word by word
void cc_l_digits(int8_t digits[256]) {
  for (int i = 0; i < 256; i++) {
    const uint32_t bit = 1u << (i & 31);
    const bool nz = (l_naf_nz_word(i >> 5) & bit) != 0, neg = (l_naf_neg_word(i >> 5) & bit) != 0;
    digits[i] = (int8_t)(nz ? (neg ? -1 : 1) : 0);
  }
}

int cc_l_top(void) { return L_NAF_TOP; }

}  // extern "C"
