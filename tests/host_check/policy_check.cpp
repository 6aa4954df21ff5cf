// policy_check.cpp - TEST BINARY: verify_policy_lane (libeddsa_amd/csrc/policy_lanes.h) - the lane of k_verify_policy, the kernel
// behind the opt-in strict rules of include/eddsa_amd.h (EDDSA_AMD_VERIFY_*) - compiled for the host CPU with -DED_HOST_CHECK
// (every bound asserted).  Built by tests/test_policy_lane_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "policy_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

extern "C" {

long pc_violations(void) { return g_violations.load(); }

// n items: sigs 64 bytes each (R | S), pubs 32 bytes each -> out[i] = verify_policy_lane(R, S, A, policy)
void pc_policy(uint8_t* out, const uint8_t* sigs, const uint8_t* pubs, size_t n, unsigned policy) {
  for (size_t i = 0; i < n; i++) {
    uint32_t rw[8], sw[8], aw[8];
    memcpy(rw, sigs + 64 * i, 32);                             // little-endian host
    memcpy(sw, sigs + 64 * i + 32, 32);
    memcpy(aw, pubs + 32 * i, 32);
    out[i] = (uint8_t)verify_policy_lane(rw, sw, aw, policy);
  }
}

}  // extern "C"
