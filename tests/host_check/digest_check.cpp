// digest_check.cpp - TEST BINARY: verify_digest_lane and rlc_digest_lane (libeddsa_amd/csrc/lanes.h, rlc_lanes.h) - the lanes of the
// kernels behind ed25519_verify_digests* - compiled for the host CPU with -DED_HOST_CHECK (every bound asserted), beside the
// hashing lanes they are the tail of.  Built by tests/test_digest_lane_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "lanes.h"
#include "rlc_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

extern "C" {

long dc_violations(void) { return g_violations.load(); }

// n digests of 64 bytes -> n x 32 bytes: the digit words verify_digest_lane leaves (t + 0x88..88, little-endian)
void dc_verify_digest(uint8_t* out, const uint8_t* digests, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint32_t dw[16], tw[8];
    memcpy(dw, digests + 64 * i, 64);                          // little-endian host
    verify_digest_lane(tw, dw);
    memcpy(out + 32 * i, tw, 32);
  }
}

// the digit words verify_hash_lane leaves for (R, A, M)
void dc_verify_hash(uint8_t out[32], const uint8_t r[32], const uint8_t a[32], const uint8_t* msg, size_t len) {
  uint32_t rw[8], aw[8], tw[8];
  memcpy(rw, r, 32); memcpy(aw, a, 32);
  verify_hash_lane(tw, rw, aw, msg, len);
  memcpy(out, tw, 32);
}

// what the two forms of the batch verification's hashing lane leave for one item: t | S mod l | leaf, 96 bytes each
void dc_rlc_both(uint8_t from_msg[96], uint8_t from_digest[96], const uint8_t sig[64], const uint8_t a[32], const uint8_t* msg, size_t len,
                 const uint8_t digest[64]) {
  uint32_t rw[8], aw[8], sw[8], tw[8], lf[8], dw[16];
  memcpy(rw, sig, 32); memcpy(aw, a, 32);
  memcpy(sw, sig + 32, 32);
  rlc_hash_lane(tw, sw, lf, rw, aw, sig + 32, msg, len);
  memcpy(from_msg, tw, 32); memcpy(from_msg + 32, sw, 32); memcpy(from_msg + 64, lf, 32);
  memcpy(sw, sig + 32, 32); memcpy(dw, digest, 64);
  rlc_digest_lane(tw, sw, lf, dw, sig + 32);
  memcpy(from_digest, tw, 32); memcpy(from_digest + 32, sw, 32); memcpy(from_digest + 64, lf, 32);
}

}  // extern "C"
