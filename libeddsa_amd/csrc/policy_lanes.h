// policy_lanes.h - the opt-in strict rules of verification (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*) as what ONE lane
// computes: plain words in, a bool out, like lanes.h, so that the same source compiles for the host under -DED_HOST_CHECK
// (tests/host_check/policy_check.cpp, every limb bound asserted).  The tests on an encoding's y - below p, one of the five
// values of the points of order dividing 8 - are the ones the batch verification routes by (rlc_lanes.h calls them here).
#pragma once
#include "lanes.h"

namespace ed {

// l as eight little-endian words
ED_DEV constexpr uint32_t l_word(int i) {
  constexpr uint32_t Lw[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0x00000000u, 0x00000000u, 0x00000000u, 0x10000000u};
  return Lw[i];
}

// the 32 bytes w as a little-endian integer: is it below l?  (one borrow chain of w - l)
ED_DEV bool words_below_l(const uint32_t w[8]) {
  uint64_t borrow = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) borrow = ((uint64_t)w[q] - l_word(q) - borrow) >> 63;
  return borrow != 0;
}

// the low 255 bits of a point encoding: is that y at least p = 2^255 - 19?
ED_DEV bool encoding_y_ge_p(const uint32_t w[8]) {
  return (w[7] & 0x7fffffffu) == 0x7fffffffu && (w[1] & w[2] & w[3] & w[4] & w[5] & w[6]) == 0xffffffffu && w[0] >= 0xffffffedu;
}

// Is y mod p the y of one of the eight points of order dividing 8?  Those are exactly the curve points with y in
// {0, 1, -1, y8, -y8} (y8 = the y of a point of order 8), and all five values are on the curve: five comparisons of the
// canonical y replace three doublings and a neutrality test.  Any y with limbs below 2^31.
ED_DEV bool fe_small_order_y(const fe& y) {
  constexpr uint32_t Y8[10] = {60155942, 32288931, 6862340, 26496934, 63071167, 28106709, 31680898, 18229030, 47743011, 1569101};
  constexpr uint32_t Y8N[10] = {6952903, 1265500, 60246523, 7057497, 4037696, 5447722, 35427965, 15325401, 19365852, 31985330};
  fe t;
  fe_canon(t, y);
  uint32_t rest = 0, m1 = 0, d8 = 0, d8n = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    if (i) rest |= t.v[i];
    m1 |= t.v[i] ^ (i == 0 ? M26 - 19 : limb_mask(i));      // p - 1
    d8 |= t.v[i] ^ Y8[i];
    d8n |= t.v[i] ^ Y8N[i];
  }
  return (rest == 0 && t.v[0] <= 1u) || m1 == 0 || d8 == 0 || d8n == 0;
}
// the same from the 32 bytes of an encoding (the sign bit is no part of y; y >= p is reduced: the non-canonical encodings
// of those points count)
ED_DEV bool encoding_small_order(const uint32_t w[8]) {
  uint32_t yw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) yw[i] = w[i];
  yw[7] &= 0x7fffffffu;
  fe y;
  fe_frombytes(y, yw);                           // tight (value < 2^255)
  return fe_small_order_y(y);
}

// Is a 32-byte string the encoding RFC 8032 5.1.3 decodes: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) has a root, and the sign bit is
// clear when that root is 0?  y_ge_p = encoding_y_ge_p of the bytes, sign = their top bit, (p, oncurve) = what ge_frombytes
// returned for them (negated or not: x = 0 is its own negative)
ED_DEV bool decoded_canonical(bool y_ge_p, uint32_t sign, const ge& p, bool oncurve) {
  return oncurve && !y_ge_p && !(sign != 0 && fe_iszero(p.X));
}

// the policy word's bits: include/eddsa_amd.h, EDDSA_AMD_VERIFY_*
enum : unsigned { POLICY_S_BELOW_L = 0x100, POLICY_A_CANONICAL = 0x200, POLICY_A_NOT_SMALL = 0x400, POLICY_R_NOT_SMALL = 0x800 };

// Does the item (R, S, A) satisfy every predicate whose bit is set in `policy`?  The verdict of the item is the
// reference's AND this.  The decoding of A (one fe_pow2523) runs only under POLICY_A_CANONICAL.
ED_DEV bool verify_policy_lane(const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8], unsigned policy) {
  bool good = true;
  if (policy & POLICY_S_BELOW_L) good = good && words_below_l(sw);
  if (policy & POLICY_A_NOT_SMALL) good = good && !encoding_small_order(aw);
  if (policy & POLICY_R_NOT_SMALL) good = good && !encoding_small_order(rw);
  if (policy & POLICY_A_CANONICAL) {
    const bool y_ge_p = encoding_y_ge_p(aw);
    ge p;
    bool oncurve;
    ge_frombytes(p, oncurve, aw, false);
    good = good && decoded_canonical(y_ge_p, aw[7] >> 31, p, oncurve);
  }
  return good;
}

}  // namespace ed
