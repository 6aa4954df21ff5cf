// classify_lanes.h - what a 32-byte string IS as a point (include/eddsa_amd.h: ed25519_point_classify_batch,
// EDDSA_AMD_POINT_*) as what ONE lane computes: plain words in, an unsigned out, like policy_lanes.h and cofactor_lanes.h,
// so that the same source compiles for the host under -DED_HOST_CHECK (tests/host_check/classify_check.cpp, every limb
// bound asserted).  Three of the four bits are tests the verify pass already has (policy_lanes.h: encoding_y_ge_p,
// decoded_canonical, encoding_small_order, over ge25519.h's ge_frombytes); the fourth, "is [l]P the neutral element", is
// the one chain below.
#pragma once
#include "lanes.h"
#include "policy_lanes.h"

namespace ed {

// the class byte's bits: include/eddsa_amd.h, EDDSA_AMD_POINT_*
enum : unsigned { POINT_ON_CURVE = 0x01, POINT_CANONICAL = 0x02, POINT_SMALL_ORDER = 0x04, POINT_PRIME_SUBGROUP = 0x08 };

// l in non-adjacent form, sum over i of d_i 2^i with d_i in {-1, 0, 1} and no two neighbours both nonzero, as two bit strings:
// bit i of nz says d_i != 0, bit i of neg says d_i = -1.  Derived from l_word() at compile time, not typed in.
struct l_naf { uint32_t nz[8], neg[8]; };
constexpr int L_NAF_TOP = 252;                   // l = 2^252 + (a 125-bit number): d_252 = 1 is the leading digit

constexpr l_naf l_naf_digits() {
  uint32_t k[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // what is left of l (a ninth word: room for the carry of k + 1)
  for (int q = 0; q < 8; q++) k[q] = l_word(q);
  l_naf d = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
  for (int i = 0; i < 256; i++) {
    if (k[0] & 1u) {
      d.nz[i >> 5] |= 1u << (i & 31);
      if ((k[0] & 3u) == 3u) {                   // d_i = -1: k + 1 is a multiple of 4
        d.neg[i >> 5] |= 1u << (i & 31);
        for (int q = 0; q < 9; q++) { k[q] += 1u; if (k[q] != 0u) break; }
      } else {
        k[0] -= 1u;                              // d_i = 1
      }
    }
    for (int q = 0; q < 8; q++) k[q] = (k[q] >> 1) | (k[q + 1] << 31);
    k[8] >>= 1;
  }
  return d;
}

// (sum of the positive digits) - (sum of the negative ones) = l, the digits are non-adjacent, d_252 = 1 leads and d_0 != 0
constexpr bool l_naf_recomposes(const l_naf& d) {
  uint64_t borrow = 0;
  for (int q = 0; q < 8; q++) {
    const uint64_t t = (uint64_t)(d.nz[q] & ~d.neg[q]) - (d.nz[q] & d.neg[q]) - borrow;
    if ((uint32_t)t != l_word(q)) return false;
    borrow = t >> 63;
  }
  if (borrow != 0) return false;
  for (int i = 0; i < 255; i++)
    if ((d.nz[i >> 5] >> (i & 31) & 1u) && (d.nz[(i + 1) >> 5] >> ((i + 1) & 31) & 1u)) return false;
  for (int i = L_NAF_TOP + 1; i < 256; i++)
    if (d.nz[i >> 5] >> (i & 31) & 1u) return false;
  return (d.nz[L_NAF_TOP >> 5] >> (L_NAF_TOP & 31) & 1u) && !(d.neg[L_NAF_TOP >> 5] >> (L_NAF_TOP & 31) & 1u) && (d.nz[0] & 1u);
}
static_assert(l_naf_recomposes(l_naf_digits()), "the signed digits of l recompose to l");

// word q of the two digit strings (q is the same in every lane: a scalar select over eight constants, no table in memory)
ED_DEV constexpr uint32_t l_naf_nz_word(int q) { constexpr l_naf d = l_naf_digits(); return d.nz[q]; }
ED_DEV constexpr uint32_t l_naf_neg_word(int q) { constexpr l_naf d = l_naf_digits(); return d.neg[q]; }

// Is [l]p the neutral element?  p: a curve point with Z = 1 and its T (what ge_frombytes returns), of ANY order - ge_dbl and
// ge_add_cached are complete on the curve, so a point of order 2, 4 or 8 and a point of mixed order walk the same chain as an
// honest key.  Left to right over the non-adjacent form of l from the accumulator p = d_252 p: 252 doublings and one addition of
// p or -p for each of the 45 other nonzero digits (46 with the leading one), p kept in cached form in registers - no table, no
// memory, no inversion.  Which
// digit comes is a property of l alone: every lane of a wave takes the same branch.  A doubling computes T only in front of
// an addition; an addition never does, because a doubling (non-adjacent digits) or the neutrality test follows it.
ED_DEV bool ge_mul_l_is_neutral(const ge& p) {
  ge_cached pc;
  ge_to_cached(pc, p);
  ge acc = p;
#pragma unroll 1
  for (int i = L_NAF_TOP - 1; i >= 0; i--) {
    const uint32_t bit = 1u << (i & 31);
    const bool add = (l_naf_nz_word(i >> 5) & bit) != 0, neg = (l_naf_neg_word(i >> 5) & bit) != 0;
    ge_dbl(acc, acc, add);
    if (add) {
      ge_cached q = pc;
      ge_cached_cneg(q, neg);
      ge_add_cached(acc, acc, q, false);
    }
  }
  return ge_is_neutral(acc);
}

// the class of the 32 bytes w (little-endian words): POINT_* bits, 0 for a string that is no curve point - such a lane leaves
// before the chain.  ON_CURVE is the reference's permissive import (y = the low 255 bits mod p, x = 0 under either sign bit),
// CANONICAL what RFC 8032 5.1.3 decodes, SMALL_ORDER [8]P = 0 by the five values of y, PRIME_SUBGROUP [l]P = 0.
ED_DEV unsigned point_classify_lane(const uint32_t w[8]) {
  const bool y_ge_p = encoding_y_ge_p(w);
  ge p;
  bool oncurve;
  ge_frombytes(p, oncurve, w, false);
  if (!oncurve) return 0;
  unsigned cls = POINT_ON_CURVE;
  if (decoded_canonical(y_ge_p, w[7] >> 31, p, oncurve)) cls |= POINT_CANONICAL;
  if (encoding_small_order(w)) cls |= POINT_SMALL_ORDER;
  if (ge_mul_l_is_neutral(p)) cls |= POINT_PRIME_SUBGROUP;
  return cls;
}

}  // namespace ed
