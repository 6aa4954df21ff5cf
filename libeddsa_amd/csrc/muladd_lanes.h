// muladd_lanes.h - the set-up of [m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch) as what ONE lane computes: plain
// words in, words out, like policy_lanes.h and classify_lanes.h, so that the same source compiles for the host under
// -DED_HOST_CHECK (tests/host_check/muladd_check.cpp, every bound asserted).  The chain itself is lanes.h: verify_main_lane over
// what this lane writes - the pass computes [t](-A) + [S]B with t := |m'|, -A := sign(m') P, S := a mod l - and the encoding is
// lanes.h: encode_lane.
//
// Why m is taken mod 8 l and not mod l: P is ANY curve point.  The group has 8 l elements; a point with a component of order 2, 4 or
// 8 is sent to different points by m and by m mod l (m - m mod l is a multiple of l, and [l] does not kill the torsion component).
// 8 l is the exponent of the group, so m mod 8 l is exact for every P.  rlc_lanes.h: rlc_key_scalar_mod_8l already finds the
// representative m' = m (mod 8 l) with |m'| <= 4 l < 2^255 from m mod l and the low bits of m; its magnitude fits the 64 signed
// four-bit windows of the chain (top digit at most 5), its sign goes into the table.  B has order l: a is taken mod l.
#pragma once
#include "lanes.h"
#include "rlc_lanes.h"

namespace ed {

// flag[item] of a muladd pass (the flags array of the verify workspace): P decoded to a curve point
enum : uint8_t { MULADD_ON_CURVE = 1 };

// m as an integer of 256 bits -> mag = |m'|, returns m' < 0, where m' = m (mod 8 l) and |m'| <= 4 l
ED_DEV bool point_muladd_scalar_lane(uint32_t mag[8], const uint32_t mw[8]) {
  sc m;
  uint32_t m0[8];
  sc_from_words<8>(m, mw);                       // m mod l: not range-checked, any 256 bits (sc.c:191-214)
  sc_to_words(m0, m);
  const bool neg = rlc_key_scalar_mod_8l(mag, m0, mw[0], 1u);   // m = m0 + k l: k mod 8 from the low words, centred
  ED_CHECK(mag[7] < 0x80000000u);                // |m'| < 2^255: the recoding below carries nothing out of bit 255
  return neg;
}

// eight words to memory (the device: two 16-byte stores, p 16-byte aligned, as kernel_io.h: store8)
ED_DEV void muladd_store8(uint32_t* p, const uint32_t w[8]) {
  word4* o = reinterpret_cast<word4*>(p);
  o[0] = word4{w[0], w[1], w[2], w[3]};
  o[1] = word4{w[4], w[5], w[6], w[7]};
}

// pw = P, mw = m, aw = a, eight little-endian words each (an absent array: the kernel hands in m = 1, a = 0).
// Writes the item's 16 digit words at `digits` in k_verify_main's format (|m'| + 0x88.. in the t slot, a mod l + 0x8000.. in the S
// slot, as lanes.h: verify_s_lane makes them) and the nine-entry table of 0..8 times sign(m') P at tab (both 16-byte aligned memory);
// returns the flag byte.  A string that is no curve point gets the neutral element's table and the digits of 0 and 0: the chain then
// walks curve points only (its additions are complete ON the curve), and the finish kernel writes the no-point string for it.
// The digit words are stored before the point is decoded and, for a string off the curve, stored again: held in registers across the
// square root and the table they cost the kernel 21 spilled registers (the table alone wants 245, as in k_keyset_build).
ED_DEV uint8_t point_muladd_prepare_lane(uint32_t* digits, uint32_t* tab, const uint32_t pw[8], const uint32_t mw[8], const uint32_t aw[8]) {
  bool neg;
  {
    uint32_t mag[8], sw[8];
    neg = point_muladd_scalar_lane(mag, mw);
    words_add_pattern(mag, 0x88888888u);
    muladd_store8(digits, mag);
#pragma unroll
    for (int q = 0; q < 8; q++) sw[q] = aw[q];
    verify_s_lane(sw);
    muladd_store8(digits + 8, sw);
  }
  ge p, o;
  bool oncurve;
  ge_frombytes(p, oncurve, pw, neg);             // sign(m') P, Z = 1
  ge_neutral(o);
  fe_cmov(p.X, o.X, !oncurve); fe_cmov(p.Y, o.Y, !oncurve); fe_cmov(p.T, o.T, !oncurve);
  if (!oncurve) {
    uint32_t z[8];
#pragma unroll
    for (int q = 0; q < 8; q++) z[q] = 0x88888888u;
    muladd_store8(digits, z);
#pragma unroll
    for (int q = 0; q < 8; q++) z[q] = 0x80008000u;
    muladd_store8(digits + 8, z);
  }
  verify_table_point_lane(tab, p);
  return (uint8_t)(oncurve ? MULADD_ON_CURVE : 0);
}

// the string of an item whose P is no curve point: 02 00 .. 00 (include/eddsa_amd.h: EDDSA_AMD_NO_POINT_BYTE0; keyed_lanes.h's "no
// key").  y = 2 is on no curve point, so it is never a result
ED_DEV void point_muladd_no_point(uint32_t w[8]) {
  w[0] = 2u;
#pragma unroll
  for (int q = 1; q < 8; q++) w[q] = 0u;
}

}  // namespace ed
