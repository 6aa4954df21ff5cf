// cofactor_lanes.h - the opt-in cofactored equation of verification (include/eddsa_amd.h: eddsa_amd_set_verify_equation,
// the rules of ZIP-215) as what ONE lane computes: plain words and pointers in, a bool out, like lanes.h, so that the same
// source compiles for the host under -DED_HOST_CHECK (tests/host_check/cofactor_check.cpp, every limb bound asserted).
//
// An item (R, S, A) with t = the hash mod l is accepted exactly when S < l, A and R decode to curve points - permissively:
// y is the low 255 bits mod p, x = 0 takes either sign bit - and [8]([S]B - [t]A - R) is the neutral element.  The lane is
// the full-length windowed evaluation of the cofactorless pass (lanes.h: verify_main_lane, over the digit words that pass's
// prepare kernel left in the workspace) with -R added and three doublings in front of a projective neutrality test: no
// inversion, no export, no comparison of bytes.  Any representative of t mod l and of S mod l gives the same answer - the
// three doublings kill what a multiple of l adds on a component of order dividing 8.
#pragma once
#include "lanes.h"
#include "policy_lanes.h"

namespace ed {

// Two steps, because two kernels run them (kernels.hip: k_cofactor_points, k_cofactor_eval - the decodings want twice the
// registers the windows can have without scratch, like k_verify_prepare and k_verify_main).

// rw, sw, aw: the item's R, S and A as little-endian words (S raw, as the caller sent it); tab: the item's table slot,
// REBUILT here as 0..8 times -A (the exact path may have written over entries 2 and 3); rslot: VERIFY_ENTRY_WORDS words of
// the item's own (its rtable slot, which no kernel reads any more), where -R waits in cached form.  Returns whether S < l
// and both encodings decode to curve points: what the equation's answer is worth anything for.
ED_DEV bool cofactor_points_lane(const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8], uint32_t* tab, uint32_t* rslot) {
  bool good = words_below_l(sw);
  {
    ge r;
    bool r_oncurve;
    ge_frombytes(r, r_oncurve, rw, true);        // -R, Z = 1
    good = good && r_oncurve;
    ge_cached c;
    ge_to_cached(c, r);
    cached_store(rslot, 0, c);
  }
  const bool a_oncurve = verify_table_lane(tab, aw);
  return good && a_oncurve;
}

// Is [8]([S]B - [t]A - R) the neutral element?  digits: the item's 16 digit words (edk_layout.h: VERIFY_DIGIT_WORDS;
// t + 0x88.. | S mod l + 0x8000..), read from memory window by window; tab, rslot: what cofactor_points_lane left;
// base16: the k * B table.  Meaningless (and harmless) when that lane returned false: the points are then not on the curve.
ED_DEV bool cofactor_equation_lane(const uint32_t* digits, const uint32_t* tab, const uint32_t* rslot, const uint32_t* base16) {
  ge acc;
  verify_main_lane(acc, digits, tab, base16);    // [S]B - [t]A as (X : Y : Z); the last addition computed no T
  {
    // the same point with its T: (X Z : Y Z : Z^2 : X Y)
    fe t;
    fe_mul(t, acc.X, acc.Y);
    fe_mul(acc.X, acc.X, acc.Z);
    fe_mul(acc.Y, acc.Y, acc.Z);
    fe_sq(acc.Z, acc.Z);
    acc.T = t;
  }
  ge_cached c;
  cached_load(c, rslot, 0);
  ge_add_cached(acc, acc, c, false);
#pragma unroll 1
  for (int k = 0; k < 3; k++) ge_dbl(acc, acc, false);
  return ge_is_neutral(acc);
}

// the item's verdict under the cofactored equation: both steps
ED_DEV bool verify_cofactored_lane(const uint32_t rw[8], const uint32_t sw[8], const uint32_t aw[8], const uint32_t* digits,
                                   uint32_t* tab, uint32_t* rslot, const uint32_t* base16) {
  const bool good = cofactor_points_lane(rw, sw, aw, tab, rslot);
  const bool neutral = cofactor_equation_lane(digits, tab, rslot, base16);
  return good && neutral;
}

}  // namespace ed
