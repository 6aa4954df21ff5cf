// halve.h - half-length scalars for Ed25519 verification, one item per lane.
//
// The reference checks  encode(S*B - t*A) == R-bytes  (ed25519-sha512.c:166-180), which costs 252 doublings
// per item because t is a 253-bit scalar on a variable base.  For an item whose A and R both decode to curve
// points (R strictly: lanes.h verify_half_point_lane) that check is the group equation Q := S*B - t*A - R' = 0,
// and for any integer u coprime to the group order 8l it is equivalent to u*Q = 0:
//     (u S mod l)*B  -  v*A  -  u*R'  =  0        with  v = u t  (mod 8 l)
// (B has order l; A and R' have orders dividing 8l, so v*A = u*t*A also when A has a torsion component).
// The extended Euclidean algorithm on (8l, t), stopped half way, gives such a pair with |u|, v < 2^134
// (Antipa, Brown, Gallant, Lambert, Struik, Vanstone: "Accelerated verification of ECDSA signatures", SAC 2005,
// there mod the prime group order; mod 8l and with u odd here so that the equivalence is exact for every input
// on the curve, which is what bit-exactness with the reference's cofactorless check needs).  The evaluation is
// then 132 doublings and three half-length scalars.  Items for which no suitable pair turns up in the two
// candidates examined, or whose expansion has a quotient of 31 bits or more before that which the Lehmer rounds
// have not already used up in partial steps (together about 1 in 10^4 random t), are handed to the exact path like off-curve keys.
//
// Three searches, each with its count of signed four-bit windows (kernels.hip: verify_route_of says which pass takes which):
//   halve_scalar_lane<134>   |u|, v < 2^134, 34 windows   keyed passes of 2^19 items and more, unkeyed ones of up to 256
//   halve_scalar_lane<138>   |u|, v < 2^138, 35 windows   the passes between (2 give-ups in 10^7)
//   halve_balanced_lane      |u|, v <= B33,  33 windows   unkeyed passes of 2^19 items and more (1.9 give-ups in 10^3); the floor:
//                                                         the lattice of the pairs has determinant 2^255, 32 windows hold 2^126.9
// The first two stop at the first remainder below their bound, whose cofactor is then about ten bits shorter than the bound; the
// third stops where remainder and cofactor are of one size and knows a way out of an even cofactor, which a bound with no bits
// to spare needs (with the first rule a bound of 2^131 gives up on 6 t in 10^3).
//
// Public data only (verification): control flow and timing depend on t.
#pragma once
#include "sc25519.h"

namespace ed {

// host test build only: how many Lehmer rounds and how many plain iterations ran (tests/test_device_source_on_host.py)
#ifdef ED_HOST_CHECK
inline thread_local long halve_counters[2];   // (per thread: the sanitizer build of the host side runs this source on several threads)
#define HALVE_COUNT(i) (++::ed::halve_counters[i])
// fault injection (tests only): n > 0 makes the n-th working half-step from now on take a quotient that is one too
// large - the failure the floating-point margins exist to exclude (the remainder wraps; the search then usually runs
// into its own give-up rules) - and n < 0 makes the |n|-th working half-step update the COFACTOR with a quotient one
// too large (remainders, hence the choice of the pair, stay right; the pair's congruence is broken).  Whatever comes
// out, lanes.h: verify_half_scalars_lane must not let a wrong pair through.
inline thread_local int halve_fault;
#define HALVE_FAULT(q, active) do { if ((active) && ::ed::halve_fault > 0 && --::ed::halve_fault == 0) (q) += 1u; } while (0)
#define HALVE_FAULT_COFACTOR(q, active) do { if ((active) && ::ed::halve_fault < 0 && ++::ed::halve_fault == 0) (q) += 1u; } while (0)
#else
#define HALVE_COUNT(i) ((void)0)
#define HALVE_FAULT(q, active) ((void)0)
#define HALVE_FAULT_COFACTOR(q, active) ((void)0)
#endif

constexpr int HALF_WINDOWS = 34;                 // 4-bit signed windows of v and |u|: values < 2^134
constexpr int HALF_BITS = 134;
constexpr int HALF_BITS_SMALL = 138;             // the bound for passes whose main kernel is shorter than the exact path: 35 windows
constexpr int HALF_WINDOWS_SMALL = 35;

// 8 l, little-endian words
ED_DEV constexpr uint32_t halve_N(int i) {
  constexpr uint32_t N[8] = {0xe7ae9f68u, 0xc09318d2u, 0x17bce6b2u, 0xa6f7cef5u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u};
  return N[i];
}

ED_DEV double halve_to_double(const uint32_t w[8]) {
  double d = (double)w[7];
#pragma unroll
  for (int k = 6; k >= 0; k--) d = __builtin_fma(d, 4294967296.0, (double)w[k]);
  return d;                                      // relative error < 2^-50
}

// a < b as 256-bit numbers
ED_DEV bool halve_less(const uint32_t a[8], const uint32_t b[8]) {
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) { c += (int64_t)a[k] - (int64_t)b[k]; c >>= 32; }
  return c != 0;
}

// a < 2^bits
ED_DEV bool halve_below(const uint32_t a[8], int bits) {
  uint32_t hi = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (32 * k >= bits) hi |= a[k];
    else if (32 * (k + 1) > bits) hi |= a[k] >> (bits - 32 * k);
  }
  return hi == 0;
}

// a / b for a >= 0, b > 0, to a relative error far below the 2^-40 margin of its caller: reciprocal estimate
// (v_rcp_f64) and two Newton steps instead of the correctly rounded division's twenty instructions
ED_DEV double halve_ratio(double a, double b) {
#ifdef ED_HOST_CHECK
  return a / b;
#else
  double y = __builtin_amdgcn_rcp(b);
  y = __builtin_fma(__builtin_fma(-b, y, 1.0), y, y);
  y = __builtin_fma(__builtin_fma(-b, y, 1.0), y, y);
  return a * y;
#endif
}

// One half-step of the Euclidean algorithm: (ra, ua) -= q * (rb, ub) with q = an underestimate (>= 1) of
// floor(ra / rb), for lanes with `active` set (which have ra >= rb > 0); q = 0 otherwise.  da, db = ra, rb as
// doubles (halve_to_double).  ua, ub: 160-bit two's complement.  Returns true, and changes nothing, when the
// quotient does not fit 31 bits (one step in 2^31: the caller gives the item up).
ED_DEV bool halve_reduce(uint32_t ra[8], uint32_t ua[5], const uint32_t rb[8], const uint32_t ub[5], double da, double db, bool active) {
  db = active ? db : 1.0;
  double qd = __builtin_floor(halve_ratio(da, db) * (1.0 - 0x1p-40));   // never above the true quotient
  const bool big = active && !(qd < 2147483647.0);
  qd = qd < 2147483647.0 ? qd : 0.0;
  uint32_t q = (uint32_t)qd;
  q = q < 1u ? 1u : q;
  q = active && !big ? q : 0u;
  HALVE_FAULT(q, active && !big);
  uint64_t carry = 0;
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    carry += (uint64_t)q * rb[k];
    c += (int64_t)ra[k] - (int64_t)(uint32_t)carry;
    ra[k] = (uint32_t)c;
    c >>= 32;
    carry >>= 32;
  }
  ED_CHECK(c == 0 && carry == 0);                // q <= floor(ra / rb): no borrow out
  HALVE_FAULT_COFACTOR(q, active && !big);
  carry = 0;
  c = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    carry += (uint64_t)q * ub[k];
    c += (int64_t)ua[k] - (int64_t)(uint32_t)carry;
    ua[k] = (uint32_t)c;
    c >>= 32;
    carry >>= 32;
  }
  return big;
}

// out = a * x - b * y for W-word numbers, a, b < 2^24.  W = 8: the result is known to lie in [0, 2^256) (checked
// on the host build); W = 5: 160-bit two's complement, modulo 2^160.
template <int W>
ED_DEV void halve_combine(uint32_t out[W], uint32_t a, const uint32_t x[W], uint32_t b, const uint32_t y[W]) {
  uint64_t ca = 0, cb = 0;
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < W; k++) {
    ca += (uint64_t)a * x[k];
    cb += (uint64_t)b * y[k];
    c += (int64_t)(uint32_t)ca - (int64_t)(uint32_t)cb;
    out[k] = (uint32_t)c;
    c >>= 32;
    ca >>= 32;
    cb >>= 32;
  }
  ED_CHECK(W != 8 || c + (int64_t)ca - (int64_t)cb == 0);
}

constexpr int HALF_LEHMER_MIN_BITS = 151;        // rounds run while both remainders have more bits than this
// One round of Lehmer's acceleration: many Euclidean half-steps on the remainders as doubles, then ONE exact update
// of the long numbers.  With nonnegative integers a0, b0, a1, b1 (kept below 2^24 as doubles)
//     R0' = a0 R0 - b0 R1,   R1' = b1 R1 - a1 R0      (and the same combinations of U0, U1)
// a half-step "R0' -= q R1'" is a0 += q a1, b0 += q b1.  d0, d1 carry a relative error below 2^-50, so the doubles
// y0, y1 that track R0', R1' are off by less than (a + b) max(d0, d1) 2^-50 < E := max(d0, d1) 2^-24; every
// quotient is taken as floor((y0 - E) / (y1 + E)), which cannot exceed the true one, so each half-step applied is a
// legitimate (possibly partial) Euclidean step and the true remainders stay nonnegative.  A half-step is refused
// when it cannot be shown to leave its remainder above 2^141 - nothing that halve_scalar_lane's rule would have
// to examine (remainders below 2^134, or 2^138) is ever produced here; the plain loop does the last bits.
// Returns whether anything was applied.  FLOOR_BITS: that floor; 141 for halve_scalar_lane, 129 for halve_balanced_lane,
// which examines nothing above 2^128.
ED_DEV constexpr double halve_pow2(int bits) { double d = 1.0; for (int k = 0; k < bits; k++) d *= 2.0; return d; }
static_assert(halve_pow2(141) == 0x1p141 && halve_pow2(129) == 0x1p129, "exact powers of two");
template <int FLOOR_BITS = 141>
ED_DEV bool halve_lehmer_round(uint32_t r0[8], uint32_t r1[8], uint32_t u0[5], uint32_t u1[5], double& d0, double& d1) {
  const double E = (d0 > d1 ? d0 : d1) * 0x1p-24;
  constexpr double FLOOR = halve_pow2(FLOOR_BITS);
  double y0 = d0, y1 = d1, a0 = 1.0, b0 = 0.0, a1 = 0.0, b1 = 1.0;
  bool progress = false, live = true;
  for (int it = 0; it < 40 && live; it++) {
    bool any = false;
    {                                            // R0' by R1'
      const double q = __builtin_floor(halve_ratio(y0 - E, y1 + E) * (1.0 - 0x1p-40));
      const double na = __builtin_fma(q, a1, a0), nb = __builtin_fma(q, b1, b0), ny = __builtin_fma(-q, y1, y0);
      if (q >= 1.0 && na < 0x1p24 && nb < 0x1p24 && ny - E >= FLOOR) { a0 = na; b0 = nb; y0 = ny; any = true; }
    }
    {                                            // R1' by R0'
      const double q = __builtin_floor(halve_ratio(y1 - E, y0 + E) * (1.0 - 0x1p-40));
      const double na = __builtin_fma(q, a0, a1), nb = __builtin_fma(q, b0, b1), ny = __builtin_fma(-q, y0, y1);
      if (q >= 1.0 && na < 0x1p24 && nb < 0x1p24 && ny - E >= FLOOR) { a1 = na; b1 = nb; y1 = ny; any = true; }
    }
    live = any;
    progress = progress || any;
  }
  if (!progress) return false;
  uint32_t t0[8], t1[8], v0[5], v1[5];
  halve_combine<8>(t0, (uint32_t)a0, r0, (uint32_t)b0, r1);
  halve_combine<8>(t1, (uint32_t)b1, r1, (uint32_t)a1, r0);
  halve_combine<5>(v0, (uint32_t)a0, u0, (uint32_t)b0, u1);
  halve_combine<5>(v1, (uint32_t)b1, u1, (uint32_t)a1, u0);
#pragma unroll
  for (int k = 0; k < 8; k++) { r0[k] = t0[k]; r1[k] = t1[k]; }
#pragma unroll
  for (int k = 0; k < 5; k++) { u0[k] = v0[k]; u1[k] = v1[k]; }
  d0 = halve_to_double(r0);
  d1 = halve_to_double(r1);
  return true;
}

// |u| < 2^BITS for a 160-bit two's complement u; mag = |u|, neg = u < 0
template <int BITS = HALF_BITS>
ED_DEV bool halve_magnitude(uint32_t mag[5], bool& neg, const uint32_t u[5]) {
  neg = (u[4] >> 31) != 0;
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    c += neg ? -(int64_t)u[k] : (int64_t)u[k];
    mag[k] = (uint32_t)c;
    c >>= 32;
  }
  return (mag[4] >> (BITS - 128)) == 0;
}

// t (< l, eight words) -> v (five words, 0 <= v < 2^BITS), |u| (five words, < 2^BITS, u odd), uneg = (u < 0)
// with v = u t (mod 8 l).  Returns false when no such pair is among the candidates examined.  BITS = 134 (34 windows)
// gives up on 8.5 t in 10^5, BITS = 138 (35 windows; an even u is retried when r >= 2^118) on 2 in 10^7.
template <int BITS = HALF_BITS>
ED_DEV bool halve_scalar_lane(uint32_t vw[5], uint32_t uw[5], bool& uneg, const uint32_t tw[8]) {
  uint32_t r0[8], r1[8], u0[5], u1[5];
#pragma unroll
  for (int k = 0; k < 8; k++) { r0[k] = halve_N(k); r1[k] = tw[k]; }
#pragma unroll
  for (int k = 0; k < 5; k++) { u0[k] = 0; u1[k] = 0; }
  u1[0] = 1;
  // the candidate is the smaller remainder with its cofactor; which = 1: (r1, u1), 0: (r0, u0)
  bool done = false, good = false, tried = false;
  int which = 1;
  // examine the candidate a completed step has produced (lanes with `fresh` set)
  auto examine = [&](const uint32_t r[8], const uint32_t u[5], bool fresh, int idx) {
    if (!fresh || done) return;
    if (!halve_below(r, BITS)) return;
    if (u[0] & 1u) {
      uint32_t m[5]; bool ng;
      good = halve_magnitude<BITS>(m, ng, u);
      done = true; which = idx;
    } else if (tried || halve_below(r, 256 - BITS)) {   // |u'| <= 8l / r < 2^BITS needs r >= 2^(256 - BITS)
      done = true; good = false; which = idx;
    } else {
      tried = true;
    }
  };
  examine(r1, u1, true, 1);
  double d0 = halve_to_double(r0), d1 = halve_to_double(r1);
  // the bulk of the way down by Lehmer rounds (about 23 bits each) ...
  for (int round = 0; round < 8; round++) {
    if (done || halve_below(r0, HALF_LEHMER_MIN_BITS) || halve_below(r1, HALF_LEHMER_MIN_BITS)) break;
    if (!halve_lehmer_round(r0, r1, u0, u1, d0, d1)) break;
    HALVE_COUNT(0);
  }
  // ... and the rest step by step, every completed step examined; each half-step's comparison also tells the next
  // one whether it has work
  bool act = !done && !halve_less(r0, r1);       // the half-step about to run has ra >= rb
  for (int it = 0; it < 160; it++) {
    if (done) break;
    HALVE_COUNT(1);
    {                                            // r0 by r1
      if (halve_reduce(r0, u0, r1, u1, d0, d1, act)) { done = true; good = false; }
      d0 = halve_to_double(r0);
      const bool lt = halve_less(r0, r1);        // the step is complete
      examine(r0, u0, act && lt, 0);
      act = !done && lt;                         // then r1 > r0: the other half-step has work
    }
    {                                            // r1 by r0
      if (halve_reduce(r1, u1, r0, u0, d1, d0, act)) { done = true; good = false; }
      d1 = halve_to_double(r1);
      const bool lt = halve_less(r1, r0);
      examine(r1, u1, act && lt, 1);
      act = !done && !halve_less(r0, r1);        // r0 >= r1: also after a half-step that had no work or left a partial quotient
    }
  }
  good = good && done;
  uint32_t usel[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    vw[k] = which ? r1[k] : r0[k];
    usel[k] = which ? u1[k] : u0[k];
  }
  halve_magnitude<BITS>(uw, uneg, usel);
  return good;
}

// ---- the balanced search: pairs that fit 33 windows ----
// B33 = 7 (16^33 - 1) / 15 = 0x777...7 (33 nibbles), about 2^130.9: the largest value whose recoding into signed four-bit
// digits (+ 0x88...8, lanes.h) leaves every window above 32 at digit 0.  The lattice {(u, v): u t = v mod 8l} has determinant
// 2^255, so no bound below 2^127.5 can be met by every t, and a 32-window bound (2^126.9) by hardly any: 33 is the floor.
constexpr int HALF_WINDOWS_BALANCED = 33;
constexpr int HALF_BITS_BALANCED = 131;          // the template argument that selects this search where a bound is one (B33 < 2^131)
ED_DEV constexpr uint32_t halve_B33(int i) { return i < 4 ? 0x77777777u : i == 4 ? 0x7u : 0u; }
// the highest window with a nonzero digit in the recoding of B33 + plus (plus = 0, 1), the digits as verify_half_main_lane reads them
constexpr int halve_b33_top_window(uint32_t plus) {
  int top = -1;
  uint64_t c = plus;
  for (int k = 0; k < 8; k++) {
    c += (uint64_t)halve_B33(k) + 0x88888888u;
    const uint32_t w = (uint32_t)c;
    c >>= 32;
    for (int n = 0; n < 8; n++)
      if ((int)((w >> (4 * n)) & 15u) - 8 != 0) top = 8 * k + n;
  }
  return c == 0 ? top : 64;
}
static_assert(halve_b33_top_window(0) == HALF_WINDOWS_BALANCED - 1 && halve_b33_top_window(1) == HALF_WINDOWS_BALANCED,
              "B33 fits 33 windows, B33 + 1 does not");
static_assert(HALF_WINDOWS_BALANCED == HALF_BITS_BALANCED / 4 + 1, "the template argument names the bound's window count like the other two");

// a <= B33 for a W-word number
template <int W>
ED_DEV bool halve_fits_b33(const uint32_t a[W]) {
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < W; k++) { c += (int64_t)halve_B33(k) - (int64_t)a[k]; c >>= 32; }
  return c == 0;                                 // no borrow: B33 - a >= 0
}

constexpr int HALF_BALANCED_STOP_BITS = 128;     // the search stops at the first remainder below 2^128
// The Lehmer rounds must not produce a remainder below the stop, and nothing above it is examined: their floor is one bit above
// it, and a round is started only with ten bits to gain, as 151 stands to 141 (a round costs what three plain iterations do).
// (Measured with the floor seven bits above the stop as 141 stands to 134, 135 / 145: two more plain iterations per item and
// 0.03-0.06 ms on a pass of 2^20: profiles/verify_balanced_pairs.txt.)
constexpr int HALF_BALANCED_LEHMER_FLOOR = 129, HALF_BALANCED_LEHMER_MIN_BITS = 139;
static_assert(HALF_BALANCED_LEHMER_FLOOR > HALF_BALANCED_STOP_BITS && HALF_BALANCED_LEHMER_MIN_BITS == HALF_BALANCED_LEHMER_FLOOR + HALF_LEHMER_MIN_BITS - 141,
              "no round reaches below the stop; the rounds' two thresholds keep their distance");
// t (< l) -> v, |u| (five words each, both <= B33, u odd), uneg = (u < 0) with v = u t (mod 8 l); false when the candidates
// hold no such pair (1.7 t in 10^3).  halve_scalar_lane takes the first remainder below its bound, which leaves |u| ten bits
// shorter than v; a bound of 33 windows has no room for that.  Here the search runs to the first remainder r_k < 2^128 (then
// |u_k| <= 8l / r_(k-1) < 2^127: both fit) and takes (u_k, r_k) when u_k is odd.  When it is even, u_(k-1) is odd and so is
// every u_(k-1) - j u_k: the candidates are the pairs (u_(k-1) - j u_k, r_(k-1) - j r_k), j = 0 (the step before), 1, 2, ...
// (partial steps) up to the quotient (the step after), in that order.  Their remainders fall and their cofactors grow with j,
// so the first j whose remainder is <= B33 decides: j = 0 when r_(k-1) <= B33, else floor((r_(k-1) - B33 - 1) / r_k) + 1.  (The
// step after is never that one: the last partial step before it leaves r_k + r_(k+1) < 2^129 < B33.)  Where that candidate's
// cofactor does not fit, no completed or partial step with an odd cofactor fits - earlier ones have larger remainders, later
// ones larger cofactors - so the result is a function of t alone and the give-ups are those of a search over all of them.
ED_DEV bool halve_balanced_lane(uint32_t vw[5], uint32_t uw[5], bool& uneg, const uint32_t tw[8]) {
  uint32_t r0[8], r1[8], u0[5], u1[5];
#pragma unroll
  for (int k = 0; k < 8; k++) { r0[k] = halve_N(k); r1[k] = tw[k]; }
#pragma unroll
  for (int k = 0; k < 5; k++) { u0[k] = 0; u1[k] = 0; }
  u1[0] = 1;
  // hit: a completed step has left a remainder below 2^128; which = 1: it is r1 (the step before: r0), 0: the other way round
  bool hit = halve_below(r1, HALF_BALANCED_STOP_BITS), bad = false;
  int which = 1;
  double d0 = halve_to_double(r0), d1 = halve_to_double(r1);
  for (int round = 0; round < 8; round++) {
    if (hit || halve_below(r0, HALF_BALANCED_LEHMER_MIN_BITS) || halve_below(r1, HALF_BALANCED_LEHMER_MIN_BITS)) break;
    if (!halve_lehmer_round<HALF_BALANCED_LEHMER_FLOOR>(r0, r1, u0, u1, d0, d1)) break;
    HALVE_COUNT(0);
  }
  // the plain loop of halve_scalar_lane; its `done` is hit || bad here
  bool act = !hit && !halve_less(r0, r1);
  for (int it = 0; it < 160; it++) {
    if (hit || bad) break;
    HALVE_COUNT(1);
    {                                            // r0 by r1
      if (halve_reduce(r0, u0, r1, u1, d0, d1, act)) bad = true;
      d0 = halve_to_double(r0);
      const bool lt = halve_less(r0, r1);
      if (!bad && act && lt && halve_below(r0, HALF_BALANCED_STOP_BITS)) { hit = true; which = 0; }
      act = !hit && !bad && lt;
    }
    {                                            // r1 by r0
      if (halve_reduce(r1, u1, r0, u0, d1, d0, act)) bad = true;
      d1 = halve_to_double(r1);
      const bool lt = halve_less(r1, r0);
      if (!bad && act && lt && halve_below(r1, HALF_BALANCED_STOP_BITS)) { hit = true; which = 1; }
      act = !hit && !bad && !halve_less(r0, r1);
    }
  }
  // (ra, ua): the step before, (rb, ub): the hit
  uint32_t ra[8], rb[8], ua[5], ub[5];
#pragma unroll
  for (int k = 0; k < 8; k++) { ra[k] = which ? r0[k] : r1[k]; rb[k] = which ? r1[k] : r0[k]; }
#pragma unroll
  for (int k = 0; k < 5; k++) { ua[k] = which ? u0[k] : u1[k]; ub[k] = which ? u1[k] : u0[k]; }
  bool good = hit && !bad;
  if (good && (ub[0] & 1u) == 0) {
    if (!halve_fits_b33<8>(ra)) {
      // (ra, ua) -= (floor(D / rb) + 1) (rb, ub) with D = ra - B33 - 1: D by quotients that never exceed the true one, like
      // every step above (a second and a third round take what the first one's margin left: at most 2), ...
      int64_t c = -1;
#pragma unroll
      for (int k = 0; k < 8; k++) { c += (int64_t)ra[k] - (int64_t)halve_B33(k); ra[k] = (uint32_t)c; c >>= 32; }
      ED_CHECK(c == 0);
      const double db = halve_to_double(rb);
      for (int it = 0; it < 4 && good && !halve_less(ra, rb); it++)
        if (halve_reduce(ra, ua, rb, ub, halve_to_double(ra), db, true)) good = false;
      good = good && halve_less(ra, rb);
      // ... then the + 1, and B33 + 1 back: the remainder is D mod rb + B33 + 1 - rb, in [B33 + 2 - rb, B33]
      uint64_t a = 1;
      c = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        a += (uint64_t)ra[k] + halve_B33(k);
        c += (int64_t)(uint32_t)a - (int64_t)rb[k];
        ra[k] = (uint32_t)c;
        a >>= 32;
        c >>= 32;
      }
      c = 0;
#pragma unroll
      for (int k = 0; k < 5; k++) { c += (int64_t)ua[k] - (int64_t)ub[k]; ua[k] = (uint32_t)c; c >>= 32; }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) rb[k] = ra[k];
#pragma unroll
    for (int k = 0; k < 5; k++) ub[k] = ua[k];
  }
  // the bounds are checked on what goes out, whichever way it came
  halve_magnitude<HALF_BITS_BALANCED>(uw, uneg, ub);
  good = good && halve_fits_b33<8>(rb) && halve_fits_b33<5>(uw) && (uw[0] & 1u) != 0;
#pragma unroll
  for (int k = 0; k < 5; k++) vw[k] = rb[k];
  return good;
}

}  // namespace ed
