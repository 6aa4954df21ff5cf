// keyed_lanes.h - what a lane of the key-set kernels (keyed_kernels.h) computes beyond lanes.h: plain words in, words out, so that
// the same source compiles for the host under -DED_HOST_CHECK (tests/host_check/keyed_check.cpp, every limb bound asserted).
//
// A key set (include/eddsa_amd.h: eddsa_amd_keyset) holds, per registered key, the 32 key bytes, one flag byte (the key decodes to
// a curve point) and the nine-entry table 0..8 * (-A) in the layout of a verify item's table slot (kernel_io.h: table_slot).  A
// keyed pass reads the three by key index where an unkeyed pass decompresses the key and builds the table per item.
#pragma once
#include "lanes.h"

namespace ed {

// One key of a key set: the table verify_table_lane builds for these bytes, into the key's slot; returns the on-curve flag.
// Entry 0 is the neutral element whatever the bytes are (verify_table_point_lane), which is what lets a keyed pass read key 0's
// entry 0 for every zero digit.
ED_DEV bool keyset_build_lane(uint32_t* tab, const uint32_t aw[8]) { return verify_table_lane(tab, aw); }

// The key bytes of an item whose index names no key of the set: y = 2, x's sign bit clear.  (y^2 - 1) / (d y^2 + 1) = 3 / (4 d + 1)
// is no square mod p, so the string decodes under no rule - the reference's import keeps the wrong root, the cofactored equation
// and A_CANONICAL reject it (tests/test_keyed_on_host.py proves it with integers).  NOT the all-zero string: that one encodes the
// point (sqrt(-1), 0) of order 4, and under the cofactored equation R = [S]B verifies for it.
ED_DEV void keyed_no_key(uint32_t aw[8]) {
  aw[0] = 2;
#pragma unroll
  for (int k = 1; k < 8; k++) aw[k] = 0;
}

// the nine entries of a key's table into an item's own slot (both 16-byte aligned): what the exact path reads and writes over
ED_DEV void keyed_table_copy(uint32_t* dst, const uint32_t* src) {
#pragma unroll 1
  for (int w = 0; w < VERIFY_ITEM_TABLE_WORDS; w += 4) {
    const uint32_t a = src[w], b = src[w + 1], c = src[w + 2], d = src[w + 3];
    dst[w] = a; dst[w + 1] = b; dst[w + 2] = c; dst[w + 3] = d;
  }
}

// ---------------------------------------------------------------------------------------------
// comb key sets (eddsa_amd_keyset_create_comb): S*B - t*A with fixed-base arithmetic for BOTH scalars
// ---------------------------------------------------------------------------------------------
// On top of the above a comb key set holds, per key, the comb of scale_base_lane built on -A instead of B (edk_layout.h:
// KEYSET_COMB_ENTRIES): entry [row][m - 1] = m * 2^(2 COMB_W row) * (-A), row < COMB_ROWS, m = 1..COMB_HALF, in the packed
// cached form of a verify table entry (one 128-byte line), key-major.  t and S are cut into COMB_DIGITS signed COMB_W-bit digits
// each (scale_base_lane's recoding), the even digits of both add up in one point and the odd digits in another, then COMB_W
// doublings and one addition: 88 additions and 6 doublings where verify_main_lane has 252 doublings and 80 additions.
// Nothing in verification is secret, so - unlike scale_base_lane's lookups - the addresses depend on the digits, as in
// verify_main_lane.  A zero digit of t reads entry 0 of the key's nine-entry table (the neutral element), a zero digit of S
// reads an entry of its row and is replaced in registers.

ED_DEV size_t comb_slot(size_t key) { return key * KEYSET_COMB_WORDS; }   // of a comb key set's comb, in words

// Row `row` of one key's comb, at rowtab = the key's comb + row * COMB_HALF entries.  One lane per (key, row): 2 COMB_W row
// doublings of -A, then m = 1..COMB_HALF by adding the row's first point again and again.  The addition is the unified one
// (ge_add_cached is complete on the curve, and serves P + P): a key of small or mixed order, for which some of the entries
// are the neutral element, needs no case of its own.  A key off the curve gets what ge_frombytes yields, like its nine-entry
// table: idle slots may walk those entries, nothing reads the result.
ED_DEV void keyset_comb_row_lane(uint32_t* rowtab, const uint32_t aw[8], int row) {
  bool oncurve;
  ge a, p;
  ge_frombytes(a, oncurve, aw, true);
#pragma unroll 1
  for (int k = 0; k < 2 * COMB_W * row; k++) ge_dbl(a, a, true);
  ge_cached c1, c;
  ge_to_cached(c1, a);
  cached_store(rowtab, 0, c1);
  p = a;
#pragma unroll 1
  for (int m = 2; m <= COMB_HALF; m++) {
    ge_add_cached(p, p, c1, true);
    ge_to_cached(c, p);
    cached_store(rowtab, m - 1, c);
  }
}

// word k of sum_j COMB_HALF * 2^(COMB_W j), j < COMB_DIGITS: the comb's offset (scale_base_lane)
ED_DEV constexpr uint32_t comb_offset_word(int k) {
  uint32_t pat = 0;
  for (int j = 0; j < COMB_DIGITS; j++) {
    const int bit = COMB_W * j + COMB_W - 1;
    if ((bit >> 5) == k) pat |= 1u << (bit & 31);
  }
  return pat;
}
// y = x + the comb's offset, nine words, from the digit words the prepare kernel leaves: dw = x + pat32 * (1, 1, ..., 1) with
// x < 2^253 (verify_digest_lane: t, 0x88888888; verify_s_lane: S mod l, 0x80008000).  The two offsets differ by a constant, which
// is why k_verify_prepare_keyed serves this route unchanged.
ED_DEV void comb_words_of_digits(uint32_t y[9], const uint32_t dw[8], uint32_t pat32) {
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    c += (int64_t)(k < 8 ? dw[k] : 0u) - (int64_t)(k < 8 ? pat32 : 0u) + (int64_t)comb_offset_word(k);
    y[k] = (uint32_t)c;
    c >>= 32;                                    // arithmetic
  }
}
// the two digits of row `row` (even | odd << COMB_W) of y, whose word k is y[k * stride]: the kernel keeps the nine words of a
// lane's y in LDS, [word][lane], rather than in registers it has no room for (the host build: stride 1)
ED_DEV uint32_t comb_row_digits(const uint32_t* y, int stride, int row) {
  const int bit = 2 * COMB_W * row, w = bit >> 5, s = bit & 31;   // row < COMB_ROWS: w <= 7
  const uint64_t v = (uint64_t)y[w * stride] | ((uint64_t)y[(w + 1) * stride] << 32);
  return (uint32_t)(v >> s) & ((1u << (2 * COMB_W)) - 1u);
}
ED_DEV int comb_digit(uint32_t two, int odd) { return (int)((two >> (odd ? COMB_W : 0)) & ((1u << COMB_W) - 1u)) - COMB_HALF; }

// where digit d's entry of a row lies.  A key's comb: |d| - 1 of the row, or `zero` (entry 0 of the key's nine-entry table) for
// d = 0.  The base point's comb (the table in its global layout, niels entries): |d| - 1, and entry 0 of the row for d = 0,
// which comb_niels_of replaces.
ED_DEV const uint32_t* comb_key_entry(const uint32_t* comb, const uint32_t* zero, int row, int d) {
  const int mag = d < 0 ? -d : d;
  return mag == 0 ? zero : comb + VERIFY_ENTRY_WORDS * (COMB_HALF * row + mag - 1);
}
ED_DEV const uint32_t* comb_base_entry(const uint32_t* bcomb, int row, int d) {
  const int mag = d < 0 ? -d : d;
  return bcomb + TABLE_ENTRY_WORDS * (COMB_HALF * row + (mag == 0 ? 0 : mag - 1));
}
ED_DEV void comb_cached_of(ge_cached& c, const cached_raw& r, int d) {
  cached_from_raw(c, r);
  ge_cached_cneg(c, d < 0);
}
ED_DEV void comb_niels_of(ge_niels& e, const cached_raw& r, int d) {
  const uint32_t w[32] = {r.q[0].x, r.q[0].y, r.q[0].z, r.q[0].w, r.q[1].x, r.q[1].y, r.q[1].z, r.q[1].w,
                          r.q[2].x, r.q[2].y, r.q[2].z, r.q[2].w, r.q[3].x, r.q[3].y, r.q[3].z, r.q[3].w,
                          r.q[4].x, r.q[4].y, r.q[4].z, r.q[4].w, r.q[5].x, r.q[5].y, r.q[5].z, r.q[5].w,
                          r.q[6].x, r.q[6].y, r.q[6].z, r.q[6].w, r.q[7].x, r.q[7].y, r.q[7].z, r.q[7].w};
  const bool none = d == 0;
#pragma unroll
  for (int j = 0; j < 10; j++) {                 // d = 0: the neutral element (1, 1, 0), as comb_select
    e.ymx.v[j] = none ? (j == 0 ? 1u : 0u) : w[j];
    e.ypx.v[j] = none ? (j == 0 ? 1u : 0u) : w[10 + j];
    e.t2d.v[j] = none ? 0u : w[20 + j];
  }
  ge_niels_cneg(e, d < 0);
}

// yt, ys (word k at [k * stride]) = t and S mod l plus the comb's offset, nine words each, from the item's digit words (t + 0x88..
// | (S mod l) + 0x8000..: what the prepare kernels leave; S is any 256-bit string in the signature and the comb covers 264 bits
// of y, so the REDUCED S is what is cut into digits - B has order l, (S mod l)*B = S*B)
ED_DEV void verify_comb_words_lane(uint32_t* yt, uint32_t* ys, int stride, const uint32_t* digits) {
  uint32_t dw[8], y[9];
#pragma unroll
  for (int k = 0; k < 8; k++) dw[k] = digits[k];
  comb_words_of_digits(y, dw, 0x88888888u);
#pragma unroll
  for (int k = 0; k < 9; k++) yt[k * stride] = y[k];
#pragma unroll
  for (int k = 0; k < 8; k++) dw[k] = digits[8 + k];
  comb_words_of_digits(y, dw, 0x80008000u);
#pragma unroll
  for (int k = 0; k < 9; k++) ys[k * stride] = y[k];
}

// out = S*B + t*(-A) from those words.  keycomb: the key's comb, zero: entry 0 of its nine-entry table, bcomb: the base point's
// comb in its global layout.  The same point as verify_main_lane's, with X, Y, Z (no T).
// A row's entries are loaded ahead of the additions that use them: while one addition runs, the entry of the next one is in
// flight, the first of the next row included (the last row loads its own again, in bounds, and drops it).
ED_DEV void verify_comb_lane(ge& out, const uint32_t* yt, const uint32_t* ys, int stride, const uint32_t* keycomb, const uint32_t* zero,
                             const uint32_t* bcomb) {
  ge r0, r1;
  cached_raw ra, rb;
  uint32_t two_s = comb_row_digits(ys, stride, 0);
  cached_load_raw(ra, comb_base_entry(bcomb, 0, comb_digit(two_s, 0)), 0);
  cached_load_raw(rb, comb_base_entry(bcomb, 0, comb_digit(two_s, 1)), 0);
#pragma unroll 1
  for (int row = 0; row < COMB_ROWS; row++) {
    const int next = row + 1 < COMB_ROWS ? row + 1 : row;
    const uint32_t two_t = comb_row_digits(yt, stride, row);
    {
      ge_niels e;
      comb_niels_of(e, ra, comb_digit(two_s, 0));
      cached_load_raw(ra, comb_key_entry(keycomb, zero, row, comb_digit(two_t, 0)), 0);
      if (row == 0) ge_from_niels(r0, e); else ge_add_niels(r0, r0, e, true);   // (the first entry IS the sum so far, as in scale_base_lane)
    }
    {
      ge_niels e;
      comb_niels_of(e, rb, comb_digit(two_s, 1));
      cached_load_raw(rb, comb_key_entry(keycomb, zero, row, comb_digit(two_t, 1)), 0);
      if (row == 0) ge_from_niels(r1, e); else ge_add_niels(r1, r1, e, true);
    }
    two_s = comb_row_digits(ys, stride, next);
    {
      ge_cached c;
      comb_cached_of(c, ra, comb_digit(two_t, 0));
      cached_load_raw(ra, comb_base_entry(bcomb, next, comb_digit(two_s, 0)), 0);
      ge_add_cached(r0, r0, c, true);
    }
    {
      ge_cached c;
      comb_cached_of(c, rb, comb_digit(two_t, 1));
      cached_load_raw(rb, comb_base_entry(bcomb, next, comb_digit(two_s, 1)), 0);
      ge_add_cached(r1, r1, c, true);
    }
  }
#pragma unroll 1
  for (int k = 0; k < COMB_W; k++) ge_dbl(r1, r1, k == COMB_W - 1);
  ge_cached c;
  ge_to_cached(c, r1);
  ge_add_cached(out, r0, c, false);
}

}  // namespace ed
