// rlc_keyed_lanes.h - what ONE lane computes in the kernels of rlc_keyed.h (batch verification over a key set:
// include/eddsa_amd.h, ed25519_verify_keyed_rlc*) beyond rlc_lanes.h, as plain functions over words so that the same source
// compiles for the host under -DED_HOST_CHECK (tests/host_check/keyed_rlc_check.cpp, every limb bound asserted).
//
// The combination of a group is the unkeyed one with the key terms collected per key:
//
//     ( sum_i z_i S_i ) B  +  sum_k ( sum_{i: key_idx[i] = k} z_i t_i  mod 8 l ) (-A_k)  +  sum_i z_i (-R_i)
//
// An item adds a_i = z_i t_i mod 8 l, as its representative in [0, 8 l), to the accumulator of (group, key); the accumulator's
// total is reduced to the centred class mod 8 l ONCE, per key: A_k may carry a component of order dividing 8 (rlc_lanes.h:
// rlc_key_scalar_mod_8l), so the sum has to be exact mod 8 l - a sum of terms taken mod l would not do.
#pragma once
#include "rlc_lanes.h"
#include "keyed_lanes.h"

namespace ed {

constexpr int RLC_KEY_ACC_WORDS = 8;            // 64-bit words of one (group, key) accumulator: word q sums the items' 32-bit words q
constexpr int RLC_KEY_ACC_BITS = 45;            // 8192 items x 32 bits: no word reaches 2^45

// a = z t mod 8 l in [0, 8 l), from a0 = z t mod l: z t = a0 + k l with k mod 8 = 5 (z t - a0) mod 8 (l = 5 mod 8 is its own
// inverse there: rlc_key_scalar_mod_8l, which centres the same k)
ED_DEV void rlc_key_term_mod_8l(uint32_t a[8], const uint32_t a0[8], uint32_t z_lo, uint32_t t_lo) {
  const uint32_t k = (((z_lo * t_lo - a0[0]) & 7u) * 5u) & 7u;
  uint64_t p = 0, c = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    p += (uint64_t)k * l_word(q);
    c += (uint64_t)(uint32_t)p + a0[q];
    a[q] = (uint32_t)c;
    c >>= 32;
    p >>= 32;
  }
  ED_CHECK(c + p == 0);                          // a < 8 l < 2^256
}

// rlc_scalars_lane for an item of a keyed pass: the same coefficient z_i, zs = z S mod l and digits of z; in place of the
// digits of the key's scalar, the term a_i = z t mod 8 l that the item adds to its key's accumulator.  (The derivation of z is
// restated here, not factored out of rlc_scalars_lane: k_rlc_scalars keeps the code object it had, and the host check holds
// the two against the same integers.)
ED_DEV void rlc_keyed_scalars_lane(uint32_t term[8], int8_t dig_r[RLC_WINDOWS_R], uint32_t zs[9],
                                   const uint32_t seed[8], uint64_t i, const uint32_t tw[8], const uint32_t sw[8]) {
  uint32_t pre[16], h[16], zw[8], aw[8];
#pragma unroll
  for (int q = 0; q < 8; q++) pre[q] = seed[q];
  pre[8] = (uint32_t)i; pre[9] = (uint32_t)(i >> 32); pre[10] = 0x00636c72u;
#pragma unroll
  for (int q = 11; q < 16; q++) pre[q] = 0;
  sha512_prefix_msg<16>(h, pre, nullptr, 0);
  zw[0] = h[0] | 1u; zw[1] = h[1]; zw[2] = h[2]; zw[3] = h[3] & 0x3fffffffu;
  zw[4] = zw[5] = zw[6] = zw[7] = 0;
  sc z, t, s, a;
  sc_from_words<8>(z, zw);
  sc_from_words<8>(t, tw);
  sc_from_words<8>(s, sw);
  sc_mul(a, z, t);
  sc_to_words(aw, a);
  sc_mul(s, z, s);
  sc_to_words(zs, s);
  zs[8] = 0;
  uint32_t tr[8];
  sc_to_words(tr, t);
  rlc_key_term_mod_8l(term, aw, zw[0], tr[0]);
  {
    uint64_t c = 0;                              // z < 2^126: no carry out of bit 127
#pragma unroll
    for (int q = 0; q < 4; q++) { c += (uint64_t)zw[q] + 0x80808080u; zw[q] = (uint32_t)c; c >>= 32; }
  }
#pragma unroll
  for (int wd = 0; wd < RLC_WINDOWS_R; wd++) dig_r[wd] = (int8_t)((int)((zw[wd >> 2] >> (8 * (wd & 3))) & 0xffu) - 128);
}

// One key of one group: the accumulator's eight word sums (each below 2^45) carried into one integer below 2^269, reduced to
// c = sum (mod 8 l) with |c| <= 4 l - from sum mod l and the sum's low bits, as rlc_key_scalar_mod_8l takes z t - and recoded
// into signed bytes exactly as rlc_scalars_lane recodes an item's scalar.  An accumulator nobody added to gives 32 zero digits.
ED_DEV void rlc_key_sum_lane(int8_t dig_a[RLC_WINDOWS_A], const uint64_t acc[RLC_KEY_ACC_WORDS]) {
  uint32_t sum[16], a0[8], m[8];
  uint64_t c = 0;
#pragma unroll
  for (int q = 0; q < RLC_KEY_ACC_WORDS; q++) {
    ED_CHECK(acc[q] < ((uint64_t)1 << RLC_KEY_ACC_BITS));
    c += acc[q];
    sum[q] = (uint32_t)c;
    c >>= 32;
  }
  sum[8] = (uint32_t)c;                          // c < 2^14
  ED_CHECK((c >> 32) == 0);
#pragma unroll
  for (int q = 9; q < 16; q++) sum[q] = 0;
  sc s;
  sc_from_words<16>(s, sum);
  sc_to_words(a0, s);
  const bool neg = rlc_key_scalar_mod_8l(m, a0, sum[0], 1u);
  words_add_pattern(m, neg ? 0x7f7f7f7fu : 0x80808080u);      // |c| < 2^255: no carry out of bit 255
#pragma unroll
  for (int wd = 0; wd < RLC_WINDOWS_A; wd++) {
    const int byte = (int)((m[wd >> 2] >> (8 * (wd & 3))) & 0xffu);
    dig_a[wd] = (int8_t)(neg ? 127 - byte : byte - 128);
  }
}

}  // namespace ed
