// keyed_rlc_check.cpp - TEST BINARY: the lane steps of batch verification over a key set (libeddsa_amd/csrc/rlc_keyed_lanes.h,
// what the kernels of rlc_keyed.h call), compiled for the host CPU with -DED_HOST_CHECK (every bound asserted): the per-key
// scalar from an accumulator's word sums, the item's term, and the whole combination of one small group evaluated the keyed
// way - one point and one scalar per KEY - by plain double-and-add instead of the workgroup's buckets.  Built by
// tests/test_keyed_rlc_on_host.py; not part of the product.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rlc_keyed_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

extern "C" {

long krc_violations(void) { return g_violations.load(); }

// k_rlc_key_scalars for one (group, key): the 32 digits from the accumulator's eight word sums
void krc_key_sum(int8_t dig[32], const uint64_t acc[8]) { rlc_key_sum_lane(dig, acc); }

// k_rlc_scalars_keyed for one item: term = z t mod 8 l (32 bytes), the digits of z, zs = z S mod l
void krc_term(uint8_t term[32], int8_t dig_r[16], uint8_t zs[32], const uint8_t seed[32], uint64_t i, const uint8_t t[32],
              const uint8_t s[32]) {
  uint32_t sd[8], tw[8], sw[8], a[8], z9[9];
  memcpy(sd, seed, 32); memcpy(tw, t, 32); memcpy(sw, s, 32);       // little-endian host
  rlc_keyed_scalars_lane(a, dig_r, z9, sd, i, tw, sw);
  memcpy(term, a, 32);
  memcpy(zs, z9, 32);
}

// The keyed pass of rlc.hip for ONE group of n <= 64 items under `count` <= 64 keys, fixed-length messages, every step from the
// lanes headers: keys decoded once (k_rlc_keys), leaves -> seed with the key bytes taken by index (k_rlc_hash_keyed), -R and the
// flags (k_rlc_points_keyed), the terms added into per-key accumulators word by word (k_rlc_scalars_keyed), one scalar per key
// (k_rlc_key_scalars), then
//   sum_w 256^w ( sum_k digA[k][w] (-A_k) + sum_i digR[i][w] (-R_i) + digB[w] B )
// by Horner with plain additions.  Returns 1 if the total is the neutral element and no item is flagged for the per-item path,
// 0 otherwise; flags_out[i] receives item i's flags (0 for an index outside the key set).
int krc_group(uint8_t* flags_out, const uint8_t* sigs, const uint8_t* keys, int count, const uint32_t* key_idx, const uint8_t* msgs,
              size_t mlen, int n) {
  if (n < 1 || n > 64 || count < 1 || count > 64) return -1;
  std::vector<ge_niels> na(count), nr(n);
  std::vector<uint8_t> kfl(count), fl(n);
  for (int k = 0; k < count; k++) {
    uint32_t aw[8];
    memcpy(aw, keys + 32 * k, 32);
    kfl[k] = rlc_decode_key_lane(na[k], aw);
  }
  std::vector<uint32_t> tw(8 * n), sw(8 * n), leaves(8 * n);
  for (int i = 0; i < n; i++) {
    uint32_t rw[8], aw[8];
    const bool known = key_idx[i] < (uint32_t)count;
    memcpy(rw, sigs + 64 * i, 32); memcpy(&sw[8 * i], sigs + 64 * i + 32, 32);
    if (known) memcpy(aw, keys + 32 * (size_t)key_idx[i], 32); else keyed_no_key(aw);
    rlc_hash_lane(&tw[8 * i], &sw[8 * i], &leaves[8 * i], rw, aw, sigs + 64 * i + 32, msgs + mlen * i, mlen);
    fl[i] = rlc_decode_r_lane(nr[i], rw);
    fl[i] = known ? (uint8_t)(fl[i] | kfl[key_idx[i]]) : (uint8_t)0;
    flags_out[i] = fl[i];
  }
  uint32_t seed[16];
  {
    std::vector<uint32_t> level = leaves;
    size_t cnt = (size_t)n;
    do {
      const size_t next = (cnt + RLC_TREE_FAN - 1) / RLC_TREE_FAN;
      std::vector<uint32_t> up(8 * next);
      for (size_t j = 0; j < next; j++) {
        const size_t lo = j * RLC_TREE_FAN, c = cnt - lo < (size_t)RLC_TREE_FAN ? cnt - lo : (size_t)RLC_TREE_FAN;
        sha512_prefix_msg<0>(seed, nullptr, reinterpret_cast<const uint8_t*>(level.data() + 8 * lo), 32 * c);
        for (int k = 0; k < 8; k++) up[8 * j + k] = seed[k];
      }
      level = up;
      cnt = next;
    } while (cnt > 1);
    for (int k = 0; k < 8; k++) seed[k] = level[k];
  }
  std::vector<uint64_t> acc((size_t)RLC_KEY_ACC_WORDS * count, 0);
  std::vector<int8_t> da(32 * count), dr(16 * n, 0);
  uint32_t sum[16] = {0};
  bool flagged = false;
  for (int i = 0; i < n; i++) {
    flagged = flagged || (fl[i] & RLC_PER_ITEM);
    if (!(fl[i] & RLC_R_VALID)) continue;
    uint32_t zs[9], term[8];
    rlc_keyed_scalars_lane(term, &dr[16 * i], zs, seed, (uint64_t)i, &tw[8 * i], &sw[8 * i]);
    for (int q = 0; q < 8; q++) acc[(size_t)RLC_KEY_ACC_WORDS * key_idx[i] + q] += term[q];
    uint64_t c = 0;
    for (int k = 0; k < 10; k++) { c += (uint64_t)sum[k] + (k < 9 ? zs[k] : 0u); sum[k] = (uint32_t)c; c >>= 32; }
  }
  for (int k = 0; k < count; k++) rlc_key_sum_lane(&da[32 * k], &acc[(size_t)RLC_KEY_ACC_WORDS * k]);
  int8_t db[32];
  rlc_group_scalar_lane(db, sum);
  alignas(128) uint32_t bentry[TABLE_ENTRY_WORDS];
  table_entry_lane(bentry, 1u, 0);                           // 1 * B, as entry 1 of base16
  ge_niels nb;
  niels_load(nb, bentry);
  ge total;
  ge_neutral(total);
  auto add_digit = [&](const ge_niels& pt, int d) {          // total += d * pt, |d| <= 128
    if (d == 0) return;
    ge_niels q = pt;
    ge_niels_cneg(q, d < 0);
    ge m;
    ge_neutral(m);
    const int mag = d < 0 ? -d : d;
    for (int bit = 7; bit >= 0; bit--) {
      ge_dbl(m, m, true);
      if ((mag >> bit) & 1) ge_add_niels(m, m, q, true);
    }
    ge_cached c;
    ge_to_cached(c, m);
    ge_add_cached(total, total, c, true);
  };
  for (int w = 31; w >= 0; w--) {
    for (int k = 0; k < 8; k++) ge_dbl(total, total, true);
    for (int k = 0; k < count; k++) add_digit(na[k], da[32 * k + w]);
    if (w < 16)
      for (int i = 0; i < n; i++) add_digit(nr[i], dr[16 * i + w]);
    add_digit(nb, db[w]);
  }
  return (ge_is_neutral(total) && !flagged) ? 1 : 0;
}

}  // extern "C"
