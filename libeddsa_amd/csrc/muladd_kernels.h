// muladd_kernels.h - the kernels of [m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch*), part of kernels.hip's translation
// unit (it uses that file's BLOCK, finish_batch8, finish_at and den_commit) and included by nothing else.
//
//   k_point_muladd_prepare   one lane per item: decode P, m mod 8 l centred, a mod l -> digit words, table of 0..8 times +-P, flag
//   k_verify_main            the chain, unchanged: 252 doublings, 64 additions from the item's table, 16 from base16
//   k_point_muladd_finish    invert Z (shared by FINISH_K items per lane), encode, or write the no-point string
// The pass lives in the verify workspace (digits, table, acc, flags) and reads nothing else of it: no work lists, no side stream.
#pragma once
#include "muladd_lanes.h"

namespace ed {

// mul == nullptr: every m = 1; add == nullptr: every a = 0 - nothing is read from an absent array.  Idle lanes of the last block
// redo the last item into a slot past the pass, as in k_verify_prepare: k_verify_main walks every slot of every tile, and a slot
// that held another pass's words could hold digits and a table of anything.
// Two blocks per CU, from the code object's metadata (tools/kernel_metadata.py, profiles/point_muladd.txt): 247 VGPRs without scratch,
// of which the table wants 245 (k_keyset_build, which builds nothing else); the lane stores its digit words before it decodes the
// point, because held across the table they made it 256 registers and 21 spilled ones.  Two waves per SIMD is what k_verify_prepare
// runs at; the kernel is a tenth of the pass.
__global__ void __launch_bounds__(BLOCK, 2)
k_point_muladd_prepare(const uint8_t* points, const uint8_t* mul, const uint8_t* add, size_t n, uint32_t* digits, uint32_t* table, uint8_t* flags) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const size_t item = g < n ? g : n - 1;
  uint32_t pw[8], mw[8], aw[8];
  load32(pw, points, item, 32);
#pragma unroll
  for (int q = 0; q < 8; q++) { mw[q] = q == 0 ? 1u : 0u; aw[q] = 0u; }
  if (mul) load32(mw, mul, item, 32);
  if (add) load32(aw, add, item, 32);
  flags[g] = point_muladd_prepare_lane(digits + digit_slot(g), table + table_slot(g), pw, mw, aw);
}

// the shared inversion with a substituted denominator: Z for the items on the curve, 1 for the others and for slots past the pass
struct muladd_finish_policy {
  uint8_t* out; uint32_t* acc; const uint8_t* flags; size_t n; int K;
  ED_DEV void den(int k, fe& z) const {
    const finish_pos p = finish_at(k, acc, K);
    fe_set(z, 1);
    const bool good = p.i < n && (flags[p.i] & MULADD_ON_CURVE) != 0;
    if (good) acc_load(z, p.acc, ACC_Z);         // never 0: the chain walked curve points, and the a = -1 law is complete on them
    den_commit(z, good, acc, k, K);
  }
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    if (p.i >= n) return;
    uint32_t w[8];
    if ((flags[p.i] & MULADD_ON_CURVE) != 0) {
      fe x, y, zinv;
      acc_load(x, p.acc, ACC_X); acc_load(y, p.acc, ACC_Y); acc_load(zinv, p.acc, ACC_Z);
      encode_lane(w, x, y, zinv);
    } else {
      point_muladd_no_point(w);
    }
    store32(out, p.i, 32, w);
  }
};

// (134 VGPRs, no scratch: the bound of k_encode_finish, whose body it shares)
__global__ void __launch_bounds__(BLOCK, 2)
k_point_muladd_finish(uint8_t* out, uint32_t* acc, const uint8_t* flags, size_t n, int K) {
  finish_batch8(muladd_finish_policy{out, acc, flags, n, K}, acc);
}

}  // namespace ed
