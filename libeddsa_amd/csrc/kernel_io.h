// kernel_io.h - how the kernels move packed byte arrays and shared tables, and how they address the HBM workspaces they hand
// to one another (sizes: edk_layout.h): used by kernels.hip and rlc.hip (the product) and by probe.hip (the layer probes, a
// separate library).
#pragma once
#include "lanes.h"

namespace ed {

// ---- packed byte-array access: 32 bytes per item as eight little-endian words ---------------

// eight words at a 16-byte aligned word pointer <-> registers: two 16-byte accesses
ED_DEV void load8(uint32_t w[8], const uint32_t* p) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0];
  const uint4 b = reinterpret_cast<const uint4*>(p)[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
ED_DEV void store8(uint32_t* p, const uint32_t w[8]) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

ED_DEV void load32(uint32_t w[8], const uint8_t* base, size_t item, size_t stride) {
  const uint8_t* p = base + item * stride;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    load8(w, reinterpret_cast<const uint32_t*>(p));
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++)
      w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
             ((uint32_t)p[4 * i + 3] << 24);
  }
}

ED_DEV void store32(uint8_t* base, size_t item, size_t stride, const uint32_t w[8]) {
  uint8_t* p = base + item * stride;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    store8(reinterpret_cast<uint32_t*>(p), w);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      p[4 * i] = (uint8_t)w[i]; p[4 * i + 1] = (uint8_t)(w[i] >> 8);
      p[4 * i + 2] = (uint8_t)(w[i] >> 16); p[4 * i + 3] = (uint8_t)(w[i] >> 24);
    }
  }
}

// copy a table of `words` 32-bit words (a multiple of 4, 16-byte aligned) from HBM into LDS (whole block)
ED_DEV void stage_table(uint32_t* lds, const uint32_t* src, int words) {
  word4* d = reinterpret_cast<word4*>(lds);
  const word4* s = reinterpret_cast<const word4*>(src);
  for (int j = threadIdx.x; j < words / 4; j += (int)blockDim.x) d[j] = s[j];
  __syncthreads();
}

// ---- the verify workspace (eddsa_kernels.h: edk_verify_ws): where item i's slot starts, in words ----
// (offsets, not pointers: the sum stays in the kernel, where table and rtable share the one product)

ED_DEV size_t digit_slot(size_t i) { return VERIFY_DIGIT_WORDS * i; }                // of digits
ED_DEV size_t table_slot(size_t i) { return i * VERIFY_ITEM_TABLE_WORDS; }           // of table and of rtable
ED_DEV size_t hdigit_slot(size_t i) { return HALF_DIGIT_WORDS * i; }                 // of hdigits
ED_DEV void hdigits_store(uint32_t* hdigits, size_t i, const uint32_t hd[HALF_DIGIT_WORDS]) {
  uint4* o = reinterpret_cast<uint4*>(hdigits + hdigit_slot(i));
#pragma unroll
  for (int q = 0; q < HALF_DIGIT_WORDS / 4; q++) o[q] = make_uint4(hd[4 * q], hd[4 * q + 1], hd[4 * q + 2], hd[4 * q + 3]);
}

// flags[i].  VERIFY_WINDOWED: the windowed evaluation owns the item's verdict (its key is a curve point, and on the half-length
// route it has a short pair); clear: the exact path does.  The other two bits exist on ONE route each: VERIFY_Z_USABLE is set and
// read by the full-length finish (verify_finish_policy) alone, VERIFY_R_CANONICAL - R is the canonical encoding of a curve point -
// by the half-length route alone (k_verify_halve, k_verify_prepare_pair; half_verdict_store).
enum : uint8_t { VERIFY_WINDOWED = 1, VERIFY_Z_USABLE = 2, VERIFY_R_CANONICAL = 4 };

// the verdict of a half-length evaluation: the exact path owns it (reject mode - exact_offcurve == 0 - has no exact path: 0), or
// the combination is the neutral element and R canonical
ED_DEV void half_verdict_store(uint8_t* ok, size_t i, uint8_t fl, bool neutral, int exact_offcurve) {
  if ((fl & VERIFY_WINDOWED) == 0) {
    if (!exact_offcurve) ok[i] = 0;
    return;
  }
  ok[i] = (uint8_t)(neutral && (fl & VERIFY_R_CANONICAL) != 0);
}

// ---- the point workspace acc[tile][word ACC_WORDS][lane VERIFY_TILE]: lane-interleaved, so that a block's accesses coalesce ----
// An item's column starts at its lane's word of the tile; limb j of coordinate c is word acc_at(c, j) of the column.

enum acc_coord { ACC_X = 0, ACC_Y = 1, ACC_Z = 2, ACC_W = 3 };   // W: the finish kernels' prefix products
static_assert(10 * (ACC_W + 1) == ACC_WORDS, "four coordinates of ten limbs");
template <class W> ED_DEV W* acc_column(W* acc, size_t tile, size_t lane) { return acc + tile * (ACC_WORDS * VERIFY_TILE) + lane; }
ED_DEV constexpr int acc_at(int coord, int j) { return (10 * coord + j) * VERIFY_TILE; }
ED_DEV void acc_load(fe& f, const uint32_t* col, int coord) {
#pragma unroll
  for (int j = 0; j < 10; j++) f.v[j] = col[acc_at(coord, j)];
}
ED_DEV void acc_put(uint32_t* col, int coord, const fe& f) {
#pragma unroll
  for (int j = 0; j < 10; j++) col[acc_at(coord, j)] = f.v[j];
}
ED_DEV void acc_put_xyz(uint32_t* col, const ge& p) {
#pragma unroll
  for (int j = 0; j < 10; j++) {
    col[acc_at(ACC_X, j)] = p.X.v[j]; col[acc_at(ACC_Y, j)] = p.Y.v[j]; col[acc_at(ACC_Z, j)] = p.Z.v[j];
  }
}

}  // namespace ed
