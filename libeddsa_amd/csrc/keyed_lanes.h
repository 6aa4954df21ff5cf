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

}  // namespace ed
