/* edk_layout.h - the numbers the host library, the launchers and the kernels share: the sizes of the generated tables and the
 * format of the HBM workspaces the kernels hand to one another.  Plain C: eddsa_amd.c allocates by these names, lanes.h and
 * kernel_io.h address by them, tests/fake_hip checks pointers against them.  Every constant is defined here and nowhere else.
 * The names of the BITS kept in the workspaces are next to the code that writes them: kernel_io.h (flags), lanes.h (the status
 * word of the half-length digits), rlc_lanes.h (the combination's flags). */
#pragma once

#ifdef __cplusplus
#define EDK_LAYOUT_ASSERT(cond, what) static_assert(cond, what)
#else
#define EDK_LAYOUT_ASSERT(cond, what) _Static_assert(cond, what)
#endif

/* ---- generated tables (kernels.hip: k_init_tables, k_init_comb_image) ---- */
#define TABLE_BASE16_ENTRIES 32769 /* k*B, k = 0..32768: 16-bit signed windows of S (4 MiB, L2/MALL); the table holds twice that: k*2^128*B follows */
#define COMB_W 6                  /* signed window width of the fixed-base comb (the reference's is 4, ed.c:397-430) */
#define COMB_HALF (1 << (COMB_W - 1))          /* digits d in [-COMB_HALF, COMB_HALF - 1] */
#define COMB_DIGITS (COMB_W == 4 ? 64 : COMB_W == 5 ? 52 : 44)   /* digits of x + offset: 64 x 4, 52 x 5 or 44 x 6 bits */
#define COMB_ROWS (COMB_DIGITS / 2)            /* even digits and odd digits share a row */
#define TABLE_COMB_ENTRIES (COMB_ROWS * COMB_HALF) /* comb[i][k] = (k+1) * 2^(2*COMB_W*i) * B, k < COMB_HALF */
#define TABLE_ENTRY_WORDS 32      /* 3 x 10 limbs + 2 padding words */
#define COMB_IMG_ENTRIES COMB_HALF       /* LDS image of a comb row: entry m - 1 = m * 2^(2*COMB_W*i) * B, m = 1..COMB_HALF */
#define COMB_IMG_ENTRY_WORDS 36   /* 30 limbs + 6 padding words: entries start 4 banks apart */
#define COMB_IMG_WORDS (COMB_ROWS * COMB_IMG_ENTRIES * COMB_IMG_ENTRY_WORDS)

/* ---- per-item slots of the verify workspace (edk_verify_ws; accessors: kernel_io.h) ---- */
#define VERIFY_TILE 256            /* items per tile = threads per block */
#define VERIFY_DIGIT_WORDS 16      /* digits [item]: t + 0x88.. | S + 0x80.., eight little-endian words each */
#define VERIFY_TABLE_ENTRIES 9     /* table, rtable [item][entry]: 0..8 times -A (-R'), cached form */
#define VERIFY_ENTRY_WORDS 32      /* ymx | ypx | t2d | z2, 255 bits packed into eight words each: one 128-byte line */
#define VERIFY_ITEM_TABLE_WORDS (VERIFY_TABLE_ENTRIES * VERIFY_ENTRY_WORDS)   /* 1152 contiguous bytes per item */
#define VERIFY_TABLE_WORDS_PER_TILE (VERIFY_TABLE_ENTRIES * VERIFY_ENTRY_WORDS * 256)
#define HALF_DIGIT_WORDS 28        /* hdigits [item]: the half-length scalars and their status word (lanes.h: verify_half_scalars_lane) */
#define KEYSET_COMB_ENTRIES TABLE_COMB_ENTRIES   /* a comb key set (eddsa_amd_keyset_create_comb), comb [key][row][m - 1]: m * 2^(2*COMB_W*row) * (-A_key),
                                                   row < COMB_ROWS, m = 1..COMB_HALF, each the cached form of a verify table entry */
#define KEYSET_COMB_WORDS (KEYSET_COMB_ENTRIES * VERIFY_ENTRY_WORDS)          /* 88 KiB per key */
#define ACC_WORDS 40               /* acc [tile][word][lane VERIFY_TILE], the point workspace: X, Y, Z and one slot (W) for the finish
                                      kernels' prefix products, ten limbs each */

/* ---- edk_verify_ws.offcount: counters and hooks, zeroed at allocation ---- */
#define EDK_OFFCOUNT_WORDS 64
#define EDK_OFFCOUNT_BYTES (EDK_OFFCOUNT_WORDS * 4)
#define EDK_OFFLIST_WORD 0          /* the length of offlist */
#define EDK_ONLIST_WORD 1           /* the length of onlist */
#define EDK_EXACT_UNIT_WORD 2       /* the next unit of work of k_verify_exact_lane_chain */
#define EDK_STALL_WORD 3            /* ... set by a wave of that kernel that gave up waiting for a hand-off: the others then leave too */
#define EDK_PASS_WORDS 4            /* words 0..3 are zeroed by every pass */
#define EDK_REFUSED_WORD 8          /* half-length pairs that the exact check of lanes.h: verify_half_scalars_lane refused since allocation (diagnostic) */
#define EDK_WITHHOLD_WORD 9         /* test hook (eddsa_amd_debug_withhold_handoff): tile + 1 whose first hand-off is never published; 0: none */
#define EDK_COLIST_WORD 10          /* the cofactored equation (kernels.hip: k_cofactor_list): the length of its work list; zeroed on the stream in front of that kernel */
#define EDK_BENTRY_WORD 32          /* words 32..63: the base point as a packed cached entry (lanes.h: exact_bentry_store) */

/* ---- edk_fixed_ws.tiles: [0] the tile counter of the persistent point kernels ---- */
#define EDK_TILES_WORDS 64
#define EDK_TILES_BYTES (EDK_TILES_WORDS * 4)

/* ---- the dom2 prefix of Ed25519ctx / Ed25519ph (RFC 8032 section 2; eddsa_kernels.h: edk_dom) ---- */
#define EDK_DOM_FIXED_BYTES 34     /* "SigEd25519 no Ed25519 collisions" | flag | len(context) */
#define EDK_DOM_CONTEXT_MAX 255
#define EDK_DOM_WORDS 73           /* the prefix as little-endian words, zero-filled behind its last byte */
#define EDK_DOM_DIGEST_BYTES 64    /* edk_verify_ws.domdig [item]: SHA-512(dom2 | R | A | M') */

EDK_LAYOUT_ASSERT(EDK_DOM_WORDS * 4 >= EDK_DOM_FIXED_BYTES + EDK_DOM_CONTEXT_MAX, "the longest prefix fits its words");
EDK_LAYOUT_ASSERT(VERIFY_ITEM_TABLE_WORDS * VERIFY_TILE == VERIFY_TABLE_WORDS_PER_TILE, "a tile of the table is its items' slots");
EDK_LAYOUT_ASSERT(KEYSET_COMB_WORDS * 4 == 704 * 128 && COMB_ROWS * COMB_HALF == 704, "a key's comb is 704 entries of one 128-byte line");
EDK_LAYOUT_ASSERT(TABLE_ENTRY_WORDS == VERIFY_ENTRY_WORDS, "an entry of the base point's comb and one of a key's comb are loaded alike");
EDK_LAYOUT_ASSERT(EDK_BENTRY_WORD + VERIFY_ENTRY_WORDS <= EDK_OFFCOUNT_WORDS, "the base-point entry lies inside offcount");
EDK_LAYOUT_ASSERT(EDK_OFFLIST_WORD < EDK_PASS_WORDS && EDK_ONLIST_WORD < EDK_PASS_WORDS && EDK_EXACT_UNIT_WORD < EDK_PASS_WORDS &&
                  EDK_STALL_WORD < EDK_PASS_WORDS && EDK_PASS_WORDS == 4, "every pass zeroes its four words");
EDK_LAYOUT_ASSERT(EDK_REFUSED_WORD >= EDK_PASS_WORDS && EDK_WITHHOLD_WORD >= EDK_PASS_WORDS && EDK_BENTRY_WORD >= EDK_PASS_WORDS &&
                  EDK_REFUSED_WORD < EDK_BENTRY_WORD && EDK_WITHHOLD_WORD < EDK_BENTRY_WORD, "... and nothing that outlives it");
EDK_LAYOUT_ASSERT(EDK_COLIST_WORD >= EDK_PASS_WORDS && EDK_COLIST_WORD < EDK_BENTRY_WORD && EDK_COLIST_WORD != EDK_REFUSED_WORD &&
                  EDK_COLIST_WORD != EDK_WITHHOLD_WORD, "the cofactored list's length has a word of its own outside the four");
