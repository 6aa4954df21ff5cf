"""The X25519 model and case pools of tools/x25519_cases.py, without a GPU: the model against the reference's table and
the oracle, the device source on the host (lanes.h: x25519_lane, x25519_ladder_lane) against the model on both pools, and
the coverage that place() promises at every size tests/test_gpu_x25519.py runs - which lane groups of the finish kernel's
shared inversion hold a zero denominator, in which slots, and beside what."""
import numpy as np
import pytest

import x25519_cases as xc
from x25519_cases import BLOCK, DEGENERATE, DEGENERATE_MODEL, ORDINARY, ORDINARY_MODEL, P, le

# (n, K) of every pass of tests/test_gpu_x25519.py: K = the items per lane that share one inversion at that size
# (csrc/kernels.hip: finish_shape_of, pinned there by static_asserts)
QUAD_SIZES = (1, 15, 16, 17, 63, 64, 65, 4099, 16384)
LANE_SHAPES = ((17229, 1), (66125, 2), (131405, 4), (262733, 8))
SHAPES = tuple((n, 1) for n in QUAD_SIZES) + LANE_SHAPES
EXTRA_SCALARS = (le(0), xc.ONES, le(2**254), le(8), le(2**255 - 8), bytes(range(32)))


def call(h, name, out_len, *args):
    import ctypes
    out = ctypes.create_string_buffer(out_len)
    getattr(h, name)(out, *args)
    return out.raw


def test_the_model_gives_the_references_table(golden):
    raw = golden("x25519_table.bin")
    assert len(raw) == 1024 * 96
    for i in range(1024):
        pt, sc, res = raw[96 * i:96 * i + 32], raw[96 * i + 32:96 * i + 64], raw[96 * i + 64:96 * i + 96]
        assert xc.model(sc, pt)[2] == res, i


def test_the_model_gives_the_oracles_bytes_on_both_pools(oracle):
    for (s, p), (_, _, out) in zip(DEGENERATE + ORDINARY, DEGENERATE_MODEL + ORDINARY_MODEL):
        assert oracle.x25519(s, p) == out, (s.hex(), p.hex())
    for s in EXTRA_SCALARS:                                          # every point of both pools under further scalars
        for _, p in DEGENERATE:
            assert oracle.x25519(s, p) == bytes(32) == xc.model(s, p)[2], (s.hex(), p.hex())
        for _, p in ORDINARY[:15]:                                   # (the pool holds 15 points, four scalars each)
            assert oracle.x25519(s, p) == xc.model(s, p)[2], (s.hex(), p.hex())
    assert len({p for _, p in ORDINARY}) == 15 == len({p for _, p in ORDINARY[:15]})


def test_the_pools_hold_what_they_promise():
    spell = {p for _, p in DEGENERATE}
    assert len(spell) == 12
    assert sum(1 for p in spell if p[31] >> 7) == 5 and sum(1 for p in spell if int.from_bytes(p, "little") in (P, P + 1)) == 2
    assert sum(1 for p in spell if int.from_bytes(p, "little") < P) == 5
    pts = [p for _, p in ORDINARY[:15]]
    assert sum(1 for p in pts[7:] if xc.on_curve(xc.fold(p))) == 4 and len(pts[7:]) == 8           # random: curve and twist
    assert {xc.fold(p) for p in pts[:5]} == {2, 9, P - 2, 18, 37}                                   # 2^255 - 1 = p + 18, 2^256 - 1 -> 18 + 19
    for pool in (DEGENERATE, ORDINARY):
        scalars = {s for s, _ in pool}
        assert {le(0), xc.ONES, le(2**254), le(8)} <= scalars and len(scalars) > 4


def test_the_device_source_on_the_host_gives_the_model_on_both_pools(hostcheck):
    """x25519_lane (ladder, fe_inv(0) = 0, finish) and the ladder alone: (x2, z2) equal the model's as VALUES, not only
    as a ratio - the one-lane ladder evaluates the same field expressions as RFC 7748 from bit 254 down"""
    hostcheck.hc_reset()
    for (s, p), (x2, z2, out) in zip(DEGENERATE + ORDINARY, DEGENERATE_MODEL + ORDINARY_MODEL):
        assert call(hostcheck, "hc_x25519", 32, s, p) == out, (s.hex(), p.hex())
        assert call(hostcheck, "hc_x25519_ladder", 64, s, p) == le(x2) + le(z2), (s.hex(), p.hex())
    assert hostcheck.hc_violations() == 0, hostcheck.hc_first_violation()


@pytest.mark.parametrize("n,K", SHAPES)
def test_place_assigns_the_pools_as_documented(n, K):
    sc, pt, want = xc.place(n, K)
    assert sc.shape == pt.shape == want.shape == (n, 32) and sc.dtype == pt.dtype == want.dtype == np.uint8
    deg = xc.degenerate_mask(n, K)
    ends = sorted(set(range(min(n, 600))) | set(range(max(n - 600, 0), n)))
    for j in ends:                                                   # the rule, restated on plain integers
        tile, lane = j // BLOCK, j % BLOCK
        block, slot = tile // K, tile % K
        assert xc.layout(j, K) == (tile, lane, block, slot)
        assert bool(deg[j]) == bool(((lane + block) % 2**K) >> slot & 1), j
    assert np.array_equal(want.any(axis=1), ~deg)                    # 32 zero bytes exactly at the degenerate items
    pool = {(s, p): m[2] for (s, p), m in zip(DEGENERATE + ORDINARY, DEGENERATE_MODEL + ORDINARY_MODEL)}
    for j in ends:
        key = (sc[j].tobytes(), pt[j].tobytes())
        assert pool[key] == want[j].tobytes() and (key in DEGENERATE) == bool(deg[j]), j


@pytest.mark.parametrize("n,K", SHAPES)
def test_place_covers_every_subset_every_slot_and_the_ragged_end(n, K):
    sc, pt, _ = xc.place(n, K)
    deg = xc.degenerate_mask(n, K)
    tiles = (n + BLOCK - 1) // BLOCK
    blocks = (tiles + K - 1) // K
    # (block, slot, lane) view of the pass, padded to whole blocks: 1 degenerate, 0 ordinary, -1 past the end
    grid = np.full(blocks * K * BLOCK, -1, np.int8)
    grid[:n] = deg
    grid = grid.reshape(blocks, K, BLOCK)
    groups = grid.transpose(0, 2, 1).reshape(-1, K)                  # one row per lane group: its K slots
    whole = groups[(groups >= 0).all(axis=1)]
    masks = (whole.astype(np.int64) << np.arange(K)).sum(axis=1)
    if n > 1:                                                        # (a pass of one item holds one ordinary item)
        assert set(masks.tolist()) == set(range(2**K))               # every subset of degenerate slots, in a group wholly in range
    assert n % BLOCK != 0 or n == 16384                              # the last tile is partly filled (2^14: the largest four-lane pass, whole tiles)
    if K > 1:
        last = grid[blocks - 1]                                      # (K, BLOCK)
        in_range, past = (last >= 0).any(axis=1), (last < 0).all(axis=1)
        assert in_range.any() and past.any()                         # the last block: tiles in range and tiles past the end
        beside = (last == 1).any(axis=0) & (last == -1).any(axis=0)  # a lane with a degenerate slot beside a slot past the end
        assert beside.any()
        assert (last[(tiles - 1) % K, :n % BLOCK] == 1).any()        # ... the partly filled tile has degenerate lanes of its own
    if n < 4099:
        return
    # every spelling and every ordinary entry in every slot: the entry by its rule, checked against the bytes on a sample
    i = np.arange(n)
    entry = np.where(deg, (5 * i) % 12, 12 + (7 * i) % 60)
    pool = {(s, p): j for j, (s, p) in enumerate(DEGENERATE + ORDINARY)}
    for j in range(0, n, 331):
        assert pool[(sc[j].tobytes(), pt[j].tobytes())] == entry[j], j
    slot = xc.layout(i, K)[3]
    for k in range(K):
        assert set(entry[slot == k].tolist()) == set(range(72)), k


def test_place_all_degenerate():
    pairs = set(DEGENERATE)
    for n in (4099, 66125, 262733):
        sc, pt, want = xc.place_all_degenerate(n)
        assert sc.shape == pt.shape == want.shape == (n, 32) and not want.any()
        assert {p.tobytes() for p in pt[:24]} == {p for _, p in DEGENERATE}
        assert all((sc[j].tobytes(), pt[j].tobytes()) in pairs for j in range(0, n, 499))
