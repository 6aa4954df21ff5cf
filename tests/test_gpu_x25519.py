"""X25519 on low-order and non-canonical points, in both ladders and every shape of the finish kernel.

A point of order dividing 8 gives z2 = 0, the one zero denominator a caller can put into the inversion that K = 1, 2, 4
or 8 items of a lane share (csrc/kernels.hip: finish_batch8, x25519_finish_policy): the item must come out as 32 zero
bytes (fld_inv(0) = 0 in the reference) and every neighbour in its lane group as its true quotient.  tools/x25519_cases.py
places such points - in all twelve spellings, canonical, + p, and with bit 255 set - by the slot they take in the finish
(every subset of a lane group's slots, beside slots past the end, in the partly filled last tile) and supplies the expected
bytes from a plain integer model, which tests/test_x25519_cases.py ties to the reference's table and to the oracle.  The
sizes are those at which csrc/kernels.hip pins K and the ladder by static_assert.  Bit-exact throughout."""
import functools

import numpy as np
import pytest

import x25519_cases as xc
from x25519_cases import DEGENERATE, DEGENERATE_MODEL, ORDINARY, ORDINARY_MODEL, P
from gpu_kit import dev

pytestmark = pytest.mark.gpu

POOL = DEGENERATE + ORDINARY
POOL_MODEL = DEGENERATE_MODEL + ORDINARY_MODEL


@functools.lru_cache(maxsize=None)
def placed(n, K):
    """place(n, K), or place_all_degenerate(n) for K = 0: computed once, read-only"""
    arrays = xc.place(n, K) if K else xc.place_all_degenerate(n)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def check(got, n, K, what):
    want = placed(n, K)[2]
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    # (i, tile, lane, block, slot, degenerate?) of the first wrong items
    assert bad.size == 0, (what, n, K, f"{bad.size} wrong", xc.describe(bad, max(K, 1), n))


def on_device(engine, n, K):
    import torch
    sc, pt, _ = placed(n, K)
    out = engine.x25519_batch(dev(sc), dev(pt))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- a. the ladders as a layer

# the two pools interleaved (a stride of 7 through the 72 entries: the short runs hold both kinds) and repeated with a period
# of 73, coprime to the 16 quads of a wave: 16 * 73 items put every entry into every quad position of a wave once
LADDER_ORDER = [7 * (j % 73 % 72) % 72 for j in range(16 * 73)]
LADDER_ITEMS = [POOL[e] for e in LADDER_ORDER]
LADDER_MODEL = [POOL_MODEL[e] for e in LADDER_ORDER]
assert all({e for e in LADDER_ORDER[q::16]} == set(range(72)) for q in range(16))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 64 * 3 + 5, 16 * 73])
def test_both_ladders_leave_the_models_x2_z2(engine, n):
    """(x2 : z2) before the inversion, from lanes.h x25519_ladder_lane (form 0, k_x25519_ladder's) and quad_lanes.h
    x25519_ladder_quad (form 1, k_x25519_ladder_quad's: DPP exchanges, whole and ragged waves): the same bytes from both,
    the model's point projectively - and the model's x2 and z2 as VALUES: both forms evaluate RFC 7748's field
    expressions from bit 254 down, so exact equality holds and is asserted"""
    items = [s + p for s, p in LADDER_ITEMS[:n]]
    lane = engine.debug_layer("x25519_ladder", items, 64, form=0)
    quad = engine.debug_layer("x25519_ladder", items, 64, form=1)
    assert len(lane) == len(quad) == n
    for j, (a, b, (x2, z2, _)) in enumerate(zip(lane, quad, LADDER_MODEL)):
        assert a == b, (n, j, a.hex(), b.hex())
        gx, gz = int.from_bytes(a[:32], "little"), int.from_bytes(a[32:], "little")
        assert gx < P and gz < P, (n, j)                             # canonical
        assert (gz == 0) == (z2 == 0) and (gx * z2 - x2 * gz) % P == 0, (n, j)
        assert (gx, gz) == (x2, z2), (n, j)                          # (u = 0 leaves (0 : 0), the other low-order points (x : 0))
    if n >= 72:
        assert sum(1 for _, z2, _ in LADDER_MODEL[:n] if z2 == 0) >= 12


def test_the_ladder_probe_checks_its_widths_and_forms(engine):
    item = POOL[0][0] + POOL[0][1]
    for bad in (lambda: engine.debug_layer("x25519_ladder", [item], 32),
                lambda: engine.debug_layer("x25519_ladder", [item[:32]], 64),
                lambda: engine.debug_layer("x25519_ladder", [item], 64, form=2)):
        with pytest.raises(engine.EddsaAmdError):
            bad()


# ---------------------------------------------------------------- b. the four-lane ladder through the product, K = 1

@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 4099, 16384])
def test_four_lane_ladder_and_finish(engine, n):
    check(on_device(engine, n, 1), n, 1, "device pointers")
    if n == 4099:
        sc, pt, _ = placed(n, 1)
        check(engine.x25519_batch(sc, pt), n, 1, "host pointers")


# ---------------------------------------------------------------- c. the one-lane ladder and every K

@pytest.mark.parametrize("n,K", [(17229, 1), (66125, 2), (131405, 4), (262733, 8)])
def test_one_lane_ladder_and_every_finish_shape(engine, n, K):
    """every subset of a lane group's K slots degenerate somewhere in the pass, the last block with slots past the end"""
    check(on_device(engine, n, K), n, K, "device pointers")


@pytest.mark.parametrize("n,K", [(66125, 2), (262733, 8)])
def test_the_same_placements_through_the_host_pipeline(engine, n, K):
    """host pointers: with the pipeline's default chunks (csrc/host_pipe.c: PIPE_FIRST_CHUNK) 66125 items travel as one
    chunk of the K = 2 shape, 262733 as two, of 2^17 and 131661 items: passes with K = 2 and K = 4, a chunk boundary
    inside the placement and lane groups other than those place() was laid out for"""
    sc, pt, _ = placed(n, K)
    check(engine.x25519_batch(sc, pt), n, K, "host pointers")


@pytest.mark.parametrize("n", [66125, 262733])
def test_every_item_degenerate(engine, n):
    """every denominator replaced: the shared product is 1 in every lane group, every output 32 zero bytes"""
    got = on_device(engine, n, 0)
    check(got, n, 0, "device pointers")
    assert not got.any()


# ---------------------------------------------------------------- e. nothing of it outlives the call

def test_the_degenerate_branch_leaves_nothing_in_the_workspace(engine):
    """the branch for z2 = 0 writes X a second time and commits a 1 into Z; the wipe at the end of the finish covers
    both (lib/x25519.c:221 burnstack): the point workspace is zero after the pass, as after one of random points"""
    try:
        for n, K in ((66125, 2), (4099, 0)):
            engine.shutdown()
            check(on_device(engine, n, K), n, K, "device pointers")
            assert engine.secret_residue() == (0, 0, 0, 0), (n, K)
    finally:
        engine.init(0)
