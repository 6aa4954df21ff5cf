"""Point classification (include/eddsa_amd.h: ed25519_point_classify_batch, EDDSA_AMD_POINT_*) in Python integers: the vectors the
CPU and the GPU tests share and the class each must get, from tests/ed_model.py alone - decode_reference, decode_strict, [8]P and
[l]P by pmul.  Nothing here comes from the engine.  Built once per process (about 11 ms of Python per [l]P)."""
import functools
import json
import os

import numpy as np

import ed_model as em

ON_CURVE, CANONICAL, SMALL_ORDER, PRIME_SUBGROUP = 0x01, 0x02, 0x04, 0x08
REGISTRABLE = ON_CURVE | CANONICAL | PRIME_SUBGROUP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def classify(enc, prime=None):
    """the class of 32 bytes.  prime: what [l]P = 0 is known to be by construction (None: computed)"""
    pt = em.decode_reference(enc)
    if pt is None:
        return 0
    cls = ON_CURVE
    if em.decode_strict(enc) is not None:
        cls |= CANONICAL
    if em.is_neutral(em.pmul(8, em.ext(pt))):
        cls |= SMALL_ORDER
    if em.is_neutral(em.pmul(em.L, em.ext(pt))) if prime is None else prime:
        cls |= PRIME_SUBGROUP
    return cls


def encode_affine(pt):
    return em.le(pt[1] | (pt[0] & 1) << 255)


@functools.lru_cache(maxsize=None)
def vectors():
    """-> (names, strings (n, 32) uint8 read-only, classes (n,) uint8 read-only)"""
    rows = []                                        # (name, 32 bytes, class)

    def put(name, enc, prime=None):
        rows.append((name, bytes(enc), classify(enc, prime)))

    for k, enc in enumerate(em.torsion_encodings()):
        put(f"torsion encoding {k}", enc)
    # k B + T: in the subgroup exactly when T is the neutral element; 16 of them cross-checked by [l]P
    torsion = sorted(em.torsion_points())
    base = em.affine(em.B)
    checked = 0
    kb = (0, 1)
    for k in range(1, 20):
        kb = em.add(kb, base)
        for t, tp in enumerate(torsion):
            enc = encode_affine(em.add(kb, tp))
            by_construction = tp == (0, 1)
            if ((k - 1) * 8 + t) % 9 == 0 and checked < 16:      # (every ninth: each T comes up twice)
                assert em.is_neutral(em.pmul(em.L, em.ext(em.decode_reference(enc)))) == by_construction
                checked += 1
            put(f"{k} B + T{t}", enc, prime=by_construction)
    assert checked == 16
    put("neutral", em.le(1))
    for y, name in ((1, "y = 1"), (em.P - 1, "y = -1")):
        for sign in (0, 1):
            put(f"{name}, sign {sign}", em.le(y | sign << 255))
    on = 0
    for y in range(em.P, 2**255):                    # the 19 non-canonical y, either sign bit
        on += em.decode_reference(em.le(y)) is not None
        for sign in (0, 1):
            put(f"y = p + {y - em.P}, sign {sign}", em.le(y | sign << 255))
    assert on == 12
    rng = np.random.default_rng(25519)
    for k in range(100):
        put(f"random {k}", rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
    seen = set()
    for name in ("verify_edges.json", "verify_torsion.json"):
        for c in json.load(open(os.path.join(GOLDEN, name))):
            pub = bytes.fromhex(c["pub"])
            if pub not in seen:
                seen.add(pub)
                put(f"{name}: key of '{c['name']}'", pub)
    names = [r[0] for r in rows]
    strings = em.arr([r[1] for r in rows], 32)
    classes = np.array([r[2] for r in rows], np.uint8)
    strings.setflags(write=False)
    classes.setflags(write=False)
    return names, strings, classes


def mismatches(got, want, names=None):
    """the first items whose class is not the expected one, readable"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    at = np.nonzero(got != want)[0][:8]
    return [(int(i), names[i % len(names)] if names else None, int(got[i]), int(want[i])) for i in at]
