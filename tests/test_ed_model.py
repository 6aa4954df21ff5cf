"""tests/ed_model.py, the integer model every feature's expected values come from, against anchors that are not the model: its
own two group laws against each other, the oracle's public keys, the vectors of RFC 8032, the reference's recorded verdicts
(tests/golden/verify_edges.json, verify_torsion.json) and the byte strings on which the two decoders have to differ.  CPU only."""
import random

import ed_model as em
from ed_model import H, L, P, le
from keyed_model import NO_KEY


def decode(enc):
    return em.ext(em.decode_reference(enc))


def test_the_model_group_law_against_the_affine_one():
    rng = random.Random(5)
    base = (em.BX, em.BY)
    assert (-em.BX * em.BX + em.BY * em.BY - 1 - em.D * em.BX * em.BX * em.BY * em.BY) % P == 0 and em.BX % 2 == 0
    assert em.is_neutral(em.pmul(L, em.B)) and not em.is_neutral(em.pmul(L - 1, em.B))
    for _ in range(20):
        k1, k2 = rng.randrange(L), rng.randrange(1 << 64)
        q = em.mul(k2, base)
        assert em.affine(em.pmul(k1, em.B)) == em.mul(k1, base)
        assert em.affine(em.pmul2(k1, em.B, k2, em.ext(q))) == em.mul(k1 + k2 * k2, base)
        assert em.affine(em.pdbl(em.ext(q))) == em.add(q, q) and em.affine(em.padd(em.ext(q), em.pneg(em.ext(q)))) == (0, 1)
        assert em.affine(decode(em.encode(em.ext(q)))) == q
    for enc in em.torsion_encodings():                   # every encoding of the eight points decodes, to a point 8 kills
        assert em.is_neutral(em.pmul(8, decode(enc)))
    # x = 0 takes either sign bit; a non-canonical y counts
    assert em.affine(decode((1 | 1 << 255).to_bytes(32, "little"))) == (0, 1) == em.affine(decode((P + 1).to_bytes(32, "little")))


def test_scalar_multiples_of_the_base_point_against_the_oracle(oracle):
    """the public key of a seed is [a]B with a clamped from SHA-512(seed): 32 random seeds"""
    rng = random.Random(20261020)
    for _ in range(32):
        seed = rng.randbytes(32)
        assert em.encode(em.pmul(em.clamped(seed), em.B)) == oracle.genpub(seed)


def test_verify_accepts_the_vectors_of_rfc8032(golden):
    """Ed25519ctx on the message, Ed25519ph on its SHA-512; and not under the other flag or another context"""
    vectors = golden("rfc8032_dom2.json")["vectors"]
    assert len(vectors) == 2
    for v in vectors:
        sig, pk, msg, context = (H(v[k]) for k in ("sig", "pk", "msg", "context"))
        mprime = em.sha(msg) if v["flag"] else msg
        assert em.encode(em.pmul(em.clamped(H(v["sk"])), em.B)) == pk
        assert em.verify(sig, pk, mprime, em.dom2(v["flag"], context))
        assert not em.verify(sig, pk, mprime, em.dom2(1 - v["flag"], context))
        assert not em.verify(sig, pk, mprime, em.dom2(v["flag"], context + b"x")) and not em.verify(sig, pk, mprime)


def test_verify_reproduces_the_recorded_verdicts_of_the_reference(golden):
    """every edge and torsion vector whose key decodes under the reference's import; the 33 edge vectors whose key is on no
    curve point belong to the exact path.  The counts are asserted: a decoder that refuses more keys fails here"""
    compared, skipped, wrong = {}, {}, []
    for name in ("verify_edges.json", "verify_torsion.json"):
        compared[name] = skipped[name] = 0
        for c in golden(name):
            sig, pub, msg = H(c["sig"]), H(c["pub"]), H(c["msg"])
            if em.decode_reference(pub) is None:
                skipped[name] += 1
                continue
            compared[name] += 1
            if em.verify(sig, pub, msg) != c["accept"]:
                wrong.append(c["name"])
    assert not wrong, wrong
    assert compared == {"verify_edges.json": 240, "verify_torsion.json": 192}
    assert skipped == {"verify_edges.json": 33, "verify_torsion.json": 0}


def test_the_two_decoders_differ_exactly_where_they_must():
    """y >= p, and x = 0 with the sign bit set: the reference's import takes them, RFC 8032's decoding refuses them"""
    strings = [le(P), le(P + 1), le(2**255 - 1), le(1 | 1 << 255)] + em.torsion_encodings()
    strings += [le(y | sign << 255) for y in (0, 1, 3, 4, P - 1, P + 2, P + 18) for sign in (0, 1)]
    differ = 0
    for enc in strings:
        v = em.num(enc)
        y, sign = v & (2**255 - 1), v >> 255
        loose, strict = em.decode_reference(enc), em.decode_strict(enc)
        if loose is None:
            assert strict is None
            continue
        x, y_mod = loose
        assert y_mod == y % P and x & 1 == (sign if x else 0) and (-x * x + y_mod * y_mod - 1 - em.D * x * x * y_mod * y_mod) % P == 0
        refused = y >= P or (x == 0 and sign == 1)
        assert (strict is None) == refused and (refused or strict == loose), enc.hex()
        differ += refused
    for enc in em.torsion_encodings():
        assert em.decode_reference(enc) is not None
    assert em.decode_reference(le(2**255 - 1)) is not None and em.decode_reference(le(P + 1)) == (0, 1)     # y = 18 and y = 1
    assert em.decode_strict(le(1)) == (0, 1) and em.decode_strict(le(1 | 1 << 255)) is None
    assert differ >= 10
    assert NO_KEY == le(2) and em.decode_reference(NO_KEY) is None and em.decode_strict(NO_KEY) is None


def test_the_inverse_of_zero_is_zero():
    """as the reference's fld_inv; the affine addition needs no case for the neutral element"""
    assert em.inv(0) == 0 and em.inv(1) == 1 and em.inv(2) * 2 % P == 1
    base = (em.BX, em.BY)
    for pt in (base, em.mul(12345, base), (0, P - 1), (0, 1)):
        assert em.add(pt, (0, 1)) == pt == em.add((0, 1), pt)
    assert em.small_order_ys() == frozenset(y for _, y in em.torsion_points()) and len(em.torsion_points()) == 8
