"""A pure-Python model of NIST P-256 for tests/test_p256_prims.py (CPU) and
tests/test_gpu_hpke_p256.py (GPU): affine arithmetic on Python integers (FIPS 186-4 D.1.2.3), SEC 1
uncompressed point encoding with full validation, and the DHKEM(P-256, HKDF-SHA256) shared secret of
RFC 9180 §4.1 over tests/hpke_suite_model.py's labelled HKDF."""
import hashlib

from tests import hpke_suite_model as M

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
GX = 0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296
GY = 0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5
G = (GX, GY)
R = 2**256 % P                       # the Montgomery radix of p256.h
KEM_ID = 0x0010


def on_curve(pt):
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x - 3 * x + B)) % P == 0


def sqrt(a):
    """A square root mod p (p = 3 mod 4), or None."""
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


SQRT_B = sqrt(B)
X0 = ((0, SQRT_B), (0, P - SQRT_B))  # the two points with x = 0


def add(p1, p2):
    """Affine addition; None is the point at infinity."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def encode(pt):
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def decode(enc):
    """The point of a 65-byte uncompressed encoding, or None (DeserializePublicKey with the
    on-curve check)."""
    if len(enc) != 65 or enc[0] != 4:
        return None
    pt = (int.from_bytes(enc[1:33], "big"), int.from_bytes(enc[33:], "big"))
    return pt if on_curve(pt) else None


def random_point(rng):
    while True:
        x = int.from_bytes(rng.bytes(32), "big") % P
        y = sqrt((x * x * x - 3 * x + B) % P)
        if y is not None:
            return (x, y if rng.integers(0, 2) else P - y)


def _poly_rem(a, b):
    """a mod b for coefficient lists (lowest degree first) over GF(p); b's leading one nonzero."""
    a = a[:]
    inv = pow(b[-1], -1, P)
    while len(a) >= len(b):
        q = a[-1] * inv % P
        for i in range(len(b)):
            a[len(a) - len(b) + i] = (a[len(a) - len(b) + i] - q * b[i]) % P
        a.pop()
        while a and a[-1] == 0:
            a.pop()
    return a


def _poly_mulmod(a, b, f):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % P
    return _poly_rem(out, f)


def point_with_small_y():
    """A curve point whose y is a small integer, so that y + p still fits 32 bytes: the first
    y = 1, 2, ... for which x^3 - 3 x + b - y^2 has exactly one root, found as the linear
    gcd(x^p - x, f)."""
    for y in range(1, 200):
        f = [(B - y * y) % P, P - 3, 0, 1]
        acc, base, e = [1], [0, 1], P
        while e:
            if e & 1:
                acc = _poly_mulmod(acc, base, f)
            base = _poly_mulmod(base, base, f)
            e >>= 1
        g = acc + [0] * (2 - len(acc))
        g[1] = (g[1] - 1) % P
        while g and g[-1] == 0:
            g.pop()
        a, b = f, g
        while b:
            a, b = b, _poly_rem(a, b)
        if len(a) == 2:
            pt = (-a[0] * pow(a[1], -1, P) % P, y)
            assert on_curve(pt)
            return pt
    raise AssertionError("no point with a small y")


def random_scalar(rng):
    return int.from_bytes(rng.bytes(40), "big") % (N - 1) + 1


def edge_scalars():
    """k = 1, 2, 3, n - 2, n - 1, (n - 1) / 2, (n + 1) / 2, 2^255, 2^32, 200 leading zero bits."""
    return [1, 2, 3, N - 2, N - 1, (N - 1) // 2, (N + 1) // 2, 1 << 255, 1 << 32,
            (1 << 55) | 0x2f5a9c13d4e6b7]


def invalid_encodings(rng):
    """Encodings DeserializePublicKey must refuse: x = p with y = sqrt(b) (a non-canonical form of a
    valid point), y + p where it fits 32 bytes, one flipped bit of y, the prefixes 0x00 / 0x02 /
    0x03, all zero, all 0xff."""
    out = [b"\x04" + P.to_bytes(32, "big") + SQRT_B.to_bytes(32, "big")]
    pt = point_with_small_y()
    out.append(b"\x04" + pt[0].to_bytes(32, "big") + (pt[1] + P).to_bytes(32, "big"))
    good = bytearray(encode(random_point(rng)))
    good[33 + int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
    out.append(bytes(good))
    for prefix in (0, 2, 3):
        out.append(bytes([prefix]) + encode(G)[1:])
    out += [bytes(65), b"\xff" * 65]
    assert all(decode(e) is None for e in out)
    return out


def kem_shared_secret(dh: bytes, enc: bytes, pk: bytes) -> bytes:
    """DHKEM(P-256, HKDF-SHA256) ExtractAndExpand (RFC 9180 §4.1): kem_context is 130 bytes."""
    sid = b"KEM" + KEM_ID.to_bytes(2, "big")
    prk = M.labeled_extract(hashlib.sha256, sid, b"", b"eae_prk", dh)
    return M.labeled_expand(hashlib.sha256, sid, prk, b"shared_secret", enc + pk, 32)
