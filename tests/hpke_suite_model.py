"""Pure-Python models shared by tests/test_hpke_prims.py (CPU) and tests/test_gpu_hpke_suites.py
(GPU): Poly1305 over big integers (RFC 8439 §2.5) with the crafted final-reduction cases, and the
RFC 9180 DHKEM shared secret and key schedule over `hmac` alone."""
import hashlib
import hmac

import numpy as np

P1305 = (1 << 130) - 5
R_CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
HASH = {1: hashlib.sha256, 2: hashlib.sha384, 3: hashlib.sha512}
NK = {1: 16, 2: 32, 3: 32}


def poly1305(key: bytes, msg: bytes) -> bytes:
    """h = (h + block || 0x01) r mod 2^130 - 5 per 16-byte block; tag = (h + s) mod 2^128."""
    r = int.from_bytes(key[:16], "little") & R_CLAMP
    s = int.from_bytes(key[16:32], "little")
    acc = 0
    for o in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[o:o + 16] + b"\x01", "little")) * r % P1305
    return ((acc + s) % (1 << 128)).to_bytes(16, "little")


def _le16(x):
    return x.to_bytes(16, "little")


# r = 1: the accumulator before the final reduction is the plain sum of the blocks (each with its
# 2^128 bit), so two blocks reach 2^130 - 2, p and p - 1.  (second block, tag with s = 0)
CRAFTED = [
    ((1 << 128) - 1, "03" + "00" * 15),   # 2^130 - 2 -> 3
    ((1 << 128) - 4, "00" * 16),          # exactly p -> 0
    ((1 << 128) - 5, "fa" + "ff" * 15),   # p - 1: must not be reduced
]


def poly1305_cases():
    """[(key, msg)]: RFC 8439 §2.5.2, 2,000 random ones of 0-130 bytes, the largest clamped r over
    1-9 all-0xff blocks, and the crafted final-reduction cases with s = 0 and s = all 0xff."""
    cases = [(bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b"),
              b"Cryptographic Forum Research Group")]
    rng = np.random.default_rng(1305)
    for i in range(2000):
        ln = i % 131
        cases.append((rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                      rng.integers(0, 256, ln, dtype=np.uint8).tobytes()))
    for nb in range(1, 10):
        for s in (bytes(16), b"\xff" * 16, rng.integers(0, 256, 16, dtype=np.uint8).tobytes()):
            cases.append((_le16(R_CLAMP) + s, b"\xff" * (16 * nb)))
    for s in (bytes(16), b"\xff" * 16):
        for second, _ in CRAFTED:
            cases.append((_le16(1) + s, _le16((1 << 128) - 1) + _le16(second)))
    return cases


def crafted_tags_s0():
    """The crafted cases' tags with s = 0, as the table of their derivation has them."""
    return [bytes.fromhex(t) for _, t in CRAFTED]


# ---- RFC 9180 ------------------------------------------------------------------------------------
def _extract(h, salt, ikm):
    return hmac.new(salt or bytes(h().digest_size), ikm, h).digest()


def _expand(h, prk, info, L):
    assert L <= h().digest_size
    return hmac.new(prk, info + b"\x01", h).digest()[:L]


def labeled_extract(h, suite_id, salt, label, ikm):
    return _extract(h, salt, b"HPKE-v1" + suite_id + label + ikm)


def labeled_expand(h, suite_id, prk, label, info, L):
    return _expand(h, prk, L.to_bytes(2, "big") + b"HPKE-v1" + suite_id + label + info, L)


def kem_shared_secret(dh: bytes, enc: bytes, pk: bytes) -> bytes:
    """DHKEM(X25519, HKDF-SHA256) ExtractAndExpand (§4.1)."""
    sid = b"KEM" + (0x20).to_bytes(2, "big")
    prk = labeled_extract(hashlib.sha256, sid, b"", b"eae_prk", dh)
    return labeled_expand(hashlib.sha256, sid, prk, b"shared_secret", enc + pk, 32)


def suite_id(kdf: int, aead: int) -> bytes:
    return b"HPKE" + b"".join(x.to_bytes(2, "big") for x in (0x20, kdf, aead))


def context_hashes(kdf: int, aead: int, info: bytes):
    h, sid = HASH[kdf], suite_id(kdf, aead)
    return (labeled_extract(h, sid, b"", b"psk_id_hash", b""),
            labeled_extract(h, sid, b"", b"info_hash", info))


def key_schedule(kdf: int, aead: int, shared_secret: bytes, info: bytes):
    """KeySchedule(mode_base) (§5.1) -> (secret, key, base_nonce)."""
    h, sid = HASH[kdf], suite_id(kdf, aead)
    psk_id_hash, info_hash = context_hashes(kdf, aead, info)
    ctx = b"\x00" + psk_id_hash + info_hash
    secret = labeled_extract(h, sid, shared_secret, b"secret", b"")
    return (secret, labeled_expand(h, sid, secret, b"key", ctx, NK[aead]),
            labeled_expand(h, sid, secret, b"base_nonce", ctx, 12))
