"""The per-lane code of the GPU HPKE open and seal (janus_amd/csrc/x25519.h, hpke_kdf256.h,
aes_gcm.h, hpke_lane.h: no HIP in them), built with g++ and checked on the CPU: X25519 against
RFC 7748 and the host ladder, AES against FIPS 197, AES-GCM against the GCM specification's
zero-key cases, its own round trip and forgeries, and the two whole lanes (hpke_seal_lane,
hpke_open_lane) for all nine X25519 suites against messages sealed by the host library under a
fixed ephemeral key -- which runs KDF 1's SHA-256 key schedule on the CPU as the kernels have it.
The P-256 form of the open lane (the shared secret given, validity in a flag) takes its shared
secret from tests/p256_model.py.  Every command also runs through a
-fsanitize=address,undefined build of the stand-alone driver (tests/native/hpke_lane_host.cpp),
which is its own program and uses every input from, and writes every output to, a heap block of
exactly its length."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import hpke_suite_model as M
from tests import p256_model as P256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hpke_lane_host.cpp")
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
PT_LENS = (0, 1, 15, 16, 17, 63, 64, 65)
AAD_LENS = (0, 1, 16, 61)
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
P25519 = 2**255 - 19
ST_HPKE_DECRYPT = 4


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_lane_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_lane_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(params=["plain", "sanitized"])
def prims(request, plain_bin, san_bin):
    return plain_bin if request.param == "plain" else san_bin


def run(binary, lines):
    r = subprocess.run([binary], input=("\n".join(lines) + "\n").encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def hx(b):
    return bytes(b).hex() or "-"


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


# ---- X25519 --------------------------------------------------------------------------------------
def test_x25519_rfc7748_vectors(prims):
    """RFC 7748 §5.2: the two input / output vectors, and the iteration after 1 and 1,000 rounds."""
    lines = [
        "x25519 a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4 "
        "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
        "x25519 4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d "
        "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
        "x25519iter 1",
        "x25519iter 1000",
    ]
    assert run(prims, lines) == [
        "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552",
        "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957",
        "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079",
        "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51",
    ]


def _host_x25519(sk, point):
    out = ctypes.create_string_buffer(32)
    assert lib().prio3gpu_x25519_batch(sk, point, 1, out, 0) == 0
    return out.raw


def test_x25519_equals_the_host_ladder(prims):
    """64 (scalar, u) pairs: u = 0, 1, p - 1, p, p + 1 (of small order: the DH value is all zero),
    u with bit 255 set (dropped), random ones."""
    rng = np.random.default_rng(7748)
    us = [v.to_bytes(32, "little") for v in (0, 1, P25519 - 1, P25519, P25519 + 1)]
    us.append(b"\xff" * 32)
    while len(us) < 64:  # every other one with the top bit set, the rest with it clear
        u = rnd(rng, 32)
        us.append(u[:31] + bytes([u[31] | 0x80 if len(us) % 2 else u[31] & 0x7f]))
    pairs = [(rnd(rng, 32), u) for u in us]
    got = run(prims, [f"x25519 {hx(k)} {hx(u)}" for k, u in pairs])
    want = [_host_x25519(k, u) for k, u in pairs]
    assert got == [w.hex() for w in want]
    assert all(w == bytes(32) for w in want[:5])


# ---- AES -----------------------------------------------------------------------------------------
def _sbox_model():
    """FIPS 197 §5.1.1: the inverse in GF(2^8) (by search) and the affine map."""
    def mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a = (a << 1) ^ (0x11b if a & 0x80 else 0)
            b >>= 1
        return r
    box = []
    for x in range(256):
        inv = next((y for y in range(256) if mul(x, y) == 1), 0)
        s = inv
        for i in range(1, 5):
            s ^= ((inv << i) | (inv >> (8 - i))) & 0xff
        box.append(s ^ 0x63)
    return bytes(box)


def test_aes_fips197_vectors_and_sbox_fill(prims):
    """FIPS 197 Appendix C.1 and C.3 through aes_expand + aes_encrypt with the S-box of
    aes_sbox_fill(sbox, 0, 1); filled by 64 callers (t, 64) it is the same 256 bytes."""
    pt = "00112233445566778899aabbccddeeff"
    out = run(prims, [f"aes {bytes(range(16)).hex()} {pt}", f"aes {bytes(range(32)).hex()} {pt}",
                      "sbox 1", "sbox 64"])
    assert out[0] == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert out[1] == "8ea2b7ca516745bfeafc49904b496089"
    assert out[2] == out[3] == _sbox_model().hex()


# ---- AES-GCM -------------------------------------------------------------------------------------
def test_gcm_zero_key_cases(prims):
    """The GCM specification's test cases 1, 2 (AES-128) and 13, 14 (AES-256): zero key, zero
    nonce, no AAD, an empty message and 16 zero bytes."""
    z12, z16 = "00" * 12, "00" * 16
    out = run(prims, [f"gcmseal {'00' * 16} {z12} - -", f"gcmseal {'00' * 16} {z12} - {z16}",
                      f"gcmseal {'00' * 32} {z12} - -", f"gcmseal {'00' * 32} {z12} - {z16}"])
    assert out == ["58e2fccefa7e3061367f1d57a4e7455a",
                   "0388dace60b6a392f328c2b971b2fe78" "ab6e47d42cec13bdf53a67b21257bddf",
                   "530f8afbc74536b9a963b4f1c4cb738b",
                   "cea7403d4d606b6e074ec5d3baf39d18" "d0d1c8a799996bf0265b98b5d48ab919"]


@pytest.mark.parametrize("nk", [16, 32])
def test_gcm_seal_then_open_round_trips_and_refuses_forgeries(prims, nk):
    """Over the length grid: the open of a seal gives the plaintext back; one flipped bit of the
    tag, of the ciphertext or of the AAD (each alone) gives false and an all-zero plaintext."""
    rng = np.random.default_rng(38 + nk)
    cases = [(rnd(rng, nk), rnd(rng, 12), rnd(rng, al), rnd(rng, pl))
             for pl in PT_LENS for al in AAD_LENS]
    cts = [bytes.fromhex(c) for c in
           run(prims, [f"gcmseal {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p in cases])]
    lines, want = [], []
    for (k, n, a, p), ct in zip(cases, cts):
        assert len(ct) == len(p) + 16
        lines.append(f"gcmopen {hx(k)} {hx(n)} {hx(a)} {hx(ct)}")
        want.append(f"1 {hx(p)}")
        bad = [(a, flip(ct, 8 * len(p) + int(rng.integers(128))))]
        if p:
            bad.append((a, flip(ct, int(rng.integers(8 * len(p))))))
        if a:
            bad.append((flip(a, int(rng.integers(8 * len(a)))), ct))
        for a2, ct2 in bad:
            lines.append(f"gcmopen {hx(k)} {hx(n)} {hx(a2)} {hx(ct2)}")
            want.append(f"0 {hx(bytes(len(p)))}")
    assert run(prims, lines) == want


# ---- the whole lane ------------------------------------------------------------------------------
def _sealed(kdf, aead, rng):
    """[(enc, dh, aad, pt, payload)] over the length grid under one recipient key, sealed by the
    host library with a fixed ephemeral key each; and the lane's batch constants as text."""
    kp = H.generate_hpke_config_and_private_key(7, H.KEM_X25519_HKDF_SHA256, kdf, aead)
    pk = kp.config.public_key
    psk_id_hash, info_hash = M.context_hashes(kdf, aead, INFO)
    head = f"{kdf} {aead}", f"{hx(pk)} {hx(psk_id_hash)} {hx(info_hash)}"
    cases = []
    for pl in PT_LENS:
        for al in AAD_LENS:
            sk_e, pt, aad = rnd(rng, 32), rnd(rng, pl), rnd(rng, al)
            _, enc, payload = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert enc == H.public_key(H.KEM_X25519_HKDF_SHA256, sk_e)
            cases.append((enc, _host_x25519(sk_e, pk), aad, pt, payload))
    return head, cases


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_seal_lane_equals_host_seal_under_a_fixed_ephemeral_key(prims, kdf, aead):
    """hpke_seal_lane over PackedBytes gives H.seal's bytes, enc in its slot and zeros up to
    ct_cap; an all-zero DH value gives status 4 and zeros in both slots."""
    (suite, consts), cases = _sealed(kdf, aead, np.random.default_rng(9180 + 10 * kdf + aead))
    lines, want = [], []
    for enc, dh, aad, pt, payload in cases:
        cap = len(payload) + 5
        lines.append(f"lseal {suite} {consts} {hx(enc)} {hx(dh)} {hx(aad)} {hx(pt)} {cap}")
        want.append(f"0 {enc.hex()} {(payload + bytes(5)).hex()}")
    enc, _, aad, pt, payload = cases[-1]
    lines.append(f"lseal {suite} {consts} {hx(enc)} {hx(bytes(32))} {hx(aad)} {hx(pt)} "
                 f"{len(payload)}")
    want.append(f"{ST_HPKE_DECRYPT} {bytes(32).hex()} {bytes(len(payload)).hex()}")
    assert run(prims, lines) == want


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_open_lane_opens_host_seals_and_rejects_with_zeros(prims, kdf, aead):
    """hpke_open_lane opens what H.seal produced (zeros from the body's end to pt_cap); a flipped
    bit of the tag, the ciphertext, the AAD or enc, and an all-zero DH value each give status 4
    and zeros up to pt_cap, which is larger than the body."""
    rng = np.random.default_rng(9181 + 10 * kdf + aead)
    (suite, consts), cases = _sealed(kdf, aead, rng)
    lines, want = [], []
    for enc, dh, aad, pt, payload in cases:
        cap = len(pt) + 3
        variants = [(enc, dh, aad, payload, True),
                    (enc, dh, aad, flip(payload, 8 * len(pt) + int(rng.integers(128))), False),
                    (flip(enc, int(rng.integers(256))), dh, aad, payload, False),
                    (enc, bytes(32), aad, payload, False)]
        if pt:
            variants.append((enc, dh, aad, flip(payload, int(rng.integers(8 * len(pt)))), False))
        if aad:
            variants.append((enc, dh, flip(aad, int(rng.integers(8 * len(aad)))), payload, False))
        for e, d, a, c, good in variants:
            lines.append(f"lopen {suite} 32 {consts} {hx(e)} {hx(d)} 1 {hx(a)} {hx(c)} {cap}")
            want.append(f"0 {(pt + bytes(3)).hex()}" if good
                        else f"{ST_HPKE_DECRYPT} {bytes(cap).hex()}")
    assert run(prims, lines) == want


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_open_lane_p256_form_takes_the_shared_secret_and_honours_the_flag(prims, kdf, aead):
    """With bc.dh_ok set the lane takes dh as the shared_secret (tests/p256_model.py's, from the
    ephemeral scalar and pkR) and skips the KEM half; dh_flag = 0 rejects a report that would
    open; an all-zero shared secret with the flag set is no marker."""
    rng = np.random.default_rng(256 + 10 * kdf + aead)
    kp = H.generate_hpke_config_and_private_key(9, H.KEM_P256_HKDF_SHA256, kdf, aead)
    pk = kp.config.public_key
    h = M.HASH[kdf]
    sid = b"HPKE" + b"".join(x.to_bytes(2, "big") for x in (P256.KEM_ID, kdf, aead))
    consts = (f"- {hx(M.labeled_extract(h, sid, b'', b'psk_id_hash', b''))} "
              f"{hx(M.labeled_extract(h, sid, b'', b'info_hash', INFO))}")
    sk_e = (1 + int.from_bytes(rnd(rng, 32), "big") % (P256.N - 1)).to_bytes(32, "big")
    dh = P256.mul(int.from_bytes(sk_e, "big"), P256.decode(pk))[0].to_bytes(32, "big")
    lines, want = [], []
    for pl, al in ((0, 0), (1, 61), (17, 1), (65, 16)):
        pt, aad = rnd(rng, pl), rnd(rng, al)
        _, enc, payload = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
        ss = P256.kem_shared_secret(dh, enc, pk)
        cap = pl + 3
        for secret, flag, good in ((ss, 1, True), (ss, 0, False), (bytes(32), 1, False),
                                   (flip(ss, int(rng.integers(256))), 1, False)):
            lines.append(f"lopen {kdf} {aead} 16 {consts} - {hx(secret)} {flag} {hx(aad)} "
                         f"{hx(payload)} {cap}")
            want.append(f"0 {(pt + bytes(3)).hex()}" if good
                        else f"{ST_HPKE_DECRYPT} {bytes(cap).hex()}")
    assert run(prims, lines) == want
