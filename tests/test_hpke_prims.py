"""janus_amd/csrc/hpke_prims.h (no HIP in it): the SHA-384/512, HMAC, RFC 9180 key schedule, ChaCha20
and Poly1305 that the kernels of hpke_gpu.h run per report for the wider HPKE suites, built with
g++ and checked on the CPU against hashlib / hmac, a big-integer Poly1305, a pure-Python RFC 9180
key schedule and messages sealed by the host library.  (KDF 1's SHA-256 schedule, hpke_kdf256.h,
runs on the CPU in tests/test_hpke_lane_prims.py; here its keys come from the Python model, the
independent reference.)  Every command also runs through a
-fsanitize=address,undefined build of the stand-alone driver (tests/native/hpke_prims_host.cpp),
which is its own program and uses every input from a heap block of exactly its length."""
import ctypes
import hashlib
import hmac
import os
import subprocess

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import hpke_suite_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hpke_prims_host.cpp")
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
MSG_LENS = (0, 1, 111, 112, 113, 127, 128, 129, 239, 240)   # around the 112-byte padding boundary
KEY_LENS = (32, 48, 64)


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_prims_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_prims_san",
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


def unhx(s):
    return b"" if s == "-" else bytes.fromhex(s)


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- SHA-384 / SHA-512 / HMAC --------------------------------------------------------------------
def test_sha_and_hmac(prims):
    rng = np.random.default_rng(512)
    lines, want = [], []
    for kdf in (2, 3):
        for ln in MSG_LENS:
            for msg in (rnd(rng, ln), b"\xff" * ln):
                lines.append(f"sha {kdf} {hx(msg)}")
                want.append(M.HASH[kdf](msg).hexdigest())
                for kl in KEY_LENS:
                    key = rnd(rng, kl)
                    lines.append(f"hmac {kdf} {hx(key)} {hx(msg)}")
                    want.append(hmac.new(key, msg, M.HASH[kdf]).hexdigest())
    lines.append("sha 3 " + hx(b"abc"))      # FIPS 180-4's example
    want.append(hashlib.sha512(b"abc").hexdigest())
    assert run(prims, lines) == want


# ---- Poly1305 ------------------------------------------------------------------------------------
def test_poly1305_model_on_crafted_cases():
    """The model itself: RFC 8439 §2.5.2, and the tags the crafted accumulators must give."""
    key, msg = M.poly1305_cases()[0]
    assert M.poly1305(key, msg).hex() == "a8061dc1305136c6c22b8baf0c0127a9"
    one = (1).to_bytes(16, "little")
    ff = ((1 << 128) - 1).to_bytes(16, "little")
    for (second, _), tag in zip(M.CRAFTED, M.crafted_tags_s0()):
        assert M.poly1305(one + bytes(16), ff + second.to_bytes(16, "little")) == tag


def test_poly1305(prims):
    cases = M.poly1305_cases()
    assert len(cases) == 1 + 2000 + 27 + 6
    out = run(prims, [f"poly {hx(k)} {hx(m)}" for k, m in cases])
    for i, ((k, m), line) in enumerate(zip(cases, out)):
        assert line == M.poly1305(k, m).hex(), (i, k.hex(), m.hex())
    assert out[0] == "a8061dc1305136c6c22b8baf0c0127a9"
    assert [unhx(x) for x in out[-6:-3]] == M.crafted_tags_s0()     # s = 0
    # s = all 0xff: (h + 2^128 - 1) mod 2^128 = h - 1, the carry out of the final add dropped
    assert out[-3:] == ["02" + "00" * 15, "ff" * 16, "f9" + "ff" * 15]


# ---- key schedule --------------------------------------------------------------------------------
def test_key_schedule(prims):
    rng = np.random.default_rng(9180)
    lines, want = [], []
    for kdf in (2, 3):
        for aead in (1, 2, 3):
            for il in (0, 21, 200):
                for _ in range(3):
                    ss, info = rnd(rng, 32), rnd(rng, il)
                    psk_id_hash, info_hash = M.context_hashes(kdf, aead, info)
                    lines.append(f"ks {kdf} {aead} {hx(ss)} {hx(psk_id_hash)} {hx(info_hash)}")
                    want.append(" ".join(x.hex() for x in M.key_schedule(kdf, aead, ss, info)))
    assert run(prims, lines) == want


# ---- ChaCha20-Poly1305 open ----------------------------------------------------------------------
PT_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
AAD_LENS = (0, 15, 16, 17, 92)


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def _x25519(sk, point):
    out = ctypes.create_string_buffer(32)
    assert lib().prio3gpu_x25519_batch(sk, point, 1, out, 0) == 0
    return out.raw


def test_rfc8439_aead_vector(prims):
    """RFC 8439 §2.8.2."""
    key = bytes(range(0x80, 0xa0))
    nonce = bytes.fromhex("070000004041424344454647")
    aad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the "
          b"future, sunscreen would be it.")
    ct = bytes.fromhex(
        "d31a8d34648e60db7b86afbc53ef7ec2a4aded51296e08fea9e2b5a736ee62d63dbea45e8ca9671282fafb69"
        "da92728b1a71de0a9e060b2905d6a5b67ecd3b3692ddbd7f2d778b8c9803aee328091b58fab324e4fad67594"
        "5585808b4831d7bc3ff4def08e4b7a9de576d26586cec64b6116")
    tag = bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")
    assert len(ct) == len(pt)
    out = run(prims, [f"open {hx(key)} {hx(nonce)} {hx(aad)} {hx(ct + tag)}"])
    assert out == [f"1 {pt.hex()}"]


@pytest.mark.parametrize("kdf", [1, 2, 3])
def test_chacha20poly1305_open_of_host_seals(prims, kdf):
    rng = np.random.default_rng(8439 + kdf)
    kp = H.generate_hpke_config_and_private_key(7, H.KEM_X25519_HKDF_SHA256, kdf,
                                                H.AEAD_CHACHA20POLY1305)
    lines, want = [], []
    for pl in PT_LENS:
        for al in AAD_LENS:
            pt, aad = rnd(rng, pl), rnd(rng, al)
            _, enc, ct = H.seal(kp.config, INFO, pt, aad)
            ss = M.kem_shared_secret(_x25519(kp.private_key, enc), enc, kp.config.public_key)
            _, key, nonce = M.key_schedule(kdf, 3, ss, INFO)
            lines.append(f"open {hx(key)} {hx(nonce)} {hx(aad)} {hx(ct)}")
            want.append(f"1 {hx(pt)}")
            bad = [(aad, _flip(ct, 8 * pl + int(rng.integers(0, 128))))]         # the tag
            if al:
                bad.append((_flip(aad, int(rng.integers(0, 8 * al))), ct))
            if pl:
                bad.append((aad, _flip(ct, int(rng.integers(0, 8 * pl)))))
            for a2, c2 in bad:
                lines.append(f"open {hx(key)} {hx(nonce)} {hx(a2)} {hx(c2)}")
                want.append(f"0 {hx(bytes(pl))}")
    assert run(prims, lines) == want
