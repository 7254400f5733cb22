"""chacha20poly1305_seal of janus_amd/csrc/hpke_prims.h (no HIP in it): the AEAD half the kernels of
hpke_seal_gpu.h run per report for ChaCha20-Poly1305, built with g++ and checked on the CPU against
RFC 8439's vector, its own open, and messages sealed by the host library under a fixed ephemeral
key.  For KDF 2 / 3 the key and base nonce come from the header's hpke_kdf512_key_nonce; for KDF 1
they come from the pure-Python RFC 9180 schedule of tests/hpke_suite_model.py, as in
tests/test_hpke_prims.py: an independent reference for the AEAD alone (the SHA-256 key schedule
of hpke_kdf256.h and the whole seal lane run on the CPU in tests/test_hpke_lane_prims.py).
Every command also runs through a -fsanitize=address,undefined build of the stand-alone driver
(tests/native/hpke_seal_host.cpp), which is its own program and uses every input from, and writes
every output to, a heap block of exactly its length."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import hpke_suite_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hpke_seal_host.cpp")
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
PT_LENS = (0, 1, 15, 16, 17, 63, 64, 65)
AAD_LENS = (0, 1, 16, 61)


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_seal_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "hpke_seal_san",
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


def test_rfc8439_aead_vector(prims):
    """RFC 8439 §2.8.2 (the constants of tests/test_hpke_prims.py)."""
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
    assert run(prims, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}"]) == [(ct + tag).hex()]


def test_seal_then_open_round_trips(prims):
    rng = np.random.default_rng(84392)
    lines, want = [], []
    for pl in PT_LENS:
        for al in AAD_LENS:
            key, nonce, aad, pt = rnd(rng, 32), rnd(rng, 12), rnd(rng, al), rnd(rng, pl)
            lines.append(f"rt {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}")
            want.append(f"1 {hx(pt)}")
    assert run(prims, lines) == want


def _x25519(sk, point):
    out = ctypes.create_string_buffer(32)
    assert lib().prio3gpu_x25519_batch(sk, point, 1, out, 0) == 0
    return out.raw


@pytest.mark.parametrize("kdf", [1, 2, 3])
def test_seal_equals_host_seal_under_a_fixed_ephemeral_key(prims, kdf):
    rng = np.random.default_rng(9180 + kdf)
    kp = H.generate_hpke_config_and_private_key(7, H.KEM_X25519_HKDF_SHA256, kdf,
                                                H.AEAD_CHACHA20POLY1305)
    lines, want = [], []
    for pl in PT_LENS:
        for al in AAD_LENS:
            sk_e, pt, aad = rnd(rng, 32), rnd(rng, pl), rnd(rng, al)
            _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert enc == H.public_key(H.KEM_X25519_HKDF_SHA256, sk_e)
            ss = M.kem_shared_secret(_x25519(sk_e, kp.config.public_key), enc,
                                     kp.config.public_key)
            if kdf == 1:
                _, key, nonce = M.key_schedule(1, 3, ss, INFO)
                lines.append(f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}")
            else:
                psk_id_hash, info_hash = M.context_hashes(kdf, 3, INFO)
                lines.append(f"hseal {kdf} {hx(ss)} {hx(psk_id_hash)} {hx(info_hash)} {hx(aad)} "
                             f"{hx(pt)}")
            want.append(ct.hex())
    assert run(prims, lines) == want
