"""The sender's side of DHKEM(P-256, HKDF-SHA256) as the GPU seal runs it per report (no HIP in
it): janus_amd/csrc/p256.h's ladder with the lane's own scalar and both affine coordinates,
p256_kem.h's p256_eph_lane / p256_eph_shared_secret (kernels k_p256_eph, k_p256_eph_kem) and
hpke_lane.h's hpke_seal_lane with bc.dh_ok set, built with g++ and checked on the CPU against
tests/p256_model.py (affine arithmetic on Python integers), RFC 9180 A.3.1 and the host library.
Every command also runs through a -fsanitize=address,undefined build of the stand-alone driver
(tests/native/p256_eph_host.cpp), which is its own program and uses every input from a heap block
of exactly its length."""
import json
import os
import subprocess

import numpy as np
import pytest

from janus_amd import hpke as H
from tests import hpke_suite_model as M
from tests import p256_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "p256_eph_host.cpp")
P, N = E.P, E.N
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
# RFC 9180 A.3.1's skEm: DHKEM(P-256, HKDF-SHA256), HKDF-SHA256, AES-128-GCM
SK_EM = bytes.fromhex("4995788ef4b9d6132b249ce59a77281493eb39af373d236a1fe415cb0c2d7beb")
ST_HPKE_DECRYPT = 4


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
                   + extra + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "p256_eph_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "p256_eph_san",
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


def h32(x):
    return x.to_bytes(32, "big").hex()


def hx(b):
    return bytes(b).hex() or "-"


# ---- the ladder with the lane's own scalar -------------------------------------------------------
@pytest.fixture(scope="module")
def mul_cases():
    """[(k, point, [k] point)] from the model, computed once for both builds: the scalars 1, 2, 3,
    n - 2, n - 1, (n +- 1) / 2, 2^255, 2^32 and 50 random ones over G, the two points with x = 0
    and five random points."""
    rng = np.random.default_rng(1861)
    points = [E.G, *E.X0] + [E.random_point(rng) for _ in range(5)]
    scalars = [1, 2, 3, N - 2, N - 1, (N - 1) // 2, (N + 1) // 2, 2**255, 2**32] \
        + [E.random_scalar(rng) for _ in range(50)]
    assert all(1 <= k < N for k in scalars)
    return [(k, pt, E.mul(k, pt)) for pt in points for k in scalars]


def test_lane_ladder_gives_both_coordinates(prims, mul_cases):
    out = run(prims, [f"mulxy {h32(k)} {E.encode(pt).hex()}" for k, pt, _ in mul_cases])
    for (k, pt, (x, y)), got in zip(mul_cases, out):
        assert got == f"1 {h32(x)} {h32(y)}", (hex(k), pt)


def test_lane_ladder_x_only_form(prims, mul_cases):
    """p256_dh_x instantiated for the lane's own scalar: the same text as the recipient's DH."""
    out = run(prims, [f"mulx {h32(k)} {E.encode(pt).hex()}" for k, pt, _ in mul_cases])
    for (k, pt, (x, _)), got in zip(mul_cases, out):
        assert got == h32(x), (hex(k), pt)


INVALID_SCALARS = [0, N, N + 1, 2**256 - 1]


def test_invalid_scalars_give_ok_0_and_zero_outputs(prims):
    rng = np.random.default_rng(7)
    pts = [E.G, E.X0[0], E.random_point(rng)]
    out = run(prims, [f"mulxy {h32(k)} {E.encode(pt).hex()}" for pt in pts for k in INVALID_SCALARS])
    assert out == [f"0 {h32(0)} {h32(0)}"] * (len(pts) * len(INVALID_SCALARS))
    pk = E.encode(E.random_point(rng))
    out = run(prims, [f"eph {h32(k)} {pk.hex()}" for k in INVALID_SCALARS])
    assert out == [f"0 {bytes(65).hex()} {bytes(32).hex()}"] * len(INVALID_SCALARS)


def test_lane_ladder_refuses_invalid_points(prims):
    bad = E.invalid_encodings(np.random.default_rng(5))
    assert run(prims, [f"mulxy {h32(3)} {e.hex()}" for e in bad]) == ["invalid"] * len(bad)


# ---- the whole eph lane --------------------------------------------------------------------------
def test_eph_lane_gives_enc_and_shared_secret(prims):
    rng = np.random.default_rng(9181)
    lines, want = [], []
    for k in [1, N - 1, 2**255] + [E.random_scalar(rng) for _ in range(6)]:
        pk_pt = E.random_point(rng)
        pk, enc = E.encode(pk_pt), E.encode(E.mul(k, E.G))
        dh = E.mul(k, pk_pt)[0].to_bytes(32, "big")
        lines.append(f"eph {h32(k)} {pk.hex()}")
        want.append(f"1 {enc.hex()} {E.kem_shared_secret(dh, enc, pk).hex()}")
    assert run(prims, lines) == want


def test_eph_lane_matches_host_public_key(prims):
    """The host library's P-256 (OpenSSL) as a second reference: enc = pk(sk_e)."""
    kp = H.generate_hpke_config_and_private_key(1, H.KEM_P256_HKDF_SHA256, 1, 1)
    sk_e = (1 + int.from_bytes(os.urandom(32), "big") % (N - 1)).to_bytes(32, "big")
    out = run(prims, [f"eph {sk_e.hex()} {kp.config.public_key.hex()}"])
    assert out[0].split()[:2] == ["1", H.public_key(H.KEM_P256_HKDF_SHA256, sk_e).hex()]


# ---- hpke_seal_lane with bc.dh_ok set ------------------------------------------------------------
def _consts(kdf, aead, info):
    h = M.HASH[kdf]
    sid = b"HPKE" + b"".join(x.to_bytes(2, "big") for x in (E.KEM_ID, kdf, aead))
    return (f"{kdf} {aead} {hx(M.labeled_extract(h, sid, b'', b'psk_id_hash', b''))} "
            f"{hx(M.labeled_extract(h, sid, b'', b'info_hash', info))}")


def test_seal_lane_reproduces_rfc9180_a31(prims):
    """0x0010 / 1 / 1 under the vector's skEm: the lane gives the vector's enc and ct."""
    with open(os.path.join(ROOT, "tests", "golden", "hpke_rfc9180_vectors.json")) as f:
        v = [x for x in json.load(f)
             if (x["kem_id"], x["kdf_id"], x["aead_id"]) == (0x10, 1, 1)][0]
    enc, ct, pk = (bytes.fromhex(v[k]) for k in ("enc", "ct", "pkRm"))
    # the vector's enc is [skEm] G: the key belongs to this vector
    assert E.encode(E.mul(int.from_bytes(SK_EM, "big"), E.G)) == enc
    info, aad, pt = (bytes.fromhex(v[k]) for k in ("info", "aad", "pt"))
    out = run(prims, [f"lseal {_consts(1, 1, info)} {SK_EM.hex()} {pk.hex()} {hx(aad)} {hx(pt)} "
                      f"{len(ct) + 3}"])
    assert out == [f"0 {enc.hex()} {(ct + bytes(3)).hex()}"]


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_seal_lane_p256_form_equals_host_seal(prims, kdf, aead):
    """Every KDF and AEAD, the context hashes from tests/hpke_suite_model.py: the lane gives
    H.seal's bytes under the same ephemeral scalar, the 65-byte enc in its slot and zeros up to
    ct_cap; an invalid scalar gives status 4 and zeros in both slots."""
    rng = np.random.default_rng(2560 + 10 * kdf + aead)
    kp = H.generate_hpke_config_and_private_key(9, H.KEM_P256_HKDF_SHA256, kdf, aead)
    pk = kp.config.public_key
    head = _consts(kdf, aead, INFO)
    lines, want = [], []
    for pl in (0, 15, 16, 17, 257):
        for al in (0, 15, 16, 17, 257):
            sk_e = h32(E.random_scalar(rng))
            pt, aad = rng.bytes(pl), rng.bytes(al)
            _, enc, payload = H.seal(kp.config, INFO, pt, aad,
                                     ephemeral_private_key=bytes.fromhex(sk_e))
            assert len(enc) == 65
            lines.append(f"lseal {head} {sk_e} {pk.hex()} {hx(aad)} {hx(pt)} {len(payload) + 5}")
            want.append(f"0 {enc.hex()} {(payload + bytes(5)).hex()}")
    for k in INVALID_SCALARS:
        lines.append(f"lseal {head} {h32(k)} {pk.hex()} {hx(rng.bytes(9))} {hx(rng.bytes(33))} 49")
        want.append(f"{ST_HPKE_DECRYPT} {bytes(65).hex()} {bytes(49).hex()}")
    assert run(prims, lines) == want
