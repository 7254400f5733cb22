"""janus_amd/csrc/p256.h and p256_kem.h (no HIP in them): the GF(p) arithmetic, point decoding,
scalar multiplication and DHKEM(P-256, HKDF-SHA256) shared secret that the kernels k_p256_dh /
k_p256_dh_idx run per report, built with g++ and checked on the CPU against tests/p256_model.py (affine arithmetic on
Python integers) and the host library.  Every command also runs through a
-fsanitize=address,undefined build of the stand-alone driver (tests/native/p256_host.cpp), which is
its own program and uses every input from a heap block of exactly its length."""
import os
import subprocess

import numpy as np
import pytest

from tests import p256_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "p256_host.cpp")
P, N = E.P, E.N


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
                   + extra + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "p256_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "p256_san",
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


# ---- GF(p) ---------------------------------------------------------------------------------------
OPS = {"mul": lambda a, b: a * b % P, "sqr": lambda a, b: a * a % P, "add": lambda a, b: (a + b) % P,
       "sub": lambda a, b: (a - b) % P, "inv": lambda a, b: pow(a, P - 2, P)}
EDGE = ([0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**224, 2**255, E.R]
        + [(2**32 - 1) << (32 * i) for i in range(8)]           # one all-ones word
        + [2**224 - 1, 2**256 - 2**224 + 2**192 - 1])           # seven; the all-ones words of p


def _field_cases():
    rng = np.random.default_rng(256)
    pairs = [(a, b) for a in EDGE for b in EDGE]
    pairs += [(int.from_bytes(rng.bytes(32), "big") % P, int.from_bytes(rng.bytes(32), "big") % P)
              for _ in range(2000)]
    return [(op, a, b) for a, b in pairs for op in OPS]


def test_field(prims):
    assert all(0 <= e < P for e in EDGE)
    cases = _field_cases()
    out = run(prims, [f"fe {op} {h32(a)} {h32(b)}" for op, a, b in cases])
    for (op, a, b), got in zip(cases, out):
        assert got == h32(OPS[op](a, b)), (op, hex(a), hex(b), got)
    assert run(prims, [f"fe inv {h32(0)} {h32(0)}"]) == [h32(0)]


# ---- decode --------------------------------------------------------------------------------------
def test_decode(prims):
    rng = np.random.default_rng(65)
    valid = [E.G, *E.X0] + [E.random_point(rng) for _ in range(20)]
    bad = E.invalid_encodings(rng) + [E.encode(E.G)[:64], E.encode(E.G) + b"\x00", b"\x04"]
    out = run(prims, [f"dec {E.encode(pt).hex()}" for pt in valid] + [f"dec {e.hex()}" for e in bad])
    assert out[:len(valid)] == [f"1 {h32(x)} {h32(y)}" for x, y in valid]
    assert out[len(valid):] == ["0"] * len(bad)


# ---- scalar multiplication -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul_cases():
    """[(k, point, x([k] point))] from the model, computed once for both builds."""
    rng = np.random.default_rng(186)
    points = [E.G, *E.X0] + [E.random_point(rng) for _ in range(5)]
    scalars = E.edge_scalars() + [E.random_scalar(rng) for _ in range(50)]
    assert all(1 <= k < N for k in scalars) and scalars[-51].bit_length() == 56
    return [(k, pt, E.mul(k, pt)[0]) for pt in points for k in scalars]


def test_scalar_mul(prims, mul_cases):
    out = run(prims, [f"mul {h32(k)} {E.encode(pt).hex()}" for k, pt, _ in mul_cases])
    for (k, pt, want), got in zip(mul_cases, out):
        assert got == h32(want), (hex(k), pt)


def test_scalar_mul_refuses_invalid_points(prims):
    rng = np.random.default_rng(4)
    bad = E.invalid_encodings(rng)
    assert run(prims, [f"mul {h32(3)} {e.hex()}" for e in bad]) == ["invalid"] * len(bad)


def test_scalar_mul_matches_host_public_key(prims):
    """The host library's P-256 (OpenSSL) as a second reference: pk = [sk] G."""
    from janus_amd import hpke as H
    kp = H.generate_hpke_config_and_private_key(1, H.KEM_P256_HKDF_SHA256, 1, 1)
    out = run(prims, [f"mul {kp.private_key.hex()} {E.encode(E.G).hex()}"])
    assert out == [kp.config.public_key[1:33].hex()]


# ---- the KEM half --------------------------------------------------------------------------------
def test_kem_shared_secret(prims):
    rng = np.random.default_rng(9180)
    lines, want = [], []
    for dh in (rng.bytes(32), bytes(32), b"\xff" * 32):
        for _ in range(3):
            enc, pk = E.encode(E.random_point(rng)), E.encode(E.random_point(rng))
            lines.append(f"kem {dh.hex()} {enc.hex()} {pk.hex()}")
            want.append(E.kem_shared_secret(dh, enc, pk).hex())
    assert run(prims, lines) == want


def test_dh_lane(prims):
    """One lane of the DH kernels end to end: a valid enc gives (1, shared secret), (0, sqrt b) with
    a scalar of our choosing included; a refused or absent enc gives (0, zeros)."""
    rng = np.random.default_rng(41)
    sk = E.random_scalar(rng)
    pk = E.encode(E.mul(sk, E.G))
    lines, want = [], []
    for pt in [E.G, *E.X0] + [E.random_point(rng) for _ in range(3)]:
        enc = E.encode(pt)
        dh = E.mul(sk, pt)[0].to_bytes(32, "big")
        lines.append(f"lane {h32(sk)} {enc.hex()} {pk.hex()}")
        want.append("1 " + E.kem_shared_secret(dh, enc, pk).hex())
    for enc in E.invalid_encodings(rng) + [E.encode(E.G)[:64], b""]:
        lines.append(f"lane {h32(sk)} {enc.hex() or '-'} {pk.hex()}")
        want.append("0 " + bytes(32).hex())
    assert run(prims, lines) == want
