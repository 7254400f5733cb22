"""janus_amd/csrc/plan_hpke.h with the "hpke_gpu_p256" option: which reports of P-256 keys the GPU
opens.  A stand-alone driver (tests/native/hpke_plan_p256_host.cpp) built with g++, plain and with
-fsanitize=address,undefined; the keypairs come from tests/p256_model.py, since a P-256 keypair
must pass the host's validation (scalar in [1, n), public key on the curve) to get a group."""
import os
import subprocess

import numpy as np
import pytest

from tests import p256_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "hpke_plan_p256_host.cpp")
SUITES, P256_OPT = 1, 2                       # HPKE_OPT_SUITES, HPKE_OPT_P256


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
                   + extra + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "plan_p256", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "plan_p256_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(params=["plain", "sanitized"])
def drv(request, plain_bin, san_bin):
    return plain_bin if request.param == "plain" else san_bin


def run(binary, line):
    r = subprocess.run([binary], input=(line + "\n").encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode().splitlines()


def _p256_key(rng, cid, kdf=1, aead=1):
    sk = E.random_scalar(rng)
    return (cid, 0x10, kdf, aead, sk.to_bytes(32, "big"), E.encode(E.mul(sk, E.G)))


def _x25519_key(rng, cid, kdf=1, aead=1):
    return (cid, 0x20, kdf, aead, rng.bytes(32), rng.bytes(32))


def plan(binary, opts, strict, task_keys, global_keys, reports):
    """reports: [(config_id, status, enc_len, payload_len)] -> (route, groups)."""
    words = ["plan", opts, int(strict), len(task_keys), len(global_keys)]
    for cid, kem, kdf, aead, sk, pk in list(task_keys) + list(global_keys):
        words += [cid, kem, kdf, aead, sk.hex() or "-", pk.hex() or "-"]
    words.append(len(reports))
    for r in reports:
        words += list(r)
    out = run(binary, " ".join(str(w) for w in words))
    assert out[0].split()[0] == "route" and out[1].split()[0] == "groups"
    return out[0].split()[1:], [int(g) for g in out[1].split()[1:]]


@pytest.fixture(scope="module")
def keys():
    rng = np.random.default_rng(10)
    return dict(x=_x25519_key(rng, 1), a=_p256_key(rng, 2), b=_p256_key(rng, 3, 3, 3),
                g=_p256_key(rng, 4, 1, 2))


REPORTS = [(1, 0, 32, 64), (2, 0, 65, 64), (3, 0, 65, 64), (4, 0, 65, 64), (2, 0, 65, 64),
           (9, 0, 65, 64), (2, 8, 65, 64)]


def test_p256_keys_form_groups_with_the_option(drv, keys):
    tks, gks = [keys["x"], keys["a"], keys["b"]], [keys["g"]]
    for strict in (False, True):
        unknown = "H" if strict else "U"
        # both options: every key has a group, in order of first appearance
        route, groups = plan(drv, SUITES | P256_OPT, strict, tks, gks, REPORTS)
        assert route == ["0", "1", "2", "3", "1", unknown, "F"] and groups == [0, 1, 2, 3]
        # "hpke_gpu_p256" alone: only the HKDF-SHA256 / AES-128-GCM key of each KEM
        route, groups = plan(drv, P256_OPT, strict, tks, gks, REPORTS)
        assert route == ["0", "1", "H", "H", "1", unknown, "F"] and groups == [0, 1]


def test_routes_without_the_option_are_todays(drv, keys):
    tks, gks = [keys["x"], keys["a"], keys["b"]], [keys["g"]]
    for strict in (False, True):
        unknown = "H" if strict else "U"
        for opts in (0, SUITES):                     # "hpke_gpu_suites" adds no KEM
            route, groups = plan(drv, opts, strict, tks, gks, REPORTS)
            assert route == ["0", "H", "H", "H", "H", unknown, "F"] and groups == [0]


def test_enc_len_in_strict_and_request_mode(drv, keys):
    reports = [(2, 0, 65, 64), (2, 0, 64, 64), (2, 0, 66, 64), (2, 0, 32, 64), (2, 0, 65, 15),
               (1, 0, 65, 64), (1, 0, 32, 64)]
    tks = [keys["x"], keys["a"]]
    route, groups = plan(drv, P256_OPT, True, tks, [], reports)
    assert route == ["0", "H", "H", "H", "H", "H", "1"] and groups == [1, 0]
    route, groups = plan(drv, P256_OPT, False, tks, [], reports)      # the kernel rejects them
    assert route == ["0", "0", "0", "0", "0", "1", "1"] and groups == [1, 0]
    # strict: a malformed first report does not keep its key from getting a group later
    route, groups = plan(drv, P256_OPT, True, tks, [], [reports[1], reports[0]])
    assert route == ["H", "0"] and groups == [1]


def test_malformed_p256_keypairs_are_the_hosts(drv, keys):
    cid, kem, kdf, aead, sk, pk = keys["a"]
    off_curve = bytearray(pk)
    off_curve[64] ^= 1
    x_is_p = b"\x04" + E.P.to_bytes(32, "big") + E.SQRT_B.to_bytes(32, "big")
    bad = [(sk + b"\x00", pk), (sk, pk[:64]), (sk[:31], pk), (bytes(32), pk),
           (E.N.to_bytes(32, "big"), pk), (b"\xff" * 32, pk), (sk, bytes(off_curve)),
           (sk, b"\x02" + pk[1:]), (sk, x_is_p), (b"", pk), (sk, b"")]
    reports = [(2, 0, 65, 64), (2, 0, 65, 64)]
    for strict in (False, True):
        for s, p in bad:
            route, groups = plan(drv, SUITES | P256_OPT, strict, [(cid, kem, kdf, aead, s, p)],
                                 [], reports)
            assert route == ["H", "H"] and groups == [], (len(s), len(p))
        good = (cid, kem, kdf, aead, (E.N - 1).to_bytes(32, "big"), E.encode(E.mul(E.N - 1, E.G)))
        route, groups = plan(drv, P256_OPT, strict, [good], [], reports)
        assert route == ["0", "0"] and groups == [0]


def test_scalar_range(drv):
    for k, want in ((0, 0), (1, 1), (E.N - 1, 1), (E.N, 0), (E.N + 1, 0), ((1 << 256) - 1, 0),
                    (1 << 255, 1), (E.N - (1 << 128), 1), (E.N + (1 << 128), 0)):
        assert run(drv, "scalar " + k.to_bytes(32, "big").hex()) == [str(want)], hex(k)
