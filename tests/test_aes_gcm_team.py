"""The team AES-GCM of janus_amd/csrc/aes_gcm_team.h (no HIP in it): what a wave of
hpke_open_team.h's kernels runs per report, built with g++ and checked on the CPU with the 64 lanes
simulated in a loop (tests/native/aes_gcm_team_host.cpp).  gf128_mul against ghash_step and an
integer model of GF(2^128), the table of powers against repeated multiplication, the striped GHASH
against ghash_bytes at every block count where the stripes change shape, the team open against
aes_gcm_open and its keystream against aes_gcm_seal, tampering, and the share sink's header check
and realigned stores.  Every command also runs through a -fsanitize=address,undefined build of the
driver, which is its own program and uses every input from, and writes every output to, a heap block
of exactly its length."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "aes_gcm_team_host.cpp")
PT_LENS = (0, 1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4101)
AAD_LENS = (0, 60, 92)
SHARE_LENS = (1, 10, 26, 48, 1018, 1019, 2576)


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "aes_gcm_team_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "aes_gcm_team_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(params=["plain", "sanitized"])
def team(request, plain_bin, san_bin):
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


def gmul(x: int, y: int) -> int:
    """x * y in GF(2^128) on 128-bit integers read big-endian, GCM's bit order (SP 800-38D §6.3)."""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xe1 << 120) if v & 1 else v >> 1
    return z


def el(v: int) -> str:
    return v.to_bytes(16, "big").hex()


ONE = 1 << 127   # the field's one: the bit of x^0 comes first


def test_gf128_mul_equals_ghash_step_and_the_integer_model(team):
    rng = np.random.default_rng(128)
    h = int.from_bytes(rnd(rng, 16), "big")
    edge = [0, ONE, 1, h, (1 << 128) - 1]
    ops = [(a, b) for a in edge for b in edge]
    ops += [(int.from_bytes(rnd(rng, 16), "big"), int.from_bytes(rnd(rng, 16), "big"))
            for _ in range(40)]
    out = run(team, [f"mul {el(a)} {el(b)}" for a, b in ops])
    assert out == [el(gmul(a, b)) for a, b in ops]
    assert run(team, [f"mul {el(h)} {el(ONE)}"]) == [el(h)]
    steps = [(int.from_bytes(rnd(rng, 16), "big"), a, b) for a, b in ops]
    out = run(team, [f"step {el(y)} {el(x)} {el(k)}" for y, x, k in steps])
    assert out == [f"{el(gmul(y ^ x, k))} {el(gmul(y ^ x, k))}" for y, x, k in steps]


def test_power_table_equals_repeated_multiplication(team):
    rng = np.random.default_rng(64)
    for h in (int.from_bytes(rnd(rng, 16), "big"), ONE, 0, (1 << 128) - 1):
        want, p = [], ONE
        for _ in range(64):
            p = gmul(p, h)
            want.append(el(p))
        assert run(team, [f"powers {el(h)}"]) == ["".join(want)]
    # and through the driver's own product, one multiplication at a time
    h = int.from_bytes(rnd(rng, 16), "big")
    table = run(team, [f"powers {el(h)}"])[0]
    p = el(h)
    for e in range(1, 64):
        p = run(team, [f"mul {p} {el(h)}"])[0]
        assert table[32 * e:32 * e + 32] == p


def test_striped_ghash_equals_ghash_bytes_for_every_block_count(team):
    rng = np.random.default_rng(6464)
    h, y0 = rnd(rng, 16), rnd(rng, 16)
    # nb = 0, below 64, multiples of 64, one past them, and ragged last blocks
    lens = sorted(set(PT_LENS) | {16 * nb for nb in (2, 63, 64, 65, 127, 128, 129, 192, 193)}
                  | {16 * 64 + 1, 16 * 128 - 1, 16 * 129 - 15})
    lines = [f"tghash {hx(h)} {hx(y0)} {hx(rnd(rng, n))}" for n in lens]
    lines += [f"tghash {hx(h)} {hx(bytes(16))} {hx(rnd(rng, n))}" for n in (0, 16, 1025)]
    for ln, o in zip(lines, run(team, lines)):
        a, b = o.split()
        assert a == b, ln[:80]
    assert run(team, [f"tghash {hx(h)} {hx(y0)} -"]) == [f"{hx(y0)} {hx(y0)}"]


def _cases(rng):
    for nk in (16, 32):
        for al in AAD_LENS:
            for pl in PT_LENS:
                yield rnd(rng, nk), rnd(rng, 12), rnd(rng, al), rnd(rng, pl)


def test_team_open_equals_lane_open_and_its_keystream_the_seal(team):
    rng = np.random.default_rng(3896)
    cases = list(_cases(rng))
    cts = run(team, [f"seal {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p in cases])
    for (k, n, a, p), ct in zip(cases, cts):
        assert len(ct.replace("-", "")) == 2 * (len(p) + 16)
    lane = run(team, [f"open {hx(k)} {hx(n)} {hx(a)} {ct}" for (k, n, a, p), ct in zip(cases, cts)])
    got = run(team, [f"topen {hx(k)} {hx(n)} {hx(a)} {ct}" for (k, n, a, p), ct in zip(cases, cts)])
    assert got == lane == [f"1 {hx(p)}" for k, n, a, p in cases]
    ks = run(team, [f"tctr {hx(k)} {hx(n)} {hx(p)}" for k, n, a, p in cases])
    assert ks == [ct[:2 * len(p)] or "-" for (k, n, a, p), ct in zip(cases, cts)]


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("nk", [16, 32])
def test_a_flipped_bit_fails_and_leaves_zeros(team, nk):
    rng = np.random.default_rng(401 + nk)
    key, nonce, aad, pt = rnd(rng, nk), rnd(rng, 12), rnd(rng, 92), rnd(rng, 4101)
    ct = bytes.fromhex(run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}"])[0])
    body = len(pt)
    bad = {"tag": (aad, _flip(ct, body + 5, 3)), "block 0": (aad, _flip(ct, 3)),
           "block 63": (aad, _flip(ct, 16 * 63 + 15, 7)), "block 64": (aad, _flip(ct, 16 * 64)),
           "partial last block": (aad, _flip(ct, body - 1, 1)), "aad": (_flip(aad, 60), ct)}
    lines = [f"topen {hx(key)} {hx(nonce)} {hx(a)} {hx(c)}" for a, c in bad.values()]
    lines += [f"open {hx(key)} {hx(nonce)} {hx(a)} {hx(c)}" for a, c in bad.values()]
    assert run(team, lines) == [f"0 {hx(bytes(body))}"] * (2 * len(bad))
    # the same through the share sink: the plaintext there is a PlaintextInputShare
    share = rnd(rng, 4101 - 6)
    frame = b"\0\0" + struct.pack(">I", len(share)) + share
    ct = bytes.fromhex(run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0])
    lines = []
    for where in (len(frame) + 5, 3, 16 * 63 + 15, 16 * 64, len(frame) - 1):
        for shift in (0, 3):
            lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {hx(_flip(ct, where))} "
                         f"{len(share)} {shift}")
    assert run(team, lines) == [f"0 0 {hx(bytes(len(share)))}"] * len(lines)


def test_share_sink_drops_the_header_and_realigns_the_row(team):
    rng = np.random.default_rng(610)
    lines, want = [], []
    for nk in (16, 32):
        for slen in SHARE_LENS:
            key, nonce, aad, share = rnd(rng, nk), rnd(rng, 12), rnd(rng, 60), rnd(rng, slen)
            frame = b"\0\0" + struct.pack(">I", slen) + share
            ct = run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0]
            for shift in (0, 1, 6, 10):   # 0: the row is aligned to 16 (pieces of 2, 4, 8, 2)
                lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {ct} {slen} {shift}")
                want.append(f"1 0 {hx(share)}")
    assert run(team, lines) == want


@pytest.mark.parametrize("header", ["extensions", "longer", "shorter", "high byte"])
def test_share_sink_refuses_another_header(team, header):
    rng = np.random.default_rng(8)
    lines = []
    for slen in (10, 48, 1019):
        key, nonce, aad = rnd(rng, 16), rnd(rng, 12), rnd(rng, 60)
        body = rnd(rng, slen)
        frame = {"extensions": b"\0\1" + body[:1] + struct.pack(">I", slen - 1) + body[1:],
                 "longer": b"\0\0" + struct.pack(">I", slen + 1) + body,
                 "shorter": b"\0\0" + struct.pack(">I", slen - 1) + body,
                 "high byte": b"\0\0" + struct.pack(">I", slen | 1 << 24) + body}[header]
        assert len(frame) == 6 + slen
        ct = run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0]
        lines += [f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {ct} {slen} {s}" for s in (0, 5)]
        assert run(team, lines[-2:]) == [f"1 1 {hx(bytes(slen))}"] * 2
