"""The team ChaCha20-Poly1305 of janus_amd/csrc/chacha_poly_team.h (no HIP in it): what a wave of
hpke_open_team.h's and hpke_seal_team.h's kernels runs per report under AEAD 3, built with g++ and
checked on the CPU with the 64 lanes simulated in a loop (tests/native/chacha_poly_team_host.cpp).
poly1305_mul and the powers a lane uses against Python integers mod 2^130 - 5, the striped MAC
against poly1305_mac and an integer Poly1305 at every body length where the stripe changes shape
(and at the largest limbs the lane join can meet), the team open and seal against
chacha20poly1305_open / _seal, RFC 8439 §2.8.2, tampering, the share sink's header check and
realigned stores, and the ciphertext sink at every kind of slot offset.  Every command also runs
through a -fsanitize=address,undefined build of the driver, which is its own program and uses every
input from, and writes every output to, a heap block of exactly its length."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "chacha_poly_team_host.cpp")
P = (1 << 130) - 5
# 0 and 1 block, around one ChaCha block, around a full trip of 64 chunks (4096 bytes; 4032 is its
# last chunk's start), around the second trip's first chunk, around two trips, and a third trip
BODY_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 4031, 4032, 4095, 4096, 4097, 4159, 4160, 8191, 8192,
             8193, 12289)
AAD_LENS = (0, 60, 92)
R_MAX = 0x0ffffffc0ffffffc0ffffffc0fffffff        # every bit the clamp leaves
LIMB_BOUND = (1 << 27) + (1 << 10)                # poly1305_mul's stated operand bound, exclusive


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "chacha_poly_team_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "chacha_poly_team_san",
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


def limbs(v: int):
    """v < 2^130 as five 26-bit limbs."""
    return [(v >> (26 * i)) & 0x3ffffff for i in range(5)]


def value(ls) -> int:
    return sum(int(x) << (26 * i) for i, x in enumerate(ls))


def clamp(r: int) -> int:
    return r & R_MAX


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def poly1305(key: bytes, msg: bytes) -> bytes:
    """RFC 8439 §2.5.1 on integers."""
    r, s = clamp(int.from_bytes(key[:16], "little")), int.from_bytes(key[16:], "little")
    h = 0
    for o in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[o:o + 16] + b"\1", "little")) * r % P
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def aead_mac_data(aad: bytes, body: bytes) -> bytes:
    return pad16(aad) + pad16(body) + struct.pack("<QQ", len(aad), len(body))


def check_partly_reduced(ls):
    """What poly1305_mul and poly1305_block promise of their result."""
    assert ls[0] < 1 << 26 and ls[1] < (1 << 26) + (1 << 10) and max(ls[2:]) < 1 << 26, ls


def test_poly1305_mul_equals_integers_mod_p(team):
    rng = np.random.default_rng(130)
    top = [LIMB_BOUND - 1] * 5                       # every limb at the stated bound
    edge = [limbs(0), limbs(1), limbs(P - 1), limbs(P), limbs((1 << 130) - 1), top,
            limbs(R_MAX)]
    ops = [(a, b) for a in edge for b in edge]
    for _ in range(20):                              # reduced operands, and unreduced ones
        ops.append((limbs(int.from_bytes(rnd(rng, 17), "little") % (1 << 130)),
                    limbs(int.from_bytes(rnd(rng, 17), "little") % (1 << 130))))
        ops.append(([int(x) for x in rng.integers(0, LIMB_BOUND, 5)],
                    [int(x) for x in rng.integers(0, LIMB_BOUND, 5)]))
    out = run(team, ["mul " + " ".join(map(str, a + b)) for a, b in ops])
    for (a, b), line in zip(ops, out):
        got = [int(x) for x in line.split()]
        check_partly_reduced(got)
        assert value(got) % P == value(a) * value(b) % P, (a, b)


def test_the_powers_a_lane_uses_equal_pow(team):
    rng = np.random.default_rng(253)
    for r in (0, 1, R_MAX, clamp(int.from_bytes(rnd(rng, 16), "little")),
              int.from_bytes(rnd(rng, 16), "little")):          # the last one is clamped there
        exps = list(range(0, 257)) + [253, 511]
        out = run(team, [f"pow {hx(r.to_bytes(16, 'little'))} {e}" for e in exps])
        for e, line in zip(exps, out):
            got = [int(x) for x in line.split()]
            check_partly_reduced(got)
            assert value(got) % P == pow(clamp(r), e, P), (hex(r), e)


def test_striped_mac_equals_the_serial_mac_at_every_stripe_shape(team):
    rng = np.random.default_rng(1305)
    cases = []
    for al in AAD_LENS:
        for bl in BODY_LENS:
            cases.append((rnd(rng, 32), rnd(rng, al), rnd(rng, bl)))
    # the lane join at its largest limbs: every block all ones under the largest r (and s)
    big = R_MAX.to_bytes(16, "little") + b"\xff" * 16
    for al in AAD_LENS:
        for bl in BODY_LENS:
            cases.append((big, b"\xff" * al, b"\xff" * bl))
    # Products mod p spread those limbs evenly, so that case does not pass 32 bits.  This one does:
    # under r = 1 a chunk of sixteen 0xff and 48 zero bytes leaves limb 1 of its lane's sum at 2^26
    # exactly (the last block's 2^128 bit carries out of limb 4 and 5 x 1 ripples up from limb 0),
    # and sixty-four of them are 2^32: without the carry pass between the butterfly's halves limb 1
    # of the sum wraps to 0.
    cases.append(((1).to_bytes(16, "little") + bytes(range(16)), b"",
                  (b"\xff" * 16 + bytes(48)) * 64))
    out = run(team, [f"tmac {hx(k)} {hx(a)} {hx(b)}" for k, a, b in cases])
    for (k, a, b), line in zip(cases, out):
        want = poly1305(k, aead_mac_data(a, b)).hex()
        assert line == f"{want} {want}", (len(a), len(b), k == big)


def _cases(rng):
    for al in AAD_LENS:
        for pl in BODY_LENS:
            yield rnd(rng, 32), rnd(rng, 12), rnd(rng, al), rnd(rng, pl)


def test_team_open_equals_lane_open(team):
    rng = np.random.default_rng(8439)
    cases = list(_cases(rng))
    cts = run(team, [f"seal {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p in cases])
    for (k, n, a, p), ct in zip(cases, cts):
        assert len(ct) == 2 * (len(p) + 16)
    lane = run(team, [f"open {hx(k)} {hx(n)} {hx(a)} {ct}" for (k, n, a, p), ct in zip(cases, cts)])
    got = run(team, [f"topen {hx(k)} {hx(n)} {hx(a)} {ct}" for (k, n, a, p), ct in zip(cases, cts)])
    assert got == lane == [f"1 {hx(p)}" for k, n, a, p in cases]


def test_team_seal_equals_lane_seal(team):
    rng = np.random.default_rng(9348)
    cases = list(_cases(rng))
    lane = run(team, [f"seal {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p in cases])
    got = run(team, [f"tseal {hx(k)} {hx(n)} {hx(a)} {hx(p)} 0" for k, n, a, p in cases])
    assert got == lane
    for (k, n, a, p), ct in zip(cases, got):
        assert len(ct) == 2 * (len(p) + 16)


def test_rfc8439_aead_vector_through_both_team_paths(team):
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
    out = run(team, [f"topen {hx(key)} {hx(nonce)} {hx(aad)} {hx(ct + tag)}",
                     f"tseal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)} 0",
                     f"tseal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)} 5"])
    assert out == [f"1 {pt.hex()}", (ct + tag).hex(), (ct + tag).hex()]
    # the MAC alone under the one-time key the RFC lists (§2.8.2, "Poly1305 Key")
    otk = bytes.fromhex("7bac2b252db447af09b67a55a4e955840ae1d6731075d9eb2a9375783ed553ff")
    assert run(team, [f"tmac {hx(otk)} {hx(aad)} {hx(ct)}"]) == [f"{tag.hex()} {tag.hex()}"]


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def test_a_flipped_bit_fails_and_leaves_zeros(team):
    rng = np.random.default_rng(403)
    key, nonce, aad, pt = rnd(rng, 32), rnd(rng, 12), rnd(rng, 92), rnd(rng, 4101)
    ct = bytes.fromhex(run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}"])[0])
    body = len(pt)
    assert body > 64 * 64 and body % 16           # a second trip that ends in a partial block
    bad = {"tag": (aad, _flip(ct, body + 5, 3)), "chunk 0": (aad, _flip(ct, 3)),
           "chunk 63": (aad, _flip(ct, 64 * 63 + 63, 7)), "chunk 64": (aad, _flip(ct, 64 * 64)),
           "partial last block": (aad, _flip(ct, body - 1, 1)), "aad": (_flip(aad, 60), ct)}
    lines = [f"topen {hx(key)} {hx(nonce)} {hx(a)} {hx(c)}" for a, c in bad.values()]
    lines += [f"open {hx(key)} {hx(nonce)} {hx(a)} {hx(c)}" for a, c in bad.values()]
    assert run(team, lines) == [f"0 {hx(bytes(body))}"] * (2 * len(bad))
    # the same through the share sink: the plaintext there is a PlaintextInputShare
    share = rnd(rng, 4101 - 6)
    frame = b"\0\0" + struct.pack(">I", len(share)) + share
    ct = bytes.fromhex(run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0])
    lines = [f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {hx(ct)} {len(share)} {s}" for s in (0, 3)]
    want = [f"1 0 {hx(share)}"] * 2
    for where in (len(frame) + 5, 3, 64 * 63 + 63, 64 * 64, len(frame) - 1):
        for shift in (0, 3):
            lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {hx(_flip(ct, where))} "
                         f"{len(share)} {shift}")
            want.append(f"0 0 {hx(bytes(len(share)))}")
    for shift in (0, 3):
        lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(_flip(aad, 60))} {hx(ct)} "
                     f"{len(share)} {shift}")
        want.append(f"0 0 {hx(bytes(len(share)))}")
    assert run(team, lines) == want


def test_share_sink_drops_the_header_and_realigns_the_row(team):
    rng = np.random.default_rng(611)
    lines, want = [], []
    for slen in (1, 10, 26, 48, 58, 59, 1018, 1019, 4090, 4091, 8200):
        key, nonce, aad, share = rnd(rng, 32), rnd(rng, 12), rnd(rng, 60), rnd(rng, slen)
        frame = b"\0\0" + struct.pack(">I", slen) + share
        ct = run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0]
        for shift in (0, 1, 6, 10):   # 0: the row is aligned to 16 (pieces of 2, 4, 8, 2)
            lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {ct} {slen} {shift}")
            want.append(f"1 0 {hx(share)}")
    assert run(team, lines) == want


@pytest.mark.parametrize("header", ["extensions", "longer", "shorter"])
def test_share_sink_refuses_another_header(team, header):
    rng = np.random.default_rng(9)
    for slen in (10, 48, 1019, 4200):
        key, nonce, aad = rnd(rng, 32), rnd(rng, 12), rnd(rng, 60)
        body = rnd(rng, slen)
        frame = {"extensions": b"\0\1" + body[:1] + struct.pack(">I", slen - 1) + body[1:],
                 "longer": b"\0\0" + struct.pack(">I", slen + 1) + body,
                 "shorter": b"\0\0" + struct.pack(">I", slen - 1) + body}[header]
        assert len(frame) == 6 + slen
        ct = run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}"])[0]
        lines = [f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {ct} {slen} {s}" for s in (0, 5)]
        assert run(team, lines) == [f"1 1 {hx(bytes(slen))}"] * 2


def test_seal_through_the_ciphertext_sink_at_every_kind_of_offset(team):
    """The driver's slot is the end of a heap block that starts on a 16-byte boundary: it answers
    with an error when a byte before the slot changed, and the sanitizer build sees one after."""
    rng = np.random.default_rng(715)
    lines, want = [], []
    for pl in BODY_LENS:
        key, nonce, aad, pt = rnd(rng, 32), rnd(rng, 12), rnd(rng, 60), rnd(rng, pl)
        lane = run(team, [f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}"])[0]
        for off in (0, 1, 7, 15):
            lines.append(f"tseal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)} {off}")
            want.append(lane)
    assert run(team, lines) == want
