"""Several waves per report, on the CPU: plan_hpke.h's team_split_plan and the sub-range stripes,
segment sums and joins of janus_amd/csrc/aes_gcm_team.h and chacha_poly_team.h (no HIP in them), the
text hpke_team_split.h's kernels run, built with g++ and checked with a segment's 64 lanes simulated
in a loop (tests/native/team_split_host.cpp).  The plan against its worked examples and invariants;
the two new exponentiations against Python integers and against repeated products; for AES-128-GCM,
AES-256-GCM and ChaCha20-Poly1305 the segments plus join against the one-team result and the serial
AEAD at every body length where a segment boundary moves; tampering in every kind of place; and the
share sink's header check, which only segment 0 may see.  Every command also runs through a
-fsanitize=address,undefined build of the driver, which is its own program and uses every input
from, and writes every output to, a heap block of exactly its length."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "team_split_host.cpp")
P = (1 << 130) - 5
R_MAX = 0x0ffffffc0ffffffc0ffffffc0fffffff
AEADS = (1, 2, 3)
KEY_LEN = {1: 16, 2: 32, 3: 32}
UNIT = {1: 64, 2: 64, 3: 256}          # one team stripe in blocks
AAD_LENS = (0, 60, 92)
SEGMENTS = (2, 3, 5)


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def plain_bin(tmp_path_factory):
    return _build(tmp_path_factory, "team_split_host", [])


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return _build(tmp_path_factory, "team_split_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(params=["plain", "sanitized"])
def drv(request, plain_bin, san_bin):
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


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


# ---- the plan -----------------------------------------------------------------------------------
def plan_model(n, body, unit, cap, min_blocks, wave_slots):
    nb = -(-body // 16)
    want = -(-wave_slots // n)
    s0 = min(cap, want, nb // min_blocks)
    if s0 < 2:
        return 1, nb
    L = -(-(-(-nb // s0)) // unit) * unit
    S = -(-nb // L)
    return (S, L) if S >= 2 else (1, nb)


def test_plan_worked_examples(plain_bin):
    table = [((1, 8192, 64, 8, 256, 2048), (2, 256)),
             ((1, 8193, 64, 8, 256, 2048), (2, 320)),
             ((1, 4080, 64, 8, 256, 2048), (1, 255)),
             ((1, 16006, 64, 8, 256, 2048), (3, 384)),
             ((1, 16006, 256, 8, 256, 2048), (2, 512)),
             ((1024, 134966, 64, 8, 4096, 2048), (2, 4224)),
             ((4096, 134966, 64, 8, 256, 2048), (1, 8436)),
             ((4096, 25600486, 256, 8, 4096, 2048), (1, 1600031)),
             ((4096, 8192, 64, 8, 256, 2048), (1, 512))]
    out = run(plain_bin, ["plan " + " ".join(map(str, args)) for args, _ in table])
    assert [tuple(map(int, line.split())) for line in out] == [want for _, want in table]


def test_plan_invariants_over_a_sweep(plain_bin):
    rng = np.random.default_rng(64)
    cases = []
    for n in (1, 2, 3, 16, 64, 255, 256, 1024, 2047, 2048, 2049, 4096):
        for unit in (64, 256):
            for min_blocks in (256, 512, 4096):
                for cap in (0, 1, 2, 3, 8, 256):
                    for body in (1, 4080, 8191, 8192, 8193, 16006, 134966, 25600486,
                                 int(rng.integers(1, 1 << 27)), int(rng.integers(1, 1 << 16))):
                        cases.append((n, body, unit, cap, min_blocks, 2048))
    out = run(plain_bin, ["plan " + " ".join(map(str, c)) for c in cases])
    for (n, body, unit, cap, min_blocks, slots), line in zip(cases, out):
        S, L = map(int, line.split())
        nb = -(-body // 16)
        assert (S, L) == plan_model(n, body, unit, cap, min_blocks, slots), (n, body, unit, cap)
        assert S >= 1 and S <= max(cap, 1)
        assert (S - 1) * L < nb <= S * L
        if S >= 2:
            assert L % unit == 0
        else:
            assert L == nb
        if nb < 2 * min_blocks or n >= slots:
            assert S == 1


# ---- the exponentiations ------------------------------------------------------------------------
def test_poly1305_pow64_equals_pow(drv):
    rng = np.random.default_rng(1305)
    exps = (0, 1, 511, 512, (1 << 20) + 3, (1 << 32) - 1, (1 << 63) + 5)
    lines, want = [], []
    for r in (1, R_MAX, int.from_bytes(rnd(rng, 16), "little")):   # clamped by the driver
        for e in exps:
            lines.append(f"pow64 {hx(r.to_bytes(16, 'little'))} {e}")
            want.append(pow(r & R_MAX, e, P))
    for line, w in zip(run(drv, lines), want):
        ls = [int(x) for x in line.split()]
        assert ls[0] < 1 << 26 and ls[1] < (1 << 26) + (1 << 10) and max(ls[2:]) < 1 << 26, ls
        assert sum(x << (26 * i) for i, x in enumerate(ls)) % P == w


def test_gf128_pow_equals_repeated_products(drv):
    rng = np.random.default_rng(128)
    lines = [f"gfpow {hx(rnd(rng, 16))} {k}" for k in (0, 1, 3, 6, 64)]
    for line in run(drv, lines):
        got, want = line.split()
        assert got == want
    one, zero = "80" + "00" * 15, "00" * 16        # H = 1 stays 1, H = 0 stays 0
    assert run(drv, [f"gfpow {one} 6", f"gfpow {zero} 6"]) == [f"{one} {one}", f"{zero} {zero}"]


# ---- segments plus join against one team and the serial AEAD ------------------------------------
def _bodies(L_blocks, S):
    """Body lengths in bytes around the boundaries of segments of L_blocks blocks."""
    lb = 16 * L_blocks
    return sorted({lb - 1, lb, lb + 1, 2 * lb, 2 * lb + 17, S * lb, (S - 1) * lb + 1})


def _split_cases(rng, aead):
    """(key, nonce, aad, text, L): every AAD length, S = 2, 3 and 5 reached exactly, and both an L
    of one unit and one whose L / 64 is no power of two (3 units)."""
    for i, S in enumerate(SEGMENTS):
        for units in (1, 3):
            L = units * UNIT[aead]
            for body in _bodies(L, S):
                if units == 3 and body not in (16 * L * S, 16 * L * (S - 1) + 1, 16 * L + 1):
                    continue      # the long segments: the boundaries that matter, to stay quick
                yield (rnd(rng, KEY_LEN[aead]), rnd(rng, 12), rnd(rng, AAD_LENS[i % 3]),
                       rnd(rng, body), L)
    for al in AAD_LENS:           # every AAD length at one shape more
        L = UNIT[aead]
        yield rnd(rng, KEY_LEN[aead]), rnd(rng, 12), rnd(rng, al), rnd(rng, 32 * L + 17), L


@pytest.mark.parametrize("aead", AEADS)
def test_split_seal_equals_team_and_serial_seal(drv, aead):
    rng = np.random.default_rng(900 + aead)
    cases = list(_split_cases(rng, aead))
    assert {-(-(-(-len(p) // 16)) // L) for *_, p, L in cases} >= set(SEGMENTS)
    args = [f"{aead} {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p, L in cases]
    split = run(drv, [f"sseal {x} {c[4]}" for x, c in zip(args, cases)])
    team = run(drv, [f"tseal {x}" for x in args])
    lane = run(drv, [f"lseal {x}" for x in args])
    assert split == team == lane
    for (k, n, a, p, L), ct in zip(cases, split):
        assert len(ct) == 2 * (len(p) + 16)


@pytest.mark.parametrize("aead", AEADS)
def test_split_open_equals_team_open(drv, aead):
    rng = np.random.default_rng(800 + aead)
    cases = list(_split_cases(rng, aead))
    args = [f"{aead} {hx(k)} {hx(n)} {hx(a)}" for k, n, a, p, L in cases]
    cts = run(drv, [f"lseal {x} {hx(c[3])}" for x, c in zip(args, cases)])
    split = run(drv, [f"sopen {x} {ct} {c[4]}" for x, ct, c in zip(args, cts, cases)])
    team = run(drv, [f"topen {x} {ct}" for x, ct in zip(args, cts)])
    assert split == team == [f"1 {hx(c[3])}" for c in cases]


@pytest.mark.parametrize("aead", AEADS)
def test_a_flipped_bit_fails_the_split_open(drv, aead):
    rng = np.random.default_rng(400 + aead)
    L = UNIT[aead]
    lb = 16 * L
    key, nonce, aad = rnd(rng, KEY_LEN[aead]), rnd(rng, 12), rnd(rng, 92)
    pt = rnd(rng, 2 * lb + 17 + 5)                  # three segments, a partial last block
    body = len(pt)
    assert body % 16 and -(-body // lb) == 3
    head = f"{aead} {hx(key)} {hx(nonce)}"
    ct = bytes.fromhex(run(drv, [f"lseal {head} {hx(aad)} {hx(pt)}"])[0])
    bad = {"first block": (aad, _flip(ct, 3)),
           "last block of the middle segment": (aad, _flip(ct, 2 * lb - 1, 7)),
           "first block of the last segment": (aad, _flip(ct, 2 * lb)),
           "partial last block": (aad, _flip(ct, body - 1, 1)),
           "tag": (aad, _flip(ct, body + 5, 3)),
           "aad": (_flip(aad, 60), ct)}
    lines = [f"sopen {head} {hx(a)} {hx(c)} {L}" for a, c in bad.values()]
    lines += [f"topen {head} {hx(a)} {hx(c)}" for a, c in bad.values()]
    assert run(drv, lines) == [f"0 {hx(bytes(body))}"] * (2 * len(bad))
    assert run(drv, [f"sopen {head} {hx(aad)} {hx(ct)} {L}"]) == [f"1 {hx(pt)}"]


@pytest.mark.parametrize("aead", AEADS)
def test_share_sink_header_check_fires_in_segment_0_only(drv, aead):
    """Every segment's sinks compare what they take for block 0 -- which only segment 0 holds.  A
    good header leaves every sink clean; another header marks segment 0's sink alone, however the
    later segments' first blocks look (here they begin with the very bytes of a bad header)."""
    rng = np.random.default_rng(600 + aead)
    L = UNIT[aead]
    lb = 16 * L
    slen = 2 * lb + 300
    head = lambda: f"{aead} {hx(rnd(rng, KEY_LEN[aead]))} {hx(rnd(rng, 12))}"
    aad = rnd(rng, 60)
    share = bytearray(rnd(rng, slen))
    for s in (1, 2):                                # plaintext bytes [s lb, s lb + 6): a bad header
        share[s * lb - 6:s * lb] = b"\0\1\xff\xff\xff\xff"
    share = bytes(share)
    lines, want = [], []
    frames = {"good": (b"\0\0" + struct.pack(">I", slen) + share, f"1 0 {hx(share)}"),
              "extensions": (b"\0\1" + share[:1] + struct.pack(">I", slen - 1) + share[1:],
                             f"1 1 {hx(bytes(slen))}"),
              "longer": (b"\0\0" + struct.pack(">I", slen + 1) + share, f"1 1 {hx(bytes(slen))}")}
    for frame, answer in frames.values():
        assert len(frame) == 6 + slen
        h = head()
        ct = run(drv, [f"lseal {h} {hx(aad)} {hx(frame)}"])[0]
        lines.append(f"sshare {h} {hx(aad)} {ct} {slen} {L}")
        want.append(answer)
        tampered = _flip(bytes.fromhex(ct), lb + 1)
        lines.append(f"sshare {h} {hx(aad)} {hx(tampered)} {slen} {L}")
        want.append(None)
    out = run(drv, lines)
    for line, w in zip(out, want):
        if w is None:                               # a failed tag: zeros whatever the header is
            ok, _mask, row = line.split()
            assert ok == "0" and row == hx(bytes(slen))
        else:
            assert line == w
