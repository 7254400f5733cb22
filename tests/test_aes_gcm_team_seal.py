"""The team AES-GCM seal of janus_amd/csrc/aes_gcm_team.h (no HIP in it): what a wave of
hpke_seal_team.h's kernels runs per report, built with g++ and checked on the CPU with the 64 lanes
simulated in a loop (tests/native/aes_gcm_team_seal_host.cpp).  The team seal against aes_gcm_seal
at every block count where the stripes change shape, its output through aes_gcm_open and the team
open (tests/native/aes_gcm_team_host.cpp, the open's own driver), the share source against the
Python-built PlaintextInputShare, and the ciphertext sink at every kind of slot alignment inside a
0xa5-filled block.  Every command also runs through a -fsanitize=address,undefined build of the
driver, which is its own program and uses every input from a heap block of exactly its length."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "aes_gcm_team_seal_host.cpp")
OPEN_SRC = os.path.join(ROOT, "tests", "native", "aes_gcm_team_host.cpp")
PT_LENS = (0, 1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4101)
AAD_LENS = (0, 60, 92)
SHARE_LENS = (1, 10, 26, 48, 1018, 1019, 2576)
SHIFTS = (0, 1, 2, 4, 6, 8, 10, 15)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(tmp_path_factory, name, src, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), src], check=True)
    return str(out)


@pytest.fixture(scope="module")
def bins(tmp_path_factory):
    """{"plain" | "sanitized": (the seal's driver, the open's driver)}"""
    return {"plain": (_build(tmp_path_factory, "team_seal_host", SRC, []),
                      _build(tmp_path_factory, "team_open_host", OPEN_SRC, [])),
            "sanitized": (_build(tmp_path_factory, "team_seal_san", SRC, SAN),
                          _build(tmp_path_factory, "team_open_san", OPEN_SRC, SAN))}


@pytest.fixture(params=["plain", "sanitized"])
def team(request, bins):
    return bins[request.param]


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


def _cases(rng):
    for nk in (16, 32):
        for al in AAD_LENS:
            for pl in PT_LENS:   # nb = 0, < 64, 64, 65, 128 +- 1, partial last blocks
                yield rnd(rng, nk), rnd(rng, 12), rnd(rng, al), rnd(rng, pl)


def test_team_seal_equals_lane_seal_and_opens_under_both_opens(team):
    seal_bin, open_bin = team
    rng = np.random.default_rng(5341)
    cases = list(_cases(rng))
    lane = run(seal_bin, [f"seal {hx(k)} {hx(n)} {hx(a)} {hx(p)}" for k, n, a, p in cases])
    got = run(seal_bin, [f"tseal {hx(k)} {hx(n)} {hx(a)} {hx(p)} 0 0" for k, n, a, p in cases])
    assert got == lane
    for (k, n, a, p), ct in zip(cases, got):
        assert len(ct) == 2 * (len(p) + 16)
    want = [f"1 {hx(p)}" for k, n, a, p in cases]
    for cmd in ("open", "topen"):
        assert run(open_bin, [f"{cmd} {hx(k)} {hx(n)} {hx(a)} {ct}"
                              for (k, n, a, p), ct in zip(cases, got)]) == want


def test_share_source_equals_the_seal_of_the_built_frame(team):
    seal_bin, open_bin = team
    rng = np.random.default_rng(77)
    lines, frames = [], []
    for nk in (16, 32):
        for slen in SHARE_LENS:
            key, nonce, aad, share = rnd(rng, nk), rnd(rng, 12), rnd(rng, 92), rnd(rng, slen)
            frame = b"\0\0" + struct.pack(">I", slen) + share
            frames.append(f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}")
            lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {hx(share)} 0 0")
    got = run(seal_bin, lines)
    assert got == run(seal_bin, frames)
    # and back through the team open's share sink: the row is the share again
    back = [f"tshare {' '.join(ln.split()[1:4])} {ct} {len(ln.split()[4]) // 2} 0"
            for ln, ct in zip(lines, got)]
    assert run(open_bin, back) == [f"1 0 {ln.split()[4]}" for ln in lines]


@pytest.mark.parametrize("shift", SHIFTS)
def test_ciphertext_sink_at_any_slot_alignment(team, shift):
    """The slot starts `shift` bytes past a 16-byte boundary of a 0xa5-filled block with 16 more
    bytes behind it: the bytes are the aligned seal's and the driver answers "err" if any byte
    outside the slot changed."""
    seal_bin, _ = team
    rng = np.random.default_rng(900 + shift)
    lines, want = [], []
    for nk in (16, 32):
        key, nonce, aad = rnd(rng, nk), rnd(rng, 12), rnd(rng, 60)
        for pl in (0, 1, 15, 16, 17, 1024, 1025, 2049):
            pt = rnd(rng, pl)
            want.append(f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)}")
            lines.append(f"tseal {hx(key)} {hx(nonce)} {hx(aad)} {hx(pt)} {shift} 16")
        for slen in SHARE_LENS:
            share = rnd(rng, slen)
            frame = b"\0\0" + struct.pack(">I", slen) + share
            want.append(f"seal {hx(key)} {hx(nonce)} {hx(aad)} {hx(frame)}")
            lines.append(f"tshare {hx(key)} {hx(nonce)} {hx(aad)} {hx(share)} {shift} 16")
    # an exact block too (no bytes behind the slot): the sanitized build sees a store past it
    lines += [ln[:ln.rindex(" ")] + " 0" for ln in lines]
    assert run(seal_bin, lines) == run(seal_bin, want) * 2
