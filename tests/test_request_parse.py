"""janus_amd/csrc/request_parse.h (no HIP in it): the PlaintextInputShare parser and the fault rule
that the kernels of helper_request.h run per report, built with g++ and checked on the CPU against
the host codec (prio3gpu_decode_plaintext_input_shares, prio3gpu_gather_prepare_inits'
fault rule, prio3gpu_apply_faults) over a few thousand generated plaintexts.  The same inputs run
through a -fsanitize=address,undefined build of the stand-alone driver
(tests/native/request_parse_host.cpp), which parses every plaintext from a heap block of exactly
its length."""
import os
import subprocess

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd.prio3 import _Sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "request_parse_host.cpp")
WANT = 32          # Prio3Sum's helper input share: two seeds
DEFER, MAX_LIST = 0xFE, 256


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                   + ["-o", str(out), SRC], check=True)
    return str(out)


@pytest.fixture(scope="module")
def parse_bin(tmp_path_factory):
    return _build(tmp_path_factory, "request_parse_host", [])


@pytest.fixture(scope="module")
def parse_bin_san(tmp_path_factory):
    return _build(tmp_path_factory, "request_parse_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(binary, lines):
    r = subprocess.run([binary], input=("\n".join(lines) + "\n").encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode().splitlines()


# ---- generated plaintexts ------------------------------------------------------------------------
def ext(t, data=b""):
    return t.to_bytes(2, "big") + len(data).to_bytes(2, "big") + data


def plaintext(exts, payload, list_len=None, payload_len=None, trailing=b""):
    body = b"".join(exts)
    ll = len(body) if list_len is None else list_len
    pl = len(payload) if payload_len is None else payload_len
    return ll.to_bytes(2, "big") + body + pl.to_bytes(4, "big") + payload + trailing


def list_of(nbytes, dup=None):
    """A valid extension list of exactly `nbytes` bytes with distinct types 1, 2, ...; `dup` =
    (i, j): item j repeats item i's type."""
    n4, odd = divmod(nbytes, 4)
    items = [ext(k + 1) for k in range(n4)]
    if odd:                       # stretch the last items' data to reach the length
        items[-1] = ext(n4, b"\x5a" * odd)
    assert sum(map(len, items)) == nbytes
    if dup:
        i, j = dup
        items[j] = items[i][:2] + items[j][2:]
    return items


def cases():
    rng = np.random.default_rng(11)
    pay = bytes(rng.integers(0, 256, WANT, dtype=np.uint8))
    out = [plaintext([], pay)]                                   # no extensions
    for k in range(1, 6):                                        # 1-5 extensions, data 0 / 1 / 7
        for dl in (0, 1, 7):
            out.append(plaintext([ext(10 + i, bytes([i]) * dl) for i in range(k)], pay))
        mixed = [ext(20 + i, b"\x01" * (0, 1, 7)[i % 3]) for i in range(k)]
        out.append(plaintext(mixed, pay))
    five = [ext(30 + i, b"\x02" * (i % 3)) for i in range(5)]
    for i, j in ((0, 1), (0, 4), (3, 4), (1, 2), (2, 4)):        # duplicate first / last / adjacent
        d = list(five)
        d[j] = d[i][:2] + d[j][2:]
        out.append(plaintext(d, pay))
    body = len(b"".join(five))
    for ll in (body + 1, body + WANT + 4, body + WANT + 5, 0xFFFF, 255, 256):   # list past the end
        out.append(plaintext(five, pay, list_len=ll))
    for ll in (body - 1, body - 2, body - 3, 3, 2, 1):           # an item running past the list
        out.append(plaintext(five, pay, list_len=ll))
    out.append(plaintext([ext(1, b"\x00" * 7)[:-3]], pay))       # data cut short by the payload
    for dpl in (-1, 1):                                          # payload length off by one
        out.append(plaintext(five, pay, payload_len=WANT + dpl))         # declared only
        out.append(plaintext(five, pay[:WANT + dpl] if dpl < 0 else pay + b"\x07"))  # real
        out.append(plaintext([], pay, payload_len=WANT + dpl))
    out.append(plaintext(five, pay, trailing=b"\x00"))           # one trailing byte
    out.append(plaintext([], pay, trailing=b"\x09"))
    for n in range(6):                                           # plaintexts of 0-5 bytes
        out.append(bytes(n))
        out.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
        out.append(plaintext([], pay)[:n])
    for nbytes in (252, 253, 254, 255, 256, 257, 258, 260, 264, 512):    # the defer boundary
        out.append(plaintext(list_of(nbytes), pay))
        out.append(plaintext(list_of(nbytes, dup=(0, nbytes // 4 - 1)), pay))
        out.append(plaintext(list_of(nbytes, dup=(nbytes // 4 - 2, nbytes // 4 - 1)), pay))
        out.append(plaintext(list_of(nbytes), pay, trailing=b"\x01"))
    out.append(plaintext([], pay, list_len=257)[:40])            # long list, short plaintext
    out.append((257).to_bytes(2, "big"))
    out.append((256).to_bytes(2, "big"))
    # random structure: valid lists with random types (collisions happen), then random damage
    while len(out) < 3000:
        k = int(rng.integers(0, 9))
        items = [ext(int(rng.integers(0, 12)), bytes(rng.integers(0, 256, int(rng.choice([0, 1, 7])),
                                                                  dtype=np.uint8)))
                 for _ in range(k)]
        pt = bytearray(plaintext(items, pay))
        what = int(rng.integers(0, 6))
        if what == 1:
            pt[int(rng.integers(0, len(pt)))] ^= 1 << int(rng.integers(0, 8))
        elif what == 2:
            pt = pt[:int(rng.integers(0, len(pt) + 1))]
        elif what == 3:
            pt += bytes(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        elif what == 4 and len(pt) > 2:
            pt[int(rng.integers(0, min(len(pt), 2 + len(b"".join(items)) + 4)))] = \
                int(rng.integers(0, 256))
        out.append(bytes(pt))
    return out


@pytest.fixture(scope="module")
def generated():
    pts = cases()
    sizes = _Sizes()
    sizes.helper_input_share = WANT
    rows, st = C.decode_plaintext_input_shares(sizes, pts, agg_id=1)
    return pts, rows, st


def _lines(pts):
    return [f"pt {WANT} {p.hex() or '-'}" for p in pts]


def _check(pts, rows, st, out):
    assert len(out) == len(pts)
    seen = {0: 0, 8: 0, DEFER: 0}
    for i, (p, line) in enumerate(zip(pts, out)):
        got, off = map(int, line.split())
        deferred = len(p) >= 2 and int.from_bytes(p[:2], "big") > MAX_LIST
        seen[got] += 1
        if deferred:
            assert got == DEFER, (i, p.hex())
            continue
        assert got == int(st[i]), (i, p.hex(), got, int(st[i]))
        if got == 0:
            assert p[off:off + WANT] == rows[i].tobytes() and off + WANT == len(p), (i, p.hex())
    assert min(seen.values()) >= 20, seen      # every outcome is exercised


def test_parser_matches_host_decode(parse_bin, generated):
    pts, rows, st = generated
    assert len(pts) >= 3000
    _check(pts, rows, st, run(parse_bin, _lines(pts)))


def test_defer_boundary(parse_bin):
    pay = bytes(WANT)
    out = run(parse_bin, _lines([plaintext(list_of(256), pay), plaintext(list_of(257), pay),
                                 plaintext(list_of(256, dup=(0, 63)), pay),
                                 plaintext(list_of(257, dup=(0, 63)), pay)]))
    assert out == [f"0 {2 + 256 + 4}", f"{DEFER} 0", "8 0", f"{DEFER} 0"]


def test_parser_under_sanitizers(parse_bin_san, generated):
    pts, rows, st = generated
    _check(pts, rows, st, run(parse_bin_san, _lines(pts)))


def test_fault_rule_matches_gather(parse_bin):
    """prepare_init_fault against prio3gpu_gather_prepare_inits' rule and apply_fault against
    prio3gpu_apply_faults."""
    want_pub, want_prep = 32, 48
    combos = [(a, b, t) for a in (0, 31, 32, 33) for b in (0, 47, 48, 49) for t in (0, 1, 2)]
    out = run(parse_bin, [f"fault {a} {b} {t} {want_pub} {want_prep}" for a, b, t in combos])
    for (a, b, t), line in zip(combos, out):
        want = 8 if a != want_pub else 5 if (t != 0 or b != want_prep) else 0
        assert int(line) == want, (a, b, t)
    pairs = [(s, f) for s in (0, 3, 4, 5, 8, DEFER, 0xFF) for f in (0, 5, 8)]
    out = run(parse_bin, [f"apply {s} {f}" for s, f in pairs])
    st = np.array([s for s, _ in pairs], np.uint8)
    C.apply_faults(st, np.array([f for _, f in pairs], np.uint8))
    assert [int(x) for x in out] == st.tolist()
