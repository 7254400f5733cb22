"""HPKE open on the GPU (janus_amd/csrc/hpke_gpu.h: k_x25519 + k_hpke_open) for
DHKEM(X25519, HKDF-SHA256) / HKDF-SHA256 / AES-128-GCM, against the RFC 9180 A.1 vector, the
RFC 7748 vectors and the host implementation (hpke.cpp).  Everything is byte-exact."""
import ctypes
import json
import os

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import lib

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "hpke_rfc9180_vectors.json")))
h = bytes.fromhex
P = (1 << 255) - 19
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    yield v
    v.close()


def _pack(items):
    """[(enc, aad, ct)] -> the arrays of open_batch_gpu."""
    encs = np.frombuffer(b"".join(e for e, _, _ in items), np.uint8)
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    cts = np.frombuffer(b"".join(c for _, _, c in items) + b"\0", np.uint8)
    aoff = np.cumsum([0] + [len(a) for _, a, _ in items]).astype(np.uint64)
    coff = np.cumsum([0] + [len(c) for _, _, c in items]).astype(np.uint64)
    return encs, aads, aoff, cts, coff


def _open(gpu, kp, info, items, status=None):
    encs, aads, aoff, cts, coff = _pack(items)
    pts, poff, st = H.open_batch_gpu(gpu, kp, info, encs, aads, aoff, cts, coff, status=status)
    return [pts[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(len(items))], st


def _flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def _vector0():
    v = VECTORS[0]
    assert (v["kem_id"], v["kdf_id"], v["aead_id"]) == (0x20, 1, 1)
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x20, 1, 1, h(v["pkRm"])), h(v["skRm"]))
    return v, kp


# ---- 1. RFC 9180 A.1 -----------------------------------------------------------------------------
def test_rfc9180_a1_single(gpu):
    v, kp = _vector0()
    pts, st = _open(gpu, kp, h(v["info"]), [(h(v["enc"]), h(v["aad"]), h(v["ct"]))])
    assert st[0] == 0 and pts[0] == h(v["pt"])


def test_rfc9180_a1_among_tampered_neighbours(gpu):
    v, kp = _vector0()
    info, enc, aad, ct, pt = (h(v[k]) for k in ("info", "enc", "aad", "ct", "pt"))
    other = H.generate_hpke_config_and_private_key(0)
    n, items, kinds = 67, [], []
    for i in range(n):
        if i % 3 == 0:
            items.append((enc, aad, ct))
            kinds.append("intact")
            continue
        kind = ("enc", "body", "tag", "aad", "info", "key")[(i // 3 + i) % 6]
        kinds.append(kind)
        if kind == "enc":
            items.append((_flip(enc, (7 * i) % 255), aad, ct))
        elif kind == "body":
            items.append((enc, aad, _flip(ct, (5 * i) % (8 * (len(ct) - 16)))))
        elif kind == "tag":
            items.append((enc, aad, _flip(ct, 8 * (len(ct) - 16) + (3 * i) % 128)))
        elif kind == "aad":
            items.append((enc, _flip(aad, i % (8 * len(aad))), ct))
        elif kind == "info":  # sealed under an info that differs in one bit from the batch's
            _, e2, c2 = H.seal(kp.config, _flip(info, i % (8 * len(info))), pt, aad)
            items.append((e2, aad, c2))
        else:  # sealed to another key: the batch's key is the wrong one
            _, e2, c2 = H.seal(other.config, info, pt, aad)
            items.append((e2, aad, c2))
    assert set(kinds) == {"intact", "enc", "body", "tag", "aad", "info", "key"}
    pts, st = _open(gpu, kp, info, items)
    for i in range(n):
        if kinds[i] == "intact":
            assert st[i] == 0 and pts[i] == pt, i
        else:
            assert st[i] == 4 and pts[i] == bytes(len(pt)), (i, kinds[i])
    # the whole batch under a flipped info / the wrong private key: nothing opens
    for kp2, info2 in ((kp, _flip(info, 9)), (H.HpkeKeypair(kp.config, other.private_key), info)):
        pts, st = _open(gpu, kp2, info2, items[:7])
        assert (st[:7] == 4).all() and all(p == bytes(len(pt)) for p in pts)


# ---- 2. X25519 ------------------------------------------------------------------------------------
def _x25519_host(sk, points):
    n = len(points) // 32
    out = ctypes.create_string_buffer(32 * max(n, 1))
    assert lib().prio3gpu_x25519_batch(sk, points, n, out, 0) == 0
    return out.raw[:32 * n]


def _x25519_gpu(gpu, sk, points):
    n = len(points) // 32
    out = ctypes.create_string_buffer(32 * max(n, 1))
    rc = lib().prio3gpu_test_x25519_gpu(gpu._ctx, sk, points, n, out)
    assert rc == 0, lib().prio3gpu_last_error()
    return out.raw[:32 * n]


SMALL_ORDER = [  # u-coordinates of the points of order 1, 2, 4, 8 (and their non-canonical forms)
    0, 1, P - 1, P, P + 1,
    int.from_bytes(h("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"), "little"),
    int.from_bytes(h("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157"), "little"),
]
EDGE = SMALL_ORDER + [(P + 5) | (1 << 255), (1 << 255) | 9, (1 << 255) - 1, (1 << 256) - 1, 2, 9]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_x25519_matches_host_ladder(gpu, n):
    rng = np.random.default_rng(n)
    pts = rng.integers(0, 256, 32 * n, dtype=np.uint8).tobytes()
    for sk in (rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), bytes(32), b"\xff" * 32):
        assert _x25519_gpu(gpu, sk, pts) == _x25519_host(sk, pts)


def test_x25519_edge_points(gpu):
    pts = b"".join(u.to_bytes(32, "little") for u in EDGE)
    rng = np.random.default_rng(2)
    for sk in (rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), bytes(32), b"\xff" * 32):
        got, want = _x25519_gpu(gpu, sk, pts), _x25519_host(sk, pts)
        assert got == want
        assert got[:32 * len(SMALL_ORDER)] == bytes(32 * len(SMALL_ORDER))  # small order: zero
        assert any(got[32 * len(SMALL_ORDER):])


def test_x25519_rfc7748_vectors(gpu):
    k1 = h("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
    u1 = h("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    r1 = "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    k2 = h("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d")
    u2 = h("e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493")
    r2 = "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"
    assert _x25519_gpu(gpu, k1, u1 * 3).hex() == r1 * 3
    assert _x25519_gpu(gpu, k2, u2 * 2).hex() == r2 * 2
    nine = (9).to_bytes(32, "little")  # the iterated test, first iteration: k = u = 9
    assert _x25519_gpu(gpu, nine, nine).hex() == \
        "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"


# ---- 3. length sweep ------------------------------------------------------------------------------
PT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 54, 255, 256, 257)
AAD_LENS = (0, 1, 15, 16, 17, 92)


def _sweep(kp):
    rng = np.random.default_rng(3)
    items, want = [], []
    for al in AAD_LENS:
        for pl in PT_LENS:
            pt = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
            aad = rng.integers(0, 256, al, dtype=np.uint8).tobytes()
            _, enc, ct = H.seal(kp.config, INFO, pt, aad)
            items.append((enc, aad, ct))
            want.append(pt)
    return items, want


def test_length_sweep(gpu):
    kp = H.generate_hpke_config_and_private_key(1)
    items, want = _sweep(kp)
    pts, st = _open(gpu, kp, INFO, items)
    assert (st[:len(items)] == 0).all()
    assert pts == want


# ---- 3a. short ciphertexts, long plaintexts -------------------------------------------------------
def _host_open(kp, info, item):
    """(status, plaintext) of the host implementation (hpke.cpp) for one (enc, aad, ct)."""
    enc, aad, ct = item
    try:
        return 0, H.open_(kp, info, enc, ct, aad)
    except H.HpkeError:
        return 4, bytes(max(0, len(ct) - 16))


SHORT_CT_LENS = (0, 1, 15)


def _short_items(kp, rng):
    """Ciphertexts shorter than a tag (0, 1, 15 bytes), the shortest valid one (16 bytes: the tag
    of an empty plaintext) and 16 bytes that are no valid tag, each between intact neighbours."""
    def sealed(pl):
        pt = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
        aad = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
        _, enc, ct = H.seal(kp.config, INFO, pt, aad)
        return (enc, aad, ct), pt
    items, want = [], []
    for kind in SHORT_CT_LENS + ("empty", "badtag"):
        it, pt = sealed(33)
        items.append(it)
        want.append((0, pt))
        if kind == "empty":
            it, pt = sealed(0)
            assert len(it[2]) == 16
            items.append(it)
            want.append((0, b""))
        elif kind == "badtag":
            (enc, aad, ct), _ = sealed(0)
            items.append((enc, aad, _flip(ct, 77)))
            want.append((4, b""))
        else:
            (enc, aad, ct), _ = sealed(40)
            items.append((enc, aad, ct[:kind]))
            want.append((4, b""))
    it, pt = sealed(17)
    return items + [it], want + [(0, pt)]


def test_short_ciphertexts(gpu):
    kp = H.generate_hpke_config_and_private_key(1)
    items, want = _short_items(kp, np.random.default_rng(31))
    assert [len(it[2]) for it in items[1::2]] == [0, 1, 15, 16, 16]
    host = [_host_open(kp, INFO, it) for it in items]
    assert host == want
    pts, st = _open(gpu, kp, INFO, items)
    assert [(int(st[i]), pts[i]) for i in range(len(items))] == want
    # the short ones first and last in the batch, and alone
    for order in (items[1::2] + items[0::2], items[0::2] + items[1::2], items[1:2], items[5:6]):
        pts, st = _open(gpu, kp, INFO, order)
        assert [(int(st[i]), pts[i]) for i in range(len(order))] == \
            [_host_open(kp, INFO, it) for it in order]


def test_short_ciphertexts_in_report_shares(gpu):
    rng = np.random.default_rng(32)
    task_id = bytes(range(1, 33))
    tk = H.generate_hpke_config_and_private_key(1)
    lens = [48, 0, 48, 1, 48, 15, 48, 16, 48]  # payload lengths; 16 = the tag of an empty plaintext
    n = len(lens)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = [1_700_000_000 + i for i in range(n)]
    public = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cts, pts_want = [], []
    for i, ln in enumerate(lens):
        aad = H.input_share_aad(task_id, nonces[i].tobytes(), times[i], public[i].tobytes())
        pt = rng.integers(0, 256, 32 if ln == 48 else 0, dtype=np.uint8).tobytes()
        cid, enc, ct = H.seal(tk.config, INFO, pt if ln >= 16 else bytes(24), aad)
        cts.append((cid, enc, ct[:ln] if ln < 16 else ct))
        assert len(cts[-1][2]) == ln
        pts_want.append(pt)
    req = C.decode_agg_init_req(bytearray(C.encode_agg_init_req(
        C.TIME_INTERVAL, None, b"", nonces, times, public, cts, np.zeros((n, 4), np.uint8))))
    pts, offs, st = _both(gpu, task_id, req, [tk], [], np.zeros(n, np.uint8), 2)
    assert st.tolist() == [0, 4, 0, 4, 0, 4, 0, 0, 0]
    assert np.diff(offs.astype(np.int64)).tolist() == [max(0, ln - 16) for ln in lens]
    for i in range(n):
        if st[i] == 0:
            assert pts[int(offs[i]):int(offs[i + 1])].tobytes() == pts_want[i], i


LONG_PT_LENS = (4064, 4080, 4081, 4112)  # 254 .. 257 blocks: CTR counters 2 .. 258 cross 0x100


def test_long_plaintexts_and_aad(gpu):
    kp = H.generate_hpke_config_and_private_key(1)
    rng = np.random.default_rng(33)
    items, want = [], []
    for pl, al in [(pl, 20) for pl in LONG_PT_LENS] + [(54, 4097), (4081, 4097)]:
        pt = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
        aad = rng.integers(0, 256, al, dtype=np.uint8).tobytes()
        _, enc, ct = H.seal(kp.config, INFO, pt, aad)
        items.append((enc, aad, ct))
        want.append(pt)
    assert [_host_open(kp, INFO, it) for it in items] == [(0, pt) for pt in want]
    pts, st = _open(gpu, kp, INFO, items)
    assert (st[:len(items)] == 0).all()
    assert pts == want
    # one flipped bit in the last block of the body (and, for the long AAD, in its last byte)
    bad = []
    for (enc, aad, ct), pt in zip(items, want):
        bad.append((enc, aad, _flip(ct, 8 * (len(pt) - 1) + 3)))
    bad.append((items[4][0], _flip(items[4][1], 8 * 4096 + 5), items[4][2]))
    mixed = [x for pair in zip(bad, items + items[:1]) for x in pair]  # bad, intact, bad, ...
    pts, st = _open(gpu, kp, INFO, mixed)
    assert st[:len(mixed)].tolist() == [4, 0] * len(bad)
    assert [_host_open(kp, INFO, it)[0] for it in mixed] == [4, 0] * len(bad)
    for i, it in enumerate(mixed):
        assert pts[i] == (bytes(len(it[2]) - 16) if i % 2 == 0 else (want + want[:1])[i // 2]), i


# ---- 4. report shares, GPU == host ----------------------------------------------------------------
def _request(task_id, nonces, times, public, payloads, keypairs, prep_share_len=4):
    n = len(nonces)
    cts = []
    for i in range(n):
        pt = b"\x00\x00" + len(payloads[i]).to_bytes(4, "big") + payloads[i]
        aad = H.input_share_aad(task_id, nonces[i].tobytes(), times[i], public[i].tobytes())
        kp = keypairs[i]
        cts.append(H.seal(kp.config, INFO, pt, aad) if kp else (99, b"\x01" * 32, b"\x02" * 40))
    lps = np.zeros((n, prep_share_len), np.uint8)
    return C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", nonces, times, public, cts, lps)


def _both(gpu, task_id, req, tks, gks, st0, threads):
    a = H.open_report_shares(task_id, req, tks, gks, st0.copy(), threads=threads)
    b = H.open_report_shares(task_id, req, tks, gks, st0.copy(), threads=threads, gpu=gpu)
    assert a[1].tolist() == b[1].tolist()      # offsets
    assert a[2].tolist() == b[2].tolist()      # statuses
    for i in np.flatnonzero(a[2] == 0):
        lo, hi = int(a[1][i]), int(a[1][i + 1])
        assert a[0][lo:hi].tobytes() == b[0][lo:hi].tobytes(), i
    return b


def test_report_shares_match_host(gpu):
    rng = np.random.default_rng(5)
    n = 200
    task_id = bytes(range(32))
    tk = H.generate_hpke_config_and_private_key(1)
    gk = H.generate_hpke_config_and_private_key(2, H.KEM_P256_HKDF_SHA256, 1, 2)
    gk_same_id = H.generate_hpke_config_and_private_key(1)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = [1_700_000_000 + i for i in range(n)]
    public = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    payloads = [bytes(rng.integers(0, 256, 48, dtype=np.uint8)) for _ in range(n)]
    kps = [tk if i % 3 == 0 else gk if i % 3 == 1 else gk_same_id for i in range(n)]
    kps[5] = None  # unknown config id
    req = C.decode_agg_init_req(bytearray(_request(task_id, nonces, times, public, payloads, kps)))
    v = req.views[7]
    req.raw[v.payload_off + 3] ^= 0x40  # corrupted payload
    st0 = np.zeros(n, np.uint8)
    st0[9] = 8  # rejected by an earlier stage: skipped
    pts, offs, st = _both(gpu, task_id, req, [tk], [gk, gk_same_id], st0, 4)
    assert st[5] == 3 and st[7] == 4 and st[9] == 8
    ok = [i for i in range(n) if i not in (5, 7, 9)]
    assert (st[ok] == 0).all()
    for i in ok:
        assert pts[int(offs[i]):int(offs[i + 1])].tobytes()[6:] == payloads[i]
    # no global keys: gk's reports have an unknown id, gk_same_id's fail to decrypt
    _, _, st2 = _both(gpu, task_id, req, [tk], [], np.zeros(n, np.uint8), 1)
    assert all(st2[i] == 3 for i in range(n) if i % 3 == 1 and i != 7)
    assert all(st2[i] == 4 for i in range(n) if i % 3 == 2 and i != 5)
    # a wrong task id changes the AAD: every open fails
    _, _, st3 = _both(gpu, bytes(32), req, [tk], [gk, gk_same_id], np.zeros(n, np.uint8), 0)
    assert set(st3.tolist()) == {3, 4}
    # the sizing call fills the offsets and touches nothing else
    tkc, keep = H._keypairs([tk])
    tid = np.frombuffer(task_id, np.uint8).copy()
    offs2 = np.zeros(n + 1, np.uint64)
    rc = lib().prio3gpu_hpke_open_report_shares_gpu(
        gpu._ctx, tid.ctypes.data, tkc, 1, None, 0, H.ROLE_CLIENT, H.ROLE_HELPER,
        req.raw.ctypes.data, req.views, n, None, offs2.ctypes.data, None, 1)
    assert rc == 0 and offs2.tolist() == offs.tolist()
    del keep


def test_report_shares_empty_request(gpu):
    empty = C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", np.zeros((0, 16), np.uint8), [],
                                  np.zeros((0, 32), np.uint8), [], np.zeros((0, 4), np.uint8))
    req = C.decode_agg_init_req(empty)
    pts, offs, st = H.open_report_shares(bytes(32), req,
                                         [H.generate_hpke_config_and_private_key(1)], gpu=gpu)
    assert offs.tolist() == [0] and st.size == 0


# ---- 5. device pointers ---------------------------------------------------------------------------
def test_device_pointers_match_host_pointers(gpu):
    kp = H.generate_hpke_config_and_private_key(1)
    items, want = _sweep(kp)
    items[3] = (items[3][0], items[3][1], _flip(items[3][2], 1))  # one failure among them
    encs, aads, aoff, cts, coff = _pack(items)
    n = len(items)
    st0 = np.zeros(n, np.uint8)
    st0[10] = 8
    hp, hoff, hst = H.open_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff, status=st0.copy())
    L, ctx = lib(), gpu._ctx
    dev = []

    def up(a):
        p = ctypes.c_void_p()
        assert L.prio3gpu_dev_alloc(ctx, max(a.nbytes, 16), ctypes.byref(p)) == 0
        assert L.prio3gpu_memcpy(ctx, p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    try:
        d = [up(a) for a in (encs, aads, aoff, cts, coff)]
        dpts = up(np.full(hp.size, 0xAA, np.uint8))
        dpoff, dst = up(np.ascontiguousarray(hoff, np.uint64)), up(st0)
        H.open_batch_gpu(gpu, kp, INFO, d[0], d[1], d[2], d[3], d[4], pts=dpts, pt_offsets=dpoff,
                         status=dst, n=n)
        gp, gst = np.zeros_like(hp), np.zeros_like(hst)
        assert L.prio3gpu_memcpy(ctx, gp.ctypes.data, dpts, gp.nbytes) == 0
        assert L.prio3gpu_memcpy(ctx, gst.ctypes.data, dst, n) == 0
    finally:
        for p in dev:
            L.prio3gpu_dev_free(ctx, p)
    total = int(hoff[-1])
    assert gst[:n].tolist() == hst[:n].tolist() and hst[3] == 4 and hst[10] == 8
    assert gp[:total].tobytes() == hp[:total].tobytes()
    for i in range(n):
        got = hp[int(hoff[i]):int(hoff[i + 1])].tobytes()
        assert got == (bytes(len(want[i])) if i in (3, 10) else want[i])


# ---- 6. driver ------------------------------------------------------------------------------------
def test_helper_driver_gpu_hpke_matches_host():
    from janus_amd.helper import HelperAggregateInit
    from janus_amd.prio3 import Prio3Gpu
    from tests.reports import CONFIGS, expected_aggregate, make_batch
    name = "sumvec_small"
    b = make_batch(name, 24)
    c = CONFIGS[name]
    v = Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                 chunk_length=c["chunk"])
    ls = v.new_state(0, b.n)
    lp, _ = v.prepare_init(ls, b.nonces, b.public, b.leader_in)
    task_id = os.urandom(32)
    tk = H.generate_hpke_config_and_private_key(3)
    times = list(range(1000, 1000 + b.n))
    cts = []
    for r in range(b.n):
        pt = b"\x00\x00" + len(b.helper_in[r]).to_bytes(4, "big") + b.helper_in[r].tobytes()
        aad = H.input_share_aad(task_id, b.nonces[r].tobytes(), times[r], b.public[r].tobytes())
        cts.append(H.seal(tk.config, INFO, pt, aad))
    cts[4] = (9, cts[4][1], cts[4][2])  # unknown config id
    cts[13] = (cts[13][0], cts[13][1], cts[13][2][:-1] + b"\x00")  # bad tag
    jobs = [slice(0, 8), slice(8, 16), slice(16, 24)]
    reqs = [C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", b.nonces[j], times[j], b.public[j],
                                  cts[j], lp[j]) for j in jobs]
    out = {}
    for mode in ("host", "gpu"):
        drv = HelperAggregateInit(v, task_id, [tk], hpke_threads=4, hpke=mode)
        hagg = v.new_aggregate(1)
        resps = drv.handle_jobs(reqs, hagg)
        st = np.zeros(b.n, np.uint8)
        for j, resp in zip(jobs, resps):
            _, st[j] = C.gather_helper_resps(v.sizes, resp, b.nonces[j], np.zeros(8, np.uint8))
        out[mode] = ([bytes(r) for r in resps], st.tolist(), hagg.read(0))
        drv.close()
    assert out["gpu"] == out["host"]
    st = np.array(out["gpu"][1])
    assert st[4] == 3 and st[13] == 4 and (np.delete(st, [4, 13]) == 0).all()
    exp, ecnt = expected_aggregate(b, "helper", mask=st == 0)
    got, cnt = out["gpu"][2]
    assert got == exp and cnt == ecnt == b.n - 2


# ---- 7. unsupported suite -------------------------------------------------------------------------
@pytest.mark.parametrize("suite", [(0x20, 1, 2), (0x20, 1, 3), (0x20, 2, 1), (0x10, 1, 1)])
def test_unsupported_suite_launches_nothing(gpu, suite):
    kp = H.generate_hpke_config_and_private_key(1, *suite)
    _, enc, ct = H.seal(kp.config, INFO, b"message", b"aad")
    L, ctx = lib(), gpu._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        with pytest.raises(ValueError):
            _open(gpu, kp, INFO, [(enc[:32].ljust(32, b"\0"), b"aad", ct)])
        assert L.prio3gpu_prof_read(ctx, ms, launches, 64) > 0
        assert sum(launches) == 0
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
