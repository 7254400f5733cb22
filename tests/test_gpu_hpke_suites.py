"""HPKE open on the GPU for every X25519 suite (janus_amd/csrc/hpke_gpu.h with the context option
"hpke_gpu_suites" = 1): KDF HKDF-SHA256 / -SHA384 / -SHA512 x AEAD AES-128-GCM / AES-256-GCM /
ChaCha20-Poly1305, against the RFC 9180 vectors (KDF 1 and 3) and the host implementation
(hpke.cpp; the only pin of the three SHA-384 suites).  Everything is byte-exact."""
import ctypes

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import hpke_suite_model as M
from tests.test_gpu_hpke import (INFO, VECTORS, _both, _flip, _host_open, _open, _pack, _request,
                                 h)

pytestmark = pytest.mark.gpu

SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
X25519_VECTORS = [v for v in VECTORS if v["kem_id"] == 0x20]


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    v.set_option("hpke_gpu_suites", 1)
    yield v
    v.close()


def _keypair(kdf, aead, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, H.KEM_X25519_HKDF_SHA256, kdf, aead)


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- 1. RFC 9180 ---------------------------------------------------------------------------------
def test_golden_file_has_the_six_x25519_vectors():
    assert sorted((v["kdf_id"], v["aead_id"]) for v in X25519_VECTORS) == \
        [(k, a) for k in (1, 3) for a in (1, 2, 3)]


@pytest.mark.parametrize("v", X25519_VECTORS, ids=lambda v: f"kdf{v['kdf_id']}-aead{v['aead_id']}")
def test_rfc9180_vector(gpu, v):
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x20, v["kdf_id"], v["aead_id"], h(v["pkRm"])),
                       h(v["skRm"]))
    info, enc, aad, ct, pt = (h(v[k]) for k in ("info", "enc", "aad", "ct", "pt"))
    pts, st = _open(gpu, kp, info, [(enc, aad, ct)])                    # alone
    assert st[0] == 0 and pts[0] == pt
    items, kinds = [], []
    for i in range(61):                                                 # one wave, tampered neighbours
        kind = ("intact", "enc", "aad", "body", "tag")[i % 5]
        kinds.append(kind)
        items.append({"intact": (enc, aad, ct),
                      "enc": (_flip(enc, (7 * i) % 255), aad, ct),
                      "aad": (enc, _flip(aad, i % (8 * len(aad))), ct),
                      "body": (enc, aad, _flip(ct, (5 * i) % (8 * (len(ct) - 16)))),
                      "tag": (enc, aad, _flip(ct, 8 * (len(ct) - 16) + (3 * i) % 128))}[kind])
    pts, st = _open(gpu, kp, info, items)
    for i, kind in enumerate(kinds):
        if kind == "intact":
            assert st[i] == 0 and pts[i] == pt, i
        else:
            assert st[i] == 4 and pts[i] == bytes(len(pt)), (i, kind)


# ---- 2. every suite against the host -------------------------------------------------------------
PT_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
AAD_LENS = (0, 15, 16, 17, 92)
LONG_PT_LENS = (4064, 4095, 4096, 4097, 4112)      # AES-256: the CTR counter crosses 0x100


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_suite_matches_host(gpu, kdf, aead):
    rng = np.random.default_rng(100 * kdf + aead)
    kp = _keypair(kdf, aead)
    items, want = [], []

    def add(pl, al, damage=None):
        pt, aad = _rnd(rng, pl), _rnd(rng, al)
        _, enc, ct = H.seal(kp.config, INFO, pt, aad)
        it = (enc, aad, ct)
        if damage:
            it = damage(it)
        items.append(it)
        want.append(_host_open(kp, INFO, it))

    for pl in PT_LENS:
        for al in AAD_LENS:
            add(pl, al)
    n_ok = len(items)
    for short in (0, 1, 15):                                            # shorter than a tag
        add(40, 20, lambda it: (it[0], it[1], it[2][:short]))
    add(33, 20, lambda it: (bytes(32), it[1], it[2]))                   # all-zero DH value
    if aead == 2:
        for pl in LONG_PT_LENS:
            add(pl, 20)
        add(54, 4097)
        add(54, 4097, lambda it: (it[0], _flip(it[1], 8 * 4096 + 7), it[2]))
    add(17, 5)                                                          # skipped on entry
    st0 = np.zeros(len(items), np.uint8)
    st0[-1] = 8
    want[-1] = (8, bytes(17))
    assert all(s == 0 for s, _ in want[:n_ok])
    assert [s for s, _ in want[n_ok:n_ok + 4]] == [4, 4, 4, 4]
    if aead == 2:
        assert [s for s, _ in want[n_ok + 4:-1]] == [0] * 6 + [4]
    pts, st = _open(gpu, kp, INFO, items, status=st0)
    got = [(int(st[i]), pts[i]) for i in range(len(items))]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(items[i][1]), len(items[i][2]), g[0], w[0])


# ---- 3. ragged last wave -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kdf,aead", [(2, 2), (3, 3)])
def test_batch_sizes(gpu, kdf, aead, n):
    rng = np.random.default_rng(n)
    kp = _keypair(kdf, aead)
    items, want = [], []
    for i in range(n):
        pt, aad = _rnd(rng, 20 + i % 37), _rnd(rng, i % 19)
        _, enc, ct = H.seal(kp.config, INFO, pt, aad)
        if i % 7 == 3:
            ct = _flip(ct, i)
        items.append((enc, aad, ct))
        want.append((4, bytes(len(pt))) if i % 7 == 3 else (0, pt))
    pts, st = _open(gpu, kp, INFO, items)
    assert [(int(st[i]), pts[i]) for i in range(n)] == want


# ---- 4. device pointers --------------------------------------------------------------------------
def test_device_pointers_match_host_pointers(gpu):
    rng = np.random.default_rng(33)
    kp = _keypair(3, 3)
    items = []
    for pl in PT_LENS:
        for al in AAD_LENS[::2]:
            pt, aad = _rnd(rng, pl), _rnd(rng, al)
            _, enc, ct = H.seal(kp.config, INFO, pt, aad)
            items.append((enc, aad, ct))
    items[3] = (items[3][0], items[3][1], _flip(items[3][2], 1))
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
    assert [int(x) for x in hst[:n]].count(0) == n - 2
    assert gp[:total].tobytes() == hp[:total].tobytes()
    for i, it in enumerate(items):
        got = hp[int(hoff[i]):int(hoff[i + 1])].tobytes()
        assert got == (bytes(len(it[2]) - 16) if i in (3, 10) else _host_open(kp, INFO, it)[1])


# ---- 5. Poly1305 alone ---------------------------------------------------------------------------
def test_poly1305_gpu_matches_model(gpu):
    cases = M.poly1305_cases()
    n = len(cases)
    keys = np.frombuffer(b"".join(k for k, _ in cases), np.uint8).copy()
    msgs = np.frombuffer(b"".join(m for _, m in cases) + b"\0", np.uint8).copy()
    offs = np.cumsum([0] + [len(m) for _, m in cases]).astype(np.uint64)
    tags = np.zeros((n, 16), np.uint8)
    rc = lib().prio3gpu_test_poly1305_gpu(gpu._ctx, keys.ctypes.data, msgs.ctypes.data,
                                          offs.ctypes.data, n, tags.ctypes.data)
    assert rc == 0, lib().prio3gpu_last_error()
    for i, (k, m) in enumerate(cases):
        assert tags[i].tobytes() == M.poly1305(k, m), (i, k.hex(), m.hex())
    assert tags[0].tobytes().hex() == "a8061dc1305136c6c22b8baf0c0127a9"
    assert [t.tobytes() for t in tags[-6:-3]] == M.crafted_tags_s0()
    assert [t.tobytes().hex() for t in tags[-3:]] == ["02" + "00" * 15, "ff" * 16,
                                                     "f9" + "ff" * 15]


# ---- 6. the option ---------------------------------------------------------------------------------
def _launches(ctx):
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    k = lib().prio3gpu_prof_read(ctx, ms, launches, 64)
    assert k > 0
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}


def test_default_is_unchanged_and_the_option_switches():
    from janus_amd._lib import Prio3GpuError
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))                                   # a fresh context
    kp = _keypair(3, 3)
    _, enc, ct = H.seal(kp.config, INFO, b"message", b"aad")
    L, ctx = lib(), v._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)  # drain
        with pytest.raises(ValueError):
            _open(v, kp, INFO, [(enc, b"aad", ct)])
        assert sum(_launches(ctx).values()) == 0
        v.set_option("hpke_gpu_suites", 1)
        pts, st = _open(v, kp, INFO, [(enc, b"aad", ct)])
        assert st[0] == 0 and pts[0] == b"message"
        got = _launches(ctx)
        assert got["k_x25519"] == 1 and got["k_hpke_open"] == 1
        v.set_option("hpke_gpu_suites", 0)
        with pytest.raises(ValueError):
            _open(v, kp, INFO, [(enc, b"aad", ct)])
        assert sum(_launches(ctx).values()) == 0
        with pytest.raises(Prio3GpuError):
            v.set_option("hpke_gpu_suites", 2)
        p256 = H.generate_hpke_config_and_private_key(1, H.KEM_P256_HKDF_SHA256, 1, 1)
        v.set_option("hpke_gpu_suites", 1)
        with pytest.raises(ValueError):                                 # P-256 stays on the host
            _open(v, p256, INFO, [(enc, b"aad", ct)])
        assert sum(_launches(ctx).values()) == 0
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
        v.close()


# ---- 7. report shares ------------------------------------------------------------------------------
def test_report_shares_match_host(gpu):
    rng = np.random.default_rng(55)
    n = 200
    task_id = bytes(range(32))
    tk1 = _keypair(1, 1, config_id=1)
    tk2 = _keypair(3, 3, config_id=2)
    gk = _keypair(2, 2, config_id=3)
    gk_p256 = H.generate_hpke_config_and_private_key(4, H.KEM_P256_HKDF_SHA256, 1, 2)
    gk_same_id = _keypair(3, 2, config_id=2)         # shares tk2's id: opened by the second trial
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = [1_700_000_000 + i for i in range(n)]
    public = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    payloads = [_rnd(rng, 48) for _ in range(n)]
    kps = [(tk1, tk2, gk, gk_p256, gk_same_id)[i % 5] for i in range(n)]
    kps[5] = None  # unknown config id
    req = C.decode_agg_init_req(bytearray(_request(task_id, nonces, times, public, payloads, kps)))
    v = req.views[7]
    req.raw[v.payload_off + 3] ^= 0x40  # corrupted payload
    st0 = np.zeros(n, np.uint8)
    st0[9] = 8  # rejected by an earlier stage: skipped
    L, ctx = lib(), gpu._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)
        pts, offs, st = _both(gpu, task_id, req, [tk1, tk2], [gk, gk_p256, gk_same_id], st0, 4)
        got = _launches(ctx)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    assert got["k_hpke_open"] == 3 and got["k_x25519"] == 3              # tk1, tk2 (+ its id), gk
    assert st[5] == 3 and st[7] == 4 and st[9] == 8
    ok = [i for i in range(n) if i not in (5, 7, 9)]
    assert (st[ok] == 0).all()
    for i in ok:
        assert pts[int(offs[i]):int(offs[i + 1])].tobytes()[6:] == payloads[i]
