"""HPKE open on the GPU for DHKEM(P-256, HKDF-SHA256) (janus_amd/csrc/p256.h, k_p256_dh, with the
context option "hpke_gpu_p256" = 1): the six RFC 9180 P-256 vectors, the scalar multiplication
against tests/p256_model.py, every KDF x AEAD against the host implementation (hpke.cpp), the two
options, and the report-share path.  Everything is byte-exact."""
import ctypes

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import Prio3GpuError, lib
from tests import p256_model as E
from tests.test_gpu_hpke import INFO, VECTORS, _both, _flip, _host_open, _open, _request, h

pytestmark = pytest.mark.gpu

P256 = H.KEM_P256_HKDF_SHA256
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
P256_VECTORS = [v for v in VECTORS if v["kem_id"] == 0x10]


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    v.set_option("hpke_gpu_suites", 1)
    v.set_option("hpke_gpu_p256", 1)
    yield v
    v.close()


def _keypair(kdf, aead, config_id=1, kem=P256):
    return H.generate_hpke_config_and_private_key(config_id, kem, kdf, aead)


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _launches(ctx):
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    k = lib().prio3gpu_prof_read(ctx, ms, launches, 64)
    assert k > 0
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}


# ---- 1. RFC 9180 ---------------------------------------------------------------------------------
def test_golden_file_has_the_six_p256_vectors():
    assert sorted((v["kdf_id"], v["aead_id"]) for v in P256_VECTORS) == \
        [(k, a) for k in (1, 3) for a in (1, 2, 3)]


@pytest.mark.parametrize("v", P256_VECTORS, ids=lambda v: f"kdf{v['kdf_id']}-aead{v['aead_id']}")
def test_rfc9180_vector(gpu, v):
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x10, v["kdf_id"], v["aead_id"], h(v["pkRm"])),
                       h(v["skRm"]))
    info, enc, aad, ct, pt = (h(v[k]) for k in ("info", "enc", "aad", "ct", "pt"))
    pts, st = _open(gpu, kp, info, [(enc, aad, ct)])                    # alone
    assert st[0] == 0 and pts[0] == pt
    items, kinds = [], []
    for i in range(61):                                                 # one wave, tampered neighbours
        kind = ("intact", "enc", "aad", "body", "tag")[i % 5]
        kinds.append(kind)
        items.append({"intact": (enc, aad, ct),
                      "enc": (_flip(enc, (7 * i) % 520), aad, ct),
                      "aad": (enc, _flip(aad, i % (8 * len(aad))), ct),
                      "body": (enc, aad, _flip(ct, (5 * i) % (8 * (len(ct) - 16)))),
                      "tag": (enc, aad, _flip(ct, 8 * (len(ct) - 16) + (3 * i) % 128))}[kind])
    pts, st = _open(gpu, kp, info, items)
    for i, kind in enumerate(kinds):
        if kind == "intact":
            assert st[i] == 0 and pts[i] == pt, i
        else:
            assert st[i] == 4 and pts[i] == bytes(len(pt)), (i, kind)


# ---- 2. the DH hook against the model ------------------------------------------------------------
def _p256_gpu(gpu, k, encs):
    n = len(encs)
    pts = np.frombuffer(b"".join(encs) + b"\0", np.uint8).copy()
    out, ok = np.full((max(n, 1), 32), 0xAA, np.uint8), np.full(max(n, 1), 0xAA, np.uint8)
    rc = lib().prio3gpu_test_p256_gpu(gpu._ctx, k.to_bytes(32, "big"), pts.ctypes.data, n,
                                      out.ctypes.data, ok.ctypes.data)
    assert rc == 0, lib().prio3gpu_last_error()
    return [out[i].tobytes() for i in range(n)], ok[:n].tolist()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_scalar_mul_matches_model(gpu, n):
    rng = np.random.default_rng(n)
    k = E.random_scalar(rng)
    points = [E.random_point(rng) for _ in range(n)]
    xs, ok = _p256_gpu(gpu, k, [E.encode(p) for p in points])
    assert ok == [1] * n
    assert xs == [E.mul(k, p)[0].to_bytes(32, "big") for p in points]


def test_scalar_mul_edge_scalars_and_points(gpu):
    rng = np.random.default_rng(7)
    points = [E.G, *E.X0] + [E.random_point(rng) for _ in range(2)]
    for k in E.edge_scalars():
        xs, ok = _p256_gpu(gpu, k, [E.encode(p) for p in points])
        assert ok == [1] * len(points), hex(k)
        assert xs == [E.mul(k, p)[0].to_bytes(32, "big") for p in points], hex(k)


def test_all_zero_x_is_a_result_not_a_failure(gpu):
    """[k] P = (0, sqrt b) for P = [k^-1] (0, sqrt b): 32 zero bytes out with ok = 1."""
    rng = np.random.default_rng(8)
    k = E.random_scalar(rng)
    p = E.mul(pow(k, -1, E.N), E.X0[0])
    xs, ok = _p256_gpu(gpu, k, [E.encode(E.G), E.encode(p), E.encode(E.X0[1])])
    assert ok == [1, 1, 1] and xs[1] == bytes(32)
    assert xs[0] == E.mul(k, E.G)[0].to_bytes(32, "big")
    assert xs[2] == E.mul(k, E.X0[1])[0].to_bytes(32, "big")


def test_invalid_encodings_in_one_wave(gpu):
    rng = np.random.default_rng(9)
    k = E.random_scalar(rng)
    bad = E.invalid_encodings(rng)
    good = [E.random_point(rng) for _ in range(len(bad) + 1)]
    encs, want_x, want_ok = [], [], []
    for i, p in enumerate(good):                                        # good, bad, good, ...
        encs.append(E.encode(p))
        want_x.append(E.mul(k, p)[0].to_bytes(32, "big"))
        want_ok.append(1)
        if i < len(bad):
            encs.append(bad[i])
            want_x.append(bytes(32))
            want_ok.append(0)
    xs, ok = _p256_gpu(gpu, k, encs)
    assert ok == want_ok and xs == want_x


def test_hook_refuses_scalars_outside_the_group_order(gpu):
    pts = np.frombuffer(E.encode(E.G), np.uint8).copy()
    out, ok = np.zeros(32, np.uint8), np.zeros(1, np.uint8)
    L, ctx = lib(), gpu._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)
        for k in (0, E.N, E.N + 1, (1 << 256) - 1):
            rc = L.prio3gpu_test_p256_gpu(ctx, k.to_bytes(32, "big"), pts.ctypes.data, 1,
                                          out.ctypes.data, ok.ctypes.data)
            assert rc == H._E_HPKE, k
        assert sum(_launches(ctx).values()) == 0
    finally:
        L.prio3gpu_prof_enable(ctx, 0)


# ---- 3. every suite against the host -------------------------------------------------------------
PT_LENS = (0, 15, 16, 17, 257)
AAD_LENS = (0, 15, 16, 17, 257)


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_suite_matches_host(gpu, kdf, aead):
    rng = np.random.default_rng(1000 + 100 * kdf + aead)
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
    add(33, 20, lambda it: (_flip(it[0], 8 * 64 + 3), it[1], it[2]))    # off the curve
    x_is_p = b"\x04" + E.P.to_bytes(32, "big") + E.SQRT_B.to_bytes(32, "big")
    assert E.decode(x_is_p) is None
    add(33, 20, lambda it: (x_is_p, it[1], it[2]))                      # x = p
    add(17, 5)                                                          # skipped on entry
    st0 = np.zeros(len(items), np.uint8)
    st0[-1] = 8
    want[-1] = (8, bytes(17))
    assert all(s == 0 for s, _ in want[:n_ok])
    assert [s for s, _ in want[n_ok:-1]] == [4] * 5
    assert E.decode(items[n_ok + 3][0]) is None
    pts, st = _open(gpu, kp, INFO, items, status=st0)
    got = [(int(st[i]), pts[i]) for i in range(len(items))]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(items[i][1]), len(items[i][2]), g[0], w[0])


# ---- 4. the options ------------------------------------------------------------------------------
def test_options():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))                                   # a fresh context
    kp11, kp33 = _keypair(1, 1), _keypair(3, 3)
    _, enc11, ct11 = H.seal(kp11.config, INFO, b"message", b"aad")
    _, enc33, ct33 = H.seal(kp33.config, INFO, b"message", b"aad")
    L, ctx = lib(), v._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0

    def refused(kp, enc, ct):
        with pytest.raises(ValueError):
            _open(v, kp, INFO, [(enc, b"aad", ct)])
        assert sum(_launches(ctx).values()) == 0

    def opened(kp, enc, ct):
        pts, st = _open(v, kp, INFO, [(enc, b"aad", ct)])
        assert st[0] == 0 and pts[0] == b"message"
        got = _launches(ctx)
        assert got["k_p256_dh"] == 1 and got["k_hpke_open"] == 1 and got["k_x25519"] == 0
        assert sum(got.values()) == 2

    try:
        _launches(ctx)  # drain
        refused(kp11, enc11, ct11)                                      # the default context
        v.set_option("hpke_gpu_suites", 1)
        refused(kp11, enc11, ct11)                                      # that option adds no KEM
        v.set_option("hpke_gpu_suites", 0)
        v.set_option("hpke_gpu_p256", 1)
        opened(kp11, enc11, ct11)
        refused(kp33, enc33, ct33)
        v.set_option("hpke_gpu_suites", 1)
        opened(kp33, enc33, ct33)
        with pytest.raises(Prio3GpuError):
            v.set_option("hpke_gpu_p256", 2)
        opened(kp33, enc33, ct33)                                       # the refused value changed nothing
        v.set_option("hpke_gpu_p256", 0)
        refused(kp33, enc33, ct33)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
        v.close()


def test_bad_keypair_is_refused_before_any_launch(gpu):
    kp = _keypair(1, 1)
    _, enc, ct = H.seal(kp.config, INFO, b"message", b"aad")
    off_curve = H.HpkeKeypair(H.HpkeConfig(1, P256, 1, 1, _flip(kp.config.public_key, 8 * 64)),
                              kp.private_key)
    zero_sk = H.HpkeKeypair(kp.config, bytes(32))
    big_sk = H.HpkeKeypair(kp.config, E.N.to_bytes(32, "big"))
    L, ctx = lib(), gpu._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)
        for bad in (off_curve, zero_sk, big_sk):
            with pytest.raises(H.HpkeError):
                _open(gpu, bad, INFO, [(enc, b"aad", ct)])
        assert sum(_launches(ctx).values()) == 0
        for bad in (zero_sk, big_sk):                                   # the host fails the same way
            with pytest.raises(H.HpkeError):
                H.open_(bad, INFO, enc, ct, b"aad")
    finally:
        L.prio3gpu_prof_enable(ctx, 0)


# ---- 5. report shares ----------------------------------------------------------------------------
def test_report_shares_match_host(gpu):
    rng = np.random.default_rng(56)
    n = 200
    task_id = bytes(range(32))
    tkx = _keypair(1, 1, config_id=1, kem=H.KEM_X25519_HKDF_SHA256)
    tka = _keypair(1, 1, config_id=2)
    tkb = _keypair(3, 3, config_id=3)
    gk_same_id = _keypair(2, 2, config_id=2)         # shares tka's id: opened by the second trial
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = [1_700_000_000 + i for i in range(n)]
    public = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    payloads = [_rnd(rng, 48) for _ in range(n)]
    kps = [(tkx, tka, tkb, gk_same_id)[i % 4] for i in range(n)]
    kps[5] = None  # unknown config id
    req = C.decode_agg_init_req(bytearray(_request(task_id, nonces, times, public, payloads, kps)))
    v = req.views[6]
    req.raw[v.payload_off + 3] ^= 0x40  # corrupted payload (tkb)
    v = req.views[10]
    req.raw[v.enc_off + 64] ^= 0x01     # tkb's enc leaves the curve
    st0 = np.zeros(n, np.uint8)
    st0[9] = 8  # rejected by an earlier stage: skipped
    L, ctx = lib(), gpu._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)
        pts, offs, st = _both(gpu, task_id, req, [tkx, tka, tkb], [gk_same_id], st0, 4)
        got = _launches(ctx)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    assert got["k_x25519"] == 1 and got["k_p256_dh"] == 2 and got["k_hpke_open"] == 3
    assert st[5] == 3 and st[6] == 4 and st[10] == 4 and st[9] == 8
    ok = [i for i in range(n) if i not in (5, 6, 9, 10)]
    assert (st[ok] == 0).all()
    for i in ok:
        assert pts[int(offs[i]):int(offs[i + 1])].tobytes()[6:] == payloads[i]
