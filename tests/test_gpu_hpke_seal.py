"""Batched HPKE seal on the GPU (janus_amd/csrc/hpke_seal_gpu.h, prio3gpu_hpke_seal_batch) for
every DHKEM(X25519, HKDF-SHA256) suite: RFC 9180 A.1.1's bytes under its own ephemeral key, and the
host implementation (hpke.cpp) under fixed ephemeral keys.  Everything is byte-exact."""
import ctypes
import json
import os

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "hpke_rfc9180_vectors.json")))
h = bytes.fromhex
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
SK_EM = h("52c4a758a802cd8b936eceea314432798d5baf2d7e9235dc084ab1b9cfa2f736")  # RFC 9180 A.1.1
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    yield v
    v.close()


@pytest.fixture(scope="module")
def gpu_wide():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    v.set_option("hpke_gpu_suites", 1)
    yield v
    v.close()


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _pack(items):
    """[(sk_e, aad, pt)] -> sk_es, aads, aad_offsets, pts, pt_offsets of seal_batch_gpu."""
    sk = np.frombuffer(b"".join(s for s, _, _ in items) + b"\0", np.uint8)[:-1]
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    pts = np.frombuffer(b"".join(p for _, _, p in items) + b"\0", np.uint8)
    return (sk, aads, _offsets([len(a) for _, a, _ in items]), pts,
            _offsets([len(p) for _, _, p in items]))


def _seal(gpu, config, info, items, **kw):
    """-> ([(enc, ct)], status)"""
    encs, cts, coff, st = H.seal_batch_gpu(gpu, config, info, *_pack(items), **kw)
    return [(encs[32 * i:32 * i + 32].tobytes(), cts[int(coff[i]):int(coff[i + 1])].tobytes())
            for i in range(len(items))], st


def _config(kdf, aead, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, H.KEM_X25519_HKDF_SHA256, kdf, aead)


def _vector0():
    v = VECTORS[0]
    assert (v["kem_id"], v["kdf_id"], v["aead_id"]) == (0x20, 1, 1)
    assert H.public_key(0x20, SK_EM) == h(v["enc"])
    return v, H.HpkeConfig(0, 0x20, 1, 1, h(v["pkRm"]))


# ---- 1. known answer -----------------------------------------------------------------------------
def test_rfc9180_a1_single(gpu):
    v, cfg = _vector0()
    got, st = _seal(gpu, cfg, h(v["info"]), [(SK_EM, h(v["aad"]), h(v["pt"]))])
    assert st[0] == 0 and got[0] == (h(v["enc"]), h(v["ct"]))


def test_rfc9180_a1_among_random_neighbours(gpu):
    v, cfg = _vector0()
    info = h(v["info"])
    rng = np.random.default_rng(9180)
    items = [(_rnd(rng, 32), _rnd(rng, i % 23), _rnd(rng, 7 + i % 41)) for i in range(67)]
    at = (0, 63, 64, 66)
    for i in at:
        items[i] = (SK_EM, h(v["aad"]), h(v["pt"]))
    got, st = _seal(gpu, cfg, info, items)
    assert not st[:67].any()
    for i, (sk_e, aad, pt) in enumerate(items):
        if i in at:
            assert got[i] == (h(v["enc"]), h(v["ct"])), i
        else:
            assert got[i] == H.seal(cfg, info, pt, aad, ephemeral_private_key=sk_e)[1:], i


# ---- 2. all nine suites --------------------------------------------------------------------------
PT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 54, 255, 4112)
AAD_LENS = (0, 7, 16, 57, 61, 100)


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_suite_matches_host(gpu, gpu_wide, kdf, aead):
    n = 130
    rng = np.random.default_rng(100 * kdf + aead)
    kp = _config(kdf, aead)
    items = [(_rnd(rng, 32), _rnd(rng, AAD_LENS[i % len(AAD_LENS)]),
              _rnd(rng, PT_LENS[i % len(PT_LENS)])) for i in range(n)]
    got, st = _seal(gpu, kp.config, INFO, items)
    assert not st[:n].any()
    for i, (sk_e, aad, pt) in enumerate(items):
        _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
        assert got[i] == (enc, ct), (i, len(aad), len(pt))
        assert H.open_(kp, INFO, got[i][0], got[i][1], aad) == pt, i
    encs = np.frombuffer(b"".join(e for e, _ in got), np.uint8)
    cts = np.frombuffer(b"".join(c for _, c in got), np.uint8)
    _, aads, aoff, _, poff = _pack(items)
    pts, ooff, ost = H.open_batch_gpu(gpu_wide, kp, INFO, encs, aads, aoff, cts,
                                      _offsets([len(c) for _, c in got]))
    assert not ost[:n].any() and ooff.tolist() == poff.tolist()
    assert pts[:int(ooff[-1])].tobytes() == b"".join(p for _, _, p in items)


# ---- 3. edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_boundary(gpu, n):
    rng = np.random.default_rng(n)
    kp = _config(1, 1)
    items = [(_rnd(rng, 32), _rnd(rng, i % 19), _rnd(rng, 20 + i % 37)) for i in range(n)]
    got, st = _seal(gpu, kp.config, INFO, items)
    assert not st[:n].any()
    # the host seal of every report would take seconds: the first and last waves, and a sample
    for i in sorted(set(range(min(n, 8))) | set(range(max(0, n - 70), n)) | set(range(0, n, 17))):
        sk_e, aad, pt = items[i]
        assert got[i] == H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:], i
    for i, (_, aad, pt) in enumerate(items):
        assert H.open_(kp, INFO, got[i][0], got[i][1], aad) == pt, i


def test_empty_batch(gpu):
    kp = _config(1, 1)
    z8, z64 = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    rc = lib().prio3gpu_hpke_seal_batch(gpu._ctx, 0x20, 1, 1, kp.config.public_key, 32, INFO,
                                        len(INFO), 0, z8.ctypes.data, z8.ctypes.data,
                                        z64.ctypes.data, z8.ctypes.data, z64.ctypes.data,
                                        z8.ctypes.data, z8.ctypes.data, z64.ctypes.data,
                                        z8.ctypes.data)
    assert rc == 0
    assert lib().prio3gpu_hpke_seal_batch(gpu._ctx, 0x20, 1, 1, kp.config.public_key, 32, INFO,
                                          len(INFO), 0, None, None, None, None, None, None, None,
                                          None, None) == 0


# ---- 4. status and slots -------------------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", [(1, 1), (3, 3)])
def test_status_and_slots(gpu, kdf, aead):
    rng = np.random.default_rng(44 + aead)
    kp = _config(kdf, aead)
    n = 70
    items = [(_rnd(rng, 32), _rnd(rng, 20), _rnd(rng, 10 + i % 30)) for i in range(n)]
    slot = [len(pt) + 16 for _, _, pt in items]
    slot[5] -= 1        # one byte short
    slot[9] += 13       # longer: zero-filled past the tag
    slot[65] += 1
    coff = _offsets(slot)
    st0 = np.zeros(n, np.uint8)
    st0[3] = 8          # skipped on entry
    st0[64] = 3
    cts = np.full(int(coff[-1]), 0xAA, np.uint8)
    encs = np.full(32 * n, 0xAA, np.uint8)
    got, st = _seal(gpu, kp.config, INFO, items, status=st0, encs=encs, cts=cts, ct_offsets=coff)
    want_st = [0] * n
    want_st[3], want_st[64], want_st[5] = 8, 3, 4
    assert st[:n].tolist() == want_st
    for i, (sk_e, aad, pt) in enumerate(items):
        if want_st[i]:
            assert got[i] == (bytes(32), bytes(slot[i])), i
        else:
            _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert got[i] == (enc, ct + bytes(slot[i] - len(ct))), i


def test_small_order_public_key(gpu):
    rng = np.random.default_rng(7)
    cfg = H.HpkeConfig(1, 0x20, 1, 1, bytes(32))
    items = [(_rnd(rng, 32), _rnd(rng, 9), _rnd(rng, 1 + i)) for i in range(66)]
    with pytest.raises(H.HpkeError):
        H.seal(cfg, INFO, items[0][2], items[0][1], ephemeral_private_key=items[0][0])
    got, st = _seal(gpu, cfg, INFO, items)
    assert st[:66].tolist() == [4] * 66
    assert got == [(bytes(32), bytes(len(pt) + 16)) for _, _, pt in items]


def test_argument_errors(gpu):
    kp = _config(1, 1)
    p256 = H.generate_hpke_config_and_private_key(1, H.KEM_P256_HKDF_SHA256, 1, 1)
    sk, aads, aoff, pts, poff = _pack([(bytes(range(32)), b"aad", b"message")])
    encs, cts, st = np.zeros(32, np.uint8), np.zeros(7 + 16, np.uint8), np.zeros(1, np.uint8)
    coff = _offsets([7 + 16])

    def call(kem, kdf, aead, pk, pk_len):
        return lib().prio3gpu_hpke_seal_batch(
            gpu._ctx, kem, kdf, aead, pk, pk_len, INFO, len(INFO), 1, sk.ctypes.data,
            aads.ctypes.data, aoff.ctypes.data, pts.ctypes.data, poff.ctypes.data,
            encs.ctypes.data, cts.ctypes.data, coff.ctypes.data, st.ctypes.data)

    L, ctx = lib(), gpu._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        assert call(0x10, 1, 1, p256.config.public_key, 65) == E_UNSUPPORTED
        assert call(0x20, 4, 1, kp.config.public_key, 32) == E_UNSUPPORTED
        assert call(0x20, 1, 4, kp.config.public_key, 32) == E_UNSUPPORTED
        assert call(0x20, 1, 1, kp.config.public_key, 31) == E_ARG
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        assert sum(launches[i] for i in range(k)) == 0          # nothing launched
        assert call(0x20, 1, 1, kp.config.public_key, 32) == 0
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        names = {L.prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}
        assert names["k_x25519_eph"] == 1 and names["k_hpke_seal"] == 1
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    assert encs.any() and st[0] == 0
    with pytest.raises(ValueError):
        H.seal_batch_gpu(gpu, p256.config, INFO, sk, aads, aoff, pts, poff)


# ---- 5. device pointers --------------------------------------------------------------------------
def test_device_tensors_match_host_arrays(gpu):
    import torch
    rng = np.random.default_rng(33)
    kp = _config(3, 2)
    items = [(_rnd(rng, 32), _rnd(rng, AAD_LENS[i % len(AAD_LENS)]),
              _rnd(rng, PT_LENS[i % len(PT_LENS)])) for i in range(70)]
    n = len(items)
    sk, aads, aoff, pts, poff = _pack(items)
    st0 = np.zeros(n, np.uint8)
    st0[10] = 8
    hencs, hcts, hcoff, hst = H.seal_batch_gpu(gpu, kp.config, INFO, sk, aads, aoff, pts, poff,
                                               status=st0.copy())
    dev = torch.device("cuda", 0)

    def up(a):
        a = np.array(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    d_encs = torch.full((32 * n,), 0xAA, dtype=torch.uint8, device=dev)
    d_cts = torch.full((int(hcoff[-1]),), 0xAA, dtype=torch.uint8, device=dev)
    d_st = up(st0)
    torch.cuda.synchronize()
    H.seal_batch_gpu(gpu, kp.config, INFO, up(sk), up(aads), up(aoff), up(pts), up(poff),
                     status=d_st, encs=d_encs, cts=d_cts, ct_offsets=up(hcoff), n=n)
    assert d_st.cpu().numpy().tolist() == hst[:n].tolist() and hst[10] == 8
    assert d_encs.cpu().numpy().tobytes() == hencs[:32 * n].tobytes()
    assert d_cts.cpu().numpy().tobytes() == hcts[:int(hcoff[-1])].tobytes()
    for i, (sk_e, aad, pt) in enumerate(items):
        if i != 10:
            _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert hencs[32 * i:32 * i + 32].tobytes() == enc
            assert hcts[int(hcoff[i]):int(hcoff[i + 1])].tobytes() == ct
