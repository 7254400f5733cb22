"""Batched HPKE seal of long plaintexts on the GPU, a wave per report
(janus_amd/csrc/hpke_seal_team.h, prio3gpu_hpke_seal_long_batch) for DHKEM(X25519, HKDF-SHA256) with
every KDF and AES-128-GCM / AES-256-GCM: RFC 9180 A.1.1's bytes under its own ephemeral key, the host
implementation (hpke.cpp) and the lane-per-report seal under fixed ephemeral keys, and the round trip
through the wave-per-report open.  Everything is byte-exact."""
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
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
SK_EM = h("52c4a758a802cd8b936eceea314432798d5baf2d7e9235dc084ab1b9cfa2f736")  # RFC 9180 A.1.1
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2)]
PT_LENS = (0, 1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4101)
AAD_LENS = (0, 60, 92)
E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    yield v
    v.close()


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _pack(items):
    """[(sk_e, aad, pt)] -> sk_es, aads, aad_offsets, pts, pt_offsets of seal_long_batch_gpu."""
    sk = np.frombuffer(b"".join(s for s, _, _ in items) + b"\0", np.uint8)[:-1]
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    pts = np.frombuffer(b"".join(p for _, _, p in items) + b"\0", np.uint8)
    return (sk, aads, _offsets([len(a) for _, a, _ in items]), pts,
            _offsets([len(p) for _, _, p in items]))


def _split(n, encs, cts, coff):
    return [(encs[32 * i:32 * i + 32].tobytes(), cts[int(coff[i]):int(coff[i + 1])].tobytes())
            for i in range(n)]


def _seal(gpu, config, info, items, fn=None, **kw):
    """-> ([(enc, ct)], status)"""
    encs, cts, coff, st = (fn or H.seal_long_batch_gpu)(gpu, config, info, *_pack(items), **kw)
    return _split(len(items), encs, cts, coff), st


def _keypair(kdf, aead, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, H.KEM_X25519_HKDF_SHA256, kdf, aead)


def _mixed(seed):
    """48 reports: every plaintext length under the AAD lengths in turn, fixed ephemeral keys."""
    rng = np.random.default_rng(seed)
    return [(_rnd(rng, 32), _rnd(rng, AAD_LENS[(j + j // len(PT_LENS)) % 3]), _rnd(rng, pl))
            for j, pl in enumerate(PT_LENS * 3)]


def _vector0():
    v = VECTORS[0]
    assert (v["kem_id"], v["kdf_id"], v["aead_id"]) == (0x20, 1, 1)
    assert H.public_key(0x20, SK_EM) == h(v["enc"])
    return v, H.HpkeConfig(0, 0x20, 1, 1, h(v["pkRm"]))


def _profile(gpu):
    """A context manager's worth in one function: (read) where read() -> {kernel name: launches}
    since the last read; profiling is on until off() is called."""
    L, ctx = lib(), gpu._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0

    def read():
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        return {L.prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}

    read()  # drain
    return read, lambda: L.prio3gpu_prof_enable(ctx, 0)


# ---- 1. known answer -----------------------------------------------------------------------------
def test_rfc9180_a1_alone_first_and_last(gpu):
    v, cfg = _vector0()
    info, kat = h(v["info"]), (SK_EM, h(v["aad"]), h(v["pt"]))
    got, st = _seal(gpu, cfg, info, [kat])
    assert st[0] == 0 and got[0] == (h(v["enc"]), h(v["ct"]))
    rng = np.random.default_rng(91)
    others = [(_rnd(rng, 32), _rnd(rng, 7), _rnd(rng, pl)) for pl in (1025, 0, 4101)]
    got, st = _seal(gpu, cfg, info, [kat] + others + [kat])           # report 0 and report 4 of 5
    assert (st[:5] == 0).all()
    assert got[0] == got[4] == (h(v["enc"]), h(v["ct"]))
    for (sk_e, aad, pt), g in zip(others, got[1:4]):
        assert g == H.seal(cfg, info, pt, aad, ephemeral_private_key=sk_e)[1:]


# ---- 2. every suite, mixed lengths ---------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", SUITES)
def test_mixed_lengths_equal_host_and_lane_seal_and_open_again(gpu, kdf, aead):
    kp = _keypair(kdf, aead)
    items = _mixed(100 * kdf + aead)
    n = len(items)
    encs, cts, coff, st = H.seal_long_batch_gpu(gpu, kp.config, INFO, *_pack(items))
    assert (st[:n] == 0).all()
    got = _split(n, encs, cts, coff)
    for (sk_e, aad, pt), g in zip(items, got):
        assert g == H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:], len(pt)
    lane, lst = _seal(gpu, kp.config, INFO, items, fn=H.seal_batch_gpu)
    assert (lst[:n] == 0).all() and got == lane
    _, aads, aoff, _, poff = _pack(items)
    pts, ooff, ost = H.open_long_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff)
    assert (ost[:n] == 0).all() and ooff.tolist() == poff.tolist()
    assert pts[:int(ooff[-1])].tobytes() == b"".join(p for _, _, p in items)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_reports_per_block_boundary(gpu, n):
    kp = _keypair(1, 1)
    items = _mixed(n)[11:11 + n]                        # 1040, 2047, 2048, 2049, 4101
    got, st = _seal(gpu, kp.config, INFO, items)
    assert (st[:n] == 0).all()
    for (sk_e, aad, pt), g in zip(items, got):
        assert g == H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:], len(pt)


# ---- 3. statuses, slots, offsets -----------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", [(1, 1), (3, 2)])
def test_status_and_slots(gpu, kdf, aead):
    rng = np.random.default_rng(44 + aead)
    kp = _keypair(kdf, aead)
    lens = (1025, 33, 40, 2049, 1024, 17, 70, 0, 16)
    n = len(lens)
    items = [(_rnd(rng, 32), _rnd(rng, 60), _rnd(rng, pl)) for pl in lens]
    slot = [pl + 16 for pl in lens]
    slot[4] -= 1        # one byte short
    slot[3] += 100      # longer: zero-filled past the tag
    slot[6] += 1
    coff = _offsets(slot)
    st0 = np.zeros(n, np.uint8)
    st0[1] = 9          # skipped on entry
    st0[8] = 3
    cts = np.full(int(coff[-1]), 0xAA, np.uint8)
    encs = np.full(32 * n, 0xAA, np.uint8)
    got, st = _seal(gpu, kp.config, INFO, items, status=st0, encs=encs, cts=cts, ct_offsets=coff)
    want_st = [0, 9, 0, 0, 4, 0, 0, 0, 3]
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
    items = [(_rnd(rng, 32), _rnd(rng, 9), _rnd(rng, pl)) for pl in (1, 16, 1025, 0, 4101)]
    encs = np.full(32 * len(items), 0xAA, np.uint8)
    cts = np.full(sum(len(p) + 16 for _, _, p in items), 0xAA, np.uint8)
    got, st = _seal(gpu, cfg, INFO, items, encs=encs, cts=cts)
    assert st[:5].tolist() == [4] * 5
    assert got == [(bytes(32), bytes(len(pt) + 16)) for _, _, pt in items]


def test_offsets_that_do_not_fit_fail_alone(gpu):
    kp = _keypair(1, 1)
    rng = np.random.default_rng(12)
    lens = (1025, 33, 40, 2049, 1024, 17, 70)
    n = len(lens)
    items = [(_rnd(rng, 32), _rnd(rng, 60), _rnd(rng, pl)) for pl in lens]
    sk, aads, aoff, pts, poff = _pack(items)
    coff = _offsets([pl + 16 for pl in lens])
    want = [H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:]
            for sk_e, aad, pt in items]
    # report 5's plaintext offsets run backwards; report 4's plaintext then runs up to report 6's
    # and no longer fits its slot
    poff2 = poff.copy()
    poff2[5] = poff2[6] + 3
    encs, cts, _, st = H.seal_long_batch_gpu(gpu, kp.config, INFO, sk, aads, aoff, pts, poff2,
                                             ct_offsets=coff)
    got = _split(n, encs, cts, coff)
    assert st[:n].tolist() == [0, 0, 0, 0, 4, 4, 0]
    for i in (0, 1, 2, 3, 6):
        assert got[i] == want[i], i
    for i in (4, 5):
        assert got[i] == (bytes(32), bytes(lens[i] + 16)), i
    # report 2's AAD ends past the AAD buffer's total
    aoff2 = aoff.copy()
    aoff2[3] = aoff2[-1] + 1
    encs, cts, _, st = H.seal_long_batch_gpu(gpu, kp.config, INFO, sk, aads, aoff2, pts, poff,
                                             ct_offsets=coff)
    got = _split(n, encs, cts, coff)
    assert st[:n].tolist() == [0, 0, 4, 4, 0, 0, 0]      # report 3's AAD then starts past its end
    for i in (0, 1, 4, 5, 6):
        assert got[i] == want[i], i


# ---- 4. suites, arguments, the profile -----------------------------------------------------------
def test_unsupported_suites_launch_nothing(gpu):
    rng = np.random.default_rng(5)
    sk, aads, aoff, pts, poff = _pack([(bytes(range(32)), b"aad", b"message")])
    read, off = _profile(gpu)
    try:
        for kem, kdf, aead in ((0x20, 1, 3), (0x10, 1, 1), (0x20, 9, 1)):
            pk = _rnd(rng, 65 if kem == 0x10 else 32)
            with pytest.raises(ValueError):
                H.seal_long_batch_gpu(gpu, H.HpkeConfig(1, kem, kdf, aead, pk), INFO, sk, aads,
                                      aoff, pts, poff)
            rc = lib().prio3gpu_hpke_seal_long_batch(gpu._ctx, kem, kdf, aead, pk, len(pk), INFO,
                                                     len(INFO), 0, None, None, None, None, None,
                                                     None, None, None, None)
            assert rc == E_UNSUPPORTED
        kp = _keypair(1, 1)
        rc = lib().prio3gpu_hpke_seal_long_batch(gpu._ctx, 0x20, 1, 1, kp.config.public_key, 31,
                                                 INFO, len(INFO), 1, None, None, None, None, None,
                                                 None, None, None, None)
        assert rc == E_ARG
        assert sum(read().values()) == 0                 # nothing launched
        encs, _, _, st = H.seal_long_batch_gpu(gpu, kp.config, INFO, sk, aads, aoff, pts, poff)
        names = read()
        assert names["k_x25519_eph"] == 1 and names["k_hpke_seal_team"] == 1
        assert names["k_hpke_seal"] == 0 and sum(names.values()) == 2
        assert encs.any() and st[0] == 0
    finally:
        off()


def test_empty_batch(gpu):
    kp = _keypair(2, 2)
    rc = lib().prio3gpu_hpke_seal_long_batch(gpu._ctx, 0x20, 2, 2, kp.config.public_key, 32, INFO,
                                             len(INFO), 0, None, None, None, None, None, None,
                                             None, None, None)
    assert rc == 0


# ---- 5. device pointers --------------------------------------------------------------------------
def test_device_tensors_equal_host_arrays(gpu):
    import torch
    kp = _keypair(3, 2)
    items = _mixed(33)[:20]
    n = len(items)
    sk, aads, aoff, pts, poff = _pack(items)
    st0 = np.zeros(n, np.uint8)
    st0[10] = 8
    hencs, hcts, hcoff, hst = H.seal_long_batch_gpu(gpu, kp.config, INFO, sk, aads, aoff, pts,
                                                    poff, status=st0.copy())
    dev = torch.device("cuda", gpu.device)

    def up(a):
        a = np.array(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    d_encs = torch.full((32 * n,), 0xAA, dtype=torch.uint8, device=dev)
    d_cts = torch.full((int(hcoff[-1]),), 0xAA, dtype=torch.uint8, device=dev)
    d_st = up(st0)
    torch.cuda.synchronize(dev)
    H.seal_long_batch_gpu(gpu, kp.config, INFO, up(sk), up(aads), up(aoff), up(pts), up(poff),
                          status=d_st, encs=d_encs, cts=d_cts, ct_offsets=up(hcoff), n=n)
    assert d_st.cpu().numpy().tolist() == hst[:n].tolist() and hst[10] == 8
    assert d_encs.cpu().numpy().tobytes() == hencs[:32 * n].tobytes()
    assert d_cts.cpu().numpy().tobytes() == hcts[:int(hcoff[-1])].tobytes()
    for i, (sk_e, aad, pt) in enumerate(items):
        if i != 10:
            _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert hencs[32 * i:32 * i + 32].tobytes() == enc
            assert hcts[int(hcoff[i]):int(hcoff[i + 1])].tobytes() == ct
