"""Batched HPKE seal on the GPU to DHKEM(P-256, HKDF-SHA256) configs behind the context's
"hpke_gpu_p256" option (janus_amd/csrc/hpke_seal_gpu.h: k_p256_eph, k_p256_eph_kem; the lane and
wave AEAD kernels with bc.dh_ok set): the option and argument errors, RFC 9180 A.3.1's bytes under
its own ephemeral key, the ladders alone against tests/p256_model.py, every suite against the host
implementation (hpke.cpp) a lane and a wave per report, statuses, pitched columns, device tensors
and the launch counts.  Everything is byte-exact."""
import ctypes
import json
import os

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import p256_model as E

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "hpke_rfc9180_vectors.json")))
h = bytes.fromhex
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
SK_EM = h("4995788ef4b9d6132b249ce59a77281493eb39af373d236a1fe415cb0c2d7beb")  # RFC 9180 A.3.1
KEM = H.KEM_P256_HKDF_SHA256
N = E.N
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
LANE_LENS = (0, 15, 16, 17, 257)
TEAM_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4101)
INVALID_SCALARS = [0, N, N + 1, 2**256 - 1]
E_ARG, E_HPKE, E_UNSUPPORTED = -1, -5, -6
SEAL_ENTRIES = ("prio3gpu_hpke_seal_batch", "prio3gpu_hpke_seal_long_batch")
SHARE_ENTRIES = ("prio3gpu_seal_input_shares", "prio3gpu_seal_input_shares_long")


def _new_gpu(**options):
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    for k, val in options.items():
        v.set_option(k, val)
    return v


@pytest.fixture(scope="module")
def gpu():
    v = _new_gpu(hpke_gpu_p256=1)
    yield v
    v.close()


@pytest.fixture(scope="module")
def gpu_chacha():
    v = _new_gpu(hpke_gpu_p256=1, hpke_team_chacha=1)
    yield v
    v.close()


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _scalar(rng):
    return E.random_scalar(rng).to_bytes(32, "big")


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _pack(items):
    """[(sk_e, aad, pt)] -> sk_es, aads, aad_offsets, pts, pt_offsets of seal_batch_gpu."""
    sk = np.frombuffer(b"".join(s for s, _, _ in items) + b"\0", np.uint8)[:-1]
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    pts = np.frombuffer(b"".join(p for _, _, p in items) + b"\0", np.uint8)
    return (sk, aads, _offsets([len(a) for _, a, _ in items]), pts,
            _offsets([len(p) for _, _, p in items]))


def _split(n, encs, cts, coff, nenc=65):
    return [(encs[nenc * i:nenc * i + nenc].tobytes(),
             cts[int(coff[i]):int(coff[i + 1])].tobytes()) for i in range(n)]


def _seal(gpu, config, info, items, fn=H.seal_batch_gpu, **kw):
    """-> ([(enc, ct)], status)"""
    encs, cts, coff, st = fn(gpu, config, info, *_pack(items), **kw)
    return _split(len(items), encs, cts, coff, H.enc_len(config.kem_id)), st


def _keypair(kdf, aead, config_id=1, kem=KEM):
    return H.generate_hpke_config_and_private_key(config_id, kem, kdf, aead)


def _profile(gpu):
    """(read, off): read() -> {kernel name: launches} since the last read."""
    L, ctx = lib(), gpu._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0

    def read():
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        return {L.prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}

    read()  # drain
    return read, lambda: L.prio3gpu_prof_enable(ctx, 0)


def _seal_rc(entry, gpu, pk, kem=KEM, n=0):
    return getattr(lib(), entry)(gpu._ctx, kem, 1, 1, pk, len(pk), INFO, len(INFO), n, None, None,
                                 None, None, None, None, None, None, None)


def _shares_rc(entry, gpu, pk, kem=KEM, n=0):
    return getattr(lib(), entry)(gpu._ctx, bytes(32), kem, 1, 1, pk, len(pk), H.ROLE_LEADER, n,
                                 None, None, None, 0, None, 0, 0, None, None, 0, None, 0, None)


# ---- 1. the option and the arguments -------------------------------------------------------------
def test_option_off_is_unsupported_and_launches_nothing():
    v = _new_gpu()
    try:
        pk = _keypair(1, 1).config.public_key
        read, off = _profile(v)
        for entry in SEAL_ENTRIES:
            assert _seal_rc(entry, v, pk) == E_UNSUPPORTED
        for entry in SHARE_ENTRIES:
            assert _shares_rc(entry, v, pk) == E_UNSUPPORTED
        sk, aads, aoff, pts, poff = _pack([(_scalar(np.random.default_rng(1)), b"aad", b"msg")])
        for fn in (H.seal_batch_gpu, H.seal_long_batch_gpu):
            with pytest.raises(ValueError):
                fn(v, H.HpkeConfig(1, KEM, 1, 1, pk), INFO, sk, aads, aoff, pts, poff)
        assert sum(read().values()) == 0
        off()
    finally:
        v.close()


def test_public_key_length_and_point_checks_launch_nothing(gpu):
    pk = _keypair(1, 1).config.public_key
    x, y = E.decode(pk)
    off_curve = E.encode((x, (y + 1) % E.P))
    x_is_p = b"\x04" + E.P.to_bytes(32, "big") + pk[33:]
    compressed = b"\x02" + pk[1:]
    read, off = _profile(gpu)
    try:
        for entry, rc in [(e, _seal_rc) for e in SEAL_ENTRIES] + \
                         [(e, _shares_rc) for e in SHARE_ENTRIES]:
            for bad in (pk[:32], pk[:64], pk + b"\0"):
                assert rc(entry, gpu, bad, n=1) == E_ARG, (entry, len(bad))
            for bad in (off_curve, x_is_p, compressed):
                assert rc(entry, gpu, bad, n=1) == E_HPKE, entry
        assert sum(read().values()) == 0
    finally:
        off()


# ---- 2. known answer -----------------------------------------------------------------------------
def _vector_a31():
    v = [x for x in VECTORS if (x["kem_id"], x["kdf_id"], x["aead_id"]) == (0x10, 1, 1)][0]
    assert E.encode(E.mul(int.from_bytes(SK_EM, "big"), E.G)) == h(v["enc"])
    return v, H.HpkeConfig(0, KEM, 1, 1, h(v["pkRm"]))


@pytest.mark.parametrize("fn", [H.seal_batch_gpu, H.seal_long_batch_gpu])
def test_rfc9180_a31_alone_first_and_last_of_130(gpu, fn):
    v, cfg = _vector_a31()
    info, kat = h(v["info"]), (SK_EM, h(v["aad"]), h(v["pt"]))
    got, st = _seal(gpu, cfg, info, [kat], fn=fn)
    assert st[0] == 0 and got[0] == (h(v["enc"]), h(v["ct"]))
    rng = np.random.default_rng(931)
    others = [(_scalar(rng), _rnd(rng, 7), _rnd(rng, int(rng.integers(0, 40))))
              for _ in range(128)]
    got, st = _seal(gpu, cfg, info, [kat] + others + [kat], fn=fn)
    assert (st[:130] == 0).all()
    assert got[0] == got[129] == (h(v["enc"]), h(v["ct"]))
    for i in (1, 64, 65, 128):
        sk_e, aad, pt = others[i - 1]
        assert got[i] == H.seal(cfg, info, pt, aad, ephemeral_private_key=sk_e)[1:], i


# ---- 3. the ladders alone ------------------------------------------------------------------------
def _eph_hook(gpu, pk, scalars):
    n = len(scalars)
    sk = np.frombuffer(b"".join(k.to_bytes(32, "big") for k in scalars), np.uint8).copy()
    enc, dh, ok = np.zeros(65 * n, np.uint8), np.zeros(32 * n, np.uint8), np.zeros(n, np.uint8)
    rc = lib().prio3gpu_test_p256_eph_gpu(gpu._ctx, pk, sk.ctypes.data, n, enc.ctypes.data,
                                          dh.ctypes.data, ok.ctypes.data)
    assert rc == 0
    return ([enc[65 * i:65 * i + 65].tobytes() for i in range(n)],
            [dh[32 * i:32 * i + 32].tobytes() for i in range(n)], ok.tolist())


def _eph_model(pk_pt, k):
    return E.encode(E.mul(k, E.G)), E.mul(k, pk_pt)[0].to_bytes(32, "big")


@pytest.fixture(scope="module")
def eph_reference():
    """130 scalars (the edge ones first) under one recipient point, the model's answers once."""
    rng = np.random.default_rng(130)
    pk_pt = E.random_point(rng)
    edge = [1, 2, 3, N - 2, N - 1, (N - 1) // 2, (N + 1) // 2, 2**255, 2**32]
    scalars = edge + [E.random_scalar(rng) for _ in range(130 - len(edge))]
    return pk_pt, scalars, [_eph_model(pk_pt, k) for k in scalars]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_eph_hook_equals_model(gpu, eph_reference, n):
    pk_pt, scalars, want = eph_reference
    enc, dh, ok = _eph_hook(gpu, E.encode(pk_pt), scalars[:n])
    assert ok == [1] * n
    assert list(zip(enc, dh)) == want[:n]


def test_eph_hook_at_a_point_with_x_zero(gpu):
    """The recipient's key (0, sqrt b): x([k] pk) from the complete formulas, no special case."""
    for pk_pt in E.X0:
        enc, dh, ok = _eph_hook(gpu, E.encode(pk_pt), [1, 2, N - 1])
        assert ok == [1, 1, 1] and dh[0] == bytes(32)
        assert list(zip(enc, dh)) == [_eph_model(pk_pt, k) for k in (1, 2, N - 1)]


def test_eph_hook_invalid_scalars_between_valid_neighbours(gpu, eph_reference):
    pk_pt, scalars, want = eph_reference
    ks, ref = list(scalars[:64]), list(want[:64])
    for slot, bad in zip((0, 17, 40, 63), INVALID_SCALARS):
        ks[slot], ref[slot] = bad, (bytes(65), bytes(32))
    enc, dh, ok = _eph_hook(gpu, E.encode(pk_pt), ks)
    assert ok == [0 if i in (0, 17, 40, 63) else 1 for i in range(64)]
    assert list(zip(enc, dh)) == ref


# ---- 4. every suite ------------------------------------------------------------------------------
def _grid(seed, lens):
    rng = np.random.default_rng(seed)
    return [(_scalar(rng), _rnd(rng, al), _rnd(rng, pl)) for pl in lens for al in lens]


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_lane_seal_equals_host_seal_and_opens(gpu, kdf, aead):
    kp = _keypair(kdf, aead)
    items = _grid(100 * kdf + aead, LANE_LENS)
    got, st = _seal(gpu, kp.config, INFO, items)
    assert (st[:len(items)] == 0).all()
    for (sk_e, aad, pt), (enc, ct) in zip(items, got):
        assert (enc, ct) == H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:]
        assert H.open_(kp, INFO, enc, ct, aad) == pt


@pytest.mark.parametrize("kdf,aead", SUITES)
def test_team_seal_equals_lane_seal(gpu, gpu_chacha, kdf, aead):
    g = gpu_chacha if aead == 3 else gpu
    kp = _keypair(kdf, aead)
    rng = np.random.default_rng(200 * kdf + aead)
    items = [(_scalar(rng), _rnd(rng, (0, 60, 92)[j % 3]), _rnd(rng, pl))
             for j, pl in enumerate(TEAM_LENS)]
    n = len(items)
    team, st = _seal(g, kp.config, INFO, items, fn=H.seal_long_batch_gpu)
    lane, lst = _seal(g, kp.config, INFO, items)
    assert (st[:n] == 0).all() and (lst[:n] == 0).all() and team == lane
    for (sk_e, aad, pt), got in zip(items, team):
        assert got == H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:], len(pt)


def test_team_chacha_needs_its_option(gpu):
    kp = _keypair(1, 3)
    with pytest.raises(ValueError):
        H.seal_long_batch_gpu(gpu, kp.config, INFO, *_pack([(_scalar(np.random.default_rng(3)),
                                                             b"a", b"p")]))


# ---- 5. statuses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [H.seal_batch_gpu, H.seal_long_batch_gpu])
def test_statuses_and_zeroed_slots(gpu, fn):
    rng = np.random.default_rng(55)
    kp = _keypair(2, 2)
    lens = (40, 33, 1025, 17, 70, 0, 16)
    n = len(lens)
    items = [(_scalar(rng), _rnd(rng, 60), _rnd(rng, pl)) for pl in lens]
    items[2] = ((N + 5).to_bytes(32, "big"),) + items[2][1:]     # an invalid scalar
    items[5] = (bytes(32),) + items[5][1:]                        # the scalar 0
    # the host refuses these keys too
    with pytest.raises(H.HpkeError):
        H.seal(kp.config, INFO, items[2][2], items[2][1], ephemeral_private_key=items[2][0])
    slot = [pl + 16 for pl in lens]
    slot[4] -= 1        # one byte short
    slot[3] += 9        # longer: zero-filled past the tag
    coff = _offsets(slot)
    st0 = np.zeros(n, np.uint8)
    st0[1] = 9          # skipped on entry
    cts = np.full(int(coff[-1]), 0xAA, np.uint8)
    encs = np.full(65 * n, 0xAA, np.uint8)
    got, st = _seal(gpu, kp.config, INFO, items, fn=fn, status=st0, encs=encs, cts=cts,
                    ct_offsets=coff)
    want_st = [0, 9, 4, 0, 4, 4, 0]
    assert st[:n].tolist() == want_st
    for i, (sk_e, aad, pt) in enumerate(items):
        if want_st[i]:
            assert got[i] == (bytes(65), bytes(slot[i])), i
        else:
            _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)
            assert got[i] == (enc, ct + bytes(slot[i] - len(ct))), i


# ---- 6. input shares into pitched columns --------------------------------------------------------
@pytest.mark.parametrize("fn", [H.seal_input_shares_gpu, H.seal_input_shares_long_gpu])
def test_seal_input_shares_writes_only_its_columns(gpu, fn):
    rng = np.random.default_rng(66)
    kp = _keypair(1, 1)
    n, slen, pslen = 9, 1031, 5
    plen = 6 + slen + 16
    tid, ids = _rnd(rng, 32), np.frombuffer(_rnd(rng, 16 * n), np.uint8).reshape(n, 16)
    times = rng.integers(0, 2**40, n).astype(np.uint64)
    pubs = np.frombuffer(_rnd(rng, pslen * n), np.uint8).reshape(n, pslen)
    shares = np.frombuffer(_rnd(rng, slen * n), np.uint8).reshape(n, slen)
    sk = np.frombuffer(b"".join(_scalar(rng) for _ in range(n)), np.uint8).reshape(n, 32)
    o_enc, o_pay = 3, 3 + 65 + 4                    # odd offsets, as in a Report row
    mat = np.full((n, o_pay + plen + 7), 0xA5, np.uint8)
    _, _, st = fn(gpu, tid, kp.config, H.ROLE_LEADER, ids, times, pubs, shares, sk,
                  mat[:, o_enc:o_enc + 65], mat[:, o_pay:o_pay + plen])
    assert (st[:n] == 0).all()
    want = np.full_like(mat, 0xA5)
    for i in range(n):
        pt = b"\0\0" + slen.to_bytes(4, "big") + shares[i].tobytes()
        aad = H.input_share_aad(tid, ids[i].tobytes(), int(times[i]), pubs[i].tobytes())
        _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk[i].tobytes())
        want[i, o_enc:o_enc + 65] = np.frombuffer(enc, np.uint8)
        want[i, o_pay:o_pay + plen] = np.frombuffer(ct, np.uint8)
    assert np.array_equal(mat, want)


# ---- 7. device tensors ---------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [H.seal_batch_gpu, H.seal_long_batch_gpu])
def test_device_tensors_equal_host_arrays(gpu, fn):
    import torch
    kp = _keypair(3, 2)
    items = _grid(77, (0, 17, 257))
    n = len(items)
    sk, aads, aoff, pts, poff = _pack(items)
    hencs, hcts, hcoff, hst = fn(gpu, kp.config, INFO, sk, aads, aoff, pts, poff)
    dev = torch.device("cuda", gpu.device)

    def up(a):
        a = np.array(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    d_encs = torch.full((65 * n,), 0xAA, dtype=torch.uint8, device=dev)
    d_cts = torch.full((int(hcoff[-1]),), 0xAA, dtype=torch.uint8, device=dev)
    d_st = up(np.zeros(n, np.uint8))
    torch.cuda.synchronize(dev)
    fn(gpu, kp.config, INFO, up(sk), up(aads), up(aoff), up(pts), up(poff), status=d_st,
       encs=d_encs, cts=d_cts, ct_offsets=up(hcoff), n=n)
    assert d_st.cpu().numpy().tolist() == hst[:n].tolist() == [0] * n
    assert d_encs.cpu().numpy().tobytes() == hencs[:65 * n].tobytes()
    assert d_cts.cpu().numpy().tobytes() == hcts[:int(hcoff[-1])].tobytes()


# ---- 8. launch counts; X25519 is untouched -------------------------------------------------------
def test_launch_counts_and_x25519_unchanged(gpu):
    rng = np.random.default_rng(88)
    kp = _keypair(1, 1)
    xkp = _keypair(1, 1, kem=H.KEM_X25519_HKDF_SHA256)
    items = [(_scalar(rng), _rnd(rng, 9), _rnd(rng, pl)) for pl in (0, 33, 1025)]
    plain = _new_gpu()
    try:
        want_x, _ = _seal(plain, xkp.config, INFO, items)
        want_xl, _ = _seal(plain, xkp.config, INFO, items, fn=H.seal_long_batch_gpu)
    finally:
        plain.close()
    read, off = _profile(gpu)
    try:
        for fn, aead_kernel in ((H.seal_batch_gpu, "k_hpke_seal"),
                                (H.seal_long_batch_gpu, "k_hpke_seal_team")):
            _seal(gpu, kp.config, INFO, items, fn=fn)
            names = read()
            assert names["k_p256_eph"] == 1 and names["k_p256_eph_kem"] == 1
            assert names[aead_kernel] == 1 and sum(names.values()) == 3
        got_x, _ = _seal(gpu, xkp.config, INFO, items)
        names = read()
        assert names["k_x25519_eph"] == 1 and names["k_hpke_seal"] == 1
        assert sum(names.values()) == 2
        got_xl, _ = _seal(gpu, xkp.config, INFO, items, fn=H.seal_long_batch_gpu)
        names = read()
        assert names["k_x25519_eph"] == 1 and names["k_hpke_seal_team"] == 1
        assert sum(names.values()) == 2
        assert got_x == want_x and got_xl == want_xl
    finally:
        off()
