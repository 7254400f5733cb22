"""A caller's device buffers that the GPU HPKE entry points read in place are never written
(engine_hpke.hip: CallSecrets, I2): after a seal with its ephemeral keys and its plaintexts or
share rows in device memory, and after an open with its encapsulated keys and its ciphertexts or
payload rows there, those buffers read back byte for byte, though the engine zeroes its own staged
copies of the same inputs on the same stream.  Every input byte is non-zero, so a clear that hit a
caller's buffer cannot read back equal.  Three reports of 1, 16 and 65 plaintext bytes: less than
one AES block, exactly one, and over one 64-byte ChaCha20 chunk; X25519 / HKDF-SHA256 with
AES-128-GCM through every entry point, and ChaCha20-Poly1305 through the wave-per-report ones.
The outputs are checked against the host implementation (hpke.cpp)."""
import struct

import numpy as np
import pytest

from janus_amd import hpke as H

pytestmark = pytest.mark.gpu

X = H.KEM_X25519_HKDF_SHA256
AES, CHACHA = H.AEAD_AES128GCM, H.AEAD_CHACHA20POLY1305
TASK_ID = bytes(range(40, 72))
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
PT_LENS = (1, 16, 65)
AAD_LENS = (0, 60, 92)
N = len(PT_LENS)


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    v.set_option("hpke_team_chacha", 1)
    yield v
    v.close()


def _keypair(aead):
    return H.generate_hpke_config_and_private_key(7, X, H.KDF_HKDF_SHA256, aead)


def _up(gpu, a):
    import torch
    d = torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", gpu.device))
    torch.cuda.synchronize(d.device)
    return d


def _same(d, a):
    return np.array_equal(d.cpu().numpy(), a)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _packed(seed):
    """sk_es, aads, aad_offsets, pts, pt_offsets of N reports; keys and plaintexts without a zero
    byte."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, N * 32, dtype=np.uint8),
            rng.integers(0, 256, sum(AAD_LENS), dtype=np.uint8), _offsets(AAD_LENS),
            rng.integers(1, 256, sum(PT_LENS), dtype=np.uint8), _offsets(PT_LENS))


def _rows(slen, seed):
    """report ids, times, public shares, share rows and ephemeral keys of N reports."""
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(1, 256, shape, dtype=np.uint8)   # noqa: E731
    times = (1_700_000_000 + 17 * np.arange(N)).astype(np.uint64)
    return r(N, 16), times, r(N, 32), r(N, slen), r(N, 32)


def _frame(share):
    return b"\0\0" + struct.pack(">I", len(share)) + bytes(share)


def _cut(a, off, i):
    return a[int(off[i]):int(off[i + 1])].tobytes()


# ---- the seals: sk_es and the plaintexts or share rows on the device -----------------------------
@pytest.mark.parametrize("seal,aead", [(H.seal_batch_gpu, AES), (H.seal_long_batch_gpu, AES),
                                       (H.seal_long_batch_gpu, CHACHA)])
def test_packed_seals_leave_device_keys_and_plaintexts(gpu, seal, aead):
    kp = _keypair(aead)
    sk, aads, aoff, pts, poff = _packed(11 + aead)
    d_sk, d_pts = _up(gpu, sk), _up(gpu, pts)
    encs, cts, coff, st = seal(gpu, kp.config, INFO, d_sk, aads, aoff, d_pts, poff)
    assert not st[:N].any()
    assert _same(d_sk, sk) and _same(d_pts, pts)
    for i in range(N):
        got = H.open_(kp, INFO, encs[32 * i:32 * i + 32].tobytes(), _cut(cts, coff, i),
                      _cut(aads, aoff, i))
        assert got == _cut(pts, poff, i), i


@pytest.mark.parametrize("slen", PT_LENS)
@pytest.mark.parametrize("seal,aead", [(H.seal_input_shares_gpu, AES),
                                       (H.seal_input_shares_long_gpu, AES),
                                       (H.seal_input_shares_long_gpu, CHACHA)])
def test_share_seals_leave_device_keys_and_rows(gpu, seal, aead, slen):
    kp = _keypair(aead)
    ids, times, pub, shares, sk = _rows(slen, 23 + aead + slen)
    d_sk, d_shares = _up(gpu, sk), _up(gpu, shares)
    encs, pays, st = seal(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids, times, pub, d_shares, d_sk)
    assert not st[:N].any()
    assert _same(d_sk, sk) and _same(d_shares, shares)
    for i in range(N):
        aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]), pub[i].tobytes())
        assert H.open_(kp, INFO, encs[i].tobytes(), pays[i].tobytes(), aad) == _frame(shares[i]), i


# ---- the opens: encs and the ciphertexts or payload rows on the device ---------------------------
@pytest.mark.parametrize("opener,aead", [(H.open_batch_gpu, AES), (H.open_long_batch_gpu, AES),
                                         (H.open_long_batch_gpu, CHACHA)])
def test_packed_opens_leave_device_encs_and_ciphertexts(gpu, opener, aead):
    kp = _keypair(aead)
    _, aads, aoff, pts, poff = _packed(37 + aead)
    sealed = [H.seal(kp.config, INFO, _cut(pts, poff, i), _cut(aads, aoff, i)) for i in range(N)]
    encs = np.frombuffer(b"".join(e for _, e, _ in sealed), np.uint8)
    cts = np.frombuffer(b"".join(c for _, _, c in sealed), np.uint8)
    coff = _offsets([len(c) for _, _, c in sealed])
    d_encs, d_cts = _up(gpu, encs), _up(gpu, cts)
    # integer device pointers: what both entry points' wrappers have always taken
    got, goff, st = opener(gpu, kp, INFO, d_encs.data_ptr(), aads, aoff, d_cts.data_ptr(), coff)
    assert not st[:N].any() and np.array_equal(goff, poff)
    assert np.array_equal(got[:len(pts)], pts)
    assert _same(d_encs, encs) and _same(d_cts, cts)


@pytest.mark.parametrize("slen", PT_LENS)
@pytest.mark.parametrize("aead", [AES, CHACHA])
def test_share_open_leaves_device_encs_and_payloads(gpu, aead, slen):
    kp = _keypair(aead)
    ids, times, pub, shares, _ = _rows(slen, 51 + aead + slen)
    sealed = [H.seal(kp.config, INFO, _frame(shares[i]),
                     H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]), pub[i].tobytes()))
              for i in range(N)]
    encs = np.frombuffer(b"".join(e for _, e, _ in sealed), np.uint8).reshape(N, 32)
    pays = np.frombuffer(b"".join(c for _, _, c in sealed), np.uint8).reshape(N, 6 + slen + 16)
    d_encs, d_pays = _up(gpu, encs), _up(gpu, pays)
    out, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub, d_encs,
                                      d_pays)
    assert not st[:N].any() and np.array_equal(out, shares)
    assert _same(d_encs, encs) and _same(d_pays, pays)


def test_open_batch_gpu_takes_torch_tensors(gpu):
    """The lane-per-report wrapper takes device tensors as its wave-per-report twin does."""
    kp = _keypair(AES)
    _, aads, aoff, pts, poff = _packed(5)
    sealed = [H.seal(kp.config, INFO, _cut(pts, poff, i), _cut(aads, aoff, i)) for i in range(N)]
    encs = np.frombuffer(b"".join(e for _, e, _ in sealed), np.uint8)
    cts = np.frombuffer(b"".join(c for _, _, c in sealed), np.uint8)
    coff = _offsets([len(c) for _, _, c in sealed])
    d_encs, d_cts = _up(gpu, encs), _up(gpu, cts)
    for opener in (H.open_batch_gpu, H.open_long_batch_gpu):
        got, _, st = opener(gpu, kp, INFO, d_encs, aads, aoff, d_cts, coff)
        assert not st[:N].any() and np.array_equal(got[:len(pts)], pts)
    assert _same(d_encs, encs) and _same(d_cts, cts)
