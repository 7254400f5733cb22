"""prio3gpu_open_input_shares (janus_amd/csrc/hpke_open_team.h: k_hpke_open_team_shares): the
mirror of prio3gpu_seal_input_shares.  Shares sealed by the GPU client come back byte for byte
from enc and payload columns at odd offsets of a report matrix, into packed rows and rows at a
128-byte pitch, on the host and on the device, and no byte outside a row is written; a plaintext
that authenticates but is no extension-free share of the row's length is status 8."""
import struct

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib

pytestmark = pytest.mark.gpu

TASK_ID = bytes(range(90, 122))
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
SHARE_LENS = (1, 10, 26, 48, 1018, 1019, 2576)
E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    yield v
    v.close()


def _keypair(kdf=1, aead=1):
    return H.generate_hpke_config_and_private_key(5, H.KEM_X25519_HKDF_SHA256, kdf, aead)


def _batch(n, slen, pslen, seed):
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)   # noqa: E731
    times = (1_700_000_000 + 31 * np.arange(n)).astype(np.uint64)
    return r(n, 16), times, (r(n, pslen) if pslen else None), r(n, slen), r(n, 32)


def _sealed_matrix(gpu, kp, ids, times, pub, shares, sk, lead=3, gap=5, tail=9):
    """The shares sealed by the GPU into the enc and payload columns of an (n, width) matrix
    filled with 0xC3: enc at column `lead`, payload `gap` bytes after it."""
    n, slen = shares.shape
    plen = 6 + slen + 16
    mat = np.full((n, lead + 32 + gap + plen + tail), 0xC3, np.uint8)
    encs, pays = mat[:, lead:lead + 32], mat[:, lead + 32 + gap:lead + 32 + gap + plen]
    _, _, st = H.seal_input_shares_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids, times, pub,
                                       shares, sk, encs, pays)
    assert not st[:n].any()
    return mat, encs, pays


@pytest.mark.parametrize("slen", SHARE_LENS)
def test_round_trip_packed_pitched_and_device(gpu, slen):
    import torch
    n, pslen = 9, (0 if slen == 10 else 32)
    kp = _keypair(1 + slen % 3, 1 + slen % 2)
    ids, times, pub, shares, sk = _batch(n, slen, pslen, slen)
    mat, encs, pays = _sealed_matrix(gpu, kp, ids, times, pub, shares, sk)
    before = mat.copy()
    # host, packed rows
    out, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub, encs, pays)
    assert not st[:n].any() and np.array_equal(out, shares)
    # host, rows at a 128-byte pitch inside a pre-filled buffer: the gaps stay
    pitch = 128 * (-(-slen // 128))
    wide = np.full((n, pitch), 0x5A, np.uint8)
    _, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub, encs, pays,
                                    out_shares=wide[:, :slen])
    assert not st[:n].any() and np.array_equal(wide[:, :slen], shares)
    assert (wide[:, slen:] == 0x5A).all()
    # device: the matrix and the rows on the GPU, rows at the pitch and, shifted by one byte,
    # at no alignment at all
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_mat = up(mat)
    d_pub = up(pub) if pslen else None
    for shift in (0, 1):
        d_wide = torch.full((n, pitch + 16), 0x5A, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, up(ids),
                                up(times.view(np.int64)), d_pub, d_mat[:, 3:35],
                                d_mat[:, 40:40 + pays.shape[1]],
                                out_shares=d_wide[:, shift:shift + slen], status=d_st)
        got = d_wide.cpu().numpy()
        assert not d_st.cpu().numpy().any()
        assert np.array_equal(got[:, shift:shift + slen], shares), shift
        assert (got[:, :shift] == 0x5A).all() and (got[:, shift + slen:] == 0x5A).all()
    assert np.array_equal(d_mat.cpu().numpy(), before) and np.array_equal(mat, before)


def test_three_leader_sized_shares(gpu):
    """SumVec(8, 1000)-sized rows: 134,944 bytes each, 8,436 blocks over 64 lanes."""
    import torch
    n, slen = 3, 134_944
    kp = _keypair()
    ids, times, pub, shares, sk = _batch(n, slen, 32, 1349)
    mat, encs, pays = _sealed_matrix(gpu, kp, ids, times, pub, shares, sk, lead=1, gap=4, tail=0)
    assert pays.shape[1] == 134_966
    # against the host open of the first row: the GPU seal is not the only witness
    pt = H.open_(kp, INFO, encs[0].tobytes(), pays[0].tobytes(),
                 H.input_share_aad(TASK_ID, ids[0].tobytes(), int(times[0]), pub[0].tobytes()))
    assert pt == b"\0\0" + struct.pack(">I", slen) + shares[0].tobytes()
    dev = torch.device("cuda", gpu.device)
    d_mat = torch.from_numpy(mat).to(dev)
    pitch = 128 * (-(-slen // 128))
    d_rows = torch.full((n, pitch), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    _, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub,
                                    d_mat[:, 1:33], d_mat[:, 37:37 + 134_966],
                                    out_shares=d_rows[:, :slen])
    got = d_rows.cpu().numpy()
    assert not st[:n].any() and np.array_equal(got[:, :slen], shares)
    assert (got[:, slen:] == 0x5A).all()
    # one flipped bit deep inside the second row: that row alone is zeros
    mat[1, 37 + 100_000] ^= 4
    out, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub,
                                      mat[:, 1:33], mat[:, 37:37 + 134_966])
    assert list(st[:n]) == [0, 4, 0] and not out[1].any()
    assert np.array_equal(out[0], shares[0]) and np.array_equal(out[2], shares[2])


@pytest.mark.parametrize("slen", [10, 48, 1019])
def test_other_headers_are_invalid_messages(gpu, slen):
    """Plaintexts of the right total length whose first six bytes are not 00 00 | u32 slen:
    authentic, so status 8 (the reference's "Leader input share decoding failed") and a zero row;
    the neighbours open."""
    kp = _keypair()
    n = 6
    ids, times, pub, shares, sk = _batch(n, slen, 32, 80 + slen)
    frames = [b"\0\0" + struct.pack(">I", slen) + shares[i].tobytes() for i in range(n)]
    body = shares[1].tobytes()
    frames[1] = b"\0\1" + body[:1] + struct.pack(">I", slen - 1) + body[1:]   # one extension byte
    frames[2] = b"\0\0" + struct.pack(">I", slen + 1) + shares[2].tobytes()
    frames[4] = b"\0\0" + struct.pack(">I", slen | 1 << 24) + shares[4].tobytes()
    encs, pays = np.zeros((n, 32), np.uint8), np.zeros((n, 6 + slen + 16), np.uint8)
    for i in range(n):
        aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]), pub[i].tobytes())
        _, enc, ct = H.seal(kp.config, INFO, frames[i], aad)
        encs[i], pays[i] = np.frombuffer(enc, np.uint8), np.frombuffer(ct, np.uint8)
    out = np.full((n, slen), 0xAA, np.uint8)
    st = np.zeros(n, np.uint8)
    st[5] = 7                                                    # skipped on entry
    H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub, encs, pays,
                            out_shares=out, status=st)
    assert list(st) == [0, 8, 8, 0, 8, 7]
    for i in (0, 3):
        assert np.array_equal(out[i], shares[i])
    for i in (1, 2, 4, 5):
        assert not out[i].any()
    # the wrong role in the info, the wrong task id: nothing authenticates
    for tid, role in ((TASK_ID, H.ROLE_HELPER), (bytes(32), H.ROLE_LEADER)):
        out, st = H.open_input_shares_gpu(gpu, tid, kp, role, ids, times, pub, encs, pays)
        assert (st[:n] == 4).all() and not out.any()


def test_pitch_and_suite_errors(gpu):
    kp = _keypair()
    n, slen = 4, 26
    ids, times, pub, shares, sk = _batch(n, slen, 32, 3)
    mat, encs, pays = _sealed_matrix(gpu, kp, ids, times, pub, shares, sk)
    out, st = np.zeros((n, slen), np.uint8), np.zeros(n, np.uint8)
    c = kp.config
    tid = np.frombuffer(TASK_ID, np.uint8).copy()
    pe, pp = np.ascontiguousarray(encs), np.ascontiguousarray(pays)

    def call(kem=c.kem_id, kdf=c.kdf_id, aead=c.aead_id, n=n, enc_pitch=32, pay_pitch=pp.shape[1],
             out_pitch=slen):
        return lib().prio3gpu_open_input_shares(
            gpu._ctx, tid.ctypes.data, kem, kdf, aead, kp.private_key, 32, c.public_key, 32,
            H.ROLE_LEADER, n, ids.ctypes.data, times.ctypes.data, pub.ctypes.data, 32,
            pe.ctypes.data, enc_pitch, pp.ctypes.data, pay_pitch, slen, out.ctypes.data,
            out_pitch, st.ctypes.data)

    assert call() == 0 and np.array_equal(out, shares)
    assert call(enc_pitch=0, pay_pitch=0, out_pitch=0) == 0 and np.array_equal(out, shares)
    assert call(enc_pitch=31) == E_ARG
    assert call(pay_pitch=pp.shape[1] - 1) == E_ARG
    assert call(out_pitch=slen - 1) == E_ARG
    assert call(aead=3) == E_UNSUPPORTED and call(kem=0x10) == E_UNSUPPORTED
    assert call(kdf=4) == E_UNSUPPORTED and call(aead=3, n=0) == E_UNSUPPORTED
    assert call(n=0) == 0
