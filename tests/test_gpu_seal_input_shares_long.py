"""prio3gpu_seal_input_shares_long (janus_amd/csrc/hpke_seal_team.h: k_hpke_seal_team_shares): the
wave-per-report twin of prio3gpu_seal_input_shares.  Share rows are sealed into packed columns,
into enc and payload columns at odd offsets of a pre-filled report matrix (no byte outside the
columns changes) and on the device; the bytes are the lane-per-report seal's and the host seal's of
the Python-built frame and AAD, and the wave-per-report open gives the rows back."""
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


def _host_seal(kp, ids, times, pub, shares, sk, i):
    """(enc, payload) of the host seal of report i's Python-built frame under its AAD."""
    frame = b"\0\0" + struct.pack(">I", shares.shape[1]) + shares[i].tobytes()
    aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]),
                            pub[i].tobytes() if pub is not None else b"")
    return H.seal(kp.config, INFO, frame, aad, ephemeral_private_key=sk[i].tobytes())[1:]


@pytest.mark.parametrize("slen", SHARE_LENS)
def test_packed_pitched_and_device_equal_lane_and_host_seal(gpu, slen):
    import torch
    n, pslen = 9, (0 if slen == 10 else 32)
    kp = _keypair(1 + slen % 3, 1 + slen % 2)
    ids, times, pub, shares, sk = _batch(n, slen, pslen, slen)
    plen = 6 + slen + 16
    want_e, want_p, st = H.seal_input_shares_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids,
                                                 times, pub, shares, sk)
    assert not st[:n].any()
    for i in range(n):
        enc, pay = _host_seal(kp, ids, times, pub, shares, sk, i)
        assert want_e[i].tobytes() == enc and want_p[i].tobytes() == pay, i
    # host, packed rows
    encs, pays, st = H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids,
                                                  times, pub, shares, sk)
    assert not st[:n].any()
    assert np.array_equal(encs, want_e) and np.array_equal(pays, want_p)
    # host, the columns at odd offsets of a pre-filled matrix: the gaps stay
    lead, gap, tail = 3, 5, 9
    mat = np.full((n, lead + 32 + gap + plen + tail), 0xA5, np.uint8)
    o_pay = lead + 32 + gap
    _, _, st = H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids, times,
                                            pub, shares, sk, mat[:, lead:lead + 32],
                                            mat[:, o_pay:o_pay + plen])
    want = np.full_like(mat, 0xA5)
    want[:, lead:lead + 32], want[:, o_pay:o_pay + plen] = want_e, want_p
    assert not st[:n].any() and np.array_equal(mat, want)
    # device: rows, keys and the matrix on the GPU; with an odd row width the columns' alignment
    # changes from row to row, with an even one (shift 1) every payload block starts at an odd
    # address
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_pub = up(pub) if pslen else None
    for shift in (0, 1):
        width = want.shape[1] + shift
        d_mat = torch.full((n, width), 0xA5, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, up(ids),
                                     up(times.view(np.int64)), d_pub, up(shares), up(sk),
                                     d_mat[:, lead:lead + 32], d_mat[:, o_pay:o_pay + plen],
                                     status=d_st)
        got = d_mat.cpu().numpy()
        assert not d_st.cpu().numpy().any()
        assert np.array_equal(got[:, :want.shape[1]], want), shift
        assert (got[:, want.shape[1]:] == 0xA5).all()
    # and back through the wave-per-report open
    out, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub,
                                      mat[:, lead:lead + 32], mat[:, o_pay:o_pay + plen])
    assert not st[:n].any() and np.array_equal(out, shares)


def test_three_leader_sized_shares(gpu):
    """SumVec(8, 1000)-sized rows: 134,944 bytes each, 8,435 blocks over 64 lanes, the payload
    column at an odd offset of a device matrix with the report's own pitch."""
    import torch
    n, slen = 3, 134_944
    kp = _keypair()
    ids, times, pub, shares, sk = _batch(n, slen, 32, 1349)
    plen = 6 + slen + 16
    assert plen == 134_966
    dev = torch.device("cuda", gpu.device)
    d_mat = torch.full((n, 135_174), 0xA5, dtype=torch.uint8, device=dev)
    d_shares = torch.from_numpy(shares).to(dev)
    torch.cuda.synchronize(dev)
    _, _, st = H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids, times,
                                            pub, d_shares, sk, d_mat[:, 63:95],
                                            d_mat[:, 99:99 + plen])
    got = d_mat.cpu().numpy()
    assert not st[:n].any()
    want_e, want_p, st = H.seal_input_shares_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids,
                                                 times, pub, shares, sk)
    assert not st[:n].any()
    assert np.array_equal(got[:, 63:95], want_e) and np.array_equal(got[:, 99:99 + plen], want_p)
    assert (got[:, :63] == 0xA5).all() and (got[:, 95:99] == 0xA5).all()
    assert (got[:, 99 + plen:] == 0xA5).all()
    # against the host seal of the first row: the lane seal is not the only witness
    enc, pay = _host_seal(kp, ids, times, pub, shares, sk, 0)
    assert got[0, 63:95].tobytes() == enc and got[0, 99:99 + plen].tobytes() == pay
    out, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub,
                                      got[:, 63:95], got[:, 99:99 + plen])
    assert not st[:n].any() and np.array_equal(out, shares)


def test_skipped_reports_and_a_small_order_key(gpu):
    n, slen = 6, 1019
    kp = _keypair(2, 2)
    ids, times, pub, shares, sk = _batch(n, slen, 32, 17)
    plen = 6 + slen + 16
    encs, pays = np.full((n, 32), 0xAA, np.uint8), np.full((n, plen), 0xAA, np.uint8)
    st = np.zeros(n, np.uint8)
    st[1], st[4] = 7, 3
    H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, H.ROLE_LEADER, ids, times, pub, shares,
                                 sk, encs, pays, st)
    assert list(st) == [0, 7, 0, 0, 3, 0]
    for i in range(n):
        if st[i]:
            assert not encs[i].any() and not pays[i].any(), i
        else:
            enc, pay = _host_seal(kp, ids, times, pub, shares, sk, i)
            assert encs[i].tobytes() == enc and pays[i].tobytes() == pay, i
    cfg = H.HpkeConfig(5, 0x20, 1, 1, bytes(32))
    encs, pays = np.full((n, 32), 0xAA, np.uint8), np.full((n, plen), 0xAA, np.uint8)
    _, _, st = H.seal_input_shares_long_gpu(gpu, TASK_ID, cfg, H.ROLE_LEADER, ids, times, pub,
                                            shares, sk, encs, pays)
    assert list(st[:n]) == [4] * n and not encs.any() and not pays.any()


def test_pitch_and_suite_errors(gpu):
    kp = _keypair()
    n, slen = 4, 26
    ids, times, pub, shares, sk = _batch(n, slen, 32, 3)
    plen = 6 + slen + 16
    encs, pays, st = np.zeros((n, 32), np.uint8), np.zeros((n, plen), np.uint8), \
        np.zeros(n, np.uint8)
    c = kp.config
    tid = np.frombuffer(TASK_ID, np.uint8).copy()

    def call(kem=c.kem_id, kdf=c.kdf_id, aead=c.aead_id, n=n, share_pitch=slen, enc_pitch=32,
             pay_pitch=plen):
        return lib().prio3gpu_seal_input_shares_long(
            gpu._ctx, tid.ctypes.data, kem, kdf, aead, c.public_key, 32, H.ROLE_LEADER, n,
            ids.ctypes.data, times.ctypes.data, pub.ctypes.data, 32, shares.ctypes.data, slen,
            share_pitch, sk.ctypes.data, encs.ctypes.data, enc_pitch, pays.ctypes.data, pay_pitch,
            st.ctypes.data)

    want = [_host_seal(kp, ids, times, pub, shares, sk, i) for i in range(n)]
    assert call() == 0
    assert [(encs[i].tobytes(), pays[i].tobytes()) for i in range(n)] == want
    encs[:], pays[:] = 0, 0
    assert call(share_pitch=0, enc_pitch=0, pay_pitch=0) == 0
    assert [(encs[i].tobytes(), pays[i].tobytes()) for i in range(n)] == want
    assert call(share_pitch=slen - 1) == E_ARG
    assert call(enc_pitch=31) == E_ARG
    assert call(pay_pitch=plen - 1) == E_ARG
    assert call(aead=3) == E_UNSUPPORTED and call(kem=0x10) == E_UNSUPPORTED
    assert call(kdf=9) == E_UNSUPPORTED and call(aead=3, n=0) == E_UNSUPPORTED
    assert call(n=0) == 0
    for bad in (H.HpkeConfig(5, 0x20, 1, 3, c.public_key), H.HpkeConfig(5, 0x10, 1, 1, bytes(65)),
                H.HpkeConfig(5, 0x20, 9, 1, c.public_key)):
        with pytest.raises(ValueError):
            H.seal_input_shares_long_gpu(gpu, TASK_ID, bad, H.ROLE_LEADER, ids, times, pub, shares,
                                         sk)
