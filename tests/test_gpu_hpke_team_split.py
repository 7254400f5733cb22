"""Several waves per report for the share-row HPKE open and seal (janus_amd/csrc/hpke_team_split.h,
the context options "hpke_team_split" and "hpke_team_split_blocks"): prio3gpu_seal_input_shares_long
and prio3gpu_open_input_shares with the option on against the same call with it off -- the bytes,
the statuses and every byte outside the columns -- for every suite the wave per report takes, at
the share lengths where a segment boundary moves; tampering in every segment; and the client
driver's reports through the upload open into prepare_init.  The profiling counts say which kernels
ran.  The options are unknown to the engine before this feature, so the first test fails there."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib

pytestmark = pytest.mark.gpu

TASK_ID = bytes(range(70, 102))
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
X = H.KEM_X25519_HKDF_SHA256
E_ARG = -1
SPLIT, BLOCKS = 8, 256
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2, 3)]
# bodies (6 + share) of 4096 k + {-1, 0, 1, 17} bytes for k = 2, 3: around two and three segments
# of the smallest size; and 16,000: three segments of 384 blocks (two of 512 for ChaCha20-Poly1305)
SHARE_LENS = [4096 * k - 6 + d for k in (2, 3) for d in (-1, 0, 1, 17)] + [16_000]
NS = (1, 3, 5)


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    v.set_option("hpke_team_chacha", 1)
    v.set_option("hpke_team_split_blocks", BLOCKS)
    yield v
    v.close()


class split:
    """`with split(gpu):` the calls inside may give a report up to SPLIT waves."""

    def __init__(self, gpu, k=SPLIT):
        self.gpu, self.k = gpu, k

    def __enter__(self):
        self.gpu.set_option("hpke_team_split", self.k)

    def __exit__(self, *exc):
        self.gpu.set_option("hpke_team_split", 0)


def _keypair(kdf=1, aead=1, kem=X):
    return H.generate_hpke_config_and_private_key(5, kem, kdf, aead)


def _batch(n, slen, pslen, seed):
    rng = np.random.default_rng(seed)
    r = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)   # noqa: E731
    times = (1_700_000_000 + 31 * np.arange(n)).astype(np.uint64)
    sk = r(n, 32)
    sk[:, 0] &= 0x7f                  # a P-256 scalar too (big-endian, below the order)
    return r(n, 16), times, (r(n, pslen) if pslen else None), r(n, slen), sk


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


def _seal(gpu, cfg, ids, times, pub, shares, sk, encs=None, pays=None, status=None):
    return H.seal_input_shares_long_gpu(gpu, TASK_ID, cfg, H.ROLE_LEADER, ids, times, pub, shares,
                                        sk, encs, pays, status)


def _open(gpu, kp, ids, times, pub, encs, pays, out=None, status=None):
    return H.open_input_shares_gpu(gpu, TASK_ID, kp, H.ROLE_LEADER, ids, times, pub, encs, pays,
                                   out_shares=out, status=status)


def _host_open(kp, ids, times, pub, encs, pays, i):
    aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]),
                            pub[i].tobytes() if pub is not None else b"")
    return H.open_(kp, INFO, encs[i].tobytes(), pays[i].tobytes(), aad)


# ---- 1. the options ------------------------------------------------------------------------------
def test_the_two_options_and_their_ranges(gpu):
    opt = lambda name, v: lib().prio3gpu_ctx_set_option(gpu._ctx, name, v)   # noqa: E731
    try:
        for v in (0, 1, 2, 8, 256):
            assert opt(b"hpke_team_split", v) == 0, v
        for v in (257, -1, 1 << 20):
            assert opt(b"hpke_team_split", v) == E_ARG, v
        for v in (256, 512, 4096, 1 << 24):
            assert opt(b"hpke_team_split_blocks", v) == 0, v
        for v in (100, 0, -256, 255, 257, 4096 + 64, (1 << 24) + 256):
            assert opt(b"hpke_team_split_blocks", v) == E_ARG, v
    finally:
        assert opt(b"hpke_team_split", 0) == 0
        assert opt(b"hpke_team_split_blocks", BLOCKS) == 0


# ---- 2. seal -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", SUITES)
def test_seal_with_the_option_on_equals_off(gpu, kdf, aead):
    """Packed host columns, and enc and payload columns at odd offsets of a pre-filled device
    matrix whose row width changes the alignment from row to row."""
    import torch
    kp = _keypair(kdf, aead)
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for j, slen in enumerate(SHARE_LENS):
        n = NS[(j + kdf) % 3]
        pslen = 0 if j == 2 else 32
        ids, times, pub, shares, sk = _batch(n, slen, pslen, 1000 * kdf + 100 * aead + j)
        plen = 6 + slen + 16
        want_e, want_p, st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
        assert not st[:n].any()
        with split(gpu):
            encs, pays, st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
        assert not st[:n].any()
        assert np.array_equal(encs, want_e) and np.array_equal(pays, want_p), slen
        if j % 3 == 0:
            continue
        lead, gap, tail = 3, 5, 8 + j % 2
        want = np.full((n, lead + 32 + gap + plen + tail), 0xA5, np.uint8)
        o_pay = lead + 32 + gap
        want[:, lead:lead + 32], want[:, o_pay:o_pay + plen] = want_e, want_p
        d_mat = torch.full(want.shape, 0xA5, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with split(gpu):
            _seal(gpu, kp.config, up(ids), up(times.view(np.int64)), up(pub) if pslen else None,
                  up(shares), up(sk), d_mat[:, lead:lead + 32], d_mat[:, o_pay:o_pay + plen],
                  d_st)
        assert not d_st.cpu().numpy().any()
        assert np.array_equal(d_mat.cpu().numpy(), want), slen


def test_seal_three_leader_sized_shares(gpu):
    """SumVec(8, 1000)-sized rows, 8,436 blocks: eight segments of 1,088."""
    import torch
    n, slen = 3, 134_944
    kp = _keypair()
    ids, times, pub, shares, sk = _batch(n, slen, 32, 1349)
    plen = 6 + slen + 16
    dev = torch.device("cuda", gpu.device)
    d_shares = torch.from_numpy(shares).to(dev)
    want_e, want_p, st = _seal(gpu, kp.config, ids, times, pub, d_shares, sk)
    assert not st[:n].any()
    d_mat = torch.full((n, 135_174), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with split(gpu):
        _, _, st = _seal(gpu, kp.config, ids, times, pub, d_shares, sk, d_mat[:, 63:95],
                         d_mat[:, 99:99 + plen])
    got = d_mat.cpu().numpy()
    assert not st[:n].any()
    assert np.array_equal(got[:, 63:95], want_e) and np.array_equal(got[:, 99:99 + plen], want_p)
    assert (got[:, :63] == 0xA5).all() and (got[:, 95:99] == 0xA5).all()
    assert (got[:, 99 + plen:] == 0xA5).all()
    with split(gpu):
        out, st = _open(gpu, kp, ids, times, pub, got[:, 63:95], got[:, 99:99 + plen])
    assert not st[:n].any() and np.array_equal(out, shares)


@pytest.mark.parametrize("aead", [1, 3])
def test_seal_skipped_reports_and_a_small_order_key(gpu, aead):
    n, slen = 5, 16_000
    kp = _keypair(2, aead)
    ids, times, pub, shares, sk = _batch(n, slen, 32, 17 + aead)
    plen = 6 + slen + 16
    st0 = np.zeros(n, np.uint8)
    st0[1], st0[4] = 7, 3
    want_e, want_p, want_st = _seal(gpu, kp.config, ids, times, pub, shares, sk,
                                    status=st0.copy())
    encs, pays = np.full((n, 32), 0xAA, np.uint8), np.full((n, plen), 0xAA, np.uint8)
    with split(gpu):
        _, _, st = _seal(gpu, kp.config, ids, times, pub, shares, sk, encs, pays, st0.copy())
    assert list(st) == list(want_st) == [0, 7, 0, 0, 3]
    assert np.array_equal(encs, want_e) and np.array_equal(pays, want_p)
    for i in (1, 4):
        assert not encs[i].any() and not pays[i].any()
    assert pays[0].any() and pays[2].any()
    cfg = H.HpkeConfig(5, 0x20, 2, aead, bytes(32))          # a public key of small order
    encs, pays = np.full((n, 32), 0xAA, np.uint8), np.full((n, plen), 0xAA, np.uint8)
    with split(gpu):
        _, _, st = _seal(gpu, cfg, ids, times, pub, shares, sk, encs, pays)
    assert list(st[:n]) == [4] * n and not encs.any() and not pays.any()


def test_seal_and_open_under_p256(gpu):
    n, slen = 3, 4096 * 3 - 6 + 17
    gpu.set_option("hpke_gpu_p256", 1)
    try:
        kp = _keypair(1, 1, H.KEM_P256_HKDF_SHA256)
        ids, times, pub, shares, sk = _batch(n, slen, 32, 256)
        sk[1] = 0                                            # no P-256 scalar: status 4
        want_e, want_p, want_st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
        with split(gpu):
            encs, pays, st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
        assert list(st[:n]) == list(want_st[:n]) == [0, 4, 0]
        assert encs.shape == (n, 65) and np.array_equal(encs, want_e)
        assert np.array_equal(pays, want_p) and not pays[1].any() and pays[0].any()
        want_out, want_st = _open(gpu, kp, ids, times, pub, encs, pays)
        with split(gpu):
            out, st = _open(gpu, kp, ids, times, pub, encs, pays)
        assert list(st[:n]) == list(want_st[:n]) == [0, 4, 0]   # enc 00 .. 00 is no point
        assert np.array_equal(out, want_out) and not out[1].any()
        assert np.array_equal(out[0], shares[0]) and np.array_equal(out[2], shares[2])
    finally:
        gpu.set_option("hpke_gpu_p256", 0)


def test_seal_launches_the_split_kernels_only_where_the_plan_splits(gpu):
    kp = _keypair()
    read, off = _profile(gpu)
    try:
        for slen, splits in ((8186, True), (4000, False)):
            ids, times, pub, shares, sk = _batch(3, slen, 32, slen)
            with split(gpu):
                _seal(gpu, kp.config, ids, times, pub, shares, sk)
            k = read()
            assert k["k_x25519_eph"] == 1
            assert k["k_hpke_seal_team_split"] == k["k_hpke_seal_team_join"] == int(splits)
            assert k["k_hpke_seal_team_shares"] == int(not splits)
            assert sum(k.values()) == 2 + int(splits)
        ids, times, pub, shares, sk = _batch(3, 8186, 32, 1)
        _seal(gpu, kp.config, ids, times, pub, shares, sk)       # the option at 0: the one wave
        k = read()
        assert k["k_hpke_seal_team_split"] == 0 and k["k_hpke_seal_team_shares"] == 1
    finally:
        off()


# ---- 3. open -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", SUITES)
def test_open_with_the_option_on_equals_off_and_the_host(gpu, kdf, aead):
    """Host rows packed, and device rows at a 128-byte pitch in a pre-filled buffer."""
    import torch
    kp = _keypair(kdf, aead)
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for j, slen in enumerate(SHARE_LENS):
        n = NS[(j + aead) % 3]
        pslen = 0 if j == 5 else 32
        ids, times, pub, shares, sk = _batch(n, slen, pslen, 2000 * kdf + 100 * aead + j)
        encs, pays, st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
        assert not st[:n].any()
        frame = b"\0\0" + struct.pack(">I", slen) + shares[n - 1].tobytes()
        assert _host_open(kp, ids, times, pub, encs, pays, n - 1) == frame
        off_out, st = _open(gpu, kp, ids, times, pub, encs, pays)
        assert not st[:n].any() and np.array_equal(off_out, shares)
        with split(gpu):
            out, st = _open(gpu, kp, ids, times, pub, encs, pays)
        assert not st[:n].any() and np.array_equal(out, shares), slen
        if j % 3 == 1:
            continue
        pitch = 128 * (-(-slen // 128))
        d_rows = torch.full((n, pitch + 128), 0x5A, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with split(gpu):
            _open(gpu, kp, up(ids), up(times.view(np.int64)), up(pub) if pslen else None,
                  up(encs), up(pays), d_rows[:, :slen], d_st)
        got = d_rows.cpu().numpy()
        assert not d_st.cpu().numpy().any()
        assert np.array_equal(got[:, :slen], shares) and (got[:, slen:] == 0x5A).all(), slen


@pytest.mark.parametrize("aead", [1, 2, 3])
def test_a_flipped_bit_in_any_segment_or_the_tag_fails_that_report_alone(gpu, aead):
    import torch
    n, slen = 3, 16_000
    kp = _keypair(1, aead)
    ids, times, pub, shares, sk = _batch(n, slen, 32, 400 + aead)
    encs, pays, st = _seal(gpu, kp.config, ids, times, pub, shares, sk)
    body = 6 + slen
    seg = 16 * (512 if aead == 3 else 384)                  # team_split_plan's L for this body
    places = {"segment 0": 3, "end of segment 0": seg - 1, "segment 1": seg + 16,
              "last segment": body - 1, "tag": body + 5}
    assert aead == 3 or 2 * seg < body - 1                  # three segments under AES-GCM
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    pitch = 128 * (-(-slen // 128))
    for where, byte in places.items():
        bad = pays.copy()
        bad[1, byte] ^= 0x10
        d_rows = torch.full((n, pitch), 0x5A, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with split(gpu):
            _open(gpu, kp, up(ids), up(times.view(np.int64)), up(pub), up(encs), up(bad),
                  d_rows[:, :slen], d_st)
        got = d_rows.cpu().numpy()
        assert list(d_st.cpu().numpy()) == [0, 4, 0], where
        assert not got[1, :slen].any(), where
        assert np.array_equal(got[0, :slen], shares[0]) and np.array_equal(got[2, :slen], shares[2])
        assert (got[:, slen:] == 0x5A).all(), where
        out, st = _open(gpu, kp, ids, times, pub, encs, bad)     # the option off: the same
        assert list(st[:n]) == [0, 4, 0] and not out[1].any()


@pytest.mark.parametrize("aead", [1, 3])
def test_open_other_headers_skipped_rows_and_a_small_order_enc(gpu, aead):
    """Authentic plaintexts whose six leading bytes are not 00 00 | u32 slen are status 8 and a
    zero row; a row skipped on entry keeps its status and is zeroed; an enc of small order (its
    DH value is all zero) is status 4.  The neighbours open."""
    kp = _keypair(3, aead)
    n, slen = 5, 8186 + 17
    ids, times, pub, shares, sk = _batch(n, slen, 32, 80 + aead)
    frames = [b"\0\0" + struct.pack(">I", slen) + shares[i].tobytes() for i in range(n)]
    body = shares[1].tobytes()
    frames[1] = b"\0\1" + body[:1] + struct.pack(">I", slen - 1) + body[1:]   # one extension byte
    frames[3] = b"\0\0" + struct.pack(">I", slen + 1) + shares[3].tobytes()
    encs, pays = np.zeros((n, 32), np.uint8), np.zeros((n, 6 + slen + 16), np.uint8)
    for i in range(n):
        aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]), pub[i].tobytes())
        _, enc, ct = H.seal(kp.config, INFO, frames[i], aad)
        encs[i], pays[i] = np.frombuffer(enc, np.uint8), np.frombuffer(ct, np.uint8)
    encs[2] = 0                                              # a point of small order
    st0 = np.zeros(n, np.uint8)
    st0[4] = 7
    want_out, want_st = _open(gpu, kp, ids, times, pub, encs, pays,
                              np.full((n, slen), 0xAA, np.uint8), st0.copy())
    out = np.full((n, slen), 0xAA, np.uint8)
    with split(gpu):
        _, st = _open(gpu, kp, ids, times, pub, encs, pays, out, st0.copy())
    assert list(st) == list(want_st) == [0, 8, 4, 8, 7]
    assert np.array_equal(out, want_out) and np.array_equal(out[0], shares[0])
    assert not out[1:].any()


def test_open_launches_the_split_kernels_only_where_the_plan_splits(gpu):
    kp = _keypair()
    read, off = _profile(gpu)
    try:
        for slen, splits in ((8186, True), (4000, False)):
            ids, times, pub, shares, sk = _batch(3, slen, 32, slen + 1)
            encs, pays, _ = _seal(gpu, kp.config, ids, times, pub, shares, sk)
            read()
            with split(gpu):
                out, st = _open(gpu, kp, ids, times, pub, encs, pays)
            assert not st[:3].any() and np.array_equal(out, shares)
            k = read()
            assert k["k_x25519"] == 1
            assert (k["k_hpke_open_team_split"] == k["k_hpke_open_team_join"]
                    == k["k_hpke_team_wipe"] == int(splits))
            assert k["k_hpke_open_team_shares"] == int(not splits)
            assert sum(k.values()) == (4 if splits else 2)
        _open(gpu, kp, ids, times, pub, encs, pays)
        k = read()                                           # the option at 0: the one wave
        assert k["k_hpke_open_team_split"] == 0 and k["k_hpke_open_team_shares"] == 1
    finally:
        off()


# ---- 4. end to end -------------------------------------------------------------------------------
N_E2E = 5


@functools.lru_cache(maxsize=None)
def _oracle_batch(name):
    from tests.reports import make_batch
    return make_batch(name, N_E2E)


@pytest.mark.parametrize("name", ["fp16_300", "sumvec_8_1000"])
def test_client_reports_open_and_prepare_like_the_oracle(name):
    from janus_amd import client as CL
    from janus_amd.prio3 import Prio3Gpu
    from janus_amd.upload import UploadBatch
    from tests.reports import CONFIGS, meas_array
    b = _oracle_batch(name)
    c = CONFIGS[name]
    v = Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                 chunk_length=c["chunk"])
    g = H.generate_hpke_config_and_private_key
    leader, helper = g(11, X, 1, 1), g(21, X, 1, 1)
    sk = np.random.default_rng(9).integers(0, 256, (2, N_E2E, 32), dtype=np.uint8)
    times = np.array([1_700_000_100 + 613 * i for i in range(N_E2E)], np.uint64)
    L, ctx = lib(), v._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()

    def launched():
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        return {L.prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}

    def reports(team_split):
        cb = CL.ClientBatch(v, TASK_ID, leader.config, helper.config, 300, team_split=team_split,
                            team_split_blocks=BLOCKS)
        try:
            return cb.prepare_reports(meas_array(b), report_ids=b.nonces, times=times,
                                      rand=b.rand, sk_es=sk, device_out=True)
        finally:
            cb.close()

    try:
        assert v.sizes.leader_input_share >= 2 * 16 * BLOCKS      # long enough to split
        assert L.prio3gpu_prof_enable(ctx, 1) == 0
        plain = reports(0)
        assert launched()["k_hpke_seal_team_split"] == 0
        d_reports = reports(SPLIT)
        assert launched()["k_hpke_seal_team_split"] == 1
        assert np.array_equal(d_reports.cpu().numpy(), plain.cpu().numpy())
        up = UploadBatch(v, TASK_ID, [leader], team_split=SPLIT, team_split_blocks=BLOCKS)
        rows, st = up.open_reports(d_reports)
        k = launched()
        assert k["k_hpke_open_team_split"] == 1 and k["k_hpke_open_team_shares"] == 0
        assert L.prio3gpu_prof_enable(ctx, 0) == 0
        assert not st.any() and rows.is_cuda and rows.stride(0) % 128 == 0
        assert np.array_equal(rows.cpu().numpy(), b.leader_in)
        ls = v.new_state(0, N_E2E)
        pub = b.public if b.public.shape[1] else None
        lp, lst = v.prepare_init(ls, b.nonces, pub, rows)
        assert not lst.any() and np.array_equal(lp, b.leader_prep)
        ls.close()
    finally:
        v.close()
