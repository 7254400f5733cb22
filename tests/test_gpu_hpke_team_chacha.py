"""ChaCha20-Poly1305 a wave per report (janus_amd/csrc/chacha_poly_team.h under the AEAD 3
instantiations of hpke_open_team.h's and hpke_seal_team.h's kernels), behind the context option
"hpke_team_chacha": the option's gate on the four long entry points, the packed seal and open
against the lane kernels and the host implementation (hpke.cpp), the share-row seal and open against
the lane seal and the oracle's shares, tampering, and the drivers (ClientBatch, UploadBatch) with
their `team_chacha` flag.  Everything is byte-exact; every call carries 9 reports (two full blocks
of four waves and a lone wave) except the three SumVec(8, 1000) ones."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from janus_amd import client as CL
from janus_amd import hpke as H
from janus_amd._lib import lib
from janus_amd.upload import UploadBatch
from tests.reports import CONFIGS, make_batch, meas_array

pytestmark = pytest.mark.gpu

X = H.KEM_X25519_HKDF_SHA256
CHACHA = H.AEAD_CHACHA20POLY1305
TASK_ID = bytes(range(70, 102))
PRECISION = 300
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
# one ChaCha block, one trip of 64 chunks and three trips, each with its neighbours; in an order
# that puts packed ciphertext slots at even and odd offsets and at several residues mod 16
PT_LENS = (1, 63, 65, 4095, 0, 4097, 12289, 64, 4096)
N = len(PT_LENS)
E_ARG, E_UNSUPPORTED = -1, -6


def _new_count():
    from janus_amd.prio3 import Prio3Gpu
    return Prio3Gpu.new_count(bytes(16))


@pytest.fixture(scope="module")
def gpu():
    """A context with the option on, and the lane open of every suite for comparison."""
    v = _new_count()
    v.set_option("hpke_team_chacha", 1)
    v.set_option("hpke_gpu_suites", 1)
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


def _keypair(kdf, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, X, kdf, CHACHA)


def _items(seed):
    rng = np.random.default_rng(seed)
    return [(_rnd(rng, 32), _rnd(rng, (0, 60, 92)[j % 3]), _rnd(rng, pl))
            for j, pl in enumerate(PT_LENS)]


def _launches(v, f):
    """(f(), {kernel name: launches during f})"""
    L, ctx = lib(), v._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        out = f()
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        return out, {L.prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}
    finally:
        L.prio3gpu_prof_enable(ctx, 0)


# ---- 1. the option's gate ------------------------------------------------------------------------
def test_option_gate_on_the_four_long_entry_points():
    v = _new_count()
    try:
        kp = _keypair(1)
        pk, sk = kp.config.public_key, kp.private_key
        tid = np.frombuffer(TASK_ID, np.uint8).copy()
        L, ctx = lib(), v._ctx

        def calls(kem, kdf, aead, pk=pk):
            return [
                L.prio3gpu_hpke_open_long_batch(ctx, kem, kdf, aead, sk, 32, pk, len(pk), INFO,
                                                len(INFO), 0, None, None, None, None, None, None,
                                                None, None),
                L.prio3gpu_open_input_shares(ctx, tid.ctypes.data, kem, kdf, aead, sk, 32, pk,
                                             len(pk), H.ROLE_LEADER, 0, None, None, None, 0, None,
                                             0, None, 0, 16, None, 0, None),
                L.prio3gpu_hpke_seal_long_batch(ctx, kem, kdf, aead, pk, len(pk), INFO, len(INFO),
                                                0, None, None, None, None, None, None, None, None,
                                                None),
                L.prio3gpu_seal_input_shares_long(ctx, tid.ctypes.data, kem, kdf, aead, pk, len(pk),
                                                  H.ROLE_LEADER, 0, None, None, None, 0, None, 16,
                                                  0, None, None, 0, None, 0, None)]

        def gated():
            sk_es, aads, aoff, pts, poff = _pack(_items(1)[:1])
            with pytest.raises(ValueError):
                H.seal_long_batch_gpu(v, kp.config, INFO, sk_es, aads, aoff, pts, poff)

        assert calls(0x20, 1, 3) == [E_UNSUPPORTED] * 4          # the default: as before
        assert calls(0x20, 1, 1) == [0] * 4
        _, k = _launches(v, gated)
        assert sum(k.values()) == 0                              # nothing launched
        with pytest.raises(Exception):
            v.set_option("hpke_team_chacha", 2)
        assert L.prio3gpu_ctx_set_option(ctx, b"hpke_team_chacha", 2) == E_ARG
        assert L.prio3gpu_ctx_set_option(ctx, b"hpke_team_chacha", -1) == E_ARG
        assert calls(0x20, 1, 3) == [E_UNSUPPORTED] * 4          # a refused value changes nothing
        v.set_option("hpke_team_chacha", 1)
        for kdf in (1, 2, 3):
            assert calls(0x20, kdf, 3) == [0] * 4
        assert calls(0x20, 1, 1) == [0] * 4 and calls(0x20, 3, 2) == [0] * 4
        # P-256, other KDF ids and unknown AEAD ids stay unsupported
        assert calls(0x10, 1, 3, pk=bytes(65)) == [E_UNSUPPORTED] * 4
        assert calls(0x20, 9, 3) == [E_UNSUPPORTED] * 4
        assert calls(0x20, 0, 3) == [E_UNSUPPORTED] * 4
        assert calls(0x20, 1, 4) == [E_UNSUPPORTED] * 4
        v.set_option("hpke_team_chacha", 0)
        assert calls(0x20, 1, 3) == [E_UNSUPPORTED] * 4
    finally:
        v.close()


# ---- 2. packed seal and open ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_seals(kdf):
    """The keypair, the items and the host's (enc, ct) of each: computed once per KDF."""
    kp = _keypair(kdf)
    items = _items(300 + kdf)
    return kp, items, [H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=sk_e)[1:]
                       for sk_e, aad, pt in items]


@pytest.mark.parametrize("kdf", [1, 2, 3])
def test_seal_long_equals_lane_and_host_and_opens_again(gpu, kdf):
    kp, items, want = _host_seals(kdf)
    (encs, cts, coff, st), k = _launches(
        gpu, lambda: H.seal_long_batch_gpu(gpu, kp.config, INFO, *_pack(items)))
    assert k["k_hpke_seal_team"] == 1 and k["k_hpke_seal"] == 0
    assert (st[:N] == 0).all()
    residues = {int(o) % 16 for o in coff[:N]}
    assert any(r % 2 for r in residues) and len(residues) >= 3      # odd and even slot offsets
    got = _split(N, encs, cts, coff)
    assert got == want
    lenc, lcts, lcoff, lst = H.seal_batch_gpu(gpu, kp.config, INFO, *_pack(items))
    assert (lst[:N] == 0).all() and _split(N, lenc, lcts, lcoff) == got
    # and open again: the wave, the lane (under "hpke_gpu_suites") and the host agree
    _, aads, aoff, _, poff = _pack(items)
    (pts, ooff, ost), k = _launches(
        gpu, lambda: H.open_long_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff))
    assert k["k_hpke_open_team"] == 1 and k["k_hpke_open"] == 0
    assert (ost[:N] == 0).all() and ooff.tolist() == poff.tolist()
    lpts, loff, lost = H.open_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff)
    assert (lost[:N] == 0).all() and loff.tolist() == poff.tolist()
    total = int(poff[-1])
    assert pts[:total].tobytes() == lpts[:total].tobytes() == b"".join(p for _, _, p in items)
    for (sk_e, aad, pt), (enc, ct) in zip(items, got):
        assert H.open_(kp, INFO, enc, ct, aad) == pt


@pytest.mark.parametrize("kdf", [1, 3])
def test_seal_long_statuses_and_slots(gpu, kdf):
    kp, items, want = _host_seals(kdf)
    slot = [pl + 16 for pl in PT_LENS]
    slot[3] -= 1        # 4095 + 16 - 1: one byte short
    slot[5] += 100      # longer: zero-filled past the tag
    slot[7] += 1
    coff = _offsets(slot)
    st0 = np.zeros(N, np.uint8)
    st0[1], st0[6] = 9, 3                                          # skipped on entry
    cts = np.full(int(coff[-1]), 0xAA, np.uint8)
    encs = np.full(32 * N, 0xAA, np.uint8)
    encs, cts, _, st = H.seal_long_batch_gpu(gpu, kp.config, INFO, *_pack(items), status=st0,
                                             encs=encs, cts=cts, ct_offsets=coff)
    want_st = [0, 9, 0, 4, 0, 0, 3, 0, 0]
    assert st[:N].tolist() == want_st
    got = _split(N, encs, cts, coff)
    for i in range(N):
        if want_st[i]:
            assert got[i] == (bytes(32), bytes(slot[i])), i
        else:
            enc, ct = want[i]
            assert got[i] == (enc, ct + bytes(slot[i] - len(ct))), i
    # a public key of small order: every DH value is zero
    cfg = H.HpkeConfig(1, X, kdf, CHACHA, bytes(32))
    encs, cts, coff, st = H.seal_long_batch_gpu(gpu, cfg, INFO, *_pack(items),
                                                encs=np.full(32 * N, 0xAA, np.uint8))
    assert st[:N].tolist() == [4] * N and not encs[:32 * N].any()
    assert not cts[:int(coff[-1])].any()


def _flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("kdf", [1, 2, 3])
def test_open_long_tampering_gives_status_4_and_zeros(gpu, kdf):
    kp, items, sealed = _host_seals(kdf)
    by_len = {len(pt): i for i, (_, _, pt) in enumerate(items)}
    big, mid, trip = by_len[12289], by_len[4097], by_len[4096]
    # (item, what is done to it); the untouched ones sit between the tampered ones
    plan = [(big, None), (big, "tag"), (mid, "first chunk"), (by_len[65], None), (big, "chunk 64"),
            (trip, "last byte"), (by_len[65], "aad"), (by_len[64], "zero dh"), (mid, None)]
    assert len(plan) == N
    encs, aads, cts = [], [], []
    for i, what in plan:
        (_, aad, pt), (enc, ct) = items[i], sealed[i]
        if what == "tag":
            ct = _flip(ct, len(pt) + 9, 6)
        elif what == "first chunk":
            ct = _flip(ct, 17)
        elif what == "chunk 64":
            ct = _flip(ct, 64 * 64 + 3, 2)
        elif what == "last byte":
            ct = _flip(ct, len(pt) - 1, 7)
        elif what == "aad":
            aad = _flip(aad, 59)
        elif what == "zero dh":
            enc = bytes(32)                                        # a point of small order
        encs.append(enc), aads.append(aad), cts.append(ct)
    lens = [len(items[i][2]) for i, _ in plan]
    poff = _offsets(lens)
    pts = np.full(int(poff[-1]), 0xAA, np.uint8)
    args = (np.frombuffer(b"".join(encs), np.uint8), np.frombuffer(b"".join(aads), np.uint8),
            _offsets([len(a) for a in aads]), np.frombuffer(b"".join(cts), np.uint8),
            _offsets([len(c) for c in cts]))
    pts, _, st = H.open_long_batch_gpu(gpu, kp, INFO, *args, pts=pts, pt_offsets=poff)
    assert st[:N].tolist() == [4 if what else 0 for _, what in plan]
    for j, (i, what) in enumerate(plan):
        got = pts[int(poff[j]):int(poff[j + 1])].tobytes()
        assert got == (bytes(lens[j]) if what else items[i][2]), (j, what)
    lpts, _, lst = H.open_batch_gpu(gpu, kp, INFO, *args)           # the lane open says the same
    assert lst[:N].tolist() == st[:N].tolist()
    assert lpts[:int(poff[-1])].tobytes() == pts.tobytes()


# ---- 3. share rows -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(name, n):
    return make_batch(name, n)


def _times(n):
    return (1_700_000_000 + 31 * np.arange(n)).astype(np.uint64)


@pytest.mark.parametrize("role", [H.ROLE_LEADER, H.ROLE_HELPER])
@pytest.mark.parametrize("name", ["sum8", "sumvec_small"])
def test_share_rows_seal_and_open(gpu, name, role):
    b = _batch(name, N)
    shares = np.ascontiguousarray(b.leader_in if role == H.ROLE_LEADER else b.helper_in)
    slen = shares.shape[1]
    pub = np.ascontiguousarray(b.public) if b.public.shape[1] else None
    ids, times = np.ascontiguousarray(b.nonces), _times(N)
    kp = _keypair(1 + (slen + role) % 3, 7)
    sk = np.random.default_rng(slen + role).integers(0, 256, (N, 32), dtype=np.uint8)
    want_e, want_p, st = H.seal_input_shares_gpu(gpu, TASK_ID, kp.config, role, ids, times, pub,
                                                 shares, sk)
    assert not st[:N].any()
    (encs, pays, st), k = _launches(
        gpu, lambda: H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, role, ids, times, pub,
                                                  shares, sk))
    assert k["k_hpke_seal_team_shares"] == 1 and k["k_hpke_seal_shares"] == 0
    assert not st[:N].any()
    assert np.array_equal(encs, want_e) and np.array_equal(pays, want_p)
    # into columns at odd offsets of a pre-filled matrix: the gaps stay
    plen = 6 + slen + 16
    lead, gap, tail = 3, 5, 9
    mat = np.full((N, lead + 32 + gap + plen + tail), 0xA5, np.uint8)
    o_pay = lead + 32 + gap
    H.seal_input_shares_long_gpu(gpu, TASK_ID, kp.config, role, ids, times, pub, shares, sk,
                                 mat[:, lead:lead + 32], mat[:, o_pay:o_pay + plen])
    full = np.full_like(mat, 0xA5)
    full[:, lead:lead + 32], full[:, o_pay:o_pay + plen] = want_e, want_p
    assert np.array_equal(mat, full)
    # open: the oracle's shares
    (rows, st), k = _launches(
        gpu, lambda: H.open_input_shares_gpu(gpu, TASK_ID, kp, role, ids, times, pub,
                                             mat[:, lead:lead + 32], mat[:, o_pay:o_pay + plen]))
    assert k["k_hpke_open_team_shares"] == 1
    assert not st[:N].any() and np.array_equal(rows, shares)
    info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, role)
    aad0 = H.input_share_aad(TASK_ID, ids[0].tobytes(), int(times[0]),
                             pub[0].tobytes() if pub is not None else b"")
    assert H.open_(kp, info, encs[0].tobytes(), pays[0].tobytes(), aad0) == \
        b"\0\0" + struct.pack(">I", slen) + shares[0].tobytes()
    # a wrong task id: status 4 and zeros
    rows = np.full((N, slen), 0xAA, np.uint8)
    rows, st = H.open_input_shares_gpu(gpu, bytes(32), kp, role, ids, times, pub, encs, pays, rows)
    assert st[:N].tolist() == [4] * N and not rows.any()
    # forged headers, sealed by the host: a length one off in rows 2 and 6, and a tampered row 4
    pays = pays.copy()
    encs = encs.copy()
    for i, off in ((2, 1), (6, -1)):
        frame = b"\0\0" + struct.pack(">I", slen + off) + shares[i].tobytes()
        aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]),
                                pub[i].tobytes() if pub is not None else b"")
        _, enc, pay = H.seal(kp.config, info, frame, aad)
        encs[i], pays[i] = np.frombuffer(enc, np.uint8), np.frombuffer(pay, np.uint8)
    pays[4, plen - 1] ^= 0x10
    rows = np.full((N, slen), 0xAA, np.uint8)
    rows, st = H.open_input_shares_gpu(gpu, TASK_ID, kp, role, ids, times, pub, encs, pays, rows)
    want_st = [0, 0, 8, 0, 4, 0, 8, 0, 0]
    assert st[:N].tolist() == want_st
    for i in range(N):
        assert np.array_equal(rows[i], shares[i]) if want_st[i] == 0 else not rows[i].any(), i


# ---- 4. the drivers: SumVec(8, 1000), a 134,944-byte leader share -------------------------------
BIG, NBIG = "sumvec_8_1000", 3
SEALS = ("k_hpke_seal", "k_hpke_seal_shares", "k_hpke_seal_team", "k_hpke_seal_team_shares")


def _vdaf(name, b):
    from janus_amd.prio3 import Prio3Gpu
    c = CONFIGS[name]
    return Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                    chunk_length=c["chunk"])


@pytest.fixture(scope="module")
def big():
    b = _batch(BIG, NBIG)
    v = _vdaf(BIG, b)
    yield v, b
    v.close()


@functools.lru_cache(maxsize=None)
def _big_keys():
    g = H.generate_hpke_config_and_private_key
    return g(11, X, 1, CHACHA), g(12, X, 2, CHACHA)


def _prepare(v, b, device_out=False, **kw):
    lkp, hkp = _big_keys()
    cb = CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION, **kw)
    times = np.array([1_700_000_000 + 977 * i for i in range(NBIG)], np.uint64)
    sk = np.random.default_rng(8).integers(0, 256, (2, NBIG, 32), dtype=np.uint8)
    try:
        return _launches(v, lambda: cb.prepare_reports(meas_array(b), report_ids=b.nonces,
                                                       times=times, rand=b.rand, sk_es=sk,
                                                       device_out=device_out))
    finally:
        cb.close()


def test_client_and_upload_with_a_chacha_leader_key(big, monkeypatch):
    v, b = big
    assert v.sizes.leader_input_share == 134_944 and v.sizes.helper_input_share == 48
    lkp, hkp = _big_keys()
    with pytest.raises(ValueError):                       # without the flag: as before
        CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION, long_seal=True)
    lane, lane_k = _prepare(v, b, long_seal=False)
    assert [lane_k[k] for k in SEALS] == [0, 2, 0, 0]
    wave, wave_k = _prepare(v, b, long_seal=True, team_chacha=True, device_out=True)
    assert [wave_k[k] for k in SEALS] == [0, 0, 0, 2] and wave_k["k_x25519_eph"] == 2
    assert wave.is_cuda and np.array_equal(wave.cpu().numpy(), lane)
    # auto: by the class attribute alone, whatever was measured
    monkeypatch.setattr(CL.ClientBatch, "LONG_SEAL_MIN_SHARE_CHACHA", 1000)
    auto, auto_k = _prepare(v, b, long_seal=None, team_chacha=True)
    assert [auto_k[k] for k in SEALS] == [0, 1, 0, 1]      # leader: the wave; helper: the lane
    assert np.array_equal(auto, lane)
    monkeypatch.setattr(CL.ClientBatch, "LONG_SEAL_MIN_SHARE_CHACHA", None)
    auto, auto_k = _prepare(v, b, long_seal=None, team_chacha=True)
    assert [auto_k[k] for k in SEALS] == [0, 2, 0, 0] and np.array_equal(auto, lane)
    monkeypatch.setattr(CL.ClientBatch, "LONG_SEAL_MIN_SHARE_CHACHA", 1000)
    auto, auto_k = _prepare(v, b, long_seal=None)          # the threshold needs the flag
    assert [auto_k[k] for k in SEALS] == [0, 2, 0, 0] and np.array_equal(auto, lane)
    # the upload: opened on the device to the oracle's shares, and prepared where they are
    up = UploadBatch(v, TASK_ID, [lkp], team_chacha=True)
    (rows, st), k = _launches(v, lambda: up.open_reports(wave))
    assert k["k_hpke_open_team_shares"] == 1
    assert not st.any() and rows.is_cuda and rows.stride(0) % 128 == 0
    assert np.array_equal(rows.cpu().numpy(), b.leader_in[:NBIG])
    ls = v.new_state(0, NBIG)
    try:
        lp, lst = v.prepare_init(ls, b.nonces, b.public, rows)
        assert not lst.any() and np.array_equal(lp, b.leader_prep)
    finally:
        ls.close()
    hrows, st = UploadBatch(v, TASK_ID, [hkp], role=H.ROLE_HELPER,
                            team_chacha=True).open_reports(lane)
    assert not st.any() and np.array_equal(hrows, b.helper_in[:NBIG])


# ---- 5. UploadBatch's routing with the flag ------------------------------------------------------
NR = 33


@pytest.mark.parametrize("device", [False, True])
def test_routing_by_config_id_with_team_chacha(device):
    """tests/test_gpu_upload.py::test_routing_by_config_id's matrix of keys: the flag moves the
    ChaCha20-Poly1305 group to the GPU and changes no status and no row."""
    import torch
    name = "sumvec_small"
    b = _batch(name, NR)
    v = _vdaf(name, b)
    g = H.generate_hpke_config_and_private_key
    k = dict(a=g(11, X, 1, 1), b=g(12, X, 2, 2), chacha=g(13, X, 1, 3), rescued=g(14, X, 3, 1),
             helper=g(21, X, 1, 1))
    times = np.array([1_700_000_100 + 613 * i for i in range(NR)], np.uint64)

    def reports_for(leader_kp, seed):
        cb = CL.ClientBatch(v, TASK_ID, leader_kp.config, k["helper"].config, PRECISION)
        sk = np.random.default_rng(seed).integers(0, 256, (2, NR, 32), dtype=np.uint8)
        try:
            return cb.prepare_reports(meas_array(b), report_ids=b.nonces, times=times,
                                      rand=b.rand, sk_es=sk)
        finally:
            cb.close()

    try:
        per_key = {w: reports_for(k[w], 10 + j) for j, w in
                   enumerate(("a", "b", "chacha", "rescued"))}
        kinds = [("a", "b", "chacha", "rescued", "unknown", "lost")[i % 6] for i in range(NR)]
        reports = np.zeros_like(per_key["a"])
        layout = CL.ReportLayout(v.sizes.public_share, v.sizes.leader_input_share,
                                 v.sizes.helper_input_share)
        o_cfg = layout.o_leader
        for i, kind in enumerate(kinds):
            reports[i] = per_key[{"unknown": "a", "lost": "b"}.get(kind, kind)][i]
            if kind == "unknown":
                reports[i, o_cfg] = 99
            elif kind == "lost":                      # sealed to b, claims a's id: no key opens it
                reports[i, o_cfg] = k["a"].config.id
        # a tampered ChaCha20-Poly1305 report: the GPU group's failure, with no global key to try
        bad = kinds.index("chacha")
        reports[bad, layout.o_leader_payload + 7] ^= 1
        stale = H.generate_hpke_config_and_private_key(14, X, 3, 1)
        keys = [k["a"], k["b"], k["chacha"], stale]
        arg = torch.from_numpy(reports).to(torch.device("cuda", v.device)) if device else reports
        want = {"a": 0, "b": 0, "chacha": 0, "rescued": 0, "unknown": 3, "lost": 4}
        want_st = [4 if i == bad else want[kind] for i, kind in enumerate(kinds)]

        def opened(**kw):
            up = UploadBatch(v, TASK_ID, keys, global_keys=[k["rescued"], k["a"]], **kw)
            (rows, st), launches = _launches(v, lambda: up.open_reports(arg))
            return (rows.cpu().numpy() if device else rows), st, launches

        rows0, st0, k0 = opened()                     # before the option is ever set
        rows1, st1, k1 = opened(team_chacha=True)
        assert list(st0) == list(st1) == want_st
        assert np.array_equal(rows0, rows1)
        for i, kind in enumerate(kinds):
            if want_st[i] == 0:
                assert np.array_equal(rows1[i], b.leader_in[i]), (i, kind)
            else:
                assert not rows1[i].any(), (i, kind)
        # key groups on the GPU: ids 11, 12 and 14 without the flag, and 13 with it
        assert k0["k_hpke_open_team_shares"] == 3 and k1["k_hpke_open_team_shares"] == 4
        # without the global key the stale task key's reports stay failed
        rows, st = UploadBatch(v, TASK_ID, keys, team_chacha=True).open_reports(arg)
        assert list(st) == [4 if kind == "rescued" else s for kind, s in zip(kinds, want_st)]
    finally:
        v.close()
