"""ClientBatch(p256=True) and UploadBatch(p256=True) (janus_amd/client.py, upload.py): reports sealed
on the GPU to DHKEM(P-256, HKDF-SHA256) configs, a lane per report (130 Count reports) and a wave
per report (66 small SumVec reports under long_seal=True), for a P-256 leader with an X25519
helper, the reverse, and both P-256.  Every report decodes, both ciphertexts are the host seal's
under the same ephemeral keys and open to the shard's shares, and the upload open returns those
shares; without `p256` both classes behave as before."""
import ctypes
import functools

import numpy as np
import pytest

from janus_amd import client as CL
from janus_amd import hpke as H
from janus_amd._lib import lib
from janus_amd.upload import UploadBatch
from tests.reports import CONFIGS, make_batch, meas_array

pytestmark = pytest.mark.gpu

TASK_ID = bytes(range(70, 102))
PRECISION = 300
X, P = H.KEM_X25519_HKDF_SHA256, H.KEM_P256_HKDF_SHA256
KEMS = [(P, X), (X, P), (P, P)]
CASES = [("count", 130, False), ("sumvec_small", 66, True)]


@functools.lru_cache(maxsize=None)
def _batch(name, n):
    return make_batch(name, n)


@functools.lru_cache(maxsize=None)
def _keys(lkem, hkem):
    return (H.generate_hpke_config_and_private_key(11, lkem, 1, 1),
            H.generate_hpke_config_and_private_key(12, hkem, 2, 2))


def _vdaf(name):
    from janus_amd.prio3 import Prio3Gpu
    c, b = CONFIGS[name], _batch(name, 1)
    return Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                    chunk_length=c["chunk"])


@pytest.fixture(scope="module", params=CASES, ids=lambda c: c[0])
def case(request):
    name, n, long_seal = request.param
    v = _vdaf(name)
    yield v, _batch(name, n), n, long_seal
    v.close()


def _launches(v, f):
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


def _sk_es(n, lkem, hkem, seed=8):
    rng = np.random.default_rng(seed)
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()   # noqa: E731
    return np.stack([CL.draw_p256_scalars(n, rnd) if kem == P else
                     np.frombuffer(rnd(32 * n), np.uint8).reshape(n, 32) for kem in (lkem, hkem)])


def _prepare(v, b, n, long_seal, lkem, hkem, sk=None):
    lkp, hkp = _keys(lkem, hkem)
    cb = CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION, long_seal=long_seal,
                        p256=True)
    times = np.array([1_700_000_000 + 977 * i for i in range(n)], np.uint64)
    try:
        return cb, cb.prepare_reports(meas_array(b), report_ids=b.nonces, times=times,
                                      rand=b.rand, sk_es=sk)
    finally:
        cb.close()


@pytest.mark.parametrize("lkem,hkem", KEMS, ids=["p256-x25519", "x25519-p256", "p256-p256"])
def test_reports_equal_host_seal_and_open_to_the_shares(case, lkem, hkem):
    v, b, n, long_seal = case
    lkp, hkp = _keys(lkem, hkem)
    sk = _sk_es(n, lkem, hkem)
    (cb, reports), names = _launches(v, lambda: _prepare(v, b, n, long_seal, lkem, hkem, sk))
    assert reports.shape == (n, cb.report_len)
    assert (cb.layout.leader_enc, cb.layout.helper_enc) == (H.enc_len(lkem), H.enc_len(hkem))
    n_p256 = (lkem == P) + (hkem == P)
    assert names["k_p256_eph"] == names["k_p256_eph_kem"] == n_p256
    assert names["k_x25519_eph"] == 2 - n_p256
    seal_kernel = "k_hpke_seal_team_shares" if long_seal else "k_hpke_seal_shares"
    assert names[seal_kernel] == 2
    for i in range(n):
        r = CL.decode_report(reports[i].tobytes())
        assert r.report_id == b.nonces[i].tobytes() and r.public_share == b.public[i].tobytes()
        aad = H.input_share_aad(TASK_ID, r.report_id, r.time, r.public_share)
        for k, (kp, role, ct, share) in enumerate((
                (lkp, H.ROLE_LEADER, r.leader_encrypted_input_share, b.leader_in[i]),
                (hkp, H.ROLE_HELPER, r.helper_encrypted_input_share, b.helper_in[i]))):
            info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, role)
            pt = CL.encode_plaintext_input_share(share.tobytes())
            assert ct.config_id == kp.config.id
            assert (kp.config.id, ct.encapsulated_key, ct.payload) == \
                H.seal(kp.config, info, pt, aad, ephemeral_private_key=sk[k, i].tobytes()), (i, k)
            assert H.open_(kp, info, ct.encapsulated_key, ct.payload, aad) == pt


@pytest.mark.parametrize("lkem,hkem", KEMS, ids=["p256-x25519", "x25519-p256", "p256-p256"])
def test_upload_open_returns_the_shares_and_statuses(case, lkem, hkem):
    v, b, n, long_seal = case
    lkp, hkp = _keys(lkem, hkem)
    _, reports = _prepare(v, b, n, long_seal, lkem, hkem)     # ephemeral scalars drawn inside
    for kp, role, want, peer in ((lkp, H.ROLE_LEADER, b.leader_in, hkem),
                                 (hkp, H.ROLE_HELPER, b.helper_in, lkem)):
        ub = UploadBatch(v, TASK_ID, [kp], role=role, p256=True, peer_enc=H.enc_len(peer))
        shares, st = ub.open_reports(reports)
        assert not st.any() and np.array_equal(shares, want[:n])
    # the leader's side: an unknown config id, a tampered payload, the global key's second trial
    L = CL.ReportLayout(v.sizes.public_share, v.sizes.leader_input_share,
                        v.sizes.helper_input_share, H.enc_len(lkem), H.enc_len(hkem))
    bad = reports.copy()
    bad[1, L.o_leader] = 99
    bad[2, L.o_leader_payload + 3] ^= 0x40
    other = H.generate_hpke_config_and_private_key(11, lkem, 1, 1)   # same id, another key
    ub = UploadBatch(v, TASK_ID, [other], global_keys=[lkp], role=H.ROLE_LEADER, p256=True,
                     peer_enc=H.enc_len(hkem))
    (shares, st), names = _launches(v, lambda: ub.open_reports(bad))
    want_st = np.zeros(n, np.uint8)
    want_st[1], want_st[2] = 3, 4
    assert st.tolist() == want_st.tolist()
    ok = want_st == 0
    assert np.array_equal(shares[ok], b.leader_in[:n][ok]) and not shares[~ok].any()
    if lkem == P:          # the first trial ran on the GPU; the second on the host
        assert names["k_p256_dh"] == 1 and names["k_hpke_open_team_shares"] == 1


def test_without_p256_both_classes_behave_as_before(case):
    v, b, n, long_seal = case
    lkp, hkp = _keys(P, X)
    with pytest.raises(ValueError):
        CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION)
    with pytest.raises(ValueError):
        CL.ClientBatch(v, TASK_ID, hkp.config, lkp.config, PRECISION, long_seal=long_seal)
    xl, xh = _keys(X, X)
    ub = UploadBatch(v, TASK_ID, [xl])
    assert not ub.p256 and (ub.layout.leader_enc, ub.layout.helper_enc) == (32, 32)
    assert ub.layout.report_len == CL.ReportLayout(
        v.sizes.public_share, v.sizes.leader_input_share, v.sizes.helper_input_share).report_len
    cb = CL.ClientBatch(v, TASK_ID, xl.config, xh.config, PRECISION, long_seal=long_seal)
    try:
        reports = cb.prepare_reports(meas_array(b)[:5], report_ids=b.nonces[:5], rand=b.rand[:5])
    finally:
        cb.close()
    shares, st = ub.open_reports(reports)
    assert not st.any() and np.array_equal(shares, b.leader_in[:5])


def test_invalid_caller_scalars_raise_hpke_error(case):
    v, b, n, long_seal = case
    sk = _sk_es(n, P, X)
    sk[0, n // 2] = np.frombuffer(CL.P256_ORDER.to_bytes(32, "big"), np.uint8)
    with pytest.raises(H.HpkeError):
        _prepare(v, b, n, long_seal, P, X, sk)
