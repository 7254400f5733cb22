"""The GPU client (janus_amd/client.py, prio3gpu_seal_input_shares): input shares sealed from their
rows without materialising a frame, against the host seal of the Python-built frames; whole
reports from ClientBatch.prepare_reports, opened on the host and checked against the oracle's
shard; and the reference's integration property end to end -- reports from the GPU client
through the leader's and the helper's aggregate-init sum to the plaintext aggregate."""
import functools

import numpy as np
import pytest

from janus_amd import client as CL
from janus_amd import codec as C
from janus_amd import hpke as H
from oracle import prio3 as O
from tests.reports import CONFIGS, make_batch, meas_array, plaintext_sum

pytestmark = pytest.mark.gpu

# SumVec(bits 1, length 9) is no entry of tests/reports.py's table (other tests enumerate it)
LOCAL_CONFIGS = {"countvec9": dict(kind=2, ctor=lambda: O.Prio3.new_sum_vec(1, 9, 3), bits=1,
                                   length=9, chunk=3)}
INSTANCES = ["count", "sum8", "hist4", "countvec9"]   # Count, Sum(8), Histogram(4), SumVec(1, 9)
TASK_ID = bytes(range(60, 92))
PRECISION = 300
LEADER_INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
HELPER_INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)


@functools.lru_cache(maxsize=None)
def _batch(name, n):
    if name not in LOCAL_CONFIGS:
        return make_batch(name, n)
    CONFIGS[name] = LOCAL_CONFIGS[name]         # make_batch looks its instance up by name
    try:
        return make_batch(name, n)
    finally:
        del CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _keys():
    return (H.generate_hpke_config_and_private_key(11, H.KEM_X25519_HKDF_SHA256, 1, 1),
            H.generate_hpke_config_and_private_key(12, H.KEM_X25519_HKDF_SHA256, 3, 3))


def _vdaf(name, b):
    from janus_amd.prio3 import Prio3Gpu
    c = LOCAL_CONFIGS.get(name) or CONFIGS[name]
    return Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                    chunk_length=c["chunk"])


def _times(n):
    return np.array([1_700_000_000 + 977 * i for i in range(n)], np.uint64)


def _sk_es(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (2, n, 32), dtype=np.uint8)


# ---- 1. seal_input_shares_gpu --------------------------------------------------------------------
@pytest.mark.parametrize("name", INSTANCES)
def test_seal_input_shares_matches_host_seal_of_the_frames(name):
    n = 65
    b = _batch(name, 130)
    v = _vdaf(name, b)
    try:
        times, sk = _times(n), _sk_es(n, 5)
        pub = b.public[:n] if b.public.shape[1] else None
        for kp, role, info, rows, k in ((_keys()[0], H.ROLE_LEADER, LEADER_INFO, b.leader_in, 0),
                                        (_keys()[1], H.ROLE_HELPER, HELPER_INFO, b.helper_in, 1)):
            slen = rows.shape[1]
            plen = 6 + slen + 16
            # shares at a pitch larger than the row; enc and payload columns at odd byte offsets
            # of a wider buffer
            wide_in = np.full((n, slen + 23), 0x5A, np.uint8)
            wide_in[:, 7:7 + slen] = rows[:n]
            out = np.full((n, 3 + 32 + 5 + plen + 9), 0xC3, np.uint8)
            encs, pays = out[:, 3:35], out[:, 40:40 + plen]
            _, _, st = H.seal_input_shares_gpu(v, TASK_ID, kp.config, role, b.nonces[:n], times,
                                               pub, wide_in[:, 7:7 + slen], sk[k], encs, pays)
            assert not st[:n].any()
            for i in range(n):
                pt = CL.encode_plaintext_input_share(rows[i].tobytes())
                aad = H.input_share_aad(TASK_ID, b.nonces[i].tobytes(), int(times[i]),
                                        b.public[i].tobytes())
                _, enc, ct = H.seal(kp.config, info, pt, aad,
                                    ephemeral_private_key=sk[k][i].tobytes())
                assert encs[i].tobytes() == enc and pays[i].tobytes() == ct, (role, i)
            mask = np.ones(out.shape, bool)
            mask[:, 3:35] = mask[:, 40:40 + plen] = False
            assert (out[mask] == 0xC3).all()                    # nothing outside the columns
            assert (wide_in[:, :7] == 0x5A).all() and (wide_in[:, 7 + slen:] == 0x5A).all()
    finally:
        v.close()


def test_seal_input_shares_on_device_rows():
    """The same call over torch device tensors (the outputs of the GPU shard are the intended
    input), columns of one device buffer as outputs."""
    import torch
    name, n = "sum8", 65
    b = _batch(name, 130)
    v = _vdaf(name, b)
    try:
        kp = _keys()[1]
        times, sk = _times(n), _sk_es(n, 6)[1]
        slen = b.helper_in.shape[1]
        plen = 6 + slen + 16
        hencs, hpays, _ = H.seal_input_shares_gpu(v, TASK_ID, kp.config, H.ROLE_HELPER,
                                                  b.nonces[:n], times, b.public[:n],
                                                  b.helper_in[:n], sk)
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out = torch.full((n, 1 + 32 + 4 + plen + 3), 0xC3, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_st[7] = 8                                             # skipped on entry
        torch.cuda.synchronize()
        H.seal_input_shares_gpu(v, TASK_ID, kp.config, H.ROLE_HELPER, up(b.nonces[:n]),
                                up(times.view(np.int64)), up(b.public[:n]), up(b.helper_in[:n]),
                                up(sk), out[:, 1:33], out[:, 37:37 + plen], status=d_st)
        got, st = out.cpu().numpy(), d_st.cpu().numpy()
        assert st.tolist() == [8 if i == 7 else 0 for i in range(n)]
        hencs[7], hpays[7] = 0, 0
        assert got[:, 1:33].tobytes() == hencs.tobytes()
        assert got[:, 37:37 + plen].tobytes() == hpays.tobytes()
        assert (got[:, 0] == 0xC3).all() and (got[:, 33:37] == 0xC3).all() \
            and (got[:, 37 + plen:] == 0xC3).all()
    finally:
        v.close()


# ---- 2. ClientBatch.prepare_reports --------------------------------------------------------------
def _reports(name, n=130):
    """(batch, vdaf, decoded reports, times) of prepare_reports over the oracle batch's nonces,
    measurements and randomness."""
    b = _batch(name, n)
    v = _vdaf(name, b)
    lkp, hkp = _keys()
    cb = CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION)
    times = _times(n)
    reports = cb.prepare_reports(meas_array(b), report_ids=b.nonces, times=times, rand=b.rand,
                                 sk_es=_sk_es(n, 8))
    assert reports.shape == (n, cb.report_len) and reports.dtype == np.uint8
    s = v.sizes
    assert cb.report_len == (16 + 8 + 4 + s.public_share + 2 * (1 + 2 + 32 + 4 + 6 + 16)
                             + s.leader_input_share + s.helper_input_share)
    cb.close()
    return b, v, [CL.decode_report(r.tobytes()) for r in reports], reports, times


@pytest.mark.parametrize("name", INSTANCES)
def test_prepare_reports_open_to_the_oracles_shares(name):
    b, v, decoded, raw, times = _reports(name)
    lkp, hkp = _keys()
    try:
        for i, r in enumerate(decoded):
            assert r.report_id == b.nonces[i].tobytes()
            assert r.time == int(times[i]) - int(times[i]) % PRECISION and r.time % PRECISION == 0
            assert r.public_share == b.public[i].tobytes()
            aad = H.input_share_aad(TASK_ID, r.report_id, r.time, r.public_share)
            for kp, info, ct, want in (
                    (lkp, LEADER_INFO, r.leader_encrypted_input_share, b.leader_in[i]),
                    (hkp, HELPER_INFO, r.helper_encrypted_input_share, b.helper_in[i])):
                assert ct.config_id == kp.config.id and len(ct.encapsulated_key) == 32
                pt = H.open_(kp, info, ct.encapsulated_key, ct.payload, aad)
                assert pt == CL.encode_plaintext_input_share(want.tobytes()), (name, i)
        if name == "count":                                     # the empty public share
            assert b.public.shape[1] == 0
            assert (raw[:, 24:28] == 0).all() and raw[0, 28] == lkp.config.id
    finally:
        v.close()


def test_prepare_reports_draws_what_is_missing():
    b = _batch("sum8", 130)
    v = _vdaf("sum8", b)
    lkp, hkp = _keys()
    try:
        cb = CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION)
        reports = cb.prepare_reports(meas_array(b)[:5])
        ids = set()
        for r in map(CL.decode_report, (x.tobytes() for x in reports)):
            ids.add(r.report_id)
            assert r.time % PRECISION == 0
            aad = H.input_share_aad(TASK_ID, r.report_id, r.time, r.public_share)
            pt = H.open_(hkp, HELPER_INFO, r.helper_encrypted_input_share.encapsulated_key,
                         r.helper_encrypted_input_share.payload, aad)
            assert pt[:6] == b"\0\0" + (len(pt) - 6).to_bytes(4, "big")
        assert len(ids) == 5
        cb.close()
    finally:
        v.close()


# ---- 3. end to end -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["countvec9", "sum8"])
def test_reports_aggregate_to_the_plaintext_sum(name):
    from janus_amd.helper import HelperAggregateInit
    b, v, decoded, _, _ = _reports(name)
    lkp, hkp = _keys()
    n, s = b.n, v.sizes
    try:
        nonces = np.frombuffer(b"".join(r.report_id for r in decoded), np.uint8).reshape(n, 16)
        times = [r.time for r in decoded]
        pub = np.frombuffer(b"".join(r.public_share for r in decoded),
                            np.uint8).reshape(n, s.public_share)
        leader_in = np.zeros((n, s.leader_input_share), np.uint8)
        for i, r in enumerate(decoded):                         # the leader's upload-time open
            ct = r.leader_encrypted_input_share
            pt = H.open_(lkp, LEADER_INFO, ct.encapsulated_key, ct.payload,
                         H.input_share_aad(TASK_ID, r.report_id, r.time, r.public_share))
            assert pt[:6] == b"\0\0" + s.leader_input_share.to_bytes(4, "big")
            leader_in[i] = np.frombuffer(pt[6:], np.uint8)
        ls, lagg, hagg = v.new_state(0, n), v.new_aggregate(1), v.new_aggregate(1)
        lp, lst = v.prepare_init(ls, nonces, pub, leader_in)
        assert not lst.any()
        req = C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", nonces, times, pub,
                                    [tuple(r.helper_encrypted_input_share) for r in decoded], lp)
        drv = HelperAggregateInit(v, TASK_ID, [hkp], hpke="fused", hpke_gpu_suites=1)
        resp = drv.handle(req, hagg)
        drv.close()
        msgs, st = C.gather_helper_resps(s, resp, nonces, np.zeros(n, np.uint8))
        assert not st.any()
        v.prepare_next(ls, msgs, lst, want_output_shares=False, agg=lagg)
        (la, lc), (ha, hc) = lagg.read(0), hagg.read(0)
        assert lc == n and hc == n
        assert v.unshard([la, ha]) == plaintext_sum(b)
        ls.close()
    finally:
        v.close()
