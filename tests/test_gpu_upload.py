"""The batched upload open (janus_amd/upload.py: UploadBatch.open_reports): the report matrix of
ClientBatch.prepare_reports back to the oracle shard's input shares, as rows the leader's
prepare_init reads in place on the device; and the routing by config id -- two GPU suites, a
ChaCha20-Poly1305 key on the host, an unknown id, a task key that fails and the global key of the
same id that rescues it."""
import functools

import numpy as np
import pytest

from janus_amd import client as CL
from janus_amd import hpke as H
from janus_amd.upload import UploadBatch
from tests.reports import CONFIGS, make_batch, meas_array

pytestmark = pytest.mark.gpu

TASK_ID = bytes(range(33, 65))
PRECISION = 300
N = 33
X = H.KEM_X25519_HKDF_SHA256


@functools.lru_cache(maxsize=None)
def _batch(name):
    return make_batch(name, N)


@functools.lru_cache(maxsize=None)
def _keys():
    g = H.generate_hpke_config_and_private_key
    return dict(a=g(11, X, 1, 1), b=g(12, X, 2, 2), chacha=g(13, X, 1, 3), rescued=g(14, X, 3, 1),
                helper=g(21, X, 1, 1))


def _vdaf(name, b):
    from janus_amd.prio3 import Prio3Gpu
    c = CONFIGS[name]
    return Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                    chunk_length=c["chunk"])


def _times():
    return np.array([1_700_000_100 + 613 * i for i in range(N)], np.uint64)


def _reports(v, b, leader_kp, seed, device_out=False):
    cb = CL.ClientBatch(v, TASK_ID, leader_kp.config, _keys()["helper"].config, PRECISION)
    sk = np.random.default_rng(seed).integers(0, 256, (2, N, 32), dtype=np.uint8)
    try:
        return cb.prepare_reports(meas_array(b), report_ids=b.nonces, times=_times(), rand=b.rand,
                                  sk_es=sk, device_out=device_out)
    finally:
        cb.close()


@pytest.mark.parametrize("name", ["sumvec_small", "sum8"])
def test_reports_open_to_the_shards_shares_and_prepare_in_place(name):
    import torch
    b = _batch(name)
    v = _vdaf(name, b)
    kp = _keys()["a"]
    try:
        d_reports = _reports(v, b, kp, 1, device_out=True)
        up = UploadBatch(v, TASK_ID, [kp])
        rows, st = up.open_reports(d_reports)
        assert not st.any()
        assert rows.is_cuda and rows.shape == (N, v.sizes.leader_input_share)
        assert rows.stride(0) % 128 == 0 and rows.stride(1) == 1
        assert np.array_equal(rows.cpu().numpy(), b.leader_in)
        # the leader's prepare_init reads those device rows at their pitch
        ls = v.new_state(0, N)
        pub = b.public if b.public.shape[1] else None
        lp, lst = v.prepare_init(ls, b.nonces, pub, rows)
        assert not lst.any() and np.array_equal(lp, b.leader_prep)
        ls.close()
        # the same matrix from host memory, and the helper's column under the helper's key
        reports = d_reports.cpu().numpy()
        hrows, st = up.open_reports(reports)
        assert not st.any() and isinstance(hrows, np.ndarray)
        assert hrows.strides[0] % 128 == 0 and np.array_equal(hrows, b.leader_in)
        hup = UploadBatch(v, TASK_ID, [_keys()["helper"]], role=H.ROLE_HELPER)
        rows, st = hup.open_reports(d_reports)
        assert not st.any() and np.array_equal(rows.cpu().numpy(), b.helper_in)
        # the leader's key does not open the helper's column, nor another task's id this one
        rows, st = UploadBatch(v, TASK_ID, [_keys()["helper"]]).open_reports(reports)
        assert (st == 3).all() and not rows.any()
        rows, st = UploadBatch(v, bytes(32), [kp]).open_reports(d_reports)
        assert (st == 4).all() and not rows.cpu().numpy().any()
        assert torch.equal(d_reports.cpu(), torch.from_numpy(reports))
    finally:
        v.close()


@pytest.mark.parametrize("device", [False, True])
def test_routing_by_config_id(device):
    import torch
    name = "sumvec_small"
    b = _batch(name)
    v = _vdaf(name, b)
    k = _keys()
    try:
        per_key = {w: _reports(v, b, k[w], 10 + j) for j, w in
                   enumerate(("a", "b", "chacha", "rescued"))}
        kinds = [("a", "b", "chacha", "rescued", "unknown", "lost")[i % 6] for i in range(N)]
        reports = np.zeros_like(per_key["a"])
        o_cfg = CL.ReportLayout(v.sizes.public_share, v.sizes.leader_input_share,
                                v.sizes.helper_input_share).o_leader
        for i, kind in enumerate(kinds):
            reports[i] = per_key[{"unknown": "a", "lost": "b"}.get(kind, kind)][i]
            if kind == "unknown":
                reports[i, o_cfg] = 99
            elif kind == "lost":                      # sealed to b, claims a's id: no key opens it
                reports[i, o_cfg] = k["a"].config.id
        # id 14: the task key is another keypair under the rescued key's id and suite
        stale = H.generate_hpke_config_and_private_key(14, X, 3, 1)
        up = UploadBatch(v, TASK_ID, [k["a"], k["b"], k["chacha"], stale],
                         global_keys=[k["rescued"], k["a"]])
        arg = torch.from_numpy(reports).to(torch.device("cuda", v.device)) if device else reports
        rows, st = up.open_reports(arg)
        rows = rows.cpu().numpy() if device else rows
        want = {"a": 0, "b": 0, "chacha": 0, "rescued": 0, "unknown": 3, "lost": 4}
        assert list(st) == [want[kind] for kind in kinds]
        for i, kind in enumerate(kinds):
            if want[kind] == 0:
                assert np.array_equal(rows[i], b.leader_in[i]), (i, kind)
            else:
                assert not rows[i].any(), (i, kind)
        # without the global key the stale task key's reports stay failed
        rows, st = UploadBatch(v, TASK_ID, [k["a"], k["b"], k["chacha"], stale]).open_reports(arg)
        assert list(st) == [4 if kind == "rescued" else want[kind] for kind in kinds]
    finally:
        v.close()
