"""The helper driver's fused mode (prio3gpu_helper_init_request) for tasks whose only key is of a
wider X25519 suite: with `hpke_gpu_suites=1` the job's responses, statuses and aggregates are
byte-identical to hpke="host" and the device did the open (k_x25519_idx and k_hpke_open_req launch
once per job); with the option off the same job is opened on the host threads, with the same
answer."""
import ctypes

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import lib
from janus_amd.helper import HelperAggregateInit
from tests.reports import expected_aggregate
from tests.test_gpu_helper_request import (TASK_ID, _batch, _vdaf, both, encode_request, items_of,
                                           same)

pytestmark = pytest.mark.gpu


def _launches(ctx):
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    k = lib().prio3gpu_prof_read(ctx, ms, launches, 64)
    assert k > 0
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}


def _drive(v, b, reqs, jobs, tk, mode, suites):
    drv = HelperAggregateInit(v, TASK_ID, [tk], hpke_threads=4, hpke=mode, hpke_gpu_suites=suites)
    hagg = v.new_aggregate(1)
    L, ctx = lib(), v._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)  # drain
        resps = drv.handle_jobs(reqs, hagg)
        got = _launches(ctx)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    st = np.zeros(b.n, np.uint8)
    for j, resp in zip(jobs, resps):
        _, st[j] = C.gather_helper_resps(v.sizes, resp, b.nonces[j],
                                         np.zeros(j.stop - j.start, np.uint8))
    out = ([bytes(r) for r in resps], st.tolist(), hagg.read(0), hagg.read_reports(0))
    drv.close()
    hagg.close()
    return out, got


@pytest.mark.parametrize("name,n,jobs", [("sumvec_small", 24, [slice(0, 8), slice(8, 16),
                                                              slice(16, 24)]),
                                         ("count", 24, [slice(0, 24)])])
@pytest.mark.parametrize("kdf,aead", [(2, 3), (3, 2)])
def test_fused_driver_wider_suite_matches_host(name, n, jobs, kdf, aead):
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(3, H.KEM_X25519_HKDF_SHA256, kdf, aead)
    times = list(range(1000, 1000 + b.n))
    items = items_of(b, times, lambda r: tk)
    items[4]["cid"] = 9                                                  # unknown config id
    items[13]["payload"] = items[13]["payload"][:-1] + b"\x00"           # bad tag
    reqs = [encode_request(items[j]) for j in jobs]
    try:
        host, lh = _drive(v, b, reqs, jobs, tk, "host", 0)
        assert lh["k_hpke_open_req"] == 0 and lh["k_x25519_idx"] == 0
        on, lon = _drive(v, b, reqs, jobs, tk, "fused", 1)
        assert on == host
        assert lon["k_hpke_open_req"] == len(jobs) and lon["k_x25519_idx"] == len(jobs)
        off, loff = _drive(v, b, reqs, jobs, tk, "fused", 0)
        assert off == host
        assert loff["k_hpke_open_req"] == 0 and loff["k_x25519_idx"] == 0
        assert loff["k_req_gather"] == len(jobs)                         # still the fused call
    finally:
        v.close()
    st = np.array(on[1])
    assert st[4] == 3 and st[13] == 4 and (np.delete(st, [4, 13]) == 0).all()
    exp, ecnt = expected_aggregate(b, "helper", mask=st == 0)
    got, cnt = on[2]
    assert got == exp and cnt == ecnt == b.n - 2


def _staged_on_host(v, req_bytes, tks, gks):
    """test_gpu_helper_request.staged with the open on the host threads."""
    req = C.decode_agg_init_req(req_bytes)
    nonces, pub, lps, faults = C.gather_prepare_inits(v.sizes, req)
    pts, offs, st = H.open_report_shares(TASK_ID, req, tks, gks, np.zeros(req.n, np.uint8),
                                         threads=2)
    hin, st = C.decode_plaintext_input_shares_raw(v.sizes, pts, offs, 1, st)
    C.apply_faults(st, faults)
    state, agg = v.new_state(1, req.n), v.new_aggregate(1)
    msgs, st = v.helper_init(state, nonces, pub, hin, lps, agg=agg, status=st)
    out = (msgs, st.copy(), nonces, [agg.read(0)])
    state.close()
    agg.close()
    return out


def test_key_groups_of_several_suites_in_one_call():
    """Two GPU key groups of different suites, a P-256 key for the host and the second trial with
    a global key of another suite, in one call: prio3gpu_hpke_open_report_shares_gpu and the fused
    call both answer as the host path does."""
    name, n = "count", 12
    b = _batch(name, n)
    v = _vdaf(name, b)
    x25519 = H.KEM_X25519_HKDF_SHA256
    tk1 = H.generate_hpke_config_and_private_key(1, x25519, 1, 1)
    tk2 = H.generate_hpke_config_and_private_key(2, x25519, 2, 3)
    gk_same_id = H.generate_hpke_config_and_private_key(1, x25519, 3, 2)   # tk1's id
    gk_p256 = H.generate_hpke_config_and_private_key(4, H.KEM_P256_HKDF_SHA256, 1, 2)
    kps = [tk1, tk2, gk_same_id, gk_p256] * 3        # 2, 6, 10: opened by the second trial
    items = items_of(b, list(range(1000, 1000 + n)), lambda r: kps[r])
    items[4]["cid"] = 77                                                 # unknown config id
    p = bytearray(items[5]["payload"])
    p[3] ^= 0x40                                                         # corrupted payload
    items[5]["payload"] = bytes(p)
    req = encode_request(items)
    tks, gks = [tk1, tk2], [gk_same_id, gk_p256]
    L, ctx = lib(), v._ctx
    try:
        host = _staged_on_host(v, req, tks, gks)
        v.set_option("hpke_gpu_suites", 1)
        assert L.prio3gpu_prof_enable(ctx, 1) == 0
        try:
            _launches(ctx)  # drain
            msgs, st, nonces, aggs = both(v, req, tks, gks)
            got = _launches(ctx)
        finally:
            L.prio3gpu_prof_enable(ctx, 0)
        same(host, (msgs, st, nonces, aggs))
    finally:
        v.close()
    assert got["k_hpke_open"] == 2 and got["k_hpke_open_req"] == 2       # tk1 (+ its id), tk2
    assert st[4] == 3 and st[5] == 4 and (np.delete(st, [4, 5]) == 0).all()
    assert aggs[0] == expected_aggregate(b, "helper", mask=st == 0)


def test_suites_option_needs_a_gpu_mode():
    b = _batch("count", 24)
    v = _vdaf("count", b)
    try:
        with pytest.raises(ValueError):
            HelperAggregateInit(v, TASK_ID, [H.generate_hpke_config_and_private_key(1)],
                                hpke="host", hpke_gpu_suites=1)
        drv = HelperAggregateInit(v, TASK_ID, [H.generate_hpke_config_and_private_key(1)],
                                  hpke="gpu", hpke_gpu_suites=1)
        drv.close()
    finally:
        v.close()
