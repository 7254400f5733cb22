"""prio3gpu_helper_init_request (janus_amd/csrc/helper_request.h): the helper's aggregate-init in
one call from the request's bytes, against the staged path built from the existing calls
  gather_prepare_inits -> open_report_shares(gpu=) -> decode_plaintext_input_shares ->
  apply_faults -> helper_init
Per-report statuses, the prep messages of the accepted reports, the report IDs and every slot's
aggregate share and count must be identical."""
import ctypes
import functools
import math

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import Prio3GpuError, lib
from tests.reports import CONFIGS, Batch, expected_aggregate, make_batch

pytestmark = pytest.mark.gpu

INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
TASK_ID = bytes(range(100, 132))


def _vdaf(name, b):
    from janus_amd.prio3 import Prio3Gpu
    c = CONFIGS[name]
    return Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                    chunk_length=c["chunk"])


@functools.lru_cache(maxsize=None)
def _batch(name, n):
    return make_batch(name, n)


def _head(b: Batch, n):
    """The first n reports of a batch (the arrays the requests are built from)."""
    return Batch(b.name, b.vdaf, b.verify_key, n, b.measurements[:n], b.nonces[:n], b.public[:n],
                 b.leader_in[:n], b.helper_in[:n], b.leader_prep[:n], b.helper_prep[:n],
                 b.prep_msg[:n], b.leader_out[:n], b.helper_out[:n])


# ---- requests ------------------------------------------------------------------------------------
def ext(t, data=b""):
    return t.to_bytes(2, "big") + len(data).to_bytes(2, "big") + data


def plaintext(payload, exts=(), trailing=b""):
    body = b"".join(exts)
    return (len(body).to_bytes(2, "big") + body + len(payload).to_bytes(4, "big") + payload
            + trailing)


def items_of(b, times, keypair_of, pt_of=None):
    """One dict per report: the PrepareInit's fields, the input share sealed to keypair_of(r)."""
    out = []
    for r in range(b.n):
        pub = b.public[r].tobytes()
        pt = pt_of(r) if pt_of else plaintext(b.helper_in[r].tobytes())
        kp = keypair_of(r)
        aad = H.input_share_aad(TASK_ID, b.nonces[r].tobytes(), times[r], pub)
        cid, enc, payload = H.seal(kp.config, INFO, pt, aad)
        out.append(dict(id=b.nonces[r].tobytes(), time=times[r], pub=pub, cid=cid, enc=enc,
                        payload=payload, mtype=0, prep_share=b.leader_prep[r].tobytes(),
                        prep_msg=b""))
    return out


def reseal(it, keypair, pt):
    aad = H.input_share_aad(TASK_ID, it["id"], it["time"], it["pub"])
    it["cid"], it["enc"], it["payload"] = H.seal(keypair.config, INFO, pt, aad)


def encode_request(items):
    """AggregationJobInitializeReq (TimeInterval, empty aggregation parameter): the layout of
    codec.cpp's header comment, with per-report lengths and ping-pong message types."""
    u32 = lambda x: len(x).to_bytes(4, "big") + x
    body = b""
    for it in items:
        share = (it["id"] + it["time"].to_bytes(8, "big") + u32(it["pub"]) + bytes([it["cid"]])
                 + len(it["enc"]).to_bytes(2, "big") + it["enc"] + u32(it["payload"]))
        if it["mtype"] == 0:
            pp = b"\x00" + u32(it["prep_share"])
        elif it["mtype"] == 1:
            pp = b"\x01" + u32(it["prep_msg"]) + u32(it["prep_share"])
        else:
            pp = b"\x02" + u32(it["prep_msg"])
        body += share + pp
    return u32(b"") + b"\x01" + u32(body)


# ---- the two paths -------------------------------------------------------------------------------
def staged(v, req_bytes, tks, gks=(), st0=None, slots=None, nslots=1):
    req = C.decode_agg_init_req(req_bytes)
    s = v.sizes
    nonces, pub, lps, faults = C.gather_prepare_inits(s, req)
    st = np.zeros(req.n, np.uint8) if st0 is None else st0.copy()
    pts, offs, st = H.open_report_shares(TASK_ID, req, tks, gks, st, threads=2, gpu=v)
    hin, st = C.decode_plaintext_input_shares_raw(s, pts, offs, 1, st)
    C.apply_faults(st, faults)
    state, agg = v.new_state(1, req.n), v.new_aggregate(nslots)
    msgs, st = v.helper_init(state, nonces, pub, hin, lps, agg=agg, batch_slots=slots, status=st)
    out = (msgs, st.copy(), nonces, [agg.read(k) for k in range(nslots)])
    state.close()
    agg.close()
    return out


def fused(v, req_bytes, tks, gks=(), st0=None, slots=None, nslots=1, msg=None, cap=None):
    req = C.decode_agg_init_req(req_bytes)
    st = np.zeros(req.n, np.uint8) if st0 is None else st0.copy()
    state, agg = v.new_state(1, cap or req.n), v.new_aggregate(nslots)
    msgs, st, nonces = v.helper_init_request(state, TASK_ID, req, tks, gks, agg=agg,
                                             batch_slots=slots, status=st, threads=2, msg=msg)
    out = (msgs, st.copy(), nonces, [agg.read(k) for k in range(nslots)])
    state.close()
    agg.close()
    return out


def same(a, b):
    """Statuses, report IDs, aggregates; the prep messages of the accepted reports."""
    assert a[1].tolist() == b[1].tolist()
    assert a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3]
    if a[0] is None:
        assert b[0] is None
    else:
        ok = a[1] == 0
        assert a[0][ok].tobytes() == b[0][ok].tobytes()


def both(v, req_bytes, tks, gks=(), **kw):
    a, f = staged(v, req_bytes, tks, gks, **kw), fused(v, req_bytes, tks, gks, **kw)
    same(a, f)
    return f


# ---- 1. the driver -------------------------------------------------------------------------------
def test_helper_driver_fused_matches_host():
    from janus_amd.helper import HelperAggregateInit
    name = "sumvec_small"
    b = _batch(name, 24)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(3)
    times = list(range(1000, 1000 + b.n))
    items = items_of(b, times, lambda r: tk)
    items[4]["cid"] = 9                                                  # unknown config id
    items[13]["payload"] = items[13]["payload"][:-1] + b"\x00"           # bad tag
    jobs = [slice(0, 8), slice(8, 16), slice(16, 24)]
    reqs = [encode_request(items[j]) for j in jobs]
    cts = [(it["cid"], it["enc"], it["payload"]) for it in items]
    assert reqs[0] == C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", b.nonces[jobs[0]],
                                            times[jobs[0]], b.public[jobs[0]], cts[jobs[0]],
                                            b.leader_prep[jobs[0]])
    out = {}
    for mode in ("host", "fused"):
        drv = HelperAggregateInit(v, TASK_ID, [tk], hpke_threads=4, hpke=mode)
        hagg = v.new_aggregate(1)
        resps = drv.handle_jobs(reqs, hagg)
        st = np.zeros(b.n, np.uint8)
        for j, resp in zip(jobs, resps):
            _, st[j] = C.gather_helper_resps(v.sizes, resp, b.nonces[j], np.zeros(8, np.uint8))
        out[mode] = ([bytes(r) for r in resps], st.tolist(), hagg.read(0), hagg.read_reports(0))
        drv.close()
    assert out["fused"] == out["host"]
    st = np.array(out["fused"][1])
    assert st[4] == 3 and st[13] == 4 and (np.delete(st, [4, 13]) == 0).all()
    exp, ecnt = expected_aggregate(b, "helper", mask=st == 0)
    got, cnt = out["fused"][2]
    assert got == exp and cnt == ecnt == b.n - 2
    v.close()


# ---- 2. status precedence ------------------------------------------------------------------------
def test_status_precedence():
    name = "sum8"
    n = 40
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(7)
    times = [1_700_000_000 + r for r in range(n)]
    items = items_of(b, times, lambda r: tk)
    hin = lambda r: b.helper_in[r].tobytes()
    want = {}
    items[2]["cid"] = 99; want[2] = 3                                    # unknown id
    items[4]["payload"] = items[4]["payload"][:-1] + bytes([items[4]["payload"][-1] ^ 1])
    want[4] = 4                                                          # bad tag
    for r, ln in ((6, 0), (7, 1), (8, 15)):                              # shorter than a tag
        items[r]["payload"] = items[r]["payload"][:ln]; want[r] = 4
    reseal(items[9], tk, b""); want[9] = 8                               # the tag of an empty pt
    assert len(items[9]["payload"]) == 16
    reseal(items[11], tk, plaintext(hin(11), [ext(1), ext(2, b"x"), ext(1, b"yy")])); want[11] = 8
    reseal(items[13], tk, plaintext(hin(13)[:-1])); want[13] = 8         # payload length - 1
    reseal(items[14], tk, plaintext(hin(14) + b"\x00")); want[14] = 8    # payload length + 1
    reseal(items[16], tk, plaintext(hin(16), trailing=b"\x00")); want[16] = 8
    items[18]["pub"] = items[18]["pub"] + b"\x00"                        # wrong public-share length
    reseal(items[18], tk, plaintext(hin(18))); want[18] = 8              # (its AAD still opens)
    items[20]["prep_share"] = items[20]["prep_share"][:-1]; want[20] = 5
    items[21]["mtype"] = 1; items[21]["prep_msg"] = bytes(16); want[21] = 5   # Continue
    items[23]["pub"] = items[23]["pub"][:-1]                             # bad tag + public share
    reseal(items[23], tk, plaintext(hin(23)))
    items[23]["payload"] = items[23]["payload"][:-2] + b"\x00\x01"; want[23] = 4
    reseal(items[25], tk, plaintext(hin(25), [ext(5), ext(5)]))          # duplicate + prep share
    items[25]["prep_share"] = items[25]["prep_share"] + b"\x00"; want[25] = 8
    st0 = np.zeros(n, np.uint8)
    st0[27] = 7; want[27] = 7                                            # rejected before the call
    reseal(items[29], tk, plaintext(hin(29), [ext(1), ext(2, b"abc")]))  # valid extensions
    msgs, st, nonces, aggs = both(v, encode_request(items), [tk], st0=st0)
    for r in range(n):
        assert st[r] == want.get(r, 0), r
    mask = st == 0
    assert aggs[0] == expected_aggregate(b, "helper", mask=mask)
    assert msgs[mask].tobytes() == b.prep_msg[mask].tobytes()
    assert nonces.tobytes() == b.nonces.tobytes()
    v.close()


# ---- 3. key selection ----------------------------------------------------------------------------
def test_key_selection():
    name = "count"
    n = 200
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(1)
    gk = H.generate_hpke_config_and_private_key(2, H.KEM_P256_HKDF_SHA256, 1, 2)
    gk_same_id = H.generate_hpke_config_and_private_key(1)
    kps = [tk if i % 3 == 0 else gk if i % 3 == 1 else gk_same_id for i in range(n)]
    times = [1_700_000_000 + i for i in range(n)]
    items = items_of(b, times, lambda r: kps[r])
    items[5]["cid"] = 77                                                 # unknown config id
    p = bytearray(items[7]["payload"])
    p[3] ^= 0x40                                                         # corrupted payload
    items[7]["payload"] = bytes(p)
    req = encode_request(items)
    st0 = np.zeros(n, np.uint8)
    st0[9] = 8
    msgs, st, _, aggs = both(v, req, [tk], [gk, gk_same_id], st0=st0)
    assert st[5] == 3 and st[7] == 4 and st[9] == 8
    ok = [i for i in range(n) if i not in (5, 7, 9)]
    assert (st[ok] == 0).all()
    assert aggs[0] == expected_aggregate(b, "helper", mask=st == 0)
    # no global keys: gk's reports have an unknown id, gk_same_id's fail to decrypt
    _, st2, _, aggs2 = both(v, req, [tk], [])
    assert all(st2[i] == 3 for i in range(n) if i % 3 == 1 and i != 7)
    assert all(st2[i] == 4 for i in range(n) if i % 3 == 2 and i != 5)
    assert aggs2[0] == expected_aggregate(b, "helper", mask=st2 == 0)
    v.close()


# ---- 4. extensions -------------------------------------------------------------------------------
def list_of(nbytes, dup=False):
    items = [ext(k + 1) for k in range(nbytes // 4)]
    if dup:
        items[-1] = items[0]
    return items


def test_extensions_move_the_payload():
    name = "sum8"
    lens = [0] + list(range(4, 20))
    n = len(lens) + 4
    b = _batch(name, 40)
    b = _head(b, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(4)
    lists = [[] if ln == 0 else [ext(9, b"\xa5" * (ln - 4))] for ln in lens]
    assert {(6 + ln) % 16 for ln in lens} == set(range(16))              # every payload offset
    lists += [list_of(256), list_of(256, dup=True), list_of(260), list_of(260, dup=True)]
    want = [0] * len(lens) + [0, 8, 0, 8]
    times = [5000 + r for r in range(n)]
    items = items_of(b, times, lambda r: tk,
                     pt_of=lambda r: plaintext(b.helper_in[r].tobytes(), lists[r]))
    msgs, st, _, aggs = both(v, encode_request(items), [tk])
    assert st.tolist() == want
    assert aggs[0] == expected_aggregate(b, "helper", mask=st == 0)
    v.close()


# ---- 5. gather alignment, ragged waves -----------------------------------------------------------
def _run_plain(name, n, nmax, exts=()):
    b = _head(_batch(name, nmax), n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(2)
    items = items_of(b, [7000 + r for r in range(n)], lambda r: tk,
                     pt_of=lambda r: plaintext(b.helper_in[r].tobytes(), exts))
    req_bytes = encode_request(items)
    msgs, st, nonces, aggs = both(v, req_bytes, [tk])
    assert (st == 0).all()
    assert nonces.tobytes() == b.nonces.tobytes()
    if msgs is not None:
        assert msgs.tobytes() == b.prep_msg.tobytes()
    assert aggs[0] == expected_aggregate(b, "helper")
    req = C.decode_agg_init_req(req_bytes)
    v.close()
    return req


# Every length of a Prio3 PrepareInit is even (seeds and Field128 elements are 16 bytes, Field64
# elements 8, the framing 94), so no config alone gives an odd stride: each report of this test
# carries one extension with one byte of data (5 bytes), which makes hist4's stride odd.
ODD = "hist4"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_gather_odd_stride(n):
    req = _run_plain(ODD, n, 130, exts=[ext(3, b"\x77")])
    if n > 1:
        stride = req.views[1].report_id_off - req.views[0].report_id_off
        assert math.gcd(stride, 16) == 1, stride
        offs = {req.views[i].prep_share_off % 16 for i in range(min(n, 16))}
        assert len(offs) == min(n, 16)       # the source rows start at every byte alignment


@pytest.mark.parametrize("name", ["count", "hist4", "sumvec_calls1", "fp16_3"])
@pytest.mark.parametrize("n", [3, 65])
def test_gather_row_shapes(name, n):
    _run_plain(name, n, 130 if name == ODD else 65)


def _gather_gpu(v, req, msg=None, msg_len=None):
    s, n, L = v.sizes, req.n, lib()
    nonces = np.full((n, 16), 0xAA, np.uint8)
    pub = np.full((n, s.public_share), 0xAA, np.uint8)
    lps = np.full((n, s.prep_share), 0xAA, np.uint8)
    faults = np.full(n, 0xAA, np.uint8)
    rc = L.prio3gpu_test_req_gather(v._ctx, req.raw.ctypes.data if msg is None else msg,
                                    req.raw.size if msg_len is None else msg_len, req.views, n,
                                    nonces.ctypes.data, pub.ctypes.data, lps.ctypes.data,
                                    faults.ctypes.data)
    assert rc == 0, L.prio3gpu_last_error()
    return nonces, pub, lps, faults


@pytest.mark.parametrize("name", ["hist4", "count", "fp16_3"])
def test_gathered_rows_equal_the_host_gather(name):
    """k_req_gather alone, row for row against prio3gpu_gather_prepare_inits: odd stride, faulty
    reports (rows zeroed), the request in host memory and at odd device addresses.  The first
    report ID and the last (intact) prep share touch the two ends of the message, where the
    aligned window does not fit and the guarded path runs."""
    n = 65
    b = _head(_batch(name, 130 if name == ODD else 65), n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(2)
    items = items_of(b, [7000 + r for r in range(n)], lambda r: tk,
                     pt_of=lambda r: plaintext(b.helper_in[r].tobytes(), [ext(3, b"\x77")]))
    items[0]["prep_share"] = items[0]["prep_share"][:-1]          # 5
    items[7]["mtype"] = 1
    items[7]["prep_msg"] = bytes(16)                              # 5
    items[9]["pub"] = items[9]["pub"] + b"\x01"                   # 8
    items[n - 2]["prep_share"] = items[n - 2]["prep_share"] + b"\x02"   # 5
    req = C.decode_agg_init_req(encode_request(items))
    want = C.gather_prepare_inits(v.sizes, req)
    assert want[3][[0, 7, 9, n - 2]].tolist() == [5, 5, 8, 5] and want[3].sum() == 23
    got = _gather_gpu(v, req)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    L, ctx = lib(), v._ctx
    p = ctypes.c_void_p()
    assert L.prio3gpu_dev_alloc(ctx, req.raw.size + 16, ctypes.byref(p)) == 0
    try:
        for shift in (1, 2, 3):
            assert L.prio3gpu_memcpy(ctx, p.value + shift, req.raw.ctypes.data, req.raw.size) == 0
            got = _gather_gpu(v, req, msg=p.value + shift)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), shift
    finally:
        L.prio3gpu_dev_free(ctx, p)
    v.close()


# ---- 6. batch slots ------------------------------------------------------------------------------
def test_batch_slots():
    name = "sum8"
    n = 40
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(6)
    items = items_of(b, [100 + r for r in range(n)], lambda r: tk)
    items[3]["payload"] = items[3]["payload"][:-1] + b"\x00"
    slots = (np.arange(n) % 2).astype(np.uint32)
    _, st, _, aggs = both(v, encode_request(items), [tk], slots=slots, nslots=2)
    for k in (0, 1):
        assert aggs[k] == expected_aggregate(b, "helper", mask=st == 0, slots=slots, slot=k)
    v.close()


# ---- 7. the request in device memory -------------------------------------------------------------
def test_request_as_device_pointer():
    name = "sum8"
    n = 40
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(6)
    gk = H.generate_hpke_config_and_private_key(6)
    items = items_of(b, [100 + r for r in range(n)], lambda r: gk if r == 5 else tk)  # a retry
    items[3]["payload"] = items[3]["payload"][:-1] + b"\x00"
    req_bytes = encode_request(items)
    host = fused(v, req_bytes, [tk], [gk])
    L, ctx = lib(), v._ctx
    raw = np.frombuffer(req_bytes, np.uint8)
    p = ctypes.c_void_p()
    assert L.prio3gpu_dev_alloc(ctx, raw.size, ctypes.byref(p)) == 0
    try:
        assert L.prio3gpu_memcpy(ctx, p, raw.ctypes.data, raw.size) == 0
        dev = fused(v, req_bytes, [tk], [gk], msg=p.value)
    finally:
        L.prio3gpu_dev_free(ctx, p)
    same(host, dev)
    assert host[1][3] == 4 and host[1][5] == 0 and (np.delete(host[1], 3) == 0).all()
    v.close()


# ---- 8. bounds -----------------------------------------------------------------------------------
def test_view_past_the_message_launches_nothing():
    name = "sum8"
    n = 40
    b = _batch(name, n)
    v = _vdaf(name, b)
    tk = H.generate_hpke_config_and_private_key(6)
    req = C.decode_agg_init_req(encode_request(items_of(b, [1] * n, lambda r: tk)))
    state, agg = v.new_state(1, n), v.new_aggregate(1)
    L, ctx = lib(), v._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        for field, val in (("payload_len", req.raw.size), ("payload_off", 2**63),
                           ("prep_share_off", req.raw.size - 3), ("report_id_off", 2**64 - 8)):
            view = req.views[17]
            old = getattr(view, field)
            setattr(view, field, val)
            assert view.payload_off + view.payload_len > req.raw.size or field != "payload_len"
            with pytest.raises(Prio3GpuError, match=r"\(-1\)"):
                v.helper_init_request(state, TASK_ID, req, [tk], agg=agg)
            setattr(view, field, old)
        assert L.prio3gpu_prof_read(ctx, ms, launches, 64) > 0
        assert sum(launches) == 0
        # an empty job: 0 and nothing launched
        tkc, keep = H._keypairs([tk])
        tid = np.frombuffer(TASK_ID, np.uint8).copy()
        st = np.zeros(1, np.uint8)
        rc = L.prio3gpu_helper_init_request(ctx, state._h, tid.ctypes.data, tkc, 1, None, 0,
                                            H.ROLE_CLIENT, H.ROLE_HELPER, req.raw.ctypes.data,
                                            req.raw.size, req.views, 0, None, None, None,
                                            st.ctypes.data, agg._h, 1)
        assert rc == 0
        assert L.prio3gpu_prof_read(ctx, ms, launches, 64) > 0
        assert sum(launches) == 0
        del keep
        # and the intact request still runs on the same state
        _, st, _ = v.helper_init_request(state, TASK_ID, req, [tk], agg=agg)
        assert (st == 0).all() and agg.read(0) == expected_aggregate(b, "helper")
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    state.close()
    agg.close()
    v.close()
