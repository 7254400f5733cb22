"""The helper driver's fused mode (prio3gpu_helper_init_request) for tasks with P-256 HPKE keys:
with `hpke_gpu_p256=1` a job over two P-256 task keys and one X25519 key gives responses, statuses
and aggregates byte-identical to hpke="host", and the device did the P-256 opens (k_p256_dh_idx
launches once per P-256 key group); with the option off the same job gives the same bytes and no
P-256 kernel runs."""
import ctypes

import numpy as np
import pytest

from janus_amd import codec as C
from janus_amd import hpke as H
from janus_amd._lib import lib
from janus_amd.helper import HelperAggregateInit
from tests.reports import expected_aggregate
from tests.test_gpu_helper_request import TASK_ID, _batch, _vdaf, encode_request, items_of

pytestmark = pytest.mark.gpu

N = 130


def _launches(ctx):
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    k = lib().prio3gpu_prof_read(ctx, ms, launches, 64)
    assert k > 0
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(launches[i]) for i in range(k)}


def _drive(v, b, req, tks, mode, p256):
    drv = HelperAggregateInit(v, TASK_ID, tks, hpke_threads=4, hpke=mode, hpke_gpu_p256=p256)
    hagg = v.new_aggregate(1)
    L, ctx = lib(), v._ctx
    assert L.prio3gpu_prof_enable(ctx, 1) == 0
    try:
        _launches(ctx)  # drain
        resps = drv.handle_jobs([req], hagg)
        got = _launches(ctx)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    _, st = C.gather_helper_resps(v.sizes, resps[0], b.nonces, np.zeros(b.n, np.uint8))
    out = ([bytes(r) for r in resps], st.tolist(), hagg.read(0), hagg.read_reports(0))
    drv.close()
    hagg.close()
    return out, got


@pytest.mark.parametrize("name", ["count", "sum8"])
def test_fused_driver_p256_matches_host(name):
    b = _batch(name, N)
    v = _vdaf(name, b)
    p256 = H.KEM_P256_HKDF_SHA256
    tka = H.generate_hpke_config_and_private_key(1, p256, 1, 1)
    tkb = H.generate_hpke_config_and_private_key(2, p256, 1, 1)
    tkx = H.generate_hpke_config_and_private_key(3, H.KEM_X25519_HKDF_SHA256, 1, 1)
    tks = [tka, tkb, tkx]
    items = items_of(b, list(range(1000, 1000 + N)), lambda r: tks[r % 3])
    enc = bytearray(items[6]["enc"])                                     # tka: off the curve
    enc[64] ^= 1
    items[6]["enc"] = bytes(enc)
    items[7]["enc"] = items[7]["enc"][:64]                               # tkb: enc_len 64
    items[13]["payload"] = items[13]["payload"][:-1] + bytes([items[13]["payload"][-1] ^ 1])
    items[20]["cid"] = 9                                                 # unknown config id
    bad = {6: 4, 7: 4, 13: 4, 20: 3}
    req = encode_request(items)
    try:
        host, lh = _drive(v, b, req, tks, "host", 0)
        assert lh["k_p256_dh_idx"] == 0 and lh["k_hpke_open_req"] == 0
        on, lon = _drive(v, b, req, tks, "fused", 1)
        assert on == host
        assert lon["k_p256_dh_idx"] == 2 and lon["k_x25519_idx"] == 1
        assert lon["k_hpke_open_req"] == 3 and lon["k_p256_dh"] == 0
        off, loff = _drive(v, b, req, tks, "fused", 0)
        assert off == host
        assert loff["k_p256_dh_idx"] == 0 and loff["k_p256_dh"] == 0
        assert loff["k_x25519_idx"] == 1 and loff["k_hpke_open_req"] == 1
        assert loff["k_req_gather"] == 1                                 # still the fused call
    finally:
        v.close()
    st = np.array(on[1])
    for i, s in bad.items():
        assert st[i] == s, i
    assert (np.delete(st, list(bad)) == 0).all()
    exp, ecnt = expected_aggregate(b, "helper", mask=st == 0)
    got, cnt = on[2]
    assert got == exp and cnt == ecnt == N - len(bad)


def test_p256_option_needs_a_gpu_mode():
    b = _batch("count", 24)
    v = _vdaf("count", b)
    try:
        with pytest.raises(ValueError):
            HelperAggregateInit(v, TASK_ID, [H.generate_hpke_config_and_private_key(1)],
                                hpke="host", hpke_gpu_p256=1)
        drv = HelperAggregateInit(v, TASK_ID, [H.generate_hpke_config_and_private_key(1)],
                                  hpke="gpu", hpke_gpu_p256=1)
        drv.close()
    finally:
        v.close()
