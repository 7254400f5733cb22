"""The client's DAP framing (janus_amd/client.py) on the CPU: Report, PlaintextInputShare and
InputShareAad against the reference's own known-answer encodings (tests/golden/
dap_report_kats.json), and the fixed-stride column layout ClientBatch writes against those
encoders, with decode_report as its inverse."""
import json
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from janus_amd import client as CL
from janus_amd import hpke as H

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dap_report_kats.json")))


def h(s):
    return bytes.fromhex(s.replace(" ", ""))


def test_kat_file_names_its_source():
    assert "messages/src/lib.rs" in KATS["source"]
    assert len(KATS["report"]) == 2 and len(KATS["plaintext_input_share"]) == 2


@pytest.mark.parametrize("k", KATS["plaintext_input_share"])
def test_plaintext_input_share(k):
    assert CL.encode_plaintext_input_share(h(k["payload"]), h(k["extensions"])) == h(k["expected"])


@pytest.mark.parametrize("k", KATS["input_share_aad"])
def test_input_share_aad(k):
    assert H.input_share_aad(h(k["task_id"]), h(k["report_id"]), k["time"],
                             h(k["public_share"])) == h(k["expected"])


def _cts(k):
    return [(k[w]["config_id"], h(k[w]["enc"]), h(k[w]["payload"])) for w in ("leader", "helper")]


@pytest.mark.parametrize("k", KATS["report"])
def test_report_encodes_and_decodes(k):
    leader, helper = _cts(k)
    enc = CL.encode_report(h(k["report_id"]), k["time"], h(k["public_share"]), leader, helper)
    assert enc == h(k["expected"])
    r = CL.decode_report(enc)
    assert (r.report_id, r.time, r.public_share) == (h(k["report_id"]), k["time"],
                                                     h(k["public_share"]))
    assert tuple(r.leader_encrypted_input_share) == leader
    assert tuple(r.helper_encrypted_input_share) == helper
    with pytest.raises(ValueError):
        CL.decode_report(enc + b"\0")
    for cut in (1, 5, len(enc) - 20):
        with pytest.raises(ValueError):
            CL.decode_report(enc[:-cut])


@pytest.mark.parametrize("pub,ls,hs", [(0, 32, 48), (16, 7, 1), (33, 135, 54)])
def test_fixed_stride_layout_is_the_report_encoding(pub, ls, hs):
    """ReportLayout's columns, filled the way ClientBatch.prepare_reports fills them with fake
    shares, are byte for byte the KAT-checked encoder's Reports."""
    n = 5
    rng = np.random.default_rng(pub + ls)
    L = CL.ReportLayout(pub, ls, hs)
    assert L.report_len == 16 + 8 + 4 + pub + 2 * (1 + 2 + 32 + 4 + 6 + 16) + ls + hs
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = CL.round_times([1_700_000_123 + 4000 * i for i in range(n)], 3600)
    assert all(int(t) % 3600 == 0 for t in times) and int(times[0]) == 1_699_999_200
    public = rng.integers(0, 256, (n, pub), dtype=np.uint8)
    reports = np.full((n, L.report_len), 0xEE, np.uint8)
    L.write_fixed(reports, ids, times, public if pub else None, 42, 13)
    fake = {}
    for which in ("leader", "helper"):
        encs, pays = L.columns(reports, which)
        assert encs.shape == (n, 32)
        assert pays.shape == (n, 6 + (ls if which == "leader" else hs) + 16)
        assert (encs == 0xEE).all() and (pays == 0xEE).all()    # the seal's columns: untouched
        fake[which] = (rng.integers(0, 256, encs.shape, dtype=np.uint8),
                       rng.integers(0, 256, pays.shape, dtype=np.uint8))
        encs[:], pays[:] = fake[which]
    for i in range(n):
        want = CL.encode_report(ids[i].tobytes(), int(times[i]), public[i].tobytes(),
                                (42, fake["leader"][0][i].tobytes(),
                                 fake["leader"][1][i].tobytes()),
                                (13, fake["helper"][0][i].tobytes(),
                                 fake["helper"][1][i].tobytes()))
        assert reports[i].tobytes() == want
        r = CL.decode_report(reports[i].tobytes())
        assert r.helper_encrypted_input_share.payload == fake["helper"][1][i].tobytes()
        with pytest.raises(ValueError):
            CL.decode_report(reports[i].tobytes() + b"\x01")
    if pub == 0:                                                # Count: 00 00 00 00, no bytes
        assert (reports[:, 24:28] == 0).all() and (reports[:, 28] == 42).all()


def test_client_batch_takes_its_layout_from_the_vdaf_sizes():
    sizes = SimpleNamespace(public_share=16, leader_input_share=135, helper_input_share=54)
    vdaf = SimpleNamespace(sizes=sizes, device=0)
    lk = H.HpkeConfig(1, H.KEM_X25519_HKDF_SHA256, 1, 1, bytes(32))
    p256 = H.HpkeConfig(2, H.KEM_P256_HKDF_SHA256, 1, 1, bytes(65))
    cb = CL.ClientBatch(vdaf, bytes(32), lk, lk, 300)
    assert cb.report_len == 16 + 8 + 4 + 16 + 2 * (1 + 2 + 32 + 4 + 6 + 16) + 135 + 54
    assert cb.layout.o_helper_payload + cb.layout.helper_payload == cb.report_len
    with pytest.raises(ValueError):
        CL.ClientBatch(vdaf, bytes(32), lk, p256, 300)
    with pytest.raises(ValueError):
        CL.ClientBatch(vdaf, bytes(31), lk, lk, 300)
    assert struct.pack(">I", cb.layout.leader_payload) == (6 + 135 + 16).to_bytes(4, "big")
