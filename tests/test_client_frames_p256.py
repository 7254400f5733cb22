"""janus_amd/client.py's Report layout with 65-byte (P-256) encapsulated keys and the draw of
ephemeral P-256 scalars, on the CPU: offsets, lengths, the `00 41` prefixes and the round trip
through `decode_report` at enc lengths (65, 32), (32, 65) and (65, 65); the three-argument form
is what it was."""
import numpy as np
import pytest

from janus_amd import client as CL

PUB, LSH, HSH = 5, 37, 9


def _filled(L, n=3, seed=1):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = rng.integers(0, 2**40, n).astype(np.uint64)
    pubs = rng.integers(0, 256, (n, PUB), dtype=np.uint8)
    m = np.zeros((n, L.report_len), np.uint8)
    L.write_fixed(m, ids, times, pubs, 7, 200)
    cols = {}
    for which in ("leader", "helper"):
        enc, pay = L.columns(m, which)
        cols[which] = (rng.integers(0, 256, enc.shape, dtype=np.uint8),
                       rng.integers(0, 256, pay.shape, dtype=np.uint8))
        enc[:], pay[:] = cols[which]
    return m, ids, times, pubs, cols


@pytest.mark.parametrize("le,he", [(65, 32), (32, 65), (65, 65)])
def test_layout_with_p256_encs(le, he):
    L = CL.ReportLayout(PUB, LSH, HSH, leader_enc=le, helper_enc=he)
    assert (L.leader_enc, L.helper_enc) == (le, he)
    assert L.o_public == 28 and L.o_leader == 28 + PUB
    assert L.o_leader_enc == L.o_leader + 3
    assert L.o_leader_payload == L.o_leader_enc + le + 4
    assert L.leader_payload == 6 + LSH + 16 and L.helper_payload == 6 + HSH + 16
    assert L.o_helper == L.o_leader_payload + L.leader_payload
    assert L.o_helper_enc == L.o_helper + 3
    assert L.o_helper_payload == L.o_helper_enc + he + 4
    assert L.report_len == L.o_helper_payload + L.helper_payload
    base = CL.ReportLayout(PUB, LSH, HSH)
    assert L.report_len == base.report_len + (le - 32) + (he - 32)
    m, ids, times, pubs, cols = _filled(L)
    for o, cfg, ne in ((L.o_leader, 7, le), (L.o_helper, 200, he)):
        assert m[:, o].tolist() == [cfg] * 3
        assert m[0, o + 1:o + 3].tolist() == ([0x00, 0x41] if ne == 65 else [0x00, 0x20])
    for i in range(3):
        r = CL.decode_report(m[i].tobytes())
        assert r.report_id == ids[i].tobytes() and r.time == int(times[i])
        assert r.public_share == pubs[i].tobytes()
        for ct, which, cfg, ne in ((r.leader_encrypted_input_share, "leader", 7, le),
                                   (r.helper_encrypted_input_share, "helper", 200, he)):
            assert ct.config_id == cfg and len(ct.encapsulated_key) == ne
            assert ct.encapsulated_key == cols[which][0][i].tobytes()
            assert ct.payload == cols[which][1][i].tobytes()
        assert CL.encode_report(r.report_id, r.time, r.public_share,
                                r.leader_encrypted_input_share,
                                r.helper_encrypted_input_share) == m[i].tobytes()


def test_default_layout_is_unchanged():
    L = CL.ReportLayout(PUB, LSH, HSH)
    assert CL.ENC_LEN == 32 and (L.leader_enc, L.helper_enc) == (32, 32)
    assert L.o_leader_enc == 28 + PUB + 3 and L.o_leader_payload == L.o_leader_enc + 36
    assert L.o_helper == L.o_leader_payload + 6 + LSH + 16
    assert L.report_len == 16 + 8 + 4 + PUB + 2 * (1 + 2 + 32 + 4 + 6 + 16) + LSH + HSH
    m, *_ = _filled(L)
    assert m[0, L.o_leader + 1:L.o_leader + 3].tolist() == [0x00, 0x20]
    assert m[0, L.o_helper + 1:L.o_helper + 3].tolist() == [0x00, 0x20]
    enc, pay = L.columns(m, "helper")
    assert enc.shape == (3, 32) and pay.shape == (3, 6 + HSH + 16)


def test_scalar_draw_redraws_zero_the_order_and_all_ones():
    """Crafted bytes: 0, n and 2^256 - 1 are refused and drawn again; n - 1 and 1 are kept."""
    n = CL.P256_ORDER
    feed = [(0).to_bytes(32, "big") + n.to_bytes(32, "big") + (n - 1).to_bytes(32, "big"),
            b"\xff" * 32,                   # redraw of slot 0: refused again
            (1).to_bytes(32, "big"),        # slot 0, third draw
            (n + 1).to_bytes(32, "big"),    # slot 1
            (2**255).to_bytes(32, "big")]
    calls = []

    def rand(k):
        calls.append(k)
        return feed.pop(0)

    out = CL.draw_p256_scalars(3, rand)
    assert [int.from_bytes(r.tobytes(), "big") for r in out] == [1, 2**255, n - 1]
    assert calls == [96, 32, 32, 32, 32] and not feed
    drawn = CL.draw_p256_scalars(64)
    assert drawn.shape == (64, 32) and drawn.dtype == np.uint8
    assert all(1 <= int.from_bytes(r.tobytes(), "big") < n for r in drawn)
