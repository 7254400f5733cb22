"""ClientBatch's `long_seal` (janus_amd/client.py): which of the seal's kernels an aggregator's
shares take never shows in the report bytes.  Prio3SumVec(8, 1000) reports -- a 134,944-byte leader
share, a 48-byte helper share -- built under long_seal=True, False and None from the same
randomness and ephemeral keys are one matrix; the profile shows which kernels ran; and the reports
sealed a wave per report open, through UploadBatch, to the oracle's shares."""
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

NAME, N = "sumvec_8_1000", 3
TASK_ID = bytes(range(60, 92))
PRECISION = 300


@functools.lru_cache(maxsize=None)
def _batch():
    return make_batch(NAME, N)


@functools.lru_cache(maxsize=None)
def _keys(leader_aead):
    return (H.generate_hpke_config_and_private_key(11, H.KEM_X25519_HKDF_SHA256, 1, leader_aead),
            H.generate_hpke_config_and_private_key(12, H.KEM_X25519_HKDF_SHA256, 2, 2))


@pytest.fixture(scope="module")
def vdaf():
    from janus_amd.prio3 import Prio3Gpu
    c, b = CONFIGS[NAME], _batch()
    v = Prio3Gpu(c["kind"], b.verify_key, bits=c["bits"], length=c["length"],
                 chunk_length=c["chunk"])
    yield v
    v.close()


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


def _prepare(v, long_seal, leader_aead=1):
    b = _batch()
    lkp, hkp = _keys(leader_aead)
    cb = CL.ClientBatch(v, TASK_ID, lkp.config, hkp.config, PRECISION, long_seal=long_seal)
    times = np.array([1_700_000_000 + 977 * i for i in range(N)], np.uint64)
    sk = np.random.default_rng(8).integers(0, 256, (2, N, 32), dtype=np.uint8)
    try:
        return _launches(v, lambda: cb.prepare_reports(meas_array(b), report_ids=b.nonces,
                                                       times=times, rand=b.rand, sk_es=sk))
    finally:
        cb.close()


SEALS = ("k_hpke_seal", "k_hpke_seal_shares", "k_hpke_seal_team", "k_hpke_seal_team_shares")


def test_report_bytes_do_not_depend_on_the_route(vdaf):
    assert vdaf.sizes.leader_input_share == 134_944 and vdaf.sizes.helper_input_share == 48
    lane, lane_k = _prepare(vdaf, False)
    wave, wave_k = _prepare(vdaf, True)
    auto, auto_k = _prepare(vdaf, None)
    assert lane.shape == (N, 135_174)
    assert np.array_equal(wave, lane) and np.array_equal(auto, lane)
    assert [lane_k[k] for k in SEALS] == [0, 2, 0, 0] and lane_k["k_x25519_eph"] == 2
    # True with an AES-GCM pair: both aggregators' shares a wave per report
    assert [wave_k[k] for k in SEALS] == [0, 0, 0, 2] and wave_k["k_x25519_eph"] == 2
    # auto: the threshold is measured, between the two shares' lengths
    assert 48 < CL.ClientBatch.LONG_SEAL_MIN_SHARE <= 134_944
    assert [auto_k[k] for k in SEALS] == [0, 1, 0, 1]    # leader: the wave; helper: the lane


def test_chacha20poly1305_leader_takes_the_lane_path(vdaf):
    lkp, hkp = _keys(3)
    with pytest.raises(ValueError):
        CL.ClientBatch(vdaf, TASK_ID, lkp.config, hkp.config, PRECISION, long_seal=True)
    with pytest.raises(ValueError):
        CL.ClientBatch(vdaf, TASK_ID, hkp.config, lkp.config, PRECISION, long_seal=True)
    auto, auto_k = _prepare(vdaf, None, leader_aead=3)
    lane, lane_k = _prepare(vdaf, False, leader_aead=3)
    assert np.array_equal(auto, lane)
    assert auto_k["k_hpke_seal_team_shares"] == 0 and auto_k["k_hpke_seal_shares"] == 2
    r = CL.decode_report(auto[1].tobytes())
    info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
    ct = r.leader_encrypted_input_share
    pt = H.open_(lkp, info, ct.encapsulated_key, ct.payload,
                 H.input_share_aad(TASK_ID, r.report_id, r.time, r.public_share))
    assert pt == CL.encode_plaintext_input_share(_batch().leader_in[1].tobytes())


def test_wave_sealed_reports_open_to_the_oracles_shares(vdaf):
    b = _batch()
    reports, _ = _prepare(vdaf, True)
    lkp, hkp = _keys(1)
    for kp, role, want in ((lkp, H.ROLE_LEADER, b.leader_in), (hkp, H.ROLE_HELPER, b.helper_in)):
        shares, st = UploadBatch(vdaf, TASK_ID, [kp], role=role).open_reports(reports)
        assert not st.any() and np.array_equal(shares, want[:N])
