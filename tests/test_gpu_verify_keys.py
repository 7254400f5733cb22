"""A verify key per report (prio3gpu_state_set_verify_keys): reports of three tasks in one engine
call, each prepared under its own task's key, against the oracle transcript of that task.

`make_batch(name, n, cfg_id=...)` derives both the verify key and the reports from `cfg_id`, so
three ids give three tasks.  Every set of reports is laid out twice: task by task (boundaries
inside the first wave and past a 256-thread block edge, or across a wave boundary with a ragged
last wave) and interleaved (key_index[r] = r % 3).  The context's own key is none of the tasks'.
"""
import ctypes

import numpy as np
import pytest

from oracle import prio3 as O
from tests.reports import CONFIGS, expected_aggregate, make_batch, plaintext_sum

pytestmark = pytest.mark.gpu

E_ARG = -1
PREP_ERROR = 5  # PRIO3GPU_VDAF_PREP_ERROR
# report count and task sizes per shape
SHAPES = {"count": (300, (5, 200, 95)), "sum8": (300, (5, 200, 95)),
          "sum5": (129, (5, 70, 54)), "sumvec_small": (129, (5, 70, 54)),
          "hist4": (129, (5, 70, 54)), "fp16_3": (129, (5, 70, 54))}
LAYOUTS = ("by_task", "interleaved")
COLS = ("nonces", "public", "leader_in", "helper_in", "leader_prep", "helper_prep", "prep_msg")
CTX_KEY = bytes(range(0xA0, 0xB0))

# The kernel ids of the parent commit, in order (prio3gpu_prof_kernel_name): the new id comes after.
PARENT_KERNELS = [
    "k_query_rand", "k_expand", "k_helper_xof", "k_jr", "k_flp_weights", "k_flp_wires",
    "k_fpv_weights", "k_fpv_wires0", "k_fpv_wires1", "k_fpv_finalize", "k_decide", "k_fpv_decide",
    "k_prepare_next", "k_accum_partial", "k_accum_spec", "k_accum_merge", "k_out_shares", "k_merge",
    "k_shard_seeds", "k_shard_meas", "k_shard_jr", "k_flp_prove", "k_shard_proof", "k_report_meta",
    "k_report_meta_fold", "k_shard_norm", "k_jr_ring", "k_flp_query_lane", "k_flp_wires_cols",
    "k_flp_wires_mfma", "k_fpv_regen", "k_x25519", "k_hpke_open", "k_req_gather", "k_x25519_idx",
    "k_hpke_open_req", "k_decode_plaintext_input_shares", "k_req_scatter", "copy_request",
    "k_p256_dh", "k_p256_dh_idx", "k_x25519_eph", "k_hpke_seal", "k_hpke_seal_shares",
    "k_hpke_open_team", "k_hpke_open_team_shares", "k_hpke_seal_team", "k_hpke_seal_team_shares",
    "k_p256_eph", "k_p256_eph_kem", "k_hpke_open_team_split", "k_hpke_open_team_join",
    "k_hpke_team_wipe", "k_hpke_seal_team_split", "k_hpke_seal_team_join"]

_tasks = {}


def tasks(name, xof=None):
    """Three tasks' oracle batches for a shape, computed once: each holds enough reports for both
    layouts (its task-by-task size, or a third of the batch for the interleaved one)."""
    key = (name, xof)
    if key not in _tasks:
        n, sizes = SHAPES[name]
        bs = [make_batch(name, max(sz, n // 3), cfg_id=f"{name}/task{k}".encode(), xof=xof)
              for k, sz in enumerate(sizes)]
        assert len({b.verify_key for b in bs}) == 3 and CTX_KEY not in {b.verify_key for b in bs}
        _tasks[key] = bs
    return _tasks[key]


class Mixed:
    """One batch of n reports of three tasks: rows[r] = (task, index in the task's batch)."""

    def __init__(self, name, layout, xof=None):
        n, sizes = SHAPES[name]
        self.name, self.n, self.tasks = name, n, tasks(name, xof)
        if layout == "by_task":
            self.rows = [(k, i) for k, sz in enumerate(sizes) for i in range(sz)]
        else:
            self.rows = [(r % 3, r // 3) for r in range(n)]
        assert len(self.rows) == n
        self.key_index = np.array([k for k, _ in self.rows], np.uint32)
        self.keys = [b.verify_key for b in self.tasks]
        for col in COLS:
            setattr(self, col, np.ascontiguousarray(
                np.stack([getattr(self.tasks[k], col)[i] for k, i in self.rows])))

    def task_mask(self, k, ok=None):
        """Which reports of task k's oracle batch are in this batch (and, with `ok`, accepted)."""
        m = np.zeros(self.tasks[k].n, bool)
        for r, (kk, i) in enumerate(self.rows):
            if kk == k and (ok is None or ok[r]):
                m[i] = True
        return m


_mixed = {}


def mixed(name, layout, xof=None):
    key = (name, layout, xof)
    if key not in _mixed:
        _mixed[key] = Mixed(name, layout, xof)
    return _mixed[key]


def gpu_vdaf(name, xof=None):
    from janus_amd.prio3 import XOF_SHAKE128, XOF_TURBOSHAKE128, Prio3Gpu
    c = CONFIGS[name]
    return Prio3Gpu(c["kind"], CTX_KEY, bits=c["bits"], length=c["length"], chunk_length=c["chunk"],
                    xof=XOF_TURBOSHAKE128 if xof is not None else XOF_SHAKE128)


def keyed_state(v, agg_id, m, key_index=None):
    st = v.new_state(agg_id, m.n)
    st.set_verify_keys(m.keys, m.key_index if key_index is None else key_index)
    return st


def check_transcripts(v, m):
    for agg_id, shares, want in ((0, m.leader_in, m.leader_prep), (1, m.helper_in, m.helper_prep)):
        st = keyed_state(v, agg_id, m)
        prep, status = v.prepare_init(st, m.nonces, m.public, shares)
        assert (status == 0).all()
        np.testing.assert_array_equal(prep, want)
        st.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_keyed_prepare_init_matches_each_task_transcript(name, layout):
    v = gpu_vdaf(name)
    check_transcripts(v, mixed(name, layout))
    v.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_keyed_two_phase_equals_keyed_prepare_init(name, layout):
    m = mixed(name, layout)
    v = gpu_vdaf(name)
    pub = m.public if v.sizes.public_share else None
    for agg_id, shares in ((0, m.leader_in), (1, m.helper_in)):
        st = keyed_state(v, agg_id, m)
        want, wst = v.prepare_init(st, m.nonces, m.public, shares)
        st2 = keyed_state(v, agg_id, m)
        status = np.zeros(m.n, np.uint8)
        got = np.zeros((m.n, v.sizes.prep_share), np.uint8)
        v.prepare_init_xof(st2, m.nonces, pub, shares, status)
        v.prepare_init_query(st2, got, status)
        assert (status == 0).all() and (wst == 0).all()
        np.testing.assert_array_equal(got, want)
        st.close()
        st2.close()
    v.close()


def run_both_aggregators(v, m, helper_key_index=None):
    """Leader keyed prepare_init, helper keyed helper_init with batch_slots = key_index, leader
    prepare_next -> (prep msgs, helper status, leader aggregate, helper aggregate)."""
    ls = keyed_state(v, 0, m)
    lp, lst = v.prepare_init(ls, m.nonces, m.public, m.leader_in)
    assert (lst == 0).all()
    np.testing.assert_array_equal(lp, m.leader_prep)
    hs = keyed_state(v, 1, m, helper_key_index)
    hagg, lagg = v.new_aggregate(3), v.new_aggregate(3)
    msgs, hst = v.helper_init(hs, m.nonces, m.public, m.helper_in, lp, agg=hagg,
                              batch_slots=m.key_index)
    lst = hst.copy()
    v.prepare_next(ls, msgs, lst, want_output_shares=False, agg=lagg, batch_slots=m.key_index)
    np.testing.assert_array_equal(lst, hst)
    ls.close()
    hs.close()
    return msgs, hst, lagg, hagg


def check_aggregates(v, m, ok, lagg, hagg):
    for k, b in enumerate(m.tasks):
        mask = m.task_mask(k, ok)
        la, lc = lagg.read(k)
        ha, hc = hagg.read(k)
        assert (la, lc) == expected_aggregate(b, "leader", mask=mask)
        assert (ha, hc) == expected_aggregate(b, "helper", mask=mask)
        assert lc == int(mask.sum())
        if m.name.startswith("fp"):
            assert v.unshard([la, ha], lc) == pytest.approx(plaintext_sum(b, mask), rel=1e-12,
                                                            abs=1e-12)
        else:
            assert v.unshard([la, ha]) == plaintext_sum(b, mask)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_keyed_helper_init_aggregates_per_task(name, layout):
    m = mixed(name, layout)
    v = gpu_vdaf(name)
    msgs, hst, lagg, hagg = run_both_aggregators(v, m)
    assert (hst == 0).all()
    if v.sizes.prep_msg:
        np.testing.assert_array_equal(msgs, m.prep_msg)
    check_aggregates(v, m, np.ones(m.n, bool), lagg, hagg)
    v.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["count", "sumvec_small"])
def test_a_key_that_matters(name, layout):
    """One report's key_index points at another task's key on the helper only: the two verifier
    shares no longer belong to one query, and that report alone is rejected."""
    m = mixed(name, layout)
    v = gpu_vdaf(name)
    r = 77
    wrong = m.key_index.copy()
    wrong[r] = (wrong[r] + 1) % 3
    msgs, hst, lagg, hagg = run_both_aggregators(v, m, wrong)
    ok = np.ones(m.n, bool)
    ok[r] = False
    assert hst[r] == PREP_ERROR and (hst[ok] == 0).all()
    if v.sizes.prep_msg:
        np.testing.assert_array_equal(msgs[ok], m.prep_msg[ok])
    check_aggregates(v, m, ok, lagg, hagg)
    v.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_keyed_prepare_init_turboshake(layout):
    v = gpu_vdaf("sumvec_small", xof=O.XofTurboShake128)
    check_transcripts(v, mixed("sumvec_small", layout, xof=O.XofTurboShake128))
    v.close()


def _prof_counts(v):
    from janus_amd._lib import lib
    ms, nl = (ctypes.c_double * 128)(), (ctypes.c_uint64 * 128)()
    k = lib().prio3gpu_prof_read(v._ctx, ms, nl, 128)
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(nl[i]) for i in range(k)}


def test_contract_errors_change_nothing():
    from janus_amd._lib import Prio3GpuError, lib
    from janus_amd import codec as C
    from janus_amd import hpke as H
    L = lib()
    m = mixed("sumvec_small", "by_task")
    v = gpu_vdaf("sumvec_small")
    n = m.n
    keys = np.frombuffer(b"".join(m.keys), np.uint8).copy()
    st = v.new_state(1, n)
    st.set_verify_keys(m.keys, m.key_index)
    want, _ = v.prepare_init(st, m.nonces, m.public, m.helper_in)
    np.testing.assert_array_equal(want, m.helper_prep)

    def setk(idx_ptr, cnt, num=3):
        return L.prio3gpu_state_set_verify_keys(st._h, keys.ctypes.data, num, idx_ptr, cnt)

    def still_as_set():
        got, status = v.prepare_init(st, m.nonces, m.public, m.helper_in)
        assert (status == 0).all()
        np.testing.assert_array_equal(got, want)

    # an index equal to num_keys, in a host array
    bad = m.key_index.copy()
    bad[40] = 3
    assert setk(bad.ctypes.data, n) == E_ARG
    assert "key_index[40]" in L.prio3gpu_last_error().decode()
    still_as_set()
    # ... and in a device array
    d = ctypes.c_void_p()
    assert L.prio3gpu_dev_alloc(v._ctx, n * 4, ctypes.byref(d)) == 0
    try:
        assert L.prio3gpu_memcpy(v._ctx, d, bad.ctypes.data, n * 4) == 0
        assert setk(d, n) == E_ARG
        assert "key_index[40]" in L.prio3gpu_last_error().decode()
        still_as_set()
        # a good device index is taken
        assert L.prio3gpu_memcpy(v._ctx, d, m.key_index.ctypes.data, n * 4) == 0
        assert setk(d, n) == 0
        still_as_set()
    finally:
        L.prio3gpu_dev_free(v._ctx, d)
    # n above the state's capacity
    big = np.zeros(n + 1, np.uint32)
    assert setk(big.ctypes.data, n + 1) == E_ARG
    still_as_set()
    # null tables with keys to set
    assert L.prio3gpu_state_set_verify_keys(st._h, None, 3, m.key_index.ctypes.data, n) == E_ARG
    assert setk(None, n) == E_ARG
    still_as_set()
    # a keyed state called with another n: nothing is launched
    L.prio3gpu_prof_enable(v._ctx, 1)
    _prof_counts(v)  # drain
    with pytest.raises(Prio3GpuError, match=r"\(-1\)"):
        v.prepare_init(st, m.nonces[:n - 1], m.public[:n - 1], m.helper_in[:n - 1])
    status = np.zeros(n - 1, np.uint8)
    with pytest.raises(Prio3GpuError, match=r"\(-1\)"):
        v.prepare_init_xof(st, m.nonces[:n - 1], m.public[:n - 1], m.helper_in[:n - 1], status)
    with pytest.raises(Prio3GpuError, match=r"\(-1\)"):
        v.helper_init(st, m.nonces[:n - 1], m.public[:n - 1], m.helper_in[:n - 1],
                      m.leader_prep[:n - 1])
    # helper_init_request and shard refuse a keyed state
    tk = H.generate_hpke_config_and_private_key(1)
    cts = [(1, b"\x01" * 32, b"\x02" * 40)] * n
    req = C.decode_agg_init_req(C.encode_agg_init_req(
        C.TIME_INTERVAL, None, b"", m.nonces, list(range(n)), m.public, cts, m.leader_prep))
    with pytest.raises(Prio3GpuError, match=r"\(-1\).*verify keys"):
        v.helper_init_request(st, bytes(32), req, [tk])
    with pytest.raises(Prio3GpuError, match=r"\(-1\).*verify keys"):
        v.shard(st, m.nonces, np.zeros((n, 10), np.uint64),
                np.zeros((n, v.random_size()), np.uint8))
    assert not any(_prof_counts(v).values())
    L.prio3gpu_prof_enable(v._ctx, 0)
    still_as_set()
    # cleared: the bytes of an untouched state under the context's key
    st.clear_verify_keys()
    fresh = v.new_state(1, n)
    a, ast = v.prepare_init(st, m.nonces, m.public, m.helper_in)
    b, bst = v.prepare_init(fresh, m.nonces, m.public, m.helper_in)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ast, bst)
    assert not np.array_equal(a, want)  # the context's key is none of the tasks'
    # and an unkeyed state takes any n again
    v.prepare_init(st, m.nonces[:7], m.public[:7], m.helper_in[:7])
    st.close()
    fresh.close()
    v.close()


@pytest.mark.parametrize("name", ["count", "sumvec_small"])
def test_unkeyed_path_launches_what_it_did(name):
    from janus_amd._lib import lib
    L = lib()
    assert [L.prio3gpu_prof_kernel_name(i).decode() for i in range(len(PARENT_KERNELS))] == \
        PARENT_KERNELS
    assert L.prio3gpu_prof_kernel_name(len(PARENT_KERNELS)).decode() == "k_query_rand_keyed"
    assert L.prio3gpu_prof_kernel_name(len(PARENT_KERNELS) + 1).decode() == ""
    m = mixed(name, "by_task")
    v = gpu_vdaf(name)
    L.prio3gpu_prof_enable(v._ctx, 1)
    _prof_counts(v)  # drain
    for agg_id, shares in ((0, m.leader_in), (1, m.helper_in)):
        st = v.new_state(agg_id, m.n)
        v.prepare_init(st, m.nonces, m.public, shares)
        plain = _prof_counts(v)
        assert plain["k_query_rand_keyed"] == 0
        assert plain["k_query_rand"] == (0 if name == "count" else 1)  # Count derives t inline
        assert plain["k_flp_query_lane"] == (1 if name == "count" else 0)
        st.set_verify_keys(m.keys, m.key_index)
        v.prepare_init(st, m.nonces, m.public, shares)
        keyed = _prof_counts(v)
        assert keyed["k_query_rand_keyed"] == 1 and keyed["k_query_rand"] == 0
        # nothing else moved
        for k in PARENT_KERNELS[1:]:
            assert keyed[k] == plain[k], k
        st.close()
    v.close()
