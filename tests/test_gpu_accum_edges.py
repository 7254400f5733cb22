"""The leader's accumulation and the aggregate merges at edge-valued shares.

Every other test drives the accumulation kernels with real reports, whose share elements are
uniform and never reach the operands at which modular accumulation goes wrong (partial sums at
p - 1, p and 0, word sums that carry, rows of all-ones words).  prepare_next checks only that the
prep message equals the corrected joint-rand seed (the FLP decision was made earlier, in
prepare_shares_to_prepare_message), so the leader's path takes crafted shares honestly:
prepare_init over arbitrary canonical leader shares, each report's prep message derived on the host
with the oracle, prepare_next accumulating exactly those rows.  Expected = Python integers:
truncate(sum of the accepted rows) mod p per slot and output element, truncate(row) per report.

Column e of the measurement share holds one of tests/accum_edges.py's families, (e + shift) mod 14
(Count has one column: its family changes from wave to wave instead).  sumvec_small has 10
columns inside the column-summed window [8, 18) and 10 outside, fewer than the 14 families, so no
cycle puts every family on both sides there: n = 300 shifts the cycle so that the families whose
word sums carry lie inside, n = 4200 leaves it unshifted, and between them every family is
column-summed once.  The wider shapes hold every family inside."""
import ctypes
import functools

import numpy as np
import pytest

from tests.accum_edges import (EVENTS, FAMILIES64, FAMILIES128, P64, P128, column,
                               fold_events)
from tests.reports import CONFIGS
from tests.test_host_plan import SPEC_RANGES, plan_restated, spec_fold_slots

gpu = pytest.mark.gpu

F = len(FAMILIES128)
VK = bytes(range(16))


# ---- the batch ---------------------------------------------------------------------------------
def slot_layout(n):
    """Whole waves on slot 0, one mixed-slot wave in the middle, whole waves on slot 2 and the
    partial last wave on slot 1 (n = 300: tests/test_gpu_spec.py's layout); n = 4200: the layout
    with two speculative chunks on slot 0."""
    if n == 4200:
        return spec_fold_slots(), 64
    mw = (n // 64) // 2
    slots = np.zeros(n, np.uint32)
    slots[64 * mw:64 * mw + 64] = np.random.default_rng(7).integers(0, 3, 64)
    slots[64 * mw + 64:] = 2
    slots[64 * (n // 64):] = 1
    return slots, mw


def to_bytes(values, es):
    return np.frombuffer(b"".join(x.to_bytes(es, "little") for x in values),
                         np.uint8).reshape(len(values), es)


def family_of(e, w, meas_len, shift):
    return (w if meas_len == 1 else e + shift) % F


def phase_for(spec, n, ones):
    """Row n - 1 (the row the clamped lanes of a partial last wave read again) holds the periodic
    family's all-ones word."""
    v = spec[1]
    at = max(i for i, x in enumerate(v) if x == ones)
    return (at - (n - 1)) % len(v)


@functools.lru_cache(None)
def make_batch(name, n, shift):
    c = CONFIGS[name]
    v = c["ctor"]()
    es, p = v.fld.ENCODED_SIZE, v.fld.MODULUS
    fams = FAMILIES128 if es == 16 else FAMILIES64
    ones = (1 << (4 * es)) - 1
    L = v.typ.MEAS_LEN
    rng = np.random.default_rng(n + L)
    slots, mw = slot_layout(n)
    # Rows that must not count.  In whole waves they lie on rows congruent to n - 1 mod 4, the
    # periodic families' all-ones-word rows: k_accum_spec subtracts edge rows, and what stays of
    # "period4 carry" in a chunk still carries out of ahi + blo (less a p - 1 row its high-word sum
    # would wrap instead).  Wave 0 loses two rows only: 32 rows of p - 1 and 30 or more of 2^64 - 1
    # still pass 2^128, 28 would not.  A batch with a second whole one-slot wave has the other
    # two there, a batch without has the 0xFF row in the mixed-slot wave.
    def pick(r):
        return r + (n - 1 - r) % 4
    w2 = n // 64 - 1 if n // 64 - 1 != mw else mw - 1
    if w2 > 0:
        status5, all_ff = [pick(64 * w2 + 5), 64 * mw + 9, n - 2], pick(64 * w2 + 33)
    else:
        status5, all_ff = [64 * mw + 9, n - 2], 64 * mw + 33
    bad = {"status5": status5, "elem_p": pick(17), "all_ff": all_ff,
           "flipped": pick(40) if v.uses_jr else None}
    meas = np.zeros((n, L, es), np.uint8)
    cache = {}
    for e in range(L):
        for w0 in ([0] if L > 1 else range((n + 63) // 64)):
            f = family_of(e, w0, L, shift)
            spec = fams[f][1]
            key = (f, w0) if spec[0] != "random" else (f, w0, e)
            if key not in cache:
                ph = phase_for(spec, n, ones) if spec[0] == "period" else 0
                cache[key] = to_bytes(column(spec, n, p, rng, at=(64 * w0 + 2, 64 * w0 + 3),
                                             phase=ph), es)
            if L > 1:
                meas[:, e] = cache[key]
            else:
                meas[64 * w0:64 * w0 + 64, e] = cache[key][64 * w0:64 * w0 + 64]
    sr = SPEC_RANGES.get(name)
    e_p = sr[1] + 1 if sr else 0        # the element equal to p: inside the window where one is
    meas[bad["elem_p"], e_p] = to_bytes([p], es)[0]
    tail = rng.integers(0, 256, (n, v.leader_input_share_len() - L * es), dtype=np.uint8)
    tail[:, es - 1:v.PROOF_LEN * es:es] &= 0x7F     # canonical proof elements; the blind is free
    lin = np.concatenate([meas.reshape(n, L * es), tail], axis=1)
    lin[bad["all_ff"]] = 0xFF
    meas = lin[:, :L * es].reshape(n, L, es)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    pub = rng.integers(0, 256, (n, v.public_share_len()), dtype=np.uint8) if v.uses_jr else None
    status = np.zeros(n, np.uint8)
    status[bad["status5"]] = 5
    status[[bad["elem_p"], bad["all_ff"]]] = 8
    if bad["flipped"] is not None:
        status[bad["flipped"]] = 5
    return dict(name=name, n=n, shift=shift, v=v, es=es, p=p, L=L, slots=slots, mw=mw, bad=bad,
                meas=meas, lin=np.ascontiguousarray(lin), nonces=nonces, pub=pub, status=status,
                fams=fams)


def truncate(c, cols):
    """prio Type::truncate on Python integers (not reduced)."""
    if c["kind"] in (1, 2, 4):
        bits = c["bits"]
        n_out = 1 if c["kind"] == 1 else c["length"]
        return [sum(cols[o * bits + b] << b for b in range(bits)) for o in range(n_out)]
    return list(cols)


def limbs(meas):
    """(n, L, es) bytes -> (n, L, es / 4) 32-bit limbs as uint64."""
    n, L, es = meas.shape
    return np.ascontiguousarray(meas).view("<u4").reshape(n, L, es // 4).astype(np.uint64)


def column_sums(lb, rows):
    """Exact integer sums of the selected rows, per column (limb sums recombined in Python)."""
    s = lb[rows].sum(axis=0, dtype=np.uint64)       # < 2^32 rows x 2^32
    return [sum(int(x) << (32 * j) for j, x in enumerate(col)) for col in s]


@functools.lru_cache(None)
def reference(name, n, shift):
    b = make_batch(name, n, shift)
    c, p, es = CONFIGS[name], b["p"], b["es"]
    lb = limbs(b["meas"])
    ok = b["status"] == 0
    aggs = []
    for q in range(3):
        rows = np.nonzero(ok & (b["slots"] == q))[0]
        out = [x % p for x in truncate(c, column_sums(lb, rows))]
        aggs.append((to_bytes(out, es).tobytes(), len(rows)))
    # per-report output shares: the weighted limb sums fit 64 bits (bits <= 32: limb < 2^32 times
    # sum_b 2^b < 2^32), recombined in Python; rejected rows are zero
    n_out = b["v"].typ.OUTPUT_LEN
    if c["kind"] in (1, 2, 4):
        bits = c["bits"]
        assert bits <= 32
        wts = (np.uint64(1) << np.arange(bits, dtype=np.uint64))[None, None, :, None]
        t = (lb[:, :n_out * bits].reshape(n, n_out, bits, es // 4) * wts).sum(axis=2,
                                                                               dtype=np.uint64)
    else:
        t = lb
    outs = np.zeros((n, n_out, es), np.uint8)
    for r in np.nonzero(ok)[0]:
        outs[r] = to_bytes([sum(int(x) << (32 * j) for j, x in enumerate(col)) % p
                            for col in t[r]], es)
    return aggs, outs.reshape(n, n_out * es)


# ---- the run -----------------------------------------------------------------------------------
def kernel_launches(v):
    from janus_amd._lib import lib
    ms, nl = (ctypes.c_double * 128)(), (ctypes.c_uint64 * 128)()
    k = lib().prio3gpu_prof_read(v._ctx, ms, nl, 128)
    return {lib().prio3gpu_prof_kernel_name(i).decode(): int(nl[i]) for i in range(k) if nl[i]}


def run_leader(b, speculate, options):
    from janus_amd._lib import check, lib
    from janus_amd.prio3 import Prio3Gpu
    c = CONFIGS[b["name"]]
    v = Prio3Gpu(c["kind"], VK, bits=c["bits"], length=c["length"], chunk_length=c["chunk"])
    v.set_option("speculate", speculate)
    for k, x in options.items():
        v.set_option(k, x)
    n, o = b["n"], b["v"]
    ls = v.new_state(0, n)
    prep, st = v.prepare_init(ls, b["nonces"], b["pub"], b["lin"])
    msgs = None
    if o.uses_jr:
        msgs = np.zeros((n, 16), np.uint8)
        for r in range(n):
            seed = o.joint_rand_seed([prep[r, -16:].tobytes(), b["pub"][r, 16:32].tobytes()])
            msgs[r] = np.frombuffer(seed, np.uint8)
        msgs[b["bad"]["flipped"], 3] ^= 0x10
    init_status = st.copy()
    st[b["bad"]["status5"]] = 5
    agg = v.new_aggregate(3)
    check(lib().prio3gpu_prof_enable(v._ctx, 1), "prof_enable")
    kernel_launches(v)  # drain
    outs, st = v.prepare_next(ls, msgs, st, want_output_shares=True, agg=agg,
                              batch_slots=b["slots"])
    launched = kernel_launches(v)
    check(lib().prio3gpu_prof_enable(v._ctx, 0), "prof_enable")
    return dict(init_status=init_status, status=st.copy(), outs=outs,
                aggs=[agg.read(q) for q in range(3)], launched=launched)


CASES = [
    ("sumvec_small", 300, 10, {}),
    ("sumvec_small", 4200, 6, {}),
    ("hist256", 300, 0, {}),
    ("countvec15", 300, 0, {}),
    ("sum32", 300, 0, {}),
    ("sumvec_8_1000", 130, 0, {}),
    ("count", 2100, 0, {}),
    ("fp16_3", 161, 0, {}),
    ("fp16_3", 161, 0, {"jr_ring": 0}),
    ("fp16_3", 161, 0, {"pair_chains": 0}),
    ("fp16_300", 161, 0, {}),
    ("fp16_300", 161, 0, {"jr_ring": 0}),
    ("fp16_300", 161, 0, {"pair_chains": 0}),
]


def case_id(c):
    return f"{c[0]}-n{c[1]}" + "".join(f"-{k}{x}" for k, x in c[3].items())


@gpu
@pytest.mark.parametrize("name,n,shift,options", CASES, ids=[case_id(c) for c in CASES])
def test_leader_accumulation_over_edge_shares(name, n, shift, options):
    b = make_batch(name, n, shift)
    want_aggs, want_outs = reference(name, n, shift)
    bad = b["bad"]
    res = {s: run_leader(b, s, options) for s in (1, 0)}
    for s, r in res.items():
        tag = f"speculate={s}"
        init = np.zeros(n, np.uint8)
        init[[bad["elem_p"], bad["all_ff"]]] = 8    # prepare_init refuses both rows
        assert np.array_equal(r["init_status"], init), tag
        assert np.array_equal(r["status"], b["status"]), tag
        for q in range(3):
            got, cnt = r["aggs"][q]
            assert cnt == want_aggs[q][1], (tag, q)
            assert got == want_aggs[q][0], (tag, q)
        assert np.array_equal(r["outs"], want_outs), tag
    assert res[0]["aggs"] == res[1]["aggs"]
    assert np.array_equal(res[0]["outs"], res[1]["outs"])
    assert np.array_equal(res[0]["status"], res[1]["status"])
    # the path the shape is meant to take was taken
    assert "k_accum_spec" not in res[0]["launched"]
    assert ("k_accum_spec" in res[1]["launched"]) == (SPEC_RANGES.get(name) is not None)
    assert "k_accum_partial" in res[1]["launched"] and "k_accum_merge" in res[1]["launched"]


# ---- what the batches cover (no GPU needed) ------------------------------------------------------
def family_sides(name, n, shift):
    b = make_batch(name, n, shift)
    sr = SPEC_RANGES.get(name)
    inside, outside = set(), set()
    for e in range(b["L"]):
        (inside if sr and sr[1] <= e < sr[2] else outside).add(family_of(e, 0, b["L"], shift))
    return inside, outside, sr


def test_every_family_is_column_summed_and_summed_directly():
    everything = set(range(F))
    summed = {}
    for name, n, shift, _ in CASES:
        inside, outside, sr = family_sides(name, n, shift)
        L = make_batch(name, n, shift)["L"]
        if L == 1:
            continue                        # Count: one column, families by wave, no window
        n_in = sr[2] - sr[1] if sr else 0
        # a side with at least 14 columns holds every family; a narrower one, distinct families
        assert len(inside) == min(F, n_in), name
        assert len(outside) >= min(F, max(sr[1], L - sr[2]) if sr else L), name
        assert inside | outside == everything or L < F, name
        summed.setdefault(name, set()).update(inside)
    for name in ("hist256", "sum32", "sumvec_8_1000", "fp16_3", "fp16_300", "sumvec_small"):
        assert summed[name] == everything, name
    assert summed["countvec15"] == set()    # too short for a window: every column direct
    # sumvec_small, n = 300: the families whose word sums carry are the column-summed ones
    inside, outside, _ = family_sides("sumvec_small", 300, 10)
    names = [f[0] for f in FAMILIES128]
    assert {names[f] for f in inside} >= {"alt p-1 / ones", "alt p-2 / ones", "period4 carry",
                                          "period4 mixed", "exactly p", "p + 1", "halves"}
    assert {names[f] for f in outside} >= {"all p-1", "all p-2", "all ones word", "all top bit"}
    # Count: every family on some wave
    assert {family_of(0, w, 1, 0) for w in range((2100 + 63) // 64)} == everything


@pytest.mark.parametrize("name,n,shift", sorted({c[:3] for c in CASES if SPEC_RANGES.get(c[0])}))
def test_speculative_chunks_take_every_path_of_the_fold(name, n, shift):
    """For the speculative chunks this batch forms (the planner's restatement of
    tests/test_host_plan.py), the accepted rows' word sums of some (chunk, column) inside the
    window carry out of ahi + blo, pass 2^128 and leave a pre-reduction value >= p."""
    b = make_batch(name, n, shift)
    _nd, e0, e1 = SPEC_RANGES[name]
    plan = plan_restated(n, b["slots"], 3, b["L"], 1)
    assert plan["sid"], name
    ok = b["status"] == 0
    lb = limbs(b["meas"])
    seen = [0] * len(EVENTS)
    for i in range(len(plan["sid"])):
        rows = [r for w in plan["wl"][plan["swb"][i]:plan["swb"][i + 1]]
                for r in range(64 * w, min(n, 64 * w + 64)) if ok[r]]
        for s0, s1, s2, s3 in lb[rows, e0:e1].sum(axis=0, dtype=np.uint64).tolist():
            a, h = s0 + (s1 << 32), s2 + (s3 << 32)     # sums of the low and of the high words
            t = (a & (2 ** 64 - 1), a >> 64, h & (2 ** 64 - 1), h >> 64)
            for k, hit in enumerate(fold_events(*t)):
                seen[k] += hit
    for k in range(3):
        assert seen[k] > 0, f"no (chunk, column) took: {EVENTS[k]}"


# ---- aggregate merges at edges -----------------------------------------------------------------
MERGE_CONTEXTS = [("count", 0, 0, 0, 0), ("hist1", 3, 0, 1, 1), ("hist255", 3, 0, 255, 15),
                  ("hist256", 3, 0, 256, 16), ("hist257", 3, 0, 257, 16)]


def merge_vdaf(kind, bits, length, chunk):
    from janus_amd.prio3 import Prio3Gpu
    return Prio3Gpu(kind, VK, bits=bits, length=length, chunk_length=chunk)


def edge_pairs(p, n_el, seed):
    """n_el (a, b) pairs: the edge pairs spread over the elements (first, last and both sides of
    the 256-thread boundary included), random canonical pairs between them."""
    rng = np.random.default_rng(seed)
    nb = 16 if p > 2 ** 64 else 8
    top = 1 << (8 * nb - 1)
    edges = [(p - 1, p - 1), (p - 1, 1), (p - 1, 0), (1, p - 2), (top, top),
             ((p - 1) // 2, (p + 1) // 2), (0, 0)]
    pairs = []
    for i in range(n_el):
        raw = rng.bytes(2 * nb)
        pairs.append((int.from_bytes(raw[:nb], "little") % p, int.from_bytes(raw[nb:], "little") % p))
    for k, i in enumerate(sorted({0, n_el - 1, n_el // 2, *range(min(n_el, 3)),
                                  *(x for x in range(250, 258) if x < n_el)})):
        pairs[i] = edges[(k + seed) % len(edges)]
    return pairs


def enc(values, p):
    return to_bytes(values, 16 if p > 2 ** 64 else 8).tobytes()


@gpu
@pytest.mark.parametrize("label,kind,bits,length,chunk", MERGE_CONTEXTS,
                         ids=[c[0] for c in MERGE_CONTEXTS])
def test_merge_and_allreduce_at_edge_elements(label, kind, bits, length, chunk):
    from janus_amd.prio3 import Comm
    v = merge_vdaf(kind, bits, length, chunk)
    p, n_el = v.modulus, v.sizes.output_len
    assert p == (P64 if kind == 0 else P128) and n_el == max(1, length)
    agg = v.new_aggregate(2)
    for seed in range(7):               # every edge pair reaches every marked element
        pairs = edge_pairs(p, n_el, seed)
        agg.reset()
        agg.merge(1, enc([a for a, _ in pairs], p), 3)
        agg.merge(1, enc([x for _, x in pairs], p), 2 ** 40)
        got, cnt = agg.read(1)
        assert cnt == 3 + 2 ** 40
        assert got == enc([(a + x) % p for a, x in pairs], p), (label, seed)
        assert agg.read(0) == (bytes(len(got)), 0)
    # k_merge_ranks with `accumulate`: total already holds edge values, local gets fresh ones
    comm = Comm(Comm.unique_id(), 1, 0, 0)
    local, total = v.new_aggregate(2), v.new_aggregate(2)
    pairs = edge_pairs(p, n_el, 1)
    total.merge(1, enc([a for a, _ in pairs], p), 5)
    want, count = [a for a, _ in pairs], 5
    for seed in (1, 4):
        fresh = [x for _, x in edge_pairs(p, n_el, seed)]
        local.merge(1, enc(fresh, p), 7)
        comm.allreduce(v, local, total)
        want = [(a + x) % p for a, x in zip(want, fresh)]
        count += 7
        assert total.read(1) == (enc(want, p), count), (label, seed)
        assert total.read(0) == (bytes(len(enc(want, p))), 0)
        for q in range(2):
            assert local.read(q) == (bytes(len(enc(want, p))), 0), "local must be empty"
    comm.close()


@gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("label,kind,bits,length,chunk", MERGE_CONTEXTS,
                         ids=[c[0] for c in MERGE_CONTEXTS])
def test_merge_refuses_a_non_canonical_element(label, kind, bits, length, chunk, device):
    """prio's AggregateShare decoding refuses an element >= p, and so do prio3gpu_unshard and
    prio3gpu_batch_aggregation_merge: prio3gpu_agg_merge_bytes must too, before it launches
    anything (2^128 - 1 added to p - 1 would leave a non-canonical aggregate in HBM)."""
    import torch
    from janus_amd._lib import lib
    from janus_amd.prio3 import _ptr
    v = merge_vdaf(kind, bits, length, chunk)
    p, n_el, es = v.modulus, v.sizes.output_len, v.sizes.field_size
    agg = v.new_aggregate(2)
    base = [p - 1] + [(7 * i + 1) % p for i in range(1, n_el)]
    agg.merge(1, enc(base, p), 11)
    before = agg.read(1)
    assert before == (enc(base, p), 11)
    for where in sorted({0, n_el // 2, n_el - 1}):
        for x in (p, 2 ** (8 * es) - 1):
            share = [(3 * i + 2) % p for i in range(n_el)]
            share[where] = x
            buf = np.frombuffer(enc(share, 2 ** (8 * es)), np.uint8).copy()
            keep = torch.from_numpy(buf).to("cuda:0") if device else buf
            rc = lib().prio3gpu_agg_merge_bytes(agg._h, 1, _ptr(keep), 5)
            msg = lib().prio3gpu_last_error().decode()
            assert rc == -1, f"element {where} = {x:#x} was merged (rc {rc})"  # PRIO3GPU_E_ARG
            assert f"element {where} of {n_el}" in msg and "out of range" in msg, msg
            assert agg.read(1) == before and agg.read(0) == (bytes(n_el * es), 0)
    # a canonical share still merges, from the same kind of pointer
    buf = np.frombuffer(enc([1] * n_el, p), np.uint8).copy()
    keep = torch.from_numpy(buf).to("cuda:0") if device else buf
    assert lib().prio3gpu_agg_merge_bytes(agg._h, 1, _ptr(keep), 1) == 0
    assert agg.read(1) == (enc([(a + 1) % p for a in base], p), 12)
