"""The engine's host planning (janus_amd/csrc/cfg.h, plan_cfg.h, plan_accum.h: no HIP in them)
built with g++ and checked on the CPU: the lengths of every VDAF instance against the oracle, the
Montgomery-form FLP tables against direct powers of the generator, the accumulation chunk plan
against a Python restatement and its structural properties, and the column-summed element range.
tests/native/host_plan_host.cpp is the driver (a text protocol on stdin / stdout).  The HPKE and
request routing header, plan_hpke.h, has its own driver and tests in tests/test_hpke_plan.py."""
import os
import subprocess

import numpy as np
import pytest

from oracle import prio3 as O
from tests.reports import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P128 = O.Field128.MODULUS
P64 = O.Field64.MODULUS


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_plan") / "host_plan_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(out),
                    os.path.join(ROOT, "tests", "native", "host_plan_host.cpp")], check=True)
    return str(out)


def run(plan_bin, lines):
    out = subprocess.run([plan_bin], input=("\n".join(lines) + "\n").encode(),
                         capture_output=True, check=True).stdout.decode()
    return out.splitlines()


# ---- derive_cfg --------------------------------------------------------------------------------
SHAPES = {name: (c["kind"], c["bits"], c["length"], c["chunk"], c["ctor"])
          for name, c in CONFIGS.items()}
SHAPES["bench_sum32"] = (1, 32, 0, 0, lambda: O.Prio3.new_sum(32))
SHAPES["bench_fp16_100000"] = (4, 16, 100000, 0,
                               lambda: O.Prio3.new_fixedpoint_boundedl2_vec_sum(16, 100000))


def test_derive_cfg_lengths_match_the_oracle(plan_bin):
    names = list(SHAPES)
    out = run(plan_bin, ["cfg %d %d %d %d" % SHAPES[k][:4] for k in names])
    assert len(out) == len(names)
    for name, line in zip(names, out):
        f = line.split()
        assert f[0] == "ok", (name, line)
        (es, meas_len, proof_len, verifier_len, jr_len, out_len, prove_rand_len, leader, helper,
         public, prep_share, prep_msg, _m, _calls, _chunk) = map(int, f[1:16])
        v = SHAPES[name][4]()
        t = v.typ
        assert es == v.fld.ENCODED_SIZE, name
        assert meas_len == t.MEAS_LEN, name
        assert proof_len == O.proof_len(t), name
        assert verifier_len == O.verifier_len(t), name
        assert jr_len == t.JOINT_RAND_LEN, name
        assert out_len == t.OUTPUT_LEN, name
        assert prove_rand_len == t.PROVE_RAND_LEN, name
        assert leader == v.leader_input_share_len(), name
        assert helper == v.helper_input_share_len(), name
        assert prep_share == v.prep_share_len(), name
        assert public == v.public_share_len(), name
        assert prep_msg == v.prep_msg_len(), name
        # the prio3gpu_sizes fill reports the same lengths
        assert list(map(int, f[16:])) == [es, meas_len, proof_len, verifier_len, jr_len, out_len,
                                          leader, helper, public, prep_share, prep_msg,
                                          out_len * es], name


def test_derive_cfg_rejects_bad_shapes(plan_bin):
    bad = ["cfg 1 0 0 0", "cfg 1 65 0 0",      # Sum: bits 0, 65
           "cfg 2 8 1000 0",                    # SumVec: chunk 0
           "cfg 4 8 3 0",                       # FixedPoint: bits 8
           "cfg 2 1 5000 1",                    # 5,000 calls: m = 8192 > 4096
           "cfg 7 1 1 1"]                       # no such kind
    out = run(plan_bin, bad + ["cfg 2 1 4095 1"])
    assert len(out) == len(bad) + 1
    for cmd, line in zip(bad, out):
        assert line.startswith("err ") and len(line) > 4, (cmd, line)
    assert out[-1].startswith("ok "), out[-1]   # m = 4096 is the largest gadget


def test_optimal_chunk_length_matches_the_oracle(plan_bin):
    out = run(plan_bin, ["chunks 1 5000", "chunks 1600030 1600030"])
    got = list(map(int, out[0].split()))
    assert got == [O.optimal_chunk_length(n) for n in range(1, 5001)]
    assert int(out[1]) == O.optimal_chunk_length(1600030)


# ---- tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,calls,es", [(2, 1, 8), (4, 2, 16), (8, 5, 16), (128, 90, 16),
                                        (64, 33, 8)])
def test_flp_tables_out_of_montgomery_form(plan_bin, m, calls, es):
    p = P128 if es == 16 else P64
    r_inv = pow(1 << (8 * es), -1, p)
    out = run(plan_bin, [f"gadget {m} {calls} {es}", f"prover {m} {es}"])
    gad = [int(x, 16) * r_inv % p for x in out[0].split()]
    prv = [int(x, 16) * r_inv % p for x in out[1].split()]
    for line in out:   # Montgomery representatives are canonical
        assert all(int(x, 16) < p and len(x) == 2 * es for x in line.split())
    alpha = pow(7, (p - 1) // m, p)
    inv_m = pow(m, -1, p)
    assert pow(alpha, m, p) == 1 and pow(alpha, m // 2, p) != 1
    assert len(gad) == 3 * m + 1
    assert gad[:m] == [pow(alpha, k, p) for k in range(m)]
    assert gad[m] == inv_m
    assert gad[m + 1:2 * m + 1] == [sum(pow(alpha, i * k, p) for k in range(1, calls + 1)) % p
                                    for i in range(m)]
    assert gad[2 * m + 1:] == [pow(alpha, k, p) * inv_m % p for k in range(m)]
    w = pow(7, (p - 1) // (2 * m), p)
    assert pow(w, 2 * m, p) == 1 and pow(w, m, p) != 1
    assert len(prv) == 2 * m + 2
    assert prv[:2 * m] == [pow(w, k, p) for k in range(2 * m)]
    assert prv[2 * m] == inv_m
    assert prv[2 * m + 1] == pow(2 * m, -1, p)


# ---- the accumulation plan ---------------------------------------------------------------------
WCH = 32


def direct_chunk(n, meas_len):
    epb = min(256, max(1, meas_len))
    tiles = -(-meas_len // epb)
    return max(256 // epb * 4, -(-n // max(1, 2048 // tiles)))


def plan_restated(n, slots, S, meas_len, spec):
    """launch_accumulate's planner as the engine had it before it moved to plan_accum.h."""
    slot = (lambda r: int(slots[r])) if slots is not None else (lambda r: 0)
    spec_w = [[] for _ in range(S)]
    direct = [[] for _ in range(S)]
    for w in range((n + 63) // 64):
        rs = range(64 * w, min(n, 64 * w + 64))
        if spec and all(slot(r) == slot(rs[0]) for r in rs):
            spec_w[slot(rs[0])].append(w)
        else:
            for r in rs:
                direct[slot(r)].append(r)
    CH = direct_chunk(n, meas_len)
    perm, cb, cs, dir_ids, spec_ids, swb, wl = [], [], [], [], [], [], []
    for s in range(S):
        for i in range(0, len(spec_w[s]), WCH):
            spec_ids.append(len(cs))
            cb.append(len(perm))
            cs.append(s)
            swb.append(len(wl))
            for w in spec_w[s][i:i + WCH]:
                wl.append(w)
                perm.extend(range(64 * w, min(n, 64 * w + 64)))
        for i in range(0, len(direct[s]), CH):
            dir_ids.append(len(cs))
            cb.append(len(perm))
            cs.append(s)
            perm.extend(direct[s][i:i + CH])
    cb.append(len(perm))
    swb.append(len(wl))
    return dict(perm=perm, cb=cb, cs=cs, dir=dir_ids, sid=spec_ids, swb=swb, wl=wl)


def slot_patterns(n, S):
    r = np.arange(n)
    mixed = np.zeros(n, np.uint32)
    w0 = 64 * ((n // 64) // 2)      # one wave in the middle holds every slot
    mixed[w0:w0 + 64] = r[w0:w0 + 64] % S
    return {"null": None,
            "one_slot": np.full(n, S - 1, np.uint32),
            "per_wave": (r // 64 % S).astype(np.uint32),
            "one_mixed_wave": mixed,
            "per_report": (r % S).astype(np.uint32)}


def spec_fold_slots():
    """tests/test_gpu_spec.py::test_sumvec_8_1000_multichunk_fold_bytes_vs_c_restatement"""
    slots = np.zeros(4200, np.uint32)
    slots[2304:4096] = 1
    slots[4096:4160] = np.random.default_rng(3).integers(0, 3, 64)
    slots[4160:] = 2
    return slots


def accum_cases():
    cases = []
    for meas_len in (32, 8000):     # one tile with 8 report groups; 32 tiles
        for n in (1, 63, 64, 65, 129, 300, 4200):
            for S in (1, 3):
                for name, slots in slot_patterns(n, S).items():
                    for spec in (0, 1):
                        cases.append((f"{name}-n{n}-S{S}", n, S, meas_len, spec, slots))
    for spec in (0, 1):
        cases.append(("spec_fold", 4200, 3, 8000, spec, spec_fold_slots()))
    return cases


def accum_cmd(n, S, meas_len, spec, slots):
    tail = "0" if slots is None else f"{n} " + " ".join(map(str, slots.tolist()))
    return f"accum {n} {S} {meas_len} {spec} {tail}"


def parse_plan(lines):
    head = lines[0].split()
    assert head[0] == "ok", lines[0]
    plan = dict(zip(("ndir", "nspec", "nch", "CH", "WCH"), map(int, head[1:])))
    for line, key in zip(lines[1:8], ("perm", "cb", "cs", "dir", "sid", "swb", "wl")):
        f = line.split()
        assert f[0] == key
        plan[key] = list(map(int, f[1:]))
    f = lines[8].split()
    assert f[0] == "layout"
    plan["layout"] = list(map(int, f[1:]))
    return plan


@pytest.fixture(scope="module")
def accum_plans(plan_bin):
    cases = accum_cases()
    out = run(plan_bin, [accum_cmd(*c[1:]) for c in cases])
    assert len(out) == 9 * len(cases)
    return [(c, parse_plan(out[9 * i:9 * i + 9])) for i, c in enumerate(cases)]


def test_accum_plan_equals_the_restatement(accum_plans):
    for (name, n, S, meas_len, spec, slots), got in accum_plans:
        want = plan_restated(n, slots, S, meas_len, spec)
        for key, arr in want.items():
            assert got[key] == arr, (name, meas_len, spec, key)
        assert (got["ndir"], got["nspec"], got["nch"]) == (len(want["dir"]), len(want["sid"]),
                                                           len(want["cs"])), name
        assert got["CH"] == direct_chunk(n, meas_len) and got["WCH"] == WCH


def test_accum_plan_properties(accum_plans):
    for (name, n, S, meas_len, spec, slots), g in accum_plans:
        tag = (name, meas_len, spec)
        slot = (lambda r: int(slots[r])) if slots is not None else (lambda r: 0)
        perm, cb, cs, nch = g["perm"], g["cb"], g["cs"], g["nch"]
        assert sorted(perm) == list(range(n)), tag       # every report exactly once
        assert len(cs) == nch and len(cb) == nch + 1 and cb[0] == 0 and cb[-1] == n, tag
        assert all(cb[k] < cb[k + 1] for k in range(nch)), tag
        for k in range(nch):                             # a chunk's reports share its slot
            assert {slot(r) for r in perm[cb[k]:cb[k + 1]]} == {cs[k]}, tag
        runs = [s for k, s in enumerate(cs) if k == 0 or cs[k - 1] != s]
        assert len(runs) == len(set(runs)), tag          # one slot's chunks are consecutive
        assert sorted(g["dir"] + g["sid"]) == list(range(nch)), tag
        if not spec:
            assert g["sid"] == [] and g["wl"] == [], tag
        swb, wl = g["swb"], g["wl"]
        assert len(swb) == g["nspec"] + 1 and swb[0] == 0 and swb[-1] == len(wl), tag
        assert len(set(wl)) == len(wl), tag
        for i, k in enumerate(g["sid"]):                 # whole uniform waves, at most 32
            waves = wl[swb[i]:swb[i + 1]]
            assert 1 <= len(waves) <= WCH, tag
            rows = [r for w in waves for r in range(64 * w, min(n, 64 * w + 64))]
            assert perm[cb[k]:cb[k + 1]] == rows, tag
            assert {slot(r) for r in rows} == {cs[k]}, tag
        for k in g["dir"]:
            assert cb[k + 1] - cb[k] <= g["CH"], tag
        # the packed device buffers: chunks = cb | cs, spec_idx = dir | sid | swb | wl
        o_cb, o_cs, chunks_len, o_dir, o_sid, o_swb, o_wl, idx_len = g["layout"]
        for spans, total in (([(o_cb, nch + 1), (o_cs, nch)], chunks_len),
                             ([(o_dir, g["ndir"]), (o_sid, g["nspec"]),
                               (o_swb, g["nspec"] + 1), (o_wl, len(wl))], idx_len)):
            end = 0
            for off, ln in sorted(spans):
                assert off >= end, tag
                end = off + ln
            assert end <= total, tag


def test_accum_plan_rejects_a_slot_out_of_range(plan_bin):
    slots = np.zeros(130, np.uint32)
    slots[77] = 3
    out = run(plan_bin, [accum_cmd(130, 3, 32, 1, slots), accum_cmd(130, 3, 32, 0, slots),
                         accum_cmd(130, 4, 32, 1, slots)])
    assert out[0].startswith("err ") and "3" in out[0]
    assert out[1].startswith("err ")
    assert out[2].startswith("ok ")


# ---- spec_range --------------------------------------------------------------------------------
# (nd, e0, e1) of every Field128 CONFIGS entry with joint randomness, as the engine computed them
# before spec_range moved to plan_accum.h; None: the share is too short for a column-summed range.
SPEC_RANGES = {
    "sum8": None, "sum32": (64, 8, 29), "sum5": None, "sum1": None, "sum2": None, "sum4": None,
    "sum16": None, "sum64": (128, 8, 60),
    "sumvec_small": (40, 8, 18), "countvec15": None, "sumvec_8_1000": (16000, 8, 7998),
    "sumvec_odd_calls": (1300, 8, 648), "sumvec_chunk128": (2000, 8, 995),
    "sumvec_chunk65": (1800, 8, 890), "hist4": None, "sumvec_calls1": None, "hist_calls1": None,
    "sumvec_calls3": None, "hist256": (512, 8, 249),
    "fp16_3": (156, 8, 71), "fp32_5": (444, 8, 218), "fp64_4": (764, 8, 375),
    "fp16_300": (9660, 8, 4827), "fp16_5000": (160060, 8, 80028),
}


def test_spec_range_literals(plan_bin):
    names = [k for k, c in CONFIGS.items() if c["kind"] != 0]
    assert sorted(names) == sorted(SPEC_RANGES)
    out = run(plan_bin, ["spec %d %d %d %d" % SHAPES[k][:4] for k in names]
              + ["spec 0 0 0 0"])
    assert out[-1] == "none"        # Count: Field64, no joint randomness
    for name, line in zip(names, out):
        want = SPEC_RANGES[name]
        if want is None:
            assert line == "none", name
            continue
        nd, e0, e1 = want
        assert line == f"ok {nd} {e0} {e1}", name
        meas_len = SHAPES[name][4]().typ.MEAS_LEN
        assert e0 == 8 and e1 <= meas_len and 2 * e1 <= nd, name
