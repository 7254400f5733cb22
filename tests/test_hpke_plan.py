"""The helper's HPKE and request routing (janus_amd/csrc/plan_hpke.h: no HIP in it) built with g++
and checked on the CPU against a Python restatement of its rules: which key opens a report, which
reports form the GPU's key groups and which are the host's in the two modes, the second trial with
a global key, the plaintext offsets, the host fallback's sets and packed upload, and the checks of
a request's views.  tests/native/hpke_plan_host.cpp is the driver (a text protocol on stdin /
stdout)."""
import os
import random
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X25519, P256 = 0x20, 0x10
REQ_DEFER, REQ_HOST = 0xFE, 0xFF
E_ARG, E_CAPACITY = -1, -4

Key = namedtuple("Key", "id kem kdf aead sklen pklen skp pkp", defaults=(32, 32, 1, 1))
Report = namedtuple("Report", "id status enc_len payload_len", defaults=(0, 32, 40))


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("hpke_plan") / "hpke_plan_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(out),
                    os.path.join(ROOT, "tests", "native", "hpke_plan_host.cpp")], check=True)
    return str(out)


def run(plan_bin, lines):
    out = subprocess.run([plan_bin], input=("\n".join(lines) + "\n").encode(),
                         capture_output=True, check=True).stdout.decode()
    return out.splitlines()


def flat(task, glob, reports):
    f = [len(task), len(glob)]
    for k in list(task) + list(glob):
        f += list(k)
    f.append(len(reports))
    for r in reports:
        f += list(r)
    return " ".join(map(str, f))


# ---- the rules, restated -------------------------------------------------------------------------
def gpu_suite(opt, kem, kdf, aead):
    if kem != X25519:
        return False
    return (kdf, aead) == (1, 1) or (bool(opt) and kdf in (1, 2, 3) and aead in (1, 2, 3))


def first(keys, cid):
    return next((j for j, k in enumerate(keys) if k.id == cid), None)


def model_plan(opt, strict, task, glob, reports):
    keys = list(task) + list(glob)
    route, groups = [], []
    for r in reports:
        t, g = first(task, r.id), first(glob, r.id)
        ki = t if t is not None else None if g is None else len(task) + g
        if r.status:
            route.append("F")
        elif ki is None:
            route.append("H" if strict else "U")
        else:
            k = keys[ki]
            ok = (gpu_suite(opt, k.kem, k.kdf, k.aead) and k.skp and k.pkp and k.sklen == 32
                  and k.pklen == 32)
            if strict:
                ok = ok and r.enc_len == 32 and r.payload_len >= 16
            if ok and ki not in groups:
                groups.append(ki)
            route.append(groups.index(ki) if ok else "H")
    members = [[i for i, x in enumerate(route) if x == k] for k in range(len(groups))]
    gbeg = [0]
    for m in members:
        gbeg.append(gbeg[-1] + len(m))
    is_task = [int(ki < len(task)) for ki in groups]
    retry = [int(x not in ("F", "U", "H") and is_task[x] == 1 and first(glob, r.id) is not None)
             for x, r in zip(route, reports)]
    offsets = [0]
    for r in reports:
        offsets.append(offsets[-1] + max(r.payload_len - 16, 0))
    return dict(route=[str(x) for x in route], groups=groups, task=is_task,
                idx=[i for m in members for i in m], gbeg=gbeg, retry=retry, offsets=offsets)


def parse_plan(lines):
    got = {}
    for line in lines:
        name, *vals = line.split()
        got[name] = vals if name == "route" else list(map(int, vals))
    return got


def plans(plan_bin, cases):
    """cases: (opt, strict, task, glob, reports) -> the driver's plan of each."""
    out = run(plan_bin, ["plan %d %d %s" % (o, s, flat(t, g, r)) for o, s, t, g, r in cases])
    assert len(out) == 7 * len(cases)
    return [parse_plan(out[7 * i:7 * i + 7]) for i in range(len(cases))]


def check_structure(p, n):
    assert len(p["gbeg"]) == len(p["groups"]) + 1 and p["gbeg"][0] == 0
    assert p["gbeg"][-1] == len(p["idx"]) and len(set(p["idx"])) == len(p["idx"])
    seen_first = []
    for k in range(len(p["groups"])):
        m = p["idx"][p["gbeg"][k]:p["gbeg"][k + 1]]
        assert m and m == sorted(m) and all(p["route"][i] == str(k) for i in m)
        seen_first.append(m[0])
    assert seen_first == sorted(seen_first)      # groups in order of first appearance
    assert sorted(p["idx"]) == [i for i in range(n) if p["route"][i] not in ("F", "U", "H")]


# ---- routing -------------------------------------------------------------------------------------
def test_empty_and_keyless(plan_bin):
    reps = [Report(1), Report(2, 4)]
    (e0, e1, u, h) = plans(plan_bin, [(0, 0, [], [], []), (1, 1, [Key(1, X25519, 1, 1)], [], []),
                                      (0, 0, [], [], reps), (0, 1, [], [], reps)])
    for e in (e0, e1):
        assert e == dict(route=[], groups=[], task=[], idx=[], gbeg=[0], retry=[], offsets=[0])
    assert u["route"] == ["U", "F"] and h["route"] == ["H", "F"]
    assert u["groups"] == h["groups"] == [] and u["offsets"] == [0, 24, 48]


def test_key_choice(plan_bin):
    """Ids: 1 task only, 2 global only, 3 in both, 4 in neither, 5 twice in each list; task key 3
    and global key 3 are byte-identical keypairs, as are the duplicates."""
    task = [Key(1, X25519, 1, 1), Key(3, X25519, 1, 1), Key(5, X25519, 1, 1), Key(5, X25519, 1, 1)]
    glob = [Key(3, X25519, 1, 1), Key(2, X25519, 1, 1), Key(5, X25519, 1, 1), Key(5, X25519, 1, 1)]
    reps = [Report(i) for i in (3, 2, 1, 4, 5, 3, 2)]
    for strict, p in enumerate(plans(plan_bin, [(0, 0, task, glob, reps),
                                                (0, 1, task, glob, reps)])):
        assert p == model_plan(0, strict, task, glob, reps)
        assert p["route"] == ["0", "1", "2", "H" if strict else "U", "3", "0", "1"]
        assert p["groups"] == [1, 5, 0, 2] and p["task"] == [1, 0, 1, 1]
        assert p["retry"] == [1, 0, 0, 0, 1, 1, 0]
        check_structure(p, len(reps))
    # the first choice is a global key: no second trial; equal bytes, two addresses, two groups
    (p,) = plans(plan_bin, [(0, 0, [], glob[:1] * 2 + glob[1:2], [Report(3), Report(2)])])
    assert p["groups"] == [0, 2] and p["task"] == [0, 0] and p["retry"] == [0, 0]
    same = [Key(1, X25519, 1, 1), Key(2, X25519, 1, 1)]
    (p,) = plans(plan_bin, [(0, 0, same, [], [Report(2), Report(1), Report(2)])])
    assert p["groups"] == [1, 0] and p["idx"] == [0, 2, 1] and p["gbeg"] == [0, 2, 3]


def test_suites_and_key_shapes(plan_bin):
    def route(opt, key):
        return [(opt, s, [key], [], [Report(key.id)]) for s in (0, 1)]
    gpu_always = [Key(1, X25519, 1, 1)]
    gpu_opt = [Key(1, X25519, 2, 3), Key(1, X25519, 3, 2)]
    host = ([Key(1, P256, 1, 1)] + [Key(1, X25519, kdf, 1) for kdf in (0, 4)]
            + [Key(1, X25519, 1, aead) for aead in (0, 4, 0xFFFF)]
            + [Key(1, X25519, 1, 1, 31, 32), Key(1, X25519, 1, 1, 32, 33),
               Key(1, X25519, 1, 1, 32, 32, 0, 1), Key(1, X25519, 1, 1, 32, 32, 1, 0)])
    cases, want = [], []
    for opt in (0, 1):
        for k in gpu_always + gpu_opt + host:
            cases += route(opt, k)
            want += 2 * ["0" if k in gpu_always or (opt and k in gpu_opt) else "H"]
    got = plans(plan_bin, cases)
    assert [p["route"][0] for p in got] == want
    for p, c in zip(got, cases):
        assert p == model_plan(*c)


def test_incoming_status_and_shapes(plan_bin):
    task = [Key(1, X25519, 1, 1)]
    reps = ([Report(1, 0, 32, pl) for pl in (0, 15, 16, 17)] + [Report(1, 4, 32, 20), Report(9, 8)]
            + [Report(1, 0, enc, 40) for enc in (31, 33, 32)])
    req, strict = plans(plan_bin, [(0, 0, task, [], reps), (0, 1, task, [], reps)])
    assert req["offsets"] == strict["offsets"] == [0, 0, 0, 0, 1, 5, 29, 53, 77, 101]
    assert req["route"] == ["0", "0", "0", "0", "F", "F", "0", "0", "0"]
    assert strict["route"] == ["H", "H", "0", "0", "F", "F", "H", "H", "0"]
    assert req["idx"] == [0, 1, 2, 3, 6, 7, 8] and strict["idx"] == [2, 3, 8]
    for p in (req, strict):
        check_structure(p, len(reps))


SUITES = [(X25519, 1, 1), (X25519, 2, 3), (X25519, 3, 2), (P256, 1, 1), (X25519, 4, 1)]


def random_case(rng, n):
    def keys():
        return [Key(rng.randrange(4), *rng.choice(SUITES), rng.choice((32, 32, 32, 31)), 32,
                    rng.choice((1, 1, 1, 0)), 1) for _ in range(rng.randrange(4))]
    reps = [Report(rng.randrange(4), rng.choice((0, 0, 0, 3, 4, 8)), rng.choice((32, 32, 32, 31)),
                   rng.choice((0, 15, 16, 17, 40, 200))) for _ in range(n)]
    return keys(), keys(), reps


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_plans_match_the_restatement(plan_bin, seed):
    rng = random.Random(seed)
    cases = []
    for n in (1, 63, 64, 65, 300):
        task, glob, reps = random_case(rng, n)
        cases += [(opt, strict, task, glob, reps) for opt in (0, 1) for strict in (0, 1)]
    for p, c in zip(plans(plan_bin, cases), cases):
        assert p == model_plan(*c)
        check_structure(p, len(c[4]))


def test_info_string(plan_bin):
    assert run(plan_bin, ["info 1 3"]) == [(b"dap-07 input share" + bytes([1, 3])).hex()]


# ---- the host fallback ---------------------------------------------------------------------------
def fallback(plan_bin, opt, want, task, glob, reps, image):
    out = run(plan_bin, ["fallback %d %d %s %s" % (opt, want, flat(task, glob, reps),
                                                   " ".join(map(str, image)))])
    assert len(out) == 4, out
    host, retry = (list(map(int, out[i].split()[1:])) for i in (0, 1))
    return host, retry, tuple(map(int, out[2].split()[1:])), bytes.fromhex(out[3].split()[1])


def test_fallback_sets(plan_bin):
    """Group 0: task key 1 with a global key of its id; group 1: task key 2 without one; group 2:
    global key 3.  Report 9 came in with a decrypt error and is nobody's."""
    task = [Key(1, X25519, 1, 1), Key(2, X25519, 1, 1), Key(4, P256, 1, 1)]
    glob = [Key(3, X25519, 1, 1), Key(1, X25519, 1, 1)]
    reps = [Report(i) for i in (1, 2, 3, 4, 1, 1, 2, 3, 1)] + [Report(1, 4)]
    image = [4, 4, 4, REQ_HOST, REQ_DEFER, 8, 0, REQ_DEFER, 0, 4]
    host, retry, layout, _ = fallback(plan_bin, 0, 16, task, glob, reps, image)
    assert host == [3, 4, 7] and retry == [0]
    assert layout == (4, 16, 16 + 4 * 16, 16 + 4 * 16 + 4)


@pytest.mark.parametrize("want", [16, 33])
@pytest.mark.parametrize("kf", [1, 3, 4, 5])
def test_fallback_packing(plan_bin, kf, want):
    task, glob = [Key(1, X25519, 1, 1), Key(2, P256, 1, 1)], [Key(1, X25519, 1, 1)]
    picks = [1, 2, 4, 7, 8][:kf]                 # alternately a retry and a host report
    reps = [Report(1 if picks.index(i) % 2 == 0 else 2) if i in picks else Report(1)
            for i in range(10)]
    image = [(4 if picks.index(i) % 2 == 0 else REQ_HOST) if i in picks else 0 for i in range(10)]
    host, retry, layout, fb = fallback(plan_bin, 0, want, task, glob, reps, image)
    assert sorted(host + retry) == picks and retry == picks[0::2] and host == picks[1::2]
    o_rows = (4 * kf + 15) // 16 * 16
    o_st = o_rows + kf * want
    assert layout == (kf, o_rows, o_st, o_st + kf) and len(fb) == o_st + kf
    exp = bytearray(o_st + kf)
    for j, i in enumerate(picks):
        exp[4 * j:4 * j + 4] = i.to_bytes(4, "little")
        exp[o_rows + j * want:o_rows + (j + 1) * want] = bytes((7 * i + 3 * b + 1) & 255
                                                               for b in range(want))
        exp[o_st + j] = (5 * i + 2) & 255
    assert fb == bytes(exp)


# ---- the request's views -------------------------------------------------------------------------
def test_span_fits(plan_bin):
    cases = [(84, 16, 100, 1), (100, 0, 100, 1), (101, 0, 100, 0), (85, 16, 100, 0),
             (2**64 - 8, 16, 100, 0), (2**64 - 8, 16, 2**64 - 1, 0), (0, 2**64 - 1, 2**64 - 1, 1)]
    out = run(plan_bin, ["span %d %d %d" % c[:3] for c in cases])
    assert list(map(int, out)) == [c[3] for c in cases]


def test_check_request_views(plan_bin):
    def view(i, **kw):
        f = dict.fromkeys("rid pso psl eo el po pl prso prsl pmo pml".split(), 0)
        f.update(kw)
        return "%d %s" % (i, " ".join(str(f[k]) for k in f))
    msg_len = 100
    good = view(0, rid=84, pso=100, eo=68, el=32, po=0, pl=100, prso=99, prsl=1)
    bad = {"rid": dict(rid=85), "pso": dict(pso=101), "el": dict(eo=69, el=32),
           "po": dict(po=2**64 - 8, pl=16), "prsl": dict(prso=50, prsl=51),
           "pml": dict(pmo=100, pml=1)}
    lines = ["views 32 64 %d 3 1 %s" % (msg_len, good)]
    lines += ["views 32 64 %d 4 2 %s %s" % (msg_len, view(3, **kw), view(2, **kw))
              for kw in bad.values()]
    out = run(plan_bin, lines)
    assert out[0] == "ok"
    assert out[1:] == ["err %d view 2 does not fit the 100-byte message" % E_ARG] * len(bad)


def gather_blocks(pub, prep, n):
    return (n * max(1, (max(pub, prep) + 15) // 16) + 255) // 256


def test_req_gather_blocks_and_capacity(plan_bin):
    n = 0x7FFFFFFF
    shapes = [(0, 0), (16, 1), (17, 32), (32, 33), (100000, 48), (0xFFFFFFF0, 16)]
    out = run(plan_bin, ["blocks %d %d %d" % (a, b, n) for a, b in shapes])
    assert list(map(int, out)) == [gather_blocks(a, b, n) for a, b in shapes]
    assert [gather_blocks(a, b, n) > 0x7FFFFFFF for a, b in shapes] == [0, 0, 0, 0, 1, 1]
    # the capacity rule through check_request_views, at the first n over the limit
    pub = 0xFFFFFFF0
    n_over = next(k for k in range(2040, 2060) if gather_blocks(pub, 0, k) > 0x7FFFFFFF)
    assert gather_blocks(pub, 0, n_over - 1) <= 0x7FFFFFFF
    out = run(plan_bin, ["views %d 0 16 %d 0" % (pub, k) for k in (n_over - 1, n_over)])
    assert out == ["ok", "err %d job too large for one gather launch" % E_CAPACITY]


# ---- the suites of the three families of entry points --------------------------------------------
OPT_SUITES, OPT_P256, OPT_TEAM_CHACHA = 1, 2, 4


def suites_model(opts, kem, kdf, aead):
    """(hpke_gpu_suite, hpke_team_suite, hpke_seal_suite), restated."""
    kem_ok = kem == X25519 or (kem == P256 and bool(opts & OPT_P256))
    nine = kdf in (1, 2, 3) and aead in (1, 2, 3)
    gpu = kem_ok and ((kdf, aead) == (1, 1) or (bool(opts & OPT_SUITES) and nine))
    team = kem_ok and nine and (aead != 3 or bool(opts & OPT_TEAM_CHACHA))
    return int(gpu), int(team), int(kem_ok and nine)


def test_suite_predicates_over_the_full_table(plan_bin):
    table = [(o, kem, kdf, aead) for o in range(8) for kem in (P256, X25519, 0x21)
             for kdf in range(5) for aead in range(5)]
    out = run(plan_bin, ["suites %d %d %d %d" % t for t in table])
    got = dict(zip(table, (tuple(map(int, line.split())) for line in out)))
    assert len(out) == len(table) == 600
    assert got == {t: suites_model(*t) for t in table}
    # the restatement itself, at the corners: (open a lane, a wave per report, seal a lane)
    assert got[(0, X25519, 1, 1)] == (1, 1, 1) and got[(0, X25519, 1, 3)] == (0, 0, 1)
    assert got[(OPT_SUITES, X25519, 3, 3)] == (1, 0, 1)
    assert got[(OPT_TEAM_CHACHA, X25519, 2, 3)] == (0, 1, 1)
    assert got[(OPT_SUITES | OPT_TEAM_CHACHA, P256, 1, 1)] == (0, 0, 0)
    assert got[(OPT_P256, P256, 1, 1)] == (1, 1, 1) and got[(OPT_P256, P256, 2, 2)] == (0, 1, 1)
    assert got[(7, P256, 3, 3)] == (1, 1, 1) and got[(7, 0x21, 1, 1)] == (0, 0, 0)
    assert got[(7, X25519, 0, 1)] == got[(7, X25519, 4, 1)] == got[(7, X25519, 1, 4)] == (0, 0, 0)


# ---- the column geometry of the input-share seals and open ---------------------------------------
def columns_model(kem, slen, ep, pp, sp):
    nenc, plen = (65 if kem == P256 else 32), 6 + slen + 16
    e, p, s = ep or nenc, pp or plen, sp or slen
    oks = [int(e >= nenc), int(p >= plen), int(s >= slen)]
    return (nenc, plen, e, p, s, *oks, int(all(oks)))


@pytest.mark.parametrize("kem,nenc", [(X25519, 32), (P256, 65)])
def test_share_columns(plan_bin, kem, nenc):
    slen, plen = 100, 122
    cases = [(kem, slen, 0, 0, 0),                        # packed
             (kem, slen, nenc, plen, slen),               # pitch = width
             (kem, slen, nenc - 1, plen, slen),           # one column a byte short, in turn
             (kem, slen, nenc, plen - 1, slen),
             (kem, slen, nenc, plen, slen - 1),
             (kem, slen, nenc + 7, 4096, slen + 1),       # gaps
             (kem, 0, 0, 0, 0), (kem, 0, 0, 21, 0),       # an empty share: the payload is 22 bytes
             (kem, 0xFFFFFFFF, 0, 0, 0),                  # no 32-bit wrap
             (kem, 0xFFFFFFFF, 0, 0xFFFFFFFF + 21, 0xFFFFFFFE)]
    out = run(plan_bin, ["columns %d %d %d %d %d" % c for c in cases])
    got = [tuple(map(int, line.split())) for line in out]
    assert got == [columns_model(*c) for c in cases]
    assert got[0] == got[1] == (nenc, plen, nenc, plen, slen, 1, 1, 1, 1)
    assert [g[5:] for g in got[2:6]] == [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 1)]
    assert got[6] == (nenc, 22, nenc, 22, 0, 1, 1, 1, 1) and got[7][5:] == (1, 0, 1, 0)
    assert got[8] == (nenc, 2**32 + 21, nenc, 2**32 + 21, 2**32 - 1, 1, 1, 1, 1)
    assert got[9][5:] == (1, 0, 0, 0)


def test_rows_span(plan_bin):
    big = 6 + 0xFFFFFFFF + 16
    cases = [(1, 0, 7), (1, 4096, 122), (2, 122, 122), (3, 10, 4), (5, 32, 0),
             (0x7FFFFFFF, big, big), (0x7FFFFFFF, 2**32, 0xFFFFFFFF)]
    out = run(plan_bin, ["rows %d %d %d" % c for c in cases])
    assert list(map(int, out)) == [(n - 1) * pitch + width for n, pitch, width in cases]
    assert list(map(int, out[:4])) == [7, 122, 244, 24]      # n = 1: the row's own width
    assert all(int(x) > 2**62 for x in out[5:])              # and nothing wrapped at 32 bits
