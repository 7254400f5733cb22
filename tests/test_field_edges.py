"""The operand sets of tests/field_edges.py really contain the cases they are named for (Python
integers only, no GPU): a later edit of a generator must not silently empty a family that
tests/test_gpu_field_ops.py relies on."""
import pytest

from tests import field_edges as FE
from tests.field_edges import F64, F128, M32

BOTH = [F128, F64]


def ids(F):
    return F.name


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_edge_elements(F):
    p, R, nl = F.p, F.R, F.nl
    E = set(FE.edge_elements(F))
    assert all(0 <= x < p for x in E)
    want = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R % p + 1, R % p - 1,
            R * R % p, R * R * R % p, p - R % p}
    for k in range(nl):
        want |= {1 << (32 * k), (1 << (32 * (k + 1))) - 1 if k + 1 < nl else 0, p - (1 << (32 * k))}
    assert want <= E
    # every 0 / 0xFFFFFFFF limb pattern that is below p
    for pat in range(1 << nl):
        x = FE.from_limbs([M32 if pat >> i & 1 else 0 for i in range(nl)])
        assert min(x, p - 1) in E
    assert len(FE.edge_pairs(F)) == len(E) ** 2
    # the constants the device code carries
    if F is F128:
        assert FE.limbs(R % p, 4) == [M32, M32, 0x1B, 0]
        assert FE.limbs(R * R % p, 4) == [0xFFFFFCF1, M32, 0x5587, 0]
        assert FE.limbs(R ** 3 % p, 4) == [0xFFF6A82F, M32, 0x01054553, 0]
        assert FE.limbs(p, 4) == [1, 0, 0xFFFFFFE4, M32]
    else:
        assert FE.limbs(R % p, 2) == [M32, 0] and FE.limbs(R * R % p, 2) == [1, 0xFFFFFFFE]


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_unary_elements(F):
    xs = FE.unary_elements(F)
    assert all(0 <= x < F.p for x in xs)
    assert set(FE.edge_elements(F)) <= set(xs)
    assert sum(x < 1 << 32 for x in xs) >= 512
    assert sum(F.p - x <= 1 << 32 for x in xs) >= 512
    assert len(xs) >= 4096 + 1024 + len(FE.edge_elements(F))
    assert len(xs) <= 50_000


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_add_families(F):
    p, R, nl = F.p, F.R, F.nl
    fam = FE.add_families(F)
    pairs = FE.binary_pairs(F, "add")
    assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
    assert len(pairs) >= len(FE.edge_pairs(F)) + 4096 and len(pairs) <= 50_000
    sums = [a + b for a, b in FE._flat(fam)]
    for s in (p - 1, p, p + 1, R - 1, R, R + 1):
        assert sums.count(s) >= 1, hex(s)
    assert sum(p < s < R for s in sums) >= 100          # no carry out, yet >= p: the second chain
    assert sum(s >= R for s in sums) >= 30
    assert sum(s < p for s in sums) >= 30
    for j in range(1, min(3, nl) + 1):
        mask = (1 << (32 * j)) - 1
        for low in (0, mask):
            hit = [s for s in sums if s & mask == low]
            assert len(hit) >= 16, (j, low)
            # on both sides of the select (a whole word of ones is R - 1 alone)
            assert any(s >= p for s in hit) and (j == nl or any(s < p for s in hit)), (j, low)
    assert any(a == p - 1 or b == p - 1 for (a, b), s in zip(FE._flat(fam), sums) if p <= s < R)


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_sub_families(F):
    p, nl = F.p, F.nl
    pairs = FE._flat(FE.sub_families(F))
    assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
    assert sum(a == b for a, b in pairs) >= len(FE.edge_elements(F))
    assert sum(a - b == 1 for a, b in pairs) >= 16 and sum(b - a == 1 for a, b in pairs) >= 16
    # a - b = 1 with a borrow through every zero low limb of a
    for k in range(1, nl):
        assert (1 << (32 * k), (1 << (32 * k)) - 1) in pairs
        assert ((1 << (32 * k)) - 1, 1 << (32 * k)) in pairs
    for j in range(1, nl):
        mask = (1 << (32 * j)) - 1
        eq = [(a, b) for a, b in pairs if a != b and (a ^ b) & mask == 0]
        assert sum(a < b for a, b in eq) >= 16 and sum(a > b for a, b in eq) >= 16, j
        # equal limbs that are zero / all ones, and a difference confined to the next limb
        assert any(a & mask == 0 for a, b in eq) and any(a & mask == mask for a, b in eq)
        assert any(abs(a - b) == 1 << (32 * j) for a, b in eq)
    assert any(b - a == p - 1 for a, b in pairs) and sum(b - a == p - 2 for a, b in pairs) >= 2
    assert len(FE.binary_pairs(F, "sub")) <= 50_000


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_mul_families(F):
    p, R, nl, c = F.p, F.R, F.nl, F.c
    fam = FE.mul_families(F)
    pairs = FE._flat(fam)
    assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
    assert len(FE.binary_pairs(F, "mul")) <= 50_000
    pre = [FE.redc_presub(F, a, b) for a, b in pairs]
    assert all(0 <= t < 2 * p for t in pre)
    # the rarest branch: the unreduced value is >= p and did not carry out of the word
    assert sum(p <= t < R for t in pre) >= 100
    # a carry out with a tiny low part
    assert sum(R <= t < R + (1 << 33) for t in pre) >= 100
    # family (i): every result is d < R - p and (nearly) every draw lands on d + p
    small = fam["(i) small results"]
    assert all(a * b * F.Rinv % p < c for a, b in small)
    assert sum(p <= FE.redc_presub(F, a, b) < R for a, b in small) >= 100
    above = fam["(ii) just above"]
    assert all(c <= a * b * F.Rinv % p < c + (1 << 33) for a, b in above)
    assert sum(FE.redc_presub(F, a, b) >= R for a, b in above) >= 100
    # zero low words: a zero reduction word in the first REDC step(s)
    for k in range(1, nl):
        mask = (1 << (32 * k)) - 1
        z = [(a, b) for a, b in pairs if a and b and a & mask == 0]
        assert len(z) >= 8, k
        assert sum(b & mask == 0 for a, b in z) >= 4, k        # both operands
        assert all((a * b) & mask == 0 for a, b in z)
    assert (p - 1, p - 1) in pairs


# ---- the families catch the faults they are built for, and uniform operands do not ------------------
def _add_model(F, a, b, select):
    """Field128Ops::add's two chains: s = a + b (carry k1), u = s + (R - p) (carry k2)."""
    s = a + b
    k1, s = s >> (8 * F.es), s & (F.R - 1)
    u = s + F.c
    k2, u = u >> (8 * F.es), u & (F.R - 1)
    return u if {"k1|k2": k1 | k2, "k1": k1, "k2": k2}[select] else s


def _redc_model(F, a, b, select="full", carry="nonzero"):
    """Word-wise REDC as the device code does it: m = -T[i], the low word's sum T[i] + m replaced
    by its carry (T[i] != 0), then the final select."""
    p, T = F.p, a * b
    for i in range(F.nl):
        w = (T >> (32 * i)) & M32
        m = -w & M32
        cy = {"nonzero": int(w != 0), "always": 1, "never": 0}[carry]
        T = (((T >> (32 * (i + 1))) + cy) << (32 * (i + 1))) + ((m * (p - 1)) << (32 * i))
    t = T >> (8 * F.es)
    if select == "full":
        return t - p if t >= p else t
    if select == "carry only":                 # misses [p, R)
        return t - p if t >= F.R else t
    return (t - p if t & (F.R - 1) >= p else t) & (F.R - 1)   # "low only": ignores the carry out


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_families_catch_wrong_selects_and_carries(F):
    p = F.p
    rand = FE.rand_pairs(F, 4096, 0xB1 + F.es)
    adds, muls = FE._flat(FE.add_families(F)), FE._flat(FE.mul_families(F))
    for a, b in adds + rand + FE.edge_pairs(F):
        assert _add_model(F, a, b, "k1|k2") == (a + b) % p
    for a, b in muls + rand + FE.edge_pairs(F):
        assert _redc_model(F, a, b) == a * b * F.Rinv % p
    # k1 alone misses the sums in [p, R), k2 alone those at or above R
    for sel, least in (("k1", 100), ("k2", 30)):
        assert sum(_add_model(F, a, b, sel) != (a + b) % p for a, b in adds) >= least, sel
    assert not any(_add_model(F, a, b, "k1") != (a + b) % p for a, b in rand)
    for sel in ("carry only", "low only"):
        assert sum(_redc_model(F, a, b, sel) != a * b * F.Rinv % p for a, b in muls) >= 100, sel
    assert not any(_redc_model(F, a, b, "carry only") != a * b * F.Rinv % p for a, b in rand)
    zero_low = FE.mul_families(F)["(iii) zero low words"]
    assert sum(_redc_model(F, a, b, carry="always") != a * b * F.Rinv % p for a, b in zero_low) >= 8
    assert not any(_redc_model(F, a, b, carry="always") != a * b * F.Rinv % p for a, b in rand)
    assert any(_redc_model(F, a, b, carry="never") != a * b * F.Rinv % p for a, b in rand)


@pytest.mark.parametrize("nterms", [1, 2, 4])
def test_fused_terms(nterms):
    F = F128
    p, R, c = F.p, F.R, F.c
    tuples = FE.fused_edge_terms(F, nterms)
    assert all(len(t) == 2 * nterms and all(0 <= v < p for v in t) for t in tuples)
    if nterms == 1:
        assert set(FE._flat(FE.mul_families(F))) <= set(tuples)
        return
    assert (p - 1, p - 1) * nterms in tuples
    res = [FE.stream_reference(F, "M" if nterms == 1 else {2: "F", 4: "Q"}[nterms], t)
           for t in tuples]
    raw = [sum(t[2 * k] * t[2 * k + 1] for k in range(nterms)) for t in tuples]
    assert sum(r < c for r in res) >= 100                     # small results
    for total in (c - 1, c, c + 1):
        assert res.count(total) >= 1
    assert sum(r == 0 and s != 0 for r, s in zip(res, raw)) >= 8     # non-zero sums == 0 mod p
    small = set(FE.mul_families(F)["(i) small results"])
    zero_low = set(FE.mul_families(F)["(iii) zero low words"])
    for t in range(nterms):   # each term position carries (i) with (iii) in the others
        assert any(tup[2 * t:2 * t + 2] in small and all(
            tup[2 * u:2 * u + 2] in zero_low for u in range(nterms) if u != t) for tup in tuples), t


@pytest.mark.parametrize("op", sorted(FE.STREAMS))
def test_multi_stream_tuples(op):
    F = F128
    streams = FE.STREAMS[op]
    tuples = FE.multi_stream_tuples(F, op)
    width = [2 * FE.TERMS.get(k, 1) for k in streams]
    assert all(len(t) == sum(width) and all(0 <= v < F.p for v in t) for t in tuples)
    assert len(tuples) <= 50_000
    pools = [set(map(tuple, FE.stream_pool(F, k))) for k in streams]
    offs = [sum(width[:s]) for s in range(len(streams))]
    in_pool = [[t[offs[s]:offs[s] + width[s]] in pools[s] for s in range(len(streams))]
               for t in tuples]
    for s in range(len(streams)):
        # every edge case of the pool appears in this position with no edge case beside it
        alone = {t[offs[s]:offs[s] + width[s]] for t, ip in zip(tuples, in_pool)
                 if ip[s] and sum(ip) == 1}
        assert alone == pools[s], (op, s)
    assert sum(all(ip) for ip in in_pool) >= max(len(pl) for pl in pools)
    ref = FE.multi_stream_reference(F, op, tuples[0])
    assert len(ref) == len(streams)


def test_multi_stream_reference_order():
    """The reference follows the stream order of the signatures in mont_fma.h / mont3.h."""
    F = F128
    R = F.Rinv
    t = tuple(range(2, 16))
    assert FE.multi_stream_reference(F, "q1_fma1_mul1", t) == (
        (2 * 3 + 4 * 5 + 6 * 7 + 8 * 9) * R % F.p, (10 * 11 + 12 * 13) * R % F.p, 14 * 15 * R % F.p)
    assert FE.multi_stream_reference(F, "fma2_mul1", t[:10]) == (
        (2 * 3 + 4 * 5) * R % F.p, (6 * 7 + 8 * 9) * R % F.p, 10 * 11 * R % F.p)
    assert FE.multi_stream_reference(F, "addsub_AASS", t[:8]) == (5, 9, F.p - 1, F.p - 1)
    assert FE.multi_stream_reference(F, "addsub_ASAA", t[:8]) == (5, F.p - 1, 13, 17)


@pytest.mark.parametrize("param", FE.DOT_PARAMS)
def test_dot_tuples(param):
    F = F128
    fam = FE.dot_tuples(F, param)
    assert all(len(t) == 2 * param and all(0 <= v < F.p for v in t) for t in FE._flat(fam))
    assert fam["max"] == [(F.p - 1, F.p - 1) * param] and not any(fam["zero"][0])
    assert len(fam["random"]) >= 4
    small = set(FE.mul_families(F)["(i) small results"])
    pos = set()
    for t in fam["(i) alone"]:
        nz = [k for k in range(param) if t[2 * k] and t[2 * k + 1]]
        assert len(nz) == 1 and t[2 * nz[0]:2 * nz[0] + 2] in small
        assert FE.dot_reference(F, t) < F.c
        pos.add(nz[0])
    assert pos == {0, param // 2, param - 1}
    for t in fam["(ii) alone"]:  # a carry out of 128 bits with a tiny low part
        assert F.c <= FE.dot_reference(F, t) < F.c + (1 << 20)
    if param in (1, 2):
        assert (F.p - 1, F.p - 1) * param in fam["fused terms"]
    # column growth: the largest sum needs the carry words above 2^64 per column
    assert (F.p - 1) ** 2 * param < 1 << (256 + 30)


def test_limb_sum_inputs():
    p = F128.p
    fam = FE.limb_sum_inputs()
    assert all(len(t) == 4 and all(0 <= x < 1 << 64 for x in t) for t in FE._flat(fam))
    for k, t in zip(FE.LIMB_SUM_KS, fam["k copies of p-1"]):
        assert FE.limb_sum_value(t) == k * (p - 1)
    for k, t in zip(FE.LIMB_SUM_KS, fam["k copies of all-ones"]):
        assert FE.limb_sum_value(t) == k * ((1 << 128) - 1)
    assert (1 << 32) - 1 in FE.LIMB_SUM_KS and 0 in FE.LIMB_SUM_KS
    near = [FE.limb_sum_value(t) for t in fam["near a multiple of p"]]
    assert all(min(v % p, p - v % p) < 1 << 64 for v in near)
    assert sum(v % p < 1 << 64 for v in near) >= 100 and sum(p - v % p < 1 << 64 for v in near) >= 100
    assert sum(v >= 1 << 128 for v in near) >= 100 and sum(v < 1 << 128 for v in near) >= 20
    assert sum(any(x >> 32 for x in t) for t in fam["near a multiple of p"]) >= 100
    # values in [p, 2^128): the final subtraction without a wrap
    assert sum(p <= v < 1 << 128 for v in near) >= 1


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_canonical_inputs(F):
    p, R, nl = F.p, F.R, F.nl
    v = FE.canonical_inputs(F)
    assert all(0 <= x < R for x in v)
    assert {p - 1, p, p + 1, R - 1} <= set(v)
    pl = FE.limbs(p, nl)
    for i in range(nl):
        for d in (1, -1):
            q = list(pl)
            q[i] = (q[i] + d) & M32
            assert FE.from_limbs(q) in v
    assert sum(x >= p for x in v) >= 1000 and sum(x < p for x in v) >= 1000


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_pow_inputs(F):
    assert {0, 1} <= set(FE.POW_PARAMS) and max(FE.POW_PARAMS) < 1 << 32
    xs = FE.pow_elements(F)
    assert {0, F.R % F.p, F.p - 1} <= set(xs)
    one = F.R % F.p
    assert FE.pow_reference(F, 0, 0) == one and FE.pow_reference(F, 5, 1) == 5
    assert FE.pow_reference(F, 3 * F.R % F.p, 4) == 81 * F.R % F.p
