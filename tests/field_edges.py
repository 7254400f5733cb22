"""Operand sets and exact references for tests/test_gpu_field_ops.py (prio3gpu_test_field_op): the
edge operands of Field128 / Field64 arithmetic that uniform XOF output never produces, as plain
Python integers.  No GPU and no library is needed to import this module;
tests/test_field_edges.py checks on the CPU that every family below really contains its cases.

Every generator is seeded and deterministic, and the sets are built once per process (cached)."""
import functools
import random


class Fld:
    def __init__(self, name, p, es):
        self.name, self.p, self.es = name, p, es
        self.nl = es // 4                 # 32-bit limbs
        self.R = 1 << (8 * es)            # Montgomery radix
        self.Rinv = pow(self.R, -1, p)
        self.c = self.R - p               # R mod p (p > R/2)

    def __repr__(self):
        return self.name


F128 = Fld("Field128", (1 << 128) - 28 * (1 << 64) + 1, 16)
F64 = Fld("Field64", (1 << 64) - (1 << 32) + 1, 8)
FIELDS = {16: F128, 8: F64}
M32 = 0xFFFFFFFF

# op numbers of prio3gpu_test_field_op (include/prio3gpu_test.h)
OPS = {"add": 0, "sub": 1, "neg": 2, "dbl": 3, "mul": 4, "to_mont": 5, "from_mont": 6,
       "is_canonical": 7, "inv": 8, "inv_plain": 9, "pow": 10, "mul2": 11, "mul3": 12, "mul5": 13,
       "fma2_mul1": 14, "q1_fma1_mul1": 15, "addsub_AASS": 16, "addsub_ASAA": 17, "addsub_A": 18,
       "dot": 19, "limb_sums": 20}
# the streams of the multi-stream programs: M = product, F = two-term sum, Q = four-term sum,
# A = modular add, S = modular sub (operand order: janus_amd/csrc/field_test_kernels.h)
STREAMS = {"mul2": "MM", "mul3": "MMM", "mul5": "MMMMM", "fma2_mul1": "FFM", "q1_fma1_mul1": "QFM",
           "addsub_AASS": "AASS", "addsub_ASAA": "ASAA", "addsub_A": "A"}
TERMS = {"M": 1, "F": 2, "Q": 4}


def limbs(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def from_limbs(ls):
    return sum(l << (32 * i) for i, l in enumerate(ls))


# ---- edge elements --------------------------------------------------------------------------------
# Minimal failing tuples found by the GPU tests are appended here (none so far: no primitive has
# disagreed with the integers).
EXTRA_EDGES = {"Field128": [], "Field64": []}


@functools.lru_cache(None)
def edge_elements(F):
    p, R, nl = F.p, F.R, F.nl
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2,
         R % p, R % p + 1, R % p - 1, R * R % p, R * R * R % p, p - R % p]
    for k in range(nl + 1):
        e += [1 << (32 * k), (1 << (32 * k)) - 1, p - (1 << (32 * k))]
    for pat in range(1 << nl):  # every limb 0 or 0xFFFFFFFF, clipped below p
        e.append(min(from_limbs([M32 if pat >> i & 1 else 0 for i in range(nl)]), p - 1))
    e += EXTRA_EDGES[F.name]
    return tuple(sorted(set(x for x in e if 0 <= x < p)))


def rand_elements(F, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(F.p) for _ in range(n)]


def rand_pairs(F, n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(F.p), rng.randrange(F.p)) for _ in range(n)]


@functools.lru_cache(None)
def unary_elements(F):
    """E, 4096 random elements, 512 below 2^32, 512 within 2^32 of p."""
    rng = random.Random(0x0E1E + F.es)
    return (list(edge_elements(F)) + rand_elements(F, 4096, 11 + F.es)
            + [rng.randrange(1 << 32) for _ in range(512)]
            + [F.p - 1 - rng.randrange(1 << 32) for _ in range(512)])


@functools.lru_cache(None)
def edge_pairs(F):
    E = edge_elements(F)
    return [(a, b) for a in E for b in E]


# ---- add ------------------------------------------------------------------------------------------
def _split(F, s, rng, k):
    """k pairs a, b < p with a + b == s (the two extreme splits first)."""
    lo, hi = max(0, s - (F.p - 1)), min(F.p - 1, s)
    assert lo <= hi, s
    aa = [lo, hi] + [rng.randint(lo, hi) for _ in range(k - 2)]
    return [(a, s - a) for a in aa]


@functools.lru_cache(None)
def add_families(F):
    """name -> pairs a, b < p, by the value of a + b."""
    p, R, nl = F.p, F.R, F.nl
    rng = random.Random(0xADD + F.es)
    fam = {}
    for name, s in (("p-1", p - 1), ("p", p), ("p+1", p + 1), ("R-1", R - 1), ("R", R),
                    ("R+1", R + 1), ("2p-2", 2 * p - 2)):
        fam["sum=" + name] = _split(F, s, rng, 16)
    fam["sum in [p,R)"] = [pr for _ in range(256) for pr in _split(F, rng.randrange(p, R), rng, 3)[2:]]
    # p <= a + b < R with the split at its extremes too (a or b = p - 1)
    fam["sum in [p,R) extreme"] = [pr for _ in range(32)
                                   for pr in _split(F, rng.randrange(p, R), rng, 2)]
    for j in range(1, min(3, nl) + 1):
        mask = (1 << (32 * j)) - 1
        for nm, low in (("zero", 0), ("ones", mask)):
            prs = []
            for i in range(48):
                # sums below p, in [p, R) and at or above R (a third each)
                s = (rng.randrange(p), rng.randrange(p, R), rng.randrange(R, 2 * p - 1))[i % 3]
                s = (s & ~mask) | low
                s = min(max(s, low), ((2 * p - 2 - low) & ~mask) | low)
                prs += _split(F, s, rng, 3)[2:]
            fam["sum low %d limbs %s" % (j, nm)] = prs
    return fam


# ---- sub ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sub_families(F):
    p, nl = F.p, F.nl
    rng = random.Random(0x5AB + F.es)
    fam = {}
    eq = list(edge_elements(F)) + rand_elements(F, 64, 0x5AC)
    fam["a==b"] = [(a, a) for a in eq]
    ones = [rng.randrange(1, p) for _ in range(64)] + [1 << (32 * k) for k in range(nl)] + [p - 1, 1]
    fam["a-b=+1"] = [(a, a - 1) for a in ones]
    fam["a-b=-1"] = [(a - 1, a) for a in ones]
    for j in range(1, min(3, nl - 1) + 1):
        sh = 32 * j
        lt, gt = [], []
        for i in range(48):
            low = (rng.randrange(1 << sh), 0, (1 << sh) - 1)[i % 3]
            # high parts below p >> sh keep both values below p whatever the low limbs are
            h1 = rng.randrange((p >> sh) - 1)
            # h1 + 1: the difference sits in the lowest unequal limb alone
            h2 = h1 + 1 if i % 4 == 0 else rng.randrange(h1 + 1, p >> sh)
            a, b = (h1 << sh) | low, (h2 << sh) | low
            lt.append((a, b))
            gt.append((b, a))
        fam["equal low %d limbs a<b" % j] = lt
        fam["equal low %d limbs a>b" % j] = gt
    fam["b-a=p-1"] = [(0, p - 1)]
    fam["b-a=p-2"] = [(0, p - 2), (1, p - 1)]
    return fam


# ---- mul ------------------------------------------------------------------------------------------
def redc_presub(F, a, b):
    """Textbook REDC of a b before the final conditional subtraction: (a b + m p) / R with
    m = -a b / p mod R; in [0, 2p)."""
    t = a * b
    m = (-t * pow(F.p, -1, F.R)) % F.R
    assert (t + m * F.p) % F.R == 0
    return (t + m * F.p) // F.R


def _mul_pair_for(F, d, rng):
    """a, b < p with a b / R == d (mod p)."""
    a = rng.randrange(1, F.p)
    return a, d * F.R % F.p * pow(a, -1, F.p) % F.p


@functools.lru_cache(None)
def mul_families(F):
    """name -> pairs.  (i): results d < R - p, whose textbook-REDC value before the subtraction is
    d + p in [p, R), no carry out; (ii): d just above, d + p >= R with a tiny low part; (iii):
    operands that are multiples of 2^32 / 2^64 / 2^96, whose reduction words are zero (m = 0)."""
    p, R, nl, c = F.p, F.R, F.nl, F.c
    rng = random.Random(0x3A1 + F.es)
    fam = {}
    if F is F64:
        # d < 2^33 covers both: d + p < 2^64 (r >= P, t2 == 0) and d + p >= 2^64 (t2 != 0)
        ds = [1, c - 1, c, c + 1, (1 << 33) - 1] + [rng.randrange(1, 1 << 33) for _ in range(507)]
        prs = [_mul_pair_for(F, d, rng) for d in ds]
        fam["(i) small results"] = [pr for pr, d in zip(prs, ds) if d < c]
        fam["(ii) just above"] = [pr for pr, d in zip(prs, ds) if d >= c]
    else:
        ds = [1, 2, c - 1, c - 2] + [rng.randrange(1, c) for _ in range(252)]
        fam["(i) small results"] = [_mul_pair_for(F, d, rng) for d in ds]
        ds = [c, c + 1, c + (1 << 20) - 1] + [rng.randrange(c, c + (1 << 20)) for _ in range(253)]
        fam["(ii) just above"] = [_mul_pair_for(F, d, rng) for d in ds]
    z = []
    for k in range(1, nl):
        sh = 32 * k
        for i in range(24):
            a = rng.randrange(1, (p >> sh) + 1) << sh
            b = rng.randrange(1, (p >> sh) + 1) << sh if i % 2 else rng.randrange(p)
            if a < p and b < p:
                z += [(a, b), (b, a)]
        z += [(1 << sh, 1 << sh), (1 << sh, p - 1), (p - (1 << sh), 1 << sh)]
    fam["(iii) zero low words"] = z
    fam["max"] = [(p - 1, p - 1), (p - 1, p - 2), (p - 1, 1), (p - 1, R % p)]
    return fam


def _flat(fam):
    return [pr for prs in fam.values() for pr in prs]


@functools.lru_cache(None)
def binary_pairs(F, op):
    """E x E, 4096 random pairs and the op's constructed families."""
    fam = {"add": add_families, "sub": sub_families, "mul": mul_families}[op](F)
    return edge_pairs(F) + rand_pairs(F, 4096, 0xB1 + F.es) + _flat(fam)


# ---- multi-stream programs ------------------------------------------------------------------------
@functools.lru_cache(None)
def fused_edge_terms(F, nterms):
    """Operand tuples (a_0, b_0, ..., a_(n-1), b_(n-1)) for one stream computing
    (sum a_k b_k) / R: the mul families in each term position, maximum accumulation, sums of small
    results that straddle R - p, and sums that vanish mod p."""
    p, c = F.p, F.c
    rng = random.Random(0xF0 + nterms)
    mf = mul_families(F)
    fi, fii, fiii = mf["(i) small results"], mf["(ii) just above"], mf["(iii) zero low words"]
    if nterms == 1:
        return [tuple(pr) for pr in _flat(mf)] + [pr for pr in edge_pairs(F)[::7]]
    out = [(p - 1, p - 1) * nterms, (p - 1, 1) * nterms, (0, 0) * nterms]
    for i in range(48):
        out.append(sum((fi[(5 * i + 31 * t) % len(fi)] for t in range(nterms)), ()))  # all (i)
        out.append(sum((fiii[(3 * i + 17 * t) % len(fiii)] for t in range(nterms)), ()))
        for t in range(nterms):
            for edge, rest in ((fi, None), (fi, fiii), (fii, fiii), (fii, None), (fiii, None)):
                tup = ()
                for u in range(nterms):
                    if u == t:
                        tup += edge[(7 * i + t) % len(edge)]
                    elif rest is None:
                        tup += (0, rng.randrange(p)) if i % 2 else (rng.randrange(p), 0)
                    else:
                        tup += rest[(11 * i + 13 * u) % len(rest)]
                out.append(tup)
    # small results d_k whose sum is R - p - 1, R - p, R - p + 1: the fused sum's final select
    for total in (c - 1, c, c + 1, 2 * c, 2 * c + 1):
        for _ in range(8):
            cuts = sorted(rng.randrange(total + 1) for _ in range(nterms - 1))
            ds = [b - a for a, b in zip([0] + cuts, cuts + [total])]
            out.append(sum((_mul_pair_for(F, d, rng) for d in ds), ()))
    # a b + (p - a) b == 0 mod p (the remaining terms zero)
    for _ in range(8):
        a, b = rng.randrange(1, p), rng.randrange(1, p)
        out.append((a, b, p - a, b) + (0, 0) * (nterms - 2))
    E = edge_elements(F)
    for _ in range(64):
        out.append(tuple(rng.choice(E) for _ in range(2 * nterms)))
    return out


@functools.lru_cache(None)
def stream_pool(F, kind):
    """Edge operand tuples for one stream of a multi-stream program."""
    if kind == "A":
        return _flat(add_families(F)) + edge_pairs(F)[::5]
    if kind == "S":
        return _flat(sub_families(F)) + edge_pairs(F)[::5]
    return fused_edge_terms(F, TERMS[kind])


@functools.lru_cache(None)
def multi_stream_tuples(F, op):
    """Each stream position in turn carries an edge case while the others hold random operands,
    then every stream carries one at once (different ones, and the same one)."""
    streams = STREAMS[op]
    rng = random.Random(0x57 + OPS[op])
    pools = [stream_pool(F, k) for k in streams]
    width = [2 * TERMS.get(k, 1) for k in streams]
    out = []
    for s, pool in enumerate(pools):
        for e in pool:
            tup = ()
            for t in range(len(streams)):
                tup += tuple(e) if t == s else tuple(rng.randrange(F.p) for _ in range(width[t]))
            out.append(tup)
    for i in range(max(len(pl) for pl in pools)):
        out.append(sum((tuple(pl[(i * (2 * t + 1) + 7 * t) % len(pl)]) for t, pl in enumerate(pools)), ()))
        out.append(sum((tuple(pl[i % len(pl)]) for pl in pools), ()))
    for _ in range(1024):
        out.append(tuple(rng.randrange(F.p) for _ in range(sum(width))))
    return out


def stream_reference(F, kind, ops):
    p = F.p
    if kind == "A":
        return (ops[0] + ops[1]) % p
    if kind == "S":
        return (ops[0] - ops[1]) % p
    return sum(ops[2 * k] * ops[2 * k + 1] for k in range(TERMS[kind])) * F.Rinv % p


def multi_stream_reference(F, op, tup):
    out, i = [], 0
    for kind in STREAMS[op]:
        w = 2 * TERMS.get(kind, 1)
        out.append(stream_reference(F, kind, tup[i:i + w]))
        i += w
    assert i == len(tup)
    return tuple(out)


# ---- dot ------------------------------------------------------------------------------------------
DOT_PARAMS = (1, 2, 89, 1024)


@functools.lru_cache(None)
def dot_tuples(F, param):
    """name -> tuples of param pairs (a_k, x_k)."""
    p = F.p
    rng = random.Random(0xD07 + param)
    mf = mul_families(F)
    fam = {"max": [(p - 1, p - 1) * param], "zero": [(0, 0) * param]}
    fam["random"] = [tuple(rng.randrange(p) for _ in range(2 * param))
                     for _ in range(64 if param <= 89 else 6)]
    # family (i), then (ii), as the only non-zero product (the other terms have one zero factor)
    for name in ("(i) small results", "(ii) just above"):
        only = []
        for i, pos in enumerate(sorted({0, param // 2, param - 1}) * (8 if param <= 89 else 2)):
            tup = ()
            for k in range(param):
                if k == pos:
                    tup += mf[name][(i * 37 + pos) % len(mf[name])]
                else:
                    tup += (0, rng.randrange(p)) if k % 2 else (rng.randrange(p), 0)
            only.append(tup)
        fam[name.split()[0] + " alone"] = only
    if param in TERMS.values():  # the fused programs' term tuples are dot products too
        fam["fused terms"] = list(fused_edge_terms(F, param))
    return fam


def dot_reference(F, tup):
    return sum(tup[2 * k] * tup[2 * k + 1] for k in range(len(tup) // 2)) * F.Rinv % F.p


# ---- limb sums ------------------------------------------------------------------------------------
LIMB_SUM_KS = (0, 1, 2, 89, 1000, (1 << 32) - 1)
XS_MAX = M32 * M32  # a sum of < 2^32 32-bit words


@functools.lru_cache(None)
def limb_sum_inputs():
    """name -> lists of xs[0..3] (u64 column sums of 32-bit limbs)."""
    p = F128.p
    rng = random.Random(0x11B)
    fam = {"k copies of p-1": [tuple(k * l for l in limbs(p - 1, 4)) for k in LIMB_SUM_KS],
           "k copies of all-ones": [tuple(k * M32 for _ in range(4)) for k in LIMB_SUM_KS]}
    near = []
    for i in range(512):
        m = rng.randrange(1 << 31) if i % 4 else rng.randrange(4)
        v = m * p + rng.randrange(-(1 << 64) + 1, 1 << 64)
        if v < 0:
            v += p
        xs = [v & M32, (v >> 32) & M32, (v >> 64) & M32, v >> 96]
        for q in (2, 1, 0):  # move weight down: limbs above 32 bits, the value unchanged
            t = rng.randrange(min(xs[q + 1], (XS_MAX - xs[q]) >> 32) + 1)
            xs[q + 1] -= t
            xs[q] += t << 32
        assert all(0 <= x <= XS_MAX for x in xs) and limb_sum_value(xs) == v
        near.append(tuple(xs))
    fam["near a multiple of p"] = near
    fam["random"] = [tuple(rng.randrange(XS_MAX + 1) for _ in range(4)) for _ in range(1024)]
    fam["max"] = [(XS_MAX,) * 4]
    return fam


def limb_sum_value(xs):
    return sum(x << (32 * q) for q, x in enumerate(xs))


# ---- is_canonical ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def canonical_inputs(F):
    """Any 2^(8 ES) values: around p, each limb of p off by one, E, random."""
    p, R, nl = F.p, F.R, F.nl
    rng = random.Random(0xCA + F.es)
    v = [p - 1, p, p + 1, R - 1, R - 2, 0]
    pl = limbs(p, nl)
    for i in range(nl):
        for d in (1, -1):
            q = list(pl)
            q[i] = (q[i] + d) & M32
            v.append(from_limbs(q))
    v += list(edge_elements(F))
    v += [rng.randrange(R) for _ in range(2048)]
    v += [rng.randrange(p, R) for _ in range(1024)]
    v += [p - 1 - rng.randrange(1 << 32) for _ in range(256)]
    return v


# ---- pow ------------------------------------------------------------------------------------------
POW_PARAMS = (0, 1, 2, 3, 0x10001, 0x80000000, 0xFFFFFFFF)


@functools.lru_cache(None)
def pow_elements(F):
    return list(edge_elements(F)) + rand_elements(F, 512, 0x90 + F.es)


def pow_reference(F, x, e):
    """x = X R in, X^e R out."""
    return pow(x * F.Rinv % F.p, e, F.p) * F.R % F.p
