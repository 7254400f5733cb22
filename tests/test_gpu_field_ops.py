"""Device field arithmetic at edge operands: every Field128 / Field64 primitive the product kernels
call (Field128Ops / Field64Ops, the generated carry chains of modadd.h, the fused Montgomery
programs of mont_fma.h and mont3.h, wide_mac / wide_reduce, inv128::inverse, inv_mont, mont_pow,
f128_reduce_limb_sums) run alone on the GPU through prio3gpu_test_field_op, one lane per operand
tuple, against exact Python integers.  Every comparison is == on bytes.

The byte-exact transcript tests feed these primitives SHAKE128 output, i.e. uniform operands,
which reach the branches that matter (a sum or an unreduced Montgomery result in [p, 2^128)
without a carry out, a zero reduction word, equal low limbs in a subtraction, ...) with
probability 2^-32 .. 2^-59 per operation.  tests/field_edges.py constructs such operands;
tests/test_field_edges.py checks on the CPU that the constructed sets contain them.

Out of scope: the compile-time A/B variants (P3G_ADD_CPP=1, P3G_INV_EXP=1, FLPQ_MUL3=0) are chosen
per build and the library ships one build, so only the default variant runs here."""
import ctypes

import pytest

from tests import field_edges as FE
from tests.field_edges import F64, F128, OPS

pytestmark = pytest.mark.gpu

BOTH = [F128, F64]
MAX_TUPLES = 50_000


def ids(F):
    return F.name


def _enc(F, values):
    return b"".join(v.to_bytes(F.es, "little") for v in values)


def run_raw(es, op, param, data, n, out_len):
    from janus_amd._lib import check, lib
    out = ctypes.create_string_buffer(max(out_len, 1))
    check(lib().prio3gpu_test_field_op(es, OPS[op], param, data, n, out), "test_field_op " + op)
    return out.raw[:out_len]


# elements per operand tuple / per result, as include/prio3gpu_test.h states them
ARITY = {"add": 2, "sub": 2, "neg": 1, "dbl": 1, "mul": 2, "to_mont": 1, "from_mont": 1,
         "is_canonical": 1, "inv": 1, "inv_plain": 1, "pow": 1, "mul2": 4, "mul3": 6, "mul5": 10,
         "fma2_mul1": 10, "q1_fma1_mul1": 14, "addsub_AASS": 8, "addsub_ASAA": 8, "addsub_A": 2}
RESULTS = {"mul2": 2, "mul3": 3, "mul5": 5, "fma2_mul1": 3, "q1_fma1_mul1": 3, "addsub_AASS": 4,
           "addsub_ASAA": 4}


def run_op(F, op, tuples, nres=1, param=0):
    """One launch per <= MAX_TUPLES tuples; returns the results' bytes."""
    arity = 2 * param if op == "dot" else ARITY[op]
    assert nres == RESULTS.get(op, 1) and all(len(t) == arity for t in tuples)
    assert all(0 <= v < F.R for t in tuples for v in t)
    got = []
    for lo in range(0, len(tuples), MAX_TUPLES):
        part = tuples[lo:lo + MAX_TUPLES]
        data = _enc(F, (v for t in part for v in t))
        raw = run_raw(F.es, op, param, data, len(part), len(part) * nres * F.es)
        got.append(raw)
    return b"".join(got)


def check_op(F, op, tuples, want, nres=1, param=0):
    """want: one tuple of nres integers per operand tuple.  Byte-exact; on a mismatch, names the
    first differing tuple."""
    assert len(tuples) == len(want) and len(tuples) > 0
    got = run_op(F, op, tuples, nres, param)
    exp = _enc(F, (v for w in want for v in w))
    if got != exp:
        step = nres * F.es
        for i in range(len(tuples)):
            g, e = got[i * step:(i + 1) * step], exp[i * step:(i + 1) * step]
            if g != e:
                gv = [int.from_bytes(g[k:k + F.es], "little") for k in range(0, step, F.es)]
                raise AssertionError("%s %s tuple %d of %d: operands %s -> got %s, want %s" % (
                    F, op, i, len(tuples), [hex(v) for v in tuples[i]], [hex(v) for v in gv],
                    [hex(v) for v in want[i]]))
    assert got == exp


# ---- binary ops -----------------------------------------------------------------------------------
BIN_REF = {"add": lambda F, a, b: (a + b) % F.p, "sub": lambda F, a, b: (a - b) % F.p,
           "mul": lambda F, a, b: a * b * F.Rinv % F.p}


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_binary(F, op):
    # add also runs the sub families and the other way round: a wrong select shows on either
    pairs = FE.binary_pairs(F, op)
    if op in ("add", "sub"):
        pairs = pairs + FE._flat(FE.sub_families(F) if op == "add" else FE.add_families(F))
    check_op(F, op, pairs, [(BIN_REF[op](F, a, b),) for a, b in pairs])


@pytest.mark.parametrize("op", ["add", "mul"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_lane_geometry(F, n, op):
    """Full waves, a one-lane wave and ragged tails (tail lanes read tuple n - 1, store nothing);
    the bytes after the n results stay untouched."""
    pairs = (FE._flat(FE.add_families(F) if op == "add" else FE.mul_families(F))[:n // 2]
             + FE.rand_pairs(F, n, 1000 + n))[:n]
    assert len(pairs) == n
    want = _enc(F, (BIN_REF[op](F, a, b) for a, b in pairs))
    from janus_amd._lib import check, lib
    guard = b"\xa5" * 64
    out = ctypes.create_string_buffer(want + guard, len(want) + len(guard))
    ctypes.memset(out, 0x5A, len(want))
    check(lib().prio3gpu_test_field_op(F.es, OPS[op], 0, _enc(F, (v for t in pairs for v in t)),
                                       n, out), "test_field_op")
    assert out.raw == want + guard


# ---- unary ops ------------------------------------------------------------------------------------
UN_REF = {"neg": lambda F, a: -a % F.p, "dbl": lambda F, a: 2 * a % F.p,
          "to_mont": lambda F, a: a * F.R % F.p, "from_mont": lambda F, a: a * F.Rinv % F.p}


@pytest.mark.parametrize("op", ["neg", "dbl", "to_mont", "from_mont"])
@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_unary(F, op):
    xs = FE.unary_elements(F)
    check_op(F, op, [(x,) for x in xs], [(UN_REF[op](F, x),) for x in xs])


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_is_canonical(F):
    xs = FE.canonical_inputs(F)
    check_op(F, "is_canonical", [(x,) for x in xs], [(1 if x < F.p else 0,) for x in xs])


@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_inv(F):
    """inv_mont: Montgomery form in and out, 0 -> 0."""
    xs = FE.unary_elements(F)
    want = [(F.R * F.R * pow(x, -1, F.p) % F.p if x else 0,) for x in xs]
    check_op(F, "inv", [(x,) for x in xs], want)
    # independently of the reference: x * inv(x) is 1 (in Montgomery form: x y / R == R)
    got = run_op(F, "inv", [(x,) for x in xs])
    for i, x in enumerate(xs):
        y = int.from_bytes(got[i * F.es:(i + 1) * F.es], "little")
        assert y < F.p
        assert (x * y * F.Rinv) % F.p == (F.R % F.p if x else 0), hex(x)


def test_inv_plain():
    F = F128
    xs = FE.unary_elements(F)
    check_op(F, "inv_plain", [(x,) for x in xs], [(pow(x, -1, F.p) if x else 0,) for x in xs])


@pytest.mark.parametrize("param", FE.POW_PARAMS)
@pytest.mark.parametrize("F", BOTH, ids=ids)
def test_pow(F, param):
    xs = FE.pow_elements(F)
    check_op(F, "pow", [(x,) for x in xs], [(FE.pow_reference(F, x, param),) for x in xs],
             param=param)


# ---- multi-stream programs ------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mul2", "mul3", "mul5", "fma2_mul1", "q1_fma1_mul1", "addsub_AASS",
                                "addsub_ASAA", "addsub_A"])
def test_multi_stream(op):
    F = F128
    tuples = FE.multi_stream_tuples(F, op)
    want = [FE.multi_stream_reference(F, op, t) for t in tuples]
    check_op(F, op, tuples, want, nres=len(FE.STREAMS[op]))


# ---- dot ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", FE.DOT_PARAMS)
def test_dot(param):
    F = F128
    tuples = FE._flat(FE.dot_tuples(F, param))
    check_op(F, "dot", tuples, [(FE.dot_reference(F, t),) for t in tuples], param=param)


# ---- limb sums ------------------------------------------------------------------------------------
def test_limb_sums():
    F = F128
    xs = FE._flat(FE.limb_sum_inputs())
    data = b"".join(x.to_bytes(8, "little") for t in xs for x in t)
    got = run_raw(16, "limb_sums", 0, data, len(xs), 16 * len(xs))
    want = _enc(F, (FE.limb_sum_value(t) % F.p for t in xs))
    for i, t in enumerate(xs):
        assert got[16 * i:16 * i + 16] == want[16 * i:16 * i + 16], [hex(x) for x in t]
    assert got == want


# ---- arguments ------------------------------------------------------------------------------------
def test_arguments():
    from janus_amd._lib import lib
    L = lib()
    E_ARG = -1
    buf, out = bytes(64), ctypes.create_string_buffer(64)
    assert L.prio3gpu_test_field_op(16, OPS["add"], 0, None, 0, None) == 0      # n == 0: nothing
    assert L.prio3gpu_test_field_op(8, OPS["mul"], 0, buf, 0, out) == 0
    assert L.prio3gpu_test_field_op(16, 21, 0, buf, 1, out) == E_ARG            # unknown op
    assert L.prio3gpu_test_field_op(16, -1, 0, buf, 1, out) == E_ARG
    assert L.prio3gpu_test_field_op(16, 21, 0, buf, 0, out) == E_ARG
    assert L.prio3gpu_test_field_op(4, OPS["add"], 0, buf, 1, out) == E_ARG     # bad size
    assert L.prio3gpu_test_field_op(32, OPS["add"], 0, buf, 1, out) == E_ARG
    for op in ("inv_plain", "mul2", "mul3", "mul5", "fma2_mul1", "q1_fma1_mul1", "addsub_AASS",
               "addsub_ASAA", "addsub_A", "dot", "limb_sums"):                   # Field128 only
        assert L.prio3gpu_test_field_op(8, OPS[op], 1, buf, 1, out) == E_ARG, op
    assert L.prio3gpu_test_field_op(16, OPS["add"], 0, None, 1, out) == E_ARG   # null pointers
    assert L.prio3gpu_test_field_op(16, OPS["add"], 0, buf, 1, None) == E_ARG
    assert L.prio3gpu_test_field_op(16, OPS["dot"], 0, buf, 1, out) == E_ARG    # no terms
    assert out.raw == bytes(64)
