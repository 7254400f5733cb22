"""Edge-valued columns of measurement-share elements for the accumulation tests
(tests/test_accum_fold.py on the CPU, tests/test_gpu_accum_edges.py on the GPU), and the events of
the speculative fold (janus_amd/csrc/accum_fold.h) stated on the mathematical quantities alone.

A column is what one measurement element holds over the n rows of a batch.  Real reports' share
elements are uniform; these are the operands at which modular accumulation can go wrong: sums that
sit at p - 1, p and 0, word sums that carry, rows of all-ones words."""
P128 = (1 << 128) - 28 * (1 << 64) + 1
P64 = (1 << 64) - (1 << 32) + 1
M64 = (1 << 64) - 1


# name ->("all", v) | ("period", [v...]) | ("rest0", [v...]) | ("random",); `w` is the half-width
# of the field's elements in bits (64 for Field128, 32 for Field64): the word that carries.
def families(p, w):
    ones = (1 << w) - 1
    return [
        ("all p-1", ("all", p - 1)),
        ("all p-2", ("all", p - 2)),
        ("all ones word", ("all", ones)),
        ("all top bit", ("all", 1 << (2 * w - 1))),
        ("alt p-1 / ones", ("period", [p - 1, ones])),
        ("alt p-2 / ones", ("period", [p - 2, ones])),
        ("period4 carry", ("period", [p - 1, p - 1, (55 << w) + ones, ones])),
        ("period4 mixed", ("period", [p - 2, ones, (27 << w) + ones, 1])),
        ("all zero", ("all", 0)),
        ("single p-1", ("rest0", [p - 1])),
        ("exactly p", ("rest0", [p - 1, 1])),
        ("p + 1", ("rest0", [p - 1, 2])),
        ("halves", ("rest0", [(p - 1) // 2, (p + 1) // 2])),
        ("uniform", ("random",)),
    ]


FAMILIES128 = families(P128, 64)
FAMILIES64 = families(P64, 32)


def column(spec, n, p, rng=None, at=(0, 1), phase=0):
    """The n values of one column.  `at`: the rows a "rest 0" family puts its non-zero values in;
    `phase` shifts a periodic family (row r holds entry (r + phase) mod period)."""
    kind = spec[0]
    if kind == "all":
        return [spec[1]] * n
    if kind == "period":
        v = spec[1]
        return [v[(r + phase) % len(v)] for r in range(n)]
    if kind == "rest0":
        out = [0] * n
        for r, x in zip(at, spec[1]):
            if r < n:
                out[r] = x
        return out
    assert kind == "random"
    nb = 16 if p > M64 else 8
    raw = rng.bytes(nb * n)
    return [int.from_bytes(raw[nb * r:nb * r + nb], "little") % p for r in range(n)]


def word_sums(values):
    """(alo, ahi, blo, bhi) of Field128 rows: the 128-bit sums of their low and of their high
    64-bit words, as k_accum_spec holds them before its fold."""
    a = sum(x & M64 for x in values)
    b = sum(x >> 64 for x in values)
    return a & M64, a >> 64, b & M64, b >> 64


def fold_reference(alo, ahi, blo, bhi):
    return (alo + ((ahi + blo) << 64) + (bhi << 128)) % P128


EVENTS = ("carry out of ahi + blo", "v + 28 x2 2^64 passes 2^128", "pre-reduction value >= p",
          "result 0", "result p-1")


def fold_events(alo, ahi, blo, bhi):
    """Which of EVENTS a tuple takes, from the quantities the fold is defined by (not its code):
    x1 = ahi + blo, x2 = bhi + carry, v = alo + 2^64 (x1 mod 2^64); the value before the last
    reduction is v + x2 (28 2^64 - 1), less 2^128 - (28 2^64 - 1) = p if v + 28 x2 2^64 passed
    2^128 (2^128 = 28 2^64 - 1 mod p)."""
    x1 = ahi + blo
    carry = x1 >> 64
    x2 = bhi + carry
    v = alo + ((x1 & M64) << 64)
    passes = v + ((28 * x2) << 64) >= 1 << 128
    pre = v + x2 * ((28 << 64) - 1) - (P128 if passes else 0)
    res = fold_reference(alo, ahi, blo, bhi)
    return (carry == 1, passes, pre >= P128, res == 0, res == P128 - 1)
