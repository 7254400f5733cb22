"""The fold at the end of k_accum_spec (janus_amd/csrc/accum_fold.h: two 64-bit word sums with
their carry counts -> one canonical Field128 element) built for the host with g++ and compared with
Python integers, (alo + ((ahi + blo) << 64) + (bhi << 128)) % p.  tests/native/accum_fold_host.cpp
is the driver (a text protocol on stdin / stdout); the function it calls is the one the kernel
calls.  Real reports never reach the fold's three data-dependent paths (uniform rows carry out of
ahi + blo with probability about 2^-59 per column), so the tuples here are built to, and the
tests assert that every path was taken (tests/accum_edges.py states the events)."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from tests.accum_edges import (EVENTS, FAMILIES128, M64, P128, column, fold_events,
                               fold_reference, word_sums)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "accum_fold_host.cpp")


@pytest.fixture(scope="module")
def fold_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("accum_fold") / "accum_fold_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(out), SRC], check=True)
    return str(out)


def run(binary, tuples):
    inp = "".join("%x %x %x %x\n" % t for t in tuples).encode()
    out = subprocess.run([binary], input=inp, capture_output=True, check=True).stdout.split()
    assert len(out) == len(tuples)
    return [int(x, 16) for x in out]


def check(binary, tuples):
    """Every tuple's fold == the Python integers; -> how often each event occurred."""
    seen = [0] * len(EVENTS)
    for t, got in zip(tuples, run(binary, tuples)):
        assert got == fold_reference(*t), [hex(x) for x in t]
        for i, hit in enumerate(fold_events(*t)):
            seen[i] += hit
    return dict(zip(EVENTS, seen))


@functools.lru_cache(None)
def grid_tuples():
    words = [0, 1, 27, 28, 1 << 63, M64 - 28, M64 - 27, M64 - 26, M64 - 1, M64]
    counts = [0, 1, 2, 27, 28, 63, 64, 2047, 1 << 20, (1 << 32) - 1]
    return [(alo, ahi, blo, bhi) for alo in words for ahi in counts for blo in words
            for bhi in counts]


ROWS = (1, 2, 4, 44, 64, 300, 2048, 65536)


@functools.lru_cache(None)
def structured_tuples():
    """Column sums of m canonical rows of every family (both phases of the periodic ones, and the
    "rest 0" values in the first rows)."""
    rng = np.random.default_rng(64)
    out = []
    for _name, spec in FAMILIES128:
        for m in ROWS:
            for phase in range(len(spec[1]) if spec[0] == "period" else 1):
                rows = column(spec, m, P128, rng, phase=phase)
                assert len(rows) == m and all(0 <= x < P128 for x in rows)
                t = word_sums(rows)
                assert fold_reference(*t) == sum(rows) % P128
                out.append(t)
    return out


def random_tuples(k=100000):
    rng = random.Random(0xF01D)
    out = []
    for i in range(k):
        # carry counts as the kernel has them (a few thousand rows) and up to the 2^32 bound
        hb = (12, 12, 32)[i % 3]
        out.append((rng.getrandbits(64), rng.getrandbits(hb), rng.getrandbits(64),
                    rng.getrandbits(hb)))
    return out


def test_grid(fold_bin):
    g = grid_tuples()
    assert len(g) == 10 ** 4
    check(fold_bin, g)


def test_structured_column_sums(fold_bin):
    check(fold_bin, structured_tuples())


def test_random_tuples(fold_bin):
    t = random_tuples()
    assert len(t) == 10 ** 5
    check(fold_bin, t)


def test_domain_beyond_the_kernels_counts(fold_bin):
    """accum_fold.h states its domain as any alo, ahi, blo and bhi < 2^59: the edges of it."""
    top = (1 << 59) - 1
    words = [0, 1, M64 - 28, M64 - 1, M64]
    check(fold_bin, [(alo, ahi, blo, bhi) for alo in words for ahi in words for blo in words
                     for bhi in (top, top - 1, 1 << 58, 1 << 32, (1 << 32) + 1)])


def test_every_path_of_the_fold_is_taken(fold_bin):
    """Each event of tests/accum_edges.py::EVENTS occurs for at least one tuple that ran, and the
    constructions that are meant to reach one do."""
    seen = check(fold_bin, grid_tuples() + structured_tuples() + random_tuples(2000))
    for name in EVENTS:
        assert seen[name] > 0, f"no tuple took: {name}"
    fam = dict(FAMILIES128)
    # rows alternating p-1 / 2^64-1 over 64 or more rows pass 2^128
    for m in (64, 300, 2048):
        assert fold_events(*word_sums(column(fam["alt p-1 / ones"], m, P128)))[1], m
    # the period-4 rows carry out of ahi + blo
    assert any(fold_events(*word_sums(column(fam["period4 carry"], m, P128)))[0] for m in ROWS)
    # one p-1, one 1 and the rest 0: exactly p before the reduction, 0 after it
    ev = fold_events(*word_sums(column(fam["exactly p"], 64, P128)))
    assert ev[2] and ev[3]
    assert fold_events(*word_sums(column(fam["single p-1"], 64, P128)))[4]


def test_sanitizer_build_over_the_grid(tmp_path):
    """The same stand-alone driver under AddressSanitizer and UBSan (shifts and the unsigned
    __int128 steps of the fold), over the grid and the structured tuples."""
    out = tmp_path / "accum_fold_host_san"
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", str(out), SRC], capture_output=True)
    if cc.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: "
                    + cc.stderr.decode(errors="replace")[-200:])
    check(str(out), grid_tuples() + structured_tuples())
