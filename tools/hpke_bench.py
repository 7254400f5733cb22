"""Batched helper HPKE open rate: host threads vs the GPU open, same request builder.

  python tools/hpke_bench.py host --threads 1,8,16 [--scalar]   host threads ('--scalar': the
                                                    scalar X25519 ladder for every report,
                                                    prio3gpu_test_hpke_set_ifma(0))
  python tools/hpke_bench.py gpu --n 4096,65536,1048576 --threads 16
                                                    prio3gpu_hpke_open_report_shares_gpu, with
                                                    the per-kernel HIP-event times of one call
  python tools/hpke_bench.py both --n 65536 --threads 16    both on the same request
  python tools/hpke_bench.py both --n 65536 --suite 0x20/3/3,0x20/2/2
                                                    the task key's suite(s), KEM/KDF/AEAD; a suite
                                                    other than 0x20/1/1 turns the context option
                                                    "hpke_gpu_suites" on for the GPU mode
  python tools/hpke_bench.py both --n 4096,65536 --reps 9 --suite 0x10/1/1
                                                    a P-256 key (KEM 0x10): the GPU mode turns
                                                    "hpke_gpu_p256" on (and "hpke_gpu_suites" for
                                                    a KDF / AEAD other than 1/1)
  python tools/hpke_bench.py 1,8,16 [scalar]        the former spelling of `host`

Each figure is the median of --reps timed calls after one warm-up call, with the min..max spread;
the GPU mode's kernel_ms are the HIP-event times of --reps further calls, median [min, max] per
kernel.  One JSON line per (suite, mode, n, threads)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from janus_amd import codec as C, hpke as H  # noqa: E402
from janus_amd._lib import lib  # noqa: E402
from test_hpke import _request  # noqa: E402


def build_request(n, tk, task_id):
    rng = np.random.default_rng(1)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    public = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    payloads = [bytes(48)] * n
    return C.decode_agg_init_req(_request(task_id, nonces, [0] * n, public, payloads, [tk] * n))


def timed(fn, reps):
    fn()  # warm-up: scratch growth, first launches
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        st = fn()
        ts.append(time.perf_counter() - t)
        assert (st == 0).all()
    return ts


def kernel_ms(ctx, fn, reps):
    """HIP-event time per kernel (prio3gpu_prof_*) of `reps` calls: {name: [median, min, max]}."""
    import ctypes
    L = lib()
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    L.prio3gpu_prof_enable(ctx, 1)
    L.prio3gpu_prof_read(ctx, ms, launches, 64)
    per = {}
    for _ in range(reps):
        fn()
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
        for i in range(k):
            if launches[i]:
                per.setdefault(L.prio3gpu_prof_kernel_name(i).decode(), []).append(ms[i])
    L.prio3gpu_prof_enable(ctx, 0)
    return {name: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
            for name, v in per.items()}


def parse_suite(text):
    kem, kdf, aead = (int(x, 0) for x in text.split("/"))
    return kem, kdf, aead


def main():
    argv = sys.argv[1:]
    if argv and argv[0][0].isdigit():  # former spelling: THREADS [scalar]
        argv = ["host", "--threads", argv[0]] + (["--scalar"] if "scalar" in argv[1:] else [])
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("host", "gpu", "both"))
    ap.add_argument("--threads", default="16")
    ap.add_argument("--n", default="4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scalar", action="store_true")
    ap.add_argument("--suite", default="0x20/1/1",
                    help="KEM/KDF/AEAD of the task key; a comma-separated list runs each in turn")
    args = ap.parse_args(argv)
    if args.scalar:
        lib().prio3gpu_test_hpke_set_ifma(0)
    task_id = bytes(32)
    gpu = None
    if args.mode != "host":
        from janus_amd.prio3 import Prio3Gpu
        gpu = Prio3Gpu.new_count(bytes(16))
    wide_on = p256_on = False
    for suite in [parse_suite(x) for x in args.suite.split(",")]:
        tk = H.generate_hpke_config_and_private_key(1, *suite)
        wide = suite[1:] != (1, 1)
        if gpu is not None and wide != wide_on:  # the default suite needs no option
            gpu.set_option("hpke_gpu_suites", int(wide))
            wide_on = wide
        p256 = suite[0] == H.KEM_P256_HKDF_SHA256
        if gpu is not None and p256 != p256_on:
            gpu.set_option("hpke_gpu_p256", int(p256))
            p256_on = p256
        for n in [int(x) for x in args.n.split(",")]:
            req = build_request(n, tk, task_id)
            for th in [int(x) for x in args.threads.split(",")]:
                for mode in (("host", "gpu") if args.mode == "both" else (args.mode,)):
                    g = gpu if mode == "gpu" else None

                    def call():
                        return H.open_report_shares(task_id, req, [tk], [], None, th, gpu=g)[2]

                    ts = timed(call, args.reps)
                    med = statistics.median(ts)
                    out = {"suite": "0x%04x/%d/%d" % suite, "mode": mode, "n": n, "threads": th,
                           "reps": args.reps, "opens_per_s": round(n / med),
                           "ms_per_call": round(med * 1e3, 3), "ms_min": round(min(ts) * 1e3, 3),
                           "ms_max": round(max(ts) * 1e3, 3)}
                    if mode == "host":
                        out["us_per_open_per_thread"] = round(med / n * th * 1e6, 2)
                    else:
                        out["kernel_ms"] = kernel_ms(gpu._ctx, call, args.reps)
                    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
