"""Helper aggregate-init over MANY SMALL aggregation jobs of SEVERAL tasks on one GPU: what a Janus
helper sees (max_aggregation_job_size defaults to 500; the sample configs set 100), timed two ways
over the same requests:

  (a) one HelperAggregateInit(hpke="host") per task on a context created with that task's verify
      key, the task's jobs through handle_jobs: one engine call per job;
  (b) HelperJobBatcher.handle_jobs over all jobs, interleaved across the tasks: the jobs coalesced
      into GPU batches of at most --max-reports reports, one keyed engine call per batch
      (prio3gpu_state_set_verify_keys).

(a) and (b) alternate within each repetition.  Responses and per-task aggregates, counts,
checksums and intervals are compared byte for byte.  Inputs as in bench_helper_e2e.py: seeded
random nonces, client randomness and measurements, shares from the GPU client shard, leader prep
shares from the GPU leader prepare_init under each task's key, helper shares sealed on the GPU to
each task's own X25519 / HKDF-SHA256 / AES-128-GCM key -- all made before timing.  One JSON line,
with the HIP-event time of the accumulation kernels per engine call of both ways (one extra,
untimed pass with prio3gpu_prof_enable).

  python tools/bench_helper_multijob.py --config sumvec --tasks 8 --job-size 100 --jobs 656
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import CONFIGS  # noqa: E402
from janus_amd import codec as C  # noqa: E402
from janus_amd import hpke as H  # noqa: E402
from janus_amd._lib import lib  # noqa: E402
from janus_amd.helper import HelperAggregateInit  # noqa: E402
from janus_amd.multijob import HelperJobBatcher, HelperTask, pack_jobs  # noqa: E402
from janus_amd.prio3 import Prio3Gpu  # noqa: E402

ACCUM = ("k_accum_partial", "k_accum_spec", "k_accum_merge")


def make_task_jobs(v, task_id, tk, n_jobs, S, config, bits, length, rng, dev):
    """`n_jobs` requests of S reports for one task (context `v` holds its verify key)."""
    s = v.sizes
    M = n_jobs * S
    ls, hs = v.new_state(0, M), v.new_state(1, M)
    nonces = rng.integers(0, 256, (M, 16), dtype=np.uint8)
    d_nonces = torch.from_numpy(nonces).to(dev)
    if config == "sumvec":
        meas = rng.integers(0, 1 << bits, (M, length), dtype=np.int64)
    else:   # Sum: a value below 2^bits; Histogram: a bucket index; Count: 0 / 1
        hi = {"sum": 1 << bits, "histogram": length, "count": 2}[config]
        meas = rng.integers(0, hi, (M, 1), dtype=np.int64)
    d_meas = torch.from_numpy(meas).to(dev)
    d_rand = torch.from_numpy(rng.integers(0, 256, (M, v.random_size()), dtype=np.uint8)).to(dev)
    d_pub = torch.empty((M, s.public_share), dtype=torch.uint8, device=dev) \
        if s.public_share else None
    d_lin = torch.empty((M, s.leader_input_share), dtype=torch.uint8, device=dev)
    d_hin = torch.empty((M, s.helper_input_share), dtype=torch.uint8, device=dev)
    v.shard(hs, d_nonces, d_meas, d_rand, out=(d_pub, d_lin, d_hin))
    lp, lst = v.prepare_init(ls, d_nonces, d_pub, d_lin)
    assert (lst == 0).all()
    pub = d_pub.cpu().numpy() if s.public_share else np.zeros((M, 0), np.uint8)
    times = [1_700_000_000 + i % 3600 for i in range(M)]
    sk_es = np.frombuffer(os.urandom(32 * M), np.uint8).reshape(M, 32).copy()
    encs, pays, sst = H.seal_input_shares_gpu(
        v, task_id, tk.config, H.ROLE_HELPER, d_nonces,
        torch.from_numpy(np.array(times, np.int64)).to(dev), d_pub, d_hin,
        torch.from_numpy(sk_es).to(dev))
    assert not sst[:M].any()
    reqs = []
    for j in range(n_jobs):
        r = slice(j * S, (j + 1) * S)
        cts = [(tk.config.id, encs[i].tobytes(), pays[i].tobytes()) for i in range(r.start, r.stop)]
        reqs.append(C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", nonces[r], times[r], pub[r],
                                          cts, lp[r]))
    ls.close()
    hs.close()
    return reqs


def prof_ms(ctx, run):
    """HIP-event milliseconds and launches by kernel name over one call of `run`."""
    L = lib()
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    L.prio3gpu_prof_enable(ctx, 1)
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        run()
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    return {L.prio3gpu_prof_kernel_name(i).decode(): (ms[i], int(launches[i]))
            for i in range(k) if launches[i]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("sumvec", "sum", "histogram", "count"), default="sumvec")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--job-size", type=int, default=100)
    ap.add_argument("--jobs", type=int, default=656, help="jobs in all, dealt to the tasks in turn")
    ap.add_argument("--max-reports", type=int, default=65536)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    T, S, J = args.tasks, args.job_size, args.jobs
    dev = torch.device("cuda", 0)
    kind, bits, length, chunk, label = CONFIGS[args.config]
    rng = np.random.default_rng(2025)
    t0 = time.time()
    tasks, vs, per_task = [], [], []
    for k in range(T):
        vk = hashlib.shake_128(b"verify-key multijob %d" % k).digest(16)
        v = Prio3Gpu(kind, vk, bits=bits, length=length, chunk_length=chunk, device=0)
        tk = H.generate_hpke_config_and_private_key(1 + k)
        task = HelperTask(hashlib.sha256(b"multijob task %d" % k).digest(), vk, [tk])
        n_jobs = len(range(k, J, T))
        per_task.append(make_task_jobs(v, task.task_id, tk, n_jobs, S, args.config, bits, length,
                                       rng, dev) if n_jobs else [])
        tasks.append(task)
        vs.append(v)
        print(f"generated task {k + 1}/{T}", file=sys.stderr, flush=True)
    jobs = [(j % T, per_task[j % T][j // T]) for j in range(J)]
    gen_s = time.time() - t0
    # (a) one driver per task; (b) the batcher on a context whose own key is no task's
    drvs = [HelperAggregateInit(vs[k], tasks[k].task_id, tasks[k].task_keys,
                                hpke_threads=args.threads, hpke="host") for k in range(T)]
    vb = Prio3Gpu(kind, bytes(16), bits=bits, length=length, chunk_length=chunk, device=0)
    bat = HelperJobBatcher(vb, tasks, hpke_threads=args.threads, max_reports=args.max_reports)

    def run_a(aggs):
        return [drvs[k].handle_jobs(per_task[k], aggs[k]) for k in range(T)]

    def run_b(agg):
        return bat.handle_jobs(jobs, agg)

    run_a([v.new_aggregate(1) for v in vs])  # warm: states, pinned pools
    run_b(bat.new_aggregate())
    aggs_a, agg_b = [v.new_aggregate(1) for v in vs], bat.new_aggregate()
    torch.cuda.synchronize()
    sec = {"a": [], "b": []}
    for _ in range(args.reps):   # alternating: both ways see the same machine state over time
        t = time.perf_counter()
        ra = run_a(aggs_a)
        torch.cuda.synchronize()
        sec["a"].append(time.perf_counter() - t)
        t = time.perf_counter()
        rb = run_b(agg_b)
        torch.cuda.synchronize()
        sec["b"].append(time.perf_counter() - t)
    for j, (k, _) in enumerate(jobs):
        assert isinstance(rb[j], bytes) and rb[j] == ra[k][j // T], f"job {j}: response differs"
    for k in range(T):
        assert agg_b.read(k) == aggs_a[k].read(0), f"task {k}: aggregate differs"
        assert agg_b.read(k)[1] == len(per_task[k]) * S * args.reps, k
        assert agg_b.read_reports(k) == aggs_a[k].read_reports(0), f"task {k}: checksum differs"
    # the accumulation kernels per engine call, one untimed pass each way
    n_batches = len(pack_jobs([S] * J, args.max_reports))
    pa = {}
    for k in range(T):
        for name, (ms, nl) in prof_ms(vs[k]._ctx, lambda: drvs[k].handle_jobs(
                per_task[k], vs[k].new_aggregate(1))).items():
            pa[name] = (pa.get(name, (0.0, 0))[0] + ms, pa.get(name, (0.0, 0))[1] + nl)
    pb = prof_ms(vb._ctx, lambda: run_b(bat.new_aggregate()))

    # which stage bounds each way: the host stages and the GPU stage one after the other
    stage_a, stage_b = {"open": 0.0, "prepare": 0.0}, {}
    for k in range(T):
        agg = vs[k].new_aggregate(1)
        for r in per_task[k]:
            t = time.perf_counter()
            o = drvs[k].open(r)
            stage_a["open"] += time.perf_counter() - t
            t = time.perf_counter()
            drvs[k].prepare(o, agg)
            stage_a["prepare"] += time.perf_counter() - t
    t = time.perf_counter()
    reqs = [bat._decode(k, r) for k, r in jobs]
    stage_b["decode_check"] = time.perf_counter() - t
    t = time.perf_counter()
    opened = [bat._open_batch(b, [k for k, _ in jobs], reqs)
              for b in pack_jobs([r.n for r in reqs], args.max_reports)]
    stage_b["open"] = time.perf_counter() - t
    agg = bat.new_aggregate()
    t = time.perf_counter()
    for o in opened:
        bat._prepare(o, agg)
    stage_b["prepare"] = time.perf_counter() - t
    stage_a = {k: round(x * 1e3, 1) for k, x in stage_a.items()}
    stage_b = {k: round(x * 1e3, 1) for k, x in stage_b.items()}

    def per_call(p, calls):
        return {"accum_ms_per_call": round(sum(p.get(n, (0.0, 0))[0] for n in ACCUM) / calls, 4),
                "accum_launches": {n: p[n][1] for n in ACCUM if n in p},
                "all_kernels_ms_per_call": round(sum(ms for ms, _ in p.values()) / calls, 4),
                "engine_calls": calls}

    def rates(xs):
        r = sorted(J * S / x for x in xs)
        return {"median_reports_per_s": round(statistics.median(r)), "min_reports_per_s": round(r[0]),
                "max_reports_per_s": round(r[-1])}

    ma, mb = rates(sec["a"]), rates(sec["b"])
    print(json.dumps({
        "what": "helper aggregate-init, many small jobs of several tasks: (a) one "
                "HelperAggregateInit per task, one engine call per job; (b) HelperJobBatcher, "
                "one keyed engine call per batch; request bytes in, response bytes out, HPKE "
                "open on host threads",
        "workload": label, "tasks": T, "job_size": S, "jobs": J, "reports": J * S,
        "max_reports": args.max_reports, "batches": n_batches, "reps": args.reps,
        "hpke_threads": args.threads, "unit": "reports/s",
        "a_per_job": {**ma, **per_call(pa, J), "stage_ms_unpipelined": stage_a},
        "b_batched": {**mb, **per_call(pb, n_batches), "stage_ms_unpipelined": stage_b},
        "b_over_a_median": round(mb["median_reports_per_s"] / ma["median_reports_per_s"], 2),
        "gen_seconds": round(gen_s, 1)}), flush=True)
    for d in drvs:
        d.close()
    bat.close()


if __name__ == "__main__":
    main()
