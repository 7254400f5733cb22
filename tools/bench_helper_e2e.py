"""End-to-end helper aggregate-init throughput on one GPU (SURVEY §8(a) A1 with its host stages):
AggregationJobInitializeReq bytes in -> batched decode -> HPKE open of every helper input share on
host threads -> GPU prepare_init + decide + prepare_next + accumulate -> AggregationJobResp bytes
out, pipelined over jobs by HelperAggregateInit.handle_jobs (decode + HPKE of job k+1 on the host
while the GPU prepares job k).  --config picks the VDAF (bench.py's CONFIGS; default
Prio3SumVec(8, 1000, 89)).  Inputs: seeded random nonces, client
randomness and measurements, shares from the GPU client shard, leader prep shares from the GPU leader prepare_init, helper shares sealed to
one X25519/HKDF-SHA256/AES-128-GCM key (on the GPU, hpke.seal_input_shares_gpu; a P-256 --suite
seals on the host) -- all made before timing.

--hpke takes one mode or a comma-separated list (host, gpu, fused).  With a list the same
requests run through every mode in turn within each repetition (mode A, B, C, A, B, C, ...), so
the modes are compared in one session on one set of inputs; one JSON line per mode, each with the
median and min..max of its repetitions.  "fused" is HelperAggregateInit(hpke="fused"): gather,
open, decode and preparation in one engine call per job (prio3gpu_helper_init_request); its line
also carries the HIP-event time of every stage of one job.

  python tools/bench_helper_e2e.py --jobs 8 --job-size 16384 --threads 16 [--hpke gpu]
  python tools/bench_helper_e2e.py --config count --jobs 4 --job-size 65536 --reps 5 \
      --hpke host,gpu,fused
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
from janus_amd.prio3 import Prio3Gpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--job-size", type=int, default=16384)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--hpke", default="host",
                    help="where the helper input shares are opened (HelperAggregateInit hpke=): "
                         "host, gpu, fused, or a comma-separated list run alternately")
    ap.add_argument("--config", choices=("sumvec", "sum", "histogram", "count"), default="sumvec")
    ap.add_argument("--suite", default="0x20/1/1",
                    help="KEM/KDF/AEAD of the task key; a suite other than 0x20/1/1 runs the gpu "
                         "and fused modes with hpke_gpu_suites=1")
    args = ap.parse_args()
    suite = tuple(int(x, 0) for x in args.suite.split("/"))
    modes = args.hpke.split(",")
    if not modes or any(m not in ("host", "gpu", "fused") for m in modes):
        ap.error("--hpke: host, gpu, fused or a comma-separated list of them")
    dev = torch.device("cuda", 0)
    kind, bits, length, chunk, label = CONFIGS[args.config]
    cfg_id = b"bench-" + args.config.encode()
    vk = hashlib.shake_128(b"verify-key" + cfg_id).digest(16)
    v = Prio3Gpu(kind, vk, bits=bits, length=length, chunk_length=chunk, device=0)
    s = v.sizes
    M, J = args.job_size, args.jobs
    rng = np.random.default_rng(2024)
    tk = H.generate_hpke_config_and_private_key(7, *suite)
    info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_HELPER)
    task_id = hashlib.sha256(b"e2e task").digest()
    t0 = time.time()
    reqs, job_nonces = [], []
    ls = v.new_state(0, M)
    hs0 = v.new_state(1, M)
    for j in range(J):
        nonces = rng.integers(0, 256, (M, 16), dtype=np.uint8)
        d_nonces = torch.from_numpy(nonces).to(dev)
        if args.config == "sumvec":
            meas = rng.integers(0, 1 << bits, (M, length), dtype=np.int64)
        else:   # Sum: a value below 2^bits; Histogram: a bucket index; Count: 0 / 1
            hi = {"sum": 1 << bits, "histogram": length, "count": 2}[args.config]
            meas = rng.integers(0, hi, (M, 1), dtype=np.int64)
        d_meas = torch.from_numpy(meas).to(dev)
        d_rand = torch.from_numpy(rng.integers(0, 256, (M, v.random_size()), dtype=np.uint8)).to(dev)
        d_pub = torch.empty((M, s.public_share), dtype=torch.uint8, device=dev) \
            if s.public_share else None
        d_lin = torch.empty((M, s.leader_input_share), dtype=torch.uint8, device=dev)
        d_hin = torch.empty((M, s.helper_input_share), dtype=torch.uint8, device=dev)
        v.shard(hs0, d_nonces, d_meas, d_rand, out=(d_pub, d_lin, d_hin))
        lp, lst = v.prepare_init(ls, d_nonces, d_pub, d_lin)
        assert (lst == 0).all()
        pub = d_pub.cpu().numpy() if s.public_share else np.zeros((M, 0), np.uint8)
        hin = d_hin.cpu().numpy()
        job_nonces.append(nonces)
        times = [1_700_000_000 + (j * M + i) % 3600 for i in range(M)]
        if tk.config.kem_id == H.KEM_X25519_HKDF_SHA256:    # sealed on the GPU, from device rows
            sk_es = np.frombuffer(os.urandom(32 * M), np.uint8).reshape(M, 32).copy()
            encs, pays, sst = H.seal_input_shares_gpu(
                v, task_id, tk.config, H.ROLE_HELPER, d_nonces,
                torch.from_numpy(np.array(times, np.int64)).to(dev), d_pub, d_hin,
                torch.from_numpy(sk_es).to(dev))
            assert not sst[:M].any()
            cts = [(tk.config.id, encs[i].tobytes(), pays[i].tobytes()) for i in range(M)]
        else:                                               # P-256 seals stay on the host
            cts = []
            for i in range(M):
                pt = b"\0\0" + len(hin[i]).to_bytes(4, "big") + hin[i].tobytes()
                aad = H.input_share_aad(task_id, nonces[i].tobytes(), times[i], pub[i].tobytes())
                cts.append(H.seal(tk.config, info, pt, aad))
        reqs.append(C.encode_agg_init_req(C.TIME_INTERVAL, None, b"", nonces, times, pub, cts, lp))
        del d_lin, d_rand, d_meas
        print(f"generated job {j + 1}/{J}", file=sys.stderr, flush=True)
    ls.close()
    hs0.close()
    gen_s = time.time() - t0
    drvs, aggs, rep_s, resps = {}, {}, {m: [] for m in modes}, {}
    for m in modes:
        wide = 1 if m != "host" and suite != (0x20, 1, 1) else 0
        drvs[m] = HelperAggregateInit(v, task_id, [tk], hpke_threads=args.threads, hpke=m,
                                      hpke_gpu_suites=wide)
        drvs[m].handle_jobs(reqs[:1], v.new_aggregate(1))  # warm (allocates the state)
        aggs[m] = v.new_aggregate(1)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for m in modes:     # alternating: every mode sees the same machine state over time
            t = time.perf_counter()
            resps[m] = drvs[m].handle_jobs(reqs, aggs[m])
            torch.cuda.synchronize()
            rep_s[m].append(time.perf_counter() - t)
    n = J * M * args.reps
    for m in modes:
        for j, resp in enumerate(resps[m]):
            _, st = C.gather_helper_resps(s, resp, job_nonces[j], np.zeros(M, np.uint8))
            assert (st == 0).all(), f"{m} job {j}: {int((st != 0).sum())} reports rejected"
            assert bytes(resp) == bytes(resps[modes[0]][j]), f"{m} job {j}: response differs"
        _, cnt = aggs[m].read(0)
        assert cnt == n, (m, cnt, n)
        assert aggs[m].read(0) == aggs[modes[0]].read(0), m
    for m in modes:
        report(args, v, s, drvs[m], m, reqs, task_id, tk, rep_s[m], gen_s, label)
        drvs[m].close()


def fused_stage_ms(v, drv, req_bytes):
    """HIP-event milliseconds of every stage of one fused job, by kernel name (copy_request is
    the request's host-to-device copy)."""
    L, ctx = lib(), v._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    L.prio3gpu_prof_enable(ctx, 1)
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        drv.handle(req_bytes, v.new_aggregate(1))
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    return {L.prio3gpu_prof_kernel_name(i).decode(): round(ms[i], 3)
            for i in range(k) if launches[i]}


def report(args, v, s, drv, mode, reqs, task_id, tk, rep_s, gen_s, label):
    J, M = args.jobs, args.job_size
    dt = sum(rep_s)
    n = J * M * args.reps
    # unpipelined per-stage times of one job (host stages one by one, then the GPU stage)
    stages = {}
    req = C.decode_agg_init_req(reqs[0])
    t = time.perf_counter()
    req = C.decode_agg_init_req(reqs[0])
    stages["decode_req"] = time.perf_counter() - t
    t = time.perf_counter()
    C.check_agg_init_req(req)
    nonces_, pub_, lps_, faults_ = C.gather_prepare_inits(s, req)
    stages["check_gather"] = time.perf_counter() - t
    t = time.perf_counter()
    if mode != "fused":     # (fused: these two happen inside the engine call of `prepare`)
        pts, offs, st_ = H.open_report_shares(task_id, req, [tk], [], None, args.threads,
                                              gpu=drv._hpke_ctx)
        stages["hpke_open"] = time.perf_counter() - t
        t = time.perf_counter()
        C.decode_plaintext_input_shares_raw(s, pts, offs, 1, st_)
        stages["decode_plaintext"] = time.perf_counter() - t
    t = time.perf_counter()
    o = drv.open(reqs[0])
    stages["open_total"] = time.perf_counter() - t
    a2 = v.new_aggregate(1)
    t = time.perf_counter()
    drv.prepare(o, a2)
    torch.cuda.synchronize()
    stages["prepare_gpu_encode"] = time.perf_counter() - t
    stages = {k: round(x * 1e3, 2) for k, x in stages.items()}
    rates = sorted(J * M / x for x in rep_s)
    extra = {"fused_stage_ms_one_job": fused_stage_ms(v, drv, reqs[0])} if mode == "fused" else {}
    print(json.dumps({
        "what": "helper aggregate-init end to end: request bytes -> decode -> HPKE open (host "
                "threads) -> GPU prepare+decide+prepare_next+accumulate -> response bytes, "
                "pipelined over jobs",
        "value": round(n / dt, 1), "unit": "reports/s", "jobs": J, "job_size": M,
        "reps": args.reps, "hpke": mode, "suite": args.suite, "hpke_threads": args.threads, "seconds": round(dt, 3),
        "reports_per_s_by_rep": [round(J * M / x) for x in rep_s],
        "median_reports_per_s": round(statistics.median(rates)),
        "min_reports_per_s": round(rates[0]), "max_reports_per_s": round(rates[-1]),
        "request_mb_per_job": round(len(reqs[0]) / 1e6, 1), "gen_seconds": round(gen_s, 1),
        "workload": label, "stage_ms_per_job": stages, **extra}), flush=True)


if __name__ == "__main__":
    main()
