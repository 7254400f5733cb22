"""Client-side seal throughput on one GPU: the batched HPKE seal of Prio3 input shares
(hpke.seal_input_shares_gpu), whole reports from ClientBatch.prepare_reports, and the host's
per-report `hpke.seal` loop over the same inputs, alternating in the same run.

Two sizes: --helper-n seals of a 54-byte plaintext (a Prio3 helper share with joint randomness:
two 16-byte seeds and a 16-byte blind behind the 6-byte PlaintextInputShare header), and
--leader-n seals of a SumVec(8, 1000) leader share (134,950-byte plaintext).  Shares are random
bytes in device memory (the seal does not look inside them); prepare_reports runs the real
Prio3SumVec(8, 1000, 89) shard.  Times are a host clock around a device synchronise, after one
warm-up call; the per-kernel HIP-event times of one call are listed beside them.  One JSON line.

  python tools/bench_client_seal.py [--helper-n 65536] [--leader-n 4096] [--reps 3]

With --long the run instead sets the wave-per-report seal (hpke.seal_input_shares_long_gpu) beside
the lane-per-report seal over the same device rows, alternating, outputs asserted equal: the
leader share, the helper share, a sweep of share lengths with the threshold it gives for
ClientBatch.LONG_SEAL_MIN_SHARE, and prepare_reports under long_seal=False and auto.

  python tools/bench_client_seal.py --long [--aead {1,2,3}] [--threshold-from-sweep] [--out FILE.jsonl]

--aead picks both aggregators' AEAD under --long (1 AES-128-GCM, the default; 2 AES-256-GCM; 3
ChaCha20-Poly1305, which sets the context option "hpke_team_chacha" and has its own threshold,
ClientBatch.LONG_SEAL_MIN_SHARE_CHACHA).
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

from janus_amd import hpke as H  # noqa: E402
from janus_amd._lib import lib  # noqa: E402
from janus_amd.client import (ClientBatch, draw_p256_scalars,  # noqa: E402
                              encode_plaintext_input_share)
from janus_amd.prio3 import Prio3Gpu  # noqa: E402

TASK_ID = hashlib.sha256(b"client seal bench").digest()


def stage_ms(v, fn):
    """HIP-event milliseconds of every kernel of one call of fn, by kernel name."""
    L, ctx = lib(), v._ctx
    ms, launches = (ctypes.c_double * 64)(), (ctypes.c_uint64 * 64)()
    L.prio3gpu_prof_enable(ctx, 1)
    try:
        L.prio3gpu_prof_read(ctx, ms, launches, 64)  # drain
        fn()
        k = L.prio3gpu_prof_read(ctx, ms, launches, 64)
    finally:
        L.prio3gpu_prof_enable(ctx, 0)
    return {L.prio3gpu_prof_kernel_name(i).decode(): round(ms[i], 3)
            for i in range(k) if launches[i]}


def ephemeral_keys(rng, config, n):
    """(n, 32) ephemeral private keys for `config`'s KEM: any bytes for X25519, big-endian
    scalars in [1, n) for P-256."""
    if config.kem_id == H.KEM_P256_HKDF_SHA256:
        return draw_p256_scalars(n, lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes())
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def seal_case(v, kp, role, n, slen, pub_len, reps, host_n, rng, dev):
    """seals/s of seal_input_shares_gpu over n device rows of slen bytes, and of the host loop
    over the first host_n of them, rep by rep in turn."""
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = np.full(n, 1_700_000_000, np.uint64)
    pub = rng.integers(0, 256, (n, pub_len), dtype=np.uint8)
    sk = ephemeral_keys(rng, kp.config, n)
    d_shares = torch.randint(0, 256, (n, slen), dtype=torch.uint8, device=dev)
    d_ids, d_pub, d_sk = (torch.from_numpy(a).to(dev) for a in (ids, pub, sk))
    d_times = torch.from_numpy(times.view(np.int64)).to(dev)
    d_encs = torch.empty((n, H.enc_len(kp.config.kem_id)), dtype=torch.uint8, device=dev)
    d_pay = torch.empty((n, 6 + slen + 16), dtype=torch.uint8, device=dev)
    info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, role)

    def gpu_call():
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        H.seal_input_shares_gpu(v, TASK_ID, kp.config, role, d_ids, d_times, d_pub, d_shares,
                                d_sk, d_encs, d_pay, status=d_st)
        torch.cuda.synchronize()
        return d_st

    assert not gpu_call().any().item()                          # warm-up
    shares = d_shares[:host_n].cpu().numpy()

    def host_loop():
        out = []
        for i in range(host_n):
            aad = H.input_share_aad(TASK_ID, ids[i].tobytes(), int(times[i]), pub[i].tobytes())
            out.append(H.seal(kp.config, info, encode_plaintext_input_share(shares[i].tobytes()),
                              aad, ephemeral_private_key=sk[i].tobytes()))
        return out

    host = host_loop()                                          # warm-up, and the byte check
    got_e, got_p = d_encs[:host_n].cpu().numpy(), d_pay[:host_n].cpu().numpy()
    for i in (0, host_n // 2, host_n - 1):
        assert (got_e[i].tobytes(), got_p[i].tobytes()) == host[i][1:], i
    gpu_s, host_s = [], []
    for _ in range(reps):
        t = time.perf_counter()
        gpu_call()
        gpu_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        host_loop()
        host_s.append(time.perf_counter() - t)
    return {"n": n, "plaintext_bytes": 6 + slen,
            "gpu_seals_per_s": round(n / statistics.median(gpu_s)),
            "gpu_seals_per_s_by_rep": [round(n / x) for x in gpu_s],
            "host_loop_n": host_n,
            "host_loop_seals_per_s": round(host_n / statistics.median(host_s)),
            "kernel_ms": stage_ms(v, gpu_call)}


def spread(xs):
    """{median, min, max} of a list of seconds, in milliseconds."""
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3),
            "max_ms": round(1e3 * max(xs), 3)}


def wins(fast, slow):
    """`fast` beats `slow` by more than the sum of the two min..max spreads."""
    return (slow["median_ms"] - fast["median_ms"]
            > (slow["max_ms"] - slow["min_ms"]) + (fast["max_ms"] - fast["min_ms"]))


def long_case(v, kp, role, n, slen, pub_len, reps, rng, dev):
    """seal_input_shares_long_gpu (a wave per report) and seal_input_shares_gpu (a lane per
    report) over the same n device rows of slen bytes, rep by rep in turn after one warm-up of
    each; the outputs must be equal."""
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = np.full(n, 1_700_000_000, np.uint64)
    pub = rng.integers(0, 256, (n, pub_len), dtype=np.uint8)
    sk = ephemeral_keys(rng, kp.config, n)
    d_shares = torch.randint(0, 256, (n, slen), dtype=torch.uint8, device=dev)
    d_ids, d_pub, d_sk = (torch.from_numpy(a).to(dev) for a in (ids, pub, sk))
    d_times = torch.from_numpy(times.view(np.int64)).to(dev)
    plen = 6 + slen + 16
    outs = {k: (torch.empty((n, H.enc_len(kp.config.kem_id)), dtype=torch.uint8, device=dev),
                torch.empty((n, plen), dtype=torch.uint8, device=dev)) for k in ("wave", "lane")}
    fns = {"wave": H.seal_input_shares_long_gpu, "lane": H.seal_input_shares_gpu}

    def call(k):
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fns[k](v, TASK_ID, kp.config, role, d_ids, d_times, d_pub, d_shares, d_sk, *outs[k],
               status=d_st)
        torch.cuda.synchronize()
        return d_st

    for k in fns:                                               # warm-up
        assert not call(k).any().item()
    assert torch.equal(outs["wave"][0], outs["lane"][0])
    assert torch.equal(outs["wave"][1], outs["lane"][1])
    secs = {"wave": [], "lane": []}
    for _ in range(reps):
        for k in fns:
            t = time.perf_counter()
            call(k)
            secs[k].append(time.perf_counter() - t)
    res = {"n": n, "share_bytes": slen, "sealed_bytes": n * (6 + slen)}
    for k in fns:
        res[k] = dict(spread(secs[k]), kernel_ms=stage_ms(v, lambda: call(k)))
    res["wave_over_lane"] = round(res["lane"]["median_ms"] / res["wave"]["median_ms"], 2)
    res["wave_wins_by_more_than_the_spreads"] = wins(res["wave"], res["lane"])
    return res


SWEEP = ((256, 16384), (1024, 8192), (2576, 4096), (16384, 4096), (65536, 4096))   # (share, n)


def long_main(args, v, lkp, hkp, rng, dev):
    """The wave-per-report seal beside the lane-per-report seal (--long): (a) the leader share,
    (b) the helper share, (c) a length sweep and the threshold it gives, (d) prepare_reports with
    long_seal=False and auto."""
    s = v.sizes
    aead = {1: "AES-128-GCM", 2: "AES-256-GCM", 3: "ChaCha20-Poly1305"}[args.aead]
    attr = "LONG_SEAL_MIN_SHARE_CHACHA" if args.aead == 3 else "LONG_SEAL_MIN_SHARE"
    kem = "P-256" if args.kem == H.KEM_P256_HKDF_SHA256 else "X25519"
    out = {"what": f"client seal on one GPU, a wave per report beside a lane per report: {kem} / "
                   f"HKDF-SHA256 / {aead} seals of Prio3 input shares from device rows, the "
                   "two paths alternating over the same inputs (outputs asserted equal), host "
                   "clock around a synchronise, median of reps with min..max; and whole "
                   "Prio3SumVec(8, 1000, 89) reports under long_seal=False and auto",
           "reps": args.reps}
    out["a_leader_share"] = long_case(v, lkp, H.ROLE_LEADER, args.leader_n, s.leader_input_share,
                                      s.public_share, args.reps, rng, dev)
    out["b_helper_share"] = long_case(v, hkp, H.ROLE_HELPER, args.helper_n, s.helper_input_share,
                                      s.public_share, args.reps, rng, dev)
    sweep = [long_case(v, lkp, H.ROLE_LEADER, n, slen, s.public_share, args.reps, rng, dev)
             for slen, n in SWEEP]
    out["c_sweep"] = sweep
    # the smallest swept length from which the wave path wins at every longer length too
    threshold = None
    for case in reversed(sweep + [out["a_leader_share"]]):
        if not case["wave_wins_by_more_than_the_spreads"]:
            break
        threshold = case["share_bytes"]
    out["c_threshold"] = threshold
    out["configured_long_seal_min_share"] = getattr(ClientBatch, attr)
    if args.threshold_from_sweep:
        setattr(ClientBatch, attr, threshold)
    n = args.reports_n
    meas = rng.integers(0, 256, (n, 1000), dtype=np.int64)
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    rand = rng.integers(0, 256, (n, v.random_size()), dtype=np.uint8)
    sk = np.stack([ephemeral_keys(rng, lkp.config, n), ephemeral_keys(rng, hkp.config, n)])
    times = np.full(n, 1_700_000_000, np.uint64)
    chacha, p256 = args.aead == 3, args.kem == H.KEM_P256_HKDF_SHA256
    cbs = {"lane": ClientBatch(v, TASK_ID, lkp.config, hkp.config, 3600, long_seal=False,
                               p256=p256),
           "auto": ClientBatch(v, TASK_ID, lkp.config, hkp.config, 3600, team_chacha=chacha,
                               p256=p256)}

    def prepare(k):
        r = cbs[k].prepare_reports(meas, report_ids=ids, times=times, rand=rand, sk_es=sk,
                                   device_out=True)
        torch.cuda.synchronize()
        return r

    got = {k: prepare(k) for k in cbs}                          # warm-up, and the byte check
    assert torch.equal(got["lane"], got["auto"])
    del got
    secs = {"lane": [], "auto": []}
    for _ in range(args.reps):
        for k in cbs:
            t = time.perf_counter()
            prepare(k)
            secs[k].append(time.perf_counter() - t)
    d = {"n": n, "report_bytes": cbs["lane"].report_len,
         "auto_min_share": getattr(ClientBatch, attr),
         "auto_wave_routes": dict(zip(("leader", "helper"), cbs["auto"]._wave))}
    for k in cbs:
        d[k] = dict(spread(secs[k]), reports_per_s=round(n / statistics.median(secs[k])),
                    kernel_ms=stage_ms(v, lambda: prepare(k)))
        cbs[k].close()
    out["d_prepare_reports"] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--helper-n", type=int, default=65536)
    ap.add_argument("--leader-n", type=int, default=4096)
    ap.add_argument("--reports-n", type=int, default=4096)
    ap.add_argument("--host-n", type=int, default=2048, help="reports of the host seal loop")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long", action="store_true",
                    help="the wave-per-report seal beside the lane-per-report seal instead")
    ap.add_argument("--threshold-from-sweep", action="store_true",
                    help="with --long: auto in prepare_reports routes by the threshold this run's "
                         "sweep gives, not by ClientBatch.LONG_SEAL_MIN_SHARE")
    ap.add_argument("--aead", type=int, choices=(1, 2, 3), default=1,
                    help="with --long: both aggregators' AEAD; 3 (ChaCha20-Poly1305) sets the "
                         'context option "hpke_team_chacha"')
    ap.add_argument("--kem", type=lambda x: int(x, 0), choices=(0x20, 0x10), default=0x20,
                    help='both aggregators\' KEM; 0x10 (P-256) sets the context option '
                         '"hpke_gpu_p256"')
    ap.add_argument("--out", help="append the JSON line to this file as well")
    args = ap.parse_args()
    if args.long:
        rng = np.random.default_rng(2026)
        vk = hashlib.shake_128(b"verify-key client seal").digest(16)
        v = Prio3Gpu.new_sum_vec(8, 1000, 89, vk, device=0)
        if args.aead == 3:
            v.set_option("hpke_team_chacha", 1)
        if args.kem == H.KEM_P256_HKDF_SHA256:
            v.set_option("hpke_gpu_p256", 1)
        X = args.kem
        line = json.dumps(long_main(args, v,
                                    H.generate_hpke_config_and_private_key(1, X, 1, args.aead),
                                    H.generate_hpke_config_and_private_key(2, X, 1, args.aead),
                                    rng, torch.device("cuda", 0)))
        v.close()
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    vk = hashlib.shake_128(b"verify-key client seal").digest(16)
    v = Prio3Gpu.new_sum_vec(8, 1000, 89, vk, device=0)
    s = v.sizes
    p256 = args.kem == H.KEM_P256_HKDF_SHA256
    if p256:
        v.set_option("hpke_gpu_p256", 1)
    lkp = H.generate_hpke_config_and_private_key(1, args.kem)
    hkp = H.generate_hpke_config_and_private_key(2, args.kem)
    out = {"what": f"client seal on one GPU: {'P-256' if p256 else 'X25519'} / HKDF-SHA256 / "
                   "AES-128-GCM seals of Prio3 "
                   "input shares from device rows, whole Prio3SumVec(8, 1000, 89) reports, and "
                   "the host's per-report seal loop over the same inputs",
           "reps": args.reps}
    assert s.helper_input_share + 6 == 54 and s.leader_input_share + 6 == 134950
    out["helper_share"] = seal_case(v, hkp, H.ROLE_HELPER, args.helper_n, s.helper_input_share,
                                    s.public_share, args.reps, min(args.host_n, args.helper_n),
                                    rng, dev)
    out["leader_share"] = seal_case(v, lkp, H.ROLE_LEADER, args.leader_n, s.leader_input_share,
                                    s.public_share, args.reps, min(64, args.leader_n), rng, dev)
    n = args.reports_n
    cb = ClientBatch(v, TASK_ID, lkp.config, hkp.config, 3600, p256=p256)
    meas = rng.integers(0, 256, (n, 1000), dtype=np.int64)
    cb.prepare_reports(meas[:256])                              # warm-up
    rep_s = []
    for _ in range(args.reps):
        t = time.perf_counter()
        r = cb.prepare_reports(meas, device_out=True)
        torch.cuda.synchronize()
        rep_s.append(time.perf_counter() - t)
    out["prepare_reports"] = {"n": n, "report_bytes": cb.report_len,
                              "reports_per_s": round(n / statistics.median(rep_s)),
                              "reports_per_s_by_rep": [round(n / x) for x in rep_s],
                              "kernel_ms": stage_ms(v, lambda: cb.prepare_reports(
                                  meas, device_out=True))}
    assert tuple(r.shape) == (n, cb.report_len)
    cb.close()
    v.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
