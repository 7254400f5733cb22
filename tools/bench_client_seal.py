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
from janus_amd.client import ClientBatch, encode_plaintext_input_share  # noqa: E402
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


def seal_case(v, kp, role, n, slen, pub_len, reps, host_n, rng, dev):
    """seals/s of seal_input_shares_gpu over n device rows of slen bytes, and of the host loop
    over the first host_n of them, rep by rep in turn."""
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = np.full(n, 1_700_000_000, np.uint64)
    pub = rng.integers(0, 256, (n, pub_len), dtype=np.uint8)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_shares = torch.randint(0, 256, (n, slen), dtype=torch.uint8, device=dev)
    d_ids, d_pub, d_sk = (torch.from_numpy(a).to(dev) for a in (ids, pub, sk))
    d_times = torch.from_numpy(times.view(np.int64)).to(dev)
    d_encs = torch.empty((n, 32), dtype=torch.uint8, device=dev)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--helper-n", type=int, default=65536)
    ap.add_argument("--leader-n", type=int, default=4096)
    ap.add_argument("--reports-n", type=int, default=4096)
    ap.add_argument("--host-n", type=int, default=2048, help="reports of the host seal loop")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    vk = hashlib.shake_128(b"verify-key client seal").digest(16)
    v = Prio3Gpu.new_sum_vec(8, 1000, 89, vk, device=0)
    s = v.sizes
    lkp = H.generate_hpke_config_and_private_key(1)
    hkp = H.generate_hpke_config_and_private_key(2)
    out = {"what": "client seal on one GPU: X25519 / HKDF-SHA256 / AES-128-GCM seals of Prio3 "
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
    cb = ClientBatch(v, TASK_ID, lkp.config, hkp.config, 3600)
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
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
