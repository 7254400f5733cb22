"""Upload-side open throughput on one GPU: Prio3 input shares opened a wave per report
(hpke.open_input_shares_gpu, k_hpke_open_team_shares) and, alternating in the same run, the same
ciphertexts through the lane-per-report prio3gpu_hpke_open_batch (k_hpke_open), the baseline.

Two cases under X25519 / HKDF-SHA256 / AES-128-GCM (--aead 2: AES-256-GCM; --aead 3:
ChaCha20-Poly1305, with the context options the two GPU paths need for it), rows in device memory:
  leader   --leader-n payloads of a SumVec(8, 1000) leader share (134,966 bytes each)
  helper   --helper-n payloads of a helper share with joint randomness (70 bytes each)
Shares are random bytes sealed on the GPU (hpke.seal_input_shares_gpu); both paths must give them
back.  Times are a host clock around a device synchronise, after one warm-up call of each path:
the median of --reps with min..max, and the per-kernel HIP-event times of one call.  One JSON line
per case, printed and appended to --out.

The first --host-n reports are also opened once by the host's hpke.open_ loop, the route
UploadBatch takes for a suite it does not give to the GPU.

  python tools/bench_upload_open.py [--leader-n 4096] [--helper-n 65536] [--reps 3] [--aead 3]
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
from janus_amd.client import draw_p256_scalars  # noqa: E402
from janus_amd.prio3 import Prio3Gpu  # noqa: E402

TASK_ID = hashlib.sha256(b"upload open bench").digest()
PUB_LEN = 32


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


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def open_case(v, kp, case, n, slen, reps, rng, dev, host_n=0):
    role = H.ROLE_LEADER
    plen = 6 + slen + 16
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = np.full(n, 1_700_000_000, np.uint64)
    pub = rng.integers(0, 256, (n, PUB_LEN), dtype=np.uint8)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nenc = H.enc_len(kp.config.kem_id)
    if nenc == 65:    # P-256: scalars in [1, n)
        sk = draw_p256_scalars(n, lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes())
    d_shares = torch.randint(0, 256, (n, slen), dtype=torch.uint8, device=dev)
    d_ids, d_pub, d_sk = (torch.from_numpy(a).to(dev) for a in (ids, pub, sk))
    d_times = torch.from_numpy(times.view(np.int64)).to(dev)
    d_encs = torch.empty((n, nenc), dtype=torch.uint8, device=dev)
    d_pay = torch.empty((n, plen), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _, _, st = H.seal_input_shares_gpu(v, TASK_ID, kp.config, role, d_ids, d_times, d_pub,
                                       d_shares, d_sk, d_encs, d_pay)
    assert not st[:n].any()
    # the wave path: share rows at a 128-byte pitch
    pitch = 128 * (-(-slen // 128))
    d_rows = torch.zeros((n, pitch), dtype=torch.uint8, device=dev)

    def team_call():
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        H.open_input_shares_gpu(v, TASK_ID, kp, role, d_ids, d_times, d_pub, d_encs, d_pay,
                                out_shares=d_rows[:, :slen], status=d_st)
        torch.cuda.synchronize()
        return d_st

    # the lane path: the same ciphertexts as packed slots, the AADs as bytes
    aad = np.zeros((n, 60 + PUB_LEN), np.uint8)
    aad[:, :32] = np.frombuffer(TASK_ID, np.uint8)
    aad[:, 32:48] = ids
    aad[:, 48:56] = times.astype(">u8").view(np.uint8).reshape(n, 8)
    aad[:, 56:60] = np.frombuffer(PUB_LEN.to_bytes(4, "big"), np.uint8)
    aad[:, 60:] = pub
    d_aad = torch.from_numpy(aad).to(dev)
    off = lambda w: torch.from_numpy(np.arange(n + 1, dtype=np.int64) * w).to(dev)  # noqa: E731
    d_aoff, d_coff, d_poff = off(60 + PUB_LEN), off(plen), off(6 + slen)
    d_pts = torch.zeros((n, 6 + slen), dtype=torch.uint8, device=dev)
    info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, role)

    def lane_call():
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        H.open_batch_gpu(v, kp, info, d_encs.data_ptr(), d_aad.data_ptr(), d_aoff.data_ptr(),
                         d_pay.data_ptr(), d_coff.data_ptr(), pts=d_pts.data_ptr(),
                         pt_offsets=d_poff.data_ptr(), status=d_st.data_ptr(), n=n)
        torch.cuda.synchronize()
        return d_st

    assert not team_call().any().item() and not lane_call().any().item()      # warm-up
    assert torch.equal(d_rows[:, :slen], d_shares) and torch.equal(d_pts[:, 6:], d_shares)
    team_ms, lane_ms = [], []
    for _ in range(reps):
        t = time.perf_counter()
        team_call()
        team_ms.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        lane_call()
        lane_ms.append(1e3 * (time.perf_counter() - t))
    tm, lm = statistics.median(team_ms), statistics.median(lane_ms)
    # UploadBatch's host route for a suite the wave does not take: hpke.open_ report by report
    host_n = min(host_n, n)
    h_enc, h_pay = d_encs[:host_n].cpu().numpy(), d_pay[:host_n].cpu().numpy()
    h_shares = d_shares[:host_n].cpu().numpy()
    t = time.perf_counter()
    for i in range(host_n):
        pt = H.open_(kp, info, h_enc[i].tobytes(), h_pay[i].tobytes(), aad[i].tobytes())
        assert pt[6:] == h_shares[i].tobytes()
    host_ms = 1e3 * (time.perf_counter() - t)
    aead = {1: "AES-128-GCM", 2: "AES-256-GCM", 3: "ChaCha20-Poly1305"}[kp.config.aead_id]
    kem = "P-256" if nenc == 65 else "X25519"
    return {"case": case, "suite": kem + " / HKDF-SHA256 / " + aead, "n": n,
            "payload_bytes": plen, "reps": reps, "host_loop_n": host_n,
            "host_loop_opens_per_s": round(host_n / host_ms * 1e3) if host_n else None,
            "wave_per_report_ms": spread(team_ms), "lane_per_report_ms": spread(lane_ms),
            "wave_opens_per_s": round(n / tm * 1e3), "lane_opens_per_s": round(n / lm * 1e3),
            "wave_gb_per_s": round(n * plen / tm / 1e6, 2),
            "lane_gb_per_s": round(n * plen / lm / 1e6, 2),
            "lane_over_wave": round(lm / tm, 2),
            "wave_kernel_ms": stage_ms(v, team_call), "lane_kernel_ms": stage_ms(v, lane_call)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leader-n", type=int, default=4096)
    ap.add_argument("--helper-n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--aead", type=int, choices=(1, 2, 3), default=1,
                    help="the key's AEAD; 2 and 3 set \"hpke_gpu_suites\" for the lane path, 3 "
                         "(ChaCha20-Poly1305) also \"hpke_team_chacha\" for the wave path")
    ap.add_argument("--kem", type=lambda x: int(x, 0), choices=(0x20, 0x10), default=0x20,
                    help="the key's KEM; 0x10 (P-256) sets \"hpke_gpu_p256\"")
    ap.add_argument("--host-n", type=int, default=256,
                    help="reports of the host's open loop, once (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upload_open",
                                                  "bench_upload_open.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    v = Prio3Gpu.new_count(bytes(16), device=0)
    if args.aead != 1:
        v.set_option("hpke_gpu_suites", 1)
    if args.aead == 3:
        v.set_option("hpke_team_chacha", 1)
    if args.kem == H.KEM_P256_HKDF_SHA256:
        v.set_option("hpke_gpu_p256", 1)
    kp = H.generate_hpke_config_and_private_key(1, args.kem, 1, args.aead)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case, n, slen in (("leader", args.leader_n, 134_944), ("helper", args.helper_n, 48)):
        if n <= 0:
            continue
        line = json.dumps(open_case(v, kp, case, n, slen, args.reps, rng, dev, args.host_n))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
    v.close()


if __name__ == "__main__":
    main()
