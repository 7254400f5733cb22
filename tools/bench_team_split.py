"""Several waves per report against one ("hpke_team_split"): prio3gpu_seal_input_shares_long and
prio3gpu_open_input_shares on small batches of very long input shares, the split path
(k_hpke_*_team_split, _join, k_hpke_team_wipe) and the option-0 path (k_hpke_seal_team_shares,
k_hpke_open_team_shares) alternating in the same run.

X25519 / HKDF-SHA256 / AES-128-GCM (--aead 2, 3: AES-256-GCM, ChaCha20-Poly1305), rows in device
memory.  Shares are random bytes; the split path must give the option-0 path's bytes (seal) and
the shares back (open).  Times are a host clock around a device synchronise, after one warm-up
call of each path: the median of --reps with min..max, and the per-kernel HIP-event times of one
call.  One JSON line per case, printed and appended to --out.

  --cases   name:n:share_len[:blocks], comma separated; without blocks (and without
            --split-blocks) "hpke_team_split_blocks" is not set and the line says "engine default".  Default: a FixedPoint16 x 100k leader
            share (25,600,480 bytes) at n = 16 and 64, and a SumVec(8, 1000) leader share
            (134,944 bytes) at n = 64, 1,024 and 4,096 (which must not split).
  --sweep   the segment-size sweep at n = 64: for 4, 16, 64 and 256 KiB ("hpke_team_split_blocks"
            256, 1,024, 4,096, 16,384) the SumVec share cut into segments of at least that size,
            and a share of exactly two such segments (the smallest shape that splits at all).

  python tools/bench_team_split.py [--split 256] [--split-blocks B] [--reps 3] [--aead 3] [--sweep]
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
from janus_amd.prio3 import Prio3Gpu  # noqa: E402

TASK_ID = hashlib.sha256(b"team split bench").digest()
PUB_LEN = 32
ROLE = H.ROLE_LEADER
E_SHARE, SUMVEC_SHARE = 25_600_480, 134_944


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


def wins(split, plain):
    """The split path wins by more than the sum of the two min..max spreads."""
    gap = statistics.median(plain) - statistics.median(split)
    return gap > (max(split) - min(split)) + (max(plain) - min(plain))


def alternate(split_call, plain_call, reps):
    split_call(), plain_call()                               # warm-up of each
    s_ms, p_ms = [], []
    for _ in range(reps):
        for call, into in ((split_call, s_ms), (plain_call, p_ms)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            into.append(1e3 * (time.perf_counter() - t))
    return s_ms, p_ms


def run_case(v, kp, name, n, slen, k, blocks, reps, rng, dev):
    plen = 6 + slen + 16
    ids = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).to(dev)
    times = torch.full((n,), 1_700_000_000, dtype=torch.int64, device=dev)
    pub = torch.from_numpy(rng.integers(0, 256, (n, PUB_LEN), dtype=np.uint8)).to(dev)
    sk = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    shares = torch.randint(0, 256, (n, slen), dtype=torch.uint8, device=dev)
    pitch = 128 * (-(-slen // 128))
    rows = torch.zeros((n, pitch), dtype=torch.uint8, device=dev)
    out = {w: (torch.zeros((n, 32), dtype=torch.uint8, device=dev),
               torch.zeros((n, plen), dtype=torch.uint8, device=dev)) for w in ("split", "plain")}
    if blocks is not None:                                   # None: the engine's own default
        v.set_option("hpke_team_split_blocks", blocks)

    def seal(which):
        def call():
            v.set_option("hpke_team_split", k if which == "split" else 0)
            st = torch.zeros(n, dtype=torch.uint8, device=dev)
            H.seal_input_shares_long_gpu(v, TASK_ID, kp.config, ROLE, ids, times, pub, shares, sk,
                                         out[which][0], out[which][1], st)
            return st
        return call

    def open_(which):
        def call():
            v.set_option("hpke_team_split", k if which == "split" else 0)
            st = torch.zeros(n, dtype=torch.uint8, device=dev)
            H.open_input_shares_gpu(v, TASK_ID, kp, ROLE, ids, times, pub, out["plain"][0],
                                    out["plain"][1], out_shares=rows[:, :slen], status=st)
            return st
        return call

    seal_s, seal_p = alternate(seal("split"), seal("plain"), reps)
    assert torch.equal(out["split"][0], out["plain"][0])
    assert torch.equal(out["split"][1], out["plain"][1])
    rows.zero_()
    assert not open_("split")().any().item() and torch.equal(rows[:, :slen], shares)
    rows.zero_()
    assert not open_("plain")().any().item() and torch.equal(rows[:, :slen], shares)
    open_s, open_p = alternate(open_("split"), open_("plain"), reps)
    seal_k, open_k = stage_ms(v, seal("split")), stage_ms(v, open_("split"))
    seal_k0, open_k0 = stage_ms(v, seal("plain")), stage_ms(v, open_("plain"))
    v.set_option("hpke_team_split", 0)
    aead = {1: "AES-128-GCM", 2: "AES-256-GCM", 3: "ChaCha20-Poly1305"}[kp.config.aead_id]
    med = statistics.median
    return {"case": name, "suite": "X25519 / HKDF-SHA256 / " + aead, "n": n, "share_bytes": slen,
            "hpke_team_split": k,
            "hpke_team_split_blocks": "engine default" if blocks is None else blocks, "reps": reps,
            "split_ran": "k_hpke_seal_team_split" in seal_k,
            "seal_split_ms": spread(seal_s), "seal_one_wave_ms": spread(seal_p),
            "seal_one_wave_over_split": round(med(seal_p) / med(seal_s), 2),
            "seal_split_wins": wins(seal_s, seal_p),
            "open_split_ms": spread(open_s), "open_one_wave_ms": spread(open_p),
            "open_one_wave_over_split": round(med(open_p) / med(open_s), 2),
            "open_split_wins": wins(open_s, open_p),
            "seal_split_gb_per_s": round(n * plen / med(seal_s) / 1e6, 2),
            "open_split_gb_per_s": round(n * plen / med(open_s) / 1e6, 2),
            "seal_split_kernel_ms": seal_k, "seal_one_wave_kernel_ms": seal_k0,
            "open_split_kernel_ms": open_k, "open_one_wave_kernel_ms": open_k0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split", type=int, default=256, help='"hpke_team_split" of the split path')
    ap.add_argument("--split-blocks", type=int, default=None,
                    help='"hpke_team_split_blocks" (default: the engine\'s)')
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--aead", type=int, choices=(1, 2, 3), default=1)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "team_split",
                                                  "bench_team_split.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    kp = H.generate_hpke_config_and_private_key(1, H.KEM_X25519_HKDF_SHA256, 1, args.aead)
    default_blocks = args.split_blocks         # None: the option is not set, the engine's default
    if args.sweep:
        cases = []
        for kib in (4, 16, 64, 256):
            blocks = kib * 64
            cases.append((f"sumvec_seg{kib}k", 64, SUMVEC_SHARE, blocks))
            cases.append((f"two_seg{kib}k", 64, 2 * 1024 * kib - 6, blocks))
    elif args.cases:
        cases = []
        for c in args.cases.split(","):
            f = c.split(":")
            cases.append((f[0], int(f[1]), int(f[2]), int(f[3]) if len(f) > 3 else default_blocks))
    else:
        cases = [("fp16_100k", 16, E_SHARE, default_blocks),
                 ("fp16_100k", 64, E_SHARE, default_blocks),
                 ("sumvec_8_1000", 64, SUMVEC_SHARE, default_blocks),
                 ("sumvec_8_1000", 1024, SUMVEC_SHARE, default_blocks),
                 ("sumvec_8_1000", 4096, SUMVEC_SHARE, default_blocks)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, n, slen, blocks in cases:
        v = Prio3Gpu.new_count(bytes(16), device=0)    # a context per case: no option is inherited
        if args.aead == 3:
            v.set_option("hpke_team_chacha", 1)
        line = json.dumps(run_case(v, kp, name, n, slen, args.split, blocks, args.reps, rng, dev))
        v.close()
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
