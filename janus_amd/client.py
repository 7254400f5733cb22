"""The DAP client, batched on the GPU: measurements in, upload-ready `Report` bytes out.

Mirrors `Client::prepare_report` of Janus's client/src/lib.rs:212-258 for a whole batch: shard
(prio3gpu_shard), wrap each input share in a `PlaintextInputShare`, `hpke::seal` it to its
aggregator under the `InputShareAad` (prio3gpu_seal_input_shares: both frames are read lane by
lane from the share rows and never built; for long AES-GCM shares
prio3gpu_seal_input_shares_long, a wave per report), and encode a `Report`.  Every report of one
`ClientBatch` has the same length, so a batch is an (n, report_len) uint8 matrix whose columns
are the fields of messages/src/lib.rs's `Report`:

  ReportMetadata   report_id[16] | time u64
  public_share     u32 length | bytes
  HpkeCiphertext   config_id u8 | u16 length | enc[32 or 65] | u32 length | payload    (leader)
  HpkeCiphertext   the same                                                            (helper)
  payload = AEAD(PlaintextInputShare = 00 00 | u32 length | input share) || tag[16]

The framing is pinned by the reference's own KATs (tests/test_client_frames.py).
"""
from __future__ import annotations

import os
import struct
import time as _time
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import hpke as H

ENC_LEN = 32        # Nenc of DHKEM(X25519, HKDF-SHA256), the KEM the GPU seals to by default
# The order n of P-256's group: an ephemeral private key is a scalar in [1, n) (RFC 9180 §7.1.3)
P256_ORDER = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
TAG_LEN = 16
PLAINTEXT_OVERHEAD = 6   # empty extension list (u16) + payload length (u32)


def encode_plaintext_input_share(payload: bytes, extensions: bytes = b"") -> bytes:
    """PlaintextInputShare (messages/src/lib.rs:1850-1895); `extensions` is the encoded list's
    body (empty: what a client sends)."""
    return struct.pack(">H", len(extensions)) + bytes(extensions) + struct.pack(
        ">I", len(payload)) + bytes(payload)


def encode_hpke_ciphertext(config_id: int, enc: bytes, payload: bytes) -> bytes:
    return (bytes([config_id]) + struct.pack(">H", len(enc)) + bytes(enc)
            + struct.pack(">I", len(payload)) + bytes(payload))


def encode_report(report_id: bytes, time: int, public_share: bytes, leader_ciphertext,
                  helper_ciphertext) -> bytes:
    """Report (messages/src/lib.rs:1529-1610); a ciphertext is (config id, enc, payload)."""
    assert len(report_id) == 16
    return (bytes(report_id) + struct.pack(">Q", time) + struct.pack(">I", len(public_share))
            + bytes(public_share) + encode_hpke_ciphertext(*leader_ciphertext)
            + encode_hpke_ciphertext(*helper_ciphertext))


class HpkeCiphertext(NamedTuple):
    config_id: int
    encapsulated_key: bytes
    payload: bytes


class Report(NamedTuple):
    report_id: bytes
    time: int
    public_share: bytes
    leader_encrypted_input_share: HpkeCiphertext
    helper_encrypted_input_share: HpkeCiphertext


def decode_report(data: bytes) -> Report:
    """Report::get_decoded: `ValueError` for a truncated encoding or trailing bytes."""
    data = bytes(data)
    pos = 0

    def take(k: int) -> bytes:
        nonlocal pos
        if k < 0 or pos + k > len(data):
            raise ValueError("Report: unexpected end of input")
        pos += k
        return data[pos - k:pos]

    def ciphertext() -> HpkeCiphertext:
        cfg = take(1)[0]
        enc = take(struct.unpack(">H", take(2))[0])
        return HpkeCiphertext(cfg, enc, take(struct.unpack(">I", take(4))[0]))

    rid = take(16)
    t = struct.unpack(">Q", take(8))[0]
    pub = take(struct.unpack(">I", take(4))[0])
    leader, helper = ciphertext(), ciphertext()
    if pos != len(data):
        raise ValueError(f"Report: {len(data) - pos} trailing bytes")
    return Report(rid, t, pub, leader, helper)


def _like(dst, a: np.ndarray):
    """The numpy array `a` as what can be assigned into `dst` (numpy array or torch tensor)."""
    if isinstance(dst, np.ndarray):
        return a
    import torch
    return torch.from_numpy(np.array(a)).to(dst.device)


class ReportLayout:
    """Column offsets of the fixed-stride Report matrix for given public-share and input-share
    lengths; `leader_enc` / `helper_enc` are the lengths of the two encapsulated keys, 32
    (X25519, the default) or 65 (P-256)."""

    def __init__(self, public_share: int, leader_share: int, helper_share: int,
                 leader_enc: int = ENC_LEN, helper_enc: int = ENC_LEN):
        self.public_share, self.leader_share, self.helper_share = (public_share, leader_share,
                                                                   helper_share)
        self.leader_enc, self.helper_enc = int(leader_enc), int(helper_enc)
        self.leader_payload = PLAINTEXT_OVERHEAD + leader_share + TAG_LEN
        self.helper_payload = PLAINTEXT_OVERHEAD + helper_share + TAG_LEN
        o = 0
        self.o_report_id, o = o, o + 16
        self.o_time, o = o, o + 8
        self.o_public_len, o = o, o + 4
        self.o_public, o = o, o + public_share
        self.o_leader = o                  # config id, 00 20 / 00 41, enc, u32 length, payload
        self.o_leader_enc = o + 3
        self.o_leader_payload = o + 3 + self.leader_enc + 4
        o = self.o_leader_payload + self.leader_payload
        self.o_helper = o
        self.o_helper_enc = o + 3
        self.o_helper_payload = o + 3 + self.helper_enc + 4
        self.report_len = self.o_helper_payload + self.helper_payload
        assert self.report_len == (16 + 8 + 4 + public_share + 2 * (1 + 2 + 4 + 6 + 16)
                                   + self.leader_enc + self.helper_enc + leader_share
                                   + helper_share)

    def write_fixed(self, reports, report_ids: np.ndarray, times: np.ndarray, public_shares,
                    leader_config_id: int, helper_config_id: int) -> None:
        """Everything of `reports` (an (n, report_len) uint8 numpy array or torch tensor) except
        the enc and payload columns: metadata, the public share with its length prefix, the
        config ids and the `00 20` (`00 41` for a 65-byte enc) / u32 length prefixes of both
        ciphertexts.  `public_shares`:
        (n, public_share) rows of the same kind as `reports`, or None when there are none."""
        n = reports.shape[0]
        head = np.empty((n, 28), np.uint8)
        head[:, :16] = np.asarray(report_ids, np.uint8).reshape(n, 16)
        head[:, 16:24] = np.asarray(times, np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
        head[:, 24:28] = np.frombuffer(struct.pack(">I", self.public_share), np.uint8)
        reports[:, :28] = _like(reports, head)
        if self.public_share:
            reports[:, self.o_public:self.o_public + self.public_share] = public_shares
        for o, cfg, plen, ne in (
                (self.o_leader, leader_config_id, self.leader_payload, self.leader_enc),
                (self.o_helper, helper_config_id, self.helper_payload, self.helper_enc)):
            pre = np.frombuffer(bytes([cfg]) + struct.pack(">H", ne), np.uint8)
            reports[:, o:o + 3] = _like(reports, pre)
            ln = np.frombuffer(struct.pack(">I", plen), np.uint8)
            reports[:, o + 3 + ne:o + 3 + ne + 4] = _like(reports, ln)

    def columns(self, reports, which: str):
        """(enc column, payload column) views of `reports` for "leader" or "helper"."""
        oe, op, pl, ne = ((self.o_leader_enc, self.o_leader_payload, self.leader_payload,
                           self.leader_enc) if which == "leader" else
                          (self.o_helper_enc, self.o_helper_payload, self.helper_payload,
                           self.helper_enc))
        return reports[:, oe:oe + ne], reports[:, op:op + pl]


def draw_p256_scalars(n: int, rand=os.urandom) -> np.ndarray:
    """n ephemeral P-256 private keys as (n, 32) big-endian bytes, each in [1, n): a draw of 0 or
    >= the group order is drawn again (RFC 9180 §7.1.3's rejection sampling; about one draw in
    2^32 is refused).  `rand(k)` gives k random bytes."""
    out = np.frombuffer(rand(32 * n), np.uint8).reshape(n, 32).copy()
    # k < n word by word from the top, for all rows at once; the rare refused row is redrawn alone
    words = out.view(">u8").reshape(n, 4)
    order = np.frombuffer(P256_ORDER.to_bytes(32, "big"), ">u8")
    below, equal = np.zeros(n, bool), np.ones(n, bool)
    for j in range(4):
        below |= equal & (words[:, j] < order[j])
        equal &= words[:, j] == order[j]
    for i in np.flatnonzero(~(below & out.any(axis=1))):
        while not 1 <= int.from_bytes(out[i].tobytes(), "big") < P256_ORDER:
            out[i] = np.frombuffer(rand(32), np.uint8)
    return out


def round_times(times, time_precision: int) -> np.ndarray:
    """Time::to_batch_interval_start: each time rounded down to a multiple of the precision."""
    t = np.asarray(times, np.uint64)
    return t - t % np.uint64(time_precision)


class ClientBatch:
    """The batched `Client` of one task: `vdaf` a `Prio3Gpu`, the two aggregators' `HpkeConfig`s
    (DHKEM(X25519, HKDF-SHA256), or with `p256` DHKEM(P-256, HKDF-SHA256) too, with any KDF and
    AEAD) and the task's time precision in seconds.

    `long_seal` picks the seal's kernels per aggregator; the report bytes never depend on it.
    False: a GPU lane per report (`hpke.seal_input_shares_gpu`).  True: a wave per report
    (`hpke.seal_input_shares_long_gpu`) for both aggregators; `ValueError` here unless both AEADs
    are AES-GCM.  None: the wave per report where the AEAD is AES-GCM and the input share has at
    least `LONG_SEAL_MIN_SHARE` bytes, else the lane.

    `team_chacha` sets the option "hpke_team_chacha" on `vdaf`'s context, with which the wave per
    report takes ChaCha20-Poly1305 too: `long_seal=True` is then allowed for such configs, and
    under `long_seal=None` such a config takes the wave from `LONG_SEAL_MIN_SHARE_CHACHA` bytes
    on.  Without it a ChaCha20-Poly1305 config is sealed a lane per report, as before.

    `team_split` and `team_split_blocks` set the options "hpke_team_split" and
    "hpke_team_split_blocks" on `vdaf`'s context: where a wave per report seals a share, a small
    batch of very long shares gets up to `team_split` waves per report, none with fewer than
    `team_split_blocks` 16-byte blocks.  Like `team_chacha`, either is set only when given: 0 (the
    default) and None leave the context as it is -- one wave per report on a context nobody
    switched, still split on a `vdaf` an earlier batch switched on (`vdaf.set_option(
    "hpke_team_split", 0)` turns it off).  The report bytes never depend on either.

    `p256` sets the option "hpke_gpu_p256" on `vdaf`'s context and admits P-256 configs: such an
    aggregator's encapsulated keys are 65 bytes (`layout`), its ephemeral private keys are drawn
    in [1, n) (`draw_p256_scalars`), and a caller's `sk_es` outside that range raise `HpkeError`.
    The `long_seal` rules do not change: the AEAD decides, the ladders cost the same on both
    paths.  Without it a P-256 config is a `ValueError`, as before."""

    # The shortest input share from which the wave-per-report seal is measured to win at every
    # longer length too: the Sum32 leader share, 1.7x at 4,096 reports; at 1,024 bytes the lane per
    # report is still ahead (DESIGN.md §8b "Seal at the client, a wave per report").  None would
    # keep the lane per report everywhere under long_seal=None.
    LONG_SEAL_MIN_SHARE: Optional[int] = 2576
    # The same rule for a ChaCha20-Poly1305 config under team_chacha=True: the smallest measured
    # length from which the wave per report wins, by more than the two spreads, at every longer
    # measured length.  4,096 shares: 1,024 bytes 1.05 ms against the lane's 1.06 (inside the
    # spreads), 2,576 bytes 1.05 against 1.42, 65,536 bytes 1.45 against 15.12, 134,944 bytes
    # 1.63 against 33.58; 65,536 shares of 48 bytes 5.36 against 1.58 (DESIGN.md §8b
    # "ChaCha20-Poly1305, a wave per report").  None would keep the lane per report.
    LONG_SEAL_MIN_SHARE_CHACHA: Optional[int] = 2576

    def __init__(self, vdaf, task_id: bytes, leader_config: H.HpkeConfig,
                 helper_config: H.HpkeConfig, time_precision: int,
                 long_seal: Optional[bool] = None, team_chacha: bool = False,
                 p256: bool = False, team_split: int = 0,
                 team_split_blocks: Optional[int] = None):
        if len(task_id) != 32:
            raise ValueError("TaskId is 32 bytes")
        if time_precision <= 0:
            raise ValueError("time precision must be positive")
        for c in (leader_config, helper_config):
            if c.kem_id != H.KEM_X25519_HKDF_SHA256 and \
                    not (p256 and c.kem_id == H.KEM_P256_HKDF_SHA256):
                raise ValueError("the GPU seals to DHKEM(X25519, HKDF-SHA256) configs only"
                                 + ("" if p256 else ", or with p256=True to P-256 ones"))
        # per aggregator, the shortest share a wave per report seals under long_seal=None (None:
        # never), or False where the wave does not take the AEAD at all
        floors = [self.LONG_SEAL_MIN_SHARE
                  if c.aead_id in (H.AEAD_AES128GCM, H.AEAD_AES256GCM) else
                  self.LONG_SEAL_MIN_SHARE_CHACHA
                  if team_chacha and c.aead_id == H.AEAD_CHACHA20POLY1305 else False
                  for c in (leader_config, helper_config)]
        if long_seal and any(f is False for f in floors):
            raise ValueError("long_seal=True needs AES-128-GCM or AES-256-GCM configs, or "
                             "ChaCha20-Poly1305 ones with team_chacha=True")
        if team_chacha:
            vdaf.set_option("hpke_team_chacha", 1)
        if p256:
            vdaf.set_option("hpke_gpu_p256", 1)
        if team_split_blocks is not None:
            vdaf.set_option("hpke_team_split_blocks", team_split_blocks)
        if team_split:
            vdaf.set_option("hpke_team_split", team_split)
        s = vdaf.sizes
        # (leader, helper): whether a wave per report seals that aggregator's shares
        self._wave = tuple(
            bool(long_seal) if long_seal is not None else
            (f is not None and f is not False and share >= f)
            for f, share in zip(floors, (s.leader_input_share, s.helper_input_share)))
        self.vdaf, self.task_id = vdaf, bytes(task_id)
        self.leader_config, self.helper_config = leader_config, helper_config
        self.time_precision = int(time_precision)
        self.layout = ReportLayout(s.public_share, s.leader_input_share, s.helper_input_share,
                                   H.enc_len(leader_config.kem_id), H.enc_len(helper_config.kem_id))
        self.report_len = self.layout.report_len
        self._state = None

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None

    def _shard_state(self, n: int):
        if self._state is None or self._state.capacity < n:
            self.close()
            self._state = self.vdaf.new_state(1, n)
        return self._state

    def prepare_reports(self, measurements, report_ids=None, times=None, rand=None, sk_es=None,
                        device_out: bool = False):
        """The batched `prepare_report`: n measurements ((n,) or (n, length) integers, as
        `Prio3Gpu.shard` takes them) -> the (n, report_len) uint8 matrix of their encoded
        Reports (a numpy array; with `device_out` the torch tensor on the GPU it was built in).
        report_ids (n, 16), rand (n, vdaf.random_size()) and sk_es (2, n, 32: the leader's and the
        helper's ephemeral private keys; for a P-256 config big-endian scalars in [1, n)) default
        to os.urandom (`draw_p256_scalars` for a P-256 config), times (n,) seconds to now; times
        are rounded down to the time precision.  Shares, frames and ciphertexts never leave the
        GPU; only the report matrix is copied back."""
        import torch
        v, L = self.vdaf, self.layout
        meas = np.asarray(measurements)
        n = meas.shape[0]
        dev = torch.device("cuda", v.device)

        def rnd(shape):
            return np.frombuffer(os.urandom(int(np.prod(shape))), np.uint8).reshape(shape).copy()

        ids = rnd((n, 16)) if report_ids is None else \
            np.ascontiguousarray(report_ids, np.uint8).reshape(n, 16)
        tm = round_times(np.full(n, int(_time.time())) if times is None else times,
                         self.time_precision)
        rand = rnd((n, v.random_size())) if rand is None else np.asarray(rand, np.uint8)
        if sk_es is None:
            sk = np.stack([draw_p256_scalars(n) if c.kem_id == H.KEM_P256_HKDF_SHA256
                           else rnd((n, 32)) for c in (self.leader_config, self.helper_config)])
        else:
            sk = np.ascontiguousarray(sk_es, np.uint8).reshape(2, n, 32)
        reports = torch.zeros((n, L.report_len), dtype=torch.uint8, device=dev)
        if n == 0:
            return reports if device_out else reports.cpu().numpy()
        d_ids = torch.from_numpy(ids.copy()).to(dev)
        d_tm = torch.from_numpy(tm.astype(np.int64)).to(dev)   # the same 64 bits
        d_meas = torch.from_numpy(np.ascontiguousarray(meas).astype(np.int64)).to(dev)
        d_rand = torch.from_numpy(np.ascontiguousarray(rand)).to(dev)
        d_sk = torch.from_numpy(sk.copy()).to(dev)
        d_pub = torch.empty((n, L.public_share), dtype=torch.uint8, device=dev) \
            if L.public_share else None
        d_lin = torch.empty((n, L.leader_share), dtype=torch.uint8, device=dev)
        d_hin = torch.empty((n, L.helper_share), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)   # the engine works on its own stream
        v.shard(self._shard_state(n), d_ids, d_meas, d_rand, out=(d_pub, d_lin, d_hin))
        L.write_fixed(reports, ids, tm, d_pub, self.leader_config.id, self.helper_config.id)
        torch.cuda.synchronize(dev)
        for which, cfg, role, shares, k in (("leader", self.leader_config, H.ROLE_LEADER, d_lin, 0),
                                            ("helper", self.helper_config, H.ROLE_HELPER, d_hin, 1)):
            encs, payloads = L.columns(reports, which)
            seal = H.seal_input_shares_long_gpu if self._wave[k] else H.seal_input_shares_gpu
            _, _, st = seal(v, self.task_id, cfg, role, d_ids, d_tm, d_pub, shares, d_sk[k], encs,
                            payloads)
            if st[:n].any():
                raise H.HpkeError(f"sealing to the {which} failed for {int((st[:n] != 0).sum())} "
                                  "reports (a public key of small order, or an ephemeral "
                                  "P-256 scalar outside [1, n))")
        d_sk.zero_()
        return reports if device_out else reports.cpu().numpy()
