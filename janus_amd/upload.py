"""The aggregator's side of an upload, batched on the GPU: `Report` bytes in, input-share rows out.

Mirrors the decode-and-decrypt half of `handle_upload_generic` (Janus's
aggregator/src/aggregator.rs:1325-1497) for a whole batch: pick the HPKE key by the ciphertext's
config id (task keys first, the global key of the same id when a task key fails to decrypt),
`hpke::open` the aggregator's encrypted input share under the `InputShareAad`, decode the
`PlaintextInputShare` and keep the share.  The batch is the (n, report_len) uint8 matrix of
`client.ReportLayout` -- what `ClientBatch.prepare_reports` writes -- and the open runs a GPU wave
per report (prio3gpu_open_input_shares: the enc and payload columns are read where they are, the
AAD and the plaintext frame are never built), so a leader's share of a hundred kilobytes is
spread over 64 lanes.  The share rows come out at a pitch that is a multiple of 128 bytes, on the
device for device input: `Prio3Gpu.prepare_init` reads them in place.

The report's time and expiry checks and the datastore write stay with the caller.
"""
from __future__ import annotations

import struct
from typing import Optional, Sequence

import numpy as np

from . import hpke as H
from .client import ENC_LEN, PLAINTEXT_OVERHEAD, ReportLayout

ST_UNKNOWN_CONFIG, ST_DECRYPT, ST_INVALID_MESSAGE = 3, 4, 8
ROW_ALIGN = 128


def _gpu_suite(c: H.HpkeConfig, team_chacha: bool = False, p256: bool = False) -> bool:
    """The suites prio3gpu_open_input_shares takes: X25519 with AES-GCM, with the context's
    "hpke_team_chacha" option (`team_chacha`) ChaCha20-Poly1305 too, and with its "hpke_gpu_p256"
    option (`p256`) the same under P-256."""
    aeads = (H.AEAD_AES128GCM, H.AEAD_AES256GCM) + \
        ((H.AEAD_CHACHA20POLY1305,) if team_chacha else ())
    kems = (H.KEM_X25519_HKDF_SHA256,) + ((H.KEM_P256_HKDF_SHA256,) if p256 else ())
    return c.kem_id in kems and c.kdf_id in (1, 2, 3) and c.aead_id in aeads


class UploadBatch:
    """The batched upload open of one task: `vdaf` a `Prio3Gpu`, the task's and the global
    `HpkeKeypair`s, and the role this aggregator plays (the leader by default: it is whom clients
    upload to).  `team_chacha` sets the option "hpke_team_chacha" on `vdaf`'s context: key groups
    under ChaCha20-Poly1305 are then opened a GPU wave per report like the AES-GCM ones, not one
    by one on the host.  `p256` sets the option "hpke_gpu_p256": key groups under DHKEM(P-256,
    HKDF-SHA256) are then opened on the GPU too, and the report matrix has this aggregator's
    encapsulated keys at the length of its first key's KEM (65 bytes for P-256) and the other
    aggregator's at `peer_enc` bytes (32, or 65 when that one's key is P-256) -- the layout
    `ClientBatch(p256=True)` writes.  Without it the layout and the routing are unchanged: a
    P-256 key group is opened on the host.  `team_split` and `team_split_blocks` set the options
    "hpke_team_split" and "hpke_team_split_blocks": a small batch of very long shares is opened
    with up to `team_split` waves per report, none with fewer than `team_split_blocks` 16-byte
    blocks.  Like `team_chacha`, either is set only when given: 0 (the default) and None leave the
    context as it is -- one wave per report on a context nobody switched, still split on a `vdaf`
    an earlier batch switched on (`vdaf.set_option("hpke_team_split", 0)` turns it off).  The
    opened rows and statuses never depend on either."""

    def __init__(self, vdaf, task_id: bytes, task_keys: Sequence[H.HpkeKeypair],
                 global_keys: Sequence[H.HpkeKeypair] = (), role: int = H.ROLE_LEADER,
                 team_chacha: bool = False, p256: bool = False, peer_enc: int = ENC_LEN,
                 team_split: int = 0, team_split_blocks: Optional[int] = None):
        if len(task_id) != 32:
            raise ValueError("TaskId is 32 bytes")
        if role not in (H.ROLE_LEADER, H.ROLE_HELPER):
            raise ValueError("an input share is sealed to the leader or to the helper")
        self.team_chacha = bool(team_chacha)
        if self.team_chacha:
            vdaf.set_option("hpke_team_chacha", 1)
        self.p256 = bool(p256)
        if self.p256:
            vdaf.set_option("hpke_gpu_p256", 1)
        if team_split_blocks is not None:
            vdaf.set_option("hpke_team_split_blocks", team_split_blocks)
        if team_split:
            vdaf.set_option("hpke_team_split", team_split)
        self.vdaf, self.task_id, self.role = vdaf, bytes(task_id), role
        self.task_keys, self.global_keys = {}, {}
        for table, kps in ((self.task_keys, task_keys), (self.global_keys, global_keys)):
            for kp in kps:
                table.setdefault(kp.config.id, kp)   # the first key of an id wins
        s = vdaf.sizes
        own_enc = ENC_LEN
        if self.p256:   # this batch's enc length: the KEM of the first key, task keys first
            for kp in list(task_keys) + list(global_keys):
                own_enc = H.enc_len(kp.config.kem_id)
                break
        encs = (own_enc, int(peer_enc)) if role == H.ROLE_LEADER else (int(peer_enc), own_enc)
        self.layout = ReportLayout(s.public_share, s.leader_input_share, s.helper_input_share,
                                   *encs)
        self.which = "leader" if role == H.ROLE_LEADER else "helper"
        self.share_len = s.leader_input_share if role == H.ROLE_LEADER else s.helper_input_share
        self.pitch = max(ROW_ALIGN, -(-self.share_len // ROW_ALIGN) * ROW_ALIGN)
        self.info = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, role)

    # -- one key group on the GPU ------------------------------------------------------------------
    def _open_group(self, kp, reports, idx, ids, times, rows, status):
        L, n = self.layout, reports.shape[0]
        dev = not isinstance(reports, np.ndarray)
        every = len(idx) == n
        if dev:
            import torch
            sel = None if every else torch.from_numpy(idx).to(reports.device)
            sub = reports if every else reports[sel]
            out = rows[:, :self.share_len] if every else \
                torch.zeros((len(idx), self.pitch), dtype=torch.uint8,
                            device=reports.device)[:, :self.share_len]
            d_ids = torch.from_numpy(ids[idx].copy()).to(reports.device)
            d_tm = torch.from_numpy(times[idx].astype(np.int64)).to(reports.device)
            pub = sub[:, L.o_public:L.o_public + L.public_share].contiguous() \
                if L.public_share else None
            torch.cuda.synchronize(reports.device)   # the engine works on its own stream
        else:
            sub = reports if every else reports[idx]
            out = rows[:, :self.share_len] if every else \
                np.zeros((len(idx), self.pitch), np.uint8)[:, :self.share_len]
            d_ids, d_tm = ids[idx].copy(), times[idx].copy()
            pub = np.ascontiguousarray(sub[:, L.o_public:L.o_public + L.public_share]) \
                if L.public_share else None
        encs, payloads = L.columns(sub, self.which)
        st = np.zeros(len(idx), np.uint8)
        H.open_input_shares_gpu(self.vdaf, self.task_id, kp, self.role, d_ids, d_tm, pub, encs,
                                payloads, out, st)
        if not every:
            rows[sel if dev else idx, :self.share_len] = out
        status[idx] = st

    # -- one report on the host --------------------------------------------------------------------
    def _open_host(self, kp, report: bytes, time: int) -> Optional[bytes]:
        """The share of one report opened by `hpke.open_` under kp; None for a decryption
        failure, `ValueError` for a plaintext that is not an extension-free share of the VDAF's
        length (the caller's status 8)."""
        L = self.layout
        oe, op, pl, ne = ((L.o_leader_enc, L.o_leader_payload, L.leader_payload, L.leader_enc)
                          if self.which == "leader" else
                          (L.o_helper_enc, L.o_helper_payload, L.helper_payload, L.helper_enc))
        aad = H.input_share_aad(self.task_id, report[:16], time,
                                report[L.o_public:L.o_public + L.public_share])
        try:
            pt = H.open_(kp, self.info, report[oe:oe + ne], report[op:op + pl], aad)
        except (H.HpkeError, ValueError):
            return None
        if pt[:PLAINTEXT_OVERHEAD] != b"\0\0" + struct.pack(">I", self.share_len) or \
                len(pt) != PLAINTEXT_OVERHEAD + self.share_len:
            raise ValueError("not an extension-free PlaintextInputShare of this length")
        return pt[PLAINTEXT_OVERHEAD:]

    def _host_rows(self, kp_of, reports, idx, times, rows, status):
        """Reports idx opened one by one on the host, each under kp_of(i)."""
        if len(idx) == 0:
            return
        dev = not isinstance(reports, np.ndarray)
        if dev:
            import torch
            sel = torch.from_numpy(idx).to(reports.device)
            host = reports[sel].cpu().numpy()
        else:
            host = reports[idx]
        got = np.zeros((len(idx), self.share_len), np.uint8)
        for j, i in enumerate(idx):
            try:
                share = self._open_host(kp_of(i), host[j].tobytes(), int(times[i]))
            except ValueError:
                status[i] = ST_INVALID_MESSAGE
                continue
            if share is None:
                status[i] = ST_DECRYPT
            else:
                status[i] = 0
                got[j] = np.frombuffer(share, np.uint8)
        if dev:
            rows[sel, :self.share_len] = torch.from_numpy(got).to(reports.device)
        else:
            rows[idx, :self.share_len] = got

    def open_reports(self, reports):
        """reports: the (n, report_len) uint8 matrix of n encoded Reports, a numpy array or a
        device tensor.  -> (shares, status): shares an (n, share_len) view of rows `pitch` bytes
        apart (a multiple of 128; numpy for numpy input, a device tensor for device input --
        what `Prio3Gpu.prepare_init` takes as input shares), status (n,) uint8: 0, 3 for a config
        id no task or global key has, 4 for a share that does not decrypt, 8 for one that
        decrypts to something other than an extension-free share of the VDAF's length.  A report
        with a non-zero status has a zero row."""
        L = self.layout
        dev = not isinstance(reports, np.ndarray)
        n = int(reports.shape[0])
        if tuple(reports.shape) != (n, L.report_len):
            raise ValueError(f"expected an (n, {L.report_len}) uint8 report matrix")
        if dev:
            import torch
            rows = torch.zeros((n, self.pitch), dtype=torch.uint8, device=reports.device)
            head = reports[:, :24].cpu().numpy()
            cfg = reports[:, L.o_leader if self.which == "leader" else L.o_helper].cpu().numpy()
        else:
            rows = np.zeros((n, self.pitch), np.uint8)
            head = reports[:, :24]
            cfg = reports[:, L.o_leader if self.which == "leader" else L.o_helper]
        status = np.zeros(n, np.uint8)
        if n == 0:
            return rows[:, :self.share_len], status
        ids = np.ascontiguousarray(head[:, :16])
        times = np.ascontiguousarray(head[:, 16:24]).view(">u8").reshape(n).astype(np.uint64)
        first = {}
        for cid in np.unique(cfg):
            idx = np.flatnonzero(cfg == cid)
            kp = self.task_keys.get(int(cid)) or self.global_keys.get(int(cid))
            first[int(cid)] = kp
            if kp is None:
                status[idx] = ST_UNKNOWN_CONFIG
            elif _gpu_suite(kp.config, self.team_chacha, self.p256) and \
                    H.enc_len(kp.config.kem_id) == (L.leader_enc if self.which == "leader"
                                                    else L.helper_enc):
                self._open_group(kp, reports, idx, ids, times, rows, status)
            else:
                self._host_rows(lambda i, kp=kp: kp, reports, idx, times, rows, status)
        # a failed task-key open gets the global key of the same id as a second trial
        retry = np.array([i for i in np.flatnonzero(status == ST_DECRYPT)
                          if int(cfg[i]) in self.task_keys and int(cfg[i]) in self.global_keys],
                         dtype=np.int64)
        self._host_rows(lambda i: self.global_keys[int(cfg[i])], reports, retry, times, rows,
                        status)
        return rows[:, :self.share_len], status
