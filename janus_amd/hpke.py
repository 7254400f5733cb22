"""HPKE for the aggregate-init path, host side: the Python mirror of Janus's
`core/src/hpke.rs` over the native RFC 9180 implementation in libprio3gpu.so
(janus_amd/csrc/hpke.cpp; C ABI include/prio3gpu.h).

  Label / HpkeApplicationInfo        core/src/hpke.rs:44-77
  seal / open                        core/src/hpke.rs:158-202
  generate_hpke_config_and_private_key   core/src/hpke.rs:204-231
  HpkeKeypair                        core/src/hpke.rs:233-255
  open_report_shares                 the helper's per-report open loop, batched over host threads
                                     (aggregator/src/aggregator.rs:1634-1700)
  seal_batch_gpu / seal_input_shares_gpu   the client's per-share seal (client/src/lib.rs:228-251),
                                     batched on the GPU (janus_amd/csrc/hpke_seal_gpu.h)
  open_long_batch_gpu / open_input_shares_gpu   the leader's open at upload
                                     (aggregator.rs:1325-1497), a GPU wave per report
                                     (janus_amd/csrc/hpke_open_team.h)

Errors: `HpkeError` where hpke::open / hpke::seal return `Error::Hpke`, `ValueError` for an
unsupported suite (`Error::InvalidConfiguration`).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._lib import lib

# HpkeKemId / HpkeKdfId / HpkeAeadId (messages/src/lib.rs)
KEM_X25519_HKDF_SHA256, KEM_P256_HKDF_SHA256 = 0x20, 0x10
KDF_HKDF_SHA256, KDF_HKDF_SHA384, KDF_HKDF_SHA512 = 1, 2, 3
AEAD_AES128GCM, AEAD_AES256GCM, AEAD_CHACHA20POLY1305 = 1, 2, 3
# Role (messages/src/lib.rs:495-500)
ROLE_COLLECTOR, ROLE_CLIENT, ROLE_LEADER, ROLE_HELPER = 0, 1, 2, 3

_E_HPKE, _E_UNSUPPORTED, _E_CAPACITY = -5, -6, -4


class HpkeError(Exception):
    pass


class Label:
    INPUT_SHARE = b"dap-07 input share"
    AGGREGATE_SHARE = b"dap-07 aggregate share"


def application_info(label: bytes, sender_role: int, recipient_role: int) -> bytes:
    """HpkeApplicationInfo::new (core/src/hpke.rs:64-77)."""
    return bytes(label) + bytes([sender_role, recipient_role])


@dataclass(frozen=True)
class HpkeConfig:
    id: int
    kem_id: int
    kdf_id: int
    aead_id: int
    public_key: bytes


@dataclass(frozen=True)
class HpkeKeypair:
    config: HpkeConfig
    private_key: bytes


def enc_len(kem_id: int) -> int:
    """Nenc of a KEM (RFC 9180 §7.1): 65 for DHKEM(P-256, HKDF-SHA256), 32 for X25519."""
    return 65 if kem_id == KEM_P256_HKDF_SHA256 else 32


def _buf(b: bytes):
    return ctypes.c_char_p(bytes(b)) if b else None


def _rc(rc: int, what: str) -> None:
    if rc == _E_UNSUPPORTED:
        raise ValueError(f"{what}: unsupported HPKE suite")
    if rc == _E_HPKE:
        raise HpkeError(f"{what} failed")
    if rc != 0:
        raise RuntimeError(f"{what}: error {rc}")


def public_key(kem_id: int, private_key: bytes) -> bytes:
    out = ctypes.create_string_buffer(65)
    ln = ctypes.c_size_t()
    _rc(lib().prio3gpu_hpke_public_key(kem_id, _buf(private_key), len(private_key), out, 65,
                                       ctypes.byref(ln)), "public key")
    return out.raw[:ln.value]


def generate_hpke_config_and_private_key(config_id: int, kem_id: int = KEM_X25519_HKDF_SHA256,
                                         kdf_id: int = KDF_HKDF_SHA256,
                                         aead_id: int = AEAD_AES128GCM) -> HpkeKeypair:
    for _ in range(64):  # P-256: rejection-sample a scalar in [1, n)
        sk = os.urandom(32)
        try:
            pk = public_key(kem_id, sk)
        except HpkeError:
            continue
        return HpkeKeypair(HpkeConfig(config_id, kem_id, kdf_id, aead_id, pk), sk)
    raise HpkeError("key generation failed")


def seal(config: HpkeConfig, info: bytes, plaintext: bytes, aad: bytes,
         ephemeral_private_key: Optional[bytes] = None):
    """-> (config id, encapsulated key, payload) = HpkeCiphertext fields."""
    enc = ctypes.create_string_buffer(65)
    ct = ctypes.create_string_buffer(len(plaintext) + 16)
    el, cl = ctypes.c_size_t(), ctypes.c_size_t()
    ske = ephemeral_private_key
    _rc(lib().prio3gpu_hpke_seal(config.kem_id, config.kdf_id, config.aead_id,
                                 _buf(config.public_key), len(config.public_key), _buf(ske),
                                 len(ske) if ske else 0, _buf(info), len(info), _buf(aad),
                                 len(aad), _buf(plaintext), len(plaintext), enc, 65,
                                 ctypes.byref(el), ct, len(ct), ctypes.byref(cl)), "HPKE seal")
    return config.id, enc.raw[:el.value], ct.raw[:cl.value]


def open_(keypair: HpkeKeypair, info: bytes, enc: bytes, payload: bytes, aad: bytes) -> bytes:
    c = keypair.config
    n = max(0, len(payload) - 16)
    pt = ctypes.create_string_buffer(max(1, n))
    ln = ctypes.c_size_t()
    _rc(lib().prio3gpu_hpke_open(c.kem_id, c.kdf_id, c.aead_id, _buf(keypair.private_key),
                                 len(keypair.private_key), _buf(c.public_key), len(c.public_key),
                                 _buf(enc), len(enc), _buf(info), len(info), _buf(aad), len(aad),
                                 # an empty payload is a decryption failure, not a null argument
                                 ctypes.c_char_p(bytes(payload)), len(payload), pt, n,
                                 ctypes.byref(ln)),
        "HPKE open")
    return pt.raw[:ln.value]


class _Keypair(ctypes.Structure):
    _fields_ = [("config_id", ctypes.c_uint8), ("kem_id", ctypes.c_uint16),
                ("kdf_id", ctypes.c_uint16), ("aead_id", ctypes.c_uint16),
                ("public_key", ctypes.c_void_p), ("public_key_len", ctypes.c_uint32),
                ("private_key", ctypes.c_void_p), ("private_key_len", ctypes.c_uint32)]


def _keypairs(kps: Sequence[HpkeKeypair]):
    arr = (_Keypair * max(1, len(kps)))()
    keep = []
    for i, kp in enumerate(kps):
        pk = ctypes.create_string_buffer(kp.config.public_key, len(kp.config.public_key))
        sk = ctypes.create_string_buffer(kp.private_key, len(kp.private_key))
        keep += [pk, sk]
        c = kp.config
        arr[i] = _Keypair(c.id, c.kem_id, c.kdf_id, c.aead_id, ctypes.addressof(pk), len(pk.raw),
                          ctypes.addressof(sk), len(sk.raw))
    return arr, keep


def input_share_aad(task_id: bytes, report_id: bytes, time: int, public_share: bytes) -> bytes:
    """InputShareAad encoding (messages/src/lib.rs:1790-1827)."""
    return (bytes(task_id) + bytes(report_id) + int(time).to_bytes(8, "big")
            + len(public_share).to_bytes(4, "big") + bytes(public_share))


def _ctx_handle(gpu):
    """A `Prio3Gpu` (its context) or a raw prio3gpu_ctx handle."""
    return getattr(gpu, "_ctx", gpu)


def _ptr(x, dtype):
    """Host numpy array -> (pointer, keep-alive); an int / c_void_p is a device pointer."""
    if isinstance(x, (int, ctypes.c_void_p)):
        return x, None
    a = np.ascontiguousarray(x, dtype)
    return a.ctypes.data, a


def _dev_ptr(x, dtype):
    """_ptr that also takes a torch tensor (host or device): its pointer, the tensor kept alive."""
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensors must be contiguous")
        return x.data_ptr(), x
    return _ptr(x, dtype)


def _open_batch_gpu(entry: str, what: str, gpu, keypair: HpkeKeypair, info: bytes, encs, aads,
                    aad_offsets, cts, ct_offsets, pts, pt_offsets, status, n):
    """`open_batch_gpu` / `open_long_batch_gpu` through the library's entry point `entry`."""
    c = keypair.config
    if n is None:
        n = len(np.asarray(ct_offsets)) - 1
    if pt_offsets is None:
        lens = np.diff(np.asarray(ct_offsets, np.uint64).astype(np.int64)) - 16
        pt_offsets = np.concatenate([[0], np.cumsum(np.maximum(lens, 0))]).astype(np.uint64)
    if pts is None:
        pts = np.zeros(max(1, int(np.asarray(pt_offsets)[-1])), np.uint8)
    if status is None:
        status = np.zeros(max(1, n), np.uint8)
    keep, args = [], []
    for x, dt in ((encs, np.uint8), (aads, np.uint8), (aad_offsets, np.uint64), (cts, np.uint8),
                  (ct_offsets, np.uint64), (pts, np.uint8), (pt_offsets, np.uint64),
                  (status, np.uint8)):
        p, k = _dev_ptr(x, dt)
        args.append(p)
        keep.append(k)
    for out, k in ((pts, keep[5]), (status, keep[7])):  # outputs must be written in place
        assert k is None or k is out, "pts / status must be contiguous uint8 arrays"
    _rc(getattr(lib(), entry)(_ctx_handle(gpu), c.kem_id, c.kdf_id, c.aead_id,
                              _buf(keypair.private_key), len(keypair.private_key),
                              _buf(c.public_key), len(c.public_key), _buf(info), len(info), n,
                              *args), what)
    del keep
    return pts, pt_offsets, status


def open_batch_gpu(gpu, keypair: HpkeKeypair, info: bytes, encs, aads, aad_offsets, cts,
                   ct_offsets, pts=None, pt_offsets=None, status=None, n: Optional[int] = None):
    """n HPKE opens under ONE keypair on the GPU (prio3gpu_hpke_open_batch).  By default only
    X25519 / HKDF-SHA256 / AES-128-GCM; after `gpu.set_option("hpke_gpu_suites", 1)` every X25519
    suite (KDF HKDF-SHA256 / -SHA384 / -SHA512 x AEAD AES-128-GCM / AES-256-GCM /
    ChaCha20-Poly1305); after `gpu.set_option("hpke_gpu_p256", 1)` the same choice under
    DHKEM(P-256, HKDF-SHA256).  `ValueError` for any other suite, nothing launched.

    `gpu` is a `Prio3Gpu` or a context handle.  Report i: enc = encs[Nenc i : Nenc i + Nenc] with
    Nenc = 32 for X25519 and 65 for P-256 (the stride follows the keypair's KEM), aad =
    aads[aad_offsets[i] : aad_offsets[i+1]], ciphertext || tag = cts[ct_offsets[i] :
    ct_offsets[i+1]].  Buffers are numpy arrays (host), integer device pointers (then `n`, `pts`,
    `pt_offsets` and `status` must be given) or, as `open_long_batch_gpu` has always taken them,
    contiguous torch tensors (host or device).  By default plaintext i has the ciphertext's
    length - 16 and the plaintexts are packed.
    -> (plaintexts, pt_offsets, status); a failed open has status 4 and zeros."""
    return _open_batch_gpu("prio3gpu_hpke_open_batch", "HPKE GPU open", gpu, keypair, info, encs,
                           aads, aad_offsets, cts, ct_offsets, pts, pt_offsets, status, n)


def _seal_batch_gpu(entry: str, gpu, config: HpkeConfig, info: bytes, sk_es, aads, aad_offsets,
                    pts, pt_offsets, status, encs, cts, ct_offsets, n):
    """`seal_batch_gpu` / `seal_long_batch_gpu` through the library's entry point `entry`."""
    if n is None:
        n = len(np.asarray(pt_offsets)) - 1
    if ct_offsets is None:
        lens = np.diff(np.asarray(pt_offsets, np.uint64).astype(np.int64)) + 16
        ct_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    if cts is None:
        cts = np.zeros(max(1, int(np.asarray(ct_offsets)[-1])), np.uint8)
    if encs is None:
        encs = np.zeros(max(1, n) * enc_len(config.kem_id), np.uint8)
    if status is None:
        status = np.zeros(max(1, n), np.uint8)
    keep, args = [], []
    for x, dt in ((sk_es, np.uint8), (aads, np.uint8), (aad_offsets, np.uint64), (pts, np.uint8),
                  (pt_offsets, np.uint64), (encs, np.uint8), (cts, np.uint8),
                  (ct_offsets, np.uint64), (status, np.uint8)):
        p, k = _dev_ptr(x, dt)
        args.append(p)
        keep.append(k)
    for out, k in ((encs, keep[5]), (cts, keep[6]), (status, keep[8])):  # written in place
        assert k is None or k is out, "encs / cts / status must be contiguous uint8 arrays"
    _rc(getattr(lib(), entry)(_ctx_handle(gpu), config.kem_id, config.kdf_id, config.aead_id,
                              _buf(config.public_key), len(config.public_key), _buf(info),
                              len(info), n, *args), "HPKE GPU seal")
    del keep
    return encs, cts, ct_offsets, status


def seal_batch_gpu(gpu, config: HpkeConfig, info: bytes, sk_es, aads, aad_offsets, pts,
                   pt_offsets, status=None, encs=None, cts=None, ct_offsets=None,
                   n: Optional[int] = None):
    """n HPKE seals to ONE recipient config on the GPU (prio3gpu_hpke_seal_batch), each under its
    own ephemeral private key: any DHKEM(X25519, HKDF-SHA256) suite (KDF HKDF-SHA256 / -SHA384 /
    -SHA512 x AEAD AES-128-GCM / AES-256-GCM / ChaCha20-Poly1305), no option needed; after
    `gpu.set_option("hpke_gpu_p256", 1)` the same choice under DHKEM(P-256, HKDF-SHA256).
    `ValueError` for any other suite (P-256 without the option), nothing launched; `HpkeError`
    for a P-256 public key that is not a point.

    `gpu` is a `Prio3Gpu` or a context handle.  Report i: ephemeral key = sk_es[32 i : 32 i + 32]
    (for P-256 a big-endian scalar; one outside [1, n) is that report's failure),
    aad = aads[aad_offsets[i] : aad_offsets[i+1]], plaintext = pts[pt_offsets[i] :
    pt_offsets[i+1]].  Buffers are numpy arrays (host), torch tensors (host or device) or integer
    device pointers (then `n`, `encs`, `cts`, `ct_offsets` and `status` must be given).  By
    default ciphertext i has the plaintext's length + 16 and the ciphertexts are packed.
    -> (encs, cts, ct_offsets, status): enc i = encs[Nenc i : Nenc i + Nenc] with Nenc = 32 for
    X25519 and 65 for P-256 (`enc_len`), ciphertext || tag i = cts[ct_offsets[i] :
    ct_offsets[i+1]] -- the bytes `seal` gives with the same ephemeral key.  A report that is not
    sealed (status non-zero on entry, a public key of small order, an invalid P-256 scalar, a slot
    that is too short) has zeros in both and, unless it was skipped, status 4."""
    return _seal_batch_gpu("prio3gpu_hpke_seal_batch", gpu, config, info, sk_es, aads,
                           aad_offsets, pts, pt_offsets, status, encs, cts, ct_offsets, n)


def seal_long_batch_gpu(gpu, config: HpkeConfig, info: bytes, sk_es, aads, aad_offsets, pts,
                        pt_offsets, status=None, encs=None, cts=None, ct_offsets=None,
                        n: Optional[int] = None):
    """`seal_batch_gpu` with one GPU wave per report instead of one lane
    (prio3gpu_hpke_seal_long_batch): for plaintexts of many kilobytes, the leader's input shares.
    DHKEM(X25519, HKDF-SHA256) with any KDF and AES-128-GCM / AES-256-GCM, no option needed, and
    after `gpu.set_option("hpke_team_chacha", 1)` ChaCha20-Poly1305 too; after
    `gpu.set_option("hpke_gpu_p256", 1)` the same under DHKEM(P-256, HKDF-SHA256).  `ValueError`
    for any other suite (P-256 or ChaCha20-Poly1305 without its option), nothing launched.  Same
    arguments and the same bytes, offsets and statuses.  -> (encs, cts, ct_offsets, status)."""
    return _seal_batch_gpu("prio3gpu_hpke_seal_long_batch", gpu, config, info, sk_es, aads,
                           aad_offsets, pts, pt_offsets, status, encs, cts, ct_offsets, n)


def _rows(x, n: int, width: int, what: str):
    """(pointer, row pitch, keep-alive) of n rows of `width` bytes: a 2-D uint8 numpy array or
    torch tensor whose rows are contiguous inside and `pitch` >= width bytes apart (a column slice
    of a wider buffer keeps its pitch), or an (integer device pointer, pitch) pair."""
    if isinstance(x, tuple):
        return int(x[0]), int(x[1]), None
    if hasattr(x, "data_ptr"):
        if tuple(x.shape) != (n, width) or x.element_size() != 1 or (width and x.stride(1) != 1):
            raise ValueError(f"{what}: expected a ({n}, {width}) uint8 tensor with contiguous rows")
        return x.data_ptr(), (x.stride(0) if n > 1 else width), x
    a = np.asarray(x)
    if a.shape != (n, width) or a.dtype != np.uint8 or (width and a.strides[1] != 1):
        raise ValueError(f"{what}: expected a ({n}, {width}) uint8 array with contiguous rows")
    return a.ctypes.data, (a.strides[0] if n > 1 else width), a


def _seal_input_shares_gpu(entry: str, gpu, task_id: bytes, config: HpkeConfig,
                           recipient_role: int, report_ids, times, public_shares, input_shares,
                           sk_es, out_encs, out_payloads, status):
    """`seal_input_shares_gpu` / `seal_input_shares_long_gpu` through the entry point `entry`."""
    tid = np.frombuffer(bytes(task_id), np.uint8).copy()
    if tid.size != 32:
        raise ValueError("TaskId is 32 bytes")
    n, slen = int(input_shares.shape[0]), int(input_shares.shape[1])
    plen = 6 + slen + 16
    nenc = enc_len(config.kem_id)
    if out_encs is None:
        out_encs = np.zeros((n, nenc), np.uint8)
    if out_payloads is None:
        out_payloads = np.zeros((n, plen), np.uint8)
    if status is None:
        status = np.zeros(max(1, n), np.uint8)
    pslen = 0 if public_shares is None else int(public_shares.shape[1])
    p_sh, sh_pitch, k0 = _rows(input_shares, n, slen, "input shares")
    p_enc, enc_pitch, k1 = _rows(out_encs, n, nenc, "out_encs")
    p_pay, pay_pitch, k2 = _rows(out_payloads, n, plen, "out_payloads")
    assert (k1 is out_encs or k1 is None) and (k2 is out_payloads or k2 is None)
    p_rid, k3 = _dev_ptr(report_ids, np.uint8)
    p_tm, k4 = _dev_ptr(times, np.uint64)
    p_pub, k5 = _dev_ptr(public_shares, np.uint8) if pslen else (None, None)
    p_sk, k6 = _dev_ptr(sk_es, np.uint8)
    p_st, k7 = _dev_ptr(status, np.uint8)
    assert k7 is None or k7 is status, "status must be a contiguous uint8 array"
    _rc(getattr(lib(), entry)(_ctx_handle(gpu), tid.ctypes.data, config.kem_id, config.kdf_id,
                              config.aead_id, _buf(config.public_key), len(config.public_key),
                              recipient_role, n, p_rid, p_tm, p_pub, pslen, p_sh, slen, sh_pitch,
                              p_sk, p_enc, enc_pitch, p_pay, pay_pitch, p_st),
        "seal input shares (GPU)")
    del k0, k1, k2, k3, k4, k5, k6, k7
    return out_encs, out_payloads, status


def seal_input_shares_gpu(gpu, task_id: bytes, config: HpkeConfig, recipient_role: int,
                          report_ids, times, public_shares, input_shares, sk_es, out_encs=None,
                          out_payloads=None, status=None):
    """Seal n Prio3 input shares to one aggregator on the GPU (prio3gpu_seal_input_shares): for
    report i, `seal(config, application_info(INPUT_SHARE, CLIENT, recipient_role),
    PlaintextInputShare(no extensions, input_shares[i]), input_share_aad(task_id, report_ids[i],
    times[i], public_shares[i]), sk_es[i])` -- neither frame is built in memory.

    report_ids (n, 16), public_shares (n, public_share_len) or None, sk_es (n, 32): uint8 numpy
    arrays or torch tensors, packed; times (n,) uint64; input_shares (n, len) uint8 whose rows may
    be a column slice of a wider buffer, like out_encs (n, Nenc: 32, or 65 for a P-256 config
    with the context's "hpke_gpu_p256" option) and out_payloads (n, 6 + len + 16):
    only those columns are written (host or device; e.g. the columns of a fixed-stride Report
    buffer; allocated as numpy arrays by default).  -> (out_encs, out_payloads, status); a report
    that is not sealed has zeros in both columns and, unless skipped on entry, status 4."""
    return _seal_input_shares_gpu("prio3gpu_seal_input_shares", gpu, task_id, config,
                                  recipient_role, report_ids, times, public_shares, input_shares,
                                  sk_es, out_encs, out_payloads, status)


def seal_input_shares_long_gpu(gpu, task_id: bytes, config: HpkeConfig, recipient_role: int,
                               report_ids, times, public_shares, input_shares, sk_es,
                               out_encs=None, out_payloads=None, status=None):
    """`seal_input_shares_gpu` with one GPU wave per report instead of one lane
    (prio3gpu_seal_input_shares_long): for the leader's input shares of many kilobytes.  Suites as
    `seal_long_batch_gpu` (ChaCha20-Poly1305 with "hpke_team_chacha"), `ValueError` otherwise; the same arguments, the same bytes in the same
    columns (at any alignment) and the same statuses.  -> (out_encs, out_payloads, status)."""
    return _seal_input_shares_gpu("prio3gpu_seal_input_shares_long", gpu, task_id, config,
                                  recipient_role, report_ids, times, public_shares, input_shares,
                                  sk_es, out_encs, out_payloads, status)


def open_long_batch_gpu(gpu, keypair: HpkeKeypair, info: bytes, encs, aads, aad_offsets, cts,
                        ct_offsets, pts=None, pt_offsets=None, status=None,
                        n: Optional[int] = None):
    """`open_batch_gpu` with one GPU wave per report instead of one lane
    (prio3gpu_hpke_open_long_batch): for ciphertexts of many kilobytes, the leader's input shares
    at upload.  DHKEM(X25519, HKDF-SHA256) with any KDF and AES-128-GCM / AES-256-GCM, no option
    needed, and after `gpu.set_option("hpke_team_chacha", 1)` ChaCha20-Poly1305 too; after
    `gpu.set_option("hpke_gpu_p256", 1)` the same under DHKEM(P-256, HKDF-SHA256), with encs 65
    bytes apart.  `ValueError` for any other suite (P-256 or ChaCha20-Poly1305 without its
    option), nothing launched; `HpkeError` for a P-256 keypair that is none.  Same
    arguments, plaintexts and statuses; buffers are numpy arrays (host), torch tensors (host or
    device) or integer device pointers (then `n`, `pts`, `pt_offsets` and `status` must be given).
    -> (plaintexts, pt_offsets, status); a failed open has status 4 and zeros."""
    return _open_batch_gpu("prio3gpu_hpke_open_long_batch", "HPKE GPU open (long)", gpu, keypair,
                           info, encs, aads, aad_offsets, cts, ct_offsets, pts, pt_offsets,
                           status, n)


def open_input_shares_gpu(gpu, task_id: bytes, keypair: HpkeKeypair, recipient_role: int,
                          report_ids, times, public_shares, encs, payloads, out_shares=None,
                          status=None):
    """Open n Prio3 input shares sealed to one aggregator on the GPU, a wave per report
    (prio3gpu_open_input_shares), the mirror of `seal_input_shares_gpu`: report i's share is the
    payload of `open_(keypair, application_info(INPUT_SHARE, CLIENT, recipient_role), encs[i],
    payloads[i], input_share_aad(task_id, report_ids[i], times[i], public_shares[i]))`, which
    must be the PlaintextInputShare with no extensions -- neither frame is built in memory.

    report_ids (n, 16), public_shares (n, public_share_len) or None: uint8 numpy arrays or torch
    tensors, packed; times (n,) uint64; encs (n, Nenc: 32, or 65 under a P-256 keypair with the
    context's "hpke_gpu_p256" option) and payloads (n, 6 + len + 16) uint8 whose
    rows may be column slices of a wider buffer (host or device; e.g. the columns of a
    fixed-stride Report matrix), like out_shares (n, len): only those columns are written (a numpy
    array by default).  -> (out_shares, status); status 4 and a zero row for a failed open, 8 and
    a zero row for an authentic plaintext that is not an extension-free share of this length.
    Suites as `open_long_batch_gpu` (ChaCha20-Poly1305 with "hpke_team_chacha"); `ValueError`
    otherwise."""
    tid = np.frombuffer(bytes(task_id), np.uint8).copy()
    if tid.size != 32:
        raise ValueError("TaskId is 32 bytes")
    c = keypair.config
    n, plen = int(payloads.shape[0]), int(payloads.shape[1])
    slen = plen - 6 - 16
    if slen < 0:
        raise ValueError("a payload holds at least the 6-byte header and the 16-byte tag")
    if out_shares is None:
        out_shares = np.zeros((n, slen), np.uint8)
    if status is None:
        status = np.zeros(max(1, n), np.uint8)
    pslen = 0 if public_shares is None else int(public_shares.shape[1])
    p_enc, enc_pitch, k0 = _rows(encs, n, enc_len(c.kem_id), "encs")
    p_pay, pay_pitch, k1 = _rows(payloads, n, plen, "payloads")
    p_out, out_pitch, k2 = _rows(out_shares, n, slen, "out_shares")
    assert k2 is out_shares or k2 is None
    p_rid, k3 = _dev_ptr(report_ids, np.uint8)
    p_tm, k4 = _dev_ptr(times, np.uint64)
    p_pub, k5 = _dev_ptr(public_shares, np.uint8) if pslen else (None, None)
    p_st, k6 = _dev_ptr(status, np.uint8)
    assert k6 is None or k6 is status, "status must be a contiguous uint8 array"
    _rc(lib().prio3gpu_open_input_shares(_ctx_handle(gpu), tid.ctypes.data, c.kem_id, c.kdf_id,
                                         c.aead_id, _buf(keypair.private_key),
                                         len(keypair.private_key), _buf(c.public_key),
                                         len(c.public_key), recipient_role, n, p_rid, p_tm, p_pub,
                                         pslen, p_enc, enc_pitch, p_pay, pay_pitch, slen, p_out,
                                         out_pitch, p_st), "open input shares (GPU)")
    del k0, k1, k2, k3, k4, k5, k6
    return out_shares, status


def open_report_shares(task_id: bytes, req, task_keys: Sequence[HpkeKeypair],
                       global_keys: Sequence[HpkeKeypair] = (),
                       status: Optional[np.ndarray] = None, threads: int = 0,
                       recipient_role: int = ROLE_HELPER, gpu=None):
    """Open every encrypted input share of a decoded AggregationJobInitializeReq
    (`janus_amd.codec.AggInitReq`) on `threads` host threads (0: all cores).  With `gpu` (a
    `Prio3Gpu` or a context handle) the reports whose first-choice key is X25519 / HKDF-SHA256 /
    AES-128-GCM -- or, with that context's "hpke_gpu_suites" option at 1, any X25519 suite, and
    with its "hpke_gpu_p256" option at 1 the same under P-256 -- are opened on that context's GPU
    instead (prio3gpu_hpke_open_report_shares_gpu); the rest (P-256 while that option is 0, the
    second trial with a global key) stay on the host threads.  Statuses, offsets and
    plaintexts are the host path's.

    -> (plaintexts uint8 array, offsets (n + 1), status); report i's PlaintextInputShare is
    plaintexts[offsets[i]:offsets[i+1]] -- the input of codec.decode_plaintext_input_shares_raw.
    Status 3 = HpkeUnknownConfigId, 4 = HpkeDecryptError (aggregator.rs:1634-1700)."""
    if gpu is not None:
        return _open_report_shares_gpu(_ctx_handle(gpu), task_id, req, task_keys, global_keys,
                                       status, threads, recipient_role)
    n = req.n
    st = np.zeros(n, np.uint8) if status is None else status
    offs = np.zeros(n + 1, np.uint64)
    tid = np.frombuffer(bytes(task_id), np.uint8).copy()
    assert tid.size == 32, "TaskId is 32 bytes"
    tk, keep_t = _keypairs(task_keys)
    gk, keep_g = _keypairs(global_keys)
    L = lib()
    _rc(L.prio3gpu_hpke_open_report_shares(tid.ctypes.data, tk, len(task_keys), gk,
                                           len(global_keys), ROLE_CLIENT, recipient_role,
                                           req.raw.ctypes.data, req.views, n, None,
                                           offs.ctypes.data, st.ctypes.data, threads), "size")
    pts = np.zeros(max(1, int(offs[-1])), np.uint8)
    _rc(L.prio3gpu_hpke_open_report_shares(tid.ctypes.data, tk, len(task_keys), gk,
                                           len(global_keys), ROLE_CLIENT, recipient_role,
                                           req.raw.ctypes.data, req.views, n, pts.ctypes.data,
                                           offs.ctypes.data, st.ctypes.data, threads),
        "open report shares")
    del keep_t, keep_g
    return pts, offs, st


def _open_report_shares_gpu(ctx, task_id, req, task_keys, global_keys, status, threads,
                            recipient_role):
    n = req.n
    st = np.zeros(n, np.uint8) if status is None else status
    offs = np.zeros(n + 1, np.uint64)
    tid = np.frombuffer(bytes(task_id), np.uint8).copy()
    assert tid.size == 32, "TaskId is 32 bytes"
    tk, keep_t = _keypairs(task_keys)
    gk, keep_g = _keypairs(global_keys)
    f = lib().prio3gpu_hpke_open_report_shares_gpu
    _rc(f(ctx, tid.ctypes.data, tk, len(task_keys), gk, len(global_keys), ROLE_CLIENT,
          recipient_role, req.raw.ctypes.data, req.views, n, None, offs.ctypes.data,
          st.ctypes.data, threads), "size")
    pts = np.zeros(max(1, int(offs[-1])), np.uint8)
    _rc(f(ctx, tid.ctypes.data, tk, len(task_keys), gk, len(global_keys), ROLE_CLIENT,
          recipient_role, req.raw.ctypes.data, req.views, n, pts.ctypes.data, offs.ctypes.data,
          st.ctypes.data, threads), "open report shares (GPU)")
    del keep_t, keep_g
    return pts, offs, st
