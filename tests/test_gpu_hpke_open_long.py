"""The wave-per-report HPKE open on the GPU (janus_amd/csrc/hpke_open_team.h,
prio3gpu_hpke_open_long_batch) for DHKEM(X25519, HKDF-SHA256) with every KDF and AES-128-GCM /
AES-256-GCM: RFC 9180 A.1.1's ciphertext, and the host implementation (hpke.cpp) over ciphertexts
of every length at which the 64-lane stripes change shape.  Everything is byte-exact."""
import json
import os

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "hpke_rfc9180_vectors.json")))
h = bytes.fromhex
P = (1 << 255) - 19
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
SUITES = [(kdf, aead) for kdf in (1, 2, 3) for aead in (1, 2)]
PT_LENS = (0, 1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4101)
AAD_LENS = (0, 60, 92)
E_ARG, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu():
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    yield v
    v.close()


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _pack(items):
    """[(enc, aad, ct)] -> the arrays of open_long_batch_gpu."""
    encs = np.frombuffer(b"".join(e for e, _, _ in items), np.uint8)
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    cts = np.frombuffer(b"".join(c for _, _, c in items) + b"\0", np.uint8)
    aoff = np.cumsum([0] + [len(a) for _, a, _ in items]).astype(np.uint64)
    coff = np.cumsum([0] + [len(c) for _, _, c in items]).astype(np.uint64)
    return encs, aads, aoff, cts, coff


def _open(gpu, kp, info, items, status=None):
    encs, aads, aoff, cts, coff = _pack(items)
    pts, poff, st = H.open_long_batch_gpu(gpu, kp, info, encs, aads, aoff, cts, coff,
                                          status=status)
    return [pts[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(len(items))], st


def _host_open(kp, info, item):
    """(status, plaintext) of the host implementation (hpke.cpp) for one (enc, aad, ct)."""
    enc, aad, ct = item
    try:
        return 0, H.open_(kp, info, enc, ct, aad)
    except H.HpkeError:
        return 4, bytes(max(0, len(ct) - 16))


def _flip(b, byte, bit=0):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def _keypair(kdf, aead, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, H.KEM_X25519_HKDF_SHA256, kdf, aead)


def _mixed(kp, seed):
    """One batch of 48 reports: every plaintext length under the AAD lengths in turn, sealed by
    the host under fixed ephemeral keys."""
    rng = np.random.default_rng(seed)
    items, want = [], []
    for j, pl in enumerate(PT_LENS * 3):
        pt, aad = _rnd(rng, pl), _rnd(rng, AAD_LENS[(j + j // len(PT_LENS)) % 3])
        _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=_rnd(rng, 32))
        items.append((enc, aad, ct))
        want.append(pt)
    return items, want


def _vector0():
    v = VECTORS[0]
    assert (v["kem_id"], v["kdf_id"], v["aead_id"]) == (0x20, 1, 1)
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x20, 1, 1, h(v["pkRm"])), h(v["skRm"]))
    return v, kp


# ---- 1. known answer -----------------------------------------------------------------------------
def test_rfc9180_a1_alone_first_and_last(gpu):
    v, kp = _vector0()
    info, enc, aad, ct, pt = (h(v[k]) for k in ("info", "enc", "aad", "ct", "pt"))
    pts, st = _open(gpu, kp, info, [(enc, aad, ct)])
    assert st[0] == 0 and pts[0] == pt
    rng = np.random.default_rng(91)
    others, plain = [], []
    for pl in (1025, 0, 70, 4101, 16):
        p, a = _rnd(rng, pl), _rnd(rng, 7)
        _, e, c = H.seal(kp.config, info, p, a)
        others.append((e, a, c))
        plain.append(p)
    pts, st = _open(gpu, kp, info, [(enc, aad, ct)] + others + [(enc, aad, ct)])
    assert (st[:7] == 0).all() and pts == [pt] + plain + [pt]


# ---- 2. every suite, mixed lengths ---------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", SUITES)
def test_mixed_lengths_equal_host_open(gpu, kdf, aead):
    kp = _keypair(kdf, aead)
    items, want = _mixed(kp, 100 * kdf + aead)
    assert [_host_open(kp, INFO, it) for it in items[::7]] == [(0, p) for p in want[::7]]
    pts, st = _open(gpu, kp, INFO, items)
    assert (st[:len(items)] == 0).all()
    assert pts == want


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_reports_per_block_boundary(gpu, n):
    kp = _keypair(1, 1)
    items, want = _mixed(kp, n)
    items, want = items[11:11 + n], want[11:11 + n]    # 1040, 2047, 2048, 2049, 4101
    pts, st = _open(gpu, kp, INFO, items)
    assert (st[:n] == 0).all() and pts == want


# ---- 3. tampering --------------------------------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", [(1, 1), (3, 2)])
def test_tampered_reports_fail_alone(gpu, kdf, aead):
    kp = _keypair(kdf, aead)
    rng = np.random.default_rng(7)
    pt, aad = _rnd(rng, 4101), _rnd(rng, 92)
    _, enc, ct = H.seal(kp.config, INFO, pt, aad)
    small = int.from_bytes(h("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"),
                           "little")
    bad = {"tag": (enc, aad, _flip(ct, len(pt) + 5, 3)), "block 0": (enc, aad, _flip(ct, 3)),
           "block 63": (enc, aad, _flip(ct, 16 * 63 + 15, 7)),
           "block 64": (enc, aad, _flip(ct, 16 * 64)),
           "partial last block": (enc, aad, _flip(ct, len(pt) - 1, 1)),
           "aad": (enc, _flip(aad, 60), ct), "enc": (_flip(enc, 9, 2), aad, ct),
           "small-order enc": (small.to_bytes(32, "little"), aad, ct),
           "zero enc": (bytes(32), aad, ct)}
    items = [(enc, aad, ct)]
    for it in bad.values():
        items += [it, (enc, aad, ct)]
    assert [_host_open(kp, INFO, it)[0] for it in items] == [0, 4] * len(bad) + [0]
    pts, st = _open(gpu, kp, INFO, items)
    for i in range(len(items)):
        if i % 2 == 0:
            assert st[i] == 0 and pts[i] == pt, i
        else:
            assert st[i] == 4 and pts[i] == bytes(len(pt)), (i, list(bad)[i // 2])


# ---- 4. statuses, slots, offsets -----------------------------------------------------------------
def test_skipped_short_and_misfit_reports(gpu):
    kp = _keypair(1, 1)
    rng = np.random.default_rng(12)
    lens = (1025, 33, 40, 2049, 1024, 17, 70)
    plain = [_rnd(rng, pl) for pl in lens]
    items = []
    for p in plain:
        a = _rnd(rng, 60)
        _, e, c = H.seal(kp.config, INFO, p, a)
        items.append((e, a, c))
    items[2] = (items[2][0], items[2][1], items[2][2][:15])     # shorter than a tag
    encs, aads, aoff, cts, coff = _pack(items)
    # slots: report 3's is 100 bytes longer than its plaintext, report 4's one byte too short
    slots = [1025, 33, 40, 2049 + 100, 1023, 17, 70]
    poff = np.cumsum([0] + slots).astype(np.uint64)
    pts = np.full(int(poff[-1]), 0xAA, np.uint8)
    st = np.zeros(len(items), np.uint8)
    st[1] = 9                                                    # skipped on entry
    H.open_long_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff, pts=pts, pt_offsets=poff,
                          status=st)
    got = [pts[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(len(items))]
    assert list(st) == [0, 9, 4, 0, 4, 0, 0]
    assert got[0] == plain[0] and got[5] == plain[5] and got[6] == plain[6]
    assert got[1] == bytes(33) and got[2] == bytes(40) and got[4] == bytes(1023)
    assert got[3] == plain[3] + bytes(100)
    # offsets out of order: the report whose ciphertext offsets run backwards fails, alone
    coff2 = coff.copy()
    coff2[5] = coff2[6] + 3
    pts, _, st = H.open_long_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff2,
                                       pt_offsets=np.cumsum([0] + list(lens)).astype(np.uint64))
    assert st[5] == 4 and st[0] == 0 and st[1] == 0 and st[3] == 0 and st[6] == 0
    assert st[4] == 4     # its ciphertext now runs into report 6's: longer than its slot
    assert pts[:1025].tobytes() == plain[0]


def test_unsupported_suites_launch_nothing(gpu):
    rng = np.random.default_rng(5)
    for kem, kdf, aead in ((0x20, 1, 3), (0x10, 1, 1), (0x20, 4, 1), (0x20, 1, 0), (0x21, 1, 1)):
        pk = _rnd(rng, 65 if kem == 0x10 else 32)
        kp = H.HpkeKeypair(H.HpkeConfig(1, kem, kdf, aead, pk), _rnd(rng, 32))
        with pytest.raises(ValueError):
            _open(gpu, kp, INFO, [(_rnd(rng, len(pk)), b"a", _rnd(rng, 40))])
        rc = lib().prio3gpu_hpke_open_long_batch(gpu._ctx, kem, kdf, aead, kp.private_key, 32, pk,
                                                 len(pk), INFO, len(INFO), 0, None, None, None,
                                                 None, None, None, None, None)
        assert rc == E_UNSUPPORTED
    kp = _keypair(1, 1)
    rc = lib().prio3gpu_hpke_open_long_batch(gpu._ctx, 0x20, 1, 1, kp.private_key, 31,
                                             kp.config.public_key, 32, INFO, len(INFO), 0, None,
                                             None, None, None, None, None, None, None)
    assert rc == E_ARG


def test_empty_batch(gpu):
    kp = _keypair(2, 2)
    rc = lib().prio3gpu_hpke_open_long_batch(gpu._ctx, 0x20, 2, 2, kp.private_key, 32,
                                             kp.config.public_key, 32, INFO, len(INFO), 0, None,
                                             None, None, None, None, None, None, None)
    assert rc == 0


def test_device_tensors_equal_host_arrays(gpu):
    import torch
    kp = _keypair(1, 2)
    items, want = _mixed(kp, 77)
    items, want = items[:20], want[:20]
    items[4] = (items[4][0], items[4][1], _flip(items[4][2], 0))
    encs, aads, aoff, cts, coff = _pack(items)
    pts, poff, st = H.open_long_batch_gpu(gpu, kp, INFO, encs, aads, aoff, cts, coff)
    dev = torch.device("cuda", gpu.device)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731
    d_pts = torch.full((len(pts),), 0xAA, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(len(items), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    H.open_long_batch_gpu(gpu, kp, INFO, up(encs), up(aads), up(aoff.astype(np.int64)), up(cts),
                          up(coff.astype(np.int64)), pts=d_pts,
                          pt_offsets=up(poff.astype(np.int64)), status=d_st, n=len(items))
    assert np.array_equal(d_st.cpu().numpy(), st[:len(items)]) and st[4] == 4
    assert np.array_equal(d_pts.cpu().numpy()[:int(poff[-1])], pts[:int(poff[-1])])
    assert [pts[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(20) if i != 4] == \
        [w for i, w in enumerate(want) if i != 4]
