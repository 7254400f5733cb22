"""Batched HPKE open of long ciphertexts on the GPU, a wave per report, under DHKEM(P-256,
HKDF-SHA256) keys behind the context's "hpke_gpu_p256" option (hpke_gpu.h's k_p256_dh, then
hpke_open_team.h's kernels with bc.dh_ok set): RFC 9180's P-256 vectors alone and among tampered
neighbours, equality with the lane-per-report open and the host, refused encapsulated keys, an
all-zero DH value that is no failure, and the input-share form over 65-byte enc columns."""
import hashlib
import json
import os

import numpy as np
import pytest

from janus_amd import hpke as H
from janus_amd._lib import lib
from tests import hpke_suite_model as M
from tests import p256_model as E

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                      "hpke_rfc9180_vectors.json")))
P256_VECTORS = [v for v in VECTORS if v["kem_id"] == 0x10]
h = bytes.fromhex
INFO = H.application_info(H.Label.INPUT_SHARE, H.ROLE_CLIENT, H.ROLE_LEADER)
KEM = H.KEM_P256_HKDF_SHA256
LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4101)
E_ARG, E_HPKE, E_UNSUPPORTED = -1, -5, -6


def _new_gpu(**options):
    from janus_amd.prio3 import Prio3Gpu
    v = Prio3Gpu.new_count(bytes(16))
    for k, val in options.items():
        v.set_option(k, val)
    return v


@pytest.fixture(scope="module")
def gpu():
    v = _new_gpu(hpke_gpu_p256=1, hpke_gpu_suites=1)
    yield v
    v.close()


@pytest.fixture(scope="module")
def gpu_chacha():
    v = _new_gpu(hpke_gpu_p256=1, hpke_gpu_suites=1, hpke_team_chacha=1)
    yield v
    v.close()


def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _open(gpu, kp, info, items, fn=H.open_long_batch_gpu):
    """[(enc, aad, ct)] -> ([plaintext slot], status)"""
    encs = np.frombuffer(b"".join(e for e, _, _ in items), np.uint8)
    aads = np.frombuffer(b"".join(a for _, a, _ in items) + b"\0", np.uint8)
    cts = np.frombuffer(b"".join(c for _, _, c in items) + b"\0", np.uint8)
    pts, poff, st = fn(gpu, kp, info, encs, aads, _offsets([len(a) for _, a, _ in items]), cts,
                       _offsets([len(c) for _, _, c in items]))
    return [pts[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(len(items))], st


def _keypair(kdf, aead, config_id=1):
    return H.generate_hpke_config_and_private_key(config_id, KEM, kdf, aead)


def _scalar(rng):
    return E.random_scalar(rng).to_bytes(32, "big")


# ---- 1. the option -------------------------------------------------------------------------------
def test_option_off_is_unsupported():
    v = _new_gpu()
    try:
        kp = _keypair(1, 1)
        _, enc, ct = H.seal(kp.config, INFO, b"message", b"aad")
        with pytest.raises(ValueError):
            _open(v, kp, INFO, [(enc, b"aad", ct)])
    finally:
        v.close()


def test_bad_keypair_is_refused_before_any_launch(gpu):
    kp = _keypair(1, 1)
    c = kp.config
    x, y = E.decode(c.public_key)
    _, enc, ct = H.seal(c, INFO, b"message", b"aad")
    off_curve = H.HpkeKeypair(H.HpkeConfig(1, KEM, 1, 1, E.encode((x, (y + 1) % E.P))),
                              kp.private_key)
    zero_sk = H.HpkeKeypair(c, bytes(32))
    big_sk = H.HpkeKeypair(c, E.N.to_bytes(32, "big"))
    for bad in (off_curve, zero_sk, big_sk):
        with pytest.raises(H.HpkeError):
            _open(gpu, bad, INFO, [(enc, b"aad", ct)])
    rc = lib().prio3gpu_hpke_open_long_batch(gpu._ctx, KEM, 1, 1, kp.private_key, 32,
                                             c.public_key, 32, INFO, len(INFO), 1, None, None,
                                             None, None, None, None, None, None)
    assert rc == E_ARG


# ---- 2. RFC 9180 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("v", P256_VECTORS, ids=lambda v: f"kdf{v['kdf_id']}-aead{v['aead_id']}")
def test_rfc9180_vector_alone_and_among_tampered_neighbours(gpu, gpu_chacha, v):
    g = gpu_chacha if v["aead_id"] == 3 else gpu
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x10, v["kdf_id"], v["aead_id"], h(v["pkRm"])),
                       h(v["skRm"]))
    info, enc, aad, ct, pt = (h(v[k]) for k in ("info", "enc", "aad", "ct", "pt"))
    pts, st = _open(g, kp, info, [(enc, aad, ct)])
    assert st[0] == 0 and pts[0] == pt
    items, kinds = [], []
    for i in range(21):
        kind = ("intact", "enc", "aad", "body", "tag")[i % 5]
        kinds.append(kind)
        items.append({"intact": (enc, aad, ct),
                      "enc": (_flip(enc, (7 * i) % 520), aad, ct),
                      "aad": (enc, _flip(aad, i % (8 * len(aad))), ct),
                      "body": (enc, aad, _flip(ct, (5 * i) % (8 * (len(ct) - 16)))),
                      "tag": (enc, aad, _flip(ct, 8 * (len(ct) - 16) + (3 * i) % 128))}[kind])
    pts, st = _open(g, kp, info, items)
    for i, kind in enumerate(kinds):
        if kind == "intact":
            assert st[i] == 0 and pts[i] == pt, i
        else:
            assert st[i] == 4 and pts[i] == bytes(len(pt)), (i, kind)


def test_chacha_vectors_need_the_team_option(gpu):
    v = [x for x in P256_VECTORS if x["aead_id"] == 3][0]
    kp = H.HpkeKeypair(H.HpkeConfig(0, 0x10, v["kdf_id"], 3, h(v["pkRm"])), h(v["skRm"]))
    with pytest.raises(ValueError):
        _open(gpu, kp, h(v["info"]), [(h(v["enc"]), h(v["aad"]), h(v["ct"]))])


# ---- 3. the lane per report and the host ---------------------------------------------------------
@pytest.mark.parametrize("kdf,aead", [(k, a) for k in (1, 2, 3) for a in (1, 2, 3)])
def test_wave_open_equals_lane_open_and_host(gpu, gpu_chacha, kdf, aead):
    g = gpu_chacha if aead == 3 else gpu
    rng = np.random.default_rng(300 * kdf + aead)
    kp = _keypair(kdf, aead)
    items, want = [], []
    for j, pl in enumerate(LENS):
        pt, aad = _rnd(rng, pl), _rnd(rng, (0, 60, 92)[j % 3])
        _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=_scalar(rng))
        if j % 4 == 3:                      # a forged tag among them
            ct, pt = _flip(ct, 8 * pl + 5), None
        items.append((enc, aad, ct))
        want.append(pt)
    wave, st = _open(g, kp, INFO, items)
    lane, lst = _open(g, kp, INFO, items, fn=H.open_batch_gpu)
    assert wave == lane and st.tolist() == lst.tolist()
    for (enc, aad, ct), pt, got, s in zip(items, want, wave, st):
        if pt is None:
            assert s == 4 and got == bytes(len(ct) - 16)
            with pytest.raises(H.HpkeError):
                H.open_(kp, INFO, enc, ct, aad)
        else:
            assert s == 0 and got == pt == H.open_(kp, INFO, enc, ct, aad)


# ---- 4. refused encapsulated keys ----------------------------------------------------------------
def test_refused_encs_fail_alone(gpu):
    rng = np.random.default_rng(44)
    kp = _keypair(1, 1)
    pt, aad = _rnd(rng, 1025), _rnd(rng, 60)
    _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=_scalar(rng))
    x, y = E.decode(enc)
    bad = [E.encode((x, (y + 1) % E.P)),                               # off the curve
           b"\x04" + E.P.to_bytes(32, "big") + E.SQRT_B.to_bytes(32, "big"),   # x = p
           b"\x03" + enc[1:]]                                          # a compressed point's prefix
    items = [(enc, aad, ct)] + [(b, aad, ct) for b in bad] + [(enc, aad, ct)]
    pts, st = _open(gpu, kp, INFO, items)
    assert st[:5].tolist() == [0, 4, 4, 4, 0]
    assert pts == [pt, bytes(1025), bytes(1025), bytes(1025), pt]


# ---- 5. an all-zero x coordinate is a DH value ---------------------------------------------------
def _aes_sbox():
    box = [0] * 256
    for x in range(256):
        inv, p = 1, x                       # x^254 in GF(2^8)
        for _ in range(7):
            p = _gmul(p, p)
            inv = _gmul(inv, p)
        s = inv if x else 0
        r = s
        for _ in range(4):
            s = ((s << 1) | (s >> 7)) & 0xff
            r ^= s
        box[x] = r ^ 0x63
    return box


def _gmul(a, b):
    r = 0
    for _ in range(8):
        if b & 1:
            r ^= a
        a = ((a << 1) ^ (0x1b if a & 0x80 else 0)) & 0xff
        b >>= 1
    return r


def _aes128_block(key, block, box):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [box[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _gmul(rcon, 2)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    rk = [sum(w[4 * r:4 * r + 4], []) for r in range(11)]
    s = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, 11):
        s = [box[b] for b in s]
        s = [s[(4 * c + 5 * i) % 16] for c in range(4) for i in range(4)]      # ShiftRows
        if r < 10:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_gmul(a[i], 2) ^ _gmul(a[(i + 1) % 4], 3) ^ a[(i + 2) % 4] ^ a[(i + 3) % 4]
                      for i in range(4)]
            s = m
        s = [a ^ b for a, b in zip(s, rk[r])]
    return bytes(s)


def _aes128_gcm_seal(key, nonce, aad, pt):
    """NIST SP 800-38D with a 96-bit nonce, on Python integers: ciphertext || tag."""
    box = _aes_sbox()
    H_ = int.from_bytes(_aes128_block(key, bytes(16), box), "big")

    def mul(x, y):
        z, v = 0, y
        for i in range(127, -1, -1):
            if (x >> i) & 1:
                z ^= v
            v = (v >> 1) ^ (0xe1 << 120 if v & 1 else 0)
        return z

    def ctr(i):
        return _aes128_block(key, nonce + i.to_bytes(4, "big"), box)

    ct = b"".join(bytes(a ^ b for a, b in zip(pt[16 * i:16 * i + 16], ctr(2 + i)))
                  for i in range((len(pt) + 15) // 16))
    y = 0
    for data in (aad, ct):
        for i in range(0, len(data), 16):
            y = mul(y ^ int.from_bytes(data[i:i + 16].ljust(16, b"\0"), "big"), H_)
    y = mul(y ^ ((8 * len(aad)) << 64 | 8 * len(ct)), H_)
    return ct + bytes(a ^ b for a, b in zip(y.to_bytes(16, "big"), ctr(1)))


def test_python_aes_gcm_reproduces_rfc9180_a31():
    """The reference AEAD of the next test, against the vector's own key, nonce and ciphertext."""
    v = [x for x in P256_VECTORS if (x["kdf_id"], x["aead_id"]) == (1, 1)][0]
    # RFC 9180 A.3.1: key and base_nonce of the vector
    key, nonce = h("868c066ef58aae6dc589b6cfdd18f97e"), h("4e0bc5018beba4bf004cca59")
    assert _aes128_gcm_seal(key, nonce, h(v["aad"]), h(v["pt"])) == h(v["ct"])


def test_all_zero_dh_value_opens(gpu):
    """enc = [skR^-1] (0, sqrt b): x([skR] enc) is all zero, a legal DH value.  The ciphertext is
    sealed in Python from the model's shared secret; the wave opens it, like the lane and the
    host."""
    rng = np.random.default_rng(0)
    kp = _keypair(1, 1)
    sk = int.from_bytes(kp.private_key, "big")
    enc = E.encode(E.mul(pow(sk, -1, E.N), E.X0[0]))
    assert E.mul(sk, E.decode(enc))[0] == 0
    ss = E.kem_shared_secret(bytes(32), enc, kp.config.public_key)
    sid = b"HPKE" + b"".join(x.to_bytes(2, "big") for x in (0x10, 1, 1))
    ctx = b"\0" + M.labeled_extract(hashlib.sha256, sid, b"", b"psk_id_hash", b"") \
        + M.labeled_extract(hashlib.sha256, sid, b"", b"info_hash", INFO)
    secret = M.labeled_extract(hashlib.sha256, sid, ss, b"secret", b"")
    key = M.labeled_expand(hashlib.sha256, sid, secret, b"key", ctx, 16)
    nonce = M.labeled_expand(hashlib.sha256, sid, secret, b"base_nonce", ctx, 12)
    pt, aad = _rnd(rng, 1100), _rnd(rng, 60)
    ct = _aes128_gcm_seal(key, nonce, aad, pt)
    assert H.open_(kp, INFO, enc, ct, aad) == pt
    for fn in (H.open_long_batch_gpu, H.open_batch_gpu):
        pts, st = _open(gpu, kp, INFO, [(enc, aad, ct), (enc, aad, _flip(ct, 3))], fn=fn)
        assert st[:2].tolist() == [0, 4] and pts == [pt, bytes(1100)]


# ---- 6. input shares from 65-byte enc columns ----------------------------------------------------
def test_open_input_shares_with_65_byte_enc_columns(gpu):
    rng = np.random.default_rng(65)
    kp = _keypair(1, 2)
    n, slen, pslen = 7, 1031, 5
    plen = 6 + slen + 16
    tid, ids = _rnd(rng, 32), np.frombuffer(_rnd(rng, 16 * n), np.uint8).reshape(n, 16)
    times = rng.integers(0, 2**40, n).astype(np.uint64)
    pubs = np.frombuffer(_rnd(rng, pslen * n), np.uint8).reshape(n, pslen)
    shares = np.frombuffer(_rnd(rng, slen * n), np.uint8).reshape(n, slen)
    o_enc, o_pay = 3, 3 + 65 + 4
    mat = np.full((n, o_pay + plen + 7), 0xA5, np.uint8)
    want_st = [0, 0, 8, 4, 0, 4, 0]
    for i in range(n):
        pt = b"\0\0" + slen.to_bytes(4, "big") + shares[i].tobytes()
        if i == 2:                           # an authentic plaintext with another header
            pt = b"\0\1" + pt[2:]
        aad = H.input_share_aad(tid, ids[i].tobytes(), int(times[i]), pubs[i].tobytes())
        _, enc, ct = H.seal(kp.config, INFO, pt, aad, ephemeral_private_key=_scalar(rng))
        if i == 3:
            ct = _flip(ct, 8 * 500)
        if i == 5:
            enc = b"\x02" + enc[1:]
        mat[i, o_enc:o_enc + 65] = np.frombuffer(enc, np.uint8)
        mat[i, o_pay:o_pay + plen] = np.frombuffer(ct, np.uint8)
    out = np.full((n, slen + 3), 0xA5, np.uint8)
    _, st = H.open_input_shares_gpu(gpu, tid, kp, H.ROLE_LEADER, ids, times, pubs,
                                    mat[:, o_enc:o_enc + 65], mat[:, o_pay:o_pay + plen],
                                    out[:, :slen])
    assert st[:n].tolist() == want_st
    assert (out[:, slen:] == 0xA5).all()
    for i in range(n):
        assert out[i, :slen].tobytes() == (shares[i].tobytes() if want_st[i] == 0 else bytes(slen))
    # packed columns of its own: the default pitch is the KEM's Nenc
    encs = np.ascontiguousarray(mat[:, o_enc:o_enc + 65])
    pays = np.ascontiguousarray(mat[:, o_pay:o_pay + plen])
    out2, st2 = H.open_input_shares_gpu(gpu, tid, kp, H.ROLE_LEADER, ids, times, pubs, encs, pays)
    assert st2[:n].tolist() == want_st and np.array_equal(out2, out[:, :slen])
