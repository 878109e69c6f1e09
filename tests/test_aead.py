"""A plain Python-integer AES-256-GCM (NIST SP 800-38D: AES by the S-box, CTR,
GHASH by shift and xor), pinned to the GCM specification's test cases 13 and 14
and to ciphertexts made by OpenSSL (tests/golden/aes256gcm_openssl.json), and
the device header's primitives built for the CPU (tests/libaeadhost.so from
tests/aead_host.cpp over grapevine_amd/csrc/gvs_aead.h) against the same
fixture.  tests/test_gpu_aead.py checks the kernels against `seal` / `open_`."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _sbox():
    xt = lambda v: ((v << 1) ^ (0x11B if v & 0x80 else 0)) & 0xFF
    exp, v = [], 1
    for _ in range(255):
        exp.append(v)
        v ^= xt(v)  # times the generator 3
    sb = []
    for x in range(256):
        s = r = exp[(255 - exp.index(x)) % 255] if x else 0
        for _ in range(4):
            r = ((r << 1) | (r >> 7)) & 0xFF
            s ^= r
        sb.append(s ^ 0x63)
    return sb, xt


SBOX, XT = _sbox()


def expand(key):
    w = [key[4 * i:4 * i + 4] for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = w[i - 1]
        if i % 8 == 0:
            t = bytes(SBOX[b] for b in t[1:] + t[:1])
            t = bytes([t[0] ^ rcon]) + t[1:]
            rcon = XT(rcon)
        elif i % 8 == 4:
            t = bytes(SBOX[b] for b in t)
        w.append(bytes(a ^ b for a, b in zip(w[i - 8], t)))
    return [b"".join(w[4 * r:4 * r + 4]) for r in range(15)]


def encrypt_block(rk, block):
    s = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, 15):
        s = [SBOX[s[(i + 4 * (i % 4)) % 16]] for i in range(16)]  # SubBytes, ShiftRows
        if r < 14:  # MixColumns
            m = []
            for c in range(0, 16, 4):
                a = s[c:c + 4]
                m += [XT(a[i]) ^ XT(a[(i + 1) % 4]) ^ a[(i + 1) % 4] ^ a[(i + 2) % 4] ^ a[(i + 3) % 4]
                      for i in range(4)]
            s = m
        s = [a ^ b for a, b in zip(s, rk[r])]
    return bytes(s)


def gf_mul(x, y):
    """GCM's bit order: bit 127 of the integer is x^0."""
    z = 0
    for i in range(127, -1, -1):
        if (y >> i) & 1:
            z ^= x
        x = (x >> 1) ^ (0xE1 << 120 if x & 1 else 0)
    return z


def _gcm(key, iv, aad, text, ct_of):
    rk = expand(key)
    ks = b"".join(encrypt_block(rk, iv + (j + 2).to_bytes(4, "big")) for j in range((len(text) + 15) // 16))
    res = bytes(a ^ b for a, b in zip(text, ks))
    ct = ct_of(text, res)
    h, y = int.from_bytes(encrypt_block(rk, bytes(16)), "big"), 0
    pad = lambda b: b + bytes(-len(b) % 16)
    data = pad(aad) + pad(ct) + (8 * len(aad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big")
    for o in range(0, len(data), 16):
        y = gf_mul(y ^ int.from_bytes(data[o:o + 16], "big"), h)
    tag = (y ^ int.from_bytes(encrypt_block(rk, iv + b"\0\0\0\1"), "big")).to_bytes(16, "big")
    return res, tag


def seal(key, iv, aad, pt):
    """-> ciphertext | tag"""
    ct, tag = _gcm(key, iv, aad, pt, lambda text, res: res)
    return ct + tag


def open_(key, iv, aad, msg):
    """ciphertext | tag -> plaintext, or None"""
    if len(msg) < 16:
        return None
    pt, tag = _gcm(key, iv, aad, msg[:-16], lambda text, res: text)
    return pt if tag == msg[-16:] else None


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "aes256gcm_openssl.json")) as f:
        return [{k: bytes.fromhex(v) for k, v in case.items()} for case in json.load(f)]


SPEC = ((b"", "530f8afbc74536b9a963b4f1c4cb738b"),  # test cases 13 and 14: zero key, zero IV
        (bytes(16), "cea7403d4d606b6e074ec5d3baf39d18" "d0d1c8a799996bf0265b98b5d48ab919"))


@pytest.mark.parametrize("pt,want", SPEC)
def test_reference_matches_the_specification(pt, want):
    assert seal(bytes(32), bytes(12), b"", pt).hex() == want
    assert open_(bytes(32), bytes(12), b"", bytes.fromhex(want)) == pt


def test_reference_matches_openssl(vectors):
    assert sorted({(len(v["pt"]), len(v["aad"])) for v in vectors}) == \
        [(n, a) for n in (0, 1, 16, 17, 1042, 1099) for a in (0, 20)]
    for v in vectors:
        assert seal(v["key"], v["iv"], v["aad"], v["pt"]) == v["ct"] + v["tag"], len(v["pt"])
        assert open_(v["key"], v["iv"], v["aad"], v["ct"] + v["tag"]) == v["pt"]
        assert open_(v["key"], v["iv"], v["aad"], v["ct"] + v["tag"][:-1] + bytes([v["tag"][-1] ^ 1])) is None


def test_host_build_matches_openssl(vectors):
    path = os.path.join(HERE, "libaeadhost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libaeadhost.so not built (make)")
    lib = ctypes.CDLL(path)
    for v in vectors + [dict(key=bytes(32), iv=bytes(12), aad=b"", pt=pt, ct=bytes.fromhex(w)[:-16],
                             tag=bytes.fromhex(w)[-16:]) for pt, w in SPEC]:
        n = len(v["pt"])
        out = ctypes.create_string_buffer(n + 16)
        lib.aead_host_seal(v["key"], v["iv"], v["aad"], len(v["aad"]), v["pt"], n, out)
        assert out.raw == v["ct"] + v["tag"], n
        back = ctypes.create_string_buffer(max(n, 1))
        assert lib.aead_host_open(v["key"], v["iv"], v["aad"], len(v["aad"]), out.raw, n + 16, back) == 1
        assert back.raw[:n] == v["pt"]
        bad = bytearray(out.raw)
        bad[n // 2] ^= 4
        assert lib.aead_host_open(v["key"], v["iv"], v["aad"], len(v["aad"]), bytes(bad), n + 16, back) == 0
        assert back.raw[:n] == bytes(n)
