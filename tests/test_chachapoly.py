"""ChaCha20-Poly1305 on the CPU: grapevine_amd/chachapoly.py (the client's half
and the GPU tests' reference) and the device header built for the host
(tests/libchachapolyhost.so from gvs_chachapoly.h) against RFC 8439 (§2.8.2,
Appendix A.5, and for Poly1305 Appendix A.3: the cases random messages almost
never reach) and against OpenSSL (tests/golden/chachapoly_openssl.json); and
the ChaChaPoly Noise suite of grapevine_amd/noise.py end to end."""
import ctypes
import hashlib
import json
import os
import random

import pytest

from grapevine_amd import abi, chachapoly, noise

from test_noise import handshake

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
CP = abi.CIPHER_CHACHAPOLY

SUNSCREEN = dict(  # RFC 8439 §2.8.2
    key=bytes(range(0x80, 0xa0)), nonce=H("070000004041424344454647"), aad=H("50515253c0c1c2c3c4c5c6c7"),
    pt=b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
       b"sunscreen would be it.",
    ct=H("d31a8d34648e60db7b86afbc53ef7ec2a4aded51296e08fea9e2b5a736ee62d63dbea45e8ca9671282fafb69da92728b"
         "1a71de0a9e060b2905d6a5b67ecd3b3692ddbd7f2d778b8c9803aee328091b58fab324e4fad675945585808b4831d7bc"
         "3ff4def08e4b7a9de576d26586cec64b6116"),
    tag=H("1ae10b594f09e26a7e902ecbd0600691"))
A5 = dict(  # RFC 8439 Appendix A.5: 265 bytes of the Internet-Drafts boilerplate
    key=H("1c9240a5eb55d38af333888604f6b5f0473917c1402b80099dca5cbc207075c0"), nonce=H("000000000102030405060708"),
    aad=H("f33388860000000000004e91"),
    ct=H("64a0861575861af460f062c79be643bd5e805cfd345cf389f108670ac76c8cb24c6cfc18755d43eea09ee94e382d26b0"
         "bdb7b73c321b0100d4f03b7f355894cf332f830e710b97ce98c8a84abd0b948114ad176e008d33bd60f982b1ff37c855"
         "9797a06ef4f0ef61c186324e2b3506383606907b6a7c02b0f9f6157b53c867e4b9166c767b804d46a59b5216cde7a4e9"
         "9040c5a40433225ee282a1b0a06c523eaf4534d7f83fa1155b0047718cbc546a0d072b04b3564eea1b422273f548271a"
         "0bb2316053fa76991955ebd63159434ecebb4e466dae5a1073a6727627097a1049e617d91d361094fa68f0ff77987130"
         "305beaba2eda04df997b714d6c6f2c29a6ad5cb4022b02709b"),
    tag=H("eead9d67890cbb22392336fea1851f38"))

_IETF = (b'Any submission to the IETF intended by the Contributor for publication as all or part of an IETF '
         b'Internet-Draft or RFC and any statement made within the context of an IETF activity is considered '
         b'an "IETF Contribution". Such statements include oral statements in IETF sessions, as well as written '
         b'and electronic communications made at any time or place, which are addressed to')
_JABBER = (b"'Twas brillig, and the slithy toves\nDid gyre and gimble in the wabe:\nAll mimsy were the "
           b"borogoves,\nAnd the mome raths outgrabe.")
_Z, _R10 = bytes(16), H("01000000000000000400000000000000")
_l = lambda b: H(b).ljust(16, b"\0")
_M10 = H("e33594d7505e43b90000000000000000" "3394d7505e4379cd0100000000000000" + "00" * 16)
A3 = [  # RFC 8439 Appendix A.3, vectors 1 to 11: (one-time key, message, tag)
    (bytes(32), bytes(64), _Z),
    (_Z + H("36e5f6b5c5e06070f0efca96227a863e"), _IETF, H("36e5f6b5c5e06070f0efca96227a863e")),
    (H("36e5f6b5c5e06070f0efca96227a863e") + _Z, _IETF, H("f3477e7cd95417af89a6b8794c310cf0")),
    (A5["key"], _JABBER, H("4541669a7eaaee61e708dc7cbcc5eb62")),
    (_l("02") + _Z, b"\xff" * 16, _l("03")),                                  # 2^130 - 5 wraps to 0 within a step
    (_l("02") + b"\xff" * 16, _l("02"), _l("03")),                            # the carry of h + s is dropped
    (_l("01") + _Z, b"\xff" * 16 + b"\xf0" + b"\xff" * 15 + _l("11"), _l("05")),  # a carry out of the top limb
    (_l("01") + _Z, b"\xff" * 16 + b"\xfb" + b"\xfe" * 15 + b"\x01" * 16, _Z),    # h = p before the final reduction
    (_l("02") + _Z, b"\xfd" + b"\xff" * 15, b"\xfa" + b"\xff" * 15),          # h just below p: not reduced
    (_R10 + _Z, _M10 + _l("01"), H("14000000000000005500000000000000")),
    (_R10 + _Z, _M10, H("13000000000000000000000000000000")),
]


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "chachapoly_openssl.json")) as f:
        return [{k: H(v) for k, v in case.items()} for case in json.load(f)["cases"]]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "libchachapolyhost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libchachapolyhost.so not built (make)")
    return ctypes.CDLL(path)


def host_seal(lib, key, nonce, aad, pt):
    out = ctypes.create_string_buffer(len(pt) + 16)
    lib.chachapoly_host_seal(key, nonce, aad, len(aad), pt, len(pt), out)
    return out.raw


def host_open(lib, key, nonce, aad, msg):
    out = ctypes.create_string_buffer(max(len(msg), 1))
    ok = lib.chachapoly_host_open(key, nonce, aad, len(aad), msg, len(msg), out)
    return out.raw[:max(len(msg) - 16, 0)] if ok else None


def host_poly1305(lib, otk, msg):
    tag = ctypes.create_string_buffer(16)
    lib.chachapoly_host_poly1305(otk, msg, len(msg), tag)
    return tag.raw


def both(lib):
    """(seal, open_) of the Python reference and of the header's host build."""
    return ((chachapoly.seal, chachapoly.open_),
            (lambda *a: host_seal(lib, *a), lambda *a: host_open(lib, *a)))


def test_rfc8439_aead_vectors(lib):
    for seal, open_ in both(lib):
        v = SUNSCREEN
        assert seal(v["key"], v["nonce"], v["aad"], v["pt"]) == v["ct"] + v["tag"]
        assert open_(v["key"], v["nonce"], v["aad"], v["ct"] + v["tag"]) == v["pt"]
        pt = open_(A5["key"], A5["nonce"], A5["aad"], A5["ct"] + A5["tag"])
        assert pt is not None and len(pt) == 265 and pt.startswith(b"Internet-Drafts are draft documents valid for")
        assert seal(A5["key"], A5["nonce"], A5["aad"], pt) == A5["ct"] + A5["tag"]


@pytest.mark.parametrize("k", range(len(A3)))
def test_poly1305_rfc8439_a3(lib, k):
    otk, msg, tag = A3[k]
    assert chachapoly.poly1305(otk, msg) == tag
    assert host_poly1305(lib, otk, msg) == tag


def test_reference_and_host_build_match_openssl(lib, vectors):
    assert {len(v["pt"]) for v in vectors} >= {0, 1, 15, 16, 17, 63, 64, 65}
    assert {len(v["aad"]) for v in vectors} >= {0, 20}
    for v in vectors:
        sealed, args = v["ct"] + v["tag"], (v["key"], v["nonce"], v["aad"])
        bad = bytearray(sealed)
        bad[len(v["pt"]) // 2] ^= 4
        for seal, open_ in both(lib):
            assert seal(*args, v["pt"]) == sealed, len(v["pt"])
            assert open_(*args, sealed) == v["pt"]
            assert open_(*args, bytes(bad)) is None and open_(*args, sealed[:15]) is None


def test_noise_chachapoly_suite_completes_and_talks():
    rng = random.Random(19)
    s, e, i_s, i_e, prologue = (rng.randbytes(32) for _ in range(5))
    ini = noise.Initiator(i_s, i_e, prologue=prologue, cipher=CP)
    got = noise.respond(s, e, ini.write_message1(b"hello"), b"evidence", prologue=prologue, cipher=CP)
    assert got is not None
    msg2, r_recv, r_send, r_h = got
    k1, k2, h = ini.read_message2(msg2)
    assert (k1, k2, h) == (r_recv, r_send, r_h) and ini.payload2 == b"evidence"
    for key, n, text in ((k1, 0, b"a request"), (k2, 0, b"its response"), (k1, 1 << 40, b"another")):
        nonce = abi.noise_nonce_chachapoly(n)
        assert nonce == bytes(4) + n.to_bytes(8, "little")
        assert chachapoly.open_(key, nonce, b"", chachapoly.seal(key, nonce, b"", text)) == text
    # the protocol name is in every hash: the same cipher under the other name does not read it
    other = noise.Initiator(i_s, i_e, chachapoly.seal, chachapoly.open_, prologue)
    other.write_message1(b"hello")
    with pytest.raises(noise.HandshakeError):
        other.read_message2(msg2)


# sha256 of message 2 | k1 | k2 | h of test_noise's case (48, 48, 32), from
# noise.respond as it was before it took `cipher=`
BEFORE = "f055ea9da48a6a33478d6a012209ad9e1856f6e00ed7074a73e7d82cd7b62674"


def test_noise_defaults_give_the_bytes_they_gave():
    from test_aead import open_, seal
    c = handshake(48, 48, 32)
    assert hashlib.sha256(b"".join(c["want"])).hexdigest() == BEFORE
    assert noise.respond(c["s"], c["e"], c["msg1"], c["payload2"], seal, c["prologue"],
                         cipher=abi.CIPHER_AESGCM) == c["want"]
    assert noise.SymmetricState(seal, open_).h == noise.PROTOCOL_NAME.ljust(64, b"\0")
    assert noise.SymmetricState(None, None, CP).h == b"Noise_IX_25519_ChaChaPoly_SHA512".ljust(64, b"\0")
