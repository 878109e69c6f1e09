"""The Noise IX initiator without a GPU: the device header's four phases built
for the CPU (tests/libninithost.so from tests/noise_init_host.cpp: four lane
states stepped through k_noise_ixi's step tables, chained with the host ladder
and the serial ciphers) against grapevine_amd/noise.py's `Initiator`, byte for
byte, for both suites at the padding edges of every variable length.
tests/test_gpu_noise_init.py checks the kernels against the same reference."""
import ctypes
import functools
import os
import random

import pytest

from grapevine_amd import abi, noise

from test_aead import open_, seal

HERE = os.path.dirname(os.path.abspath(__file__))
CIPHERS = (abi.CIPHER_AESGCM, abi.CIPHER_CHACHAPOLY)
# 64 + (31 + 16) + 17 = 128: the last payload 2 whose ct_p is hashed in one block; 111 / 112: in two
P2 = (0, 31, 32, 111, 112, 2048)
CASES = [(pl, l1, 31) for pl in (0, 64) for l1 in (0, 64)] + [(64, 64, p2) for p2 in P2 if p2 != 31]
SPOIL = {"ct_s": lambda m: m[:40] + bytes([m[40] ^ 1]) + m[41:],
         "ct_p": lambda m: m[:100] + bytes([m[100] ^ 1]) + m[101:],
         "tag": lambda m: m[:-1] + bytes([m[-1] ^ 0x80]),
         "short": lambda m: m[:95],
         "re": lambda m: bytes(32) + m[32:]}  # small-order u = 0


@functools.lru_cache(None)
def handshake(cipher, pl, l1, p2):
    """One handshake by the Python reference, made once: the initiator's
    (s, e), message 1 and h after it, the responder's message 2, and what
    `read_message2` returns and keeps."""
    rng = random.Random(f"init/{cipher}/{pl}/{l1}/{p2}")
    s, e, r_s, r_e = (rng.randbytes(32) for _ in range(4))
    prologue, payload1, payload2 = rng.randbytes(pl), rng.randbytes(l1), rng.randbytes(p2)
    aead = (seal, open_) if cipher == abi.CIPHER_AESGCM else (None, None)
    ini = noise.Initiator(s, e, *aead, prologue, cipher)
    msg1 = ini.write_message1(payload1)
    state = ini.ss.h
    msg2 = noise.respond(r_s, r_e, msg1, payload2, aead[0], prologue, cipher)[0]
    k1, k2, h = ini.read_message2(msg2)
    assert ini.payload2 == payload2
    return dict(cipher=cipher, s=s, e=e, prologue=prologue, payload1=payload1, msg1=msg1, state=state, msg2=msg2,
                r_s=r_s, r_e=r_e, want=(ini.rs, payload2, k1, k2, h))


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "libninithost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libninithost.so not built (make)")
    return ctypes.CDLL(path)


def host_finish(lib, c, msg2):
    rs, k1, k2, hh, pay = (ctypes.create_string_buffer(n) for n in (32, 32, 32, 64, 2048))
    plen = ctypes.c_uint32(7)
    rc = lib.nxi_host_finish(c["cipher"], c["s"], c["e"], c["state"], msg2, len(msg2), rs, pay, 2048,
                             ctypes.byref(plen), k1, k2, hh)  # -1: lane states disagree
    assert not any(pay.raw[plen.value:])  # the slot is written whole
    return rc, (rs.raw, pay.raw[:plen.value], k1.raw, k2.raw, hh.raw)


@pytest.mark.parametrize("pl,l1,p2", CASES)
@pytest.mark.parametrize("cipher", CIPHERS)
def test_host_phases_match_the_specification(lib, cipher, pl, l1, p2):
    c = handshake(cipher, pl, l1, p2)
    msg1, state = ctypes.create_string_buffer(64 + l1), ctypes.create_string_buffer(64)
    assert lib.nxi_host_initiate(cipher, c["s"], c["e"], c["prologue"], pl, c["payload1"], l1, msg1, state) == 1
    assert (msg1.raw, state.raw) == (c["msg1"], c["state"])
    assert host_finish(lib, c, c["msg2"]) == (1, c["want"])


@pytest.mark.parametrize("what", sorted(SPOIL))
@pytest.mark.parametrize("cipher", CIPHERS)
def test_host_rejections_are_zero(lib, cipher, what):
    c = handshake(cipher, 64, 64, 32)
    assert host_finish(lib, c, SPOIL[what](c["msg2"])) == (0, (bytes(32), b"", bytes(32), bytes(32), bytes(64)))
