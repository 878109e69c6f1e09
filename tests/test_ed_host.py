"""The device Ed25519 check (gvs_ed25519.h: SHA-512, the strict Edwards
decoding, the whole per-thread verification) built for the CPU
(tests/libedhost.so from tests/ed_host.cpp) and checked against hashlib, the
oracle (oracle/sr25519.py) and signatures made by the openssl CLI.  The GPU
tests (tests/test_gpu_ed25519.py) check the kernel itself."""
import ctypes
import hashlib
import os
import random

import pytest

from oracle import sr25519 as sr

import ed_cases

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libedhost.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("tests/libedhost.so not built (make)")
    return ctypes.CDLL(LIB)


def test_sha512_matches_hashlib(lib):
    rng = random.Random(11)
    out = ctypes.create_string_buffer(64)
    for n in (0, 1, 111, 112, 127, 128, 129, 239, 240, 500):
        data = rng.randbytes(n)
        lib.ed_host_sha512(data, n, out)
        assert out.raw == hashlib.sha512(data).digest(), n


def test_decode_matches_oracle(lib):
    rng = random.Random(12)
    inputs = [rng.randbytes(32) for _ in range(200)]
    for k in (0, 1, 18):
        for sign in (0, 1):
            inputs.append((sr.P + k | sign << 255).to_bytes(32, "little"))  # y >= p
    for y in (1, sr.P - 1, 0):
        for sign in (0, 1):
            inputs.append((y | sign << 255).to_bytes(32, "little"))
    out = ctypes.create_string_buffer(64)
    accepted = 0
    for b in inputs:
        want = sr._ed_decode(b)
        ok = lib.ed_host_decode(b, out)
        assert ok == (want is not None), b.hex()
        if ok:
            accepted += 1
            assert int.from_bytes(out.raw[:32], "little") == want[0], b.hex()
            assert int.from_bytes(out.raw[32:], "little") == want[1], b.hex()
    assert 60 < accepted < 160  # about half of all strings are points
    # the identity is a point; with the sign bit it is not a strict encoding
    assert lib.ed_host_decode((1).to_bytes(32, "little"), out) == 1
    assert lib.ed_host_decode((1 | 1 << 255).to_bytes(32, "little"), out) == 0


def test_verify_on_the_openssl_fixture(lib):
    for r in ed_cases.fixture():
        assert lib.ed_host_verify(r["pk"], r["msg"], len(r["msg"]), r["sig"]) == 1, len(r["msg"])
        for t in ed_cases.bit_flips(r):
            assert lib.ed_host_verify(t["pk"], t["msg"], len(t["msg"]), t["sig"]) == 0, len(r["msg"])


@pytest.mark.parametrize("msg_len", [0, 32, 176])
def test_verify_matches_oracle_on_tampered_cases(lib, msg_len):
    cs = ed_cases.cases(random.Random(13 + msg_len), 24, msg_len)
    valid = 0
    for pk, msg, sig, kind in cs:
        want = sr.ed25519_verify(pk, msg, sig)
        assert bool(lib.ed_host_verify(pk, msg, len(msg), sig)) == want, (kind, pk.hex(), sig.hex())
        valid += want
    assert valid >= len(cs) // 6


def test_verify_on_small_order_keys(lib):
    for pk, msg, sig in ed_cases.small_order_cases():
        want = sr.ed25519_verify(pk, msg, sig)
        assert bool(lib.ed_host_verify(pk, msg, len(msg), sig)) == want, pk.hex()
    pk, msg, sig = ed_cases.small_order_cases()[0]
    assert sr.ed25519_verify(pk, msg, sig)  # the identity key: accepted (no small-order test)
