"""The device challenge stream (gvs_chacha.h: the ChaCha20 block function and
the draw selection) built for the CPU (tests/libchachahost.so from
tests/chacha_host.cpp) and checked against keystream made by the openssl CLI
at block counters either side of the 32-bit carry
(tests/golden/chacha20_openssl_counters.json), RFC 8439 §2.3.2, and
grapevine_amd/server.py's ChallengeRng.  The GPU tests
(tests/test_gpu_challenge.py) check the kernel itself."""
import ctypes
import json
import os
import random

import pytest

from grapevine_amd import server as gs

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libchachahost.so")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/libchachahost.so not built (make)")
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "chacha20_openssl_counters.json")) as f:
        return [(bytes.fromhex(v["key"]), int(v["counter"]), bytes.fromhex(v["keystream"]))
                for v in json.load(f)]


def block(lib, key, counter, stream=0):
    out = ctypes.create_string_buffer(64)
    lib.chacha_host_block(key, U64(counter), U64(stream), out)
    return out.raw


def draw(lib, seed, d):
    out = ctypes.create_string_buffer(32)
    lib.chacha_host_draw(seed, U64(d), out)
    return out.raw


def test_fixture_covers_the_counters(vectors):
    assert len({k for k, _, _ in vectors}) == 3
    for key in {k for k, _, _ in vectors}:
        assert sorted(c for k, c, _ in vectors if k == key) == \
            [0, 1, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, (1 << 63) - 1]
    assert all(len(ks) == 128 for _, _, ks in vectors)


def test_python_block_matches_openssl(vectors):
    """The checker of the other tests is itself pinned to openssl at these counters."""
    for key, c, ks in vectors:
        assert gs.chacha20_block(key, c) + gs.chacha20_block(key, c + 1) == ks, (key.hex(), c)


def test_host_block_matches_openssl(lib, vectors):
    for key, c, ks in vectors:
        assert block(lib, key, c) == ks[:64], (key.hex(), c)
        assert block(lib, key, c + 1) == ks[64:], (key.hex(), c + 1)  # over the 32-bit carry too


def test_host_block_reproduces_rfc8439(lib):
    """RFC 8439 §2.3.2: key 00..1f, block counter 1, nonce 00:00:00:09 00:00:00:4a
    00:00:00:00.  In the 64-bit layout the nonce's first word is the counter's
    high word and the rest is the stream id."""
    key = bytes(range(32))
    got = block(lib, key, 1 | 0x09000000 << 32, 0x4A000000)
    want = bytes.fromhex(
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert got[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert got == want
    assert got == gs.chacha20_block(key, 1 | 0x09000000 << 32, 0x4A000000)


def test_draw_selection_matches_challenge_rng(lib):
    rng = random.Random(21)
    for _ in range(4):
        seed = rng.randbytes(32)
        r = gs.ChallengeRng(seed)
        for d in range(10):
            assert draw(lib, seed, d) == r.draw(32), d
        for d in ((1 << 33) - 1, 1 << 33, (1 << 33) + 1, (1 << 64) - 1):
            assert draw(lib, seed, d) == gs.chacha20_block(seed, d >> 1)[32 * (d & 1):][:32], d
