"""The long ChaCha20-Poly1305 schedule (grapevine_amd/csrc/gvs_chachapoly_long.h:
the chunk grid, the 1 024-way Horner from the front, the power table, the
final exponents, the masked second pass of open) built for the CPU
(tests/libchachapolylonghost.so from tests/chachapoly_long_host.cpp) against
grapevine_amd/chachapoly.py.  `batch` is also what
tests/test_gpu_chachapoly_long.py runs on the device."""
import ctypes
import os
import random

import pytest

from grapevine_amd import abi, chachapoly

HERE = os.path.dirname(os.path.abspath(__file__))
T = 1024  # the Horner stride in 16-byte cells (kClT): four per thread of a 256-thread workgroup
AADS = (0, 20, 64)
# Block and chunk edges, both sides of the short path's limit, the lengths that
# put the grid's end E = nc + 5 at jT - 1, jT and jT + 1 with a last block of
# 16, 1 and 15 bytes, and the maximum.
TEXT_LENS = [0, 1, 16, 63, 64, 65, 2048, 2049] + \
    [16 * (j * T + de - 6) + last for j in (1, 2, 4) for de in (-1, 0, 1) for last in (16, 1, 15)] + \
    [abi.AEAD_LONG_TEXT_MAX]

_BATCH = {}


def batch(aad_len):
    """One message per length under a key and a nonce of its own (every other
    nonce a Noise counter above 2^32) and the reference's ciphertexts, made
    once per AAD length."""
    if aad_len not in _BATCH:
        rng = random.Random(8439 + aad_len)
        keys = [rng.randbytes(32) for _ in TEXT_LENS]
        nonces = [abi.noise_nonce_chachapoly((1 << 32) * (k + 1) + k) if k % 2 else rng.randbytes(12)
                  for k in range(len(TEXT_LENS))]
        aads = [rng.randbytes(aad_len) for _ in TEXT_LENS]
        pts = [rng.randbytes(n) for n in TEXT_LENS]
        _BATCH[aad_len] = keys, nonces, aads, pts, [chachapoly.seal(*x) for x in zip(keys, nonces, aads, pts)]
    return _BATCH[aad_len]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "libchachapolylonghost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libchachapolylonghost.so not built (make)")
    return ctypes.CDLL(path)


@pytest.mark.parametrize("aad_len", AADS)
def test_host_schedule_matches_the_reference(lib, aad_len):
    for key, nonce, aad, pt, want in zip(*batch(aad_len)):
        n = len(pt)
        out, back = ctypes.create_string_buffer(n + 16), ctypes.create_string_buffer(max(n, 1))
        lib.chachapoly_long_host_seal(key, nonce, aad, aad_len, pt, n, out)
        assert out.raw == want, n
        assert lib.chachapoly_long_host_open(key, nonce, aad, aad_len, want, n + 16, back) == 1 and back.raw[:n] == pt, n
        for at in (n // 2, n + 15):  # a ciphertext byte (with no text, the tag's first byte) and a tag byte
            assert lib.chachapoly_long_host_open(key, nonce, aad, aad_len, flip(want, at, 0x10), n + 16, back) == 0, (n, at)
            assert back.raw[:n] == bytes(n), (n, at)


def test_poly1305_with_r_all_ones(lib):
    """The GPU tests cannot choose r; here every bit of r is set before the
    clamp and every block is 0xff, over two tiles and three cells."""
    otk, msg, tag = b"\xff" * 32, b"\xff" * (16 * (2 * T + 3)), ctypes.create_string_buffer(16)
    lib.chachapoly_long_host_poly1305(otk, msg, len(msg) // 16, tag)
    assert tag.raw == chachapoly.poly1305(otk, msg)
