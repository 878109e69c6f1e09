"""The long channel cipher's schedule (grapevine_amd/csrc/gvs_aead_long.h: the
strided Horner from the end of the hash input, the power table, the masked
second pass of open) built for the CPU (tests/libaeadlonghost.so from
tests/aead_long_host.cpp) against `seal` / `open_` of tests/test_aead.py.
`batch` is also what tests/test_gpu_aead_long.py runs on the device."""
import ctypes
import os
import random

import pytest

from grapevine_amd import abi

from test_aead import seal

HERE = os.path.dirname(os.path.abspath(__file__))
T = 512  # the schedule's slots (kAlT): two per thread of a 256-thread workgroup
AADS = (0, 20, 64)


def text_lens(aad_len):
    """Block edges, both sides of the short path's limit, the lengths that put
    the hash-block count m = na + nc + 1 at jT - 1, jT and jT + 1 with a last
    block of 16, 1 and 15 bytes, and the maximum."""
    na = -(-aad_len // 16)
    edges = [16 * (j * T + dm - na - 2) + last for j in (1, 2) for dm in (-1, 0, 1) for last in (16, 1, 15)]
    return [0, 1, 16, 2048, 2049] + edges + [abi.AEAD_LONG_TEXT_MAX]


_BATCH = {}


def batch(aad_len):
    """One message per length under a key and an IV of its own (every other IV
    a Noise counter) and the reference's ciphertexts, made once per AAD length."""
    if aad_len not in _BATCH:
        rng = random.Random(4000 + aad_len)
        lens = text_lens(aad_len)
        keys = [rng.randbytes(32) for _ in lens]
        ivs = [abi.noise_iv((1 << 32) * k + k) if k % 2 else rng.randbytes(12) for k in range(len(lens))]
        aads = [rng.randbytes(aad_len) for _ in lens]
        pts = [rng.randbytes(n) for n in lens]
        _BATCH[aad_len] = keys, ivs, aads, pts, [seal(*x) for x in zip(keys, ivs, aads, pts)]
    return _BATCH[aad_len]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


@pytest.mark.parametrize("aad_len", AADS)
def test_host_schedule_matches_the_reference(aad_len):
    path = os.path.join(HERE, "libaeadlonghost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libaeadlonghost.so not built (make)")
    lib = ctypes.CDLL(path)
    for key, iv, aad, pt, want in zip(*batch(aad_len)):
        n = len(pt)
        out, back = ctypes.create_string_buffer(n + 16), ctypes.create_string_buffer(max(n, 1))
        lib.aead_long_host_seal(key, iv, aad, aad_len, pt, n, out)
        assert out.raw == want, n
        assert lib.aead_long_host_open(key, iv, aad, aad_len, want, n + 16, back) == 1 and back.raw[:n] == pt, n
        for at in (n // 2, n + 15):  # a ciphertext byte (with no text, the tag's first byte) and a tag byte
            assert lib.aead_long_host_open(key, iv, aad, aad_len, flip(want, at, 0x10), n + 16, back) == 0, (n, at)
            assert back.raw[:n] == bytes(n), (n, at)
