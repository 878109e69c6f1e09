"""The long Noise IX responder without a GPU: k_noise_ix_tail's schedule built
for the CPU and chained with the short responder's host pieces
(tests/libnlonghost.so from tests/noise_long_host.cpp) against
grapevine_amd/noise.py's `respond`, byte for byte, at the block edges of
H(h | ct_p) (payloads of 128 k - 97 and 128 k - 96 bytes)."""
import ctypes
import os

import pytest

from test_noise import HERE, handshake

P2 = (0, 31, 2048, 2049, 2079, 2080, 5000, 65439)


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "libnlonghost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libnlonghost.so not built (make)")
    return ctypes.CDLL(path)


def host_respond(lib, c, extra):
    """The slot is 96 + p2 rounded up to 16 bytes, and `extra` more."""
    p2 = len(c["payload2"])
    stride = -(-(96 + p2) // 16) * 16 + extra
    msg2, k1, k2, hh = (ctypes.create_string_buffer(n) for n in (stride, 32, 32, 64))
    rc = lib.nx_long_host_respond(c["s"], c["e"], c["prologue"], len(c["prologue"]), c["msg1"], len(c["msg1"]),
                                  c["payload2"], p2, msg2, stride, k1, k2, hh)
    return rc, msg2.raw, (k1.raw, k2.raw, hh.raw)


@pytest.mark.parametrize("p2", P2)
@pytest.mark.parametrize("l", (0, 48))
def test_host_tail_matches_the_specification(lib, l, p2):
    c = handshake.__wrapped__(l, l, p2)  # a case of its own: reading message 2 uses its Initiator up
    rc, slot, keys = host_respond(lib, c, 32 if p2 < 65000 else 0)
    assert rc == 1 and (slot[:96 + p2],) + keys == c["want"] and not any(slot[96 + p2:])
    assert c["ini"].read_message2(slot[:96 + p2]) == keys and c["ini"].payload2 == c["payload2"]


@pytest.mark.parametrize("bad", ["re", "rs", "short", "long"])
def test_host_rejections_are_zero(lib, bad):
    c = handshake(48, 47, 2080, bad)
    assert c["want"] is None
    rc, slot, keys = host_respond(lib, c, 16)
    assert rc == 0 and not any(slot) and keys == (bytes(32), bytes(32), bytes(64))
