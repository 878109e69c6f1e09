"""The Noise IX responder without a GPU: the device header's three phases
built for the CPU (tests/libnhost.so from tests/noise_host.cpp: four lane
states stepped through k_noise_ix's step tables, chained with the host ladder
and the serial AES-256-GCM) against grapevine_amd/noise.py's `respond`, byte
for byte, at the padding edges of every variable length, and the Python
`Initiator` completing against its output.  tests/test_gpu_noise.py checks the
kernels against the same reference."""
import ctypes
import functools
import os
import random

import pytest

from grapevine_amd import noise

from test_aead import open_, seal

HERE = os.path.dirname(os.path.abspath(__file__))
# 64 + 47 + 17 = 128: the last payload 1 / prologue hashed in one block;
# 64 + (31 + 16) + 17 = 128: the last payload 2
EDGE = (0, 47, 48, 64)
P2 = (0, 1, 31, 32, 159, 160, 2048)
CASES = [(pl, l1, 31) for pl in EDGE for l1 in EDGE] + [(l, l, p2) for l in (0, 48) for p2 in P2 if p2 != 31]


@functools.lru_cache(None)
def handshake(pl, l1, p2, bad=None):
    """One handshake's inputs and noise.respond's result, made once: the
    responder's (s, e), the prologue, message 1 from an `Initiator` (kept, to
    read message 2 with) and payload 2.  bad: a way to spoil message 1."""
    rng = random.Random(f"{pl}/{l1}/{p2}")
    s, e, i_s, i_e = (rng.randbytes(32) for _ in range(4))
    prologue, payload1, payload2 = rng.randbytes(pl), rng.randbytes(l1), rng.randbytes(p2)
    ini = noise.Initiator(i_s, i_e, seal, open_, prologue)
    msg1 = ini.write_message1(payload1)
    if bad == "re":  # small-order u = 0 as the ephemeral key
        msg1 = bytes(32) + msg1[32:]
    elif bad == "rs":  # small-order u = 1 as the static key
        msg1 = msg1[:32] + (1).to_bytes(32, "little") + msg1[64:]
    elif bad == "short":
        msg1 = msg1[:63]
    elif bad == "long":
        msg1 = msg1[:64] + rng.randbytes(65)
    return dict(s=s, e=e, prologue=prologue, msg1=msg1, payload2=payload2, ini=ini,
                want=noise.respond(s, e, msg1, payload2, seal, prologue))


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(HERE, "libnhost.so")
    if not os.path.exists(path):
        pytest.fail("tests/libnhost.so not built (make)")
    return ctypes.CDLL(path)


def host_respond(lib, c):
    p2 = len(c["payload2"])
    msg2, k1, k2, hh = (ctypes.create_string_buffer(n) for n in (96 + p2, 32, 32, 64))
    rc = lib.nx_host_respond(c["s"], c["e"], c["prologue"], len(c["prologue"]), c["msg1"], len(c["msg1"]),
                             c["payload2"], p2, msg2, k1, k2, hh)  # -1: lane states disagree
    return rc, (msg2.raw, k1.raw, k2.raw, hh.raw)


@pytest.mark.parametrize("pl,l1,p2", CASES)
def test_host_phases_match_the_specification(lib, pl, l1, p2):
    c = handshake(pl, l1, p2)
    assert c["want"] is not None and len(c["want"][0]) == 96 + p2
    rc, got = host_respond(lib, c)
    assert rc == 1 and got == c["want"]
    k1, k2, h = c["ini"].read_message2(got[0])
    assert (k1, k2, h) == got[1:] and c["ini"].payload2 == c["payload2"]
    assert c["ini"].rs == noise.x25519(c["s"])


@pytest.mark.parametrize("bad", ["re", "rs", "short", "long"])
def test_host_rejections_are_zero(lib, bad):
    c = handshake(48, 47, 32, bad)
    assert c["want"] is None
    rc, got = host_respond(lib, c)
    assert rc == 0 and got == (bytes(96 + 32), bytes(32), bytes(32), bytes(64))
