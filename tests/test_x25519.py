"""The channel's key agreement without a GPU: grapevine_amd/x25519.py (the
Python-integer X25519 and the HKDF over hmac / hashlib) against the openssl
fixture and RFC 7748's vector (tests/golden/x25519_openssl.json), and the
device ladder and HKDF built for the CPU (tests/libxhost.so from
tests/x25519_host.cpp: a quad as four lane states stepped in a loop) against
the Python ones.  tests/test_gpu_x25519.py checks the kernels on the same
inputs."""
import ctypes
import functools
import json
import os
import random

import pytest

from grapevine_amd import x25519 as xr

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libxhost.so")
le = lambda v: v.to_bytes(32, "little")
# small-order u (0, 1, p-1 and their non-canonical forms p, p+1), the largest
# u, and the base point with the ignored top bit set
EDGE_U = [le(v) for v in (0, 1, xr.P - 1, xr.P, xr.P + 1, 2 ** 255 - 1, 9 | 1 << 255)]
SMALL_ORDER = EDGE_U[:5]


def fixture():
    with open(os.path.join(HERE, "golden", "x25519_openssl.json")) as f:
        return [{k: bytes.fromhex(v) for k, v in r.items()} for r in json.load(f)]


@functools.lru_cache(None)
def cases():
    """259 (scalar, u, X25519(scalar, u)) by the Python reference, made once:
    RFC 7748's vector, the edge u under random scalars, the edge scalars (all
    zero, all ones, every bit the clamp changes set the wrong way) over random
    and edge u, the rest of the fixture, then random items."""
    rng = random.Random(25519)
    wrong_way = lambda: le(int.from_bytes(rng.randbytes(32), "little") & ~(1 << 254) | 7 | 1 << 255)
    fx = fixture()
    sc_u = [(fx[0]["scalar"], fx[0]["u"])] + [(rng.randbytes(32), u) for u in EDGE_U]
    edge_s = (bytes(32), b"\xff" * 32, wrong_way())
    sc_u += [(s, u) for s in edge_s for u in (rng.randbytes(32), EDGE_U[2], EDGE_U[5])]
    sc_u += [(r["scalar"], r["u"]) for r in fx[1:]]
    sc_u += [(rng.randbytes(32), rng.randbytes(32)) for _ in range(259 - len(sc_u))]
    return [(s, u, xr.x25519(s, u)) for s, u in sc_u]


def test_python_x25519_on_the_fixture():
    fx = fixture()
    assert len(fx) == 13
    for r in fx:
        assert xr.x25519(r["scalar"], r["u"]) == r["out"]
    for u in SMALL_ORDER:
        assert xr.x25519(fx[0]["scalar"], u) == bytes(32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("tests/libxhost.so not built (make)")
    return ctypes.CDLL(LIB)


def test_host_quad_ladder_matches_python(lib):
    out = ctypes.create_string_buffer(32)
    for s, u, want in cases()[:40]:  # every edge, the fixture, a few random items
        rc = lib.x_host_x25519(s, u, out)  # -1: the quad's lanes disagree
        assert (rc, out.raw) == (int(want != bytes(32)), want), (s.hex(), u.hex())
    s = cases()[0][0]
    assert lib.x_host_x25519(s, None, out) == 1 and out.raw == xr.x25519(s)  # null: the base point


@pytest.mark.parametrize("ikm_len", [0, 32])
def test_host_hkdf_matches_hmac(lib, ikm_len):
    rng = random.Random(512 + ikm_len)
    o1, o2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    for ck in (bytes(64), b"\xff" * 64, rng.randbytes(64), rng.randbytes(64)):
        ikm = rng.randbytes(ikm_len)
        lib.x_host_hkdf(ck, ikm or None, ikm_len, o1, o2)
        assert (o1.raw, o2.raw) == xr.noise_hkdf(ck, ikm)
