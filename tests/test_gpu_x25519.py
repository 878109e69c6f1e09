"""GPU parity of the channel's key agreement (include/gvstore.h gvs_x25519 and
gvs_noise_hkdf, kernels k_x25519 and k_noise_hkdf of gvs_x25519.h) against the
Python references of grapevine_amd/x25519.py, bit for bit, and one handshake's
worth of both feeding the channel cipher."""
import random

import numpy as np
import pytest

from grapevine_amd import abi
from grapevine_amd import x25519 as xr

from test_gpu_challenge import small_store
from test_x25519 import cases

pytestmark = pytest.mark.gpu

# one quad beside fifteen idle ones; a partly filled second wavefront; a second
# workgroup; a ragged last workgroup
SIZES = (1, 17, 65, 259)


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


def arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)


def strided(torch, rows, stride):
    """Device rows `stride` bytes apart, 0xA5 between them."""
    d = torch.full((len(rows), stride), 0xA5, dtype=torch.uint8, device="cuda")
    d[:, :rows.shape[1]] = torch.from_numpy(rows.copy()).cuda()
    return d


@pytest.mark.parametrize("n", SIZES)
def test_x25519_matches_the_reference(store, n):
    torch = pytest.importorskip("torch")
    sc, u, want = (arr(col, 32) for col in zip(*cases()[:n]))
    want_ok = want.any(axis=1)
    assert n < 17 or (not want_ok[1:6].any() and want_ok[[0, 6, 7]].all())  # the small-order u are in
    out, ok = store.x25519(sc, u)
    assert (out == want).all() and (ok == want_ok).all(), np.nonzero((out != want).any(axis=1))[0][:8]
    # the device form, every stride larger than its element
    d_sc, d_u = strided(torch, sc, 40), strided(torch, u, 48)
    d_out = torch.full((n, 36), 0xA5, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    assert store.lib.gvs_x25519_device(store.h, d_sc.data_ptr(), 40, d_u.data_ptr(), 48, n, d_out.data_ptr(), 36,
                                       d_ok.data_ptr()) == 0
    got = d_out.cpu().numpy()
    assert (got[:, :32] == want).all() and (got[:, 32:] == 0xA5).all()
    assert (d_ok.cpu().numpy() == want_ok).all()


@pytest.mark.parametrize("n", SIZES)
def test_null_points_are_the_base_point(store, n):
    sc = arr([c[0] for c in cases()[:n]], 32)
    pk, ok = store.x25519(sc)
    pk9, _ = store.x25519(sc, arr([xr.BASE_POINT] * n, 32))
    assert (pk == pk9).all() and ok.all()
    assert pk[n - 1].tobytes() == xr.x25519(sc[n - 1].tobytes())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ikm_len", [0, 32])
def test_noise_hkdf_matches_the_reference(store, n, ikm_len):
    torch = pytest.importorskip("torch")
    rng = random.Random(64 * n + ikm_len)
    cks = [bytes(64), b"\xff" * 64][:n] + [rng.randbytes(64) for _ in range(n - 2)]
    ikm = [rng.randbytes(ikm_len) for _ in range(n)]
    want1, want2 = (arr(col, 64) for col in zip(*[xr.noise_hkdf(c, i) for c, i in zip(cks, ikm)]))
    o1, o2 = store.noise_hkdf(arr(cks, 64), arr(ikm, 32) if ikm_len else None)
    assert (o1 == want1).all() and (o2 == want2).all()
    d_ck = strided(torch, arr(cks, 64), 72)
    d_ikm = strided(torch, arr(ikm, 32), 40) if ikm_len else None
    d_o = torch.full((2, n, 80), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert store.lib.gvs_noise_hkdf_device(store.h, d_ck.data_ptr(), 72, d_ikm.data_ptr() if ikm_len else None, 40,
                                           ikm_len, n, d_o[0].data_ptr(), d_o[1].data_ptr(), 80) == 0
    got = d_o.cpu().numpy()
    assert (got[0, :, :64] == want1).all() and (got[1, :, :64] == want2).all() and (got[:, :, 64:] == 0xA5).all()


def test_misuse_is_refused(store):
    lib, h, bad = store.lib, store.h, abi.GVS_ERR_INVALID_ARG
    buf = np.zeros(256, np.uint8)  # never read: every call fails its argument check
    b = buf.ctypes.data
    assert lib.gvs_x25519(h, None, None, 1, b, b) == bad
    assert lib.gvs_x25519_device(h, b, 31, None, 0, 1, b, 32, None) == bad
    assert lib.gvs_x25519_device(h, b, 32, b, 31, 1, b, 32, None) == bad
    assert lib.gvs_x25519_device(h, b, 32, None, 0, 1, b, 31, None) == bad
    assert lib.gvs_noise_hkdf(h, b, b, 16, 1, b, b) == bad
    assert lib.gvs_noise_hkdf(h, b, None, 32, 1, b, b) == bad
    assert lib.gvs_noise_hkdf_device(h, b, 63, None, 0, 0, 1, b, b, 64) == bad
    assert lib.gvs_noise_hkdf_device(h, b, 64, b, 31, 32, 1, b, b, 64) == bad
    assert lib.gvs_noise_hkdf_device(h, b, 64, None, 0, 0, 1, b, b, 63) == bad
    assert lib.gvs_x25519(h, None, None, 0, None, None) == 0  # n = 0 is a no-op
    assert lib.gvs_noise_hkdf(h, None, None, 0, 0, None, None) == 0


def test_handshake_keys_open_the_channel(store):
    """An IX-shaped key agreement between an initiator (e, s) and a responder
    (e, s): public keys, the ee, se and es products from both sides, three
    MixKeys from a fixed chaining key and a Split, all on the device; the two
    sides agree with each other and with the Python chain, and a message sealed
    under the initiator's sending key opens under the responder's receiving
    key and under no other."""
    rng = random.Random(7748)
    ie, is_, re, rs = (rng.randbytes(32) for _ in range(4))
    pub, ok = store.x25519(arr([ie, is_, re, rs], 32))
    assert ok.all()
    # initiator: e*RE, s*RE, e*RS; responder: e*IE, e*IS, s*IE
    dh, ok = store.x25519(arr([ie, is_, ie, re, re, rs], 32), pub[[2, 2, 3, 0, 1, 0]])
    assert ok.all() and (dh[:3] == dh[3:]).all()
    assert dh[1].tobytes() == xr.x25519(is_, xr.x25519(re))
    ck = np.tile(np.frombuffer(b"Noise_IX_25519_AESGCM_SHA512".ljust(64, b"\0"), np.uint8), (2, 1))
    want = ck[0].tobytes()
    for step in range(3):  # MixKey(ee), MixKey(se), MixKey(es): row 0 the initiator's, row 1 the responder's
        ck, _ = store.noise_hkdf(ck, dh[[step, 3 + step]])
        want, _ = xr.noise_hkdf(want, dh[step].tobytes())
    k1, k2 = store.noise_hkdf(ck)  # Split
    assert (k1[0] == k1[1]).all() and (k2[0] == k2[1]).all()
    assert (k1[0].tobytes(), k2[0].tobytes()) == xr.noise_hkdf(want)
    send, other = k1[:1, :32], k2[:1, :32]  # the initiator sends under o1, receives under o2
    iv, msg = arr([abi.noise_iv(0)], 12), [b"the first transport message"]
    sealed = store.aead_seal(send, iv, msg)
    opened, ok, _ = store.aead_open(k1[1:, :32], iv, sealed)
    assert ok.all() and opened == msg
    _, ok, _ = store.aead_open(other, iv, sealed)
    assert not ok.any()
