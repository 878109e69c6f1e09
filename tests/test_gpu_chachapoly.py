"""GPU parity of the second channel cipher (include/gvstore.h gvs_chachapoly_open /
gvs_chachapoly_seal, kernel k_chachapoly of gvs_chachapoly.h) against
grapevine_amd/chachapoly.py (itself pinned to RFC 8439 and to OpenSSL by
tests/test_chachapoly.py), of the channel wire call with a cipher chosen against
the seeded wire call on the plaintext in a twin store, and of the responder with
a cipher chosen against grapevine_amd/noise.py."""
import ctypes
import random

import numpy as np
import pytest

from grapevine_amd import abi, chachapoly, noise
from grapevine_amd.chachapoly import open_, seal

from test_gpu_aead import arr, channel_batch, flip  # noqa: F401  (the 200 signed requests)
from test_gpu_challenge import small_store

pytestmark = pytest.mark.gpu
CP = abi.CIPHER_CHACHAPOLY

# the 16- and 64-byte edges, and the ends of a row's first and second pass of 16
# ChaCha blocks (block 0 is the key block: 15 and 31 blocks of text)
TEXT_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 959, 960, 961, 1983, 1984, 1985, 2047, 2048)
NONCES = [abi.noise_nonce_chachapoly(c) for c in (0, 1, 1 << 32, (1 << 64) - 2)]
AADS, NS = (0, 1, 16, 20, 64), (1, 5, 15, 16, 17, 67)  # n: the row, wave and workgroup edges
GUARD = 64


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


_BATCH = {}


def batch(aad_len):
    """67 messages of every length in TEXT_LENS and their reference
    ciphertexts, made once per AAD length; the tests slice it."""
    if aad_len not in _BATCH:
        rng = random.Random(8439 + aad_len)
        keys = [rng.randbytes(32) for _ in range(67)]
        nonces = [NONCES[k // 2 % 4] if k % 2 else rng.randbytes(12) for k in range(67)]
        aads = [rng.randbytes(aad_len) for _ in range(67)]
        pts = [rng.randbytes(TEXT_LENS[k % len(TEXT_LENS)]) for k in range(67)]
        _BATCH[aad_len] = keys, nonces, aads, pts, [seal(*x) for x in zip(keys, nonces, aads, pts)]
    return _BATCH[aad_len]


def device_call(store, do_seal, keys, nonces, aads, msgs):
    """gvs_chachapoly_{seal,open}_device on torch tensors whose output slots and
    a guard after the last are 0xA5 -> (outputs, ok, slab, guard)."""
    import torch
    n = len(msgs)
    slab, lens, stride = store._wire_slab(msgs, -(-max(len(m) for m in msgs) // 16) * 16 or 16)
    aad, alens, astride = store._wire_slab(aads, 64)
    ostride = stride + 16 if do_seal else stride
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d = [up(x) for x in (arr(keys, 32), arr(nonces, 12), aad, alens, slab, lens)]
    out = torch.full((n * ostride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    olens, ok = (torch.zeros(n * 4, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    fn = store.lib.gvs_chachapoly_seal_device if do_seal else store.lib.gvs_chachapoly_open_device
    rc = fn(store.h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), astride, d[3].data_ptr(), d[4].data_ptr(),
            stride, d[5].data_ptr(), n, out.data_ptr(), ostride, olens.data_ptr(), *([] if do_seal else [ok.data_ptr()]))
    assert rc == 0, store.lib.gvs_last_error(store.h)
    out, olens = out.cpu().numpy(), olens.cpu().numpy().view(np.uint32)
    rows = out[:n * ostride].reshape(n, ostride)
    return [rows[k, :olens[k]].tobytes() for k in range(n)], ok.cpu().numpy().view(np.uint32).astype(bool), rows, out[n * ostride:]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("aad_len,n", [(a, n) for a in AADS for n in NS])
def test_seal_and_open_match_the_reference(store, form, aad_len, n):
    keys, nonces, aads, pts, want = [x[:n] for x in batch(aad_len)]
    if form == "host":
        got = store.chachapoly_seal(arr(keys, 32), arr(nonces, 12), pts, aads if aad_len else None)
        back, ok, _ = store.chachapoly_open(arr(keys, 32), arr(nonces, 12), want, aads if aad_len else None)
    else:
        pytest.importorskip("torch")
        got, _, rows, guard = device_call(store, True, keys, nonces, aads, pts)
        assert (guard == 0xA5).all()
        assert all(not rows[k, len(want[k]):].any() for k in range(n))  # written whole: zero past the tag
        back, ok, rows, guard = device_call(store, False, keys, nonces, aads, want)
        assert (guard == 0xA5).all() and all(not rows[k, len(pts[k]):].any() for k in range(n))
    assert got == want, [k for k in range(n) if got[k] != want[k]]
    assert ok.all() and back == pts, [k for k in range(n) if back[k] != pts[k]]


@pytest.mark.parametrize("what", ["ct_first", "ct_last", "tag", "aad", "nonce", "key", "short"])
def test_rejection_spares_the_neighbours(store, what):
    """Message 2 of 6 (one wave and the next) is spoiled; it alone must fail."""
    keys, nonces, aads, pts, want = [list(x[13:19]) for x in batch(20)]  # lengths 1985, 2047, 2048, 0, 1, 15
    assert len(pts[2]) == 2048
    msgs = list(want)
    if what == "ct_first":
        msgs[2] = flip(msgs[2], 0)
    elif what == "ct_last":
        msgs[2] = flip(msgs[2], len(pts[2]) - 1, 0x80)
    elif what == "tag":
        msgs[2] = flip(msgs[2], len(msgs[2]) - 1)
    elif what == "aad":
        aads[2] = flip(aads[2], 19)
    elif what == "nonce":
        nonces[2] = flip(nonces[2], 11)
    elif what == "key":
        keys[2] = flip(keys[2], 31, 0x40)
    else:
        msgs[2] = msgs[2][:15]
    back, ok, slab = store.chachapoly_open(arr(keys, 32), arr(nonces, 12), msgs, aads)
    assert ok.tolist() == [k != 2 for k in range(6)]
    assert back == [b"" if k == 2 else pts[k] for k in range(6)]
    assert not slab[2].any()  # the whole slot, not only its length


# --------------------------------------------------------- the channel wire call

def channel_call(store, b, lo, hi, form, cipher, sealed):
    """The channel call with a cipher chosen (cipher None: the call without
    one), host form or device form on torch tensors -> (responses, statuses)."""
    k = lambda d: (b["keys"][d][lo:hi], b["ivs"][d][lo:hi])
    if form == "host":
        got, _, st, _ = store.process_wire_batch_channel(sealed, b["times"][lo:hi], b["seeds"][lo:hi], b["draws"][lo:hi],
                                                         *k(0), *k(1), cipher=cipher)
        return got, st
    import torch
    n, stride, ostride = hi - lo, 1120, 1072
    slab, lens, _ = store._wire_slab(sealed, stride)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    args = [up(x) for x in (slab, lens, b["times"][lo:hi], b["seeds"][lo:hi], b["draws"][lo:hi], *k(0), *k(1))]
    out, olens, sigs, st = (torch.zeros(n * w, dtype=torch.uint8, device="cuda") for w in (ostride, 4, 64, 4))
    torch.cuda.synchronize()
    p = [a.data_ptr() for a in args]
    fn, head = store.lib.gvs_process_wire_batch_channel_device, [store.h]
    if cipher is not None:
        fn, head = store.lib.gvs_process_wire_batch_channel_cipher_device, [store.h, cipher]
    rc = fn(*head, p[0], stride, p[1], n, *p[2:], out.data_ptr(), ostride, olens.data_ptr(), sigs.data_ptr(),
            st.data_ptr(), None)
    assert rc == 0, store.lib.gvs_last_error(store.h)
    out, olens = out.cpu().numpy().reshape(n, ostride), olens.cpu().numpy().view(np.uint32)
    return [out[k, :olens[k]].tobytes() for k in range(n)], st.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("form", ["host", "device"])
def test_channel_with_chachapoly_equals_seeded_on_the_plaintext(channel_batch, form):  # noqa: F811
    b = channel_batch  # its IV rows serve as nonces: any 12 bytes do
    if form == "device":
        pytest.importorskip("torch")
    sealed = [seal(b["keys"][0][k].tobytes(), b["ivs"][0][k].tobytes(), b"", m) for k, m in enumerate(b["msgs"])]
    for k in b["bad"]:
        sealed[k] = flip(sealed[k], len(sealed[k]) - 7, 0x20)
    chan, twin = small_store(ed25519_auth=b["ed"]), small_store(ed25519_auth=b["ed"])
    try:
        for lo, hi in ((0, 100), (100, 200)):  # the second batch holds the spoiled tags
            bad = [k - lo for k in b["bad"] if lo <= k < hi]
            chan.set_timing(form == "host")
            got, st = channel_call(chan, b, lo, hi, form, CP, sealed[lo:hi])
            if form == "host":
                names = list(chan.last_timings())
                assert names[0] == "chachapoly_open" and names[-1] == "chachapoly_seal", names
            plain = [b"" if k in bad else m for k, m in enumerate(b["msgs"][lo:hi])]
            want, _, wst, _ = twin.process_wire_batch_seeded(plain, b["times"][lo:hi], b["seeds"][lo:hi], b["draws"][lo:hi])
            wst = wst.copy()
            wst[bad] = abi.WIRE_BAD_CHANNEL_TAG
            assert st.tolist() == wst.tolist()
            assert all(not got[k] for k in bad)
            opened = [open_(b["keys"][1][lo + k].tobytes(), b["ivs"][1][lo + k].tobytes(), b"", got[k]) if got[k] else b""
                      for k in range(hi - lo)]
            assert opened == want
        assert chan.stats() == twin.stats()
        assert chan.dump_messages().tobytes() == twin.dump_messages().tobytes()
    finally:
        chan.close()
        twin.close()


@pytest.mark.parametrize("form", ["host", "device"])
def test_channel_with_aesgcm_returns_the_old_call_s_bytes(channel_batch, form):  # noqa: F811
    b = channel_batch
    if form == "device":
        pytest.importorskip("torch")
    new, old = small_store(ed25519_auth=b["ed"]), small_store(ed25519_auth=b["ed"])
    try:
        got, st = channel_call(new, b, 100, 200, form, abi.CIPHER_AESGCM, b["sealed"][100:200])
        want, wst = channel_call(old, b, 100, 200, form, None, b["sealed"][100:200])
        assert got == want and st.tolist() == wst.tolist() and any(got)
        assert new.dump_messages().tobytes() == old.dump_messages().tobytes()
    finally:
        new.close()
        old.close()


# --------------------------------------------------------- the responder

def handshakes(n, p2, seed):
    rng = random.Random(f"cp/{n}/{p2}/{seed}")
    s, prologue = rng.randbytes(32), rng.randbytes(seed % 3 * 20)
    eph = [rng.randbytes(32) for _ in range(n)]
    inis = [noise.Initiator(rng.randbytes(32), rng.randbytes(32), prologue=prologue, cipher=CP) for _ in range(n)]
    msg1 = [ini.write_message1(rng.randbytes(k % 5 * 16)) for k, ini in enumerate(inis)]
    pays = [rng.randbytes(p2) for _ in range(n)]
    return s, prologue, eph, inis, msg1, pays


def check_respond(got, want):
    msg2, rk, sk, hh, ok, slab = got
    for k, w in enumerate(want):
        if w is None:
            assert not ok[k] and msg2[k] == b"" and not (slab[k].any() or rk[k].any() or sk[k].any() or hh[k].any())
        else:
            assert ok[k] and (msg2[k], rk[k].tobytes(), sk[k].tobytes(), hh[k].tobytes()) == w, k


@pytest.mark.parametrize("n,p2", [(n, p) for n in (1, 63, 64, 65) for p in (0, 32, 960, 2048)])
def test_responder_matches_the_reference(store, n, p2):
    s, prologue, eph, _, msg1, pays = handshakes(n, p2, n + p2)
    want = [noise.respond(s, eph[k], msg1[k], pays[k], prologue=prologue, cipher=CP) for k in range(n)]
    check_respond(store.noise_ix_respond(s, arr(eph, 32), msg1, pays, prologue, cipher=CP), want)


def test_responder_device_form_a_spoiled_message_and_five_clients(store):
    torch = pytest.importorskip("torch")
    s, prologue, eph, inis, msg1, pays = handshakes(5, 40, 7)
    msg1[3] = bytes(32) + msg1[3][32:]  # a small-order ephemeral key
    want = [noise.respond(s, eph[k], msg1[k], pays[k], prologue=prologue, cipher=CP) for k in range(5)]
    assert want[3] is None and all(w is not None for k, w in enumerate(want) if k != 3)
    host = store.noise_ix_respond(s, arr(eph, 32), msg1, pays, prologue, cipher=CP)
    check_respond(host, want)
    slab, lens, stride = store._wire_slab(msg1, 128)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_e, d_m1, d_l1, d_p = up(arr(eph, 32)), up(slab), up(lens).view(torch.int32), up(arr(pays, 40))
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")
    m2, rk, sk, hh = z(5, 144), z(5, 32), z(5, 32), z(5, 64)
    m2l, ok = (torch.zeros(5, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    store.noise_ix_respond_device(s, d_e, d_m1, d_l1, d_p, 40, m2, m2l, rk, sk, hh, ok, prologue=prologue, cipher=CP)
    m2, m2l = m2.cpu().numpy(), m2l.cpu().numpy()
    check_respond(([m2[k, :m2l[k]].tobytes() for k in range(5)], rk.cpu().numpy(), sk.cpu().numpy(), hh.cpu().numpy(),
                   ok.cpu().numpy().astype(bool), m2), want)
    # the four good clients finish and exchange a request through the device's cipher
    live = [k for k in range(5) if k != 3]
    keys = {k: inis[k].read_message2(host[0][k])[:2] for k in live}
    assert all(inis[k].payload2 == pays[k] for k in live)
    n0 = [abi.noise_nonce_chachapoly(0)] * 4
    reqs = [seal(keys[k][0], n0[0], b"", b"request %d" % k) for k in live]
    back, okk, _ = store.chachapoly_open(host[1][live], arr(n0, 12), reqs)
    assert okk.all() and back == [b"request %d" % k for k in live]
    resp = store.chachapoly_seal(host[2][live], arr(n0, 12), [b"response %d" % k for k in live])
    assert [open_(keys[k][1], n0[0], b"", r) for k, r in zip(live, resp)] == [b"response %d" % k for k in live]


def test_responder_with_aesgcm_returns_the_old_call_s_bytes(store):
    from test_aead import open_ as gcm_open, seal as gcm_seal
    rng = random.Random(5)
    s, eph = rng.randbytes(32), [rng.randbytes(32) for _ in range(5)]
    msg1 = [noise.Initiator(rng.randbytes(32), rng.randbytes(32), gcm_seal, gcm_open).write_message1() for _ in range(5)]
    new = store.noise_ix_respond(s, arr(eph, 32), msg1, b"x" * 33, cipher=abi.CIPHER_AESGCM)
    old = store.noise_ix_respond(s, arr(eph, 32), msg1, b"x" * 33)
    assert new[0] == old[0] and all(old[0]) and all(np.array_equal(a, c) for a, c in zip(new[1:], old[1:]))


def test_misuse_is_invalid_arg(store):
    b = np.zeros(4096, np.uint8)
    p, u = b.ctypes.data, np.zeros(4, np.uint32).ctypes.data
    lib, h, bad = store.lib, store.h, abi.GVS_ERR_INVALID_ARG
    assert lib.gvs_noise_ix_respond_cipher(h, 2, bytes(32), b"", 0, p, p, 64, u, None, 0, 0, 1, p, 96, u, p, p, p, u) == bad
    assert lib.gvs_process_wire_batch_channel_cipher(h, 2, p, 1120, u, 1, p, None, None, p, p, p, p, p, 1072, u, None,
                                                     None, None) == bad
    for in_stride, out_stride in ((24, 64), (64, 40), (0, 64), (64, 2080)):  # not whole blocks, none, over the maximum
        assert lib.gvs_chachapoly_seal(h, p, p, None, 16, None, p, in_stride, u, 1, p, out_stride, u) == bad
        assert lib.gvs_chachapoly_open(h, p, p, None, 16, None, p, in_stride, u, 1, p, out_stride, u, u) == bad
    assert lib.gvs_chachapoly_seal(h, p, p, p, 24, u, p, 64, u, 1, p, 64, u) == bad  # the AAD stride
