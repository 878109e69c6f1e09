"""GPU parity of the long ChaCha20-Poly1305 calls (include/gvstore.h
gvs_chachapoly_open_long / gvs_chachapoly_seal_long, kernel k_chachapoly_long
of gvs_chachapoly_long.h) against grapevine_amd/chachapoly.py at the lengths
of tests/test_chachapoly_long.py, and of the long responder with the suite
chosen (gvs_noise_ix_respond_long_cipher) against grapevine_amd/noise.py."""
import functools
import random

import numpy as np
import pytest

from grapevine_amd import abi, noise
from grapevine_amd.chachapoly import open_, seal

from test_chachapoly_long import AADS, TEXT_LENS, batch, flip
from test_gpu_challenge import small_store
from test_gpu_noise import SPOIL, check
from test_noise import EDGE

pytestmark = pytest.mark.gpu
CP = abi.CIPHER_CHACHAPOLY
WIDE = 65536  # the widest stride: every slot far wider than most texts
up16 = lambda v: -(-v // 16) * 16


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


def arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)


def device_call(store, do_seal, keys, nonces, aads, msgs):
    """The device form on torch tensors with WIDE strides, the output between
    two 64-byte guards, all pre-filled with 0xA5 -> (slots, lengths, ok, guards)."""
    import torch
    n = len(msgs)
    up = lambda a: torch.from_numpy(np.array(a)).cuda()
    slab, lens, _ = store._wire_slab(msgs, WIDE)
    aad, alens, _ = store._wire_slab(aads, 64) if aads else (None, None, 0)
    d = [up(x) if x is not None else None for x in (arr(keys, 32), arr(nonces, 12), aad, alens, slab, lens)]
    ptr = lambda x: x.data_ptr() if x is not None else None
    out = torch.full((128 + n * WIDE,), 0xA5, dtype=torch.uint8, device="cuda")
    olens, ok = (torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    fn = store.lib.gvs_chachapoly_seal_long_device if do_seal else store.lib.gvs_chachapoly_open_long_device
    rc = fn(store.h, ptr(d[0]), ptr(d[1]), ptr(d[2]), 64, ptr(d[3]), ptr(d[4]), WIDE, ptr(d[5]), n,
            out.data_ptr() + 64, WIDE, olens.data_ptr(), *([] if do_seal else [ok.data_ptr()]))
    assert rc == 0, store.lib.gvs_last_error(store.h)
    out = out.cpu().numpy()
    return (out[64:-64].reshape(n, WIDE), olens.cpu().numpy().view(np.uint32), ok.cpu().numpy() == 1,
            np.concatenate([out[:64], out[-64:]]))


# every length in one call, host and device; n = 1 and 3 from the batch's middle (2 049 bytes onwards)
CASES = [(a, form, None) for a in AADS for form in ("host", "device")] + [(20, "host", 1), (20, "device", 3)]


@pytest.mark.parametrize("aad_len,form,n", CASES)
def test_seal_and_open_match_the_reference(store, aad_len, form, n):
    keys, nonces, aads, pts, want = [x[7:7 + n] if n else x for x in batch(aad_len)]
    aads = aads if aad_len else None
    if form == "host":
        assert store.chachapoly_seal_long(arr(keys, 32), arr(nonces, 12), pts, aads) == want
        back, ok, slab = store.chachapoly_open_long(arr(keys, 32), arr(nonces, 12), want, aads)
        assert ok.all() and back == pts, [k for k in range(len(pts)) if back[k] != pts[k]]
        assert all(not slab[k, len(p):].any() for k, p in enumerate(pts))
        return
    pytest.importorskip("torch")
    for do_seal, src, res in ((True, pts, want), (False, want, pts)):
        slots, lens, ok, guards = device_call(store, do_seal, keys, nonces, aads, src)
        assert lens.tolist() == [len(r) for r in res] and (do_seal or ok.all())
        for k, r in enumerate(res):  # the result, then zeros to the stride
            assert slots[k, :len(r)].tobytes() == r and not slots[k, len(r):].any(), (do_seal, len(r))
        assert (guards == 0xA5).all()


@pytest.mark.parametrize("what", ["ct_first", "ct_last", "tag", "aad", "nonce"])
@pytest.mark.parametrize("length", [2049, abi.AEAD_LONG_TEXT_MAX])
def test_rejection_spares_the_neighbours(store, length, what):
    """Message 2 of 5 is spoiled; it alone must fail, with a zeroed slot."""
    at = TEXT_LENS.index(length)
    keys, nonces, aads, pts, msgs = [[x[k] for k in (1, 3, at, 5, 2)] for x in batch(20)]
    if what in ("aad", "nonce"):
        (aads if what == "aad" else nonces)[2] = flip((aads if what == "aad" else nonces)[2], 11)
    else:
        msgs[2] = flip(msgs[2], {"ct_first": 0, "ct_last": length - 1, "tag": length + 15}[what], 0x80)
    back, ok, slab = store.chachapoly_open_long(arr(keys, 32), arr(nonces, 12), msgs, aads)
    assert ok.tolist() == [k != 2 for k in range(5)]
    assert back == [b"" if k == 2 else pts[k] for k in range(5)]
    assert not slab[2].any()


def test_short_lengths_equal_the_short_path(store):
    keys, nonces, aads, pts, want = [[x[k] for k in (0, 1, 2, 6)] for x in batch(20)]  # 0, 1, 16 and 2 048 bytes
    assert [len(p) for p in pts] == [0, 1, 16, 2048]
    assert store.chachapoly_seal_long(arr(keys, 32), arr(nonces, 12), pts, aads) == \
        store.chachapoly_seal(arr(keys, 32), arr(nonces, 12), pts, aads) == want


# (text length, in_stride, out_stride, n, aad_stride)
MISUSE = {"text": (65520, 65520, 65536, 1, 0), "stride_over": (16, 65552, 65552, 1, 0), "stride_odd": (16, 24, 48, 1, 0),
          "staging": (16, WIDE, WIDE, 1000, 144000)}  # 1000 x (2 x 65536 + 144000) B > 256 MiB


@pytest.mark.parametrize("what", list(MISUSE))
def test_misuse_is_refused(store, what):
    text, in_stride, out_stride, n, aad_stride = MISUSE[what]
    assert what != "staging" or n * (in_stride + out_stride + aad_stride) > abi.AEAD_LONG_STAGE_MAX
    z = lambda *shape: np.zeros(shape, np.uint8)
    keys, nonces, aad = z(n, 32), z(n, 12), z(n, aad_stride) if aad_stride else None
    src, out, olens = z(n, in_stride), z(n, out_stride), np.zeros(n, np.uint32)
    lens, alens = np.full(n, text, np.uint32), np.zeros(n, np.uint32)
    call = lambda m: store.lib.gvs_chachapoly_seal_long(
        store.h, keys.ctypes.data, nonces.ctypes.data, aad.ctypes.data if aad is not None else None,
        max(aad_stride, 16), alens.ctypes.data, src.ctypes.data, in_stride, lens.ctypes.data, m, out.ctypes.data,
        out_stride, olens.ctypes.data)
    assert call(n) == abi.GVS_ERR_INVALID_ARG
    if what == "staging":  # the same call is fine with fewer messages
        assert call(2) == 0 and olens[:2].tolist() == [32, 32]


# --------------------------------------------------------- the long responder

@functools.lru_cache(None)
def shakes(n, p2, shared=False, cipher=CP):
    """n handshakes under one static key and prologue, made once: payloads of
    p2 bytes (one for all when `shared`); `want` is noise.respond's answer."""
    rng = random.Random(f"cpl/{n}/{p2}")
    s, prologue, eph = rng.randbytes(32), rng.randbytes(47), [rng.randbytes(32) for _ in range(n)]
    gcm = cipher != CP
    if gcm:
        from test_aead import open_ as gcm_open, seal as gcm_seal
    inis = [noise.Initiator(rng.randbytes(32), rng.randbytes(32), *((gcm_seal, gcm_open) if gcm else ()),
                            prologue=prologue, cipher=cipher) for _ in range(n)]
    msg1 = [ini.write_message1(rng.randbytes(EDGE[k % 4])) for k, ini in enumerate(inis)]
    pays = [rng.randbytes(p2)] * n if shared else [rng.randbytes(p2) for _ in range(n)]
    want = None if gcm else [noise.respond(s, eph[k], msg1[k], pays[k], prologue=prologue, cipher=CP) for k in range(n)]
    return dict(s=s, prologue=prologue, e=eph, ini=inis, msg1=msg1, payload=pays, want=want)


def respond_device(store, torch, b, p2, shared):
    """The device form: every stride larger than its element, 0xA5 between
    rows and in a 64-byte guard after the last message-2 row."""
    n = len(b["msg1"])
    def dev(items, stride, guard=0):
        a = np.full(n * stride + guard, 0xA5, np.uint8)
        for k, it in enumerate(items):
            a[k * stride:k * stride + len(it)] = np.frombuffer(it, np.uint8)
        return torch.from_numpy(a).cuda()
    view = lambda t, width, stride: t[:n * stride].view(n, stride)[:, :width]
    d_e, d_m1 = view(dev(b["e"], 32), 32, 32), view(dev(b["msg1"], 136), 131, 136)
    d_l1 = torch.tensor([len(m) for m in b["msg1"]], dtype=torch.int32, device="cuda")
    ps, ms = up16(p2) + 16, min(up16(96 + p2) + 32, 65536)
    d_pay = None
    if p2:
        d_pay = dev(b["payload"][:1], ps)[:p2] if shared else view(dev(b["payload"], ps), p2, ps)
    flat = dev([], ms, guard=64)
    d_m2 = view(flat, ms, ms)
    d_l2, d_ok = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    d_rk, d_sk = (torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    d_hh = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    store.noise_ix_respond_long_device(b["s"], d_e, d_m1, d_l1, d_pay, p2, d_m2, d_l2, d_rk, d_sk, d_hh, d_ok,
                                       prologue=b["prologue"], cipher=CP)
    slab, lens = d_m2.cpu().numpy(), d_l2.cpu().numpy()
    assert (flat[n * ms:].cpu().numpy() == 0xA5).all()
    return ([slab[k, :lens[k]].tobytes() for k in range(n)], d_rk.cpu().numpy(), d_sk.cpu().numpy(),
            d_hh.cpu().numpy(), d_ok.cpu().numpy(), slab)


@pytest.mark.parametrize("form", ("host", "device"))
@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("n,p2", [(n, p) for p in (0, 2049, 5000) for n in (1, 65)] + [(3, 65439)])
def test_respond_long_with_chachapoly_matches_the_reference(store, n, p2, shared, form):
    b = shakes(n, p2, shared)
    if form == "host":
        got = store.noise_ix_respond_long(b["s"], arr(b["e"], 32), b["msg1"], b["payload"][0] if shared else b["payload"],
                                          b["prologue"], msg2_stride=min(up16(96 + p2) + 16, 65536), cipher=CP)
    else:
        got = respond_device(store, pytest.importorskip("torch"), b, p2, shared)
    check(got, b["want"], p2)


def test_respond_long_with_aesgcm_returns_the_old_call_s_bytes(store):
    b = shakes(5, 2080, cipher=abi.CIPHER_AESGCM)
    args = (b["s"], arr(b["e"], 32), b["msg1"], b["payload"], b["prologue"])
    new, old = store.noise_ix_respond_long(*args, cipher=abi.CIPHER_AESGCM), store.noise_ix_respond_long(*args)
    assert new[0] == old[0] and all(len(m) == 96 + 2080 for m in old[0]) and old[4].all()
    assert all(np.array_equal(x, y) for x, y in zip(new[1:5], old[1:5]))


@pytest.mark.parametrize("what", sorted(SPOIL))
def test_a_bad_message_fails_alone(store, what):
    b = shakes(5, 2080)
    msg1 = list(b["msg1"])
    msg1[2] = SPOIL[what](msg1[2], random.Random(what))
    assert noise.respond(b["s"], b["e"][2], msg1[2], b["payload"][2], prologue=b["prologue"], cipher=CP) is None
    got = store.noise_ix_respond_long(b["s"], arr(b["e"], 32), msg1, b["payload"], b["prologue"], cipher=CP)
    check(got, b["want"][:2] + [None] + b["want"][3:], 2080)


def test_initiators_read_their_evidence_and_exchange_more(store):
    b, n, n0 = shakes(5, 5000), 5, abi.noise_nonce_chachapoly(0)
    msgs, rk, sk, hh, ok, _ = store.noise_ix_respond_long(b["s"], arr(b["e"], 32), b["msg1"], b["payload"],
                                                          b["prologue"], cipher=CP)
    assert ok.all()
    keys = [b["ini"][k].read_message2(msgs[k]) for k in range(n)]
    for k, (k1, k2, h) in enumerate(keys):
        assert (k1, k2, h) == (rk[k].tobytes(), sk[k].tobytes(), hh[k].tobytes())
        assert b["ini"][k].payload2 == b["payload"][k]
    rng, nonces = random.Random(23), arr([n0] * n, 12)
    evidence = [rng.randbytes(5000) for _ in range(n)]
    for (k1, k2, _), e, c in zip(keys, evidence, store.chachapoly_seal_long(sk, nonces, evidence)):
        assert open_(k2, n0, b"", c) == e and open_(k1, n0, b"", c) is None
    back, good, _ = store.chachapoly_open_long(rk, nonces, [seal(k1, n0, b"", e) for (k1, _, _), e in zip(keys, evidence)])
    assert good.all() and back == evidence


def test_an_unknown_cipher_is_refused(store):
    b = np.zeros(4096, np.uint8)
    p, u = b.ctypes.data, np.zeros(4, np.uint32).ctypes.data
    assert store.lib.gvs_noise_ix_respond_long_cipher(store.h, 2, bytes(32), b"", 0, p, p, 64, u, None, 0, 0, 1, p, 96,
                                                      u, p, p, p, u) == abi.GVS_ERR_INVALID_ARG
