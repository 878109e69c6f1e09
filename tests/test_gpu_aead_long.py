"""GPU parity of the long channel cipher (include/gvstore.h gvs_aead_open_long /
gvs_aead_seal_long, kernel k_aead_long of gvs_aead_long.h) against the
Python-integer AES-256-GCM of tests/test_aead.py, at the lengths of
tests/test_aead_long.py: around the short path's limit, around one and two
strides of the hash schedule, and a whole Noise message."""
import random

import numpy as np
import pytest

from grapevine_amd import abi, noise

from test_aead import open_, seal
from test_aead_long import AADS, batch, flip, text_lens
from test_gpu_challenge import small_store

pytestmark = pytest.mark.gpu
WIDE = 65536  # the widest stride: every slot far wider than most texts


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


def arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)


def device_call(store, do_seal, keys, ivs, aads, msgs):
    """The device form on torch tensors with WIDE strides, the output between
    two 64-byte guards, all pre-filled with 0xA5 -> (slots, lengths, ok, guards)."""
    import torch
    n = len(msgs)
    up = lambda a: torch.from_numpy(np.array(a)).cuda()
    slab, lens, _ = store._wire_slab(msgs, WIDE)
    aad, alens, _ = store._wire_slab(aads, 64) if aads else (None, None, 0)
    d = [up(x) if x is not None else None for x in (arr(keys, 32), arr(ivs, 12), aad, alens, slab, lens)]
    ptr = lambda x: x.data_ptr() if x is not None else None
    out = torch.full((128 + n * WIDE,), 0xA5, dtype=torch.uint8, device="cuda")
    olens, ok = (torch.full((n,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    fn = store.lib.gvs_aead_seal_long_device if do_seal else store.lib.gvs_aead_open_long_device
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
    keys, ivs, aads, pts, want = [x[4:4 + n] if n else x for x in batch(aad_len)]
    aads = aads if aad_len else None
    if form == "host":
        assert store.aead_seal_long(arr(keys, 32), arr(ivs, 12), pts, aads) == want
        back, ok, slab = store.aead_open_long(arr(keys, 32), arr(ivs, 12), want, aads)
        assert ok.all() and back == pts, [k for k in range(len(pts)) if back[k] != pts[k]]
        assert all(not slab[k, len(p):].any() for k, p in enumerate(pts))
        return
    pytest.importorskip("torch")
    for do_seal, src, res in ((True, pts, want), (False, want, pts)):
        slots, lens, ok, guards = device_call(store, do_seal, keys, ivs, aads, src)
        assert lens.tolist() == [len(r) for r in res] and (do_seal or ok.all())
        for k, r in enumerate(res):  # the result, then zeros to the stride
            assert slots[k, :len(r)].tobytes() == r and not slots[k, len(r):].any(), (do_seal, len(r))
        assert (guards == 0xA5).all()


@pytest.mark.parametrize("what", ["ct_first", "ct_last", "tag", "aad", "iv"])
@pytest.mark.parametrize("length", [2049, abi.AEAD_LONG_TEXT_MAX])
def test_rejection_spares_the_neighbours(store, length, what):
    """Message 2 of 5 is spoiled; it alone must fail, with a zeroed slot."""
    at = text_lens(20).index(length)
    keys, ivs, aads, pts, msgs = [[x[k] for k in (1, 3, at, 5, 2)] for x in batch(20)]
    if what == "ct_first":
        msgs[2] = flip(msgs[2], 0)
    elif what == "ct_last":
        msgs[2] = flip(msgs[2], length - 1, 0x80)
    elif what == "tag":
        msgs[2] = flip(msgs[2], length + 15)
    elif what == "aad":
        aads[2] = flip(aads[2], 19)
    else:
        ivs[2] = flip(ivs[2], 11)
    back, ok, slab = store.aead_open_long(arr(keys, 32), arr(ivs, 12), msgs, aads)
    assert ok.tolist() == [k != 2 for k in range(5)]
    assert back == [b"" if k == 2 else pts[k] for k in range(5)]
    assert not slab[2].any()


# (text length, in_stride, out_stride, n, aad_stride)
MISUSE = {"text": (65520, 65520, 65536, 1, 0), "stride_over": (16, 65552, 65552, 1, 0), "stride_odd": (16, 24, 48, 1, 0),
          "staging": (16, WIDE, WIDE, 1000, 144000)}  # 1000 x (2 x 65536 + 144000) B > 256 MiB


@pytest.mark.parametrize("what", list(MISUSE))
def test_misuse_is_refused(store, what):
    text, in_stride, out_stride, n, aad_stride = MISUSE[what]
    assert what != "staging" or n * (in_stride + out_stride + aad_stride) > abi.AEAD_LONG_STAGE_MAX
    z = lambda *shape: np.zeros(shape, np.uint8)
    keys, ivs, aad = z(n, 32), z(n, 12), z(n, aad_stride) if aad_stride else None
    src, out, olens = z(n, in_stride), z(n, out_stride), np.zeros(n, np.uint32)
    lens, alens = np.full(n, text, np.uint32), np.zeros(n, np.uint32)
    call = lambda m: store.lib.gvs_aead_seal_long(
        store.h, keys.ctypes.data, ivs.ctypes.data, aad.ctypes.data if aad is not None else None, max(aad_stride, 16),
        alens.ctypes.data, src.ctypes.data, in_stride, lens.ctypes.data, m, out.ctypes.data, out_stride,
        olens.ctypes.data)
    assert call(n) == abi.GVS_ERR_INVALID_ARG
    if what == "staging":  # the same call is fine with fewer messages
        assert call(2) == 0 and olens[:2].tolist() == [32, 32]


def test_short_lengths_equal_the_short_path(store):
    keys, ivs, aads, pts, want = [x[:4] for x in batch(20)]  # 0, 1, 16 and 2 048 bytes
    assert store.aead_seal_long(arr(keys, 32), arr(ivs, 12), pts, aads) == \
        store.aead_seal(arr(keys, 32), arr(ivs, 12), pts, aads) == want


def test_evidence_after_the_handshake(store):
    """Five initiators complete against the device; 5 000 bytes of evidence
    sealed on the device under send_keys open at the initiators, and their
    5 000 bytes open on the device under recv_keys."""
    rng, n = random.Random(17), 5
    s, pro, eph = rng.randbytes(32), b"evidence", [rng.randbytes(32) for _ in range(n)]
    inis = [noise.Initiator(rng.randbytes(32), rng.randbytes(32), seal, open_, pro) for _ in range(n)]
    msgs, rk, sk, _, ok, _ = store.noise_ix_respond(s, arr(eph, 32), [i.write_message1() for i in inis], b"", pro)
    assert ok.all()
    k12 = [i.read_message2(m)[:2] for i, m in zip(inis, msgs)]
    iv0, ivs = abi.noise_iv(0), arr([abi.noise_iv(0)] * n, 12)
    evidence = [rng.randbytes(5000) for _ in range(n)]
    for (k1, k2), e, c in zip(k12, evidence, store.aead_seal_long(sk, ivs, evidence)):
        assert open_(k2, iv0, b"", c) == e and open_(k1, iv0, b"", c) is None
    back, good, _ = store.aead_open_long(rk, ivs, [seal(k1, iv0, b"", e) for (k1, _), e in zip(k12, evidence)])
    assert good.all() and back == evidence
