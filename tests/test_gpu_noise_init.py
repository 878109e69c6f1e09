"""GPU parity of the Noise IX initiator (include/gvstore.h gvs_noise_ix_initiate
and gvs_noise_ix_finish: k_x25519, k_noise_ixi<M1|A|B|C> of gvs_noise_init.h
and the opening ciphers) against grapevine_amd/noise.py's `Initiator`, bit for
bit in both suites; whole batches of handshakes completed device to device
against gvs_noise_ix_respond_cipher_device; the per-item rejections."""
import functools
import random

import numpy as np
import pytest

from grapevine_amd import abi, noise

from test_aead import open_, seal
from test_gpu_challenge import small_store
from test_noise_init import CIPHERS, P2, SPOIL

pytestmark = pytest.mark.gpu

SIZES = (1, 17, 65)  # one quad; past a wavefront's 16 quads; past a workgroup's 64


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


@functools.lru_cache(None)
def batch(cipher, n, plen):
    """n handshakes by the Python reference under one static key, made once:
    prologue and payload 1 of plen bytes, item k's payload 2 of P2[k % 6]."""
    rng = random.Random(f"gpu-init/{cipher}/{plen}")
    aead = (seal, open_) if cipher == abi.CIPHER_AESGCM else (None, None)
    b = dict(s=rng.randbytes(32), r_s=rng.randbytes(32), prologue=rng.randbytes(plen), e=[], pay1=[], msg1=[],
             state=[], msg2=[], want=[])
    for k in range(n):
        e, r_e, pay1, pay2 = rng.randbytes(32), rng.randbytes(32), rng.randbytes(plen), rng.randbytes(P2[k % len(P2)])
        ini = noise.Initiator(b["s"], e, *aead, b["prologue"], cipher)
        b["msg1"].append(ini.write_message1(pay1))
        b["state"].append(ini.ss.h)
        b["msg2"].append(noise.respond(b["r_s"], r_e, b["msg1"][k], pay2, aead[0], b["prologue"], cipher)[0])
        k1, k2, h = ini.read_message2(b["msg2"][k])
        b["want"].append((True, ini.rs, pay2, k1, k2, h))
        b["e"].append(e)
        b["pay1"].append(pay1)
    return b


NONE = (False, bytes(32), b"", bytes(32), bytes(32), bytes(64))


def rows(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width)


def finished(got):
    """noise_ix_finish's result as one tuple per handshake, the slots checked to be written whole"""
    rs, pays, sk, rk, hh, ok, slab = got
    assert all(not slab[k, len(p):].any() for k, p in enumerate(pays))
    return [(bool(ok[k]), rs[k].tobytes(), pays[k], sk[k].tobytes(), rk[k].tobytes(), hh[k].tobytes())
            for k in range(len(pays))]


def dev(torch, items, width, stride):
    """items as rows of a CUDA tensor, `stride` apart with 0xA5 between them"""
    a = np.full((len(items), stride), 0xA5, np.uint8)
    for k, it in enumerate(items):
        a[k, :len(it)] = np.frombuffer(it, np.uint8)
    return torch.from_numpy(a).cuda()[:, :width]


def filled(torch, n, *widths):
    """output tensors pre-filled with 0xA5 (a width of 0: an int32 vector)"""
    return tuple(torch.full((n, w) if w else (n,), 0xA5 if w else 7, dtype=torch.uint8 if w else torch.int32,
                            device="cuda") for w in widths)


@pytest.mark.parametrize("n,plen", [(n, 64) for n in SIZES] + [(5, 0)])
@pytest.mark.parametrize("cipher", CIPHERS)
def test_both_forms_match_the_python_initiator(store, cipher, n, plen):
    torch = pytest.importorskip("torch")
    b = batch(cipher, max(SIZES) if plen else n, plen)
    # the host forms, a static key per handshake
    statics, eph = rows([b["s"]] * n, 32), rows(b["e"][:n], 32)
    msg1, states, slab = store.noise_ix_initiate(statics, eph, b["pay1"][:n], b["prologue"], 64 + plen + 3, cipher)
    assert msg1 == b["msg1"][:n] and [s.tobytes() for s in states] == b["state"][:n]
    assert not slab[:, 64 + plen:].any()
    assert finished(store.noise_ix_finish(statics, eph, states, b["msg2"][:n], cipher=cipher)) == b["want"][:n]
    # the device forms: one static key for all, every stride larger than its element, 0xA5 in every output
    d_s, d_e = torch.from_numpy(np.frombuffer(b["s"], np.uint8).copy()).cuda(), dev(torch, b["e"][:n], 32, 32)
    d_pay = dev(torch, b["pay1"][:n], plen, plen + 5) if plen else None
    out1 = filled(torch, n, 64 + plen + 7, 0, 64)
    d_m2 = dev(torch, b["msg2"][:n], 96 + 2048 + 1, 96 + 2048 + 9)
    d_l2 = torch.tensor([len(m) for m in b["msg2"][:n]], dtype=torch.int32, device="cuda")
    out2 = filled(torch, n, 32, 2048 + 3, 0, 32, 32, 64, 0)
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    d_m1, d_l1, d_st = store.noise_ix_initiate(d_s, d_e, d_pay, b["prologue"], cipher=cipher, device=True, out=out1)
    slab, lens = d_m1.cpu().numpy(), d_l1.cpu().numpy()
    assert [slab[k, :lens[k]].tobytes() for k in range(n)] == b["msg1"][:n] and not slab[:, 64 + plen:].any()
    assert [s.tobytes() for s in d_st.cpu().numpy()] == b["state"][:n]
    rs, pay, pl, sk, rk, hh, ok = (t.cpu().numpy() for t in store.noise_ix_finish(
        d_s, d_e, d_st, d_m2, d_l2, cipher=cipher, device=True, out=out2))
    assert finished((rs, [pay[k, :pl[k]].tobytes() for k in range(n)], sk, rk, hh, ok, pay)) == b["want"][:n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cipher", CIPHERS)
def test_handshakes_complete_device_to_device(store, cipher, n):
    torch = pytest.importorskip("torch")
    rng = random.Random(f"d2d/{cipher}/{n}")
    r_s, prologue, p2 = rng.randbytes(32), rng.randbytes(33), 111
    u8 = lambda w: torch.from_numpy(np.frombuffer(rng.randbytes(n * w), np.uint8).reshape(n, w).copy()).cuda()
    d_s, d_e, d_re, d_pay1, d_pay2 = u8(32), u8(32), u8(32), u8(17), u8(p2)
    torch.cuda.synchronize()
    d_m1, d_l1, d_st = store.noise_ix_initiate(d_s, d_e, d_pay1, prologue, cipher=cipher, device=True)
    d_m2, d_l2, r_rk, r_sk, r_hh, r_ok = filled(torch, n, 96 + p2 + 5, 0, 32, 32, 64, 0)
    store.noise_ix_respond_device(r_s, d_re, d_m1, d_l1, d_pay2, p2, d_m2, d_l2, r_rk, r_sk, r_hh, r_ok,
                                  prologue=prologue, cipher=cipher)
    rs, pay, pl, sk, rk, hh, ok = store.noise_ix_finish(d_s, d_e, d_st, d_m2, d_l2, cipher=cipher, device=True)
    assert r_ok.cpu().numpy().all() and ok.cpu().numpy().all()
    assert torch.equal(sk, r_rk) and torch.equal(rk, r_sk) and torch.equal(hh, r_hh) and sk.any() and rk.any()
    assert (rs.cpu().numpy() == np.frombuffer(noise.x25519(r_s), np.uint8)).all()
    assert (pl.cpu().numpy() == p2).all() and torch.equal(pay[:, :p2], d_pay2) and not pay[:, p2:].any()
    # the transport: what the initiator seals under send_keys the responder opens under its recv_keys
    texts, iv = [rng.randbytes(1099) for _ in range(n)], np.zeros((n, 12), np.uint8)
    seal_, open__ = (store.aead_seal, store.aead_open) if cipher == abi.CIPHER_AESGCM else \
        (store.chachapoly_seal, store.chachapoly_open)
    opened, good, _ = open__(r_rk.cpu().numpy(), iv, seal_(sk.cpu().numpy(), iv, texts))
    assert good.all() and opened == texts


@pytest.mark.parametrize("cipher", CIPHERS)
def test_a_bad_message_fails_alone(store, cipher):
    b, n = batch(cipher, max(SIZES), 64), 8
    msg2, want = list(b["msg2"][:n]), list(b["want"][:n])
    for k, what in enumerate(sorted(SPOIL), 1):  # items 1 .. 5; 0, 6 and 7 stay clean
        msg2[k], want[k] = SPOIL[what](msg2[k]), NONE
    got = store.noise_ix_finish(b["s"], rows(b["e"][:n], 32), rows(b["state"][:n], 64), msg2, cipher=cipher)
    assert finished(got) == want


def test_misuse_is_refused(store):
    lib, h, bad = store.lib, store.h, abi.GVS_ERR_INVALID_ARG
    buf = np.zeros(4096, np.uint8)  # never read: every call fails its argument check
    p = buf.ctypes.data
    call = lambda cipher=0, plen=0, stride=128, lens=p, n=1: lib.gvs_noise_ix_initiate(
        h, cipher, b"", 0, p, 0, p, p, 0, plen, n, p, stride, lens, p)
    assert call(cipher=2) == bad and call(plen=65, stride=256) == bad and call(stride=63) == bad
    assert call(lens=None) == bad
    assert lib.gvs_noise_ix_finish(h, 2, p, 0, p, p, p, 96, p, 1, p, p, 0, p, p, p, p, p) == bad
    assert lib.gvs_noise_ix_finish(h, 0, p, 0, p, p, p, 95, p, 1, p, p, 0, p, p, p, p, p) == bad
    assert lib.gvs_noise_ix_finish(h, 0, p, 0, p, p, p, 96, p, 1, p, p, 0, p, p, p, p, None) == bad
    assert call(n=0) == 0  # n = 0 is a no-op
    # the store serves a batch afterwards
    b = batch(abi.CIPHER_AESGCM, max(SIZES), 64)
    assert store.noise_ix_initiate(b["s"], rows(b["e"][:3], 32), b["pay1"][:3], b["prologue"])[0] == b["msg1"][:3]
