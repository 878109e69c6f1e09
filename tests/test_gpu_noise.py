"""GPU parity of the Noise IX responder (include/gvstore.h gvs_noise_ix_respond:
k_x25519, k_noise_ix<A|B|C> of gvs_noise.h and k_aead<true> in one call)
against grapevine_amd/noise.py's `respond`, bit for bit, its per-item
rejections, and a Python `Initiator` completing against the device and talking
through the channel cipher under the keys the call returned."""
import functools
import random

import numpy as np
import pytest

from grapevine_amd import abi, noise

from test_aead import open_, seal
from test_gpu_challenge import small_store
from test_noise import EDGE

pytestmark = pytest.mark.gpu

# one quad; either side of a wavefront's 16 quads; across a workgroup's 64
SIZES = (1, 15, 16, 17, 65)
PROLOGUE_LEN = {0: 0, 32: 47, 160: 64}  # by payload 2's length: one block, its last byte, two blocks
SPOIL = {"re": lambda m, rng: bytes(32) + m[32:],                           # small-order u = 0
         "rs": lambda m, rng: m[:32] + (1).to_bytes(32, "little") + m[64:],  # small-order u = 1
         "short": lambda m, rng: m[:63],
         "long": lambda m, rng: m[:64] + rng.randbytes(65)}


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


@functools.lru_cache(None)
def batch(p2):
    """65 handshakes under one static key and prologue, made once: item k's
    payload 1 has EDGE[k % 4] bytes.  `want` is noise.respond's answer."""
    rng = random.Random(900 + p2)
    b = dict(s=rng.randbytes(32), prologue=rng.randbytes(PROLOGUE_LEN[p2]), e=[], msg1=[], payload=[], ini=[], want=[])
    for k in range(max(SIZES)):
        ini = noise.Initiator(rng.randbytes(32), rng.randbytes(32), seal, open_, b["prologue"])
        b["ini"].append(ini)
        b["e"].append(rng.randbytes(32))
        b["msg1"].append(ini.write_message1(rng.randbytes(EDGE[k % 4])))
        b["payload"].append(rng.randbytes(p2))
        b["want"].append(noise.respond(b["s"], b["e"][k], b["msg1"][k], b["payload"][k], seal, b["prologue"]))
    return b


def rows(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width)


def check(got, want, p2):
    """(msg2 list, recv, send, hashes, ok, slab) against respond()'s results;
    None: a rejected item, everything zero."""
    msgs, rk, sk, hh, ok, slab = got
    for k, w in enumerate(want):
        m2, k1, k2, h = w or (b"", bytes(32), bytes(32), bytes(64))
        assert (bool(ok[k]), msgs[k], rk[k].tobytes(), sk[k].tobytes(), hh[k].tobytes()) == \
            (w is not None, m2, k1, k2, h), k
        assert not slab[k, len(m2):].any(), k  # the slot is written whole


@pytest.mark.parametrize("p2", sorted(PROLOGUE_LEN))
@pytest.mark.parametrize("n", SIZES)
def test_respond_matches_the_reference(store, n, p2):
    torch = pytest.importorskip("torch")
    b = batch(p2)
    got = store.noise_ix_respond(b["s"], rows(b["e"][:n], 32), b["msg1"][:n], b["payload"][:n], b["prologue"],
                                 msg2_stride=96 + p2 + 3)
    check(got, b["want"][:n], p2)
    # the device form: every stride larger than its element, 0xA5 between rows
    def dev(items, width, stride):
        a = np.full((n, stride), 0xA5, np.uint8)
        for k, it in enumerate(items):
            a[k, :len(it)] = np.frombuffer(it, np.uint8)
        return torch.from_numpy(a).cuda()[:, :width]
    d_e = dev(b["e"][:n], 32, 32)
    d_m1 = dev(b["msg1"][:n], 131, 136)
    d_l1 = torch.tensor([len(m) for m in b["msg1"][:n]], dtype=torch.int32, device="cuda")
    d_pay = dev(b["payload"][:n], p2, p2 + 5) if p2 else None
    d_m2 = torch.full((n, 96 + p2 + 7), 0xA5, dtype=torch.uint8, device="cuda")
    d_l2, d_ok = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    d_rk, d_sk = (torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    d_hh = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    store.noise_ix_respond_device(b["s"], d_e, d_m1, d_l1, d_pay, p2, d_m2, d_l2, d_rk, d_sk, d_hh, d_ok,
                                  prologue=b["prologue"])
    slab, lens = d_m2.cpu().numpy(), d_l2.cpu().numpy()
    check(([slab[k, :lens[k]].tobytes() for k in range(n)], d_rk.cpu().numpy(), d_sk.cpu().numpy(),
           d_hh.cpu().numpy(), d_ok.cpu().numpy(), slab), b["want"][:n], p2)


@pytest.mark.parametrize("what", sorted(SPOIL))
def test_a_bad_message_fails_alone(store, what):
    b = batch(32)
    msg1 = list(b["msg1"][:5])
    msg1[2] = SPOIL[what](msg1[2], random.Random(what))
    assert noise.respond(b["s"], b["e"][2], msg1[2], b["payload"][2], seal, b["prologue"]) is None
    got = store.noise_ix_respond(b["s"], rows(b["e"][:5], 32), msg1, b["payload"][:5], b["prologue"])
    check(got, b["want"][:2] + [None] + b["want"][3:5], 32)


def test_initiators_complete_and_the_channel_opens(store):
    b, n = batch(160), 5
    iv = rows([abi.noise_iv(0)] * n, 12)
    msgs, rk, sk, hh, ok, _ = store.noise_ix_respond(b["s"], rows(b["e"][:n], 32), b["msg1"][:n],
                                                     b["payload"][:n], b["prologue"])
    assert ok.all()
    keys = [b["ini"][k].read_message2(msgs[k]) for k in range(n)]
    for k, (k1, k2, h) in enumerate(keys):
        assert (k1, k2, h) == (rk[k].tobytes(), sk[k].tobytes(), hh[k].tobytes())
        assert b["ini"][k].payload2 == b["payload"][k] and b["ini"][k].rs == noise.x25519(b["s"])
    # a request sealed by the client under k1 opens under recv_keys, not under send_keys
    reqs = [b"request %d" % k for k in range(n)]
    sealed = [seal(k1, abi.noise_iv(0), b"", r) for (k1, _, _), r in zip(keys, reqs)]
    opened, good, _ = store.aead_open(rk, iv, sealed)
    assert good.all() and opened == reqs
    assert not store.aead_open(sk, iv, sealed)[1].any()
    # a response sealed under send_keys opens at the client under k2, not under k1
    resps = [b"response %d" % k for k in range(n)]
    for (k1, k2, _), r, c in zip(keys, resps, store.aead_seal(sk, iv, resps)):
        assert open_(k2, abi.noise_iv(0), b"", c) == r and open_(k1, abi.noise_iv(0), b"", c) is None


def test_misuse_is_refused(store):
    lib, h, bad = store.lib, store.h, abi.GVS_ERR_INVALID_ARG
    buf = np.zeros(4096, np.uint8)  # never read: every call fails its argument check
    p, key = buf.ctypes.data, bytes(32)
    call = lambda pro_len, p2, m2s, n=1, ok=p: lib.gvs_noise_ix_respond(
        h, key, bytes(64), pro_len, p, p, 128, p, p, 0, p2, n, p, m2s, p, p, p, p, ok)
    assert call(0, 2049, 96 + 2049) == bad
    assert call(0, 32, 95 + 32) == bad
    assert call(65, 32, 96 + 32) == bad
    assert call(0, 32, 96 + 32, ok=None) == bad  # a missing required array
    assert call(0, 32, 96 + 32, n=0) == 0  # n = 0 is a no-op
