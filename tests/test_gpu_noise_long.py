"""GPU parity of the long Noise IX responder (gvs_noise_ix_respond_long: the
short chain up to phase B, then k_aead_long<true> and k_noise_ix_tail of
gvs_noise_long.h) against grapevine_amd/noise.py's `respond`, bit for bit."""
import functools
import random

import numpy as np
import pytest

from grapevine_amd import abi, noise
from grapevine_amd.store import ObliviousStore

from test_aead import open_, seal
from test_gpu_challenge import small_store
from test_gpu_noise import SPOIL, check, rows
from test_noise import EDGE

pytestmark = pytest.mark.gpu

# (n, p2): the Python cipher is slow, so Noise's limit runs at n = 1 and 3 only
CASES = [(n, p) for p in (0, 2049, 2079, 2080, 5000) for n in (1, 63, 64, 65)] + [(1, 65439), (3, 65439)]
OWN = (1, 62, 63, 64)  # the handshakes with a payload of their own (per-handshake rows); the others' are equal
up16 = lambda v: -(-v // 16) * 16


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


@functools.lru_cache(None)
def item(p2, k, shared=False):
    """Handshake k of the batch with p2-byte payloads, made once: one static
    key, prologue and common payload per p2; `want` is noise.respond's answer
    (with the common payload when `shared`)."""
    rng = random.Random(f"long/{p2}")
    s, prologue, common = rng.randbytes(32), rng.randbytes(47), rng.randbytes(p2)
    rng = random.Random(f"long/{p2}/{k}")
    ini = noise.Initiator(rng.randbytes(32), rng.randbytes(32), seal, open_, prologue)
    e, msg1, own = rng.randbytes(32), ini.write_message1(rng.randbytes(EDGE[k % 4])), rng.randbytes(p2)
    payload = own if k in OWN and not shared else common
    return dict(s=s, prologue=prologue, e=e, msg1=msg1, payload=payload, ini=ini,
                want=noise.respond(s, e, msg1, payload, seal, prologue))


def batch(p2, n, shared=False):
    its = [item(p2, k, shared and k in OWN) for k in range(n)]
    return dict(its[0], e=[i["e"] for i in its], msg1=[i["msg1"] for i in its], payload=[i["payload"] for i in its],
                ini=[i["ini"] for i in its], want=[i["want"] for i in its])


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("n,p2", CASES)
def test_respond_long_matches_the_reference(store, n, p2, shared):
    torch = pytest.importorskip("torch")
    b = batch(p2, n, shared)
    got = store.noise_ix_respond_long(b["s"], rows(b["e"], 32), b["msg1"], b["payload"][0] if shared else b["payload"],
                                      b["prologue"], msg2_stride=min(up16(96 + p2) + 16, 65536))
    check(got, b["want"], p2)
    # the device form: every stride larger than its element, 0xA5 between rows and in a guard after the last
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
                                       prologue=b["prologue"])
    slab, lens = d_m2.cpu().numpy(), d_l2.cpu().numpy()
    check(([slab[k, :lens[k]].tobytes() for k in range(n)], d_rk.cpu().numpy(), d_sk.cpu().numpy(),
           d_hh.cpu().numpy(), d_ok.cpu().numpy(), slab), b["want"], p2)
    assert (flat[n * ms:].cpu().numpy() == 0xA5).all()


@pytest.mark.parametrize("p2", (0, 32, 2048))
def test_long_and_short_calls_agree(store, p2):
    b = batch(p2, 5)
    args = (b["s"], rows(b["e"], 32), b["msg1"], b["payload"], b["prologue"])
    short, lng = store.noise_ix_respond(*args), store.noise_ix_respond_long(*args)
    assert short[0] == lng[0] and all(len(m) == 96 + p2 for m in lng[0])
    assert all((x == y).all() for x, y in zip(short[1:5], lng[1:5]))


@pytest.mark.parametrize("p2", (2080, 65439))
@pytest.mark.parametrize("what", sorted(SPOIL))
def test_a_bad_message_fails_alone(store, what, p2):
    b = batch(p2, 5)
    msg1 = list(b["msg1"])
    msg1[2] = SPOIL[what](msg1[2], random.Random(what))
    assert noise.respond(b["s"], b["e"][2], msg1[2], b["payload"][2], seal, b["prologue"]) is None
    got = store.noise_ix_respond_long(b["s"], rows(b["e"], 32), msg1, b["payload"], b["prologue"])
    check(got, b["want"][:2] + [None] + b["want"][3:], p2)


def test_initiators_read_their_evidence_and_the_channel_opens(store):
    b, n = batch(5000, 5), 5
    iv = rows([abi.noise_iv(0)] * n, 12)
    msgs, rk, sk, hh, ok, _ = store.noise_ix_respond_long(b["s"], rows(b["e"], 32), b["msg1"], b["payload"],
                                                          b["prologue"])
    assert ok.all()
    keys = [b["ini"][k].read_message2(msgs[k]) for k in range(n)]
    for k, (k1, k2, h) in enumerate(keys):
        assert (k1, k2, h) == (rk[k].tobytes(), sk[k].tobytes(), hh[k].tobytes())
        assert b["ini"][k].payload2 == b["payload"][k] and b["ini"][k].rs == noise.x25519(b["s"])
    # a request crosses under k1 / recv_keys, a response under send_keys / k2
    reqs = [b"request %d" % k for k in range(n)]
    opened, good, _ = store.aead_open(rk, iv, [seal(k1, abi.noise_iv(0), b"", r) for (k1, _, _), r in zip(keys, reqs)])
    assert good.all() and opened == reqs
    for (_, k2, _), c in zip(keys, store.aead_seal(sk, iv, reqs)):
        assert open_(k2, abi.noise_iv(0), b"", c) in reqs


def test_misuse_is_refused():
    torch = pytest.importorskip("torch")
    big = ObliviousStore(abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=2048))
    lib, h, bad = big.lib, big.h, abi.GVS_ERR_INVALID_ARG
    buf = np.zeros(4096, np.uint8)  # never read: every call fails its argument check
    p, key = buf.ctypes.data, bytes(32)
    call = lambda p2, m2s, n=1, pstride=0, fn=lib.gvs_noise_ix_respond_long, m2=p: fn(
        h, key, bytes(64), 0, p, p, 128, p, p, pstride, p2, n, m2, m2s, p, p, p, p, p)
    assert call(65440, 65536) == bad
    assert call(2080, 96 + 2080 + 8) == bad  # a stride that is no multiple of 16
    assert call(2080, 96 + 2080, n=2, pstride=2088) == bad
    assert call(2080, 96 + 2080 - 16) == bad  # below 96 + p2
    assert call(65439, 65552) == bad  # above 65 536
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda").data_ptr()
    assert call(32, 128, fn=lib.gvs_noise_ix_respond_long_device, m2=d + 8) == bad  # an unaligned device msg2
    # within a batch of this store, but 192 KiB each of sealed and staged payloads and slots pass the 256 MiB cap
    assert call(65439, 65536, n=1400, pstride=65440) == bad
    assert call(32, 128, n=0) == 0  # n = 0 is a no-op
    big.close()
