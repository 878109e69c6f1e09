"""GPU: the double-buffered host pipeline under gvs_process_batches and
gvs_process_wire_batches[_seeded], and the single-call staging
beside it, against the contract of include/gvstore.h:

  * a refused call (the epoch limit) zeroes every output array, in all four
    K-batch calls;
  * a failing batch in the middle delivers the earlier batches' results (the
    oracle's) and zeroes every output array from its own offset on, on the
    store pipeline and on the wire pipeline, explicit and seeded;
  * pinned and pageable columns mixed on the wire pipeline, with both slots
    reused, give the oracle's bytes;
  * calls of different kinds back to back on one handle.
"""
import functools

import numpy as np
import pytest

from grapevine_amd import abi, wire
from grapevine_amd.store import ObliviousStore
from oracle import ffi

from parity import diff_responses
from test_gpu_wire import small_store, to_wire
from test_kv_oracle import SECRET

pytestmark = pytest.mark.gpu

LIMIT = 0xFFFFFF00  # the epoch limit (tests/test_gpu_epoch.py)


@pytest.mark.parametrize("call", ["gvs_process_batches", "gvs_process_batches_device",
                                  "gvs_process_wire_batches", "gvs_process_wire_batches_seeded"])
def test_refused_batches_zero_every_output(call):
    """include/gvstore.h: the K-batch calls zero the results of the batches
    they did not apply.  At the epoch limit that is every batch: the call
    returns GVS_ERR_EPOCH_EXHAUSTED with *applied == 0 and every output array
    (pre-filled with 0xAA) all zero.  Nothing runs on the device."""
    import ctypes
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024,
                          secret_key=SECRET, auth_storage=True)
    store = ObliviousStore(cfg)
    try:
        store._check(store.lib.gvs_test_set_epoch(store.h, LIMIT))
        counts, n = np.array([5, 3], np.uint32), 8
        applied = ctypes.c_uint32(7)
        filled = lambda *shape: np.full(shape, 0xAA, np.uint8)
        if call == "gvs_process_batches":
            outs = [filled(n, 1040)]
            rc = store.lib.gvs_process_batches(store.h, np.zeros(n, abi.REQUEST_DTYPE).ctypes.data,
                                               counts.ctypes.data, 2, outs[0].ctypes.data, ctypes.byref(applied))
        elif call == "gvs_process_batches_device":
            torch = pytest.importorskip("torch")
            d_in = torch.zeros(n * 1040, dtype=torch.uint8, device="cuda")
            d_out = torch.full((n * 1040,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = store.lib.gvs_process_batches_device(store.h, d_in.data_ptr(), counts.ctypes.data, 2,
                                                      d_out.data_ptr(), ctypes.byref(applied))
            outs = [d_out.cpu().numpy()]
        else:
            slab, lens, times = np.zeros((n, 1104), np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
            out, olens, status = filled(n, 1042), filled(n, 4), filled(n, 4)
            head = (store.h, slab.ctypes.data, 1104, lens.ctypes.data, counts.ctypes.data, 2, times.ctypes.data)
            tail = (out.ctypes.data, 1042, olens.ctypes.data, status.ctypes.data)
            outs = [out, olens, status]
            if call == "gvs_process_wire_batches":
                rc = store.lib.gvs_process_wire_batches(*head, None, *tail, ctypes.byref(applied))
            else:
                seeds, draws, chal = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint64), filled(n, 32)
                outs.append(chal)
                rc = store.lib.gvs_process_wire_batches_seeded(*head, seeds.ctypes.data, draws.ctypes.data,
                                                               *tail, chal.ctypes.data, ctypes.byref(applied))
        assert rc == abi.GVS_ERR_EPOCH_EXHAUSTED and applied.value == 0
        for k, o in enumerate(outs):
            assert not o.any(), f"output array {k} of {call} was not zeroed"
    finally:
        store.close()


def test_host_pipeline_failing_batch_delivers_and_zeroes():
    """A batch that overflows a router bucket stops the pipeline there: the
    batches before it are applied, it and the later ones are not, and the
    store goes on from that state.  The applied batches' responses are the
    oracle's, and the responses from the failing batch on are zero."""
    S = 4
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024,
                          shard_count=S, route_capacity=320)
    store, cl = ObliviousStore(cfg), ffi.Cluster(cfg)
    cl.seed(14)
    p = ffi.gen_params(n_identities=300)
    hot = ffi.gen_params(create=100, read=0, update=0, delete=0, hot=60, n_identities=300)
    ok = [cl.gen_batch(S * 1024, p) for _ in range(2)]
    want = [cl.process_batch(b) for b in ok]
    bad = cl.gen_batch(S * 1024, hot)
    assert cl.process_batch(bad) is None
    later = cl.gen_batch(S * 1024, p)
    import ctypes
    reqs = np.concatenate(ok + [bad, later])
    out = np.full(len(reqs) * 1040, 0xAA, np.uint8).view(abi.RESPONSE_DTYPE)
    counts = np.full(4, S * 1024, np.uint32)
    applied = ctypes.c_uint32(0)
    rc = store.lib.gvs_process_batches(store.h, reqs.ctypes.data, counts.ctypes.data, 4, out.ctypes.data,
                                       ctypes.byref(applied))
    assert rc == abi.GVS_ERR_BATCH_OVERFLOW and applied.value == 2
    assert store.stats()["messages"] == cl.messages
    assert store.stats()["batches"] == 2 and store.stats()["epoch"] == 2
    # the two applied batches' responses were delivered; from the failing batch on `out` is zero
    for k in range(2):
        d = diff_responses(out[k * S * 1024:(k + 1) * S * 1024], want[k], ok[k])
        assert not d, "\n".join(d)
    assert not out[2 * S * 1024:].view(np.uint8).any(), "unapplied responses must be zero"
    # `later` was not applied: it runs now, as the oracle's next batch
    got = store.process_batches([later])
    d = diff_responses(got[0], cl.process_batch(later), later)
    assert not d, "\n".join(d)
    assert store.dump_messages().tobytes() == cl.dump_messages().tobytes()


def call_wire_batches(store, slab, lens, counts, times, out, olens, status, seeds=None, draws=None,
                      chal_out=None):
    """gvs_process_wire_batches, or with seeds its seeded form, on the caller's
    own arrays -> (return code, batches applied)."""
    import ctypes
    applied = ctypes.c_uint32(0)
    ptr = lambda a: a.ctypes.data if a is not None else None
    head = (store.h, ptr(slab), slab.shape[1], ptr(lens), ptr(counts), len(counts), ptr(times))
    tail = (ptr(out), out.shape[1], ptr(olens), ptr(status))
    if seeds is None:
        rc = store.lib.gvs_process_wire_batches(*head, None, *tail, ctypes.byref(applied))
    else:
        rc = store.lib.gvs_process_wire_batches_seeded(*head, ptr(seeds), ptr(draws), *tail, ptr(chal_out),
                                                       ctypes.byref(applied))
    return rc, applied.value


def challenge(seed, draw):
    """Draw number `draw` of ChaCha20Rng(seed), by the Python block function."""
    from grapevine_amd import server as gs
    return gs.chacha20_block(seed, draw >> 1)[32 * (draw & 1):][:32]


@functools.lru_cache(maxsize=None)
def signers300():
    """A schnorrkel key for each of the oracle generator's 300 identities, a
    channel seed and a draw index of its own, the challenge at that draw and
    the identity's signature over it: {identity: (public key, seed, draw,
    challenge, signature)}, computed once."""
    import random
    from oracle import sr25519 as sr
    rng = random.Random(5)
    table = {}
    for i in range(300):
        x, seed = rng.randrange(1, sr.L), rng.randbytes(32)
        draw = (0, 1, 2, (1 << 33) - 1, 1 << 33, (1 << 64) - 1)[i % 6]
        chal = challenge(seed, draw)
        table[ffi.identity(i)] = (sr.public_key(x), seed, draw, chal, sr.sign(x, chal, rng.randrange(1, sr.L)))
    return table


# no key: the zero identity with a zero signature, which does not verify
NOBODY = (bytes(32), bytes(32), 0, challenge(bytes(32), 0), bytes(64))


def with_keys(b):
    """A generated batch with signers300's public keys for identities; a
    request of an identity without a key becomes the hard error the signature
    check makes of it."""
    keys = signers300()
    b["request_type"][[bytes(a) not in keys for a in b["auth_identity"]]] = 0
    for f in ("auth_identity", "recipient"):
        b[f] = [np.frombuffer(keys.get(bytes(v), (bytes(v),))[0], np.uint8) for v in b[f]]
    return b


def signing_columns(reqs):
    """Per request of a with_keys batch: its identity's signature, seed, draw
    index and challenge, as the arrays the seeded calls take and return."""
    by_pk = {v[0]: v for v in signers300().values()}
    who = [by_pk.get(bytes(a), NOBODY) for a in reqs["auth_identity"]]
    col = lambda i: np.array([np.frombuffer(w[i], np.uint8) for w in who]).reshape(len(who), -1)
    return col(4), col(1), np.array([w[2] for w in who], np.uint64), col(3)


@pytest.mark.parametrize("seeded", [False, True], ids=["explicit", "seeded"])
def test_wire_pipeline_failing_batch_delivers_and_zeroes(seeded):
    """gvs_process_wire_batches[_seeded] on a 4-shard store: a batch that
    overflows a router bucket stops the pipeline there (the batches before it
    applied and their results delivered, it and the later one not, and every
    output array zero from its first message on), as gvs_process_batches does.
    Seeded: the generator's identities become public keys, and every request
    carries its identity's signature over the challenge its seed and draw
    give, so the batches pass the check as they are; the oracle's cluster
    still finds `bad` overflowing and the others not."""
    S = 4
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024,
                          shard_count=S, route_capacity=320)
    store, cl = ObliviousStore(cfg), ffi.Cluster(cfg)
    cl.seed(15)
    p = ffi.gen_params(n_identities=300)
    hot = ffi.gen_params(create=100, read=0, update=0, delete=0, hot=60, n_identities=300)
    if seeded:
        from oracle import sr25519 as sr
        assert not sr.verify(NOBODY[0], NOBODY[3], NOBODY[4])

    def gen(params):
        b = cl.gen_batch(S * 1024, params)
        return with_keys(b) if seeded else b

    ok = [gen(p) for _ in range(2)]
    want = [[wire.encode_response(r) for r in cl.process_batch(b)] for b in ok]
    bad = gen(hot)
    assert cl.process_batch(bad) is None
    later = gen(p)
    batches = ok + [bad, later]
    reqs = np.concatenate(batches)
    sigs, seeds, draws, chal = signing_columns(reqs) if seeded else (None,) * 4

    def msgs(b, sigs=None):
        q = b.copy()
        q["request_type"][q["request_type"] == 0] = 0xFFFFFFFF  # still a hard error
        return wire.encode_requests(q, sigs)

    total, first_bad = 4 * S * 1024, 2 * S * 1024
    slab = np.zeros((total, 1104), np.uint8)
    slab[:, :wire.REQUEST_WIRE_BYTES] = msgs(reqs, sigs)
    lens = np.full(total, wire.REQUEST_WIRE_BYTES, np.uint32)
    counts = np.full(4, S * 1024, np.uint32)
    times = np.concatenate([b["timestamp"] for b in batches])
    out = np.full((total, 1042), 0xAA, np.uint8)
    olens, status = np.full(total, 0xAAAAAAAA, np.uint32), np.full(total, 0xAAAAAAAA, np.uint32)
    extra = {}
    if seeded:
        extra = dict(seeds=seeds, draws=draws, chal_out=np.full((total, 32), 0xAA, np.uint8))
    rc, applied = call_wire_batches(store, slab, lens, counts, times, out, olens, status, **extra)
    assert rc == abi.GVS_ERR_BATCH_OVERFLOW and applied == 2
    assert store.stats()["messages"] == cl.messages
    assert store.stats()["batches"] == 2
    # the two applied batches' results are the oracle's ...
    got = [out[k, :olens[k]].tobytes() for k in range(first_bad)]
    diff = [k for k in range(first_bad) if got[k] != (want[0] + want[1])[k]]
    assert not diff, f"{len(diff)} responses differ (first {diff[:5]})"
    unsigned = ~reqs["auth_identity"].any(axis=1) if seeded else np.zeros(total, bool)
    assert unsigned.sum() < 100
    assert (status[:first_bad] == np.where(unsigned, abi.WIRE_BAD_SIGNATURE, 0)[:first_bad]).all()
    # ... and from the failing batch on every output array is zero
    assert not out[first_bad:].any() and not olens[first_bad:].any() and not status[first_bad:].any()
    if seeded:
        assert (extra["chal_out"][:first_bad] == chal[:first_bad]).all()
        assert not extra["chal_out"][first_bad:].any()
    # `later` was not applied: it runs now, as the oracle's next batch
    w = cl.process_batch(later)
    lo = 3 * S * 1024
    rc, applied = call_wire_batches(store, slab[lo:], lens[lo:], counts[:1], times[lo:], out[lo:], olens[lo:],
                                    status[lo:], **{k: v[lo:] for k, v in extra.items()})
    assert (rc, applied) == (0, 1)
    assert [out[k, :olens[k]].tobytes() for k in range(lo, total)] == [wire.encode_response(r) for r in w]
    assert store.dump_messages().tobytes() == cl.dump_messages().tobytes()
    store.close()


@pytest.mark.parametrize("pin", ["in", "out", "both", "small"])
def test_wire_batches_mixed_pinned_columns(pin):
    """gvs_process_wire_batches with columns in pinned memory (gvs_host_alloc:
    copied without staging) beside pageable ones gives the same bytes as the
    oracle, batch by batch: the message slab, the response slab, both, or
    ("small") in_lens and times with both slabs pageable.  Four batches, so
    that both slots are reused, the last of one message."""
    store, model = small_store()
    model.seed(37)
    params = ffi.gen_params(n_identities=200, hot=10)
    rng = np.random.default_rng(23)
    sizes = [1024, 300, 1024, 1]
    msgs, times, wants = [], [], []
    for n in sizes:
        reqs = model.gen_batch(n, params)
        m = to_wire(reqs, rng)
        t = reqs["timestamp"].copy()
        q, _, _ = wire.decode_requests(m, timestamps=t, strict=False)
        wants += [wire.encode_response(r) for r in model.process_batch(q)]
        msgs += m
        times.append(t)
    total, stride = len(msgs), 1104

    def array(pinned, count, dtype):
        return store.host_array(count, dtype) if pinned else np.zeros(count, dtype)

    slab = array(pin in ("in", "both"), total * stride, np.uint8).reshape(total, stride)
    out = array(pin in ("out", "both"), total * 1042, np.uint8).reshape(total, 1042)
    lens, t = array(pin == "small", total, np.uint32), array(pin == "small", total, np.uint64)
    slab[:] = 0
    for k, m in enumerate(msgs):
        slab[k, :len(m)] = np.frombuffer(m, np.uint8)
    lens[:] = [len(m) for m in msgs]
    t[:] = np.concatenate(times)
    olens = np.zeros(total, np.uint32)
    status = None if pin == "both" else np.zeros(total, np.uint32)  # decode_status is optional
    rc, applied = call_wire_batches(store, slab, lens, np.array(sizes, np.uint32), t, out, olens, status)
    assert (rc, applied) == (0, len(sizes))
    got = [out[k, :olens[k]].tobytes() for k in range(total)]
    bad = [k for k in range(total) if got[k] != wants[k]]
    assert not bad, f"{len(bad)} responses differ (first {bad[:5]})"
    store.close()


def test_host_calls_back_to_back():
    """Calls of different kinds one after the other on one handle, each
    checked as its own tests check it: they share the pipeline's streams and
    events, the device scratch and the bounce slots, which only go wrong from
    one call to the next."""
    from oracle import sr25519 as sr
    from parity import diff_responses
    store, model = small_store()
    model.seed(41)
    params = ffi.gen_params(n_identities=300, hot=10)
    rng = np.random.default_rng(29)

    def wire_batch(n):
        reqs = model.gen_batch(n, params)
        msgs, t = to_wire(reqs, rng), reqs["timestamp"].copy()
        q, sig, st = wire.decode_requests(msgs, timestamps=t, strict=False)
        return msgs, t, sig, st, [wire.encode_response(r) for r in model.process_batch(q)]

    def counts_match():
        st_ = store.stats()
        assert (st_["messages"], st_["mailboxes"]) == (model.messages, model.mailboxes)

    # gvs_process_wire_batches
    wb = [wire_batch(n) for n in (1024, 300, 40)]
    got = store.process_wire_batches([b[0] for b in wb], np.concatenate([b[1] for b in wb]), in_stride=1104)
    for (g, gst), (_, _, _, st, want) in zip(got, wb):
        assert (gst == st).all() and g == want
    counts_match()
    # gvs_process_batches
    batches = [model.gen_batch(n, params) for n in (1024, 7, 600)]
    want = [model.process_batch(b) for b in batches]
    for g, w, b in zip(store.process_batches(batches), want, batches):
        d = diff_responses(g, w, b)
        assert not d, "\n".join(d)
    counts_match()
    # gvs_process_wire_batches_seeded: every request signed by its identity's key, one spoiled
    sizes = (200, 1, 60)
    reqs = with_keys(model.gen_batch(sum(sizes), params))
    sigs, seeds, draws, chal = signing_columns(reqs)
    spoiled = int(np.nonzero(reqs["request_type"])[0][5])
    sigs[spoiled, 3] ^= 1
    q = reqs.copy()
    q["request_type"][q["request_type"] == 0] = 0xFFFFFFFF  # still a hard error
    msgs = [m.tobytes() for m in wire.encode_requests(q, sigs)]
    want_st = np.where(reqs["auth_identity"].any(axis=1), 0, abi.WIRE_BAD_SIGNATURE)
    want_st[spoiled] = abi.WIRE_BAD_SIGNATURE
    reqs["request_type"][spoiled] = 0
    cut = np.cumsum(sizes)[:-1]
    want = [[wire.encode_response(r) for r in model.process_batch(b)] for b in np.split(reqs, cut)]
    got = store.process_wire_batches_seeded([msgs[:200], msgs[200:201], msgs[201:]], reqs["timestamp"],
                                            seeds, draws, in_stride=1104)
    assert [g[0] for g in got] == want
    assert (np.concatenate([g[1] for g in got]) == want_st).all()
    assert (np.concatenate([g[2] for g in got]) == chal).all()
    counts_match()
    # gvs_process_wire_batch
    msgs, t, sig, st, want = wire_batch(1024)
    got, got_sig, got_st = store.process_wire_batch(msgs, t, in_stride=1104)
    assert got == want and (got_st == st).all() and got_sig.tobytes() == sig.tobytes()
    counts_match()
    # gvs_sr25519_verify: 64 signatures over their challenges, every fourth spoiled
    who = list(signers300().values())[:64]
    pks, msgs, sigs = (np.array([np.frombuffer(w[i], np.uint8) for w in who]) for i in (0, 3, 4))
    sigs[::4, 40] ^= 0x10
    ok = store.sr25519_verify(pks, msgs, sigs)
    assert ok.tolist() == [sr.verify(bytes(p), bytes(m), bytes(s)) for p, m, s in zip(pks, msgs, sigs)]
    assert ok.sum() == 48
    # gvs_challenge_derive
    seeds = np.array([np.frombuffer(w[1], np.uint8) for w in who])
    draws = np.array([w[2] for w in who], np.uint64)
    assert (store.challenge_derive(seeds, draws) == msgs).all()
    from parity import diff_tables
    assert not diff_tables(store.dump_messages(), model.dump_messages())
    store.close()
