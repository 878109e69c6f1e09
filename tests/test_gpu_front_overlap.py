"""The forked request front of gvs_process_batches_device (DESIGN.md §3
"Forked request front"): in a K-batch device call on a plain single-GPU
message store, batch t + 1's front (k_copy, k_meta, the Key128 sort, the GtxOp
scan) runs on a side stream beside batch t's post-pass kernels, into the front
context batch t does not use.

The judge is the CPU oracle, bit for bit, at the smallest shape the pipeline
takes.  The oracle keeps no mailbox rows, so the mailbox region (rows and side
entries) is compared with a twin store that took the same batches one per call,
the path the rest of the suite holds against the oracle.
"""
import math

import numpy as np
import pytest

from grapevine_amd import abi
from grapevine_amd.store import GvsError, ObliviousStore
from oracle import ffi

from parity import diff_responses, diff_tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 1024
SINGLE_KEYS = ["copy", "meta", "sort_s1", "gtx", "m1", "alloc", "sort_r", "rtx", "rpass", "rr1", "rr2",
               "post", "m2r", "m2"]


def make_cfg(Q=16, Sr=32, **kw):
    return abi.make_config(4096, mailbox_partitions=Q, mailbox_partition_slots=Sr, max_batch=B, **kw)


def device_call(store, batches):
    """One gvs_process_batches_device call -> the responses of all batches."""
    sizes = [len(b) for b in batches]
    reqs = np.concatenate(batches)
    d_in = torch.from_numpy(reqs.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((max(len(reqs), 1) * 1040,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        applied = store.process_batches_device(d_in.data_ptr(), sizes, d_out.data_ptr())
    except GvsError as err:
        err.responses = d_out.cpu().numpy()[:len(reqs) * 1040].view(abi.RESPONSE_DTYPE)
        raise
    assert applied == len(sizes)
    return d_out.cpu().numpy()[:len(reqs) * 1040].view(abi.RESPONSE_DTYPE)


def mailbox_region(store):
    cfg = store.config
    R = cfg.mailbox_partitions * cfg.mailbox_partition_slots
    return (store.dump_raw(abi.RAW_MAILBOXES, 0, R * 1024).tobytes(),
            store.dump_raw(abi.RAW_SIDE, 0, R * 16).tobytes())


def check_state(store, model, twin=None):
    st = store.stats()
    assert (st["messages"], st["mailboxes"], st["creation_counter"]) == \
        (model.messages, model.mailboxes, model.creation_counter), st
    dt = diff_tables(store.dump_messages(), model.dump_messages())
    assert not dt, "\n".join(dt)
    if twin is not None:
        assert twin.stats() == st
        assert mailbox_region(store) == mailbox_region(twin), "mailbox region differs from the twin's"


def dependent_batches(model, params, sizes):
    """Each batch generated after the model took the one before (as
    parity.run_stream does): batch t + 1 names ids and mailboxes of batch t."""
    batches, want = [], []
    for n in sizes:
        b = model.gen_batch(n, params)
        batches.append(b)
        want.append(model.process_batch(b))
    return batches, want


def check_call(store, model, params, sizes, twin=None):
    batches, want = dependent_batches(model, params, sizes)
    got = device_call(store, batches)
    d = diff_responses(got, np.concatenate(want), np.concatenate(batches))
    assert not d, f"{sizes}: " + "\n".join(d)
    if twin is not None:
        for b, w in zip(batches, want):
            assert twin.process_batch(b).tobytes() == w.tobytes()
    check_state(store, model, twin)


HOT = dict(create=35, read=25, update=20, delete=20, nxt=60, hot=30, n_identities=60)


def test_cross_batch_dependence():
    """Five full batches over 60 identities, each naming what the one before
    created, in one call: a stale or shared front buffer shows here."""
    cfg = make_cfg()
    store, twin, model = ObliviousStore(cfg), ObliviousStore(cfg), ffi.Model(cfg)
    assert store.get_option("front_overlap") == 1
    model.seed(0xF0)
    check_call(store, model, ffi.gen_params(**HOT), [B] * 5, twin)
    assert store.stats()["batches"] == 5


@pytest.mark.parametrize("sizes", [[1024, 1, 0, 700, 1024, 1024], [1024], [1024, 1024]])
def test_sizes(sizes):
    cfg = make_cfg()
    store, twin, model = ObliviousStore(cfg), ObliviousStore(cfg), ffi.Model(cfg)
    model.seed(0xF1)
    check_call(store, model, ffi.gen_params(n_identities=300), sizes, twin)


def test_on_versus_off():
    """The same batches through a store with the overlap and one without:
    responses and both tables byte for byte."""
    cfg = make_cfg()
    on, off, model = ObliviousStore(cfg), ObliviousStore(cfg), ffi.Model(cfg)
    off.set_option("front_overlap", 0)
    assert (on.get_option("front_overlap"), off.get_option("front_overlap")) == (1, 0)
    model.seed(0xF2)
    for sizes in ([B] * 4, [B, 300, B]):
        batches, want = dependent_batches(model, ffi.gen_params(**HOT), sizes)
        g_on, g_off = device_call(on, batches), device_call(off, batches)
        assert g_on.tobytes() == g_off.tobytes()
        assert g_on.tobytes() == np.concatenate(want).tobytes()
    assert on.dump_messages().tobytes() == off.dump_messages().tobytes()
    assert mailbox_region(on) == mailbox_region(off)
    off.set_option("front_overlap", 1)  # and back on, on a store that has run without
    batches, want = dependent_batches(model, ffi.gen_params(**HOT), [B] * 3)
    assert device_call(off, batches).tobytes() == device_call(on, batches).tobytes()
    check_state(off, model, on)


def test_alternating_call_types():
    """A K-batch device call, a single batch, the host pipeline, another
    K-batch device call, on one store: the front contexts and the deferred
    write pass hand over between the call types."""
    cfg = make_cfg()
    store, model = ObliviousStore(cfg), ffi.Model(cfg)
    model.seed(0xF3)
    p = ffi.gen_params(**HOT)
    check_call(store, model, p, [B] * 3)
    b = model.gen_batch(B, p)
    w = model.process_batch(b)
    d = diff_responses(store.process_batch(b), w, b)
    assert not d, "\n".join(d)
    check_state(store, model)
    batches, want = dependent_batches(model, p, [B, 500, B])
    for g, w, b in zip(store.process_batches(batches), want, batches):
        d = diff_responses(g, w, b)
        assert not d, "\n".join(d)
    check_state(store, model)
    check_call(store, model, p, [B] * 4)  # even: the last front ran in the second context
    check_call(store, model, p, [B] * 2)


def distinct_recipient_creates(n):
    reqs = np.zeros(n, dtype=abi.REQUEST_DTYPE)
    reqs["request_type"] = 1
    reqs["timestamp"] = 1
    for i in range(n):
        reqs["auth_identity"][i] = np.frombuffer(ffi.identity(1 + i % 7), dtype=np.uint8)
        reqs["recipient"][i] = np.frombuffer(ffi.identity(10_000 + i), dtype=np.uint8)
    return reqs


def test_failure_in_the_middle():
    """One mailbox partition holds min(kGroupMax, B) = 512 group slots: 1024
    creates to 1024 recipients overflow them (error bit 1).  [ok, ok, bad, ok]
    in one call applies two batches; the fourth, whose front ran beside the
    failing batch, leaves nothing behind and runs in the next call."""
    cfg = make_cfg(Q=1, Sr=64)
    store, twin, model = ObliviousStore(cfg), ObliviousStore(cfg), ffi.Model(cfg)
    assert store.get_option("group_slots") < B
    bad = distinct_recipient_creates(B)
    with pytest.raises(GvsError) as ei:  # not vacuous: this batch alone overflows
        twin.process_batch(bad)
    assert ei.value.code == abi.GVS_ERR_BATCH_OVERFLOW
    model.seed(0xF5)
    p = ffi.gen_params(n_identities=40)
    ok, want = dependent_batches(model, p, [B, B])
    later = model.gen_batch(B, p)  # generated against the state after the two
    with pytest.raises(GvsError) as ei:
        device_call(store, ok + [bad, later])
    assert ei.value.code == abi.GVS_ERR_BATCH_OVERFLOW and ei.value.applied == 2
    got = ei.value.responses
    d = diff_responses(got[:2 * B], np.concatenate(want), np.concatenate(ok))
    assert not d, "\n".join(d)
    assert not got[2 * B:].view(np.uint8).any(), "unapplied responses must be zero"
    assert store.stats()["batches"] == 2
    check_state(store, model)
    w = model.process_batch(later)
    g = device_call(store, [later])
    d = diff_responses(g, w, later)
    assert not d, "\n".join(d)
    check_call(store, model, p, [B, B])


def test_marks():
    cfg = make_cfg()
    store, model = ObliviousStore(cfg), ffi.Model(cfg)
    model.seed(0xF6)
    p = ffi.gen_params(n_identities=300)
    store.set_timing(True)
    check_call(store, model, p, [B] * 3)
    t = store.last_timings()
    assert "rpass" in t
    assert all(math.isfinite(v) and v >= 0.0 for v in t.values()), t
    assert list(t) == SINGLE_KEYS
    store.process_batch(model.gen_batch(B, p))
    t1 = store.last_timings()
    assert list(t1) == SINGLE_KEYS
    assert all(math.isfinite(v) and v >= 0.0 for v in t1.values()), t1


@pytest.mark.parametrize("kw", [dict(auth_storage=True), dict(shard_count=4)])
def test_ineligible_stores(kw):
    store = ObliviousStore(make_cfg(**kw))
    assert store.get_option("front_overlap") == 0
    for v in (0, 1):
        with pytest.raises(GvsError) as ei:
            store.set_option("front_overlap", v)
        assert ei.value.code == abi.GVS_ERR_INVALID_ARG
    store.close()
