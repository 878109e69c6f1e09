"""GPU parity of the batched Ed25519 challenge check (include/gvstore.h
gvs_ed25519_verify, and gvs_process_wire_batch with challenges on a store
created with GVS_FLAG_ED25519_AUTH) against signatures made by the openssl CLI
(tests/golden/ed25519_openssl_lens.json) and against the CPU rule
oracle/sr25519.py::ed25519_verify: RFC 8032 strict decoding, cofactorless,
s < l, no small-order test.  Every verdict must equal the oracle's."""
import ctypes
import random

import numpy as np
import pytest

from grapevine_amd import abi, wire
from grapevine_amd.ed25519 import Ed25519Signer
from grapevine_amd.store import BlockStore, GvsError, ObliviousStore
from oracle import ffi
from oracle import sr25519 as sr

import ed_cases
import wire_cases

pytestmark = pytest.mark.gpu


def small_store(**kw):
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024, **kw)
    return ObliviousStore(cfg), ffi.Model(cfg)


def arr(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), width)


def device_verdicts(store, triples):
    """One launch over (pk, msg, sig) triples of one message length."""
    msg_len = len(triples[0][1])
    return store.ed25519_verify(arr([t[0] for t in triples], 32), arr([t[1] for t in triples], msg_len),
                                arr([t[2] for t in triples], 64))


def test_openssl_fixture_verifies_and_bit_flips_do_not():
    store, _ = small_store()
    for r in ed_cases.fixture():
        recs = [r] + ed_cases.bit_flips(r)  # the record, then R, s, pk, msg each with a flipped bit
        got = device_verdicts(store, [(t["pk"], t["msg"], t["sig"]) for t in recs])
        assert got.tolist() == [True, False, False, False, False], (len(r["msg"]), got.tolist())
    store.close()


@pytest.mark.parametrize("msg_len", [0, 32, 47, 48, 176])
def test_verify_matches_oracle(msg_len):
    store, _ = small_store()
    cs = ed_cases.cases(random.Random(1000 + msg_len), 96, msg_len)
    want = np.array([sr.ed25519_verify(pk, msg, sig) for pk, msg, sig, _ in cs])
    got = device_verdicts(store, cs)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(k), cs[k][3], bool(got[k]), bool(want[k])) for k in bad[:8]]
    assert want.sum() >= 96 // 6  # the mix has not degenerated into rejections only
    store.close()


def test_small_order_keys():
    store, _ = small_store()
    cs = ed_cases.small_order_cases()
    want = np.array([sr.ed25519_verify(pk, msg, sig) for pk, msg, sig in cs])
    got = device_verdicts(store, cs)
    assert got.tolist() == want.tolist(), [(cs[k][0].hex(), bool(got[k])) for k in np.nonzero(got != want)[0]]
    ident, ident_signed = (1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little")
    for k, (pk, _, _) in enumerate(cs):
        if pk == ident:
            assert got[k]  # cofactorless, no small-order test: encode([s]B) || s passes
        if pk == ident_signed:
            assert not got[k]  # x = 0 with the sign bit set is not a strict encoding
    store.close()


@pytest.fixture(scope="module")
def valid700():
    rng = random.Random(6)
    signers = [Ed25519Signer(rng.randbytes(32)) for _ in range(7)]
    msgs = [rng.randbytes(32) for _ in range(700)]
    sigs = [signers[i % 7].sign(msgs[i]) for i in range(700)]
    assert sr.ed25519_verify(signers[3].public_key, msgs[3], sigs[3])
    return [(signers[i % 7].public_key, msgs[i], sigs[i]) for i in range(700)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_launch_shapes_all_valid(valid700, n):
    """The 64-thread block edge and the tail threads: n valid signatures all pass."""
    store, _ = small_store()
    got = device_verdicts(store, valid700[:n])
    assert len(got) == n and got.all(), np.nonzero(~got)[0][:10]
    store.close()


def test_device_entry_with_request_slab_strides(valid700):
    """gvs_ed25519_verify_device with keys inside a request slab (pk_stride
    1040) and packed signatures; one tampered signature is the only rejection."""
    torch = pytest.importorskip("torch")
    store, _ = small_store()
    n = 65
    reqs = np.zeros(n, abi.REQUEST_DTYPE)
    sigs = bytearray(b"".join(t[2] for t in valid700[:n]))
    sigs[64 * 17 + 3] ^= 2
    for k in range(n):
        reqs[k]["auth_identity"] = np.frombuffer(valid700[k][0], np.uint8)
    d_reqs = torch.from_numpy(reqs.view(np.uint8).copy()).cuda()
    d_msgs = torch.from_numpy(arr([t[1] for t in valid700[:n]], 32).copy()).cuda()
    d_sigs = torch.from_numpy(np.frombuffer(bytes(sigs), np.uint8).copy()).cuda()
    d_ok = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    rc = store.lib.gvs_ed25519_verify_device(store.h, d_reqs.data_ptr() + 16, 1040, d_msgs.data_ptr(), 32,
                                             32, d_sigs.data_ptr(), 64, n, d_ok.data_ptr())
    assert rc == 0
    assert d_ok.cpu().numpy().tolist() == [0 if k == 17 else 1 for k in range(n)]
    # argument checks mirror the schnorrkel entry point's
    assert store.lib.gvs_ed25519_verify_device(store.h, d_reqs.data_ptr(), 31, d_msgs.data_ptr(), 32, 32,
                                               d_sigs.data_ptr(), 64, n, d_ok.data_ptr()) == abi.GVS_ERR_INVALID_ARG
    assert store.lib.gvs_ed25519_verify_device(store.h, d_reqs.data_ptr(), 32, d_msgs.data_ptr(), 16, 32,
                                               d_sigs.data_ptr(), 64, n, d_ok.data_ptr()) == abi.GVS_ERR_INVALID_ARG
    store.close()


class SignedWire:
    """Wire batches whose identities are Ed25519 public keys, each request
    signed over its challenge, every ninth signature forged."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.params = ffi.gen_params(n_identities=60, hot=5)
        self.keymap = {}
        self.stranger = Ed25519Signer(bytes(32))

    def key_for(self, ident):
        if ident not in self.keymap:
            self.keymap[ident] = Ed25519Signer(self.rng.randbytes(32))
        return self.keymap[ident]

    def batch(self, model, n=1024):
        """-> (msgs, times, challenges, reqs, the requests whose validity is
        not by construction: forged ones and those of unknown identities)."""
        rng = self.rng
        reqs = model.gen_batch(n, self.params)
        for q in reqs:  # identities and recipients become real Ed25519 keys
            for f in ("auth_identity", "recipient"):
                v = bytes(q[f])
                if any(v):
                    q[f] = np.frombuffer(self.key_for(v).public_key, np.uint8)
        by_pk = {s.public_key: s for s in self.keymap.values()}
        chal = np.frombuffer(rng.randbytes(32 * len(reqs)), np.uint8).reshape(-1, 32)
        msgs, doubtful = [], []
        for k, q in enumerate(reqs):
            pk = bytes(q["auth_identity"])
            sig = bytearray(by_pk.get(pk, self.stranger).sign(bytes(chal[k])))
            if k % 9 == 4:
                sig[rng.randrange(64)] ^= 1 << rng.randrange(8)
            if k % 9 == 4 or pk not in by_pk:
                doubtful.append(k)
            f = dict(rt=int(q["request_type"]), auth=pk, sig=bytes(sig), id=bytes(q["msg_id"]),
                     rc=bytes(q["recipient"]), pl=bytes(q["payload"]))
            msgs.append(wire_cases.canonical(f))
        return msgs, reqs["timestamp"].copy(), chal, reqs, doubtful


def test_wire_batch_with_ed25519_challenges():
    """tests/test_gpu_sr25519.py::test_wire_batch_with_challenges on a store
    created with ed25519_auth=True: the device decodes, verifies Ed25519
    signatures over the challenges, runs the store and encodes; a forged
    request is a hard error (empty response, GVS_WIRE_BAD_SIGNATURE)."""
    store, model = small_store(ed25519_auth=True)
    model.seed(41)
    gen = SignedWire(77)
    kept = []
    for b in range(2):
        msgs, times, chal, reqs, doubtful = gen.batch(model)
        q, sig, st = wire.decode_requests(msgs, timestamps=times, strict=False)
        valid = np.ones(len(reqs), bool)
        for k in doubtful:  # oracle verdicts where validity is not by construction
            valid[k] = sr.ed25519_verify(bytes(reqs[k]["auth_identity"]), bytes(chal[k]), bytes(sig[k]))
        for k in np.nonzero(~valid)[0]:
            q[k]["request_type"] = 0
            st[k] = st[k] or abi.WIRE_BAD_SIGNATURE
        want = [wire.encode_response(r) for r in model.process_batch(q)]
        got, got_sig, got_st = store.process_wire_batch(msgs, times, challenges=chal)
        assert (got_st == st).all(), np.nonzero(got_st != st)[0][:10]
        diff = [k for k in range(len(want)) if got[k] != want[k]]
        assert not diff, f"batch {b}: {len(diff)} responses differ (first {diff[:5]})"
        assert (~valid).sum() > 50
        s = store.stats()
        assert (s["messages"], s["mailboxes"]) == (model.messages, model.mailboxes)
        kept.append((msgs, times, chal, want, st))
    store.close()
    # the same two batches through the double-buffered host entry point
    # (gvs_process_wire_batches) of a fresh Ed25519 store
    store, _ = small_store(ed25519_auth=True)
    res = store.process_wire_batches([k[0] for k in kept], np.concatenate([k[1] for k in kept]),
                                     challenges=np.concatenate([k[2] for k in kept]))
    for (_, _, _, want, st), (got, got_st) in zip(kept, res):
        assert (got_st == st).all() and got == want
    store.close()


def test_wire_stage_is_named_ed_verify():
    store, model = small_store(ed25519_auth=True)
    model.seed(3)
    msgs, times, chal, _, _ = SignedWire(5).batch(model, 64)
    store.set_timing(True)
    store.process_wire_batch(msgs, times, challenges=chal)
    names = list(store.last_timings())
    assert "ed_verify" in names and "sr_verify" not in names, names
    store.close()


def test_flag_is_refused_by_the_block_store():
    cfg = abi.make_oram_config(4096, max_batch=1024)
    cfg.flags = abi.FLAG_ED25519_AUTH
    with pytest.raises(GvsError) as e:
        BlockStore(cfg)
    assert e.value.code == abi.GVS_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    from grapevine_amd.store import load_library
    assert load_library().gvs_omap_create(ctypes.byref(cfg), ctypes.byref(h)) == abi.GVS_ERR_INVALID_ARG


def test_flag_combines_with_sealed_storage():
    store, _ = small_store(ed25519_auth=True, auth_storage=True)
    assert store.config.flags == abi.FLAG_AUTH_STORAGE | abi.FLAG_ED25519_AUTH
    store.close()


def test_default_store_rejects_ed25519_signed_batch():
    """Without the flag nothing changes: the schnorrkel check rejects every
    Ed25519-signed request (no marker bit or another equation)."""
    store, model = small_store()
    model.seed(41)
    msgs, times, chal, _, _ = SignedWire(77).batch(model)
    got, _, st = store.process_wire_batch(msgs, times, challenges=chal)
    decoded = wire.decode_requests(msgs, timestamps=times, strict=False)[2] == 0
    assert decoded.sum() > 900
    assert (st[decoded] == abi.WIRE_BAD_SIGNATURE).all() and not any(got)
    s = store.stats()
    assert (s["messages"], s["mailboxes"]) == (0, 0)
    store.close()
