"""GPU parity of the device challenge stream (include/gvstore.h
gvs_challenge_derive[_device], kernel k_challenge of gvs_chacha.h) against the
Python block function (grapevine_amd/server.py::chacha20_block, itself pinned
to openssl by tests/test_chacha_host.py), and of the seeded wire calls
(gvs_process_wire_batch_seeded, gvs_process_wire_batches_seeded) against the
explicit-challenge calls fed the Python stream: two stores of one config must
end byte for byte alike."""
import random

import numpy as np
import pytest

from grapevine_amd import abi, wire
from grapevine_amd import server as gs
from grapevine_amd.ed25519 import Ed25519Signer
from grapevine_amd.store import GvsError, ObliviousStore
from oracle import sr25519 as sr

import wire_cases

pytestmark = pytest.mark.gpu

DRAWS = (0, 1, 2, 3, (1 << 33) - 1, 1 << 33, (1 << 33) + 1, (1 << 64) - 1)
SIZES = (0, 1, 255, 256, 257, 1024)


def small_store(**kw):
    return ObliviousStore(abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32,
                                          max_batch=1024, **kw))


def python_challenges(seeds, draws):
    rows = [gs.chacha20_block(bytes(s), int(d) >> 1)[32 * (int(d) & 1):][:32] for s, d in zip(seeds, draws)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 32)


@pytest.fixture(scope="module")
def stream1024():
    """1024 random seeds, the draw indices cycling through DRAWS, and the
    Python stream's challenges; computed once, sliced by the tests."""
    rng = random.Random(31)
    seeds = np.frombuffer(rng.randbytes(32 * 1024), np.uint8).reshape(1024, 32)
    draws = np.array([DRAWS[k % len(DRAWS)] for k in range(1024)], np.uint64)
    want = python_challenges(seeds, draws)
    for a in (seeds, draws, want):
        a.setflags(write=False)
    return seeds, draws, want


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


@pytest.mark.parametrize("n", SIZES)
def test_derive_host_form(store, stream1024, n):
    seeds, draws, want = stream1024
    got = store.challenge_derive(seeds[:n], draws[:n])
    assert got.shape == (n, 32)
    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
    assert not len(bad), [(int(k), int(draws[k])) for k in bad[:8]]


@pytest.mark.parametrize("n", SIZES)
def test_derive_device_form(store, stream1024, n):
    torch = pytest.importorskip("torch")
    seeds, draws, want = stream1024
    d_seeds = torch.from_numpy(seeds.copy()).cuda()
    d_draws = torch.from_numpy(draws.view(np.int64).copy()).cuda()
    d_out = torch.full((1024 + 2, 32), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's copies done before the engine stream runs
    rc = store.lib.gvs_challenge_derive_device(store.h, d_seeds.data_ptr(), d_draws.data_ptr(), n,
                                               d_out.data_ptr() + 32)
    assert rc == 0
    out = d_out.cpu().numpy()
    assert (out[1:1 + n] == want[:n]).all(), np.nonzero((out[1:1 + n] != want[:n]).any(axis=1))[0][:8]
    assert (out[0] == 0xA5).all() and (out[1 + n:] == 0xA5).all()  # nothing outside [0, n)


def test_derive_argument_checks(store, stream1024):
    torch = pytest.importorskip("torch")
    seeds, draws, _ = stream1024
    d_seeds = torch.from_numpy(seeds[:8].copy()).cuda()
    d_draws = torch.from_numpy(draws[:8].view(np.int64).copy()).cuda()
    d_out = torch.zeros((9, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, h, bad = store.lib, store.h, abi.GVS_ERR_INVALID_ARG
    assert lib.gvs_challenge_derive_device(h, None, d_draws.data_ptr(), 8, d_out.data_ptr()) == bad
    assert lib.gvs_challenge_derive_device(h, d_seeds.data_ptr(), None, 8, d_out.data_ptr()) == bad
    assert lib.gvs_challenge_derive_device(h, d_seeds.data_ptr(), d_draws.data_ptr(), 8, None) == bad
    assert lib.gvs_challenge_derive_device(h, d_seeds.data_ptr(), d_draws.data_ptr(), 8,
                                           d_out.data_ptr() + 8) == bad  # not 16-byte aligned
    assert lib.gvs_challenge_derive(h, None, draws[:8].ctypes.data, 8, None) == bad
    assert lib.gvs_challenge_derive(None, None, None, 0, None) == bad


# ------------------------------------------------------------- the wire calls

class SrSigner:
    def __init__(self, rng):
        self.x, self.rng = rng.randrange(1, sr.L), rng
        self.public_key = sr.public_key(self.x)

    def sign(self, challenge):
        return sr.sign(self.x, challenge, self.rng.randrange(1, sr.L))


def signed_batch(make_signer, seed):
    """40 wire messages from 6 connections, one seed each, each connection's
    requests signed over its stream in order: 19 CREATEs to the next identity,
    19 READs, one request signed over the draw after its own (index 11) and
    one malformed message (index 23).  -> dict of the messages, times, seeds,
    the draw indices the server passes, and the Python stream at those
    indices."""
    rng = random.Random(seed)
    signers = [make_signer(random.Random(seed * 100 + i)) for i in range(6)]
    conn_seed = [rng.randbytes(32) for _ in signers]
    # connection c starts at an index of its own, so that both halves of a block and the
    # carry into the counter's high word occur
    next_draw = [0, 1, 7, (1 << 33) - 1, (1 << 33) - 2, (1 << 64) - 8]
    msgs, seeds, draws = [], [], []
    for k in range(40):
        c = k % 6
        d, next_draw[c] = next_draw[c], next_draw[c] + 1
        seeds.append(conn_seed[c])
        draws.append(d)
        if k == 23:
            msgs.append(b"\x0d\x01")  # truncated fixed32: the server drew for it all the same
            continue
        signed_draw = d + 1 if k == 11 else d
        chal = gs.chacha20_block(conn_seed[c], signed_draw >> 1)[32 * (signed_draw & 1):][:32]
        f = dict(rt=abi.REQUEST_TYPE_CREATE if k < 20 else abi.REQUEST_TYPE_READ,
                 auth=signers[c].public_key, sig=signers[c].sign(chal), id=bytes(16),
                 rc=signers[(c + 1) % 6].public_key if k < 20 else bytes(32),
                 pl=rng.randbytes(936) if k < 20 else bytes(936))
        msgs.append(wire_cases.canonical(f))
    seeds = np.frombuffer(b"".join(seeds), np.uint8).reshape(-1, 32)
    draws = np.array(draws, np.uint64)
    return dict(msgs=msgs, times=np.full(40, 1_700_000_000, np.uint64), seeds=seeds, draws=draws,
                chal=python_challenges(seeds, draws))


@pytest.fixture(scope="module")
def sr_batch():
    return signed_batch(SrSigner, 7)


@pytest.fixture(scope="module")
def ed_batch():
    return signed_batch(lambda rng: Ed25519Signer(rng.randbytes(32)), 8)


def check_statuses(b, resp, st):
    want = np.zeros(40, np.uint32)
    want[11], want[23] = abi.WIRE_BAD_SIGNATURE, abi.WIRE_DECODE_ERROR
    assert st.tolist() == want.tolist()
    assert resp[11] == b"" and resp[23] == b""
    ok = [wire.decode_responses([r])[0]["status_code"] == abi.STATUS_CODE_SUCCESS
          for k, r in enumerate(resp) if k not in (11, 23)]
    assert sum(ok) >= 19  # the CREATEs (but the rejected one) went in: the check passed the valid ones


def seeded_equals_explicit(b, **kw):
    seeded, explicit = small_store(**kw), small_store(**kw)
    try:
        r1, s1, st1, chal = seeded.process_wire_batch_seeded(b["msgs"], b["times"], b["seeds"], b["draws"])
        r2, s2, st2 = explicit.process_wire_batch(b["msgs"], b["times"], challenges=b["chal"])
        assert (chal == b["chal"]).all(), np.nonzero((chal != b["chal"]).any(axis=1))[0]
        assert r1 == r2, [k for k in range(40) if r1[k] != r2[k]]
        assert s1.tobytes() == s2.tobytes() and st1.tobytes() == st2.tobytes()
        assert seeded.stats() == explicit.stats()
        check_statuses(b, r1, st1)
    finally:
        seeded.close()
        explicit.close()


def test_seeded_equals_explicit_schnorrkel(sr_batch):
    seeded_equals_explicit(sr_batch)


def test_seeded_equals_explicit_ed25519(ed_batch):
    seeded_equals_explicit(ed_batch, ed25519_auth=True)


def test_seeded_equals_explicit_sharded(sr_batch):
    seeded_equals_explicit(sr_batch, shard_count=4)


def test_wire_stage_is_named_challenge(sr_batch):
    b = sr_batch
    store = small_store()
    store.set_timing(True)
    store.process_wire_batch_seeded(b["msgs"], b["times"], b["seeds"], b["draws"])
    names = list(store.last_timings())
    assert names[:2] == ["challenge", "wire_decode"] and "sr_verify" in names, names
    store.process_wire_batch(b["msgs"], b["times"], challenges=b["chal"])
    assert "challenge" not in list(store.last_timings())
    store.close()


def test_wire_batches_seeded(sr_batch):
    """Three batches, the middle one empty, against process_wire_batches fed the Python stream."""
    b = sr_batch
    batches = [b["msgs"][:17], [], b["msgs"][17:]]
    seeded, explicit = small_store(), small_store()
    got = seeded.process_wire_batches_seeded(batches, b["times"], b["seeds"], b["draws"])
    want = explicit.process_wire_batches(batches, b["times"], challenges=b["chal"])
    assert [len(g[0]) for g in got] == [17, 0, 23]
    o = 0
    for (r1, st1, chal), (r2, st2) in zip(got, want):
        assert r1 == r2 and st1.tobytes() == st2.tobytes()
        assert (chal == b["chal"][o:o + len(r1)]).all()
        o += len(r1)
    assert seeded.stats() == explicit.stats()
    check_statuses(b, [r for g in got for r in g[0]], np.concatenate([g[1] for g in got]))
    seeded.close()
    explicit.close()


def test_misuse(sr_batch):
    b = sr_batch
    store, plain = small_store(), small_store()
    for seeds, draws in ((b["seeds"], None), (None, b["draws"])):
        with pytest.raises(GvsError) as e:
            store.process_wire_batch_seeded(b["msgs"], b["times"], seeds, draws)
        assert e.value.code == abi.GVS_ERR_INVALID_ARG
        with pytest.raises(GvsError) as e:
            store.process_wire_batches_seeded([b["msgs"]], b["times"], seeds, draws)
        assert e.value.code == abi.GVS_ERR_INVALID_ARG
    big = [b"\x0d\x01"] * 1025  # more than max_batch
    with pytest.raises(GvsError) as e:
        store.process_wire_batch_seeded(big, 1, np.zeros((1025, 32), np.uint8), np.zeros(1025, np.uint64))
    assert e.value.code == abi.GVS_ERR_INVALID_ARG
    assert store.stats() == plain.stats()  # nothing was applied
    # no seeds and no draws: unchecked, as challenges=None (the wrongly signed request goes in)
    r1, s1, st1, chal = store.process_wire_batch_seeded(b["msgs"], b["times"], None, None)
    r2, s2, st2 = plain.process_wire_batch(b["msgs"], b["times"], challenges=None)
    assert r1 == r2 and s1.tobytes() == s2.tobytes() and st1.tobytes() == st2.tobytes()
    assert st1[11] == abi.WIRE_OK and r1[11] != b"" and not chal.any()
    assert store.stats() == plain.stats()
    store.close()
    plain.close()
