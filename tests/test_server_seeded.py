"""GrapevineServer(device_challenges=True) on CPU: the server keeps (seed, next
draw index) per channel and the store derives the challenges
(process_wire_batch_seeded).  The store is tests/test_server.py's oracle
double, extended here with a process_wire_batch_seeded that derives with the
Python block function; the clients sign over their own ChallengeRng stream,
so every accepted call shows that the two sides drew the same 32 bytes.  The
GPU form (tests/test_gpu_server_seeded.py) serves from the HIP store."""
import functools
import random

import numpy as np
import pytest

from grapevine_amd import abi
from grapevine_amd import server as gs

import test_server
from test_server import OracleWireStore, Signer, check_results, run_clients

grpc = pytest.importorskip("grpc")


def python_challenges(seeds, draws):
    """(n, 32) uint8: draw number draws[k] of ChaCha20Rng(seeds[k]), by
    grapevine_amd/server.py::chacha20_block."""
    rows = [gs.chacha20_block(bytes(s), int(d) >> 1)[32 * (int(d) & 1):][:32] for s, d in zip(seeds, draws)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 32)


class SeededOracleWireStore(OracleWireStore):
    """The oracle double with ObliviousStore.process_wire_batch_seeded's contract."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.seeded_calls, self.draws_seen = 0, []

    def process_wire_batch(self, *a, **kw):
        raise AssertionError("device_challenges=True must not use the explicit-challenge call")

    def process_wire_batch_seeded(self, msgs, times, seeds, draws, in_stride=None, out_stride=1042):
        assert (seeds is None) == (draws is None)
        chal = np.zeros((len(msgs), 32), np.uint8)
        if seeds is not None:
            chal = python_challenges(seeds, draws)
            self.draws_seen.extend(int(d) for d in draws)
        self.seeded_calls += 1
        resp, sig, st = OracleWireStore.process_wire_batch(self, msgs, times,
                                                           challenges=chal if seeds is not None else None)
        return resp, sig, st, chal


def seeded_server(monkeypatch):
    """run_clients builds its server as gs.GrapevineServer(store, ...)."""
    monkeypatch.setattr(test_server.gs, "GrapevineServer",
                        functools.partial(gs.GrapevineServer, device_challenges=True))


CFG = dict(mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024)


def test_grpc_flow_with_device_challenges(monkeypatch):
    """The Auth/Query flow of tests/test_server.py, forged call included
    (run_clients asserts UNAUTHENTICATED for it and success for the next call
    on the same channel)."""
    server_cls = gs.GrapevineServer
    seeded_server(monkeypatch)
    store = SeededOracleWireStore(abi.make_config(4096, **CFG))
    seen = []

    def on_batch(msgs, times, chal, resp, status):
        seen.append((len(msgs), np.array(chal), np.array(status)))

    srv, signers, results = run_clients(store, on_batch=on_batch)
    assert isinstance(srv, server_cls) and srv.device_challenges
    check_results(signers, results)
    assert not srv.hook_errors, srv.hook_errors
    assert store.seeded_calls == srv.batches == len(seen)
    assert sum(n for n, _, _ in seen) == 4 * 3 * 2 + 3  # + forged, read, malformed
    assert sum(int((st == abi.WIRE_BAD_SIGNATURE).sum()) for _, _, st in seen) == 1  # the forged call only
    # on_batch saw the derived challenges, 32 B per request, none left at zero
    assert all(c.shape == (n, 32) and c.any(axis=1).all() for n, c, _ in seen)
    # client 0 made 6 + 3 calls: its channel's draws ran 0..8 with no gap
    assert sorted(store.draws_seen).count(8) == 1 and max(store.draws_seen) == 8


def test_oversized_request_advances_the_draw_index():
    """A request larger than a wire slot never reaches the store, but the
    client drew a challenge for it: the channel's index moves on, and the next
    call on the channel verifies."""
    store = SeededOracleWireStore(abi.make_config(4096, **CFG))
    srv = gs.GrapevineServer(store, window_ms=1.0, clock=lambda: 1_700_000_123, call_timeout=30,
                             device_challenges=True).start()
    c = gs.GrapevineClient(f"insecure-grapevine://127.0.0.1:{srv.port}", Signer(random.Random(5))).auth()
    assert c.query(abi.REQUEST_TYPE_READ)["status_code"] == abi.STATUS_CODE_NOT_FOUND
    c.rng.draw(32)  # the client's draw for the oversized request
    with pytest.raises(grpc.RpcError) as e:
        c.call(bytes(abi.WIRE_SLOT_MAX + 1))
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert c.query(abi.REQUEST_TYPE_READ)["status_code"] == abi.STATUS_CODE_NOT_FOUND
    c.close()
    srv.stop()
    assert store.draws_seen == [0, 2]  # draw 1 was the oversized request's


def test_verify_false_derives_nothing():
    store = SeededOracleWireStore(abi.make_config(4096, **CFG))
    seen = []
    srv = gs.GrapevineServer(store, window_ms=1.0, verify=False, call_timeout=30, device_challenges=True,
                             on_batch=lambda m, t, chal, r, s: seen.append(np.array(chal))).start()
    c = gs.GrapevineClient(f"insecure-grapevine://127.0.0.1:{srv.port}", Signer(random.Random(6))).auth()
    assert c.query(abi.REQUEST_TYPE_READ)["status_code"] == abi.STATUS_CODE_NOT_FOUND
    c.close()
    srv.stop()
    assert store.seeded_calls == 1 and store.draws_seen == []
    assert len(seen) == 1 and seen[0].shape == (1, 32) and not seen[0].any()


def test_default_server_is_unchanged():
    """device_challenges defaults to False: channels hold a ChallengeRng and
    batches go through process_wire_batch with host-drawn challenges."""
    srv = gs.GrapevineServer(OracleWireStore(abi.make_config(4096, **CFG)), window_ms=1.0, call_timeout=30).start()
    c = gs.GrapevineClient(f"insecure-grapevine://127.0.0.1:{srv.port}", Signer(random.Random(7))).auth()
    assert c.query(abi.REQUEST_TYPE_READ)["status_code"] == abi.STATUS_CODE_NOT_FOUND
    (rng, _), = srv.channels.values()
    assert isinstance(rng, gs.ChallengeRng) and not srv.device_challenges
    c.close()
    srv.stop()
