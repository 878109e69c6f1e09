"""The gRPC front-end serving an Ed25519 store (grapevine_amd/server.py over
an ObliviousStore created with ed25519_auth=True): the Auth/Query flow of
tests/test_server.py with four Ed25519Signer clients, a forged call answered
UNAUTHENTICATED, and every GPU batch the server formed replayed through the
oracle double (oracle/sr25519.py::ed25519_verify in front of the model) --
responses and statuses bit-exact."""
import numpy as np
import pytest

from grapevine_amd import abi, wire
from grapevine_amd.ed25519 import Ed25519Signer
from grapevine_amd.store import ObliviousStore
from oracle import sr25519 as sr

import test_server
from test_server import OracleWireStore, check_results, run_clients

pytestmark = pytest.mark.gpu
pytest.importorskip("grpc")


class OracleEdWireStore(OracleWireStore):
    """The oracle double with the Ed25519 rule as its challenge check."""

    def process_wire_batch(self, msgs, times, in_stride=None, out_stride=1042, challenges=None):
        q, sig, st = wire.decode_requests(msgs, timestamps=times, strict=False)
        if challenges is not None:
            for k in range(len(msgs)):
                if st[k] == 0 and not sr.ed25519_verify(bytes(q[k]["auth_identity"]), bytes(challenges[k]),
                                                        bytes(sig[k])):
                    q[k]["request_type"] = 0
                    st[k] = abi.WIRE_BAD_SIGNATURE
        with self.lock:
            out = self.model.process_batch(q)
        return [wire.encode_response(r) for r in out], sig, st


def test_grpc_flow_on_ed25519_gpu_store_bit_exact(monkeypatch):
    # run_clients builds its signers from test_server.Signer(rng)
    monkeypatch.setattr(test_server, "Signer", lambda rng: Ed25519Signer(rng.randbytes(32)))
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024,
                          ed25519_auth=True)
    store = ObliviousStore(cfg)
    double = OracleEdWireStore(cfg)
    mismatches, seen, rejected = [], [], []

    def replay(msgs, times, chal, resp, status):
        want, _, wst = double.process_wire_batch(msgs, times, challenges=chal)
        seen.append(len(msgs))
        rejected.append(int((np.asarray(status) == abi.WIRE_BAD_SIGNATURE).sum()))
        if list(resp) != want or not np.array_equal(status, wst):
            mismatches.append((len(seen), [k for k in range(len(msgs)) if resp[k] != want[k]][:5]))

    srv, signers, results = run_clients(store, on_batch=replay)  # asserts UNAUTHENTICATED on the forged call
    assert all(isinstance(s, Ed25519Signer) for s in signers)
    check_results(signers, results)  # every create and read-back succeeded
    assert not srv.hook_errors, srv.hook_errors
    assert not mismatches, mismatches
    assert sum(seen) == 4 * 3 * 2 + 3 and len(seen) < sum(seen)  # + forged, read, malformed
    assert sum(rejected) == 1  # the forged call, and only it
    st = store.stats()
    assert (st["messages"], st["mailboxes"]) == (double.model.messages, double.model.mailboxes)
    store.close()
