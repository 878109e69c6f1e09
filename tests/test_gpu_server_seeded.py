"""The gRPC front-end with device_challenges=True serving a schnorrkel HIP
store: tests/test_gpu_ed_server.py's flow, the server keeping only (seed,
draw index) per channel and k_challenge deriving every batch's challenges.
The clients sign over their own Python ChaCha20 stream, so every accepted
call pins the device stream to it; every GPU batch is replayed through the
oracle double with the challenges on_batch received -- responses and statuses
bit-exact."""
import functools

import numpy as np
import pytest

from grapevine_amd import abi
from grapevine_amd import server as gs
from grapevine_amd.store import ObliviousStore

import test_server
from test_server import OracleWireStore, check_results, run_clients

pytestmark = pytest.mark.gpu
pytest.importorskip("grpc")


def test_grpc_flow_with_device_challenges_bit_exact(monkeypatch):
    # run_clients builds its server as gs.GrapevineServer(store, ...)
    monkeypatch.setattr(test_server.gs, "GrapevineServer",
                        functools.partial(gs.GrapevineServer, device_challenges=True))
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024)
    store = ObliviousStore(cfg)
    double = OracleWireStore(cfg)
    mismatches, seen, rejected = [], [], []

    def replay(msgs, times, chal, resp, status):
        want, _, wst = double.process_wire_batch(msgs, times, challenges=chal)
        seen.append(len(msgs))
        rejected.append(int((np.asarray(status) == abi.WIRE_BAD_SIGNATURE).sum()))
        if list(resp) != want or not np.array_equal(status, wst):
            mismatches.append((len(seen), [k for k in range(len(msgs)) if resp[k] != want[k]][:5]))

    srv, signers, results = run_clients(store, on_batch=replay)  # asserts UNAUTHENTICATED on the forged call
    assert srv.device_challenges
    check_results(signers, results)  # every create and read-back succeeded
    assert not srv.hook_errors, srv.hook_errors
    assert not mismatches, mismatches
    assert sum(seen) == 4 * 3 * 2 + 3 and len(seen) < sum(seen)  # + forged, read, malformed
    assert sum(rejected) == 1  # the forged call, and only it
    st = store.stats()
    assert (st["messages"], st["mailboxes"]) == (double.model.messages, double.model.mailboxes)
    store.close()
