"""Timing of the channel wire call against the seeded wire call in one process
(not part of the product):  python tools/aead_ab.py [lib.so] [out.json]
A store of the headline size (2^24 messages, 64K-request batches), 64K wire
requests with random identities, no signature check (seeds and draws NULL in
both calls, so that every request is applied and every response is a full
1042 B to seal), each sealed on the device under a key of its own; then
alternating back-to-back calls of
gvs_process_wire_batch_seeded_device on the plaintexts and
gvs_process_wire_batch_channel_device on the ciphertexts.  Prints every call's
HIP-event time and wall time, the channel call's "aead_open" (65 536 x 1099 B)
and "aead_seal" (65 536 x 1042 B, fewer where a request failed) marks, and the
ratio of the medians; writes them to out.json when given."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, wire, store as gs  # noqa: E402
from tools.challenge_ab import spread, stages  # noqa: E402

W_IN, W_OUT = 1120, 1072


def run(path=None, log2n=24, n=65536, rounds=8):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << log2n, max_batch=n)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    rng = np.random.default_rng(5)
    q = np.zeros(n, abi.REQUEST_DTYPE)
    q["request_type"] = rng.integers(1, 5, n)
    for f, w in (("auth_identity", 32), ("msg_id", 16), ("recipient", 32), ("payload", 936)):
        q[f] = rng.integers(0, 256, (n, w), dtype=np.uint8)
    slab = np.zeros((n, W_IN), np.uint8)
    slab[:, :wire.REQUEST_WIRE_BYTES] = wire.encode_requests(q, rng.integers(0, 256, (n, 64), dtype=np.uint8))
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_in = cuda(slab)
    d_lens = torch.full((n,), wire.REQUEST_WIRE_BYTES, dtype=torch.int32, device="cuda")
    d_times = torch.full((n,), 1_700_000_000, dtype=torch.int64, device="cuda")
    d_keys = [cuda(rng.integers(0, 256, (n, 32), dtype=np.uint8)) for _ in range(2)]
    d_ivs = [cuda(rng.integers(0, 256, (n, 12), dtype=np.uint8)) for _ in range(2)]
    d_ct = torch.zeros((n, W_IN), dtype=torch.uint8, device="cuda")
    d_ctlens = torch.zeros((n,), dtype=torch.int32, device="cuda")
    d_out = torch.empty((n, W_OUT), dtype=torch.uint8, device="cuda")
    d_olen = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.gvs_aead_seal_device(h, d_keys[0].data_ptr(), d_ivs[0].data_ptr(), None, 16, None,
                                    d_in.data_ptr(), W_IN, d_lens.data_ptr(), n, d_ct.data_ptr(), W_IN,
                                    d_ctlens.data_ptr()) == 0

    def seeded():
        return lib.gvs_process_wire_batch_seeded_device(
            h, d_in.data_ptr(), W_IN, d_lens.data_ptr(), n, d_times.data_ptr(), None, None, d_out.data_ptr(), W_OUT, d_olen.data_ptr(), None, None, None)

    def channel():
        return lib.gvs_process_wire_batch_channel_device(
            h, d_ct.data_ptr(), W_IN, d_ctlens.data_ptr(), n, d_times.data_ptr(), None, None, d_keys[0].data_ptr(), d_ivs[0].data_ptr(), d_keys[1].data_ptr(),
            d_ivs[1].data_ptr(), d_out.data_ptr(), W_OUT, d_olen.data_ptr(), None, None, None)

    res = {"seeded": dict(event_ms=[], wall_ms=[]), "channel": dict(event_ms=[], wall_ms=[])}
    k_ms = dict(aead_open=[], aead_seal=[])
    sealed = 0
    for _ in range(rounds):  # alternating, so that clocks and neighbours hit both alike
        for name, call in (("seeded", seeded), ("channel", channel)):
            t0 = time.perf_counter()
            rc = call()
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, rc, lib.gvs_last_error(h))
            st = stages(lib, h)
            res[name]["event_ms"].append(round(sum(ms for _, ms in st), 4))
            res[name]["wall_ms"].append(round(wall, 4))
            if name == "channel":
                for k in k_ms:
                    k_ms[k].append(round(dict(st)[k], 4))
                sealed = int((d_olen > 0).sum())
    lib.gvs_destroy(h)
    out = dict(n=n, log2_capacity=log2n, rounds=rounds, responses_sealed=sealed, ghash_multiply="shift-and-xor")
    for k, v in k_ms.items():  # the first round warms the kernels up (code object load)
        out[k + "_ms"] = v
        out[k + "_median_ms"] = statistics.median(v[1:])
        out[k + "_spread"] = spread(v[1:])
    for name, r in res.items():
        out[name] = dict(r, event_median_ms=statistics.median(r["event_ms"][1:]),
                         wall_median_ms=statistics.median(r["wall_ms"][1:]),
                         event_spread=spread(r["event_ms"][1:]), wall_spread=spread(r["wall_ms"][1:]))
    out["channel_over_seeded_event"] = round(out["channel"]["event_median_ms"] / out["seeded"]["event_median_ms"], 4)
    out["channel_over_seeded_wall"] = round(out["channel"]["wall_median_ms"] / out["seeded"]["wall_median_ms"], 4)
    return out


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
