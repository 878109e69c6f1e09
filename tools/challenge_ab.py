"""Timing of the seeded wire call against the explicit-challenge wire call in
one process (not part of the product):  python tools/challenge_ab.py [lib.so] [out.json]
A store of the headline size (2^24 messages, 64K-request batches), then
alternating back-to-back calls of gvs_process_wire_batch_device (challenges
given) and gvs_process_wire_batch_seeded_device (seeds and draw indices given)
over the same 64K wire requests; prints every call's HIP-event time (the sum
of its stage marks) and wall time, k_challenge's own time from the seeded
call's "challenge" mark, and the ratio of the medians, and writes them to
out.json when given.  Beside them: the host time of drawing the same 64K
challenges from grapevine_amd/server.py's ChallengeRng (1024 channels, 64
draws each).  The requests carry random keys and signatures: every check
fails, and decode, check, store and encode do the same work as for valid
traffic, since none of them branches on those bytes."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, wire, server, store as gs  # noqa: E402

W_IN = 1104


def stages(lib, h):
    names = (ctypes.c_char_p * 32)()
    ms = (ctypes.c_float * 32)()
    c = lib.gvs_last_timings(h, names, ms, 32)
    return [(names[i].decode(), float(ms[i])) for i in range(max(c, 0))]


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def run(path=None, log2n=24, n=65536, rounds=8, channels=1024):
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
    # request k is draw k // channels of channel k % channels
    seeds_c = rng.integers(0, 256, (channels, 32), dtype=np.uint8)
    seeds = seeds_c[np.arange(n) % channels]
    draws = (np.arange(n) // channels).astype(np.uint64)
    t0 = time.perf_counter()
    rngs = [server.ChallengeRng(bytes(s)) for s in seeds_c]
    chal = np.frombuffer(b"".join(rngs[k % channels].draw(32) for k in range(n)), np.uint8).reshape(n, 32)
    host_s = time.perf_counter() - t0
    d_in = torch.from_numpy(slab).cuda()
    d_lens = torch.full((n,), wire.REQUEST_WIRE_BYTES, dtype=torch.int32, device="cuda")
    d_times = torch.full((n,), 1_700_000_000, dtype=torch.int64, device="cuda")
    d_chal = torch.from_numpy(chal.copy()).cuda()
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
    d_draws = torch.from_numpy(draws.view(np.int64)).cuda()
    d_out = torch.empty((n, wire.RESPONSE_WIRE_BYTES), dtype=torch.uint8, device="cuda")
    d_olen = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_cout = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def explicit():
        return lib.gvs_process_wire_batch_device(
            h, d_in.data_ptr(), W_IN, d_lens.data_ptr(), n, d_times.data_ptr(), d_chal.data_ptr(),
            d_out.data_ptr(), wire.RESPONSE_WIRE_BYTES, d_olen.data_ptr(), None, None)

    def seeded():
        return lib.gvs_process_wire_batch_seeded_device(
            h, d_in.data_ptr(), W_IN, d_lens.data_ptr(), n, d_times.data_ptr(), d_seeds.data_ptr(),
            d_draws.data_ptr(), d_out.data_ptr(), wire.RESPONSE_WIRE_BYTES, d_olen.data_ptr(), None, None,
            d_cout.data_ptr())

    res = {"explicit": dict(event_ms=[], wall_ms=[]), "seeded": dict(event_ms=[], wall_ms=[])}
    k_ms = []
    for _ in range(rounds):  # alternating, so that clocks and neighbours hit both alike
        for name, call in (("explicit", explicit), ("seeded", seeded)):
            t0 = time.perf_counter()
            rc = call()
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, rc, lib.gvs_last_error(h))
            st = stages(lib, h)
            res[name]["event_ms"].append(round(sum(ms for _, ms in st), 4))
            res[name]["wall_ms"].append(round(wall, 4))
            if name == "seeded":
                k_ms.append(round(dict(st)["challenge"], 4))
    derived_ok = bool((d_cout.cpu().numpy() == chal).all())  # the device stream is the host's
    lib.gvs_destroy(h)
    out = dict(n=n, log2_capacity=log2n, channels=channels, rounds=rounds, derived_equals_host=derived_ok,
               host_challenge_rng_s=round(host_s, 3), k_challenge_ms=k_ms,
               k_challenge_median_ms=statistics.median(k_ms[1:]))
    for name, r in res.items():  # the first round warms the kernels up (code object load)
        out[name] = dict(r, event_median_ms=statistics.median(r["event_ms"][1:]),
                         wall_median_ms=statistics.median(r["wall_ms"][1:]),
                         event_spread=spread(r["event_ms"][1:]), wall_spread=spread(r["wall_ms"][1:]))
    out["seeded_over_explicit_event"] = round(out["seeded"]["event_median_ms"] / out["explicit"]["event_median_ms"], 4)
    out["seeded_over_explicit_wall"] = round(out["seeded"]["wall_median_ms"] / out["explicit"]["wall_median_ms"], 4)
    return out


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
