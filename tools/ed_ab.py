"""Timing of gvs_ed25519_verify_device against gvs_sr25519_verify_device in
one process (not part of the product):  python tools/ed_ab.py [lib.so] [out.json]
A small store, then alternating back-to-back launches of the two checks over
the same 64K random (pk, 32-B message, signature) triples; prints every
launch's HIP-event time and the ratio of the medians, and writes them to
out.json when given.  Random bytes take the same instruction stream as real
signatures: neither kernel branches on them."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, store as gs  # noqa: E402


def last_ms(lib, h):
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    return round(ms[0], 4) if c > 0 else None


def run(path=None, n=65536, rounds=8):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << 16, max_batch=4096)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    pks = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    sigs = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device="cuda", generator=g)
    ok = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx = b"grapevine-challenge"
    sr, ed = [], []
    for _ in range(rounds):  # alternating, so that clocks and neighbours hit both alike
        assert lib.gvs_sr25519_verify_device(h, pks.data_ptr(), 32, msgs.data_ptr(), 32, 32,
                                             sigs.data_ptr(), 64, n, ctx, len(ctx), ok.data_ptr()) == 0
        sr.append(last_ms(lib, h))
        assert lib.gvs_ed25519_verify_device(h, pks.data_ptr(), 32, msgs.data_ptr(), 32, 32,
                                             sigs.data_ptr(), 64, n, ok.data_ptr()) == 0
        ed.append(last_ms(lib, h))
    lib.gvs_destroy(h)
    # the first round warms both kernels up (code object load)
    m_sr, m_ed = statistics.median(sr[1:]), statistics.median(ed[1:])
    return dict(n=n, msg_len=32, sr_verify_ms=sr, ed_verify_ms=ed, sr_median_ms=m_sr,
                ed_median_ms=m_ed, ed_over_sr=round(m_ed / m_sr, 4))


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
