"""Timing of gvs_x25519_device beside gvs_ed25519_verify_device in one process
(not part of the product):  python tools/x25519_ab.py [lib.so] [out.json]
A small store, then at each n alternating back-to-back launches of the quad
ladder (one DPP quad per scalar multiplication, ~1 030 dependent field
multiplies) and of the Ed25519 check (one lane per signature, ~3 100
multiplies: the yardstick, an existing kernel that is never compared against
the code under test), on device buffers of random bytes; neither kernel
branches on them.  gvs_noise_hkdf_device is timed at the same n, both input
lengths.  A warm-up round, then the median of 7 HIP-event times with its
spread (min, max); prints the result and writes it to out.json when given."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, store as gs  # noqa: E402

SIZES = (256, 4096, 16384, 65536)
ROUNDS = 7


def last_ms(lib, h):
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    return round(ms[0], 4) if c > 0 else None


def summary(ms, n):
    med = statistics.median(ms)
    return dict(ms=ms, median_ms=med, min_ms=min(ms), max_ms=max(ms), per_item_us=round(1e3 * med / n, 4),
                items_per_s=round(n / med * 1e3))


def run(path=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << 16, max_batch=4096)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    rand = lambda n, w: torch.randint(0, 256, (n, w), dtype=torch.uint8, device="cuda", generator=g)
    out = []
    for n in SIZES:
        a32, b32, c64, d64 = rand(n, 32), rand(n, 32), rand(n, 64), rand(n, 64)
        o32, o64 = torch.empty((n, 32), dtype=torch.uint8, device="cuda"), rand(n, 64)
        ok = torch.empty((n,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        calls = dict(
            x25519=lambda: lib.gvs_x25519_device(h, a32.data_ptr(), 32, b32.data_ptr(), 32, n, o32.data_ptr(), 32,
                                                 ok.data_ptr()),
            ed_verify=lambda: lib.gvs_ed25519_verify_device(h, a32.data_ptr(), 32, b32.data_ptr(), 32, 32,
                                                            c64.data_ptr(), 64, n, ok.data_ptr()),
            hkdf_mixkey=lambda: lib.gvs_noise_hkdf_device(h, c64.data_ptr(), 64, a32.data_ptr(), 32, 32, n,
                                                          d64.data_ptr(), o64.data_ptr(), 64),
            hkdf_split=lambda: lib.gvs_noise_hkdf_device(h, c64.data_ptr(), 64, None, 0, 0, n, d64.data_ptr(),
                                                         o64.data_ptr(), 64))
        ms = {k: [] for k in calls}
        for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit all alike
            for k, call in calls.items():
                assert call() == 0, k
                if r:  # round 0 warms every kernel up at this n
                    ms[k].append(last_ms(lib, h))
        row = dict(n=n, **{k: summary(v, n) for k, v in ms.items()})
        row["x25519_over_ed_verify"] = round(row["x25519"]["median_ms"] / row["ed_verify"]["median_ms"], 4)
        out.append(row)
    lib.gvs_destroy(h)
    return dict(rounds=ROUNDS, sizes=out)


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
