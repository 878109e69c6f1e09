"""Timing of the long channel cipher (gvs_aead_seal_long_device /
gvs_aead_open_long_device, kernel k_aead_long) beside the short one (not part
of the product):
    python tools/aead_long_ab.py [lib.so] [out.json]
1. n in {256, 1024, 4096} messages of {4096, 16384, 65519} bytes through the
   long calls; the yardstick is k_aead, which is not the new code:
   gvs_aead_seal_device / gvs_aead_open_device on the same total bytes cut into
   2 048-byte messages (in calls of at most 65 536 messages, their times added).
2. 65 536 messages of 1 099 and of 2 048 bytes through both, where both apply.
One process, the two sides alternating; at each shape a warm-up round in which
both sides must open what they sealed (and, in 2, seal the same bytes), then
the median of 7 with (min, max) of the wall clock around the synchronous call
and of the call's stage time from gvs_last_timings (HIP events around the
kernel).  Bytes per second are text bytes over the stage median."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, store as gs  # noqa: E402

SHAPES = [(n, text) for text in (4096, 16384, 65519) for n in (256, 1024, 4096)]
OVERLAP = [(65536, 1099), (65536, 2048)]
ROUNDS, CHUNK, CUT = 7, 65536, 2048


def stage_ms(lib, h):
    names, ms = (ctypes.c_char_p * 16)(), (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    return sum(ms[k] for k in range(c))


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


class Side:
    """n messages of `text` bytes with keys and IVs of their own, device arrays
    for sealing and opening them through the short or the long calls."""

    def __init__(self, lib, h, long, n, text, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
        self.lib, self.h, self.n, self.text, self.suffix = lib, h, n, text, "_long" if long else ""
        self.stride = -(-text // 16) * 16
        self.keys, self.ivs, self.pt = rnd(n, 32), rnd(n, 12), rnd(n, self.stride)
        self.pt[:, text:] = 0
        self.ct = torch.zeros((n, self.stride + 16), dtype=torch.uint8, device="cuda")
        self.back = torch.zeros((n, self.stride + 16), dtype=torch.uint8, device="cuda")
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device="cuda")
        self.len_pt, self.len_ct, self.olen, self.ok = i32(text), i32(text + 16), i32(0), i32(0)
        torch.cuda.synchronize()

    def call(self, seal):
        """-> (wall ms, stage ms) of the whole side, in calls of at most CHUNK messages"""
        fn = getattr(self.lib, f"gvs_aead_{'seal' if seal else 'open'}{self.suffix}_device")
        src, dst, lens = (self.pt, self.ct, self.len_pt) if seal else (self.ct, self.back, self.len_ct)
        wall = stage = 0.0
        for lo in range(0, self.n, CHUNK):
            m = min(CHUNK, self.n - lo)
            p = lambda x: x[lo:].data_ptr()
            args = [self.h, p(self.keys), p(self.ivs), None, 16, None, p(src), src.shape[1], p(lens), m, p(dst),
                    dst.shape[1], p(self.olen)] + ([] if seal else [p(self.ok)])
            t0 = time.perf_counter()
            rc = fn(*args)
            wall += 1e3 * (time.perf_counter() - t0)
            assert rc == 0, self.lib.gvs_last_error(self.h)
            stage += stage_ms(self.lib, self.h)
        return wall, stage

    def check(self):
        assert bool((self.ok == 1).all()) and bool((self.olen == self.text).all())
        assert torch.equal(self.back[:, :self.stride], self.pt) and not bool(self.back[:, self.stride:].any())


def measure(lib, h, n, text, same):
    total = n * text
    sides = dict(long=Side(lib, h, True, n, text, 1),
                 short=Side(lib, h, False, n, text, 1) if same else Side(lib, h, False, -(-total // CUT), CUT, 2))
    res = {f"{s}_{op}": dict(wall=[], stage=[]) for s in sides for op in ("seal", "open")}
    for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit both alike
        for op in ("seal", "open"):
            for name, side in sides.items():
                wall, stage = side.call(op == "seal")
                if r:
                    res[f"{name}_{op}"]["wall"].append(wall)
                    res[f"{name}_{op}"]["stage"].append(stage)
        if r == 0:  # the warm-up round: both sides opened what they sealed
            for side in sides.values():
                side.check()
            assert not same or torch.equal(sides["long"].ct, sides["short"].ct)
    row = dict(n=n, text=text, short_messages=sides["short"].n, short_text=sides["short"].text)
    for k, v in res.items():
        side = sides[k.split("_")[0]]
        row[k] = dict(wall_ms=summary(v["wall"]), stage_ms=summary(v["stage"]),
                      gb_per_s=round(side.n * side.text / statistics.median(v["stage"]) / 1e6, 2))
    for op in ("seal", "open"):  # per byte: the short side may carry a few bytes more (its last message is whole)
        per = lambda s: row[f"{s}_{op}"]["stage_ms"]["median"] / (sides[s].n * sides[s].text)
        row[f"short_over_long_{op}"] = round(per("short") / per("long"), 3)
    return row


def run(path=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << 16, max_batch=CHUNK)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    out = dict(rounds=ROUNDS, clock="ms; stage = HIP events around the kernel, wall = around the synchronous call",
               cipher=[measure(lib, h, n, text, False) for n, text in SHAPES],
               overlap=[measure(lib, h, n, text, True) for n, text in OVERLAP])
    lib.gvs_destroy(h)
    return out


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
