"""Timing of the long ChaCha20-Poly1305 calls (gvs_chachapoly_seal_long_device /
gvs_chachapoly_open_long_device, kernel k_chachapoly_long) beside k_aead_long
and the short k_chachapoly, and of the long responder with either suite (not
part of the product):
    python tools/chachapoly_long_ab.py [lib.so] [out.json] [other_build.so]
1. 4 096 messages of {4096, 16384, 65519} bytes through the new calls, through
   gvs_aead_*_long_device on the same messages, and through the short
   gvs_chachapoly_*_device on the same total bytes cut into 2 048-byte
   messages (in calls of at most 65 536 messages, their times added); then
   65 536 messages of 2 048 bytes, where the long and the short kernel both
   apply.  With other_build.so (the same engine built with the other value of
   GVS_CL_OPEN_KEEPS_BLOCK0) its long calls are a fourth side.
2. gvs_noise_ix_respond_long_cipher_device, 1 024 handshakes with payloads of
   5 000 and 65 439 bytes, cipher 1 against cipher 0, stage by stage.
One process, the sides alternating; at each shape a warm-up round in which
every side must open what it sealed, then the median of 7 with (min, max) of
the stage times from gvs_last_timings (HIP events around the kernels).  Bytes
per second are text bytes over the stage median."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, store as gs  # noqa: E402

SHAPES, OVERLAP, HANDSHAKES = [(4096, 4096), (4096, 16384), (4096, 65519)], (65536, 2048), [(1024, 5000), (1024, 65439)]
ROUNDS, CHUNK, CUT = 7, 65536, 2048


def stages(lib, h):
    names, ms = (ctypes.c_char_p * 16)(), (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    return {names[k].decode(): ms[k] for k in range(c)}


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def rnd(g, *shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)


class Side:
    """n messages of `text` bytes with keys and nonces of their own, device
    arrays for sealing and opening them through the calls named `stem`."""

    def __init__(self, lib, h, stem, n, text, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.lib, self.h, self.stem, self.n, self.text = lib, h, stem, n, text
        self.stride = -(-text // 16) * 16
        self.keys, self.ivs, self.pt = rnd(g, n, 32), rnd(g, n, 12), rnd(g, n, self.stride)
        self.pt[:, text:] = 0
        self.ct, self.back = (torch.zeros((n, self.stride + 16), dtype=torch.uint8, device="cuda") for _ in range(2))
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device="cuda")
        self.len_pt, self.len_ct, self.olen, self.ok = i32(text), i32(text + 16), i32(0), i32(0)
        torch.cuda.synchronize()

    def call(self, seal):
        """-> stage ms of the whole side, in calls of at most CHUNK messages"""
        fn = getattr(self.lib, self.stem % ("seal" if seal else "open"))
        src, dst, lens = (self.pt, self.ct, self.len_pt) if seal else (self.ct, self.back, self.len_ct)
        total = 0.0
        for lo in range(0, self.n, CHUNK):
            p = lambda x: x[lo:].data_ptr()
            rc = fn(self.h, p(self.keys), p(self.ivs), None, 16, None, p(src), src.shape[1], p(lens),
                    min(CHUNK, self.n - lo), p(dst), dst.shape[1], p(self.olen), *([] if seal else [p(self.ok)]))
            assert rc == 0, self.lib.gvs_last_error(self.h)
            total += sum(stages(self.lib, self.h).values())
        return total

    def check(self):
        assert bool((self.ok == 1).all()) and bool((self.olen == self.text).all())
        assert torch.equal(self.back[:, :self.stride], self.pt) and not bool(self.back[:, self.stride:].any())


def measure(libs, n, text, same):
    (lib, h), other = libs[0], libs[1:]
    cut = (n, text) if same else (-(-n * text // CUT), CUT)
    sides = dict(long=Side(lib, h, "gvs_chachapoly_%s_long_device", n, text, 1),
                 gcm_long=Side(lib, h, "gvs_aead_%s_long_device", n, text, 1),
                 short=Side(lib, h, "gvs_chachapoly_%s_device", *cut, 1 if same else 2))
    for olib, oh in other:
        sides["long_other_build"] = Side(olib, oh, "gvs_chachapoly_%s_long_device", n, text, 1)
    res = {f"{s}_{op}": [] for s in sides for op in ("seal", "open")}
    for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit all alike
        for op in ("seal", "open"):
            for name, side in sides.items():
                ms = side.call(op == "seal")
                if r:
                    res[f"{name}_{op}"].append(ms)
        if r == 0:  # the warm-up round: every side opened what it sealed, and the same kernels agree
            for side in sides.values():
                side.check()
            assert not same or torch.equal(sides["long"].ct, sides["short"].ct)
            assert not other or torch.equal(sides["long"].ct, sides["long_other_build"].ct)
    row = dict(n=n, text=text, short_messages=cut[0], short_text=cut[1])
    for k, v in res.items():
        side = sides[k.rsplit("_", 1)[0]]
        row[k] = dict(stage_ms=summary(v), gb_per_s=round(side.n * side.text / statistics.median(v) / 1e6, 2))
    for op in ("seal", "open"):  # per byte: the short side may carry a few bytes more (its last message is whole)
        per = lambda s: row[f"{s}_{op}"]["stage_ms"]["median"] / (sides[s].n * sides[s].text)
        row[f"gcm_long_over_long_{op}"] = round(per("gcm_long") / per("long"), 3)
        row[f"short_over_long_{op}"] = round(per("short") / per("long"), 3)
    return row


def handshakes(lib, h, n, p2):
    """Any 64 bytes are a message 1 of IX (two keys in clear); one payload row per handshake."""
    g = torch.Generator(device="cuda").manual_seed(p2)
    ps, ms = -(-p2 // 16) * 16, -(-(96 + p2) // 16) * 16
    eph, msg1, pay = rnd(g, n, 32), rnd(g, n, 64), rnd(g, n, ps)
    eph[:, 0] &= 248
    l1, l2, ok = (torch.full((n,), 64, dtype=torch.int32, device="cuda") for _ in range(3))
    msg2, rk, sk, hh = (torch.zeros((n, w), dtype=torch.uint8, device="cuda") for w in (ms, 32, 32, 64))
    torch.cuda.synchronize()
    res = {c: {} for c in (0, 1)}
    for r in range(ROUNDS + 1):
        for c in (0, 1):
            rc = lib.gvs_noise_ix_respond_long_cipher_device(
                h, c, bytes(range(32)), b"", 0, eph.data_ptr(), msg1.data_ptr(), 64, l1.data_ptr(), pay.data_ptr(), ps,
                p2, n, msg2.data_ptr(), ms, l2.data_ptr(), rk.data_ptr(), sk.data_ptr(), hh.data_ptr(), ok.data_ptr())
            assert rc == 0 and bool((ok == 1).all()) and bool((l2 == 96 + p2).all())
            for name, v in stages(lib, h).items() if r else ():
                res[c].setdefault(name, []).append(v)
    row = dict(n=n, payload=p2)
    for c, name in ((0, "aesgcm"), (1, "chachapoly")):
        total = [sum(v) for v in zip(*res[c].values())]
        row[name] = dict(total_ms=summary(total), stages_ms={k: summary(v) for k, v in res[c].items()},
                         noise_tail_share=round(statistics.median(res[c]["noise_tail"]) / statistics.median(total), 3))
    row["aesgcm_over_chachapoly"] = round(row["aesgcm"]["total_ms"]["median"] / row["chachapoly"]["total_ms"]["median"], 3)
    return row


def run(path=None, other=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    libs = []
    for p in [path] + ([other] if other else []):
        lib, h = gs.load_library(p), ctypes.c_void_p()
        cfg = abi.make_config(1 << 16, max_batch=CHUNK)
        assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
        lib.gvs_set_timing(h, 1)
        libs.append((lib, h))
    out = dict(rounds=ROUNDS, clock="ms; HIP events around the kernels (gvs_last_timings)",
               cipher=[measure(libs, n, text, False) for n, text in SHAPES], overlap=measure(libs, *OVERLAP, True),
               responder=[handshakes(*libs[0], n, p2) for n, p2 in HANDSHAKES])
    for lib, h in libs:
        lib.gvs_destroy(h)
    return out


if __name__ == "__main__":
    arg = lambda k: sys.argv[k] if len(sys.argv) > k and sys.argv[k] else None
    res = run(arg(1), arg(3))
    print(json.dumps(res), flush=True)
    if arg(2):
        with open(arg(2), "w") as f:
            json.dump(res, f, indent=1)
