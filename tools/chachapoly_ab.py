"""Timing of the ChaCha20-Poly1305 channel cipher against AES-256-GCM in one
process (not part of the product):  python tools/chachapoly_ab.py [lib.so] [out.json]
The set-up of tools/aead_ab.py (a store of 2^24 messages, 64K wire requests, no
signature check, every request sealed on the device under a key of its own),
then eight rounds, the first a warm-up, in which the sides alternate:
  kernels   gvs_aead_open_device / gvs_chachapoly_open_device on n x 1099 B and
            gvs_aead_seal_device / gvs_chachapoly_seal_device on n x 1042 B,
            n = 65 536 and n = 1 024 (the calls' own stage marks, HIP events)
  wire      the seeded wire batch on the plaintexts, the channel call with
            cipher 0 and with cipher 1 on their ciphertexts (sum of the marks)
  noise     1 024 and 4 096 handshakes through gvs_noise_ix_respond_cipher_device
            with cipher 0 and cipher 1 (wall time of the synchronous call)
Prints the medians of the seven timed rounds with their minimum and maximum and
the ratios of the medians; writes them to out.json when given."""
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
from tools.challenge_ab import stages  # noqa: E402

W_IN, W_OUT = 1120, 1072
CIPHERS = ((abi.CIPHER_AESGCM, "aead"), (abi.CIPHER_CHACHAPOLY, "chachapoly"))


def summary(xs):
    xs = xs[1:]  # the first round warms the kernels up (code object load)
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


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
    i32 = lambda v, k=n: torch.full((k,), v, dtype=torch.int32, device="cuda")
    d_in, d_lens, d_rlens = cuda(slab), i32(wire.REQUEST_WIRE_BYTES), i32(abi.WIRE_RESPONSE_BYTES)
    d_times = torch.full((n,), 1_700_000_000, dtype=torch.int64, device="cuda")
    d_keys = [cuda(rng.integers(0, 256, (n, 32), dtype=np.uint8)) for _ in range(2)]
    d_ivs = [cuda(rng.integers(0, 256, (n, 12), dtype=np.uint8)) for _ in range(2)]
    d_ct = {c: torch.zeros((n, W_IN), dtype=torch.uint8, device="cuda") for c, _ in CIPHERS}
    d_ctlens = torch.zeros((n,), dtype=torch.int32, device="cuda")
    d_out = torch.empty((n, W_IN), dtype=torch.uint8, device="cuda")
    d_olen, d_ok = i32(0), i32(0)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()

    def cipher_call(name, seal, k):  # k messages: open k x 1099 B of ciphertext, or seal k x 1042 B of d_in's rows
        fn = getattr(lib, "gvs_%s_%s_device" % (name, "seal" if seal else "open"))
        c = abi.CIPHER_CHACHAPOLY if name == "chachapoly" else abi.CIPHER_AESGCM
        src, lens = (d_in, d_rlens) if seal else (d_ct[c], d_ctlens)
        return fn(h, p(d_keys[0]), p(d_ivs[0]), None, 16, None, p(src), W_IN, p(lens), k, p(d_out), W_IN, p(d_olen),
                  *([] if seal else [p(d_ok)]))

    for c, name in CIPHERS:  # the requests' ciphertexts under each cipher
        fn = getattr(lib, "gvs_%s_seal_device" % name)
        assert fn(h, p(d_keys[0]), p(d_ivs[0]), None, 16, None, p(d_in), W_IN, p(d_lens), n, p(d_ct[c]), W_IN,
                  p(d_ctlens)) == 0

    def seeded():
        return lib.gvs_process_wire_batch_seeded_device(h, p(d_in), W_IN, p(d_lens), n, p(d_times), None, None, p(d_out),
                                                        W_OUT, p(d_olen), None, None, None)

    def channel(c):
        return lambda: lib.gvs_process_wire_batch_channel_cipher_device(
            h, c, p(d_ct[c]), W_IN, p(d_ctlens), n, p(d_times), None, None, p(d_keys[0]), p(d_ivs[0]), p(d_keys[1]),
            p(d_ivs[1]), p(d_out), W_OUT, p(d_olen), None, None, None)

    # handshakes: any 32 bytes serve as keys; a small-order one would only zero its own outputs
    hs = 4096
    d_eph, d_m1 = cuda(rng.integers(0, 256, (hs, 32), dtype=np.uint8)), cuda(rng.integers(0, 256, (hs, 64), dtype=np.uint8))
    d_m1l, d_m2l, d_hok = i32(64, hs), i32(0, hs), i32(0, hs)
    d_m2 = torch.empty((hs, 96), dtype=torch.uint8, device="cuda")
    d_rk, d_sk, d_hh = (torch.empty((hs, w), dtype=torch.uint8, device="cuda") for w in (32, 32, 64))
    static = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    torch.cuda.synchronize()

    def noise(c, k):
        return lambda: lib.gvs_noise_ix_respond_cipher_device(h, c, static, b"", 0, p(d_eph), p(d_m1), 64, p(d_m1l), None,
                                                              0, 0, k, p(d_m2), 96, p(d_m2l), p(d_rk), p(d_sk), p(d_hh),
                                                              p(d_hok))

    sides = []  # (result name, call, which stage mark: None = the sum of the marks, "wall" = wall time)
    for k in (n, 1024):
        for seal in (False, True):
            for _, name in CIPHERS:
                mark = "%s_%s" % (name, "seal" if seal else "open")
                sides.append(("%s_n%d" % (mark, k), (lambda name=name, seal=seal, k=k: cipher_call(name, seal, k)), mark))
    sides += [("wire_seeded", seeded, None), ("wire_channel_aead", channel(0), None),
              ("wire_channel_chachapoly", channel(1), None)]
    sides += [("noise_%s_n%d" % (name, k), noise(c, k), "wall") for k in (1024, hs) for c, name in CIPHERS]
    ms = {name: [] for name, _, _ in sides}
    for _ in range(rounds):  # alternating, so that clocks and neighbours hit all sides alike
        for name, call, mark in sides:
            t0 = time.perf_counter()
            rc = call()
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, rc, lib.gvs_last_error(h))
            st = stages(lib, h)
            ms[name].append(wall if mark == "wall" else sum(v for _, v in st) if mark is None else dict(st)[mark])
    lib.gvs_destroy(h)
    out = dict(n=n, log2_capacity=log2n, rounds=rounds, timed_rounds=rounds - 1)
    out.update({name: summary(v) for name, v in ms.items()})
    ratio = lambda a, b: round(out[a]["median_ms"] / out[b]["median_ms"], 4)
    for k in (n, 1024):
        for op in ("open", "seal"):
            out["chachapoly_over_aead_%s_n%d" % (op, k)] = ratio("chachapoly_%s_n%d" % (op, k), "aead_%s_n%d" % (op, k))
    for name in ("aead", "chachapoly"):
        out["wire_channel_%s_over_seeded" % name] = ratio("wire_channel_" + name, "wire_seeded")
    for k in (1024, hs):
        out["noise_chachapoly_over_aead_n%d" % k] = ratio("noise_chachapoly_n%d" % k, "noise_aead_n%d" % k)
    return out


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
