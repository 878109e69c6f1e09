"""Timing of gvs_noise_ix_respond_device beside the same handshakes composed
from the entry points that were there before it (not part of the product):
    python tools/noise_ab.py [lib.so] [out.json]
The yardstick is gvs_x25519_device, gvs_noise_hkdf_device x 4 and
gvs_aead_seal_device x 2 with the transcript hashed by hashlib on the host in
between: it is not the new code, and its arrays for k_x25519 are made before
the clock starts.  One process, the two sides alternating; at each (n, p2) a
warm-up round, in which both sides must return the same keys, then the median
of 7 wall-clock times with its spread (min, max), and the one call's stage
times from gvs_last_timings beside them.  Prints the result and writes it to
out.json when given."""
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, noise, store as gs  # noqa: E402

SIZES = (256, 1024, 4096)
P2 = (0, 2048)
ROUNDS = 7


def stages(lib, h):
    names, ms = (ctypes.c_char_p * 16)(), (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    return [(names[k].decode(), round(ms[k], 4)) for k in range(c)]


def summary(ms):
    return dict(ms=[round(v, 4) for v in ms], median_ms=round(statistics.median(ms), 4),
                min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def run(path=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << 16, max_batch=4096)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    rng = np.random.default_rng(34)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sha = lambda *parts: hashlib.sha512(b"".join(parts)).digest()
    out = []
    for n in SIZES:
        for p2 in P2:
            s, pro = rng.bytes(32), rng.bytes(16)
            eph = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            msg1 = rng.integers(0, 256, (n, 64), dtype=np.uint8)  # random u-coordinates: no payload 1
            msg1[:, 31] &= 0x7F
            msg1[:, 63] &= 0x7F
            pay = rng.integers(0, 256, (n, max(p2, 16)), dtype=np.uint8)
            d_e, d_m1, d_pay = dev(eph), dev(msg1), dev(pay)
            d_l1 = i32(n, 64)
            d_m2, d_l2, d_ok = u8(n, 96 + p2), i32(n, 0), i32(n, 0)
            d_rk, d_sk, d_hh = u8(n, 32), u8(n, 32), u8(n, 64)

            def one_call():
                return lib.gvs_noise_ix_respond_device(
                    h, s, pro, len(pro), d_e.data_ptr(), d_m1.data_ptr(), 64, d_l1.data_ptr(), d_pay.data_ptr(),
                    pay.shape[1], p2, n, d_m2.data_ptr(), 96 + p2, d_l2.data_ptr(), d_rk.data_ptr(),
                    d_sk.data_ptr(), d_hh.data_ptr(), d_ok.data_ptr())

            # the composed side's k_x25519 rows, as the one call's gather makes them
            nine = np.zeros(32, np.uint8)
            nine[0] = 9
            sb = np.frombuffer(s, np.uint8)
            sc = np.concatenate([np.stack([eph, eph, eph, np.tile(sb, (n, 1))], 1).reshape(4 * n, 32), sb[None]])
            pt = np.concatenate([np.stack([np.tile(nine, (n, 1)), msg1[:, :32], msg1[:, 32:], msg1[:, :32]],
                                          1).reshape(4 * n, 32), nine[None]])
            c_sc, c_pt, c_x, c_xok = dev(sc), dev(pt), u8(4 * n + 1, 32), i32(4 * n + 1, 0)
            c_ck, c_o1, c_o2 = u8(n, 64), u8(n, 64), u8(n, 64)
            c_iv, c_al, c_olen = torch.zeros((n, 12), dtype=torch.uint8, device="cuda"), i32(n, 64), i32(n, 0)
            c_len1, c_len2 = i32(n, 32), i32(n, p2)
            c_ct1, c_ct2 = u8(n, 48), u8(n, pay.shape[1] + 16)
            h0 = noise.PROTOCOL_NAME.ljust(64, b"\0")

            def composed():
                x = lambda k: c_x.data_ptr() + 32 * k
                assert lib.gvs_x25519_device(h, c_sc.data_ptr(), 32, c_pt.data_ptr(), 32, 4 * n + 1, c_x.data_ptr(),
                                             32, c_xok.data_ptr()) == 0
                xo = c_x.cpu().numpy()
                hp = sha(h0, pro)
                hs = [sha(sha(sha(sha(hp, msg1[k, :32].tobytes()), msg1[k, 32:].tobytes())),
                          xo[4 * k].tobytes()) for k in range(n)]
                c_ck.copy_(dev(np.tile(np.frombuffer(h0, np.uint8), (n, 1))))
                torch.cuda.synchronize()
                hkdf = lambda ikm, ln: lib.gvs_noise_hkdf_device(h, c_ck.data_ptr(), 64, ikm, 128, ln, n,
                                                                 c_o1.data_ptr(), c_o2.data_ptr(), 64)

                def mix_key_and_seal(item, text, stride, lens, ct):
                    assert hkdf(x(item), 32) == 0
                    c_ck.copy_(c_o1)
                    key, aad = c_o2[:, :32].contiguous(), dev(np.frombuffer(b"".join(hs), np.uint8).reshape(n, 64))
                    torch.cuda.synchronize()
                    assert lib.gvs_aead_seal_device(h, key.data_ptr(), c_iv.data_ptr(), aad.data_ptr(), 64,
                                                    c_al.data_ptr(), text.data_ptr(), stride, lens.data_ptr(), n,
                                                    ct.data_ptr(), ct.shape[1], c_olen.data_ptr()) == 0
                    got = ct.cpu().numpy()
                    return [sha(hs[k], got[k, :ct.shape[1] if ct is c_ct1 else p2 + 16].tobytes()) for k in range(n)]

                assert hkdf(x(1), 32) == 0  # ee
                c_ck.copy_(c_o1)
                torch.cuda.synchronize()
                spub = c_x[4 * n:].expand(n, 32).contiguous()
                hs = mix_key_and_seal(2, spub, 32, c_len1, c_ct1)   # se, then s
                hs = mix_key_and_seal(3, d_pay, pay.shape[1], c_len2, c_ct2)  # es, then the payload
                assert hkdf(None, 0) == 0  # Split
                return c_o1[:, :32].cpu().numpy(), c_o2[:, :32].cpu().numpy(), hs

            ms = dict(one_call=[], composed=[])
            per_stage = []
            for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit both alike
                t0 = time.perf_counter()
                assert one_call() == 0
                t1 = time.perf_counter()
                st = stages(lib, h)
                t2 = time.perf_counter()
                k1, k2, hs = composed()
                t3 = time.perf_counter()
                if r == 0:  # the warm-up round: both sides ran the same handshakes
                    assert d_ok.cpu().numpy().all()
                    assert (d_rk.cpu().numpy() == k1).all() and (d_sk.cpu().numpy() == k2).all()
                    assert d_hh.cpu().numpy().tobytes() == b"".join(hs)
                    continue
                ms["one_call"].append(1e3 * (t1 - t0))
                ms["composed"].append(1e3 * (t3 - t2))
                per_stage.append(st)
            row = dict(n=n, p2=p2, **{k: summary(v) for k, v in ms.items()})
            row["stage_median_ms"] = [(per_stage[0][k][0], round(statistics.median(s[k][1] for s in per_stage), 4))
                                      for k in range(len(per_stage[0]))]
            row["composed_over_one_call"] = round(row["composed"]["median_ms"] / row["one_call"]["median_ms"], 2)
            out.append(row)
    lib.gvs_destroy(h)
    return dict(rounds=ROUNDS, clock="wall, ms", cases=out)


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
