"""Timing of gvs_noise_ix_respond_long_device beside what was there before it
for the same job (not part of the product):
    python tools/noise_long_ab.py [lib.so] [out.json]
The yardstick is DESIGN.md §16's former decision 3: gvs_noise_ix_respond_device
with an empty payload, then gvs_aead_seal_long_device of the evidence under the
send keys it returned, as a transport message.  It does less: the evidence
stays out of the handshake hash.  One process, the two sides alternating; at
each (n, p2) a warm-up round, in which both sides must accept every handshake
and return the same transport keys (Split reads ck, which no payload enters),
then the median of 7 wall-clock times with its spread (min, max), the long
call's stage times from gvs_last_timings, and the difference of the two sides
beside blocks x the measured per-step time of noise_tail.  At p2 = 2 048 the
short call runs too, for its noise_c stage.  A case the long call refuses (its
work area past GVS_AEAD_LONG_STAGE_MAX) is recorded as refused.  Prints the
result and writes it to out.json when given."""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grapevine_amd import abi, store as gs  # noqa: E402
from noise_ab import stages, summary  # noqa: E402  (tools/ is the script's directory)

SIZES = (256, 1024, 4096)
P2 = (2048, 5000, 16384, 65439)
ROUNDS = 7
up16 = lambda v: -(-v // 16) * 16


def run(path=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib = gs.load_library(path)
    cfg = abi.make_config(1 << 16, max_batch=4096)
    h = ctypes.c_void_p()
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    gen = torch.Generator(device="cuda").manual_seed(35)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")
    s, pro = bytes(range(32)), bytes(16)
    out = []
    for n in SIZES:
        d_e, d_m1, d_l1 = rnd(n, 32), rnd(n, 64), i32(n, 64)  # random u-coordinates: no payload 1
        d_m1[:, 31] &= 0x7F
        d_m1[:, 63] &= 0x7F
        for p2 in P2:
            ps, ms2 = up16(p2), up16(96 + p2)
            d_pay, d_m2, d_m2s = rnd(n, ps), u8(n, ms2), u8(n, 96 + 2048)
            d_l2, d_ok, d_rk, d_sk, d_hh = i32(n, 0), i32(n, 0), u8(n, 32), u8(n, 32), u8(n, 64)
            y_l2, y_ok, y_rk, y_sk, y_m2 = i32(n, 0), i32(n, 0), u8(n, 32), u8(n, 32), u8(n, 96)
            y_iv, y_len, y_ct, y_olen = torch.zeros((n, 12), dtype=torch.uint8, device="cuda"), i32(n, p2), \
                u8(n, up16(p2 + 16)), i32(n, 0)
            torch.cuda.synchronize()

            def respond(fn, plen, stride, m2, l2, rk, sk, hh, ok):
                return fn(h, s, pro, len(pro), d_e.data_ptr(), d_m1.data_ptr(), 64, d_l1.data_ptr(), d_pay.data_ptr(),
                          stride, plen, n, m2.data_ptr(), m2.shape[1], l2.data_ptr(), rk.data_ptr(), sk.data_ptr(),
                          hh.data_ptr() if hh is not None else None, ok.data_ptr())

            long_call = lambda: respond(lib.gvs_noise_ix_respond_long_device, p2, ps, d_m2, d_l2, d_rk, d_sk, d_hh, d_ok)
            short_call = lambda: respond(lib.gvs_noise_ix_respond_device, p2, ps, d_m2s, d_l2, d_rk, d_sk, d_hh, d_ok)

            def yardstick():
                assert respond(lib.gvs_noise_ix_respond_device, 0, ps, y_m2, y_l2, y_rk, y_sk, None, y_ok) == 0
                assert lib.gvs_aead_seal_long_device(h, y_sk.data_ptr(), y_iv.data_ptr(), None, 0, None, d_pay.data_ptr(),
                                                     ps, y_len.data_ptr(), n, y_ct.data_ptr(), y_ct.shape[1],
                                                     y_olen.data_ptr()) == 0

            row = dict(n=n, p2=p2, blocks=(64 + p2 + 16 + 17 + 127) // 128)
            rc = long_call()
            if rc == abi.GVS_ERR_INVALID_ARG and n * up16(p2 + 16) > (250 << 20):  # n sealed payloads: the cap
                row["long"] = "refused: the work area passes GVS_AEAD_LONG_STAGE_MAX"
                t = []
                for r in range(ROUNDS + 1):
                    t0 = time.perf_counter()
                    yardstick()
                    t.append(1e3 * (time.perf_counter() - t0))
                row["yardstick"] = summary(t[1:])
                out.append(row)
                continue
            assert rc == 0
            ms, per_stage, noise_c = dict(long=[], yardstick=[]), [], []
            for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit both alike
                t0 = time.perf_counter()
                assert long_call() == 0
                t1 = time.perf_counter()
                st = stages(lib, h)
                t2 = time.perf_counter()
                yardstick()
                t3 = time.perf_counter()
                if r == 0:  # the warm-up round: the same handshakes, accepted, and the same transport keys
                    assert d_ok.cpu().numpy().all() and y_ok.cpu().numpy().all()
                    assert torch.equal(d_rk, y_rk) and torch.equal(d_sk, y_sk)
                    assert (d_l2.cpu().numpy() == 96 + p2).all() and (y_olen.cpu().numpy() == p2 + 16).all()
                    continue
                ms["long"].append(1e3 * (t1 - t0))
                ms["yardstick"].append(1e3 * (t3 - t2))
                per_stage.append(st)
                if p2 <= 2048:
                    assert short_call() == 0
                    noise_c.append(dict(stages(lib, h))["noise_c"])
            row.update({k: summary(v) for k, v in ms.items()})
            med = [(per_stage[0][k][0], round(statistics.median(s[k][1] for s in per_stage), 4))
                   for k in range(len(per_stage[0]))]
            row["stage_median_ms"] = med
            tail = dict(med)["noise_tail"]
            row["tail_us_per_step"] = round(1e3 * tail / (row["blocks"] + 12), 3)
            row["long_minus_yardstick_ms"] = round(row["long"]["median_ms"] - row["yardstick"]["median_ms"], 4)
            row["blocks_x_step_ms"] = round(row["blocks"] * row["tail_us_per_step"] / 1e3, 4)
            if noise_c:
                row["short_noise_c_ms"] = summary(noise_c)
                row["noise_c_over_noise_tail"] = round(statistics.median(noise_c) / tail, 2)
            out.append(row)
    lib.gvs_destroy(h)
    return dict(rounds=ROUNDS, clock="wall, ms", cases=out)


if __name__ == "__main__":
    res = run(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] else None)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
