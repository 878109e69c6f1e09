"""Timing of the device Noise IX initiator (gvs_noise_ix_initiate_device,
gvs_noise_ix_finish_device) beside the responder on the same handshakes and
beside `finish` composed from the entry points that were there before it (not
part of the product):
    python tools/noise_init_ab.py [lib.so] [out.json]
For both suites, n = 1 024 and 4 096, payload 2 of 0 and 2 048 bytes:
initiate, gvs_noise_ix_respond_cipher_device on its message 1, finish on the
responder's message 2, and the composed finish: gvs_x25519_device x 2,
gvs_noise_hkdf_device x 4 and gvs_aead_open_device / gvs_chachapoly_open_device
x 2 with the transcript hashed by hashlib on the host in between.  One process,
the sides alternating; a warm-up round, in which both sides of the handshake
and the composed finish must return the same keys; then the median of 7 with
(min, max): wall clock of every side, and the calls' stage times from
gvs_last_timings (HIP events around the kernels).  Prints the result and
writes it to out.json when given."""
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

SIZES, P2, ROUNDS = (1024, 4096), (0, 2048), 7


def stages(lib, h):
    names, ms = (ctypes.c_char_p * 16)(), (ctypes.c_float * 16)()
    c = lib.gvs_last_timings(h, names, ms, 16)
    out = {}
    for k in range(c):  # a chain opens or seals twice: the second mark of a name is "<name>_2"
        name = names[k].decode()
        out[name + "_2" if name in out else name] = ms[k]
    return out


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def shape(lib, h, cipher, n, p2):
    g = torch.Generator(device="cuda").manual_seed(1000 * cipher + p2 + n)
    rnd = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    i32 = lambda v=0: torch.full((n,), v, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    ps, m2s = max(p2, 16), -(-(96 + p2) // 16) * 16
    s, e, r_e, pay2 = rnd(32), rnd(n, 32), rnd(n, 32), rnd(n, ps)
    r_s, pro = bytes(range(32)), b"noise_init_ab"
    m1, l1, st = u8(n, 64), i32(), u8(n, 64)
    m2, l2, r_rk, r_sk, r_hh, r_ok = u8(n, m2s), i32(), u8(n, 32), u8(n, 32), u8(n, 64), i32()
    rs, out2, pl, sk, rk, hh, ok = u8(n, 32), u8(n, ps), i32(), u8(n, 32), u8(n, 32), u8(n, 64), i32()
    torch.cuda.synchronize()

    def initiate():
        return lib.gvs_noise_ix_initiate_device(h, cipher, pro, len(pro), p(s), 0, p(e), None, 0, 0, n, p(m1), 64,
                                                p(l1), p(st))

    def respond():
        return lib.gvs_noise_ix_respond_cipher_device(h, cipher, r_s, pro, len(pro), p(r_e), p(m1), 64, p(l1), p(pay2),
                                                      ps, p2, n, p(m2), m2s, p(l2), p(r_rk), p(r_sk), p(r_hh), p(r_ok))

    def finish():
        return lib.gvs_noise_ix_finish_device(h, cipher, p(s), 0, p(e), p(st), p(m2), m2s, p(l2), n, p(rs), p(out2),
                                              ps, p(pl), p(sk), p(rk), p(hh), p(ok))

    # the composed side's arrays, made before the clock starts
    c_x, c_xok, c_es = u8(2 * n, 32), torch.zeros(2 * n, dtype=torch.int32, device="cuda"), u8(n, 32)
    c_ck, c_o1, c_o2, c_iv, c_al, c_olen, c_ok = u8(n, 64), u8(n, 64), u8(n, 64), u8(n, 12), i32(64), i32(), i32()
    c_rs, c_pt, c_len1, c_len2 = u8(n, 32), u8(n, m2s - 96 + 16), i32(48), i32(p2 + 16)
    sha = lambda *parts: hashlib.sha512(b"".join(parts)).digest()
    opener = lib.gvs_chachapoly_open_device if cipher else lib.gvs_aead_open_device
    name = np.frombuffer(noise.PROTOCOL_NAMES[cipher].ljust(64, b"\0"), np.uint8)

    def composed():
        msgs, h1 = m2.cpu().numpy(), st.cpu().numpy()
        sc, pt = torch.cat([e, s.expand(n, 32)]).contiguous(), m2[:, :32].repeat(2, 1).contiguous()
        assert lib.gvs_x25519_device(h, p(sc), 32, p(pt), 32, 2 * n, p(c_x), 32, p(c_xok)) == 0  # ee, se
        hs = [sha(h1[k].tobytes(), msgs[k, :32].tobytes()) for k in range(n)]
        c_ck.copy_(torch.from_numpy(np.tile(name, (n, 1))))
        torch.cuda.synchronize()

        def mix_key(ikm, ln=32):
            assert lib.gvs_noise_hkdf_device(h, p(c_ck), 64, ikm, 32, ln, n, p(c_o1), p(c_o2), 64) == 0
            c_ck.copy_(c_o1)
            torch.cuda.synchronize()

        def open_and_hash(ct, lens, out, width):
            key = c_o2[:, :32].contiguous()
            aad = torch.from_numpy(np.frombuffer(b"".join(hs), np.uint8).reshape(n, 64).copy()).cuda()
            torch.cuda.synchronize()
            assert opener(h, p(key), p(c_iv), p(aad), 64, p(c_al), p(ct), ct.shape[1], p(lens), n, p(out), out.shape[1],
                          p(c_olen), p(c_ok)) == 0
            got = ct.cpu().numpy()
            return [sha(hs[k], got[k, :width].tobytes()) for k in range(n)]

        mix_key(p(c_x))
        mix_key(p(c_x) + 32 * n)
        hs = open_and_hash(m2[:, 32:80].contiguous(), c_len1, c_rs, 48)
        assert lib.gvs_x25519_device(h, p(e), 32, p(c_rs), 32, n, p(c_es), 32, p(c_xok)) == 0  # es
        mix_key(p(c_es))
        hs = open_and_hash(m2[:, 80:].contiguous(), c_len2, c_pt, p2 + 16)
        mix_key(None, 0)  # Split
        return c_o1[:, :32].cpu().numpy(), c_o2[:, :32].cpu().numpy(), hs

    sides = dict(initiate=initiate, respond=respond, finish=finish)
    wall, per_stage = {k: [] for k in (*sides, "composed_finish")}, {k: {} for k in sides}
    for r in range(ROUNDS + 1):  # alternating, so that clocks and neighbours hit all alike
        for side, fn in sides.items():
            t0 = time.perf_counter()
            assert fn() == 0, lib.gvs_last_error(h)
            if r:
                wall[side].append(1e3 * (time.perf_counter() - t0))
                for k, v in stages(lib, h).items():
                    per_stage[side].setdefault(k, []).append(v)
        t0 = time.perf_counter()
        k1, k2, hs = composed()
        if r:
            wall["composed_finish"].append(1e3 * (time.perf_counter() - t0))
        else:  # the warm-up round: the two device sides and the composed finish ran the same handshakes
            assert bool(ok.all()) and bool(r_ok.all()) and bool(c_ok.all()) and bool((pl == p2).all())
            assert torch.equal(sk, r_rk) and torch.equal(rk, r_sk) and torch.equal(hh, r_hh)
            assert torch.equal(out2[:, :p2], pay2[:, :p2])
            assert (sk.cpu().numpy() == k1).all() and (rk.cpu().numpy() == k2).all()
            assert hh.cpu().numpy().tobytes() == b"".join(hs)
    row = dict(cipher=cipher, n=n, p2=p2, wall_ms={k: summary(v) for k, v in wall.items()})
    for side in sides:
        total = [sum(v) for v in zip(*per_stage[side].values())]
        row[side] = dict(stages_total_ms=summary(total), stages_ms={k: summary(v) for k, v in per_stage[side].items()})
    med = lambda side: row[side]["stages_total_ms"]["median"]
    row["finish_over_respond"] = round(med("finish") / med("respond"), 3)
    row["initiator_over_respond"] = round((med("initiate") + med("finish")) / med("respond"), 3)
    row["composed_over_finish_wall"] = round(row["wall_ms"]["composed_finish"]["median"] / row["wall_ms"]["finish"]["median"], 2)
    return row


def run(path=None):
    torch.zeros(1, device="cuda")  # torch's HIP runtime opens the device before the engine's
    torch.cuda.synchronize()
    lib, h = gs.load_library(path), ctypes.c_void_p()
    cfg = abi.make_config(1 << 16, max_batch=4096)
    assert lib.gvs_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    lib.gvs_set_timing(h, 1)
    rows = [shape(lib, h, c, n, p2) for c in (abi.CIPHER_AESGCM, abi.CIPHER_CHACHAPOLY) for n in SIZES for p2 in P2]
    lib.gvs_destroy(h)
    return dict(rounds=ROUNDS, clock="ms; wall: time.perf_counter around a synchronous call; stages: HIP events "
                "around the kernels (gvs_last_timings)", rows=rows)


if __name__ == "__main__":
    arg = lambda k: sys.argv[k] if len(sys.argv) > k and sys.argv[k] else None
    res = run(arg(1))
    print(json.dumps(res), flush=True)
    if arg(2):
        with open(arg(2), "w") as f:
            json.dump(res, f, indent=1)
