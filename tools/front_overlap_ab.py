"""Timing of the K-batch device call with and without the forked request
front, in one process (not part of the product):

    python tools/front_overlap_ab.py [--rounds R] [--steps K] [--mixes a,b,...]
                                     [--bench-parent FILE --bench-head FILE] [--out out.json]

A store of the headline size (2^24 messages prefilled to 75 %, 64K-request
batches, bench.py's prefill and request generator).  Then R rounds; each round
one timed K-batch gvs_process_batches_device call with front_overlap 0 and one
with 1 (the order swaps from round to round, so that clocks and neighbours hit
both alike), on fresh batches of bench.py's mix.  A call's time is the wall
time of the call and the gvs_synchronize behind it (the last batch's deferred
write pass), as bench.py times its steps.  The first round warms up and is
left out of the medians.

--mixes: afterwards the same K-batch call (front_overlap as the store
defaults) under request mixes that differ in what the batches hold, the
request generator reseeded alike before every call, the mixes rotated from
round to round.  Per mix: the median and the range of the call time; the
first mix is the reference, and every other median is expected inside the
reference's range (the schedule of the forked front is fixed by two events
and does not follow the requests).  The mixes mirror tools/oblivious_probe.py's
MIXES, drawn on the device against the prefilled messages.

--bench-parent / --bench-head: files of bench.py's JSON lines from alternating
plain runs of the parent commit's library and this one's on one box; their
ms_per_step sets go into the JSON, with whether they are disjoint.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from grapevine_amd import abi  # noqa: E402
from grapevine_amd.store import ObliviousStore  # noqa: E402

# percentages: create, read, update, delete; next = share of READ/DELETE that
# ask for the next message; hot = share of the requests aimed at 64 hot
# identities; miss = share of by-id requests naming an id that is not stored
MIXES = {
    "main": dict(create=25, read=25, update=25, delete=25, nxt=50),
    "rud": dict(create=0, read=34, update=33, delete=33, nxt=50),
    "all_create": dict(create=100, read=0, update=0, delete=0, nxt=0),
    "hot_next": dict(create=30, read=35, update=0, delete=35, nxt=100, hot=100),
    "all_miss_read": dict(create=0, read=100, update=0, delete=0, nxt=0, miss=100),
}


def gen_mix(dev, B, count, known, pool, g, ts0, create, read, update, delete, nxt, hot=0, miss=0):
    """bench.gen_batches with the mix as parameters."""
    out = []
    nk = known.shape[0]
    for b in range(count):
        r = torch.empty((B, 1040), dtype=torch.uint8, device=dev)
        r[:, :1024] = torch.randint(0, 256, (B, 1024), dtype=torch.uint8, device=dev, generator=g)
        r[:, 1024:] = 0
        roll = torch.randint(0, 100, (B,), device=dev, generator=g)
        c1, c2, c3 = create, create + read, create + read + update
        typ = torch.where(roll < c1, 1, torch.where(roll < c2, 2, torch.where(roll < c3, 3, 4)))
        nx = (torch.randint(0, 100, (B,), device=dev, generator=g) < nxt) & ((typ == 2) | (typ == 4))
        byid = (typ != 1) & ~nx
        k = torch.randint(0, nk, (B,), device=dev, generator=g)
        kn = known[k]  # (B, 80): id, sender, recipient
        coin = torch.randint(0, 2, (B, 1), device=dev, generator=g).bool()
        auth_byid = torch.where(coin, kn[:, 16:48], kn[:, 48:80])
        pi = torch.randint(0, pool.shape[0], (B, 2), device=dev, generator=g)
        is_hot = torch.randint(0, 100, (B,), device=dev, generator=g) < hot
        pi = torch.where(is_hot[:, None], pi % 64, pi)
        is_miss = (torch.randint(0, 100, (B,), device=dev, generator=g) < miss) & byid
        auth = torch.where(byid[:, None], auth_byid, pool[pi[:, 0]])
        # next: the mailbox of a stored message's recipient, or a hot identity's
        auth = torch.where(nx[:, None], torch.where(is_hot[:, None], pool[pi[:, 1]], kn[:, 48:80]), auth)
        rcpt = torch.where(byid[:, None], kn[:, 48:80], pool[pi[:, 1]])
        mid = torch.where((byid & ~is_miss)[:, None], kn[:, 0:16], r[:, 0:16])
        mid = torch.where(nx[:, None], torch.zeros_like(mid), mid)
        r[:, 0:16] = mid
        r[:, 16:48] = auth
        r[:, 48:80] = rcpt
        ts = torch.arange(B, device=dev, dtype=torch.int64) + ts0 + b * B + 1
        r[:, 80:88] = ts.view(torch.uint8).reshape(B, 8)
        r[:, 1024:1028] = typ.to(torch.int32).view(torch.uint8).reshape(B, 4)
        out.append(r)
    return out


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed_call(store, dev, batches, d_out):
    d_in = torch.cat(batches).contiguous()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    store.process_batches_device(d_in.data_ptr(), [b.shape[0] for b in batches], d_out.data_ptr())
    store.synchronize()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def bench_lines(path):
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("{"):
                out.append(round(float(json.loads(line)["ms_per_step"]), 4))
    return out


def run(a):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, B, K = 1 << a.log2n, a.batch, a.steps
    store = ObliviousStore(abi.make_config(N, max_batch=B))
    g = torch.Generator(device=dev)
    g.manual_seed(0x6772617065 + 3)
    pool = torch.randint(0, 256, (1 << 19, 32), dtype=torch.uint8, device=dev, generator=g)
    pool[:, 0] |= 1
    known = bench.prefill(torch, store, dev, B, int(N * a.fill), pool, g, 1_700_000_000)
    d_out = torch.empty((K * B, 1040), dtype=torch.uint8, device=dev)
    default = store.get_option("front_overlap")
    res = dict(log2_capacity=a.log2n, batch=B, steps=K, rounds=a.rounds, front_overlap_default=default)

    ms = {0: [], 1: []}
    for rnd in range(a.rounds):
        for v in ((0, 1), (1, 0))[rnd % 2]:
            batches = bench.gen_batches(torch, dev, B, K, known, pool, g, 1_800_000_000 + rnd * K * B)
            store.set_option("front_overlap", v)
            ms[v].append(round(timed_call(store, dev, batches, d_out) / K, 4))
    store.set_option("front_overlap", default)
    for v, name in ((0, "off"), (1, "on")):
        xs = ms[v][1:]
        res[name] = dict(ms_per_batch=ms[v], median=statistics.median(xs), min=min(xs), max=max(xs),
                         spread=spread(xs))
    res["saving_us_per_batch"] = round((res["off"]["median"] - res["on"]["median"]) * 1e3, 1)
    res["on_over_off"] = round(res["on"]["median"] / res["off"]["median"], 4)
    res["disjoint"] = res["on"]["max"] < res["off"]["min"]

    mixes = [m for m in a.mixes.split(",") if m]
    if mixes:
        t = {m: [] for m in mixes}
        for rnd in range(a.rounds):
            r = rnd % len(mixes)
            for m in mixes[r:] + mixes[:r]:
                g.manual_seed(0xAB0000 + rnd)  # every mix sees the same draws
                batches = gen_mix(dev, B, K, known, pool, g, 1_900_000_000 + rnd * K * B, **MIXES[m])
                t[m].append(round(timed_call(store, dev, batches, d_out) / K, 4))
        ref = t[mixes[0]][1:]
        res["mixes"] = {m: dict(ms_per_batch=xs, median=statistics.median(xs[1:]), min=min(xs[1:]),
                                max=max(xs[1:]),
                                median_in_reference_range=min(ref) <= statistics.median(xs[1:]) <= max(ref))
                        for m, xs in t.items()}
        res["mix_reference"] = mixes[0]
    if a.bench_parent and a.bench_head:
        p, h = bench_lines(a.bench_parent), bench_lines(a.bench_head)
        res["bench_ms_per_step"] = dict(parent=p, head=h, parent_spread=spread(p), head_spread=spread(h),
                                        disjoint=max(h) < min(p),
                                        saving_us=round((statistics.median(p) - statistics.median(h)) * 1e3, 1))
    store.close()
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--log2n", type=int, default=24)
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--fill", type=float, default=0.75)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=8, help="timed calls per setting and per mix (the first warms up)")
    p.add_argument("--mixes", default="", help="comma-separated mixes of " + ",".join(MIXES) + "; the first is the reference")
    p.add_argument("--bench-parent", default="")
    p.add_argument("--bench-head", default="")
    p.add_argument("--out", default="")
    a = p.parse_args()
    res = run(a)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
