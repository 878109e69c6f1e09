"""bench.py's response checks (check_batch) hold for the oracle's responses and
catch corrupted ones (CPU; torch on the host)."""
import numpy as np
import torch

import bench
from grapevine_amd import abi
from oracle import ffi


def as_t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 1040).copy())


def test_oracle_responses_pass_and_corruption_is_caught():
    cfg = abi.make_config(4096, mailbox_partitions=16, mailbox_partition_slots=32, max_batch=1024)
    m = ffi.Model(cfg)
    m.seed(3)
    m.process_batch(m.gen_batch(1024, ffi.gen_params(create=100, read=0, update=0, delete=0,
                                                     n_identities=100)))
    reqs = m.gen_batch(1024, ffi.gen_params(n_identities=100))
    out = m.process_batch(reqs)
    r, o = as_t(reqs), as_t(out)
    viol, cre, dels = bench.check_batch(torch, r, o)
    assert viol == 0
    assert cre == int(((reqs["request_type"] == 1) & (out["status_code"] == 1)).sum())
    assert dels == int(((reqs["request_type"] == 4) & (out["status_code"] == 1)).sum())
    ok = np.nonzero((out["status_code"] == 1) & (reqs["request_type"] == 1))[0]
    fail = np.nonzero((out["status_code"] >= 2) & (out["status_code"] <= 7))[0]
    bad = o.clone()
    bad[ok[0], 100] ^= 1    # a payload byte of a successful CREATE's echo ...
    bad[fail[0], 200] ^= 1  # ... and of a failure record
    v2, _, _ = bench.check_batch(torch, r, bad)
    assert v2 == 2


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float arrays within 64 MB, the same from call to call,
    and a changed byte of any response changes `row_digest`."""
    g = torch.Generator()
    g.manual_seed(5)
    n = 2 * bench.DUMP_ROWS + 3  # more rows than the sample holds, not a multiple of the digest's chunk
    o = torch.randint(0, 256, (n, 1040), dtype=torch.uint8, generator=g)
    o[:, 1025:1028] = 0
    bench.dump_outputs(str(tmp_path / "a"), o)
    bench.dump_outputs(str(tmp_path / "b"), o)
    assert all(p.suffix == ".npy" for p in (tmp_path / "a").iterdir())
    names = sorted(p.stem for p in (tmp_path / "a").iterdir())
    assert names == ["responses_sample", "row_digest", "sample_rows", "status"]
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # at the benchmark's batch size too: 64K statuses and digests beside the fixed sample
    assert a["responses_sample"].nbytes + 65536 * (4 + 4) + bench.DUMP_ROWS * 8 <= 64 << 20
    for k in names:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy")), k
    rows = a["sample_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and len(np.unique(rows)) == len(rows)
    h = o.numpy()
    assert np.array_equal(a["responses_sample"], h[rows].astype(np.float32))
    assert np.array_equal(a["status"], h[:, 1024].astype(np.float32))
    w = np.arange(1040) % 61 + 1
    assert np.array_equal(a["row_digest"], (h.astype(np.int64) @ w).astype(np.float32))
    o2 = o.clone()
    o2[n - 1, 517] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), o2)
    c = np.load(tmp_path / "c" / "row_digest.npy")
    assert (c != a["row_digest"]).nonzero()[0].tolist() == [n - 1]


def test_plain_run_options():
    """--full is off by default; the side measurements' options parse either way."""
    import sys
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
        sys.argv += ["--full", "--dump-outputs", "d", "--no-cpu", "--host-steps", "0"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "d" and a.no_cpu and a.host_steps == 0
    finally:
        sys.argv = argv
