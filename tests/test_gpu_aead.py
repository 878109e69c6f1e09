"""GPU parity of the channel cipher (include/gvstore.h gvs_aead_open / gvs_aead_seal,
kernel k_aead of gvs_aead.h) against the Python-integer AES-256-GCM of
tests/test_aead.py (itself pinned to the GCM specification and to OpenSSL), and
of the channel wire call (gvs_process_wire_batch_channel[_device]) against the
seeded wire call fed the same plaintexts in a twin store."""
import random

import numpy as np
import pytest

from grapevine_amd import abi
from grapevine_amd.ed25519 import Ed25519Signer

from test_aead import SPEC, open_, seal
from test_aead import vectors  # noqa: F401  (the OpenSSL fixture)
from test_gpu_challenge import SrSigner, signed_batch, small_store

pytestmark = pytest.mark.gpu

# block edges, and both sides of one and of two 64-block hash chunks once the
# AAD blocks and the length block are counted
TEXT_LENS = (0, 1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1099, 2047, 2048)
NOISE_IVS = [abi.noise_iv(c) for c in (0, 1, 1 << 32, (1 << 64) - 2)]
# (AAD length, messages, one key for all)
CASES = [(a, n, False) for a in (0, 1, 16, 20) for n in (1, 5, 67)] + [(20, 67, True)]


@pytest.fixture(scope="module")
def store():
    s = small_store()
    yield s
    s.close()


_BATCH = {}


def batch(aad_len, same_key):
    """67 messages of every length in TEXT_LENS and their reference
    ciphertexts, made once per (AAD length, key choice); the tests slice it."""
    if (aad_len, same_key) not in _BATCH:
        rng = random.Random(1000 * aad_len + same_key)
        one = rng.randbytes(32)
        keys = [one if same_key else rng.randbytes(32) for _ in range(67)]
        ivs = [NOISE_IVS[k // 2 % 4] if k % 2 else rng.randbytes(12) for k in range(67)]
        aads = [rng.randbytes(aad_len) for _ in range(67)]
        pts = [rng.randbytes(TEXT_LENS[k % len(TEXT_LENS)]) for k in range(67)]
        want = [seal(*x) for x in zip(keys, ivs, aads, pts)]
        _BATCH[aad_len, same_key] = keys, ivs, aads, pts, want
    return _BATCH[aad_len, same_key]


def arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)


@pytest.mark.parametrize("aad_len,n,same_key", CASES)
def test_seal_and_open_match_the_reference(store, aad_len, n, same_key):
    keys, ivs, aads, pts, want = [x[:n] for x in batch(aad_len, same_key)]
    aads = aads if aad_len else None
    got = store.aead_seal(arr(keys, 32), arr(ivs, 12), pts, aads)
    assert got == want, [k for k in range(n) if got[k] != want[k]]
    back, ok, _ = store.aead_open(arr(keys, 32), arr(ivs, 12), want, aads)
    assert ok.all() and back == pts, [k for k in range(n) if back[k] != pts[k]]


def test_fixed_cases(store, vectors):  # noqa: F811
    v = vectors + [dict(key=bytes(32), iv=bytes(12), aad=b"", pt=pt, ct=bytes.fromhex(w)[:-16],
                        tag=bytes.fromhex(w)[-16:]) for pt, w in SPEC]
    keys, ivs = arr([c["key"] for c in v], 32), arr([c["iv"] for c in v], 12)
    sealed = [c["ct"] + c["tag"] for c in v]
    assert store.aead_seal(keys, ivs, [c["pt"] for c in v], [c["aad"] for c in v]) == sealed
    back, ok, _ = store.aead_open(keys, ivs, sealed, [c["aad"] for c in v])
    assert ok.all() and back == [c["pt"] for c in v]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


@pytest.mark.parametrize("what", ["ct_first", "ct_last", "tag", "aad", "iv", "key", "short"])
def test_rejection_spares_the_neighbours(store, what):
    """Message 2 of 6 (two workgroups) is spoiled; it alone must fail."""
    keys, ivs, aads, pts, want = [list(x[11:17]) for x in batch(20, False)]  # lengths 1099, 2047, 2048, 0, 1, 15
    assert len(pts[2]) == 2048
    msgs = list(want)
    if what == "ct_first":
        msgs[2] = flip(msgs[2], 0)
    elif what == "ct_last":
        msgs[2] = flip(msgs[2], len(pts[2]) - 1, 0x80)
    elif what == "tag":
        msgs[2] = flip(msgs[2], len(msgs[2]) - 1)
    elif what == "aad":
        aads[2] = flip(aads[2], 19)
    elif what == "iv":
        ivs[2] = flip(ivs[2], 11)
    elif what == "key":
        keys[2] = flip(keys[2], 31, 0x40)
    else:
        msgs[2] = msgs[2][:15]
    back, ok, slab = store.aead_open(arr(keys, 32), arr(ivs, 12), msgs, aads)
    assert ok.tolist() == [k != 2 for k in range(6)]
    assert back == [b"" if k == 2 else pts[k] for k in range(6)]
    assert not slab[2].any()  # the whole slot, not only its length


# --------------------------------------------------------- the channel wire call

@pytest.fixture(scope="module", params=["schnorrkel", "ed25519"])
def channel_batch(request):
    """200 requests (five of test_gpu_challenge's signed batches) with a cipher
    pair per request, sealed by the Python reference; 103, 150 and 199 get a
    spoiled tag."""
    ed = request.param == "ed25519"
    make = (lambda rng: Ed25519Signer(rng.randbytes(32))) if ed else SrSigner
    parts = [signed_batch(make, 50 + 10 * ed + j) for j in range(5)]
    b = {k: np.concatenate([p[k] for p in parts]) for k in ("times", "seeds", "draws")}
    b["msgs"] = [m for p in parts for m in p["msgs"]]
    rng = random.Random(77 + ed)
    b["keys"] = [arr([rng.randbytes(32) for _ in range(200)], 32) for _ in range(2)]
    b["ivs"] = [arr([abi.noise_iv(rng.choice((0, 1, 1 << 32)) + k) for k in range(200)], 12) for _ in range(2)]
    b["sealed"] = [seal(b["keys"][0][k].tobytes(), b["ivs"][0][k].tobytes(), b"", m)
                   for k, m in enumerate(b["msgs"])]
    b["bad"] = (103, 150, 199)
    for k in b["bad"]:
        b["sealed"][k] = flip(b["sealed"][k], len(b["sealed"][k]) - 7, 0x20)
    b["ed"] = ed
    return b


def channel_device(store, b, lo, hi):
    """gvs_process_wire_batch_channel_device on torch tensors -> what the host form returns."""
    import torch
    n, stride, ostride = hi - lo, 1120, 1072
    slab, lens, _ = store._wire_slab(b["sealed"][lo:hi], stride)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    args = [up(x) for x in (slab, lens, b["times"][lo:hi], b["seeds"][lo:hi], b["draws"][lo:hi],
                            b["keys"][0][lo:hi], b["ivs"][0][lo:hi], b["keys"][1][lo:hi], b["ivs"][1][lo:hi])]
    out, olens, sigs, st = (torch.zeros(n * w, dtype=torch.uint8, device="cuda") for w in (ostride, 4, 64, 4))
    torch.cuda.synchronize()
    p = [a.data_ptr() for a in args]
    rc = store.lib.gvs_process_wire_batch_channel_device(
        store.h, p[0], stride, p[1], n, *p[2:], out.data_ptr(), ostride, olens.data_ptr(),
        sigs.data_ptr(), st.data_ptr(), None)
    assert rc == 0, store.lib.gvs_last_error(store.h)
    out, olens = out.cpu().numpy().reshape(n, ostride), olens.cpu().numpy().view(np.uint32)
    return [out[k, :olens[k]].tobytes() for k in range(n)], None, st.cpu().numpy().view(np.uint32), None


@pytest.mark.parametrize("form", ["host", "device"])
def test_channel_equals_seeded_on_the_plaintext(channel_batch, form):
    b = channel_batch
    if form == "device":
        pytest.importorskip("torch")
    chan, twin = small_store(ed25519_auth=b["ed"]), small_store(ed25519_auth=b["ed"])
    try:
        for lo, hi in ((0, 100), (100, 200)):  # the second batch holds the spoiled tags
            bad = [k - lo for k in b["bad"] if lo <= k < hi]
            if form == "host":
                chan.set_timing(True)
                got, _, st, _ = chan.process_wire_batch_channel(
                    b["sealed"][lo:hi], b["times"][lo:hi], b["seeds"][lo:hi], b["draws"][lo:hi],
                    b["keys"][0][lo:hi], b["ivs"][0][lo:hi], b["keys"][1][lo:hi], b["ivs"][1][lo:hi])
                names = list(chan.last_timings())
                assert names[0] == "aead_open" and names[-1] == "aead_seal", names
            else:
                got, _, st, _ = channel_device(chan, b, lo, hi)
            plain = [b"" if k in bad else m for k, m in enumerate(b["msgs"][lo:hi])]
            want, _, wst, _ = twin.process_wire_batch_seeded(plain, b["times"][lo:hi], b["seeds"][lo:hi],
                                                             b["draws"][lo:hi])
            wst = wst.copy()
            wst[bad] = abi.WIRE_BAD_CHANNEL_TAG
            assert st.tolist() == wst.tolist()
            assert [k for k in range(hi - lo) if not got[k]] == [k for k in range(hi - lo) if not want[k]]
            assert all(not got[k] for k in bad)
            live = [k for k in range(hi - lo) if got[k]]
            opened, ok, _ = chan.aead_open(b["keys"][1][lo:hi][live], b["ivs"][1][lo:hi][live], [got[k] for k in live])
            assert ok.all() and opened == [want[k] for k in live]
            k = live[-1]  # and one through the reference
            assert open_(b["keys"][1][lo + k].tobytes(), b["ivs"][1][lo + k].tobytes(), b"", got[k]) == want[k]
        assert chan.stats() == twin.stats()
        assert chan.dump_messages().tobytes() == twin.dump_messages().tobytes()
    finally:
        chan.close()
        twin.close()
