"""The client-side Ed25519 signer (grapevine_amd/ed25519.py, RFC 8032
§5.1.5-5.1.6) against keys and signatures made by the openssl CLI
(tests/golden/ed25519_openssl_lens.json, from make_ed25519_lens.py): Ed25519
signing is deterministic, so the signer must reproduce each fixture public key
and signature bit for bit from the seed.  Its signatures at the lengths the
fixture cannot hold (0) and the wire path uses (32) pass the oracle's check."""
import json
import os

from grapevine_amd.ed25519 import Ed25519Signer
from oracle import sr25519 as sr

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    with open(os.path.join(HERE, "golden", "ed25519_openssl_lens.json")) as f:
        return [{k: bytes.fromhex(v) for k, v in rec.items()} for rec in json.load(f)]


def test_fixture_covers_the_padding_boundaries():
    assert [len(r["msg"]) for r in fixture()] == [1, 32, 47, 48, 111, 112, 175, 176, 400]


def test_signer_reproduces_openssl_bit_for_bit():
    for r in fixture():
        s = Ed25519Signer(r["seed"])
        assert s.public_key == r["pk"], len(r["msg"])
        assert s.sign(r["msg"]) == r["sig"], len(r["msg"])


def test_oracle_accepts_the_fixture():
    for r in fixture():
        assert sr.ed25519_verify(r["pk"], r["msg"], r["sig"]), len(r["msg"])


def test_signer_signatures_pass_the_oracle_at_lengths_0_and_32():
    s = Ed25519Signer(bytes(range(32)))
    for msg in (b"", bytes(range(100, 132))):
        sig = s.sign(msg)
        assert len(sig) == 64 and sr.ed25519_verify(s.public_key, msg, sig)
        bad = bytearray(sig)
        bad[3] ^= 4
        assert not sr.ed25519_verify(s.public_key, msg, bytes(bad))


def test_signer_module_does_not_use_the_oracle():
    import grapevine_amd.ed25519 as m
    src = open(m.__file__).read()
    assert "oracle" not in src  # product code: its own point arithmetic
