"""Generate tests/golden/x25519_openssl.json: X25519 (scalar, peer public key,
shared secret) triples derived by the openssl CLI, an independent
implementation of RFC 7748, and the RFC's own §5.2 vector.  The raw scalar
and the peer's u-coordinate are wrapped in the fixed DER prefixes of a PKCS#8
X25519 private key and a SubjectPublicKeyInfo.  tests/test_x25519.py checks
grapevine_amd/x25519.py and the device ladder against them.

    python tests/golden/make_x25519.py
"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PRIV_DER = bytes.fromhex("302e020100300506032b656e04220420")
PUB_DER = bytes.fromhex("302a300506032b656e032100")
RFC7748 = dict(scalar="a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
               u="e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
               out="c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")


def main(n=12):
    out = [RFC7748]
    with tempfile.TemporaryDirectory() as d:
        key, peer = os.path.join(d, "k.der"), os.path.join(d, "p.der")
        for _ in range(n):
            scalar, peer_scalar = os.urandom(32), os.urandom(32)
            with open(peer, "wb") as f:  # the peer's public key, made by openssl from a scalar of its own
                f.write(PRIV_DER + peer_scalar)
            u = subprocess.run(["openssl", "pkey", "-inform", "DER", "-in", peer, "-pubout", "-outform", "DER"],
                               check=True, capture_output=True).stdout[-32:]
            with open(key, "wb") as f:
                f.write(PRIV_DER + scalar)
            with open(peer, "wb") as f:
                f.write(PUB_DER + u)
            secret = subprocess.run(["openssl", "pkeyutl", "-derive", "-keyform", "DER", "-inkey", key,
                                     "-peerform", "DER", "-peerkey", peer], check=True, capture_output=True).stdout
            assert len(secret) == 32
            out.append(dict(scalar=scalar.hex(), u=u.hex(), out=secret.hex()))
    with open(os.path.join(HERE, "x25519_openssl.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
