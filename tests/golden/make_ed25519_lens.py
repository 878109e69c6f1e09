"""Generate tests/golden/ed25519_openssl_lens.json: Ed25519 seeds, public
keys, messages and signatures made by the openssl CLI, one per message length
that matters to the device SHA-512 of R || A || M (64 + len bytes): 47/48 and
175/176 are where 64 + len crosses the 111/112 and 239/240 padding boundaries,
32 is the wire path's challenge length.  OpenSSL 3.0.2 refuses an empty -rawin
input, so length 0 is covered by grapevine_amd/ed25519.py's signer in the tests.

    python tests/golden/make_ed25519_lens.py
"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 32, 47, 48, 111, 112, 175, 176, 400)


def main():
    out = []
    with tempfile.TemporaryDirectory() as d:
        for n in LENGTHS:
            key, msg, sig = (os.path.join(d, f) for f in ("k.pem", "m.bin", "s.bin"))
            subprocess.run(["openssl", "genpkey", "-algorithm", "ed25519", "-out", key], check=True)
            priv = subprocess.run(["openssl", "pkey", "-in", key, "-outform", "DER"],
                                  check=True, capture_output=True).stdout
            pub = subprocess.run(["openssl", "pkey", "-in", key, "-pubout", "-outform", "DER"],
                                 check=True, capture_output=True).stdout
            m = os.urandom(n)
            with open(msg, "wb") as f:
                f.write(m)
            subprocess.run(["openssl", "pkeyutl", "-sign", "-inkey", key, "-rawin", "-in", msg,
                            "-out", sig], check=True)
            with open(sig, "rb") as f:
                s = f.read()
            out.append(dict(seed=priv[-32:].hex(), pk=pub[-32:].hex(), msg=m.hex(), sig=s.hex()))
    with open(os.path.join(HERE, "ed25519_openssl_lens.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
