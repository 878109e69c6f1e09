"""Generate tests/golden/chacha20_openssl_counters.json: two ChaCha20 blocks
(128 bytes of keystream) from the openssl CLI at block counters away from 0.
openssl's 16-byte IV is the little-endian 32-bit block counter followed by the
96-bit nonce; packed as two little-endian 64-bit words (counter, 0) it is
rand_chacha's layout with a 64-bit block counter and stream 0, and openssl
carries the counter from its low word into the next one as that layout does.
The counters sit at 0, 1, either side of the carry out of the low 32 bits, and
the top of the signed 64-bit range.  tests/test_chacha_host.py checks the
device block function (grapevine_amd/csrc/gvs_chacha.h, built for the CPU)
and grapevine_amd/server.py's against it.

    python tests/golden/make_chacha20_counters.py
"""
import json
import os
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTERS = (0, 1, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, (1 << 63) - 1)


def main():
    out = []
    with tempfile.TemporaryDirectory() as d:
        zin, zout = os.path.join(d, "z"), os.path.join(d, "k")
        with open(zin, "wb") as f:
            f.write(bytes(128))
        for key in (bytes(range(32)), os.urandom(32), os.urandom(32)):
            for counter in COUNTERS:
                iv = struct.pack("<QQ", counter, 0)
                subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex(),
                                "-in", zin, "-out", zout], check=True)
                with open(zout, "rb") as f:
                    out.append(dict(key=key.hex(), counter=str(counter), keystream=f.read().hex()))
    with open(os.path.join(HERE, "chacha20_openssl_counters.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
