"""Ed25519 test cases shared by tests/test_ed_host.py (the device code built
for the CPU) and tests/test_gpu_ed25519.py (the kernel): the openssl fixture,
and signed messages with every kind of tampering in rotation."""
import json
import os

from grapevine_amd.ed25519 import Ed25519Signer
from oracle import sr25519 as sr

HERE = os.path.dirname(os.path.abspath(__file__))

# a quarter of the slots are untouched so that valid signatures stay in the mix
KINDS = ("none", "r_bit", "s_bit", "s_plus_l", "other_key", "other_msg", "none", "random_pk",
         "random_sig", "pk_ge_p", "pk_sign", "none")


def fixture():
    with open(os.path.join(HERE, "golden", "ed25519_openssl_lens.json")) as f:
        return [{k: bytes.fromhex(v) for k, v in rec.items()} for rec in json.load(f)]


def cases(rng, n, msg_len):
    """n (pk, msg, sig, kind) tuples signed by Ed25519Signer, KINDS in rotation."""
    signers = [Ed25519Signer(rng.randbytes(32)) for _ in range(8)]
    out = []
    for i in range(n):
        j = i % len(signers)
        msg = rng.randbytes(msg_len)
        sig = bytearray(signers[j].sign(msg))
        pk = bytearray(signers[j].public_key)
        kind = KINDS[i % len(KINDS)]
        if kind == "r_bit":
            sig[rng.randrange(32)] ^= 1 << rng.randrange(8)
        elif kind == "s_bit":
            sig[32 + rng.randrange(32)] ^= 1 << rng.randrange(8)
        elif kind == "s_plus_l":
            big = int.from_bytes(sig[32:], "little") + sr.L  # same scalar mod l, not canonical
            if big < 1 << 256:
                sig[32:] = big.to_bytes(32, "little")
        elif kind == "other_key":
            pk = bytearray(signers[(j + 1) % len(signers)].public_key)
        elif kind == "other_msg" and msg_len:
            msg = bytes([msg[0] ^ 0x80]) + msg[1:]
        elif kind == "random_pk":
            pk = bytearray(rng.randbytes(32))
        elif kind == "random_sig":
            sig = bytearray(rng.randbytes(64))
        elif kind == "pk_ge_p":
            pk = bytearray((sr.P + rng.randrange(19) | rng.randrange(2) << 255).to_bytes(32, "little"))
        elif kind == "pk_sign":
            pk[31] ^= 0x80
        out.append((bytes(pk), msg, bytes(sig), kind))
    return out


def bit_flips(rec):
    """The fixture record with one bit flipped in each of R, s, pk and msg."""
    out = []
    for field, at in (("sig", 5), ("sig", 40), ("pk", 9), ("msg", 0)):
        t = dict(rec)
        b = bytearray(t[field])
        b[at % len(b)] ^= 0x10
        t[field] = bytes(b)
        out.append(t)
    return out


def small_order_cases():
    """(pk, msg, sig) on keys of small order: the identity (y = 1) with
    sig = encode([s]B) || s, which the cofactorless rule accepts for any
    message (h*A is the identity); the same key with the sign bit set (not a
    strict encoding); y = p - 1 (order 2) and y = 0 (order 4)."""
    out = []
    ident = (1).to_bytes(32, "little")
    for s in (0, 5, sr.L - 1):
        sig = sr._ed_encode(sr.scalar_mult(s, sr.BASE)) + s.to_bytes(32, "little")
        out.append((ident, b"small order %d" % (s % 7), sig))
        out.append(((1 | 1 << 255).to_bytes(32, "little"), b"small order %d" % (s % 7), sig))
        for y in (sr.P - 1, 0):
            for sign in (0, 1):
                out.append(((y | sign << 255).to_bytes(32, "little"), b"small order %d" % (s % 7), sig))
    return out
