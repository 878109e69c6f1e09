"""Ed25519 signing for clients of a store created with `ed25519_auth=True`
(GVS_FLAG_ED25519_AUTH): RFC 8032 §5.1.5 (key generation) and §5.1.6 (sign),
pure Ed25519 with no context, in plain Python on hashlib.sha512.

`Ed25519Signer` fits `GrapevineClient`'s signer protocol (`.public_key`,
`.sign(challenge) -> 64 B`): the signed message is the 32 challenge bytes.
Signing is a client-side step of a few milliseconds per request; the batched
verification is the device kernel (gvs_ed25519_verify).  Not constant time:
for tests, tools and reference clients, not for keys that matter.
"""
import hashlib

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P


def _add(p, q):
    """Extended coordinates, a = -1 (RFC 8032 §5.1.4)."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def _encode(p):
    x, y, z, _ = p
    zi = pow(z, P - 2, P)
    x, y = x * zi % P, y * zi % P
    return (y | (x & 1) << 255).to_bytes(32, "little")


def _base():
    y = 4 * pow(5, P - 2, P) % P
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if x & 1:
        x = P - x
    return x, y, 1, x * y % P


BASE = _base()
_BASE_POW2 = []  # [2^i]B, filled on first use


def _mul_base(k):
    """[k]B for k < 2^256 from the doublings of B (additions only)."""
    if not _BASE_POW2:
        p = BASE
        for _ in range(256):
            _BASE_POW2.append(p)
            p = _add(p, p)
    acc = (0, 1, 1, 0)
    for i in range(k.bit_length()):
        if k >> i & 1:
            acc = _add(acc, _BASE_POW2[i])
    return acc


class Ed25519Signer:
    """The key pair of a 32-byte seed (the RFC 8032 private key)."""

    def __init__(self, seed):
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("an Ed25519 seed is 32 bytes")
        h = hashlib.sha512(seed).digest()
        a = int.from_bytes(h[:32], "little")
        self._a = (a & ((1 << 254) - 8)) | (1 << 254)  # clamp: §5.1.5 step 2
        self._prefix = h[32:]
        self.public_key = _encode(_mul_base(self._a))

    def sign(self, message):
        message = bytes(message)
        r = int.from_bytes(hashlib.sha512(self._prefix + message).digest(), "little") % L
        r_bytes = _encode(_mul_base(r))
        k = int.from_bytes(hashlib.sha512(r_bytes + self.public_key + message).digest(), "little") % L
        return r_bytes + ((r + k * self._a) % L).to_bytes(32, "little")
