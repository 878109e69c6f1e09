"""The client's half of the channel's key agreement, in plain Python: X25519
(RFC 7748 §5) on Python integers and Noise's HKDF (two outputs) over hmac /
hashlib SHA-512.  The batched device forms are `ObliviousStore.x25519` and
`ObliviousStore.noise_hkdf` (gvs_x25519, gvs_noise_hkdf); these are what a
client runs for its own handshake, and the references the tests compare the
kernels against.  Not constant time: for tests, tools and reference clients,
not for keys that matter.
"""
import hashlib
import hmac

P = 2 ** 255 - 19
A24 = 121665
BASE_POINT = (9).to_bytes(32, "little")


def clamp(scalar):
    """decodeScalar25519: 32 bytes -> the integer the ladder runs on."""
    k = int.from_bytes(bytes(scalar), "little")
    return (k & ((1 << 254) - 8)) | (1 << 254)


def x25519(scalar, u=BASE_POINT):
    """X25519(scalar, u) -> 32 bytes.  The top bit of u is ignored and a
    non-canonical u (>= p) is reduced, as RFC 7748 asks; an all-zero result
    (a small-order u) is returned as it is: the caller decides."""
    k = clamp(scalar)
    x1 = (int.from_bytes(bytes(u), "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = k >> t & 1
        if swap ^ bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = aa - bb
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def noise_hkdf(ck, ikm=b""):
    """Noise's HKDF(chaining_key, input_key_material, 2) with HMAC-SHA-512:
    (o1, o2), 64 bytes each.  MixKey(dh) is ck, k = o1, o2[:32]; Split() is
    noise_hkdf(ck) with the two cipher keys o1[:32] and o2[:32]."""
    mac = lambda key, msg: hmac.new(bytes(key), bytes(msg), hashlib.sha512).digest()
    temp = mac(ck, ikm)
    o1 = mac(temp, b"\x01")
    return o1, mac(temp, o1 + b"\x02")
