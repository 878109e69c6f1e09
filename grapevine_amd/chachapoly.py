"""ChaCha20-Poly1305 (RFC 8439 §2.8) in plain Python integers: Noise's
ChaChaPoly, the client's half of a channel that uses `abi.CIPHER_CHACHAPOLY`
and the reference the tests compare the device calls
(`ObliviousStore.chachapoly_seal` / `chachapoly_open`, gvs_chachapoly.h)
against.  `seal` and `open_` have the shape `grapevine_amd.noise` takes its
AEAD in.  Not constant time: for tests, tools and reference clients.

The ChaCha20 block is `server.chacha20_block`: RFC 8439's 32-bit counter and
96-bit nonce are rand_chacha's two 64-bit words read the other way, so the
same function serves both layouts unchanged.
"""
import struct

from .server import chacha20_block

TAG_BYTES = 16
_P = (1 << 130) - 5


def block(key, counter, nonce):
    """The 64-byte block of RFC 8439 §2.3: state words 12 = counter, 13..15 =
    the 12-byte nonce."""
    n0, n1, n2 = struct.unpack("<3I", nonce)
    return chacha20_block(key, (counter & 0xFFFFFFFF) | n0 << 32, n1 | n2 << 32)


def chacha20(key, counter, nonce, data):
    """data XOR the keystream from block `counter` on (§2.4)."""
    ks = b"".join(block(key, counter + k, nonce) for k in range(-(-len(data) // 64)))
    return bytes(a ^ b for a, b in zip(data, ks))


def poly1305(otk, msg):
    """§2.5: the tag of msg under the 32-byte one-time key r | s."""
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(otk[16:32], "little")
    acc = 0
    for o in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[o:o + 16] + b"\x01", "little")) * r % _P
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def mac_data(aad, ct):
    """§2.8: pad16(AAD) | pad16(ciphertext) | le64(|AAD|) | le64(|ciphertext|)."""
    pad = lambda b: bytes(b) + bytes(-len(b) % 16)
    return pad(aad) + pad(ct) + struct.pack("<QQ", len(aad), len(ct))


def seal(key, nonce, aad, pt):
    """-> ciphertext | tag."""
    ct = chacha20(key, 1, nonce, pt)
    return ct + poly1305(block(key, 0, nonce)[:32], mac_data(aad, ct))


def open_(key, nonce, aad, msg):
    """ciphertext | tag -> the plaintext, or None if it does not verify."""
    if len(msg) < TAG_BYTES:
        return None
    ct, tag = msg[:-TAG_BYTES], msg[-TAG_BYTES:]
    if poly1305(block(key, 0, nonce)[:32], mac_data(aad, ct)) != tag:
        return None
    return chacha20(key, 1, nonce, ct)
