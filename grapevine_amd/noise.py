"""Noise_IX_25519_AESGCM_SHA512 in plain Python, written from the Noise
specification (rev. 34): the symmetric state of §5.2 over hashlib / hmac, the
DH of grapevine_amd.x25519, and the two halves of the IX pattern
    -> e, s
    <- e, ee, se, s, es
`Initiator` is the client's half; `respond` is the responder's, the reference
the tests compare the device call (`ObliviousStore.noise_ix_respond`,
gvs_noise_ix_respond) against.  The AEAD is passed in: `seal(key, iv, aad,
plaintext) -> ciphertext | tag` and `open_(key, iv, aad, ciphertext | tag) ->
plaintext or None` (the tests pass tests/test_aead.py's).  `cipher=
abi.CIPHER_CHACHAPOLY` selects Noise_IX_25519_ChaChaPoly_SHA512 instead: the
other protocol name, the little-endian nonce, and grapevine_amd.chachapoly for
an AEAD that is not passed.  Not constant time: for tests, tools and reference
clients.
"""
import hashlib

from . import abi, chachapoly
from .x25519 import noise_hkdf, x25519

PROTOCOL_NAME = b"Noise_IX_25519_AESGCM_SHA512"
PROTOCOL_NAMES = {abi.CIPHER_AESGCM: PROTOCOL_NAME, abi.CIPHER_CHACHAPOLY: b"Noise_IX_25519_ChaChaPoly_SHA512"}
NONCES = {abi.CIPHER_AESGCM: abi.noise_iv, abi.CIPHER_CHACHAPOLY: abi.noise_nonce_chachapoly}
DHLEN, HASHLEN, TAGLEN = 32, 64, 16


class HandshakeError(ValueError):
    pass


class SymmetricState:
    """§5.2, with the CipherState (§5.1) folded in: k is None until the first
    MixKey, and every MixKey sets the nonce back to 0."""

    def __init__(self, seal, open_, cipher=abi.CIPHER_AESGCM):
        # InitializeSymmetric: a name of at most HASHLEN bytes is zero-padded
        name = PROTOCOL_NAMES[cipher]
        self.h = name.ljust(HASHLEN, b"\0") if len(name) <= HASHLEN else hashlib.sha512(name).digest()
        self.ck, self.k, self.n = self.h, None, 0
        self.nonce = NONCES[cipher]
        if cipher == abi.CIPHER_CHACHAPOLY:
            seal, open_ = seal or chachapoly.seal, open_ or chachapoly.open_
        self.seal, self.open_ = seal, open_

    def mix_hash(self, data):
        self.h = hashlib.sha512(self.h + bytes(data)).digest()

    def mix_key(self, ikm):
        self.ck, temp_k = noise_hkdf(self.ck, ikm)
        self.k, self.n = temp_k[:32], 0  # HASHLEN is 64: temp_k is truncated

    def encrypt_and_hash(self, plaintext):
        if self.k is None:
            ct = bytes(plaintext)
        else:
            ct = self.seal(self.k, self.nonce(self.n), self.h, bytes(plaintext))
            self.n += 1
        self.mix_hash(ct)
        return ct

    def decrypt_and_hash(self, ct):
        if self.k is None:
            pt = bytes(ct)
        else:
            pt = self.open_(self.k, self.nonce(self.n), self.h, bytes(ct))
            if pt is None:
                raise HandshakeError("a handshake ciphertext does not verify")
            self.n += 1
        self.mix_hash(ct)
        return pt

    def split(self):
        k1, k2 = noise_hkdf(self.ck)
        return k1[:32], k2[:32]


def dh(secret, public):
    """DH(key_pair, public_key); an all-zero result (a small-order public key)
    is refused, x25519-dalek's was_contributory."""
    out = x25519(secret, public)
    if out == bytes(DHLEN):
        raise HandshakeError("non-contributory DH")
    return out


class Initiator:
    """The client's half: write_message1() -> bytes, then read_message2(msg2)
    -> (k1, k2, h); k1 seals what the initiator sends, k2 opens what it
    receives.  rs and payload2 hold what message 2 carried."""

    def __init__(self, static_secret, ephemeral_secret, seal=None, open_=None, prologue=b"",
                 cipher=abi.CIPHER_AESGCM):
        self.s, self.e = bytes(static_secret), bytes(ephemeral_secret)
        self.ss = SymmetricState(seal, open_, cipher)
        self.ss.mix_hash(prologue)
        self.rs = self.payload2 = None

    def write_message1(self, payload=b""):
        ss = self.ss
        e_pub, s_pub = x25519(self.e), x25519(self.s)
        ss.mix_hash(e_pub)                      # e
        out = e_pub + ss.encrypt_and_hash(s_pub)  # s: no key yet, in clear
        return out + ss.encrypt_and_hash(payload)

    def read_message2(self, msg):
        ss = self.ss
        if len(msg) < DHLEN + DHLEN + TAGLEN + TAGLEN:
            raise HandshakeError("message 2 is too short")
        re = msg[:DHLEN]
        ss.mix_hash(re)                                          # e
        ss.mix_key(dh(self.e, re))                               # ee
        ss.mix_key(dh(self.s, re))                               # se: our static, their ephemeral
        self.rs = ss.decrypt_and_hash(msg[DHLEN:2 * DHLEN + TAGLEN])  # s
        ss.mix_key(dh(self.e, self.rs))                          # es: our ephemeral, their static
        self.payload2 = ss.decrypt_and_hash(msg[2 * DHLEN + TAGLEN:])
        k1, k2 = ss.split()
        return k1, k2, ss.h


def respond(static_secret, ephemeral_secret, msg1, payload, seal=None, prologue=b"", cipher=abi.CIPHER_AESGCM):
    """The responder's half in one step: message 1 -> (message 2, k1, k2, h),
    or None where gvs_noise_ix_respond sets ok = 0 (a message 1 shorter than
    its two keys or longer than them and abi.NOISE_PAYLOAD1_MAX, a
    non-contributory DH).  k1 opens what the initiator sends, k2 seals what
    the responder sends."""
    if not 2 * DHLEN <= len(msg1) <= 2 * DHLEN + abi.NOISE_PAYLOAD1_MAX:
        return None
    ss = SymmetricState(seal, None, cipher)
    ss.mix_hash(prologue)
    re = msg1[:DHLEN]
    ss.mix_hash(re)                                   # e
    rs = ss.decrypt_and_hash(msg1[DHLEN:2 * DHLEN])   # s, in clear
    ss.decrypt_and_hash(msg1[2 * DHLEN:])             # payload 1, in clear
    try:
        e_pub = x25519(ephemeral_secret)
        ss.mix_hash(e_pub)                            # e
        ss.mix_key(dh(ephemeral_secret, re))          # ee
        ss.mix_key(dh(ephemeral_secret, rs))          # se: their static, our ephemeral
        out = e_pub + ss.encrypt_and_hash(x25519(static_secret))  # s
        ss.mix_key(dh(static_secret, re))             # es: their ephemeral, our static
    except HandshakeError:
        return None
    out += ss.encrypt_and_hash(payload)
    k1, k2 = ss.split()
    return out, k1, k2, ss.h
