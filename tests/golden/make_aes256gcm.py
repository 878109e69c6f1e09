"""Generate tests/golden/aes256gcm_openssl.json: AES-256-GCM ciphertexts and
tags made by OpenSSL 3.0's libcrypto (EVP_aes_256_gcm through ctypes; the
openssl CLI has no AEAD mode) under random keys and 96-bit IVs, for every pair
of a text length in 0, 1, 16, 17, 1042 (a wire response), 1099 (a wire request)
and an AAD length in 0, 20.

    python tests/golden/make_aes256gcm.py
"""
import ctypes
import ctypes.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TEXT_LENS = (0, 1, 16, 17, 1042, 1099)
AAD_LENS = (0, 20)
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def seal(c, key, iv, aad, pt):
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    c.EVP_CIPHER_CTX_new.restype = vp
    c.EVP_aes_256_gcm.restype = vp
    c.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
    c.EVP_EncryptUpdate.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32), ctypes.c_char_p, i32]
    c.EVP_EncryptFinal_ex.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
    c.EVP_CIPHER_CTX_ctrl.argtypes = [vp, i32, i32, vp]
    c.EVP_CIPHER_CTX_free.argtypes = [vp]
    ctx, n = c.EVP_CIPHER_CTX_new(), i32(0)
    assert c.EVP_EncryptInit_ex(ctx, c.EVP_aes_256_gcm(), None, None, None) == 1
    assert c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, 12, None) == 1
    assert c.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
    if aad:
        assert c.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
    ct = ctypes.create_string_buffer(len(pt) + 16)
    if pt:
        assert c.EVP_EncryptUpdate(ctx, ct, ctypes.byref(n), pt, len(pt)) == 1 and n.value == len(pt)
    assert c.EVP_EncryptFinal_ex(ctx, None, ctypes.byref(n)) == 1
    tag = ctypes.create_string_buffer(16)
    assert c.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, ctypes.cast(tag, vp)) == 1
    c.EVP_CIPHER_CTX_free(ctx)
    return ct.raw[:len(pt)], tag.raw


def main():
    c = ctypes.CDLL(ctypes.util.find_library("crypto"))
    out = []
    for n in TEXT_LENS:
        for a in AAD_LENS:
            key, iv, aad, pt = os.urandom(32), os.urandom(12), os.urandom(a), os.urandom(n)
            ct, tag = seal(c, key, iv, aad, pt)
            out.append(dict(key=key.hex(), iv=iv.hex(), aad=aad.hex(), pt=pt.hex(), ct=ct.hex(), tag=tag.hex()))
    with open(os.path.join(HERE, "aes256gcm_openssl.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
