// gvs_chacha_rounds.h — the ChaCha quarter round and double round over 16
// named registers x0 .. x15, shared by the challenge stream (gvs_chacha.h,
// rand_chacha's state layout) and the channel's second cipher
// (gvs_chachapoly.h, RFC 8439's).  Every index is a compile-time constant, so
// nothing is spilled to scratch.
#pragma once

#define GVS_CC_QR(a, b, c, d)                \
  a += b; d = __builtin_rotateleft32(d ^ a, 16); \
  c += d; b = __builtin_rotateleft32(b ^ c, 12); \
  a += b; d = __builtin_rotateleft32(d ^ a, 8);  \
  c += d; b = __builtin_rotateleft32(b ^ c, 7);

// two rounds: the four columns, then the four diagonals
#define GVS_CC_DR                                                 \
  GVS_CC_QR(x0, x4, x8, x12) GVS_CC_QR(x1, x5, x9, x13)           \
  GVS_CC_QR(x2, x6, x10, x14) GVS_CC_QR(x3, x7, x11, x15)         \
  GVS_CC_QR(x0, x5, x10, x15) GVS_CC_QR(x1, x6, x11, x12)         \
  GVS_CC_QR(x2, x7, x8, x13) GVS_CC_QR(x3, x4, x9, x14)

// the 20 rounds
#define GVS_CC_ROUNDS20                                 \
  GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR     \
  GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR
