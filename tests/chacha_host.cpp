// chacha_host.cpp — the ChaCha20 block function and the draw selection of the
// device challenge stream (grapevine_amd/csrc/gvs_chacha.h, host-callable),
// built for the CPU so that tests/test_chacha_host.py can check them against
// the openssl-made fixture, RFC 8439 and grapevine_amd/server.py without a
// GPU.  Test infrastructure only.
#include "../grapevine_amd/csrc/gvs_chacha.h"

using namespace gvs;

static void key_words(const uint8_t* key, uint32_t w[8]) {
  for (int i = 0; i < 8; ++i)
    w[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 |
           (uint32_t)key[4 * i + 3] << 24;
}

static void put_words(const uint32_t* w, int n, uint8_t* out) {
  for (int i = 0; i < 4 * n; ++i) out[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}

extern "C" {

// out (64 B) = block `counter` of stream `stream` under key (32 B)
void chacha_host_block(const uint8_t* key, uint64_t counter, uint64_t stream, uint8_t* out) {
  uint32_t k[8], b[16];
  key_words(key, k);
  chacha20_block(k, counter, stream, b);
  put_words(b, 16, out);
}

// out (32 B) = draw number `draw` of ChaCha20Rng(seed)
void chacha_host_draw(const uint8_t* seed, uint64_t draw, uint8_t* out) {
  uint32_t k[8], c[8];
  key_words(seed, k);
  challenge_draw(k, draw, c);
  put_words(c, 8, out);
}
}
