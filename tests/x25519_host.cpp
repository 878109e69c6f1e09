// x25519_host.cpp — the device X25519 quad ladder and Noise HKDF
// (grapevine_amd/csrc/gvs_x25519.h, host-callable) built for the CPU: a quad
// is four lane states stepped in a loop, the same schedule the kernel runs
// with DPP moves.  tests/test_x25519.py checks it against the Python
// reference (grapevine_amd/x25519.py) without a GPU.  With -DXHOST_MAIN it is
// a program of its own that runs the fixture file given as its argument (for
// a sanitizer build).  Test infrastructure only.
#include "../grapevine_amd/csrc/gvs_x25519.h"

using namespace gvs::sr;

extern "C" {

// out (32 B) = X25519(scalar, point), point null for the base point.  Returns
// 1 if the result is non-zero, 0 if all zero, -1 if the four lanes of the
// quad disagree (they hold the same canonical result).
int x_host_x25519(const uint8_t* scalar, const uint8_t* point, uint8_t* out) {
  Fe r[4];
  x25519_quad_host(scalar, point, r);
  uint32_t any = 0, diff = 0;
  for (int i = 0; i < 8; ++i) {
    any |= r[0].v[i];
    for (int l = 1; l < 4; ++l) diff |= r[l].v[i] ^ r[0].v[i];
  }
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(r[0].v[i / 4] >> (8 * (i % 4)));
  return diff ? -1 : (any ? 1 : 0);
}

// o1, o2 (64 B each) = Noise HKDF(ck (64 B), ikm (ikm_len = 0 or 32 B))
void x_host_hkdf(const uint8_t* ck, const uint8_t* ikm, uint32_t ikm_len, uint8_t* o1, uint8_t* o2) {
  noise_hkdf_one(ck, ikm, ikm_len, o1, o2);
}
}

#ifdef XHOST_MAIN
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// every quoted string of 64 hex digits in the file, in order: the fixture's
// (scalar, u, out) triples
static std::vector<std::vector<uint8_t>> hex32_strings(const char* path) {
  std::vector<std::vector<uint8_t>> all;
  FILE* f = std::fopen(path, "rb");
  if (!f) return all;
  std::string s;
  for (int c; (c = std::fgetc(f)) != EOF;) s.push_back((char)c);
  std::fclose(f);
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] != '"') continue;
    const size_t e = s.find('"', i + 1);
    if (e == std::string::npos) break;
    if (e - i - 1 == 64) {
      std::vector<uint8_t> b(32);
      unsigned v = 0;
      bool hex = true;
      for (int k = 0; k < 32 && hex; ++k) {
        hex = std::sscanf(s.c_str() + i + 1 + 2 * k, "%2x", &v) == 1;
        b[k] = (uint8_t)v;
      }
      if (hex) all.push_back(b);
    }
    i = e;
  }
  return all;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const auto v = hex32_strings(argv[1]);
  if (v.size() < 3 || v.size() % 3) return 2;
  int bad = 0;
  uint8_t out[32], o1[64], o2[64], ck[64] = {0};
  for (size_t k = 0; k + 2 < v.size(); k += 3) {
    const int ok = x_host_x25519(v[k].data(), v[k + 1].data(), out);
    bad += ok != 1 || std::memcmp(out, v[k + 2].data(), 32) != 0;
    x_host_hkdf(ck, out, 32, o1, o2);  // chained: the sanitizer sees both ikm lengths
    x_host_hkdf(o1, nullptr, 0, ck, o2);
  }
  std::printf("%zu fixtures, %d wrong\n", v.size() / 3, bad);
  return bad ? 1 : 0;
}
#endif
