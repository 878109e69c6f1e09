// gvs_noise_init.h — the initiator's side of Noise_IX_25519_{AESGCM,ChaChaPoly}
// _SHA512 (Noise specification rev. 34, pattern IX: -> e, s   <- e, ee, se, s,
// es) on the device, batched over handshakes: k_noise_ixi<PHASE> is the
// symmetric state between the launches of k_x25519 and the opening ciphers that
// gvs_noise_ix_initiate and gvs_noise_ix_finish chain.
//
// The initiator's chain is not the responder's: es = X(e, rs) needs rs, which
// is known only once ct_s is opened under the key that ee and se give.  So
//   initiate   k_noise_ixi_scalars, k_x25519 (base point: e_pub, s_pub),
//              k_noise_ixi<M1>
//   finish     k_noise_ixi_gather, k_x25519 (ee, se), k_noise_ixi<A>, open ct_s,
//              k_x25519 (es), k_noise_ixi<B>, open ct_p, k_noise_ixi<C>
//
// One DPP quad per handshake at k_x25519's launch shape, the lane roles, the
// HKDF's eight steps, the exchange after every step and the big-endian words of
// gvs_noise.h (NxLane, NxQuadDev, NxQuadHost, nx_xword, nx_blocks).  The step
// tables are this file's; T is the transcript (lanes 2 and 3), K the HKDF
// (lanes 0 and 1), and a transcript of b blocks takes b steps:
//   M1   6 steps    T  prologue 0 1 | e_pub 2 | s_pub 3 | payload 1 4 5
//                   K  dry: no key is mixed before message 2
//   A   16 steps    T  re 0
//                   K  MixKey(ee) 0..7, MixKey(se) 8..15
//   B    8 steps    T  ct_s 0 1
//                   K  MixKey(es) 0..7
//   C   max(8, nx_blocks(ct_p)) steps, 8 .. 17, per handshake
//                   T  ct_p 0 .. nx_blocks(ct_p) - 1
//                   K  Split 0..7
// The Split reads ck alone, so it starts with ct_p's first block and the HMAC
// lanes work through the first eight transcript steps; SHA-512 chains block to
// block, so past those the transcript cannot be shared out and a long ct_p's
// last blocks run with lanes 0 and 1 dry.  A handshake with a short ct_p ends
// after eight steps: the trip count follows its own clear length.
//
// What depends on data: the clear lengths only (the call's prologue and
// payload 1 lengths, msg2_lens per item) drive trip counts and addresses.  The
// secrets, the DH outputs, ck, k, the ciphers' verdicts and ok reach selects
// only; a handshake that fails runs every step and issues every store, with
// zeros (es of a ct_s that did not open is X(e, 0) = 0).
#pragma once
#include "gvs_noise.h"

namespace gvs {
namespace sr {

constexpr int kNxiM1 = 0, kNxiA = 1, kNxiB = 2, kNxiC = 3;
constexpr uint32_t kNxiStateBytes = 64;   // GVS_NOISE_INIT_STATE_BYTES
constexpr uint32_t kNxiPayload2Max = 2048;  // GVS_AEAD_TEXT_MAX: the short form

// a phase's HKDFs on lanes 0 and 1
template <int PH>
__host__ __device__ constexpr int nxi_hkdfs() { return PH == kNxiM1 ? 0 : (PH == kNxiA ? 2 : 1); }

// One call's arrays.  initiate: x25519 item k is e_pub of handshake k, item
// n + k (n: one static for all) is s_pub.  finish: item 2k is ee, 2k + 1 se;
// es has its own launch (xout3, xok3).
struct NxiArgs {
  uint32_t n, s_rows;        // s_rows: 1 a static key per handshake, 0 one for all
  const uint8_t* pro;        // the prologue in a 64-byte cell
  uint32_t pro_len;
  const uint8_t* payload;    // payload 1, payload_stride apart (0: one for all); null when empty
  uint32_t payload_stride, payload_len;
  uint8_t* msg1;             // the caller's slots, msg1_stride (>= 64 + payload_len) apart, written whole
  uint32_t msg1_stride;
  uint32_t* msg1_lens;
  uint8_t* states;           // n x 64 B: h after message 1 (M1 writes, A reads)
  const uint8_t* xout;       // k_x25519's results
  const uint32_t* xok;       // finish: 2n non-zero flags
  const uint8_t* xout3;      // n x 32 B: es
  const uint32_t* xok3;
  const uint8_t* msg2;       // re 32 | ct_s 48 | ct_p, msg2_stride (>= 96) apart
  uint32_t msg2_stride;
  const uint32_t* msg2_lens;
  uint8_t* st;               // n x 128 B between the phases: ck 64 | h 64
  uint8_t* key;              // n x 32 B: the next open's keys
  uint8_t* aad;              // n x 64 B: its AAD (h)
  const uint8_t* ct1;        // n x 48 B: ct_s
  const uint8_t* ct2;        // ct_p, ct2_stride apart
  uint32_t ct2_stride;
  const uint8_t* pt1;        // n x 32 B: what ct_s opened to (zero if it did not)
  const uint8_t* pt2;        // what ct_p opened to, pt2_stride apart
  uint32_t pt2_stride;
  const uint32_t *ok1, *ok2;  // the two opens' verdicts
  uint8_t* rs;               // n x 32 B
  uint8_t* payload2;         // the caller's slots, payload2_stride apart, written whole
  uint32_t payload2_stride;
  uint32_t* payload2_lens;
  uint8_t *send, *recv;      // n x 32 B: k1, k2
  uint8_t* hashes;           // n x 64 B, may be null
  uint32_t* ok;
};

// Message 2's clear length: whether the handshake can go on, and ct_p's length
// (16, an empty payload's, where it cannot: the steps run all the same)
GVS_SR_FN bool nxi_len_ok(const NxiArgs& a, uint32_t len2) {
  return (len2 >= kNxMsg2Fixed) & (len2 <= kNxMsg2Fixed + kNxiPayload2Max) & (len2 <= a.msg2_stride) &
         (len2 - kNxMsg2Fixed <= a.payload2_stride);
}

// The transcript's step table (above): what lanes 2 and 3 hash in step t, block
// b of H(h | s).  False: nothing.
template <int PH>
GVS_SR_FN bool nxi_slot(const NxiArgs& a, uint32_t i, uint32_t ctlen, int t, NxSeg& s, uint32_t& b) {
  b = 0;
  if (PH == kNxiM1) {
    if (t < 2) {  // the prologue: two slots
      s = NxSeg{a.pro, 0u, a.pro_len, kNxPrologueMax};
      b = (uint32_t)t;
    } else if (t == 2) {
      s = NxSeg{a.xout + 32u * (uint64_t)i, 0u, 32u, 32u};  // e_pub
    } else if (t == 3) {
      s = NxSeg{a.xout + 32u * ((uint64_t)a.n + (a.s_rows ? i : 0u)), 0u, 32u, 32u};  // s_pub
    } else if (t < 6) {  // payload 1: two slots, even when it is empty (then the prologue cell, none of it taken)
      s = a.payload_len ? NxSeg{a.payload + (uint64_t)i * a.payload_stride, 0u, a.payload_len, a.payload_len}
                        : NxSeg{a.pro, 0u, 0u, kNxPrologueMax};
      b = (uint32_t)t - 4u;
    } else {
      return false;
    }
  } else if (PH == kNxiA) {
    if (t != 0) return false;
    s = NxSeg{a.msg2 + (uint64_t)i * a.msg2_stride, 0u, 32u, 32u};  // re
  } else if (PH == kNxiB) {
    if (t >= 2) return false;
    s = NxSeg{a.ct1 + 48u * (uint64_t)i, 0u, 48u, 48u};  // ct_s: 112 bytes hashed, two blocks
    b = (uint32_t)t;
  } else {
    if ((uint32_t)t >= nx_blocks(ctlen)) return false;
    s = NxSeg{a.ct2 + (uint64_t)i * a.ct2_stride, 0u, ctlen, a.ct2_stride};  // ct_p
    b = (uint32_t)t;
  }
  return true;
}

// Step t, first half: the lane's block and input state, one compression, the
// result in L.r.  u is the HKDF's step on lanes 0 and 1 (-1: none).
template <int PH>
GVS_SR_FN void nxi_front(const NxiArgs& a, uint32_t i, uint32_t ctlen, int t, uint32_t lane, NxLane& L) {
  constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                               0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                               0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  const int u = t < 8 * nxi_hkdfs<PH>() ? (t & 7) : -1;
  const uint64_t tx = 0ull - (uint64_t)(lane >= 2u);
  uint64_t w[16], s[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = 0;
  bool fresh = false;
  if (u == 0 || u == 3) {  // the padded key block, from the initial state
    const uint64_t pad = lane == 0 ? kNxIpad : kNxOpad;
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.key[j] ^ pad, w[8 + j] = pad;
    fresh = true;
  } else if (u == 1) {  // the HKDF's input: a DH output, or nothing (Split)
    if (PH == kNxiC) {
      w[0] = kNxEnd;
      w[15] = 128u * 8u;
    } else {
      const uint8_t* ikm = PH == kNxiA ? a.xout + 32u * (2u * (uint64_t)i + (uint32_t)(t >> 3))  // ee, then se
                                       : a.xout3 + 32u * (uint64_t)i;                            // es
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = ld_be64(ikm + 8 * j);
      w[4] = kNxEnd;
      w[15] = 160u * 8u;
    }
  } else if (u == 4) {
    w[0] = 0x0180ull << 48;
    w[15] = 129u * 8u;
  } else if (u == 6) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.key[j];  // o1
    w[8] = 0x0280ull << 48;
    w[15] = 193u * 8u;
  } else if (u >= 0) {  // 2, 5, 7: the outer block over the partner's inner digest
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.mb[j];
    w[8] = kNxEnd;
    w[15] = 192u * 8u;
  }
  uint64_t fm = fresh ? ~tx : 0;  // lanes that start from the initial state
  NxSeg sg;
  uint32_t b;
  L.act = L.last = 0;
  if (nxi_slot<PH>(a, i, ctlen, t, sg, b)) {
    const uint32_t nb = nx_blocks(sg.len);
    L.act = 0ull - (uint64_t)(b < nb);
    L.last = 0ull - (uint64_t)(b + 1u == nb);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint64_t x;
      if (b == 0 && j < 8)
        x = L.key[j];  // h
      else
        x = nx_xword(sg, 128u * b + 8u * (uint32_t)j - 64u);
      if (j == 15) x |= L.last & (uint64_t)(64u + sg.len) * 8u;
      w[j] = nx_sel(tx, x, w[j]);
    }
    if (b == 0) fm |= tx;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = L.r[j] = nx_sel(fm, kIv[j], L.hs[j]);
  sha512_rounds<0>(s, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) L.r[j] += s[j];
}

// Step t, second half, after the pairs exchanged results: what each lane keeps
template <int PH>
GVS_SR_FN void nxi_back(int t, uint32_t lane, NxLane& L) {
  const int u = t < 8 * nxi_hkdfs<PH>() ? (t & 7) : -1;
  const uint64_t l0 = 0ull - (uint64_t)(lane == 0u), l1 = 0ull - (uint64_t)(lane == 1u), kk = l0 | l1;
  // lanes 0, 1
  const uint64_t keep_hs = (u == 0 || u == 3) ? kk : ((u == 1 || u == 4 || u == 6) ? l0 : 0);
  const uint64_t both = (u == 2 || u == 5 || u == 7) ? kk : 0;  // lane 1's result, on both lanes
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t o = nx_sel(l1, L.r[j], L.mb[j]);
    L.hs[j] = nx_sel(keep_hs, L.r[j], L.hs[j]);
    if (u == 3) L.ps[j] = nx_sel(kk, L.r[j], L.ps[j]);
    if (u == 2 || u == 5) L.key[j] = nx_sel(both, o, L.key[j]);  // temp; o1, the next ck
    if (u == 5) L.hs[j] = nx_sel(kk, L.ps[j], L.hs[j]);           // o2 starts from temp's pad states too
    if (u == 7) L.ps[j] = nx_sel(both, o, L.ps[j]);               // o2
    // lanes 2, 3
    L.hs[j] = nx_sel(L.act & ~kk, L.r[j], L.hs[j]);
    L.key[j] = nx_sel(L.act & L.last & ~kk, L.r[j], L.key[j]);
  }
}

// What a phase leaves behind, a part per lane
template <int PH>
GVS_SR_FN void nxi_store(const NxiArgs& a, uint32_t i, bool len_ok, uint32_t len2, uint32_t lane, const NxLane& L) {
  const uint64_t all = ~0ull;
  if (PH == kNxiM1) {
    if (lane == 2) nx_st64(a.states + 64u * (uint64_t)i, L.key, 8, all);  // h
    if (lane == 3) a.msg1_lens[i] = 64u + a.payload_len;
    // message 1 = e_pub | s_pub | payload 1, the rest of the slot zero: byte j by lane j % 4
    const uint8_t *ep = a.xout + 32u * (uint64_t)i, *sp = a.xout + 32u * ((uint64_t)a.n + (a.s_rows ? i : 0u)),
                  *pay = a.payload_len ? a.payload + (uint64_t)i * a.payload_stride : a.pro;
    uint8_t* o = a.msg1 + (uint64_t)i * a.msg1_stride;
    for (uint32_t j = lane; j < a.msg1_stride; j += 4u) {
      uint32_t v = 0;
      if (j < 32u)
        v = ep[j];
      else if (j < 64u)
        v = sp[j - 32u];
      else if (j < 64u + a.payload_len)
        v = pay[j - 64u];
      o[j] = (uint8_t)v;
    }
    return;
  }
  if (PH != kNxiC) {
    uint8_t* st = a.st + 128u * (uint64_t)i;
    if (lane == 0) nx_st64(st, L.key, 8, all);                       // ck
    if (lane == 1) nx_st64(a.key + 32u * (uint64_t)i, L.ps, 4, all);  // k = o2[0:32]
    if (lane == 2) {
      nx_st64(st + 64, L.key, 8, all);  // h, and h as the open's AAD
      nx_st64(a.aad + 64u * (uint64_t)i, L.key, 8, all);
    }
    return;
  }
  // the three DH flags and the two verdicts, merged without a branch
  const uint32_t good = (uint32_t)len_ok & (uint32_t)(a.xok[2u * (uint64_t)i] != 0) &
                        (uint32_t)(a.xok[2u * (uint64_t)i + 1u] != 0) & (uint32_t)(a.xok3[i] != 0) &
                        (uint32_t)(a.ok1[i] != 0) & (uint32_t)(a.ok2[i] != 0);
  const uint64_t m = 0ull - (uint64_t)good;
  if (lane == 0) nx_st64(a.send + 32u * (uint64_t)i, L.key, 4, m);  // k1 = o1[0:32]
  if (lane == 1) nx_st64(a.recv + 32u * (uint64_t)i, L.ps, 4, m);   // k2 = o2[0:32]
  if (lane == 2 && a.hashes) nx_st64(a.hashes + 64u * (uint64_t)i, L.key, 8, m);
  if (lane == 3) {
    a.ok[i] = good;
    a.payload2_lens[i] = (len2 - kNxMsg2Fixed) & (uint32_t)m;
  }
  const uint8_t *r = a.pt1 + 32u * (uint64_t)i, *p = a.pt2 + (uint64_t)i * a.pt2_stride;
#pragma unroll
  for (uint32_t j = 0; j < 8u; ++j) a.rs[32u * (uint64_t)i + 4u * j + lane] = (uint8_t)(r[4u * j + lane] & (uint32_t)m);
  // payload 2, the rest of the slot zero: byte j by lane j % 4
  const uint32_t plen = len_ok ? len2 - kNxMsg2Fixed : 0u;  // <= pt2_stride
  uint8_t* o = a.payload2 + (uint64_t)i * a.payload2_stride;
  for (uint32_t j = lane; j < a.payload2_stride; j += 4u) {
    const uint32_t v = p[j < plen ? j : 0u];
    o[j] = (uint8_t)((j < plen ? v : 0u) & (uint32_t)m);
  }
}

// One handshake's phase: load, the schedule, store (live: not a tail quad's
// repeat of the last item).  CHACHAPOLY: the suite's cipher, which only the
// protocol name sees: h0 of M1, and ck of A (no key is mixed before message 2)
template <int PH, bool CHACHAPOLY, class Q>
GVS_SR_FN_NI void nxi_item(Q& q, const NxiArgs& a, uint32_t i, bool live) {
  const uint32_t len2 = PH == kNxiC ? a.msg2_lens[i] : 0u;
  const bool len_ok = PH == kNxiC ? nxi_len_ok(a, len2) : true;
  const uint32_t ctlen = len_ok ? len2 - 80u : 16u;
  q.each([&](uint32_t lane, NxLane& L) {
    constexpr uint64_t kNameGcm[8] = {0x4e6f6973655f4958ull, 0x5f32353531395f41ull, 0x455347434d5f5348ull,
                                      0x4135313200000000ull, 0, 0, 0, 0};
    constexpr uint64_t kNameCp[8] = {0x4e6f6973655f4958ull, 0x5f32353531395f43ull, 0x6861436861506f6cull,
                                     0x795f534841353132ull, 0, 0, 0, 0};
    const bool name = PH == kNxiM1 || (PH == kNxiA && lane < 2u);
    const uint8_t* st = PH == kNxiM1 ? nullptr
                        : PH == kNxiA ? a.states + 64u * (uint64_t)i
                                      : a.st + 128u * (uint64_t)i + (lane >= 2u ? 64u : 0u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t nm = CHACHAPOLY ? kNameCp[j] : kNameGcm[j];
      L.key[j] = PH == kNxiM1 ? nm : nx_sel(0ull - (uint64_t)name, nm, ld_be64(st + 8 * j));
      L.hs[j] = L.ps[j] = L.mb[j] = L.r[j] = 0;
    }
    L.act = L.last = 0;
  });
  const int hk = 8 * nxi_hkdfs<PH>(), nb = (int)nx_blocks(ctlen);
  const int steps = PH == kNxiM1 ? 6 : (PH == kNxiC ? (nb > hk ? nb : hk) : hk);
#pragma unroll 1
  for (int t = 0; t < steps; ++t) {
    q.each([&](uint32_t lane, NxLane& L) { nxi_front<PH>(a, i, ctlen, t, lane, L); });
    q.swap();
    q.each([&](uint32_t lane, NxLane& L) { nxi_back<PH>(t, lane, L); });
  }
  if (live) q.each([&](uint32_t lane, NxLane& L) { nxi_store<PH>(a, i, len_ok, len2, lane, L); });
}

// Host form (tests/noise_init_host.cpp): one handshake's phase on four lane
// states.  False if the lanes disagree where they hold the same value: ck and
// o2 on lanes 0 and 1, h on lanes 2 and 3.
template <int PH, bool CHACHAPOLY>
inline bool nxi_item_host(const NxiArgs& a, uint32_t i) {
  NxQuadHost q;
  nxi_item<PH, CHACHAPOLY>(q, a, i, true);
  uint64_t d = 0;
  for (int j = 0; j < 8; ++j)
    d |= (q.L[0].key[j] ^ q.L[1].key[j]) | (q.L[0].ps[j] ^ q.L[1].ps[j]) | (q.L[2].key[j] ^ q.L[3].key[j]);
  return d == 0;
}

#if defined(__HIPCC__)

// phases B and C do not see the protocol name: they are built for CHACHAPOLY = false only
template <int PH, bool CHACHAPOLY = false>
__global__ void __launch_bounds__(kXThreads) k_noise_ixi(NxiArgs a) {
  const uint32_t k = blockIdx.x * kXItems + (threadIdx.x >> 2);
  const uint32_t kk = k < a.n ? k : a.n - 1;  // tail quads redo the last item: every lane stays in the DPP moves
  NxQuadDev q;
  q.lane = threadIdx.x & 3u;
  nxi_item<PH, CHACHAPOLY>(q, a, kk, k < a.n);
}

// initiate's first launch: the n + (1 or n) scalars of the base-point
// multiplications in one array of k_x25519's fixed stride, and the prologue cell
struct NxiScalarArgs {
  uint8_t pro[64];         // the prologue, zero-padded
  const uint8_t* eph;      // n x 32 B
  const uint8_t* statics;  // static_stride apart (0: one)
  uint32_t static_stride, n;
  uint8_t* xsc;            // (n + (static_stride ? n : 1)) x 32 B
  uint8_t* pro_out;        // 64 B
};

__global__ void __launch_bounds__(kXThreads) k_noise_ixi_scalars(NxiScalarArgs a) {
  const uint32_t r = blockIdx.x * kXThreads + threadIdx.x, rows = a.n + (a.static_stride ? a.n : 1u);
  if (r < rows) {
    const uint8_t* src = r < a.n ? a.eph + 32u * (uint64_t)r : a.statics + (uint64_t)(r - a.n) * a.static_stride;
#pragma unroll
    for (int j = 0; j < 32; ++j) a.xsc[32u * (uint64_t)r + j] = src[j];
  }
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < 64; ++j) a.pro_out[j] = a.pro[j];
  }
}

// finish's first launch: k_x25519's 2n (scalar, point) rows, (e, re) and
// (s, re); ct_s and ct_p out of the caller's slots into rows the ciphers can
// read (16-byte aligned, strides in whole blocks); the opens' nonces (Noise's
// counter 0: all zero) and lengths.  A message 2 of a bad length opens as 0
// bytes, which the cipher refuses.
struct NxiGatherArgs {
  const uint8_t* eph;      // n x 32 B
  const uint8_t* statics;  // static_stride apart (0: one)
  uint32_t static_stride;
  const uint8_t* msg2;
  uint32_t msg2_stride;
  const uint32_t* msg2_lens;
  uint32_t payload2_stride, ct2_stride, n;
  uint8_t *xsc, *xpt;      // 2n x 32 B each
  uint8_t *ct1, *ct2;
  uint32_t* iv;            // n x 12 B
  uint32_t *aad_lens, *len1, *len2;
};

__global__ void __launch_bounds__(kXThreads) k_noise_ixi_gather(NxiGatherArgs a) {
  const uint32_t i = blockIdx.x * kXItems + (threadIdx.x >> 2), k = threadIdx.x & 3u;
  if (i < a.n) {
    const uint8_t* m2 = a.msg2 + (uint64_t)i * a.msg2_stride;
    if (k < 2u) {  // row 2i + k
      const uint8_t* sc = k == 0u ? a.eph + 32u * (uint64_t)i : a.statics + (uint64_t)i * a.static_stride;
      uint8_t *so = a.xsc + 32u * (2u * (uint64_t)i + k), *po = a.xpt + 32u * (2u * (uint64_t)i + k);
#pragma unroll
      for (int j = 0; j < 32; ++j) so[j] = sc[j], po[j] = m2[j];
    } else {  // ct_s, 24 bytes each
      const uint32_t o = 24u * (k - 2u);
#pragma unroll
      for (int j = 0; j < 24; ++j) a.ct1[48u * (uint64_t)i + o + j] = m2[32u + o + j];
    }
    if (k < 3u) a.iv[3u * (uint64_t)i + k] = 0;
    if (k == 3u) {
      const uint32_t len = a.msg2_lens[i];
      const bool len_ok = (len >= kNxMsg2Fixed) & (len <= kNxMsg2Fixed + kNxiPayload2Max) & (len <= a.msg2_stride) &
                          (len - kNxMsg2Fixed <= a.payload2_stride);
      a.aad_lens[i] = 64u, a.len1[i] = 48u, a.len2[i] = len_ok ? len - 80u : 0u;
    }
  }
  // the workgroup's 64 ct_p rows, byte after byte across its threads
  const uint32_t i0 = blockIdx.x * kXItems;
  for (uint32_t x = threadIdx.x; x < kXItems * a.ct2_stride; x += kXThreads) {
    const uint32_t it = i0 + x / a.ct2_stride, off = x % a.ct2_stride;
    if (it >= a.n) break;
    a.ct2[(uint64_t)it * a.ct2_stride + off] =
        80u + off < a.msg2_stride ? a.msg2[(uint64_t)it * a.msg2_stride + 80u + off] : (uint8_t)0;
  }
}

#endif  // __HIPCC__

}  // namespace sr
}  // namespace gvs
