// noise_planes_check.cpp — csrc/noise_planes.h against a per-pixel brute force
// of its definitions (tests/test_noise_planes_cpu.py).  For every generated
// bit-plane: each word's l3, candidate, zone and small bits, and the seq /
// clear sets for intensities 2, 3, 4 and (all_seq) 6.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "noise_planes.h"

namespace {

struct Image {
  int W, H, nwr;
  std::vector<uint8_t> px;      // 1 = dark
  std::vector<uint32_t> plane;  // the packed plane, exactly nwr * H words
  Image(int w, int h) : W(w), H(h), nwr((w + 31) >> 5), px((size_t)w * h, 0) {}
  void set(int x, int y) {
    if (x >= 0 && y >= 0 && x < W && y < H) px[(size_t)y * W + x] = 1;
  }
  bool dark(int x, int y) const { return x >= 0 && y >= 0 && x < W && y < H && px[(size_t)y * W + x]; }
  void pack() {
    plane.assign((size_t)nwr * H, 0u);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++)
        if (px[(size_t)y * W + x]) plane[(size_t)y * nwr + (x >> 5)] |= 1u << (x & 31);
  }
};

uint32_t rng_state = 12345u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

void salt(Image& im, double density) {
  const uint32_t thr = (uint32_t)(density * (1 << 24));
  for (auto& p : im.px) p = rnd() < thr;
}
void thirds(Image& im) {
  for (int y = 0; y < im.H; y += 3)
    for (int x = 0; x < im.W; x += 3) im.set(x, y);
}
// The hand-placed cases, at row phase y0: small components at the word and
// zone edges, chains and L shapes across a word boundary, an l3 block whose
// dilation crosses words, pairs at Chebyshev 7 and 8, the image's last
// column, row and partial word.
void placed(Image& im, int y0) {
  static const int xs[8] = {30, 31, 32, 33, 62, 63, 64, 65};
  int y = y0;
  for (int n = 1; n <= 4; n++, y += 40)  // horizontal runs of 1..4, 10 rows apart
    for (int i = 0; i < 8; i++)
      for (int k = 0; k < n; k++) im.set(xs[i] + k, y + 10 * (i & 3));
  for (int n = 4; n <= 5; n++, y += 12) {  // diagonal chains of 4 and 5 across x = 63 | 64, 95 | 96
    for (int k = 0; k < n; k++) im.set(62 + k, y + k);
    for (int k = 0; k < n; k++) im.set(97 - k, y + k);
  }
  for (int k = 0; k < 3; k++) {  // L shapes of 4 and 5 across x = 63 | 64
    im.set(62 + k, y);
    im.set(126 + k, y);
  }
  im.set(62, y + 1);
  im.set(126, y + 1);
  im.set(126, y + 2);
  y += 12;
  for (int r = 0; r < 3; r++)  // 3x3 block ending at x = 31, tail at 32, 33
    for (int c = 0; c < 3; c++) im.set(29 + c, y + r);
  im.set(32, y + 1);
  im.set(33, y + 1);
  for (int r = 0; r < 3; r++)  // the same at x = 63
    for (int c = 0; c < 3; c++) im.set(61 + c, y + r);
  im.set(64, y + 1);
  im.set(65, y + 1);
  y += 12;
  im.set(60, y);  // pairs at Chebyshev 7 and 8 across x = 63 | 64, and a row apart
  im.set(67, y);
  im.set(92, y);
  im.set(100, y);
  im.set(124, y);
  im.set(131, y + 1);
  im.set(156, y);
  im.set(164, y + 1);
  y += 12;
  for (int e = 0; e < 2; e++) {  // components on x = 31 | 32 and 39 | 40
    im.set(31 + 8 * e, y);
    im.set(32 + 8 * e, y + 3);
    im.set(31 + 8 * e, y + 6);
    im.set(32 + 8 * e, y + 6);
  }
  y += 12;
  for (int k = 0; k < 2; k++) {  // the last column and the partial last word
    im.set(im.W - 1, y + 5 * k);
    im.set(im.W - 1 - k, y + 2);
    im.set((im.W - 1) & ~31, y + 5 * k);
    im.set(((im.W - 1) & ~31) - 1, y + 5 * k + 1);
  }
  for (int x = 40; x < im.W; x += 9) {  // the last rows
    im.set(x, im.H - 1);
    if (x % 2) im.set(x + 1, im.H - 2);
  }
  for (int yy = 31; yy <= 40; yy += 3) {  // rows 31 | 32 and 39 | 40
    im.set(50 + 10 * (yy - 31), yy);
    im.set(51 + 10 * (yy - 31), yy + (yy & 1));
  }
}

// ---- the definitions, pixel by pixel ---------------------------------------
struct Brute {
  const Image& im;
  std::vector<uint8_t> l3, cand, small;
  explicit Brute(const Image& i) : im(i), l3(i.px.size()), cand(i.px.size()), small(i.px.size()) {
    for (int y = 0; y < im.H; y++)
      for (int x = 0; x < im.W; x++) {
        int n = 0;
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) n += im.dark(x + dx, y + dy);
        l3[at(x, y)] = im.dark(x, y) && n >= 5;
      }
    for (int y = 0; y < im.H; y++)
      for (int x = 0; x < im.W; x++) {
        bool near = false;
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) near |= is(l3, x + dx, y + dy);
        cand[at(x, y)] = im.dark(x, y) && !near;
        small[at(x, y)] = im.dark(x, y) && component(x, y).size() <= 4;
      }
  }
  size_t at(int x, int y) const { return (size_t)y * im.W + x; }
  bool is(const std::vector<uint8_t>& p, int x, int y) const {
    return x >= 0 && y >= 0 && x < im.W && y < im.H && p[at(x, y)];
  }
  // the 8-connected dark component of (x, y), given up beyond 5 pixels
  std::vector<std::pair<int, int>> component(int x, int y) const {
    std::vector<std::pair<int, int>> c{{x, y}};
    for (size_t i = 0; i < c.size() && c.size() <= 4; i++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const std::pair<int, int> q{c[i].first + dx, c[i].second + dy};
          if (im.dark(q.first, q.second) && std::find(c.begin(), c.end(), q) == c.end()) c.push_back(q);
        }
    return c;
  }
  bool ring_test(int x, int y, int N) const {
    int count = 1;
    for (int L = 1; L <= N; L++) {
      int lc = 0;
      for (int dy = -L; dy <= L; dy++)
        for (int dx = -L; dx <= L; dx++)
          if (std::max(abs(dx), abs(dy)) == L) lc += im.dark(x + dx, y + dy);
      count += lc;
      if (!lc) break;
    }
    return count <= N;
  }
  void lists(int N, std::vector<uint32_t>& seq, std::vector<uint32_t>& clear) const {
    const bool all_seq = N > 4;
    for (int y = 0; y < im.H; y++)
      for (int x = 0; x < im.W; x++) {
        if (!im.dark(x, y)) continue;
        const uint32_t key = ((uint32_t)y << 16) | (uint32_t)x;
        if (all_seq) {
          seq.push_back(key);
          continue;
        }
        if (x < 32 || y < 32) {
          if (!(x >= 8 && y >= 7 && l3[at(x, y)])) seq.push_back(key);
          continue;
        }
        if (!small[at(x, y)]) continue;
        const auto c = component(x, y);
        int x0 = x, x1 = x, y0 = y, y1 = y;
        for (auto& p : c) {
          x0 = std::min(x0, p.first);
          x1 = std::max(x1, p.first);
          y0 = std::min(y0, p.second);
          y1 = std::max(y1, p.second);
        }
        bool eligible = x0 >= 40 && y0 >= 40;
        if (eligible) {
          size_t cnt = 0;
          for (int yy = y0 - 7; yy <= y1 + 7; yy++)
            for (int xx = x0 - 7; xx <= x1 + 7; xx++) cnt += is(small, xx, yy);
          eligible = cnt == c.size();
        }
        if (!eligible) {
          seq.push_back(key);
          continue;
        }
        bool clr = false;
        for (auto& p : c) clr |= ring_test(p.first, p.second, N);
        if (clr) clear.push_back(key);
      }
  }
};

int failures = 0;
void fail(const char* what, const Image& im, const char* name, int a, int b) {
  if (failures++ < 20) printf("FAIL %s: %s %dx%d at (%d, %d)\n", what, name, im.W, im.H, a, b);
}

constexpr int R = 16;  // the kernels' rows a thread

void check(Image& im, const char* name) {
  im.pack();
  const Brute bf(im);
  const NpPlane P{im.plane.data(), im.nwr, im.H};
  std::vector<uint32_t> small(im.plane.size(), 0u);
  std::vector<uint32_t> zone[2] = {std::vector<uint32_t>(small.size()), std::vector<uint32_t>(small.size())};
  for (int y0 = 0; y0 < im.H; y0 += R)
    for (int wi = 0; wi < im.nwr; wi++) {
      uint32_t l3w[R], cw[R], zw[R], za[R];
      np_strip<R>(P, wi, y0, 0, l3w, cw, zw);
      np_strip<R>(P, wi, y0, 1, l3w, cw, za);
      for (int r = 0; r < R && y0 + r < im.H; r++) {
        const int y = y0 + r;
        uint32_t sw = 0;
        for (int b = 0; b < 32; b++) {
          const int x = 32 * wi + b;
          const bool in = x < im.W;
          if (((l3w[r] >> b) & 1) != (in && bf.l3[bf.at(x, y)])) fail("l3", im, name, x, y);
          if (((cw[r] >> b) & 1) != (in && bf.cand[bf.at(x, y)])) fail("cand", im, name, x, y);
          if (((za[r] >> b) & 1) != (uint32_t)im.dark(x, y)) fail("zone (all_seq)", im, name, x, y);
          const bool z = im.dark(x, y) && (x < 32 || y < 32) && !(x >= 8 && y >= 7 && bf.l3[bf.at(x, y)]);
          if (((zw[r] >> b) & 1) != z) fail("zone", im, name, x, y);
          if ((cw[r] >> b) & 1) {
            uint32_t comp[9], D[9];
            if (np_flood9(P, x, y, comp, D) <= kNpSmallMax) sw |= 1u << b;
          }
          if (((sw >> b) & 1) != (in && bf.small[bf.at(x, y)])) fail("small", im, name, x, y);
        }
        small[(size_t)y * im.nwr + wi] = sw;
        zone[0][(size_t)y * im.nwr + wi] = zw[r];
        zone[1][(size_t)y * im.nwr + wi] = za[r];
      }
    }
  const NpPlane S{small.data(), im.nwr, im.H};
  static const int Ns[4] = {2, 3, 4, 6};
  for (int N : Ns) {
    std::vector<uint32_t> seq, clear, bseq, bclear;
    const bool all_seq = N > 4;
    for (int y = 0; y < im.H; y++)
      for (int x = 0; x < im.W; x++) {
        const size_t w = (size_t)y * im.nwr + (x >> 5);
        const uint32_t key = ((uint32_t)y << 16) | (uint32_t)x;
        if ((zone[all_seq][w] >> (x & 31)) & 1) seq.push_back(key);
        if (all_seq || x < kNpZone || y < kNpZone || !((small[w] >> (x & 31)) & 1)) continue;
        const int v = np_verdict(P, S, x, y, N);
        if (v == NP_SEQ) seq.push_back(key);
        if (v == NP_CLEAR) clear.push_back(key);
      }
    bf.lists(N, bseq, bclear);
    if (seq != bseq) fail("seq set", im, name, N, (int)seq.size() - (int)bseq.size());
    if (clear != bclear) fail("clear set", im, name, N, (int)clear.size() - (int)bclear.size());
  }
}

}  // namespace

int main() {
  static const int sizes[8][2] = {{1, 1},   {31, 50},  {32, 41},   {33, 200},
                                  {65, 130}, {97, 83}, {129, 257}, {2480, 96}};
  int planes = 0;
  for (auto& sz : sizes) {
    static const double dens[3] = {0.02, 0.12, 0.55};
    for (double d : dens) {
      Image im(sz[0], sz[1]);
      salt(im, d);
      check(im, "salt");
      planes++;
    }
    {
      Image im(sz[0], sz[1]);
      thirds(im);
      check(im, "thirds");
      planes++;
    }
    for (int y0 = 40; y0 < 56; y0++) {  // every phase of a 16-row strip
      Image im(sz[0], sz[1]);
      placed(im, y0);
      check(im, "placed");
      planes++;
    }
    {
      Image im(sz[0], sz[1]);  // the placed cases among light salt
      salt(im, 0.004);
      placed(im, 3);
      check(im, "placed + salt");
      planes++;
    }
  }
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok: %d planes, every word and both lists equal the definitions\n", planes);
  return 0;
}
