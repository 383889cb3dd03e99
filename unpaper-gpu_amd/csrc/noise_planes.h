/* noise_planes.h — the noisefilter's GRAY8 classification as operators on the
 * dark bit-plane (kernels_noise.hip: k_noise_cand, k_noise_verdict), in one
 * place.
 *
 * The plane is k_noise_bits's: bit b of word w of row y is (pixel 32 w + b <
 * white), nwr = ceil(W / 32) words a row, rows packed nwr words apart with no
 * padding, columns >= W zero.  Every operator here reads the true plane
 * through np_word, which answers 0 for a row outside [0, H) and for a word
 * index outside [0, nwr) (never the neighbouring row's word), so a pixel
 * outside the image is not dark and no operator has an edge case of its own.
 *
 *   l3     dark with >= 5 dark pixels in its 3x3 block: all 8-adjacent to the
 *          centre, so one component of >= 5 pixels
 *   cand   dark & ~(l3 | 8-dilation of l3): a pixel 8-adjacent to an l3 pixel
 *          is in that component; only the rest need a flood
 *   small  candidates whose 8-connected dark component has <= 4 pixels
 *          (np_flood9; a pixel of such a component has < 5 dark pixels in its
 *          3x3 block and no l3 neighbour, so the candidates hold all of them)
 *   zone   what the sequential replay takes unjudged: dark pixels with x < 32
 *          or y < 32, without the l3 ones at x >= 8, y >= 7 (or, all_seq,
 *          every dark pixel)
 *   verdict  of a small pixel at x >= 32, y >= 32 (np_verdict)
 *
 * Plain C++ with no HIP dependency, so a host program can check every word
 * against a per-pixel brute force of these definitions
 * (tests/test_noise_planes_cpu.py).
 */
#ifndef UNPAPER_HIP_NOISE_PLANES_H
#define UNPAPER_HIP_NOISE_PLANES_H

#include <stdint.h>

#ifdef __HIPCC__
#define NP_FN __host__ __device__ static inline
#else
#define NP_FN static inline
#endif

enum {
  kNpZone = 32,     /* sequential edge zone (x or y < 32) */
  kNpEligible = 40, /* parallel verdicts only for components at >= 40 */
  kNpSmallMax = 4   /* a small component's pixels (the parallel path's N <= 4) */
};

typedef struct NpPlane {
  const uint32_t* w;
  int32_t nwr, H;
} NpPlane;

NP_FN int np_popc(uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}
NP_FN int np_ctz(uint32_t v) { /* v != 0 */
#ifdef __HIP_DEVICE_COMPILE__
  return __ffs((int)v) - 1;
#else
  return __builtin_ctz(v);
#endif
}

/* The load is unconditional, from the clamped position, and masked after: a
 * caller's loads (a strip's rows, a flood's box) are then all in flight
 * together instead of one round trip per bounds test. */
NP_FN uint32_t np_word(const NpPlane P, int32_t wi, int32_t y) {
  const int32_t cw = wi < 0 ? 0 : wi >= P.nwr ? P.nwr - 1 : wi;
  const int32_t cy = y < 0 ? 0 : y >= P.H ? P.H - 1 : y;
  const uint32_t v = P.w[(int64_t)cy * P.nwr + cw];
  return ((cw == wi) & (cy == y)) ? v : 0u;
}

/* bits [x, x + n) of row y (1 <= n <= 32; x may be negative or past the row) */
NP_FN uint32_t np_bits(const NpPlane P, int32_t x, int32_t y, int n) {
  const int32_t wi = x >> 5; /* floor (arithmetic shift) */
  const int off = x & 31;
  const uint64_t v = np_word(P, wi, y) | ((uint64_t)np_word(P, wi + 1, y) << 32);
  return (uint32_t)(v >> off) & (n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u));
}

/* ---- the streaming operators, a word at a time ---------------------------
 * A row of word column wi is its word v with the words left and right of it.
 * The 3-sums of the word's 32 columns take the neighbours' adjoining bits;
 * the dilation of l3 into the word's end columns takes l3 of the two columns
 * next to the word (31 of the left word, 0 of the right one), which are
 * counted on their own from the three columns around each (eL, eR). */
typedef struct NpRow {
  uint32_t v, s0, s1; /* the word; (s1 s0) = pixel + left + right, bit-sliced */
  uint32_t hl, hr;    /* dark pixels of columns -2..0 and 31..33 of the word */
  uint32_t dl, dr;    /* columns -1 and 32 themselves */
} NpRow;
NP_FN NpRow np_row(const NpPlane P, int32_t wi, int32_t y) {
  const uint32_t l = np_word(P, wi - 1, y), v = np_word(P, wi, y), r = np_word(P, wi + 1, y);
  const uint32_t L = (v << 1) | (l >> 31), R = (v >> 1) | (r << 31); /* left of column x: bit x - 1 */
  NpRow o;
  o.v = v;
  o.s0 = v ^ L ^ R;
  o.s1 = (v & L) | (v & R) | (L & R);
  o.hl = (uint32_t)np_popc((l >> 30) | ((v & 1u) << 2));
  o.hr = (uint32_t)np_popc((v >> 31) | ((r & 3u) << 1));
  o.dl = l >> 31;
  o.dr = r & 1u;
  return o;
}

/* l3 of row b from the sums of rows a (above), b, c (below): the word's, and
 * in bits 0 / 1 of *edge those of columns -1 / 32 */
NP_FN uint32_t np_l3(const NpRow a, const NpRow b, const NpRow c, uint32_t* edge) {
  const uint32_t t0 = a.s0 ^ b.s0 ^ c.s0;                              /* weight 1 */
  const uint32_t k0 = (a.s0 & b.s0) | (a.s0 & c.s0) | (b.s0 & c.s0);   /* carry into 2 */
  const uint32_t x = a.s1 ^ b.s1 ^ c.s1;
  const uint32_t m = (a.s1 & b.s1) | (a.s1 & c.s1) | (b.s1 & c.s1);    /* weight 4 */
  const uint32_t u1 = x ^ k0, k1 = x & k0;                             /* weight 2, carry into 4 */
  const uint32_t u2 = m ^ k1, u3 = m & k1;                             /* weights 4, 8 */
  *edge = (b.dl & (uint32_t)(a.hl + b.hl + c.hl >= 5u)) |
          ((b.dr & (uint32_t)(a.hr + b.hr + c.hr >= 5u)) << 1);
  return b.v & (u3 | (u2 & (u1 | t0)));                                /* count >= 5 */
}

/* the candidates of the word v from the l3 words and edges of the rows above,
 * of and below it */
NP_FN uint32_t np_cand(uint32_t v, uint32_t la, uint32_t lb, uint32_t lc, uint32_t ea,
                       uint32_t eb, uint32_t ec) {
  const uint32_t o = la | lb | lc, e = ea | eb | ec;
  return v & ~(o | (o << 1) | (o >> 1) | (e & 1u) | ((e >> 1) << 31));
}

/* the zone pixels of word wi of row y (dark, l3: the word's bits) */
NP_FN uint32_t np_zone(uint32_t dark, uint32_t l3, int32_t wi, int32_t y, int all_seq) {
  if (all_seq) return dark;
  const uint32_t in = y < kNpZone || wi == 0 ? 0xFFFFFFFFu : 0u;
  const uint32_t noop = y >= 7 ? (wi == 0 ? 0xFFFFFF00u : 0xFFFFFFFFu) : 0u; /* x >= 8 */
  return dark & in & ~(l3 & noop);
}

/* R consecutive rows y0 .. y0 + R - 1 of word column wi, sliding: each row's
 * sums are formed once.  Any of the outputs may be dropped by the caller
 * (fully unrolled, so unused ones cost nothing). */
template <int R>
NP_FN void np_strip(const NpPlane P, int32_t wi, int32_t y0, int all_seq, uint32_t* l3w,
                    uint32_t* candw, uint32_t* zonew) {
  NpRow ra = np_row(P, wi, y0 - 2), rb = np_row(P, wi, y0 - 1), rc = np_row(P, wi, y0);
  uint32_t ea, eb, ec;
  uint32_t la = np_l3(ra, rb, rc, &ea); /* row y0 - 1 */
  ra = rb;
  rb = rc;
  rc = np_row(P, wi, y0 + 1);
  uint32_t lb = np_l3(ra, rb, rc, &eb); /* row y0 */
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < R; r++) {
    /* after the shift ra, rb, rc: rows y0 + r, + 1, + 2; la, lb: l3 of rows
     * y0 + r - 1, y0 + r */
    ra = rb;
    rb = rc;
    rc = np_row(P, wi, y0 + r + 2);
    const uint32_t lc = np_l3(ra, rb, rc, &ec); /* row y0 + r + 1 */
    l3w[r] = lb;
    candw[r] = np_cand(ra.v, la, lb, lc, ea, eb, ec);
    zonew[r] = np_zone(ra.v, lb, wi, y0 + r, all_seq);
    la = lb;
    lb = lc;
    ea = eb;
    eb = ec;
  }
}

/* ---- the sparse operators -------------------------------------------------
 * Dark component of (x, y) restricted to its 9x9 box; returns its pixel count
 * (growth capped after 4 dilations) and the mask rows (bit i of comp[r]:
 * pixel (x - 4 + i, y - 4 + r)).  Every dilation step only adds pixels
 * connected to the centre and a step that adds none ends the search, so four
 * steps reach either the whole component (<= 4 pixels, all within 3 of the
 * centre) or more than 4 pixels.  D: the box's dark rows, same layout. */
NP_FN int np_flood9(const NpPlane P, int32_t x, int32_t y, uint32_t* comp, uint32_t* D) {
  uint32_t cur[9];
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 9; r++) {
    D[r] = np_bits(P, x - 4, y - 4 + r, 9);
    cur[r] = 0;
  }
  cur[4] = 1u << 4;
  int n = 1;
  for (int it = 0; it < 4; it++) {
    uint32_t nx[9];
    int same = 1;
    n = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 9; r++) {
      uint32_t u = cur[r] | (r > 0 ? cur[r - 1] : 0) | (r < 8 ? cur[r + 1] : 0);
      u = (u | (u << 1) | (u >> 1)) & D[r];
      nx[r] = u;
      same &= (u == cur[r]);
      n += np_popc(u);
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 9; r++) cur[r] = nx[r];
    if (n > kNpSmallMax || same) break;
  }
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 9; r++) comp[r] = cur[r];
  return n;
}

/* The reference's ring test of the pixel at the centre of the 9x9 dark box D
 * for intensity N <= 4 (noisefilter_count_pixel_neighbors, filters.c:256-300):
 * count 1, then each level's ring until an empty one or past N. */
NP_FN int np_ring_test(const uint32_t* D, int N) {
  int count = 1, go = 1;
#if defined(__clang__)
#pragma unroll
#endif
  for (int L = 1; L <= 4; L++) {
    if (!go || L > N) break;
    const uint32_t span = ((1u << (2 * L + 1)) - 1u) << (4 - L);
    const uint32_t ends = (1u << (4 - L)) | (1u << (4 + L));
    int lc = np_popc(D[4 - L] & span) + np_popc(D[4 + L] & span);
    for (int r = 4 - L + 1; r <= 4 + L - 1; r++) lc += np_popc(D[r] & ends);
    count += lc;
    go = lc != 0;
  }
  return count <= N;
}

enum { NP_NONE = 0, NP_SEQ = 1, NP_CLEAR = 2 };

/* The verdict of the small pixel (x, y), x >= 32 and y >= 32, for intensity
 * N <= 4: NP_SEQ (the sequential replay decides), NP_CLEAR (cleared in
 * parallel) or NP_NONE (stays).  Its component C (<= 4 pixels) is eligible for
 * the parallel verdict when it lies at >= 40 from the left and the top and no
 * foreign small pixel is within Chebyshev 7 of it, checked on C's bounding
 * box dilated by 7: a superset, so a component rejected here merely takes the
 * exact sequential path.  An eligible component is cleared iff one of its
 * pixels passes the ring test on the original image (filters.c:256-300;
 * nothing that test reads ever changes, and at >= 40 the reference's unsigned
 * ring-loop skips never apply).  On GRAY8 every dark pixel is a trigger. */
NP_FN int np_verdict(const NpPlane dark, const NpPlane small, int32_t x, int32_t y, int N) {
  uint32_t comp[9], D[9];
  if (np_flood9(dark, x, y, comp, D) > kNpSmallMax) return NP_SEQ; /* not small: never asked */
  int by0 = 4, by1 = -4, nc = 0; /* bounding box, offsets from (x, y) */
  uint32_t any = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 9; r++) {
    if (comp[r]) {
      if (by0 > r - 4) by0 = r - 4;
      by1 = r - 4;
      any |= comp[r];
      nc += np_popc(comp[r]);
    }
  }
  const int bx0 = np_ctz(any) - 4, bx1 = 27 - (int)__builtin_clz(any);
  if (x + bx0 < kNpEligible || y + by0 < kNpEligible) return NP_SEQ;
  {
    const int32_t X0 = x + bx0 - 7;
    const int n = bx1 - bx0 + 15; /* <= 18 */
    const int32_t r0 = y + by0 - 7, r1 = y + by1 + 7; /* at most 4 + 14 rows */
    int cnt = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < 18; j++) {
      const int c = np_popc(np_bits(small, X0, r0 + j, n));
      cnt += r0 + j <= r1 ? c : 0;
    }
    if (cnt != nc) return NP_SEQ;
  }
  /* the centre's box is the flood's; another pixel's box is read */
  if (np_ring_test(D, N)) return NP_CLEAR;
  comp[4] &= ~(1u << 4);
  for (int cr = 1; cr < 8; cr++) { /* a small component lies within 3 of the centre */
    uint32_t m = comp[cr];
    while (m) {
      const int cb = np_ctz(m);
      m &= m - 1;
      const int32_t cx = x + cb - 4, cy = y + cr - 4;
#if defined(__clang__)
#pragma unroll
#endif
      for (int r = 0; r < 9; r++) D[r] = np_bits(dark, cx - 4, cy - 4 + r, 9);
      if (np_ring_test(D, N)) return NP_CLEAR;
    }
  }
  return NP_NONE;
}

#endif /* UNPAPER_HIP_NOISE_PLANES_H */
