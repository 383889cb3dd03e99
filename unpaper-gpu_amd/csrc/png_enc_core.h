/* png_enc_core.h — the lossless PNG encoder's core, shared by the host twin
 * (png_enc.cpp) and the device kernels (kernels_png.hip) so that both produce
 * the same bytes.  What it codes is the zlib stream of a PNG IDAT chunk, which
 * is also the body of a PDF /FlateDecode image with /Predictor 15.
 *
 * Samples (PNG sense).  GRAY8 colour type 0, RGB24 type 2, Y400A type 4, all
 * depth 8; MONOBLACK type 0 depth 1 with its bits as they are, MONOWHITE the
 * same with its bits inverted on load (in PNG 1 is white).  A bilevel row's
 * pixels are bits [off, off + width) of the source row; the pad bits after the
 * last pixel are written 0 and nothing outside the range is read as a pixel.
 *
 * Filtered stream.  Row y is the bytes f[y * line .. (y + 1) * line): the
 * filter number, then row_bytes filtered bytes (line = row_bytes + 1).  Byte
 * formats take None (0), Sub (1) or Up (2), the one whose filtered bytes have
 * the least sum of |signed value|, ties to the lowest number (so row 0, where
 * Up equals None, never takes Up).  Bilevel rows take None.
 *
 * LZ77.  The stream is cut into segments of kSegBytes bytes (the last one
 * shorter).  Each is parsed greedily on its own, left to right.  At position i
 * the candidates are, in this order, the distances 1 .. bpp (bpp = bytes per
 * pixel, 1 for bilevel) and then `line` (the byte above in the stream) when
 * line <= 32768; a candidate d needs d <= i.  The match length is the count
 * of equal bytes, capped at 258 and at the segment's end (a token never
 * crosses it, so with 256-byte segments a match is at most 256 long; a match's
 * source may lie in earlier segments).  The longest
 * match wins, the first candidate among equals; below 3 the byte is a literal.
 *
 * Entropy coding.  One dynamic-Huffman block (BTYPE=10) per page over the
 * page's histograms (end-of-block counted once; when no match occurs the
 * distance symbol 0 is counted once so that one distance code exists).
 * Code lengths (build_lengths):
 *   1. the used symbols are sorted by (count, symbol number) ascending;
 *   2. a two-queue Huffman build joins the two lightest nodes; between a leaf
 *      and an internal node of equal weight the leaf is taken first, internal
 *      nodes are taken in the order they were made;
 *   3. the number of codes of each depth is taken; depths above the limit
 *      count at the limit, and while the Kraft sum exceeds 1 one code moves:
 *      a code leaves the limit, and of the longest shorter depth that has a
 *      code one code is lengthened by one bit and gets the moved code as its
 *      sibling;
 *   4. the lengths are handed out along the sorted order, the longest to the
 *      least frequent symbol.  One used symbol gets length 1.
 * The limit is 15 bits, and 7 for the code-length alphabet.  Codes are the
 * canonical ones of RFC 1951 3.2.2, kept bit-reversed for LSB-first packing.
 * The block header writes all 19 code-length-code lengths (HCLEN = 15) and
 * then every literal/length and distance length as a plain symbol 0..15; the
 * repeat codes 16/17/18 are never used.  HLIT and HDIST end at the last used
 * symbol.
 *
 * A page whose coded size would reach its stored size is written as stored
 * blocks (BTYPE=00) of 65535 bytes instead, so every page is at most
 * total + 5 * ceil(total / 65535) + 6 bytes.  zlib wrapper: 78 01, the block(s),
 * the Adler-32 of the filtered bytes (per segment sums, combined).
 */
#ifndef UNPAPER_HIP_PNG_ENC_CORE_H
#define UNPAPER_HIP_PNG_ENC_CORE_H

#include <stdint.h>

#include "unpaper_hip.h"

#ifdef __HIPCC__
#define PNG_FN __host__ __device__ static inline
#define PNG_MEMBER __host__ __device__
#else
#define PNG_FN static inline
#define PNG_MEMBER
#endif

namespace uph {
namespace pngenc {

constexpr int kSegBytes = 256;   // filtered bytes a lane parses, by measurement
constexpr int kLL = 286;         // literal/length symbols
constexpr int kDD = 30;          // distance symbols
constexpr int kSyms = kLL + kDD;
constexpr int kCL = 19;          // code-length alphabet
constexpr int kEob = 256;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kWindow = 32768;
constexpr int64_t kStoredBlock = 65535;
constexpr uint32_t kAdlerMod = 65521;

struct Shape {
  int32_t fmt, width, height;
  int32_t depth, colour_type, channels;
  int32_t bpp;        // filter and match distance of a pixel, in bytes (1 for bilevel)
  int32_t invert;     // MONOWHITE
  int64_t row_bytes;  // sample bytes a row
  int64_t line;       // row_bytes + 1
  int64_t total;      // height * line: the filtered stream
};

PNG_FN bool shape_of(int32_t fmt, int32_t width, int32_t height, Shape* s) {
  s->fmt = fmt;
  s->width = width;
  s->height = height;
  s->depth = 8;
  s->invert = 0;
  switch (fmt) {
    case UPHIP_FMT_GRAY8: s->colour_type = 0; s->channels = 1; break;
    case UPHIP_FMT_RGB24: s->colour_type = 2; s->channels = 3; break;
    case UPHIP_FMT_Y400A: s->colour_type = 4; s->channels = 2; break;
    case UPHIP_FMT_MONOWHITE: s->invert = 1;  // falls through
    case UPHIP_FMT_MONOBLACK: s->colour_type = 0; s->channels = 1; s->depth = 1; break;
    default: return false;
  }
  s->bpp = s->depth == 8 ? s->channels : 1;
  s->row_bytes = s->depth == 8 ? (int64_t)width * s->channels : ((int64_t)width + 7) / 8;
  s->line = s->row_bytes + 1;
  s->total = s->line * height;
  return true;
}

PNG_FN int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
PNG_FN int64_t segments_of(int64_t total) { return (total + kSegBytes - 1) / kSegBytes; }
PNG_FN int64_t stored_size(int64_t total) {
  return total + 5 * ((total + kStoredBlock - 1) / kStoredBlock) + 6;
}

/* Sample byte k of a row read through R (uint32_t byte(int64_t i): byte i from
 * the byte that holds the row's first pixel); `off` is the bit of byte 0 that
 * holds pixel 0 (0 for byte formats). */
template <class R>
PNG_FN uint32_t sample(const R& r, const Shape& s, int off, int64_t k) {
  if (s.depth == 8) return r.byte(k);
  const int64_t bit = (int64_t)off + 8 * k;
  const int64_t left = (int64_t)s.width - 8 * k;
  const int n = left < 8 ? (int)left : 8;
  const int64_t i = bit >> 3;
  const int sh = (int)(bit & 7);
  uint32_t v = r.byte(i) << sh;
  if (sh + n > 8) v |= r.byte(i + 1) >> (8 - sh);
  if (s.invert) v = ~v;
  return v & (0xFF00u >> n) & 0xFFu;
}

PNG_FN uint32_t filter_byte(int f, uint32_t x, uint32_t a, uint32_t b) {
  return (x - (f == 1 ? a : f == 2 ? b : 0u)) & 0xFFu;
}
PNG_FN uint32_t filter_cost(uint32_t v) { return v < 128 ? v : 256 - v; }

/* Adds to sum[0..2] the None / Sub / Up costs of sample bytes k0, k0 + step, ..
 * of a row (`up` is read only when has_up). */
template <class R>
PNG_FN void filter_sums(const R& cur, int off, const R& up, int up_off, bool has_up, const Shape& s, int64_t k0,
                        int64_t step, uint32_t sum[3]) {
  for (int64_t k = k0; k < s.row_bytes; k += step) {
    const uint32_t x = sample(cur, s, off, k);
    const uint32_t a = k >= s.bpp ? sample(cur, s, off, k - s.bpp) : 0u;
    const uint32_t b = has_up ? sample(up, s, up_off, k) : 0u;
    sum[0] += filter_cost(x);
    sum[1] += filter_cost(filter_byte(1, x, a, b));
    sum[2] += filter_cost(filter_byte(2, x, a, b));
  }
}

PNG_FN int choose_filter(const Shape& s, const uint32_t sum[3]) {
  if (s.depth != 8) return 0;
  int f = 0;
  if (sum[1] < sum[f]) f = 1;
  if (sum[2] < sum[f]) f = 2;
  return f;
}

/* Writes filtered bytes k0, k0 + step, .. of a row to dst (dst[0] is the
 * filter number's place; the caller writes it). */
template <class R>
PNG_FN void filter_row(const R& cur, int off, const R& up, int up_off, bool has_up, const Shape& s, int f, int64_t k0,
                       int64_t step, uint8_t* dst) {
  for (int64_t k = k0; k < s.row_bytes; k += step) {
    const uint32_t x = sample(cur, s, off, k);
    const uint32_t a = (f == 1 && k >= s.bpp) ? sample(cur, s, off, k - s.bpp) : 0u;
    const uint32_t b = (f == 2 && has_up) ? sample(up, s, up_off, k) : 0u;
    dst[1 + k] = (uint8_t)filter_byte(f, x, a, b);
  }
}

// ---- tokens ---------------------------------------------------------------

PNG_FN void length_symbol(int len, int* sym, int* ebits, uint32_t* eval) {
  if (len <= 10) {
    *sym = 257 + len - 3; *ebits = 0; *eval = 0;
  } else if (len == 258) {
    *sym = 285; *ebits = 0; *eval = 0;
  } else {
    const uint32_t l = (uint32_t)(len - 3);
    const int e = 31 - __builtin_clz(l) - 2;
    *sym = 261 + 4 * e + (int)((l >> e) & 3);
    *ebits = e;
    *eval = l & ((1u << e) - 1);
  }
}

PNG_FN void distance_symbol(int dist, int* sym, int* ebits, uint32_t* eval) {
  const uint32_t x = (uint32_t)(dist - 1);
  if (x < 4) {
    *sym = (int)x; *ebits = 0; *eval = 0;
  } else {
    const int nb = 31 - __builtin_clz(x);
    *sym = 2 * nb + (int)((x >> (nb - 1)) & 1);
    *ebits = nb - 1;
    *eval = x & ((1u << (nb - 1)) - 1);
  }
}

PNG_FN int match_length(const uint8_t* f, int64_t i, int64_t d, int cap) {
  int n = 0;
  while (n < cap && f[i + n] == f[i + n - d]) n++;
  return n;
}

/* The greedy parse of stream bytes [begin, end) (one segment).  V has
 * literal(uint32_t byte) and match(int len, int dist). */
template <class V>
PNG_FN void parse_segment(const uint8_t* f, int64_t begin, int64_t end, const Shape& s, V& v) {
  const bool above = s.line <= kWindow;
  int64_t i = begin;
  while (i < end) {
    const int cap = end - i < kMaxMatch ? (int)(end - i) : kMaxMatch;
    int best = 0, dist = 0;
    if (cap >= kMinMatch) {
      for (int d = 1; d <= s.bpp && best < cap; d++) {
        if (d > i) break;
        const int n = match_length(f, i, d, cap);
        if (n > best) { best = n; dist = d; }
      }
      if (above && s.line <= i && best < cap) {
        const int n = match_length(f, i, s.line, cap);
        if (n > best) { best = n; dist = (int)s.line; }
      }
    }
    if (best >= kMinMatch) {
      v.match(best, dist);
      i += best;
    } else {
      v.literal(f[i]);
      i++;
    }
  }
}

/* Adler-32 sums of n bytes on their own: a = sum of the bytes, b = sum of
 * (n - k) * byte k, both mod 65521 (n <= kSegBytes keeps them in 32 bits). */
PNG_FN void adler_segment(const uint8_t* p, int n, uint32_t* a, uint32_t* b) {
  uint32_t sa = 0, sb = 0;
  for (int k = 0; k < n; k++) {
    sa += p[k];
    sb += sa;
  }
  *a = sa % kAdlerMod;
  *b = sb % kAdlerMod;
}
/* (A, B) after n more bytes whose own sums are (a, b): adler32_combine. */
PNG_FN void adler_append(uint32_t* A, uint32_t* B, uint64_t n, uint32_t a, uint32_t b) {
  *B = (uint32_t)((*B + (n % kAdlerMod) * *A + b) % kAdlerMod);
  *A = (*A + a) % kAdlerMod;
}

// ---- code tables ----------------------------------------------------------

/* How many used symbols sort before symbol s by (count, number): its place in
 * the sorted order (s itself must be used). */
PNG_FN int sorted_place(const uint32_t* freq, int n, int s) {
  int r = 0;
  const uint32_t fs = freq[s];
  for (int t = 0; t < n; t++) {
    const uint32_t ft = freq[t];
    if (ft && (ft < fs || (ft == fs && t < s))) r++;
  }
  return r;
}

/* Code lengths of the m used symbols, order[0..m) sorted ascending (the
 * file's head, steps 2-4).  len[0..n) is written; w needs 2 * m entries. */
PNG_FN void build_lengths(const uint32_t* freq, int n, const uint16_t* order, int m, int maxbits, uint8_t* len,
                          uint32_t* w) {
  for (int i = 0; i < n; i++) len[i] = 0;
  if (m == 0) return;
  if (m == 1) {
    len[order[0]] = 1;
    return;
  }
  // w[0..m): leaves; w[m..2m-1): internal nodes in the order made.  Once a
  // node has been joined its w becomes its parent's index.
  for (int i = 0; i < m; i++) w[i] = freq[order[i]];
  int leaf = 0, inner = m, made = m;
  for (; made < 2 * m - 1; made++) {
    uint32_t sum = 0;
    for (int k = 0; k < 2; k++) {
      int pick;
      if (leaf < m && (inner >= made || w[leaf] <= w[inner]))
        pick = leaf++;
      else
        pick = inner++;
      sum += w[pick];
      w[pick] = (uint32_t)made;
    }
    w[made] = sum;
  }
  // depths from the root down (a parent's index is above its children's)
  int count[32];
  for (int i = 0; i < 32; i++) count[i] = 0;
  w[2 * m - 2] = 0;
  for (int i = 2 * m - 3; i >= 0; i--) {
    w[i] = w[w[i]] + 1;
    if (i < m) count[w[i] < (uint32_t)maxbits ? w[i] : (uint32_t)maxbits]++;
  }
  uint32_t kraft = 0;
  for (int l = 1; l <= maxbits; l++) kraft += (uint32_t)count[l] << (maxbits - l);
  while (kraft > (1u << maxbits)) {
    count[maxbits]--;
    for (int l = maxbits - 1; l > 0; l--)
      if (count[l]) {
        count[l]--;
        count[l + 1] += 2;
        break;
      }
    kraft--;
  }
  int at = 0;
  for (int l = maxbits; l > 0; l--)
    for (int c = count[l]; c > 0; c--) len[order[at++]] = (uint8_t)l;
}

PNG_FN uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

/* Canonical codes of len[0..n): code[s] = reversed code | length << 16. */
PNG_FN void canonical_codes(const uint8_t* len, int n, uint32_t* code) {
  uint32_t count[16], next[16];
  for (int i = 0; i < 16; i++) count[i] = 0;
  for (int i = 0; i < n; i++) count[len[i]]++;
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int l = 1; l < 16; l++) {
    c = (c + count[l - 1]) << 1;
    next[l] = c;
  }
  for (int i = 0; i < n; i++) {
    const int l = len[i];
    code[i] = l ? (reverse_bits(next[l]++, l) | (uint32_t)l << 16) : 0u;
  }
}

/* A page's counts and codes: the hand-off between the passes. */
struct PageTab {
  uint32_t freq[kSyms];   // literal/length then distance counts
  uint32_t code[kSyms];   // reversed code | length << 16
  uint32_t clcode[kCL];   // the code-length alphabet's codes, the same form
  int32_t hlit, hdist;    // lengths sent: hlit literal/length, hdist distance
  int32_t head_bits;      // block header: BFINAL, BTYPE and the tables
  int32_t stored;         // the page goes out as stored blocks
  uint32_t adler;
  int32_t pad;
  int64_t token_bits;     // all segments' tokens
  int64_t size;           // the zlib stream's bytes
};

/* The block header into sink S (put(uint32_t bits, int n), LSB first). */
template <class S>
PNG_FN void put_block_header(const PageTab& t, S& s) {
  constexpr int order[kCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  s.put(1, 1);  // BFINAL
  s.put(2, 2);  // BTYPE = 10
  s.put((uint32_t)(t.hlit - 257), 5);
  s.put((uint32_t)(t.hdist - 1), 5);
  s.put(kCL - 4, 4);
  for (int i = 0; i < kCL; i++) s.put(t.clcode[order[i]] >> 16, 3);
  for (int i = 0; i < t.hlit; i++) {
    const uint32_t c = t.clcode[t.code[i] >> 16];
    s.put(c & 0xFFFFu, (int)(c >> 16));
  }
  for (int i = 0; i < t.hdist; i++) {
    const uint32_t c = t.clcode[t.code[kLL + i] >> 16];
    s.put(c & 0xFFFFu, (int)(c >> 16));
  }
}

struct CountSink {
  int64_t bits = 0;
  PNG_MEMBER void put(uint32_t, int n) { bits += n; }
};

/* Parse visitor that codes the tokens into sink S with the codes of `code`. */
template <class S>
struct CodeTokens {
  const uint32_t* code;
  S& s;
  PNG_MEMBER CodeTokens(const uint32_t* c, S& sink) : code(c), s(sink) {}
  PNG_MEMBER void literal(uint32_t b) {
    const uint32_t c = code[b];
    s.put(c & 0xFFFFu, (int)(c >> 16));
  }
  PNG_MEMBER void match(int len, int dist) {
    int sym, eb;
    uint32_t ev;
    length_symbol(len, &sym, &eb, &ev);
    uint32_t c = code[sym];
    s.put((c & 0xFFFFu) | ev << (c >> 16), (int)(c >> 16) + eb);
    distance_symbol(dist, &sym, &eb, &ev);
    c = code[kLL + sym];
    s.put((c & 0xFFFFu) | ev << (c >> 16), (int)(c >> 16) + eb);
  }
};

/* Lane 0's part of the table kernel and the host's: from the page's counts
 * (end-of-block and the lone distance symbol already counted) and the sorted
 * orders to the codes and the header's size.  w needs 2 * kLL entries. */
PNG_FN void build_tables(PageTab* t, const uint16_t* ll_order, int ll_used, const uint16_t* dd_order, int dd_used,
                         uint32_t* w) {
  uint8_t len[kLL];
  build_lengths(t->freq, kLL, ll_order, ll_used, 15, len, w);
  canonical_codes(len, kLL, t->code);
  int hlit = kLL;
  while (hlit > 257 && !len[hlit - 1]) hlit--;
  uint8_t dlen[kDD + 2];
  build_lengths(t->freq + kLL, kDD, dd_order, dd_used, 15, dlen, w);
  canonical_codes(dlen, kDD, t->code + kLL);
  int hdist = kDD;
  while (hdist > 1 && !dlen[hdist - 1]) hdist--;
  t->hlit = hlit;
  t->hdist = hdist;
  // the code-length alphabet over the lengths sent
  uint32_t cf[kCL];
  for (int i = 0; i < kCL; i++) cf[i] = 0;
  for (int i = 0; i < hlit; i++) cf[len[i]]++;
  for (int i = 0; i < hdist; i++) cf[dlen[i]]++;
  uint16_t co[kCL];
  int cu = 0;
  for (int i = 0; i < kCL; i++)
    if (cf[i]) co[sorted_place(cf, kCL, i)] = (uint16_t)i, cu++;
  uint8_t cl[kCL];
  build_lengths(cf, kCL, co, cu, 7, cl, w);
  canonical_codes(cl, kCL, t->clcode);
  CountSink cs;
  put_block_header(*t, cs);
  t->head_bits = (int32_t)cs.bits;
}

/* The stream's size and form once token_bits is known. */
PNG_FN void decide_size(PageTab* t, int64_t total) {
  const int eob = (int)(t->code[kEob] >> 16);
  const int64_t coded = 2 + ((int64_t)t->head_bits + t->token_bits + eob + 7) / 8 + 4;
  const int64_t stored = stored_size(total);
  t->stored = coded >= stored;
  t->size = t->stored ? stored : coded;
}

/* Where byte i of the filtered stream lies in a stored stream. */
PNG_FN int64_t stored_place(int64_t i) { return 2 + 5 * (i / kStoredBlock + 1) + i; }
/* The 5 header bytes of the stored block that starts at filtered byte i. */
PNG_FN void stored_header(int64_t i, int64_t total, uint8_t h[5]) {
  const int64_t n = total - i < kStoredBlock ? total - i : kStoredBlock;
  h[0] = i + n >= total ? 1 : 0;
  h[1] = (uint8_t)(n & 255);
  h[2] = (uint8_t)(n >> 8);
  h[3] = (uint8_t)(~n & 255);
  h[4] = (uint8_t)((~n >> 8) & 255);
}

}  // namespace pngenc
}  // namespace uph

#endif
