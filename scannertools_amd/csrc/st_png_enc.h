// ImageEncoder, PNG: what the kernels (st_png_enc.hip) and their CPU twin (st_png_enc_host.cpp) share, so that the two cannot
// drift: the filters, the token of a position inside a run, the length symbols, the length-limited code construction and the
// block header.  DESIGN.md 4.18; tests/ref_png_encode_np.py restates all of it independently.
#ifndef ST_PNG_ENC_H_
#define ST_PNG_ENC_H_

#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define ST_PNG_HD __host__ __device__ inline
#else
#define ST_PNG_HD inline
#endif

constexpr int kPngPiece = 32768;         // filtered bytes per deflate block and IDAT chunk
constexpr int kPngLitLen = 286;          // literal/length symbols
constexpr int kPngClSyms = 19;           // code-length symbols (16, 17 and 18 are never used)
constexpr int kPngHeadBytes = 33;        // signature and IHDR
constexpr int kPngTailBytes = 21 + 12;   // the IDAT with the final empty block and the Adler-32; IEND
constexpr int kPngChunkMax = 12 + 2 + 5 + kPngPiece;   // a piece's IDAT chunk: length, type, CRC; zlib header; stored header
constexpr unsigned kAdlerMod = 65521u;

struct StPngEncGeom {
  int h, w, c, rb;         // rb: bytes of a row without its filter-type byte
  size_t fb;               // filtered bytes of a frame: h * (1 + rb)
  size_t stride;           // fb rounded up to 16: the frames' distance in the call's filtered buffer
  int pieces;              // ceil(fb / 32768)
};
ST_PNG_HD void st_png_enc_geom(int h, int w, int c, StPngEncGeom* g) {
  g->h = h; g->w = w; g->c = c; g->rb = w * c;
  g->fb = (size_t)h * (size_t)(1 + g->rb);
  g->stride = (g->fb + 15) / 16 * 16;
  g->pieces = (int)((g->fb + kPngPiece - 1) / kPngPiece);
}
ST_PNG_HD int st_png_piece_len(size_t fb, int p) {
  const size_t at = (size_t)p * kPngPiece;
  return fb - at < (size_t)kPngPiece ? (int)(fb - at) : kPngPiece;
}

// One filtered byte.  x: the byte; a: left, b: above, c: above left (0 outside the picture).
ST_PNG_HD int st_png_paeth(int a, int b, int c) {
  int pa = b - c, pb = a - c, pc = a + b - 2 * c;
  pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
ST_PNG_HD unsigned st_png_filter_byte(int ft, int x, int a, int b, int c) {
  const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : ft == 4 ? st_png_paeth(a, b, c) : 0;
  return (unsigned)(x - pred) & 0xffu;
}
ST_PNG_HD unsigned st_png_filter_cost(unsigned v) { return v < 128u ? v : 256u - v; }   // min(b, 256 - b)

// The token that begins k bytes into a maximal run of R equal bytes: 0 none, 1 a literal, else a match of that length at
// distance 1.  The run is its first byte as a literal, (R - 1) / 258 matches of 258, and the remainder as one match when it
// has three bytes or more, as literals otherwise.
ST_PNG_HD int st_png_token(int k, int R) {
  if (k == 0) return 1;
  const int j = k - 1, T = R - 1;
  const int whole = T / 258 * 258, r = T - whole;
  if (j < whole) return j % 258 == 0 ? 258 : 0;
  if (r >= 3) return j == whole ? r : 0;
  return 1;
}

// length 3 .. 258 -> its symbol 257 .. 285, the number of extra bits and their value
ST_PNG_HD int st_png_len_symbol(int len, int* nbits, int* extra) {
  if (len == 258) { *nbits = 0; *extra = 0; return 285; }
  const int l = len - 3;
  if (l < 8) { *nbits = 0; *extra = 0; return 257 + l; }
  int e = 1;
  while ((l >> (e + 3)) != 0) ++e;   // 8..15 -> 1, 16..31 -> 2, .. 128..254 -> 5
  *nbits = e;
  *extra = l & ((1 << e) - 1);
  return 257 + 4 * e + 4 + ((l >> e) & 3);
}

// ---- length-limited prefix codes ------------------------------------------------------------------------------------------
// The symbols with a count, or dummies (the lowest-numbered symbols without one, weight 1) so that there are two: in `order`,
// by (weight, symbol) ascending.  Serial; the kernel ranks the 286 literal/length symbols with all its threads instead, which
// gives the same order because the key is a total order.
struct StPngHuffWork {
  uint32_t weight[2 * kPngLitLen];   // leaves in `order`'s order, then the merged nodes as they are made
  uint16_t parent[2 * kPngLitLen];
  uint16_t depth[2 * kPngLitLen];
  uint16_t order[kPngLitLen];
  uint16_t count[kPngLitLen + 2];    // codes per length
};

ST_PNG_HD uint32_t st_png_huff_weight(const uint32_t* freq, int s, int nused) {
  // with fewer than two counted symbols the lowest-numbered others stand in with weight 1
  if (freq[s]) return freq[s];
  if (nused >= 2) return 0;
  int need = 2 - nused;   // dummies: the first `need` symbols without a count
  for (int i = 0; i < s; ++i)
    if (!freq[i]) --need;
  return need > 0 ? 1u : 0u;
}

ST_PNG_HD int st_png_huff_order(const uint32_t* freq, int nsym, StPngHuffWork* wk) {
  uint16_t* order = wk->order;
  int nused = 0, m = 0;
  for (int i = 0; i < nsym; ++i) nused += freq[i] != 0;
  for (int i = 0; i < nsym; ++i) {
    const uint32_t wi = st_png_huff_weight(freq, i, nused);
    if (!wi) continue;
    int at = m++;   // insertion: (weight, symbol) ascending; symbols arrive ascending, so ties stay behind their equals
    while (at > 0 && st_png_huff_weight(freq, order[at - 1], nused) > wi) {
      order[at] = order[at - 1];
      --at;
    }
    order[at] = (uint16_t)i;
  }
  for (int k = 0; k < m; ++k) wk->weight[k] = st_png_huff_weight(freq, order[k], nused);
  return m;
}

// The code lengths of the m >= 2 symbols in wk->order (weights in wk->weight[0 .. m), ascending): Huffman's algorithm on two
// queues -- the leaves in order and the merged nodes in the order they were made; of two equal weights the leaf goes first --,
// the number of codes per depth, depths beyond `limit` folded back the way libjpeg's jpeg_gen_optimal_table does it (a pair
// of the deepest codes moves up one level beside a code from the deepest level above that has room, which moves down), and the
// lengths dealt out again by weight: the longest to the first symbols of the order.  Kraft's sum stays exactly 1 throughout.
// len[] is written for all nsym symbols (0: no code).  2^limit >= m is the caller's to ensure.
// The four steps are functions of their own because the kernel runs the second, the fourth and the codes with all its threads.
// 1. the merges; returns the number of nodes (the root is the last).  The two queue heads' weights stay in locals.
ST_PNG_HD int st_png_huff_merge(StPngHuffWork* wk, int m) {
  uint32_t* W = wk->weight;
  int leaf = 0, node = m, made = m;   // next leaf, next unmerged node, next node to make
  uint32_t wl = W[0], wn = 0;         // their weights, where they exist
  for (int step = 0; step < m - 1; ++step) {
    uint32_t sum = 0;
    for (int q = 0; q < 2; ++q) {
      int pick;
      if (leaf < m && (node >= made || wl <= wn)) {
        pick = leaf++;
        sum += wl;
        if (leaf < m) wl = W[leaf];
      } else {
        pick = node++;
        sum += wn;
        if (node < made) wn = W[node];
      }
      wk->parent[pick] = (uint16_t)made;
    }
    W[made] = sum;
    if (node == made) wn = sum;   // the queue of merged nodes was empty: this is its head
    ++made;
  }
  return made;
}
// 2. the number of codes per depth, serially from the root down; returns the deepest
ST_PNG_HD int st_png_huff_depths(StPngHuffWork* wk, int m, int made) {
  for (int i = 0; i <= m; ++i) wk->count[i] = 0;
  int deepest = 0;
  wk->depth[made - 1] = 0;
  for (int i = made - 2; i >= 0; --i) {
    const int d = wk->depth[wk->parent[i]] + 1;
    wk->depth[i] = (uint16_t)d;
    if (i < m) {
      wk->count[d]++;
      deepest = d > deepest ? d : deepest;
    }
  }
  return deepest;
}
// 3. depths beyond the limit folded back; returns the longest length left
ST_PNG_HD int st_png_huff_fold(StPngHuffWork* wk, int deepest, int limit) {
  for (int i = deepest; i > limit; --i)
    while (wk->count[i] > 0) {
      int j = i - 2;
      while (j > 0 && wk->count[j] == 0) --j;
      wk->count[i] -= 2;
      wk->count[i - 1] += 1;
      wk->count[j + 1] += 2;
      wk->count[j] -= 1;
    }
  return deepest < limit ? deepest : limit;
}
// 4. the length of the k-th symbol of the order: the longest lengths go to the first
ST_PNG_HD int st_png_huff_deal(const StPngHuffWork* wk, int top, int k) {
  int L = top;
  while (L > 1 && k >= (int)wk->count[L]) k -= (int)wk->count[L--];
  return L;
}
ST_PNG_HD void st_png_huff_lengths(StPngHuffWork* wk, int m, int nsym, int limit, uint8_t* len) {
  const int made = st_png_huff_merge(wk, m);
  const int top = st_png_huff_fold(wk, st_png_huff_depths(wk, m, made), limit);
  for (int i = 0; i < nsym; ++i) len[i] = 0;
  for (int k = 0; k < m; ++k) len[wk->order[k]] = (uint8_t)st_png_huff_deal(wk, top, k);
}

// canonical codes (RFC 1951 3.2.2), bit-reversed so that they go into an LSB-first buffer as they are: the first code of
// every length from the number of codes per length (count[1 .. limit]), a symbol's code that plus the number of lower-numbered
// symbols of its length
ST_PNG_HD void st_png_huff_first(const uint16_t* count, int limit, uint32_t* first) {
  unsigned c = 0;
  first[0] = 0;
  for (int b = 1; b <= limit; ++b) {
    c = (c + (b > 1 ? count[b - 1] : 0u)) << 1;
    first[b] = c;
  }
}
ST_PNG_HD unsigned st_png_rev(unsigned v, int L) {
  unsigned r = 0;
  for (int b = 0; b < L; ++b) r |= ((v >> b) & 1u) << (L - 1 - b);
  return r;
}
ST_PNG_HD void st_png_huff_codes(const uint8_t* len, int nsym, int limit, uint16_t* code) {
  uint32_t next[17];
  uint16_t cnt[17];
  for (int i = 0; i <= limit; ++i) cnt[i] = 0;
  for (int i = 0; i < nsym; ++i) cnt[len[i]]++;
  st_png_huff_first(cnt, limit, next);
  for (int i = 0; i < nsym; ++i) {
    const int L = len[i];
    code[i] = (uint16_t)(L ? st_png_rev(next[L]++, L) : 0u);
  }
}

// ---- a piece's dynamic block ----------------------------------------------------------------------------------------------
struct StPngBlockTables {
  uint8_t len[kPngLitLen + 2];     // literal/length code lengths
  uint16_t code[kPngLitLen + 2];   // bit-reversed
  uint8_t cl_len[kPngClSyms + 1];
  uint16_t cl_code[kPngClSyms + 1];
  int hlit, hclen;                 // literal/length lengths sent (257 ..), code-length lengths sent (4 .. 19)
  uint32_t header_bits;            // BFINAL .. the last code length
};

ST_PNG_HD int st_png_cl_order(int i) {   // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
  return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1);
}

// The tables of a piece from its symbol counts (freq[256], the end of the block, counted in).  wk->order / wk->weight hold
// the m counted literal/length symbols already (st_png_huff_order, or the kernel's ranking).  The code-length sequence is
// the hlit literal/length lengths and the one distance length as they are: trailing unused length symbols are not sent,
// runs are not folded into the symbols 16, 17 and 18.
// the code-length code from the counts of the lengths sent (clf[19]: the hlit literal/length lengths and the distance length)
ST_PNG_HD void st_png_block_cl(StPngHuffWork* wk, const uint32_t* clf, int hlit, StPngBlockTables* t) {
  const int m2 = st_png_huff_order(clf, kPngClSyms, wk);
  st_png_huff_lengths(wk, m2, kPngClSyms, 7, t->cl_len);
  st_png_huff_codes(t->cl_len, kPngClSyms, 7, t->cl_code);
  int hclen = kPngClSyms;
  while (hclen > 4 && !t->cl_len[st_png_cl_order(hclen - 1)]) --hclen;
  t->hlit = hlit;
  t->hclen = hclen;
}
ST_PNG_HD void st_png_block_tables(StPngHuffWork* wk, int m, StPngBlockTables* t) {
  st_png_huff_lengths(wk, m, kPngLitLen, 15, t->len);
  st_png_huff_codes(t->len, kPngLitLen, 15, t->code);
  int hlit = kPngLitLen;
  while (hlit > 257 && !t->len[hlit - 1]) --hlit;
  uint32_t clf[kPngClSyms];
  for (int i = 0; i < kPngClSyms; ++i) clf[i] = 0;
  for (int i = 0; i < hlit; ++i) clf[t->len[i]]++;
  clf[1]++;   // the distance code 0, one bit
  st_png_block_cl(wk, clf, hlit, t);
  uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)t->hclen + t->cl_len[1];
  for (int i = 0; i < hlit; ++i) bits += t->cl_len[t->len[i]];
  t->header_bits = bits;
}

// BFINAL = 0, BTYPE = 2, HLIT, HDIST = 1 code, HCLEN, the code-length code's lengths, then the lengths; put(value, bits)
template <class Put>
ST_PNG_HD void st_png_block_header_front(const StPngBlockTables& t, Put put) {   // 17 + 3 * hclen bits
  put(0u, 1);
  put(2u, 2);
  put((unsigned)(t.hlit - 257), 5);
  put(0u, 5);
  put((unsigned)(t.hclen - 4), 4);
  for (int i = 0; i < t.hclen; ++i) put((unsigned)t.cl_len[st_png_cl_order(i)], 3);
}
template <class Put>
ST_PNG_HD void st_png_block_header(const StPngBlockTables& t, Put put) {
  st_png_block_header_front(t, put);
  for (int i = 0; i < t.hlit; ++i) put((unsigned)t.cl_code[t.len[i]], (int)t.cl_len[t.len[i]]);
  put((unsigned)t.cl_code[1], (int)t.cl_len[1]);
}

// bytes of a piece written as a dynamic block followed by the empty stored block, from the block's bits (header, tokens and
// the end-of-block code); the piece is written stored (5 + its bytes) unless this is shorter
ST_PNG_HD uint32_t st_png_coded_bytes(uint32_t block_bits) { return (block_bits + 3 + 7) / 8 + 4; }

// CRC-32 (reflected, 0xEDB88320) as a polynomial: x^0 is bit 31.  a * b mod P, and x^(8 n) mod P
ST_PNG_HD uint32_t st_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
ST_PNG_HD uint32_t st_crc_x8n(uint32_t n) {
  uint32_t p = 0x80000000u, sq = 0x00800000u;   // x^0; x^8
  for (; n; n >>= 1) {
    if (n & 1u) p = st_crc_mul(sq, p);
    sq = st_crc_mul(sq, sq);
  }
  return p;
}
ST_PNG_HD uint32_t st_crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
  return i;
}

#endif  // ST_PNG_ENC_H_
