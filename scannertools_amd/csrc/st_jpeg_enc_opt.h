// Optimised Huffman tables for the ImageEncoder op, shared by the host (st_jpeg_optimal_table,
// st_jpeg_symbol_stats in st_jpeg_enc_host.cpp) and the device (k_jpeg_sym_stats, k_jpeg_opt_tables in st_jpeg_enc.hip):
// __host__ __device__ inline functions that also compile as plain C++17, where the two qualifiers are defined away.
//   - st_jpeg_opt_block_symbols: the symbols jchuff's htest_one_block counts for one block -- exactly those code_block emits;
//   - st_jpeg_opt_least / st_jpeg_opt_better / st_jpeg_opt_merge / st_jpeg_opt_lengths: jpeg_gen_optimal_table in libjpeg 6b's
//     form, cut where a wave can share the two minimum searches of a merge step;
//   - st_jpeg_opt_codes: the canonical codes (T.81 Annex C) as the (length << 16 | code) words k_jpeg_entropy reads;
//   - st_jpeg_opt_dht: the bytes of one DHT segment.
// Every index is bounded by construction: symbols are 0 .. 255 (256: the reserved pseudo-symbol), chains of `others` end at -1
// and never repeat an entry (an entry is appended to a chain at most once: when it is c2, after which its frequency is 0 and it
// is never chosen again), and a code size above 32 -- where libjpeg stops -- is counted apart, see st_jpeg_opt_lengths.
#ifndef ST_JPEG_ENC_OPT_H_
#define ST_JPEG_ENC_OPT_H_

#include <stddef.h>
#include <stdint.h>

#ifndef __HIP__
#define __host__
#define __device__
#endif

constexpr int kJpegOptSymbols = 257;   // 256 symbols and the pseudo-symbol 256 whose code is all ones and is never written
constexpr int kJpegOptMaxLen = 32;     // longest code before the limiting, as in libjpeg (MAX_CLEN)
// The four tables in the order of their DHT segments: DC luma, AC luma, DC chroma, AC chroma.
constexpr int kJpegOptTables = 4;
__host__ __device__ inline int st_jpeg_opt_class_id(int t) { return t == 0 ? 0x00 : t == 1 ? 0x10 : t == 2 ? 0x01 : 0x11; }
// ... and where each table's words start among the kJpegEncHuffWords (st_jpeg_enc_host.h), and how many there are
__host__ __device__ inline int st_jpeg_opt_tab_off(int t) { return t == 0 ? 0 : t == 1 ? 32 : t == 2 ? 16 : 288; }
__host__ __device__ inline int st_jpeg_opt_tab_words(int t) { return (t & 1) ? 256 : 16; }
// A worst-case block with ANY table of codes up to 16 bits: a DC code and 11 magnitude bits, 63 AC codes with 10 magnitude bits.
constexpr int kJpegEncBlockBitsOpt = (16 + 11) + 63 * (16 + 10);   // 1665
constexpr size_t kJpegEncBlockBytesOpt = 209;                      // 1665 bits are 208.125 bytes
constexpr size_t kJpegEncBlockStuffedOpt = 418;
constexpr size_t kJpegEncHeaderPrefix = 177;   // SOI, APP0, two DQT, SOF0: what stands in front of the four DHT segments
constexpr size_t kJpegEncHeaderStride = 640;   // a frame's header in device memory: at most 629 bytes, padded

// The magnitude category of v, at most `most` (the transform kernel clamps: 11 for DC differences, 10 for AC values).
__host__ __device__ inline int st_jpeg_opt_category(int v, int most) {
  unsigned t = (unsigned)(v < 0 ? -v : v);
  int n = 0;
  while (t) {
    ++n;
    t >>= 1;
  }
  return n > most ? most : n;
}

// The symbols of one block: add(0, category of the DC difference), then add(1, symbol) per AC symbol -- 0xF0 per run of 16
// zeros in front of a non-zero coefficient, (run << 4) | size per non-zero coefficient, 0x00 when the block ends in zeros.
// at(k): the coefficient at position k = 1 .. 63 of the zigzag scan.
template <class Coef, class Add>
__host__ __device__ inline void st_jpeg_opt_block_symbols(const Coef& at, int diff, const Add& add) {
  add(0, st_jpeg_opt_category(diff, 11));
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = at(k);
    if (v == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {
      add(1, 0xF0);
      run -= 16;
    }
    add(1, (run << 4) | st_jpeg_opt_category(v, 10));
    run = 0;
  }
  if (run > 0) add(1, 0x00);
}

// Of two candidates (frequency, index; index < 0: none) the one the reference's upward scan with `<=` ends on: the smaller
// frequency, and among equal frequencies the LARGER index.  Associative and commutative, so a reduction in any order gives it.
__host__ __device__ inline bool st_jpeg_opt_better(uint64_t va, int ia, uint64_t vb, int ib) {   // is a the one to keep?
  if (ib < 0) return true;
  if (ia < 0) return false;
  return va < vb || (va == vb && ia > ib);
}

// The entry of freq[lo, hi) with the least non-zero frequency, `exclude` left out; -1 where there is none.
__host__ __device__ inline int st_jpeg_opt_least(const uint64_t* freq, int lo, int hi, int exclude, uint64_t* value) {
  int best = -1;
  uint64_t v = 0;
  for (int i = lo; i < hi; ++i)
    if (freq[i] && i != exclude && st_jpeg_opt_better(freq[i], i, v, best)) {
      v = freq[i];
      best = i;
    }
  *value = v;
  return best;
}

// One merge step: c2's tree joins c1's.  The walks end because each chain is a list without repeats of at most 257 entries.
__host__ __device__ inline void st_jpeg_opt_merge(uint64_t* freq, int* codesize, int* others, int c1, int c2) {
  freq[c1] += freq[c2];
  freq[c2] = 0;
  codesize[c1]++;
  int guard = kJpegOptSymbols;
  while (others[c1] >= 0 && --guard > 0) {
    c1 = others[c1];
    codesize[c1]++;
  }
  others[c1] = c2;
  codesize[c2]++;
  guard = kJpegOptSymbols;
  while (others[c2] >= 0 && --guard > 0) {
    c2 = others[c2];
    codesize[c2]++;
  }
}

// From the code sizes to the DHT's bits[16] and vals: count the lengths, shorten codes of more than 16 bits as the reference
// does (T.81 K.2's adjustment), take the pseudo-symbol out of the longest length in use, list the symbols by length and value.
// The merge loop leaves a COMPLETE code (Kraft sum 1 with the pseudo-symbol), and each adjustment step keeps it complete, so the
// deepest length always holds an even number of codes and a shorter length in use exists below it: the inner loops end.
// A code size is at most 256 in principle (257 leaves).  The reference refuses more than 32 (JERR_HUFF_CLEN_OVERFLOW), which
// takes frequencies that grow like Fibonacci numbers over 34 symbols or more -- some 15 million symbols of one table in one
// frame, in that proportion.  The device cannot stop a call there, so such a histogram gets a table that is valid though
// neither optimal nor the reference's: every symbol in use a code of 9 or 10 bits.  Returns the number of symbols whose size
// was above 32 (0 for every histogram libjpeg accepts).
__host__ __device__ inline int st_jpeg_opt_lengths(const int* codesize, uint8_t bits16[16], uint8_t* vals, int* nvals) {
  int bits[kJpegOptMaxLen + 1];
  int over = 0;
  for (int i = 0; i <= kJpegOptMaxLen; ++i) bits[i] = 0;
  for (int i = 0; i < kJpegOptSymbols; ++i)
    if (codesize[i]) {
      if (codesize[i] > kJpegOptMaxLen) ++over;
      else bits[codesize[i]]++;
    }
  if (over) {
    int p = 0;
    for (int s = 0; s < 256; ++s)
      if (codesize[s]) vals[p++] = (uint8_t)s;
    for (int i = 0; i < 16; ++i) bits16[i] = 0;
    bits16[8] = (uint8_t)(p < 128 ? p : 128);          // 128 / 512 + 128 / 1024 < 1, and no code is all ones
    bits16[9] = (uint8_t)(p < 128 ? 0 : p - 128);
    *nvals = p;
    return over;
  }
  for (int i = kJpegOptMaxLen; i > 16; --i)
    while (bits[i] > 0) {
      int j = i - 2;
      while (j > 0 && bits[j] == 0) --j;
      if (j == 0 || bits[i] < 2) {   // never with a complete code; kept so that the loop ends whatever it is given
        bits[i - 1] += bits[i];
        bits[i] = 0;
        break;
      }
      bits[i] -= 2;
      bits[i - 1]++;
      bits[j + 1] += 2;
      bits[j]--;
    }
  int top = 16;
  while (top > 0 && bits[top] == 0) --top;
  if (top > 0) bits[top]--;
  for (int i = 0; i < 16; ++i) bits16[i] = (uint8_t)(bits[i + 1] > 255 ? 255 : bits[i + 1]);
  int p = 0;
  for (int len = 1; len <= kJpegOptMaxLen; ++len)
    for (int s = 0; s < 256; ++s)
      if (codesize[s] == len) vals[p++] = (uint8_t)s;   // p <= 256: each symbol has one size
  *nvals = p;
  return 0;
}

// The canonical codes of (bits16, vals) as (length << 16) | code at tab[symbol], symbol < words (16 for a DC table, 256 for an
// AC one; a symbol beyond it is skipped); tab[0, words) is zeroed first: 0 for a symbol without a code.
__host__ __device__ inline void st_jpeg_opt_codes(const uint8_t bits16[16], const uint8_t* vals, int nvals, uint32_t* tab, int words) {
  for (int i = 0; i < words; ++i) tab[i] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits16[len - 1] && k < nvals; ++i, ++k, ++code)
      if (vals[k] < words) tab[vals[k]] = ((uint32_t)len << 16) | (code & 0xffffu);
    code <<= 1;
  }
}

// Bytes of the DHT segment of a table with nvals symbols, marker included.
__host__ __device__ inline int st_jpeg_opt_dht_bytes(int nvals) { return 2 + 2 + 1 + 16 + nvals; }
// The segment's byte i, i < st_jpeg_opt_dht_bytes(nvals): so that the lanes of a wave can write it side by side.
__host__ __device__ inline uint8_t st_jpeg_opt_dht_byte(const uint8_t bits16[16], const uint8_t* vals, int nvals, int class_id, int i) {
  const int len = 2 + 1 + 16 + nvals;
  if (i == 0) return 0xFF;
  if (i == 1) return 0xC4;
  if (i == 2) return (uint8_t)(len >> 8);
  if (i == 3) return (uint8_t)len;
  if (i == 4) return (uint8_t)class_id;
  if (i < 21) return bits16[i - 5];
  return vals[i - 21];
}

// The whole construction for one histogram, serially: what the host runs and what the device's wave-shared loop must equal.
// Scratch is the caller's (4 KiB): the device keeps it in LDS.
struct StJpegOptWork {
  uint64_t freq[kJpegOptSymbols];
  int codesize[kJpegOptSymbols];
  int others[kJpegOptSymbols];
};

__host__ __device__ inline void st_jpeg_opt_begin(StJpegOptWork* w, int i, uint64_t count) {   // i = 0 .. 256
  w->freq[i] = i == 256 ? 1 : count;
  w->codesize[i] = 0;
  w->others[i] = -1;
}

inline int st_jpeg_opt_table_serial(const uint64_t freq[256], StJpegOptWork* w, uint8_t bits16[16], uint8_t* vals, int* nvals) {
  for (int i = 0; i < kJpegOptSymbols; ++i) st_jpeg_opt_begin(w, i, i < 256 ? freq[i] : 1);
  for (int step = 0; step < kJpegOptSymbols; ++step) {   // at most 256 merges join 257 entries
    uint64_t v;
    const int c1 = st_jpeg_opt_least(w->freq, 0, kJpegOptSymbols, -1, &v);
    const int c2 = st_jpeg_opt_least(w->freq, 0, kJpegOptSymbols, c1, &v);
    if (c2 < 0) break;
    st_jpeg_opt_merge(w->freq, w->codesize, w->others, c1, c2);
  }
  return st_jpeg_opt_lengths(w->codesize, bits16, vals, nvals);
}

#endif  // ST_JPEG_ENC_OPT_H_
