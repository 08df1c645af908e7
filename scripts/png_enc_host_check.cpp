// Runs the host side of the PNG encoder (st_png_encode_bound, st_png_encode_host, st_png_huff_limited, st_png_encode_check)
// over frames made here -- every geometry and content kind of tests/png_encode_cases.py, every filter -- with heap buffers of
// exactly the sizes the calls are promised, decodes every stream back with st_png_decode_host and compares, so that a build with
// -fsanitize=address,undefined reports any read or write out of bounds and any undefined arithmetic.
// Stand-alone: compile it together with the two host sources (no HIP, no GPU):
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iscannertools_amd/csrc \
//       scripts/png_enc_host_check.cpp scannertools_amd/csrc/st_png_enc_host.cpp scannertools_amd/csrc/st_png_host.cpp -o png_enc_host_check
//   ./png_enc_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scannertools_hip.h"

namespace {
int failures = 0, streams = 0;
unsigned long long rng_state = 88172645463325252ull;
unsigned rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 24);
}

enum Kind { NOISE, SMOOTH, ZEROS, ONES, RUNS, SHEET, FIB };

void fill(uint8_t* f, int h, int w, int c, Kind k) {
  const size_t n = (size_t)h * w * c;
  for (size_t i = 0; i < n; ++i) {
    const int y = (int)(i / ((size_t)w * c)), x = (int)(i / c % w), ch = (int)(i % c);
    switch (k) {
      case NOISE: f[i] = (uint8_t)rnd(); break;
      case SMOOTH: f[i] = (uint8_t)(3 * x + 2 * y + 40 * ch + rnd() % 5); break;
      case ZEROS: f[i] = 0; break;
      case ONES: f[i] = 255; break;
      case RUNS: f[i] = (uint8_t)((i / (1 + (i * 7 / 1000) % 600)) & 1 ? 7 : i % 3); break;
      case SHEET: f[i] = (y > h / 4 && y < 3 * h / 4 && x > w / 4 && x < 3 * w / 4) ? (uint8_t)(x + y + rnd() % 7) : 0; break;
      case FIB: {   // value v about fib(v) times
        unsigned r = rnd() % 28657, v = 1, a = 1, b = 1;
        while (r >= a && v < 22) { r -= a; const unsigned t = a + b; a = b; b = t; ++v; }
        f[i] = (uint8_t)v;
        break;
      }
    }
  }
}

void one(int h, int w, int c, Kind k, int filter) {
  const size_t n = (size_t)h * w * c;
  uint8_t* frame = (uint8_t*)malloc(n);
  fill(frame, h, w, c, k);
  size_t size = 0;
  if (st_png_encode_host(frame, h, w, c, filter, nullptr, 0, &size) != ST_OK || size == 0 || (long long)size > st_png_encode_bound(h, w, c)) {
    printf("%dx%dx%d kind %d filter %d: no size, or beyond the bound\n", h, w, c, (int)k, filter);
    ++failures;
    free(frame);
    return;
  }
  uint8_t* buf = (uint8_t*)malloc(size);   // exactly the stream
  size_t again = 0;
  const int st = st_png_encode_host(frame, h, w, c, filter, buf, size, &again);
  uint8_t* back = (uint8_t*)malloc(n);
  st_png_info info;
  const int dec = st == ST_OK ? st_png_decode_host(buf, size, back, n, &info) : -1;
  if (st != ST_OK || again != size || dec != ST_OK || info.h != h || info.w != w || info.channels != c || memcmp(back, frame, n) != 0) {
    printf("%dx%dx%d kind %d filter %d: encode %d, decode %d (%s)\n", h, w, c, (int)k, filter, st, dec, dec > 0 ? info.message : "");
    ++failures;
  }
  if (size > 1 && st_png_encode_host(frame, h, w, c, filter, buf, size - 1, &again) != ST_ERR_INVALID) {
    printf("a buffer one byte short was not refused\n");
    ++failures;
  }
  ++streams;
  free(back);
  free(buf);
  free(frame);
}

void huff(const std::vector<uint32_t>& counts, int limit) {
  uint32_t* c = (uint32_t*)malloc(counts.size() * sizeof(uint32_t));
  uint8_t* len = (uint8_t*)malloc(counts.size());
  memcpy(c, counts.data(), counts.size() * sizeof(uint32_t));
  if (st_png_huff_limited(c, (int)counts.size(), limit, len) != ST_OK) {
    printf("huff: refused %zu symbols at limit %d\n", counts.size(), limit);
    ++failures;
  } else {
    unsigned long long kraft = 0;
    for (size_t i = 0; i < counts.size(); ++i) {
      if (len[i] > limit || (counts[i] && !len[i])) ++failures;
      if (len[i]) kraft += 1ull << (limit - len[i]);
    }
    if (kraft != 1ull << limit) {
      printf("huff: Kraft sum %llu / %llu\n", kraft, 1ull << limit);
      ++failures;
    }
  }
  free(len);
  free(c);
}
}  // namespace

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, 3}, {1, 1, 4}, {1, 5, 3}, {5, 1, 3}, {3, 7, 3}, {17, 21, 4}, {33, 65, 3}, {64, 64, 3},
                           {7, 4680, 1}, {128, 255, 1}, {33, 992, 1}, {128, 1023, 1}, {1, 28656, 1}, {90, 130, 3}};
  for (const auto& s : shapes)
    for (int k = NOISE; k <= FIB; ++k)
      for (int filter = ST_PNG_FILTER_NONE; filter <= ST_PNG_FILTER_ADAPTIVE; ++filter) {
        if ((size_t)s[0] * s[1] * s[2] > 40000 && filter != ST_PNG_FILTER_NONE && filter != ST_PNG_FILTER_ADAPTIVE && filter != ST_PNG_FILTER_PAETH) continue;
        one(s[0], s[1], s[2], (Kind)k, filter);
      }
  std::vector<uint32_t> fib = {1, 1};
  while (fib.size() < 30) fib.push_back(fib[fib.size() - 1] + fib[fib.size() - 2]);
  std::vector<uint32_t> h286(286, 0);
  h286[40] = 17;
  huff(h286, 15);
  h286[7] = 1000000;
  huff(h286, 15);
  huff(std::vector<uint32_t>(286, 3), 15);
  huff(std::vector<uint32_t>(286, 0), 15);
  for (int n : {20, 30}) {
    std::vector<uint32_t> v(286, 0);
    for (int i = 0; i < n; ++i) v[i] = fib[i];
    huff(v, 15);
  }
  huff(std::vector<uint32_t>(fib.begin(), fib.begin() + 19), 7);
  huff(std::vector<uint32_t>(fib.rbegin() + 11, fib.rend()), 7);
  for (int sym = 2; sym <= 19; ++sym) {
    std::vector<uint32_t> v(sym);
    for (int t = 0; t < 50; ++t) {
      for (auto& x : v) x = rnd() % 3 ? rnd() % (1u << (rnd() % 20)) : 0;
      huff(v, 7);
    }
  }
  char msg[160];
  uint8_t px[4] = {1, 2, 3, 4};
  size_t size = 5;
  const int bad[][4] = {{1, 1, 2, 5}, {0, 1, 3, 5}, {1, 65536, 3, 5}, {1, 1, 3, 6}, {1, 1, 3, -1}};
  for (const auto& b : bad)
    if (st_png_encode_check(b[0], b[1], b[2], b[3], msg, sizeof msg) != ST_ERR_INVALID || !msg[0] ||
        st_png_encode_host(px, b[0], b[1], b[2], b[3], px, 4, &size) != ST_ERR_INVALID || size != 5 || st_png_encode_bound(b[0], b[1], b[2]) != (b[3] == 5 ? -1 : st_png_encode_bound(1, 1, 3))) {
      printf("refusal %d %d %d %d\n", b[0], b[1], b[2], b[3]);
      ++failures;
    }
  printf("%d streams encoded and decoded back, %d failure(s)\n", streams, failures);
  return failures ? 1 : 0;
}
