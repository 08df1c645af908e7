// Runs the host side of the PNG decoder (st_png_probe, st_png_filtered, st_png_decode_host: the container parser, the inflater
// and the CPU twin) over a corpus of streams and over every truncation of its valid ones, with heap buffers of exactly the
// sizes the calls are promised, so that a build with -fsanitize=address,undefined reports any read or write out of bounds.
// Stand-alone: compile it together with scannertools_amd/csrc/st_png_host.cpp (no HIP, no GPU):
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iscannertools_amd/csrc \
//       scripts/png_host_check.cpp scannertools_amd/csrc/st_png_host.cpp -o png_host_check
//   ./png_host_check tests/golden/png_host_corpus.bin
// The corpus (tests/golden/make_png_golden.py writes it): "PNGC", then per stream one byte 'V' (decodes) or 'M' (must be
// refused), its length as 4 little-endian bytes, and its bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scannertools_hip.h"

namespace {
int failures = 0;

// the three calls on a private copy of exactly `size` bytes; returns st_png_decode_host's status
int run(const uint8_t* data, size_t size) {
  uint8_t* buf = (uint8_t*)malloc(size ? size : 1);
  memcpy(buf, data, size);
  st_png_info info;
  const int probe = st_png_probe(buf, size, &info);
  size_t raw_bytes = 16, frame_bytes = 16;
  if (probe == ST_OK) {
    const int samples = info.color_type == 0 || info.color_type == 3 ? 1 : info.color_type == 4 ? 2 : info.color_type == 2 ? 3 : 4;
    raw_bytes = (size_t)info.h * (1 + ((size_t)info.w * samples * info.bit_depth + 7) / 8);
    frame_bytes = (size_t)info.h * info.w * info.channels;
  }
  uint8_t* raw = (uint8_t*)malloc(raw_bytes);
  uint8_t* frame = (uint8_t*)malloc(frame_bytes);
  st_png_info i2, i3;
  const int filtered = st_png_filtered(buf, size, raw, raw_bytes, &i2);
  const int decoded = st_png_decode_host(buf, size, frame, frame_bytes, &i3);
  if ((filtered == ST_OK) != (decoded == ST_OK)) {
    printf("stage 1 and the whole decode disagree: %d (%s) / %d (%s)\n", filtered, i2.message, decoded, i3.message);
    ++failures;
  }
  if (decoded != ST_OK && i3.message[0] == 0) {
    printf("status %d without a message\n", decoded);
    ++failures;
  }
  free(frame);
  free(raw);
  free(buf);
  return decoded;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> all;
  uint8_t chunk[65536];
  for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) all.insert(all.end(), chunk, chunk + k);
  fclose(f);
  if (all.size() < 4 || memcmp(all.data(), "PNGC", 4) != 0) {
    fprintf(stderr, "%s is not a corpus\n", argv[1]);
    return 2;
  }
  int streams = 0, truncations = 0;
  for (size_t pos = 4; pos < all.size();) {
    if (all.size() - pos < 5) { fprintf(stderr, "corpus cut short\n"); return 2; }
    const bool valid = all[pos] == 'V';
    const size_t len = (size_t)all[pos + 1] | (size_t)all[pos + 2] << 8 | (size_t)all[pos + 3] << 16 | (size_t)all[pos + 4] << 24;
    pos += 5;
    if (all.size() - pos < len) { fprintf(stderr, "corpus cut short\n"); return 2; }
    const uint8_t* s = all.data() + pos;
    const int st = run(s, len);
    if (valid != (st == ST_OK)) {
      printf("stream %d: %s, status %d\n", streams, valid ? "must decode" : "must be refused", st);
      ++failures;
    }
    if (valid)
      for (size_t cut = 0; cut < len; ++cut, ++truncations)
        if (run(s, cut) == ST_OK) {
          printf("stream %d cut to %zu of %zu bytes still decodes\n", streams, cut, len);
          ++failures;
        }
    pos += len;
    ++streams;
  }
  printf("png_host_check: %d streams, %d truncations, %d failures\n", streams, truncations, failures);
  return failures ? 1 : 0;
}
