// What the readers of Caffe's two file formats share (pose_net.h: the pose network; caffe_net.h: any network of the layer set):
// a whole file into memory, the floats of a BlobProto, the tokens of a protobuf text file.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "proto_lite.h"

namespace scanner {
namespace caffe_files {

// Whole file into memory; false for anything that is not a readable regular file of a plausible size (a directory
// opens with fopen() and reports LONG_MAX from ftell()).
inline bool read_file(const std::string& path, std::string* out) {
  struct stat sb;
  if (stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
  constexpr long kMaxModelBytes = 1L << 32;  // the COCO body model is 209 MB
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  bool ok = fseek(f, 0, SEEK_END) == 0;
  const long n = ok ? ftell(f) : -1;
  ok = ok && n >= 0 && n <= kMaxModelBytes && fseek(f, 0, SEEK_SET) == 0;
  if (ok) {
    out->resize((size_t)n);
    ok = n == 0 || fread(&(*out)[0], 1, out->size(), f) == out->size();
  }
  fclose(f);
  return ok;
}

inline bool blob_floats(const std::string& blob, std::vector<float>* out) {
  std::vector<proto_lite::Field> fs;
  if (!proto_lite::parse((const uint8_t*)blob.data(), blob.size(), &fs)) return false;
  out->clear();
  for (auto& f : fs) {
    if (f.number != 5) continue;
    if (f.wire == 2) {
      const size_t n = f.bytes.size() / 4, at = out->size();
      out->resize(at + n);
      memcpy(out->data() + at, f.bytes.data(), n * 4);
    } else if (f.wire == 5) {
      out->push_back(proto_lite::as_float(f));
    }
  }
  return true;
}

// tokens of a protobuf text file: identifiers / numbers, quoted strings (with a leading quote mark), '{', '}', ':'; '#' starts
// a comment
inline bool prototxt_tokens(const std::string& text, std::vector<std::string>* tok, std::string* err) {
  for (size_t i = 0; i < text.size();) {
    const char c = text[i];
    if (c == '#') { while (i < text.size() && text[i] != '\n') ++i; continue; }
    if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == ',' || c == ';') { ++i; continue; }
    if (c == '{' || c == '}' || c == ':') { tok->push_back(std::string(1, c)); ++i; continue; }
    if (c == '"' || c == '\'') {
      size_t j = i + 1;
      while (j < text.size() && text[j] != c) j += text[j] == '\\' ? 2 : 1;
      if (j >= text.size()) { *err = "unterminated string in the prototxt"; return false; }
      tok->push_back("\"" + text.substr(i + 1, j - i - 1));  // strings carry a leading quote mark
      i = j + 1;
      continue;
    }
    size_t j = i;
    while (j < text.size() && !strchr(" \t\n\r{}:#\"',;", text[j])) ++j;
    tok->push_back(text.substr(i, j - i));
    i = j;
  }
  return true;
}

}  // namespace caffe_files
}  // namespace scanner
