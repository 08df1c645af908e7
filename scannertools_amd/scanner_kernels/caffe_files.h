// The one reader of Caffe's two file formats (users: pose_net.h, the pose network; caffe_net.h, any network of the layer set):
// a whole file into memory, a caffemodel's blobs by layer name (read_caffemodel), a deploy description as a tree (read_prototxt).
// Python twin: scannertools_amd/caffe_files.py.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <string>
#include <utility>
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

// ---- caffemodel ----------------------------------------------------------------------------------------------------------
// NetParameter wire format ([EXT] caffe.proto): layer = 100 (LayerParameter: name = 1, blobs = 7) or the V1 `layers` = 2
// (name = 4, blobs = 6); BlobProto: data = 5 (packed float).  Only the float payloads are read: the shapes are the description's.
using Blobs = std::map<std::string, std::vector<std::vector<float>>>;

// Every layer of the file that carries blobs (any number of them), by name.
// The file is untrusted input and this reader sits behind extern "C" entry points and kernel constructors: nothing
// may leave it as an exception (std::bad_alloc / std::length_error on a hostile length field would otherwise
// cross the C ABI and end the host process instead of becoming a validate() error).
inline bool read_caffemodel(const std::string& path, Blobs* out, std::string* err) {
  try {
    std::string buf;
    if (!read_file(path, &buf)) { *err = "cannot read the weights file " + path; return false; }
    std::vector<proto_lite::Field> top;
    if (!proto_lite::parse((const uint8_t*)buf.data(), buf.size(), &top)) { *err = path + " is not a serialized NetParameter"; return false; }
    for (auto& f : top) {
      if (f.wire != 2 || (f.number != 100 && f.number != 2)) continue;
      const uint32_t name_field = f.number == 100 ? 1 : 4, blob_field = f.number == 100 ? 7 : 6;
      std::vector<proto_lite::Field> lf;
      if (!proto_lite::parse((const uint8_t*)f.bytes.data(), f.bytes.size(), &lf)) { *err = "malformed layer in " + path; return false; }
      std::string name;
      std::vector<std::vector<float>> blobs;
      for (auto& g : lf) {
        if (g.number == name_field && g.wire == 2) name = g.bytes;
        else if (g.number == blob_field && g.wire == 2) {
          blobs.emplace_back();
          if (!blob_floats(g.bytes, &blobs.back())) { *err = "malformed blob in " + path; return false; }
        }
      }
      if (!name.empty() && !blobs.empty()) (*out)[name] = std::move(blobs);
    }
    return true;
  } catch (const std::exception& e) {
    *err = "cannot parse " + path + ": " + e.what();
  } catch (...) {
    *err = "cannot parse " + path;
  }
  out->clear();
  return false;
}

// ---- prototxt ------------------------------------------------------------------------------------------------------------
// protobuf text format as a tree
struct Msg {
  std::vector<std::pair<std::string, std::string>> scalars;
  std::vector<std::pair<std::string, Msg>> subs;
  const std::string* get(const std::string& k) const {
    for (auto& s : scalars)
      if (s.first == k) return &s.second;
    return nullptr;
  }
  std::vector<std::string> all(const std::string& k) const {
    std::vector<std::string> v;
    for (auto& s : scalars)
      if (s.first == k) v.push_back(s.second);
    return v;
  }
  const Msg* sub(const std::string& k) const {
    for (auto& s : subs)
      if (s.first == k) return &s.second;
    return nullptr;
  }
  int geti(const std::string& k, int dflt) const { auto* s = get(k); return s ? atoi(s->c_str()) : dflt; }
  float getf(const std::string& k, float dflt) const { auto* s = get(k); return s ? strtof(s->c_str(), nullptr) : dflt; }
  bool getb(const std::string& k, bool dflt) const { auto* s = get(k); return s ? (*s == "true" || *s == "1") : dflt; }
};

inline bool parse_msg(const std::vector<std::string>& tok, size_t* i, bool closing, int depth, Msg* out, std::string* err) {
  if (depth > 64) { *err = "prototxt nests deeper than 64 messages"; return false; }
  while (*i < tok.size()) {
    const std::string& t = tok[*i];
    if (t == "}") {
      if (!closing) { *err = "unbalanced '}' in the prototxt"; return false; }
      ++*i;
      return true;
    }
    if (t == "{" || t == ":") { *err = "unexpected '" + t + "' in the prototxt"; return false; }
    size_t j = *i + 1;
    if (j < tok.size() && tok[j] == ":") ++j;
    if (j >= tok.size()) { *err = "field " + t + " has no value in the prototxt"; return false; }
    if (tok[j] == "{") {
      *i = j + 1;
      out->subs.emplace_back(t, Msg());
      if (!parse_msg(tok, i, true, depth + 1, &out->subs.back().second, err)) return false;
    } else {
      std::string v = tok[j];
      if (!v.empty() && v[0] == '"') v = v.substr(1);
      out->scalars.emplace_back(t, v);
      *i = j + 1;
    }
  }
  if (closing) { *err = "missing '}' in the prototxt"; return false; }
  return true;
}

// file -> tokens -> tree; a text that is no prototxt is refused with the path behind the reason
inline bool read_prototxt(const std::string& path, Msg* out, std::string* err) {
  std::string text;
  if (!read_file(path, &text)) { *err = "cannot read the model description " + path; return false; }
  std::vector<std::string> tok;
  size_t i = 0;
  if (!prototxt_tokens(text, &tok, err) || !parse_msg(tok, &i, false, 0, out, err)) { *err += " (" + path + ")"; return false; }
  return true;
}

}  // namespace caffe_files
}  // namespace scanner
