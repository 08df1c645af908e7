// A Caffe network of the supported layer set as a sequence of C-ABI layer calls: what the forward pass behind CaffeKernel::execute
// (/root/reference/scannertools_caffe/scannertools_caffe_cpp/caffe_kernel.cpp:382, net_->ForwardPrefilled()) computes for a deploy
// prototxt and a caffemodel.  Caffe itself is not in the reference tree; the layer rules are restated from its public sources
// ([EXT], unpinned):
//   Input (and the legacy input: / input_dim / input_shape header), Convolution (square kernel, pad, stride, group, bias_term;
//   dilation 1), ReLU (negative_slope 0), Pooling (MAX / AVE, global_pooling), LRN (ACROSS_CHANNELS), Concat (axis 1), InnerProduct,
//   Dropout (identity), Split (aliases), Softmax (axis 1).  V1 upper-case type names are accepted.  Anything else is refused by name.
// Plan (host only, no GPU): the layers are walked in file order -- Caffe's execution order -- from the input blob to the requested
// output blob; in-place layers make a new VERSION of their blob in the same buffer.  A ReLU is fused into the Convolution /
// InnerProduct that produced its bottom when nothing else reads that version.  A Concat bottom whose channel offset is a multiple
// of 16 and that nothing else reads is written by its producer straight into the Concat's buffer; the others are copied.
// Layout: NHWC float32, channel stride a multiple of 16, pad channels zero (buffers are zeroed when allocated and no kernel writes
// outside its channels).  Stride-1 "same" convolutions with odd k <= 7 and group 1 run on the MFMA kernels of st_conv.hip, every
// other geometry on st_conv2d_general_nhwc_f32.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <exception>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "caffe_files.h"
#include "net_weights.h"
#include "scannertools_hip.h"

namespace scanner {
namespace caffe_net {

using caffe_files::Blobs;
using caffe_files::Msg;

// ---- layers --------------------------------------------------------------------------------------------------------------
enum Kind { kInput, kConv, kReLU, kPool, kLRN, kConcat, kIP, kDropout, kSplit, kSoftmax };

struct Layer {
  std::string name, type;
  Kind kind = kInput;
  std::vector<std::string> bottoms, tops;
  int num_output = 0, k = 1, stride = 1, pad = 0, group = 1;
  bool bias = true, global = false, ave = false;
  int local_size = 5;
  float alpha = 1.f, beta = 0.75f, lrn_k = 1.f;
  std::vector<int> in_shape;   // Input: dims
};

struct Shape { int c = 0, h = 1, w = 1, axes = 4; };

// one launch of the forward pass
struct Step {
  Kind kind;
  int layer;
  int relu = 0;
  bool mfma = false;          // Convolution on st_conv2d_nhwc_f32_tiled
  std::vector<int> in;        // blob versions
  int out = -1;
};

// where a blob version lives: buffer, channel offset inside it
struct Place { int buf = -1, off = 0; };

struct Plan {
  std::vector<Layer> layers;
  std::vector<Step> steps;
  std::vector<Shape> shape;            // per blob version
  std::vector<Place> place;            // per blob version
  std::vector<Shape> buf_shape;        // per buffer: c = channel stride
  int input = -1, output = -1;         // blob versions
  Shape in_shape, out_shape;
};

inline std::string canon(const std::string& type) {
  std::string s;
  for (char c : type)
    if (c != '_') s += (char)tolower((unsigned char)c);
  return s;
}
inline int pad16(int c) { return (c + 15) / 16 * 16; }

inline bool parse_layers(const std::string& path, std::vector<Layer>* out, std::string* err) {
  Msg net;
  if (!caffe_files::read_prototxt(path, &net, err)) return false;
  // the legacy header: input: "data" + input_dim x 4 or input_shape { dim ... }
  if (const std::string* in = net.get("input")) {
    Layer l;
    l.name = *in; l.type = "Input"; l.kind = kInput; l.tops = {*in};
    for (auto& d : net.all("input_dim")) l.in_shape.push_back(atoi(d.c_str()));
    if (l.in_shape.empty())
      if (const Msg* s = net.sub("input_shape"))
        for (auto& d : s->all("dim")) l.in_shape.push_back(atoi(d.c_str()));
    out->push_back(l);
  }
  static const std::map<std::string, Kind> kinds = {{"input", kInput}, {"convolution", kConv}, {"relu", kReLU}, {"pooling", kPool}, {"lrn", kLRN},
                                                    {"concat", kConcat}, {"innerproduct", kIP}, {"dropout", kDropout}, {"split", kSplit},
                                                    {"softmax", kSoftmax}};
  for (auto& s : net.subs) {
    if (s.first != "layer" && s.first != "layers") continue;
    const Msg& m = s.second;
    Layer l;
    if (auto* v = m.get("name")) l.name = *v;
    if (auto* v = m.get("type")) l.type = *v;
    l.bottoms = m.all("bottom");
    l.tops = m.all("top");
    auto it = kinds.find(canon(l.type));
    if (it == kinds.end()) {
      l.num_output = -1;   // refused by name when the layer lies on the path
      out->push_back(l);
      continue;
    }
    l.kind = it->second;
    auto refuse = [&](const std::string& what) { *err = "layer " + l.name + " (" + l.type + "): " + what; return false; };
    auto square = [&](const Msg& p, const char* base, const char* hname, const char* wname, int dflt, int* v) {
      *v = p.geti(base, dflt);
      if (p.get(hname) || p.get(wname)) {
        if (p.geti(hname, dflt) != p.geti(wname, dflt)) return false;
        *v = p.geti(hname, dflt);
      }
      return true;
    };
    static const Msg empty;
    if (l.kind == kInput) {
      if (const Msg* p = m.sub("input_param"))
        if (const Msg* sh = p->sub("shape"))
          for (auto& d : sh->all("dim")) l.in_shape.push_back(atoi(d.c_str()));
    } else if (l.kind == kConv) {
      const Msg& p = m.sub("convolution_param") ? *m.sub("convolution_param") : empty;
      l.num_output = p.geti("num_output", 0);
      if (!square(p, "kernel_size", "kernel_h", "kernel_w", 0, &l.k) || !square(p, "pad", "pad_h", "pad_w", 0, &l.pad) ||
          !square(p, "stride", "stride_h", "stride_w", 1, &l.stride))
        return refuse("only square kernels, pads and strides are implemented");
      l.group = p.geti("group", 1);
      l.bias = p.getb("bias_term", true);
      if (p.geti("dilation", 1) != 1) return refuse("dilation other than 1 is not implemented");
      if (l.num_output <= 0 || l.k <= 0 || l.stride <= 0 || l.pad < 0 || l.group <= 0) return refuse("bad convolution_param");
    } else if (l.kind == kReLU) {
      const Msg& p = m.sub("relu_param") ? *m.sub("relu_param") : empty;
      if (p.getf("negative_slope", 0.f) != 0.f) return refuse("a negative_slope other than 0 is not implemented");
    } else if (l.kind == kPool) {
      const Msg& p = m.sub("pooling_param") ? *m.sub("pooling_param") : empty;
      const std::string method = p.get("pool") ? *p.get("pool") : "MAX";
      if (method != "MAX" && method != "AVE" && method != "0" && method != "1") return refuse("pooling method " + method + " is not implemented (MAX, AVE)");
      l.ave = method == "AVE" || method == "1";
      l.global = p.getb("global_pooling", false);
      if (!square(p, "kernel_size", "kernel_h", "kernel_w", 0, &l.k) || !square(p, "pad", "pad_h", "pad_w", 0, &l.pad) ||
          !square(p, "stride", "stride_h", "stride_w", 1, &l.stride))
        return refuse("only square kernels, pads and strides are implemented");
      if (!l.global && (l.k <= 0 || l.stride <= 0 || l.pad < 0 || l.pad >= l.k)) return refuse("bad pooling_param");
    } else if (l.kind == kLRN) {
      const Msg& p = m.sub("lrn_param") ? *m.sub("lrn_param") : empty;
      const std::string region = p.get("norm_region") ? *p.get("norm_region") : "ACROSS_CHANNELS";
      if (region != "ACROSS_CHANNELS" && region != "0") return refuse("norm_region " + region + " is not implemented (ACROSS_CHANNELS)");
      l.local_size = p.geti("local_size", 5);
      l.alpha = p.getf("alpha", 1.f); l.beta = p.getf("beta", 0.75f); l.lrn_k = p.getf("k", 1.f);
      if (l.local_size <= 0 || !(l.local_size & 1)) return refuse("local_size must be odd");
    } else if (l.kind == kConcat) {
      const Msg& p = m.sub("concat_param") ? *m.sub("concat_param") : empty;
      if (p.geti("axis", 1) != 1 || p.geti("concat_dim", 1) != 1) return refuse("only axis 1 is implemented");
    } else if (l.kind == kIP) {
      const Msg& p = m.sub("inner_product_param") ? *m.sub("inner_product_param") : empty;
      l.num_output = p.geti("num_output", 0);
      l.bias = p.getb("bias_term", true);
      if (p.geti("axis", 1) != 1 || p.getb("transpose", false)) return refuse("only axis 1 without transpose is implemented");
      if (l.num_output <= 0) return refuse("bad inner_product_param");
    } else if (l.kind == kSoftmax) {
      const Msg& p = m.sub("softmax_param") ? *m.sub("softmax_param") : empty;
      if (p.geti("axis", 1) != 1) return refuse("only axis 1 is implemented");
    }
    out->push_back(l);
  }
  return true;
}

// The plan for an input of (c, h, w): c 0 takes the description's own channel count, h or w 0 its own size.  weights (may be
// null): every Convolution / InnerProduct on the path must have blobs of the right element counts; strict_ip false leaves an
// InnerProduct whose input length does not match its weights to the caller (validate() does not know the frame size yet).
inline bool make_plan(const std::string& prototxt, const Blobs* weights, int c, int h, int w, const std::string& input_blob,
                      const std::string& output_blob, bool strict_ip, Plan* plan, std::string* err) try {
  Plan& p = *plan;
  p = Plan();
  if (!parse_layers(prototxt, &p.layers, err)) return false;
  // file order is execution order; a blob name stands for its latest version
  std::map<std::string, int> cur;
  std::vector<int> producer;                         // version -> layer
  std::vector<std::vector<int>> lin(p.layers.size()), lout(p.layers.size());
  for (size_t li = 0; li < p.layers.size(); ++li) {
    const Layer& l = p.layers[li];
    // a layer of a type outside the set is refused by name if it lies on the path; of the others only an Input has no bottom
    if (l.num_output != -1 && (l.tops.empty() || (l.bottoms.empty() && l.kind != kInput))) {
      *err = "malformed description: layer " + l.name + " (" + l.type + ") names no " + (l.tops.empty() ? "top" : "bottom") + " blob";
      return false;
    }
    for (auto& b : l.bottoms) {
      auto it = cur.find(b);
      if (it == cur.end()) {
        *err = "malformed description: layer " + l.name + " reads blob " + b + ", which no earlier layer produces (a cycle or a missing layer)";
        return false;
      }
      lin[li].push_back(it->second);
    }
    for (auto& t : l.tops) {
      cur[t] = (int)producer.size();
      lout[li].push_back((int)producer.size());
      producer.push_back((int)li);
    }
  }
  const size_t nv = producer.size();
  // the input blob: a top of an Input layer (or the legacy header)
  {
    int found = -1;
    for (size_t li = 0; li < p.layers.size(); ++li)
      if (p.layers[li].kind == kInput && p.layers[li].num_output != -1)
        for (size_t t = 0; t < p.layers[li].tops.size(); ++t)
          if (p.layers[li].tops[t] == input_blob) found = lout[li][t];
    if (found < 0) { *err = "the description has no input blob named " + input_blob; return false; }
    p.input = found;
  }
  if (!cur.count(output_blob)) { *err = "the description produces no blob named " + output_blob; return false; }
  p.output = cur[output_blob];
  // layers the output needs
  std::vector<char> need_layer(p.layers.size(), 0), need_v(nv, 0);
  {
    std::vector<int> stack = {p.output};
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      if (need_v[v]) continue;
      need_v[v] = 1;
      need_layer[producer[v]] = 1;
      for (int b : lin[producer[v]]) stack.push_back(b);
    }
  }
  if (!need_v[p.input]) { *err = "blob " + output_blob + " does not depend on the input blob " + input_blob; return false; }
  // shapes
  p.shape.assign(nv, Shape());
  for (size_t li = 0; li < p.layers.size(); ++li) {
    if (!need_layer[li]) continue;
    const Layer& l = p.layers[li];
    auto refuse = [&](const std::string& what) { *err = "layer " + l.name + " (" + l.type + "): " + what; return false; };
    if (l.num_output == -1) return refuse("layer type " + l.type + " is not implemented (Input, Convolution, ReLU, Pooling, LRN, Concat, InnerProduct, Dropout, Split, Softmax)");
    if (l.kind == kInput) {
      if (lout[li][0] != p.input && need_v[lout[li][0]]) return refuse("a second input blob is not implemented");
      Shape s;
      s.c = c > 0 ? c : (l.in_shape.size() >= 2 ? l.in_shape[1] : 0);
      s.h = h > 0 ? h : (l.in_shape.size() >= 3 ? l.in_shape[2] : 0);
      s.w = w > 0 ? w : (l.in_shape.size() >= 4 ? l.in_shape[3] : 0);
      if (l.in_shape.size() >= 2 && s.c != l.in_shape[1])
        return refuse("the input has " + std::to_string(s.c) + " channels, the description's input blob " + std::to_string(l.in_shape[1]));
      if (s.c <= 0 || s.h <= 0 || s.w <= 0) return refuse("malformed description: the input blob has no shape");
      for (int v : lout[li]) p.shape[v] = s;
      continue;
    }
    const Shape b0 = p.shape[lin[li][0]];
    Shape s = b0;
    if (l.kind != kConcat && lin[li].size() != 1) return refuse("more than one bottom blob");
    if (l.kind != kSplit && lout[li].size() != 1) return refuse("more than one top blob");
    switch (l.kind) {
      case kConv:
        s.c = l.num_output;
        s.h = st_conv_out_size(b0.h, l.k, l.stride, l.pad); s.w = st_conv_out_size(b0.w, l.k, l.stride, l.pad);
        if (b0.c % l.group || l.num_output % l.group) return refuse("group does not divide the channel counts");
        if (s.h <= 0 || s.w <= 0) return refuse("the kernel is larger than its padded input (" + std::to_string(b0.h) + " x " + std::to_string(b0.w) + ")");
        break;
      case kPool:
        if (l.global) { s.h = s.w = 1; }
        else { s.h = st_pool_out_size(b0.h, l.k, l.stride, l.pad); s.w = st_pool_out_size(b0.w, l.k, l.stride, l.pad); }
        if (s.h <= 0 || s.w <= 0) return refuse("the kernel is larger than its padded input (" + std::to_string(b0.h) + " x " + std::to_string(b0.w) + ")");
        break;
      case kConcat:
        s.c = 0;
        for (int v : lin[li]) {
          if (p.shape[v].h != b0.h || p.shape[v].w != b0.w) return refuse("bottom blobs of different sizes");
          s.c += p.shape[v].c;
        }
        break;
      case kIP: s.c = l.num_output; s.h = s.w = 1; s.axes = 2; break;
      default: break;
    }
    for (int v : lout[li]) p.shape[v] = s;
    if (weights && (l.kind == kConv || l.kind == kIP)) {
      auto it = weights->find(l.name);
      if (it == weights->end()) return refuse("the weights file has no blobs for this layer");
      const auto& bl = it->second;
      const size_t want = l.kind == kConv ? (size_t)l.num_output * (b0.c / l.group) * l.k * l.k : (size_t)l.num_output * b0.c * b0.h * b0.w;
      if (bl.size() < (l.bias ? 2u : 1u)) return refuse("the weights file holds " + std::to_string(bl.size()) + " blobs for this layer, " + (l.bias ? "2" : "1") + " are needed");
      if (l.bias && bl[1].size() != (size_t)l.num_output)
        return refuse("the bias blob holds " + std::to_string(bl[1].size()) + " values, num_output is " + std::to_string(l.num_output));
      if (l.kind == kIP && bl[0].size() != want && (strict_ip || bl[0].size() % (size_t)l.num_output))
        return refuse("the input is " + std::to_string(b0.c) + " x " + std::to_string(b0.h) + " x " + std::to_string(b0.w) + " = " + std::to_string((size_t)b0.c * b0.h * b0.w) +
                      " values per frame, the weights are for " + std::to_string(bl[0].size() / (size_t)l.num_output));
      if (l.kind == kConv && bl[0].size() != want)
        return refuse("the weight blob holds " + std::to_string(bl[0].size()) + " values, the layer needs " + std::to_string(want));
    }
  }
  // readers of every version among the needed layers
  std::vector<std::vector<int>> readers(nv);
  for (size_t li = 0; li < p.layers.size(); ++li)
    if (need_layer[li])
      for (int v : lin[li]) readers[v].push_back((int)li);
  // steps; fused ReLUs, Dropout and Split only alias
  p.place.assign(nv, Place());
  std::vector<int> step_of(nv, -1);      // version -> the step that computes its buffer's contents (through aliases)
  auto new_buffer = [&](const Shape& s) {
    Shape b = s;
    b.c = pad16(s.c);
    p.buf_shape.push_back(b);
    return (int)p.buf_shape.size() - 1;
  };
  for (size_t li = 0; li < p.layers.size(); ++li) {
    if (!need_layer[li]) continue;
    const Layer& l = p.layers[li];
    if (l.kind == kInput) {
      const int b = new_buffer(p.shape[p.input]);
      for (int v : lout[li]) p.place[v].buf = b;
      continue;
    }
    const int v0 = lin[li][0];
    if (l.kind == kDropout || l.kind == kSplit) {
      for (int v : lout[li]) { p.place[v] = p.place[v0]; step_of[v] = step_of[v0]; }
      continue;
    }
    if (l.kind == kReLU) {
      const int s = step_of[v0];
      const bool only = readers[v0].size() == 1 && v0 != p.output;
      if (only && s >= 0 && (p.steps[s].kind == kConv || p.steps[s].kind == kIP) && p.steps[s].out == v0 && !p.steps[s].relu) {
        p.steps[s].relu = 1;
        p.steps[s].out = lout[li][0];
        p.place[lout[li][0]] = p.place[v0];
        step_of[lout[li][0]] = s;
        continue;
      }
    }
    Step st;
    st.kind = l.kind; st.layer = (int)li; st.in = lin[li]; st.out = lout[li][0];
    const bool in_place = l.kind == kReLU && l.tops[0] == l.bottoms[0];
    if (in_place) p.place[st.out] = p.place[v0];
    else p.place[st.out].buf = new_buffer(p.shape[st.out]);
    if (l.kind == kConv) st.mfma = l.stride == 1 && (l.k & 1) && l.k <= 7 && 2 * l.pad + 1 == l.k && l.group == 1;
    step_of[st.out] = (int)p.steps.size();
    p.steps.push_back(st);
  }
  // Concat bottoms their producers can write in place of a copy: the offset is a multiple of 16, the Concat is the only reader of
  // every version in the bottom's buffer, and the buffer has one writing step that is no Concat
  for (auto& st : p.steps) {
    if (st.kind != kConcat) continue;
    int off = 0;
    for (int v : st.in) {
      const int c = p.shape[v].c, buf = p.place[v].buf;
      bool direct = off % 16 == 0 && p.place[v].off == 0 && buf != p.place[p.input].buf && v != p.output;
      int writers = 0;
      for (auto& o : p.steps) {
        if (p.place[o.out].buf != buf) continue;
        ++writers;
        if (o.kind == kConcat) direct = false;
      }
      // readers of the buffer's versions: this Concat, or layers that only alias the buffer (Dropout, Split, a fused ReLU)
      for (size_t u = 0; u < nv && direct; ++u)
        if (need_v[u] && p.place[u].buf == buf)
          for (int r : readers[u]) {
            bool has_step = false;
            for (auto& o : p.steps) has_step = has_step || o.layer == r;
            const bool alias_only = !has_step && p.place[lout[r][0]].buf == buf;
            if (r != st.layer && !alias_only) direct = false;
          }
      if (direct && writers == 1) {
        for (size_t u = 0; u < nv; ++u)
          if (p.place[u].buf == buf) { p.place[u].buf = p.place[st.out].buf; p.place[u].off = off; }
      }
      off += c;
    }
  }
  p.in_shape = p.shape[p.input];
  p.out_shape = p.shape[p.output];
  return true;
} catch (const std::exception& e) {
  *err = "cannot plan " + prototxt + ": " + e.what();
  return false;
}

// ---- the network on one GPU ------------------------------------------------------------------------------------------------
class Net {
 public:
  ~Net() { release(); }
  const Plan& plan() const { return plan_; }

  // Reads both files and checks the description against the weights (no GPU).  h, w 0: the description's own input size.
  bool load(const std::string& prototxt, const std::string& caffemodel, const std::string& input_blob, const std::string& output_blob, std::string* err) {
    release();
    prototxt_ = prototxt; input_blob_ = input_blob; output_blob_ = output_blob;
    weights_.clear();
    if (!caffe_files::read_caffemodel(caffemodel, &weights_, err)) return false;
    Plan p;
    return make_plan(prototxt_, &weights_, 0, 0, 0, input_blob_, output_blob_, false, &p, err);
  }

  // The plan for frames of (c, h, w); weights are packed and uploaded to the current device on first use.
  bool prepare(st_ctx* ctx, int c, int h, int w, std::string* err) {
    if (planned_ && plan_.in_shape.c == c && plan_.in_shape.h == h && plan_.in_shape.w == w) return true;
    free_buffers();
    planned_ = false;
    if (!make_plan(prototxt_, &weights_, c, h, w, input_blob_, output_blob_, true, &plan_, err)) return false;
    for (auto& st : plan_.steps)
      if ((st.kind == kConv || st.kind == kIP) && !upload(ctx, st, err)) return false;
    planned_ = true;
    return true;
  }

  // inputs: n device pointers to planar (c, h, w) float32 frames; outputs: n device pointers to planar frames of plan().out_shape
  // step_ms (measurement only; the caller has enabled ST_K_CONV timing): per step of plan().steps the milliseconds of its launches,
  // read -- with a synchronisation -- after every step
  bool forward(st_ctx* ctx, const float* const* inputs, int n, float* const* outputs, std::string* err, std::vector<double>* step_ms = nullptr) {
    if (!planned_ || n <= 0) { *err = "caffe net: not prepared"; return false; }
    if (!reserve(n, err)) return false;
    auto fail = [&](const char* what) { *err = std::string(what) + ": " + st_ctx_last_error(ctx); return false; };
    const Plan& p = plan_;
    const Shape is = p.in_shape;
    const int ics = p.buf_shape[p.place[p.input].buf].c;
    for (int i = 0; i < n; ++i)
      if (st_planar_to_nhwc_f32(ctx, inputs[i], 1, is.c, is.h, is.w, bufs_[p.place[p.input].buf] + (size_t)i * is.h * is.w * ics, ics) != ST_OK)
        return fail("st_planar_to_nhwc_f32");
    if (step_ms && st_ctx_timing_reset(ctx) != ST_OK) return fail("st_ctx_timing_reset");
    for (auto& st : p.steps) {
      const Layer& l = p.layers[st.layer];
      const Shape xs = p.shape[st.in[0]], ys = p.shape[st.out];
      const Place xp = p.place[st.in[0]], yp = p.place[st.out];
      const float* x = bufs_[xp.buf];
      float* y = bufs_[yp.buf];
      const int xcs = p.buf_shape[xp.buf].c, ycs = p.buf_shape[yp.buf].c;
      const long long ypix = (long long)n * ys.h * ys.w;
      int rc = ST_OK;
      switch (st.kind) {
        case kConv: {
          Packed& k = packed_[l.name];
          if (st.mfma) rc = st_conv2d_nhwc_f32_tiled(ctx, x, n, xs.h, xs.w, pad16(xs.c), xcs, xp.off, k.w, k.wt, k.b, l.k, l.k, l.num_output, k.cout_pad, st.relu, y, ycs, yp.off);
          else rc = st_conv2d_general_nhwc_f32(ctx, x, n, xs.h, xs.w, xs.c, xcs, xp.off, k.w, k.b, l.k, l.stride, l.pad, l.group, l.num_output, st.relu, y, ycs, yp.off);
          break;
        }
        case kIP: {
          Packed& k = packed_[l.name];
          rc = st_inner_product_f32(ctx, x, n, xs.h * xs.w * xcs, xs.h * xs.w * xcs, k.w, k.b, l.num_output, st.relu, y + yp.off, ycs);
          break;
        }
        case kReLU: rc = st_copy_channels_nhwc_f32(ctx, x, ypix, xs.c, xcs, xp.off, 1, y, ycs, yp.off); break;
        case kPool: rc = st_pool_nhwc_f32(ctx, x, n, xs.h, xs.w, xs.c, xcs, xp.off, l.ave ? ST_POOL_AVE : ST_POOL_MAX, l.k, l.stride, l.pad, l.global ? 1 : 0, y, ycs, yp.off); break;
        case kLRN: rc = st_lrn_nhwc_f32(ctx, x, ypix, xs.c, xcs, xp.off, l.local_size, l.alpha, l.beta, l.lrn_k, y, ycs, yp.off); break;
        case kSoftmax: rc = st_softmax_nhwc_f32(ctx, x, ypix, xs.c, xcs, xp.off, y, ycs, yp.off); break;
        case kConcat: {
          int off = 0;
          for (int v : st.in) {
            const Place bp = p.place[v];
            if (!(bp.buf == yp.buf && bp.off == yp.off + off))
              rc = rc != ST_OK ? rc : st_copy_channels_nhwc_f32(ctx, bufs_[bp.buf], ypix, p.shape[v].c, p.buf_shape[bp.buf].c, bp.off, 0, y, ycs, yp.off + off);
            off += p.shape[v].c;
          }
          break;
        }
        default: break;
      }
      if (rc != ST_OK) { *err = "layer " + l.name + ": " + st_ctx_last_error(ctx); return false; }
      if (step_ms) {
        int launches = 0;
        double ms = 0.0;
        if (st_ctx_timing_read(ctx, ST_K_CONV, &launches, &ms) != ST_OK || st_ctx_timing_reset(ctx) != ST_OK) return fail("st_ctx_timing_read");
        step_ms->push_back(ms);
      }
    }
    const Place op = p.place[p.output];
    const Shape os = p.out_shape;
    if (st_nhwc_to_planar_f32(ctx, bufs_[op.buf], n, os.h, os.w, os.c, p.buf_shape[op.buf].c, op.off, outputs) != ST_OK) return fail("st_nhwc_to_planar_f32");
    return true;
  }

  void release() {
    free_buffers();
    packed_.clear();
    planned_ = false;
  }

 private:
  // w: Convolution: [cout_pad][k][k][cin_pad] (MFMA) or [cout][k][k][cin / group]; InnerProduct: st_inner_product_pack_weights' order
  struct Packed : net_weights::DeviceWeights {
    long long key = -1;   // InnerProduct: the bottom geometry the weights were permuted for
  };

  bool upload(st_ctx* ctx, const Step& st, std::string* err) {
    const Layer& l = plan_.layers[st.layer];
    const Shape xs = plan_.shape[st.in[0]];
    const int xcs = plan_.buf_shape[plan_.place[st.in[0]].buf].c;
    Packed& k = packed_[l.name];
    const long long key = l.kind == kIP ? ((long long)xs.h << 40) | ((long long)xs.w << 20) | xcs : 0;
    if (k.w && k.key == key) return true;
    k.release();
    k.key = key;
    const auto& bl = weights_[l.name];
    const int co = l.num_output;
    auto oom = [&]() { *err = "out of device memory while uploading layer " + l.name; return false; };
    if (l.kind == kConv && st.mfma) {
      if (!net_weights::upload_mfma(bl[0].data(), l.bias ? bl[1].data() : nullptr, co, xs.c, l.k, pad16(xs.c), nullptr, &k)) return oom();
      const int rc = net_weights::pack_tile(ctx, l.k, &k);
      if (rc == ST_ERR_OOM) return oom();
      if (rc != ST_OK) { *err = "layer " + l.name + ": " + st_ctx_last_error(ctx); return false; }
    } else if (l.kind == kConv) {
      const int cg = xs.c / l.group, kk = l.k * l.k;
      std::vector<float> wp((size_t)co * kk * cg), bp(co, 0.f);
      for (int o = 0; o < co; ++o) {
        if (l.bias) bp[o] = bl[1][o];
        for (int c = 0; c < cg; ++c)
          for (int t = 0; t < kk; ++t) wp[((size_t)o * kk + t) * cg + c] = bl[0][((size_t)o * cg + c) * kk + t];
      }
      if (!net_weights::to_device(wp, &k.w) || !net_weights::to_device(bp, &k.b)) return oom();
    } else {
      // the bottom is flattened C, H, W in the file and H, W, padded C in the buffer
      const size_t hw = (size_t)xs.h * xs.w, kp = hw * xcs;
      std::vector<float> wp((size_t)co * kp, 0.f), bp(co, 0.f);
      for (int o = 0; o < co; ++o) {
        if (l.bias) bp[o] = bl[1][o];
        for (int c = 0; c < xs.c; ++c)
          for (size_t q = 0; q < hw; ++q) wp[(size_t)o * kp + q * xcs + c] = bl[0][((size_t)o * xs.c + c) * hw + q];
      }
      float* rowmajor = nullptr;
      const long long nb = st_inner_product_packed_bytes((int)kp, co);
      bool ok = nb > 0 && net_weights::to_device(wp, &rowmajor) && net_weights::to_device(bp, &k.b) && hipMalloc(&k.w, (size_t)nb) == hipSuccess;
      if (ok && (st_inner_product_pack_weights(ctx, rowmajor, (int)kp, co, k.w) != ST_OK || st_ctx_sync(ctx) != ST_OK)) {
        *err = "layer " + l.name + ": " + st_ctx_last_error(ctx);
        (void)hipFree(rowmajor);
        return false;
      }
      if (rowmajor) (void)hipFree(rowmajor);
      if (!ok) return oom();
    }
    return true;
  }

  bool reserve(int n, std::string* err) {
    if (n <= cap_n_ && !bufs_.empty()) return true;
    free_buffers();
    bufs_.assign(plan_.buf_shape.size(), nullptr);
    std::vector<char> used(bufs_.size(), 0);   // a buffer whose blob moved into a Concat's is not needed
    for (auto& pl : plan_.place)
      if (pl.buf >= 0) used[pl.buf] = 1;
    for (size_t i = 0; i < bufs_.size(); ++i) {
      if (!used[i]) continue;
      const Shape& s = plan_.buf_shape[i];
      const size_t bytes = (size_t)n * s.h * s.w * s.c * 4;
      // pad channels are read (against zero weights) and never written: zero once
      if (hipMalloc(&bufs_[i], bytes) != hipSuccess || hipMemset(bufs_[i], 0, bytes) != hipSuccess) {
        *err = "caffe net: out of device memory for a batch of " + std::to_string(n) + " frames";
        free_buffers();
        return false;
      }
    }
    if (hipDeviceSynchronize() != hipSuccess) { *err = "caffe net: hipDeviceSynchronize failed"; return false; }   // the layer calls run on the context's own stream
    cap_n_ = n;
    return true;
  }
  void free_buffers() {
    for (auto& b : bufs_)
      if (b) (void)hipFree(b);
    bufs_.clear();
    cap_n_ = 0;
  }

  std::string prototxt_, input_blob_, output_blob_;
  Blobs weights_;
  Plan plan_;
  bool planned_ = false;
  std::map<std::string, Packed> packed_;
  std::vector<float*> bufs_;
  int cap_n_ = 0;
};

}  // namespace caffe_net
}  // namespace scanner
