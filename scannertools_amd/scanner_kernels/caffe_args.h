// The one reader of the NetDescriptor the caffe ops' argument messages carry
// (the reference's scannertools_caffe_cpp/scannertools_caffe.proto:5-48):
//   CaffeArgs / CaffeInputArgs {net_descriptor = 1, batch_size = 2}           Caffe, CaffeInput
//   FacenetArgs / CPM2Args     {caffe_args = 1 (a CaffeArgs), ...}            Facenet, FacenetInput, CPM2
// The outer messages' own scalars (scale, threshold, templates_path) stay with their ops.  Of a sub-message that is repeated the
// last occurrence counts (proto_lite::nested).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "proto_lite.h"

namespace scanner {

struct NetDescriptorLite {
  std::string model_path, model_weights_path;                         // 1, 2
  std::vector<std::string> input_layer_names, output_layer_names;     // 3, 4
  int32_t input_width = 0, input_height = 0, pad_mod = 0;             // 5, 6, 14
  std::vector<float> mean_colors;                                     // 7, packed or not
  bool normalize = false, preserve_aspect_ratio = false, transpose = false, uses_python = false;   // 11, 12, 13, 15
};

struct CaffeArgsLite : NetDescriptorLite {
  int32_t batch_size = 0;
};

// false: mean_colors is not a whole number of floats
inline bool parse_net_descriptor(const std::vector<proto_lite::Field>& fields, NetDescriptorLite* out) {
  for (auto& f : fields) {
    if (f.wire == 2) {
      if (f.number == 1) out->model_path = f.bytes;
      if (f.number == 2) out->model_weights_path = f.bytes;
      if (f.number == 3) out->input_layer_names.push_back(f.bytes);
      if (f.number == 4) out->output_layer_names.push_back(f.bytes);
    } else if (f.wire == 0) {
      if (f.number == 5) out->input_width = (int32_t)f.value;   // a negative int32 travels as a 64-bit varint
      if (f.number == 6) out->input_height = (int32_t)f.value;
      if (f.number == 11) out->normalize = f.value != 0;
      if (f.number == 12) out->preserve_aspect_ratio = f.value != 0;
      if (f.number == 13) out->transpose = f.value != 0;
      if (f.number == 14) out->pad_mod = (int32_t)f.value;
      if (f.number == 15) out->uses_python = f.value != 0;
    }
  }
  return proto_lite::repeated_floats(fields, 7, &out->mean_colors);
}

// CaffeArgs{net_descriptor (1){...}, batch_size (2)}
inline bool read_caffe_args(const std::vector<proto_lite::Field>& fields, CaffeArgsLite* out) {
  std::vector<proto_lite::Field> net;
  for (auto& f : fields)
    if (f.number == 2 && f.wire == 0) out->batch_size = (int32_t)f.value;
  return proto_lite::nested(fields, 1, &net) && parse_net_descriptor(net, out);
}
inline bool parse_caffe_args(const uint8_t* data, size_t size, CaffeArgsLite* out) {
  std::vector<proto_lite::Field> fields;
  return proto_lite::parse(data, size, &fields) && read_caffe_args(fields, out);
}

// FacenetArgs / CPM2Args {caffe_args (1), ...} -> the CaffeArgs inside (facenet_kernel.cpp:21-31); top: the outer message's
// fields, for the op's own scalars
inline bool parse_wrapped_caffe_args(const uint8_t* data, size_t size, CaffeArgsLite* out, std::vector<proto_lite::Field>* top) {
  std::vector<proto_lite::Field> inner;
  return proto_lite::parse(data, size, top) && proto_lite::nested(*top, 1, &inner) && read_caffe_args(inner, out);
}

}  // namespace scanner
