// Facenet op for Scanner on MI355X: frames -> FacenetInput -> Facenet -> the detector's output maps.
//
// Drop-in for the reference's op (/root/reference/scannertools_caffe/scannertools_caffe_cpp/facenet_kernel.cpp:37-46):
// frame_input("facenet_input") -> frame_output("facenet_output"), protobuf_name("FacenetArgs").  It is the Caffe kernel with
// FacenetArgs.caffe_args unwrapped and the input blob reshaped to (C, shape[1], shape[2]) of the incoming frame, FacenetInput's
// W x H planes (caffe_kernel_hip.h).  Registered batched on both device types, as FacenetInput is (the reference leaves both
// unbatched).
#include "caffe_kernel_hip.h"

namespace scanner {
using FacenetKernelHIP = CaffeKernelHIPImpl<false, true>;
using FacenetKernelHIPStaged = CaffeKernelHIPImpl<true, true>;

REGISTER_OP(Facenet).frame_input("facenet_input").frame_output("facenet_output").protobuf_name("FacenetArgs");

REGISTER_KERNEL(Facenet, FacenetKernelHIPStaged).device(DeviceType::CPU).num_devices(1).batch();
REGISTER_KERNEL(Facenet, FacenetKernelHIP).device(DeviceType::GPU).num_devices(1).batch();
}
