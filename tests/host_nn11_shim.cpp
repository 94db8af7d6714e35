// Host-side instantiation of the product's NN_11 header (csrc/nn11.hpp), beside host_td_target_shim.cpp: torch-layout
// weights are packed with the header's own pack routines, and the scalar forward of host_conv_ref.hpp runs over them.
// TEST ONLY: built by tests/test_nn11_host.py into a temp dir with g++; it is not a backend of the product.
#include "host_conv_ref.hpp"

using namespace tq;

// weights / biases: 12 host pointers each in torch layout (conv1..conv11, linear1); stack u8 [P][2][d][d] -> q f32 [P][3]
extern "C" int shim_nn11_forward(int d, const float* const* weights, const float* const* biases, const uint8_t* stack,
                                 int64_t P, float* q) {
    if (!size_ok(d)) return -1;
    const PackedNet net = nn11_packed(d, weights, biases);
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t p = 0; p < P; ++p) {
        std::vector<uint16_t> buf[2] = {std::vector<uint16_t>((size_t)d * d * NN11_MAX_CP), std::vector<uint16_t>((size_t)d * d * NN11_MAX_CP)};
        uint16_t* act[NN11_LAYERS + 1];
        for (int l = 0; l <= NN11_LAYERS; ++l) act[l] = buf[l & 1].data();
        forward_one<NN11_MAX_CP>(d, net, stack + p * 2 * d * d, act, q + p * NN11_OUT);
    }
    return 0;
}

// perspectives per workgroup of the conv kernels (the tile edge tests/test_gpu_nn11.py aims at)
extern "C" int shim_nn11_group(int d) { return nn11_group(d); }

// nn11_bf16 itself, element by element: what packs weights and stores stacks, activations and gradients
extern "C" void shim_nn11_bf16(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = nn11_bf16(x[i]);
}
// ... and the backward's ReLU mask over stored bf16 activations
extern "C" void shim_nn11_mask(const uint16_t* a, int64_t n, uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = nn11_mask(a[i]) ? 1 : 0;
}
