// The learner's step through the wide nets NN_8 and NN_17 (src/Learner_mp.py:140-169): NN_11's (nn11_grad.hpp; numerics
// contract in include/toricenv.h) for a plain conv net given by slot s.  Every kernel is that
// header's: the head (nn11_head, k_nn11_head, k_nn11_dblin), the last layer's gradient and the linear layer's three
// kernels over the feature pitch 224, the wgrad kernels at eight waves and 2048 rows to a chunk (k_conv_wgrad<7 | 8, 8,
// 2048>, k_conv_wgrad1<256, 2048>), the sum over partial images (k_nn11_wreduce over a bias pitch of 256) and the dgrad
// pack's body; the dgrad itself is k_nnw_conv<..., NN11DgradMask> (nnw.hpp) over the packed image.  What is here is where
// a layer's dgrad image lies and how the wgrad's sum over records is cut.
// How a sum is cut depends on (net, layer, d, n) alone; no atomics.
#pragma once
#include "nn11_grad.hpp"
#include "nnw.hpp"

namespace tq {

// first element of layer l = 2..layers of slot s in the handle's one dgrad image (l = layers + 1: its size)
TQ_HD int64_t nnw_dimg_offset(int s, int l) {
    int64_t o = 0;
    for (int i = 2; i < l; ++i) o += conv_dimg_elems(nnw_cin(s, i), nnw_cout(s, i));
    return o;
}

// ---- how the wgrad's sum over records is cut: a function of d alone.  About 2048 rows to a workgroup, twice NN_11's:
// a partial image is up to 9 x 256 x 256 f32 = 2.25 MiB, four times NN_11's, and one is kept per chunk.
// At max_batch = 4096 and d = 21 that is 4 records to a chunk, 1024 chunks, 2.25 GiB of partial images.
constexpr int NNW_WG_WAVES = 8;                 // wavefronts of a wgrad workgroup: one per tile of 32 output channels
constexpr int NNW_WG_CHUNK_ROWS = 2048;
static_assert(32 * NNW_WG_WAVES == NNW_MAX_CP && 32 * NN11_WG_WAVES == NN11_MAX_CP, "a wgrad workgroup spans its family's widest image");
TQ_HD int nnw_wgrad_persp(int d) { return conv_wgrad_persp(NNW_WG_CHUNK_ROWS, d); }
TQ_HD int64_t nnw_wgrad_chunks(int d, int64_t n) { const int p = nnw_wgrad_persp(d); return (n + p - 1) / p; }
constexpr int64_t NNW_WPART_ELEMS = (int64_t)9 * NNW_MAX_CP * NNW_MAX_CP;          // f32 per partial image, at most
// layer l's output grid: (d-2)^2 pixels for the last conv, d^2 otherwise
TQ_HD int nnw_layer_pixels(int s, int l, int d) { return l == nnw_layers(s) ? nn11_out_pixels(d) : d * d; }

#if defined(__HIPCC__)
// one block row (blockIdx.y) per layer l = y + 2 of slot s
__global__ __launch_bounds__(256) void k_nnw_pack_dgrad(NNWPack p, int s, uint16_t* dimg) {
    const int l = (int)blockIdx.y + 2;
    conv_pack_dgrad(nnw_cin(s, l), nnw_cout(s, l), p.w[l - 1], dimg + nnw_dimg_offset(s, l));
}
#endif  // __HIPCC__

}  // namespace tq
