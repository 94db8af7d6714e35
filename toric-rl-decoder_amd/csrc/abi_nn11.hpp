// The NN_11 forward's entry points of include/toricenv.h (part of toricenv.hip's translation unit), over the frame all
// network handles share (abi_forward.hpp), and what they share with the learner step's (abi_nn11_grad.hpp): the packed
// network on the device, the one launcher of k_nn11_conv and the forward over it.
#pragma once
#include "abi_forward.hpp"
#include "nn11_grad.hpp"

namespace {
// The packed network of one handle.  The padding of every image is the zeros alloc() leaves: k_nn11_pack writes it as
// zeros again, and the optimizer's re-pack (k_nn11_opt) does not touch it.
struct NN11Net {
    int loaded;
    uint16_t* wimg;                        // the eleven conv layers' bf16 fragment images, back to back
    float* bias;                           // their padded f32 biases, back to back
    float* limg;                           // linear weights f32[3][(d-2)^2][64] (bf16-rounded values)
    float* lbias;                          // f32[3]
    uint16_t* dimg;                        // the dgrad fragment images of conv2..conv11, back to back; NULL: forward only

    void alloc(DeviceBuffers& mem, int d, bool with_dgrad) {
        constexpr int L = tq::NN11_LAYERS;
        mem.zeroed(&wimg, (size_t)tq::nn11_wimg_offset(L + 1) * sizeof(uint16_t));
        mem.zeroed(&bias, (size_t)tq::nn11_bias_offset(L + 1) * sizeof(float));
        mem.zeroed(&limg, (size_t)tq::nn11_lin_elems(d) * sizeof(float));
        mem.zeroed(&lbias, 16);
        if (with_dgrad) mem.zeroed(&dimg, (size_t)tq::nn11_dimg_offset(L + 1) * sizeof(uint16_t));
    }
    // torch-layout f32 weights and biases (12 device pointers each) -> the images, on `stream`
    int load(int d, const float* const* weights, const float* const* biases, hipStream_t stream) {
        constexpr int L = tq::NN11_LAYERS;
        tq::NN11Pack p;
        if (int rc = pointer_lists(weights, biases, L + 1, p.w, p.b)) return rc;
        if (int rc = launch(tq::k_nn11_pack, dim3(64, L + 1), dim3(256), stream, p, d, wimg, bias, limg, lbias)) return rc;
        if (dimg)
            if (int rc = launch(tq::k_nn11_pack_dgrad, dim3(64, L - 1), dim3(256), stream, p, dimg)) return rc;
        loaded = 1;
        return TQ_OK;
    }
};

// One convolution over `rows` perspectives.  Every k_nn11_conv the library holds is in the list below, by (k-steps,
// n-tiles, mode): five shapes of the forward (EPI = NN11_EPI_BIAS_RELU, `aux` the padded bias) and four of the dgrad
// (NN11_EPI_MASK, `aux` the activation image whose sign masks); and conv1 once more with GATHER, whose perspectives are
// the rows `g` lists of the stack `in`.
template <int D, int EPI, typename... ROWS>
int nn11_conv(int mode, int ks, int nt, const void* in, int dtype, const uint16_t* img, const void* aux, uint16_t* out, int64_t rows,
              hipStream_t stream, ROWS... g) {
    constexpr bool GATHER = sizeof...(ROWS) != 0;
    constexpr int G = tq::NN11Geom<D>::G, THREADS = tq::NN11Geom<D>::THREADS;
    const dim3 grid((unsigned)((rows + G - 1) / G)), block(THREADS);
#define NN11_SHAPE(KS, NT, MODE)                         \
    if (ks == KS && nt == NT && mode == tq::MODE)        \
        return launch(tq::k_nn11_conv<D, KS, NT, tq::MODE, EPI, GATHER, ROWS...>, grid, block, stream, in, dtype, img, aux, out, rows, g...)
    if constexpr (GATHER) {
        NN11_SHAPE(2, 4, NN11_CIRCULAR);
    } else if constexpr (EPI == tq::NN11_EPI_BIAS_RELU) {
        NN11_SHAPE(2, 4, NN11_CIRCULAR);
        NN11_SHAPE(6, 2, NN11_VALID);
        NN11_SHAPE(8, 4, NN11_ZERO);
        NN11_SHAPE(8, 3, NN11_ZERO);
        NN11_SHAPE(6, 3, NN11_ZERO);
    } else {
        NN11_SHAPE(4, 3, NN11_FULL);
        NN11_SHAPE(8, 4, NN11_ZERO);
        NN11_SHAPE(6, 4, NN11_ZERO);
        NN11_SHAPE(6, 3, NN11_ZERO);
    }
#undef NN11_SHAPE
    return fail(TQ_E_INVALID, "nn11: no kernel for layer shape (%d k-steps, %d n-tiles, mode %d, epilogue %d)", ks, nt, mode, EPI);
}

// The forward of `rows` perspectives: conv l = 1..11 writes its bf16 image to out[l] (conv1 reads the stack, conv l
// reads out[l - 1]), the linear layer reads out[11] and writes q.  GATHER: perspective i is row g.rows[i] of the stack.
template <int D, typename... ROWS>
int nn11_forward(const NN11Net& net, const void* stack, int dtype, int64_t rows, uint16_t* const* out, float* q, hipStream_t stream,
                 ROWS... g) {
    constexpr int L = tq::NN11_LAYERS;
    constexpr bool GATHER = sizeof...(ROWS) != 0;
    if constexpr (GATHER)
        if (int rc = nn11_conv<D, tq::NN11_EPI_BIAS_RELU>(tq::nn11_mode(1), tq::nn11_ksteps(1), tq::nn11_ntiles(1), stack, dtype,
                                                          net.wimg, net.bias, out[1], rows, stream, g...)) return rc;
    for (int l = GATHER ? 2 : 1; l <= L; ++l)
        if (int rc = nn11_conv<D, tq::NN11_EPI_BIAS_RELU>(tq::nn11_mode(l), tq::nn11_ksteps(l), tq::nn11_ntiles(l),
                                                          l == 1 ? stack : out[l - 1], l == 1 ? dtype : 0,
                                                          net.wimg + tq::nn11_wimg_offset(l), net.bias + tq::nn11_bias_offset(l),
                                                          out[l], rows, stream)) return rc;
    return launch(tq::k_nn_linear<64>, dim3((unsigned)((rows + 3) / 4)), dim3(256), stream, out[L], net.limg, net.lbias, q, rows,
                  tq::nn11_out_pixels(D));
}
}  // namespace

struct tq_nn11 {                           // made by `new tq_nn11()`: every member starts as zero
    int d, device;
    int64_t max_rows;
    NN11Net net;
    uint16_t* act[2];                      // activation images of one pass, taking turns: max_rows * d^2 * 128 bf16 each
    uint16_t* out[tq::NN11_LAYERS + 1];    // out[l], l = 1..11: the one of the two that layer l writes
    int* latch;                            // device error latch of tq_nn11_forward_rows (NN11_ERR_INDEX)
    DeviceBuffers mem;
};

extern "C" {

int tq_nn11_destroy(tq_nn11* h) { return destroy_handle(h); }

int tq_nn11_create(tq_nn11** out, int d, int64_t max_rows, int device) {
    return create_handle(out, "nn11", d, device, no_check, [&] { return max_rows_check(max_rows); }, [&](tq_nn11* h) {
        h->max_rows = max_rows;
        h->net.alloc(h->mem, d, false);
        for (int i = 0; i < 2; ++i)
            h->mem.zeroed(&h->act[i], (size_t)max_rows * d * d * tq::NN11_MAX_CP * sizeof(uint16_t));
        for (int l = 1; l <= tq::NN11_LAYERS; ++l) h->out[l] = h->act[(l + 1) & 1];
        h->mem.zeroed(&h->latch, 16);
    });
}

int tq_nn11_load(tq_nn11* h, const float* const* weights, const float* const* biases, void* stream_) {
    ENTER(h, "nn11 handle");
    return h->net.load(h->d, weights, biases, stream);
}

int tq_nn11_forward(tq_nn11* h, const void* stack, int dtype, int64_t rows, float* q, void* stream_) {
    ENTER(h, "nn11 handle");
    bool done;
    if (int rc = forward_args("nn11", h->net.loaded, stack, dtype, rows, q, &done); rc || done) return rc;
    return forward_passes(h->d, h->max_rows, stack, dtype, false, rows, q, [&](auto D, const void* s, int64_t, int64_t n, float* qn) {
        return nn11_forward<D()>(h->net, s, dtype, n, h->out, qn, stream);
    });
}

int tq_nn11_forward_rows(tq_nn11* h, const void* stack, int dtype, int64_t stack_rows, const int32_t* rows, int64_t n, float* q,
                         void* stream_) {
    ENTER(h, "nn11 handle");
    bool done;
    if (int rc = forward_args("nn11", h->net.loaded, stack, dtype, n, q, &done); rc || done) return rc;
    if (stack_rows < 0) return fail(TQ_E_INVALID, "negative stack_rows");
    if (!rows) return fail(TQ_E_INVALID, "rows is NULL");
    return forward_passes(h->d, h->max_rows, stack, dtype, true, n, q, [&](auto D, const void* s, int64_t first, int64_t m, float* qm) {
        return nn11_forward<D()>(h->net, s, dtype, m, h->out, qm, stream, tq::NN11Rows{rows + first, stack_rows, h->latch});
    });
}

int tq_nn11_check(tq_nn11* h, void* stream_) {
    ENTER(h, "nn11 handle");
    int flag;
    if (int rc = read_latch(h->latch, stream, &flag)) return rc;
    if (flag & tq::NN11_ERR_INDEX) return fail(TQ_E_INDEX, "tq_nn11_forward_rows: a row index outside [0, stack_rows) was given");
    return TQ_OK;
}

}  // extern "C"
